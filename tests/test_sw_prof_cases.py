"""The shapes fsgpu_sw_shape gives every query length, and the conditions the world of tests/sw_prof_cases.py meets for every instantiation of k_sw and
k_sw2 -- all on the CPU.  Conditions on inputs, asserted from the model's records (never from how a target was made); the model's answers are
recomputed and compared with the frozen ones, and on the sections where saturation decides ((b), (c)) the model is held to the C oracle
(helpers.o_sw, which tests/test_oracle_vs_ref.py pins to the compiled reference)."""
import ctypes as C

import numpy as np
import pytest

import helpers
import sw_model as sm
import sw_prof_cases as K
from foldseek_amd import api

FIELDS = ("score", "qEnd", "dbEnd", "word")
AAS = (True, False)


# ---- the shape of every length ----------------------------------------------------------------------------------------------------------------------
def test_shape_of_every_length():
    shapes = [None] + [api.sw_shape(L) for L in range(1, api.FSGPU_MAX_SEQ_LEN + 1)]
    assert api.FSGPU_MAX_SEQ_LEN == 65535
    assert {R for _, R in shapes[1:]} == set(K.CLASSES) == set(api.SW_R_CLASSES)
    for L in range(1, 65536):
        n, R = shapes[L]
        assert (n == 1) == (L <= 512) and n == -(-L // 512), L
        if n > 1:
            assert R == 8, L
        else:
            assert 64 * R >= L and R == K.class_of(L) and all(64 * r < L for r in K.CLASSES if r < R), L
    tops = [L for L in range(1, 512) if shapes[L][1] != shapes[L + 1][1]] + [512]
    assert tops == [64, 128, 192, 256, 384, 512] and shapes[513] == (2, 8) and shapes[1025] == (3, 8) and shapes[65535] == (128, 8)
    assert [shapes[K.BOTTOM[R]][1] for R in K.CLASSES] == list(K.CLASSES) and [shapes[64 * R][1] for R in K.CLASSES] == list(K.CLASSES)
    for bad in (0, -1, 65536):
        with pytest.raises(api.FsgpuError):
            api.sw_shape(bad)
    n = C.c_int(0)
    assert api.lib().fsgpu_sw_shape(100, None, C.byref(n)) == -1 and api.lib().fsgpu_sw_shape(100, C.byref(n), None) == -1
    assert {"fsgpu_sw_shape", "fsgpu_sw_kernel_counts"} <= set(api.exported_symbols())


# ---- the world --------------------------------------------------------------------------------------------------------------------------------------
def test_world_lengths_and_database():
    d = K.db()
    for sec in "abc":
        for aa in AAS:
            qs = [q for q in K.section(sec) if q.aa == aa]
            assert {q.L for q in qs if q.L <= 512} >= ({64 * R for R in K.CLASSES} | set(K.BOTTOM.values())) - ({1} if sec == "b" else set()), (sec, aa)
            assert {q.cls for q in qs} == set(K.CLASSES)
    assert {q.L for q in K.section("b") if q.kind == "long"} == {513, 1025}
    assert {1, 2, 63, 64, 65, 130} <= set(d.lengths.tolist()) and (d.data3di >= 32).any()
    assert (d.t3[d.tag["allX"]] == K.X).all() and (d.data3di[d.offsets[d.tag["masked"]]:][:50] >= 32).all() and (d.t3[d.tag["masked"]] < 20).all()
    assert all((q.go, q.ge) in ((10, 1), (8, 2), (3, 1)) for q in K.world())
    for aa in AAS:
        assert {(q.go, q.ge) for q in K.section("a") if q.aa == aa and q.cls == 3} == {(10, 1), (8, 2)}
        assert {(q.go, q.ge) for q in K.section("a") if q.aa == aa and q.cls == 6} == {(10, 1), (3, 1)}
    # sections (a) and (b) stay inside the range where the AA + 3Di sum cannot leave int16: what they find is not the finding of (c)
    for q in K.section("a") + K.section("b"):
        if q.aa:
            for pA, p3 in ((q.pAf, q.p3f), (q.pAr, q.p3r)):
                s = pA.astype(np.int32) + p3.astype(np.int32)
                assert s.max() <= 32767 and s.min() >= -32768, q.name
    for q in K.section("a"):
        assert max(np.abs(t).max() for t in (q.pAf, q.p3f, q.pAr, q.p3r) if t is not None) <= 255, q.name      # ordinary: matrix entry + bias


def test_frozen_answers_are_the_models():
    """the whole world again through the live model"""
    live = K.compute_all()
    froz = K.frozen()
    assert sorted(live) == sorted(froz)
    for name, (_, f, r) in live.items():
        assert f.tobytes() == froz[name][0].tobytes() and r.tobytes() == froz[name][1].tobytes(), name
    assert sum(len(v[0]) for v in froz.values()) >= 1500


def _rows_seen(qs, word):
    """{direction: rows in which a record of these queries with that word ends (score > 0)}"""
    out = {}
    for d in (0, 1):
        rows = set()
        for q in qs:
            w = K.want(q, d)
            rows |= set(w["qEnd"][(w["word"] == word) & (w["score"] > 0)].tolist())
        out[d] = rows
    return out


@pytest.mark.parametrize("aa", AAS, ids=["aa", "3di"])
@pytest.mark.parametrize("R", K.CLASSES)
def test_a_every_register_of_three_lanes_and_both_tie_rules(R, aa):
    qs = [q for q in K.section("a") if q.cls == R and q.aa == aa]
    need = {lane * R + rr for lane in K.LANES for rr in range(R)}
    for go_ge in {(q.go, q.ge) for q in qs}:
        seen = _rows_seen([q for q in qs if (q.go, q.ge) == go_ge and q.kind == "rand"], 1)
        assert need <= seen[0] and need <= seen[1], (R, aa, go_ge, sorted(need - seen[0]), sorted(need - seen[1]))
    # the class's shortest member: a record in its last row, in the partly filled last live lane
    bot = next(q for q in qs if q.name.startswith("a/rand bottom"))
    assert all(bot.L - 1 in set(K.want(bot, d)["qEnd"].tolist()) for d in (0, 1))
    # ties: some record chosen among several columns holding the maximum, some among several rows of the best column -- in both directions
    for d in (0, 1):
        ncols = nrows = 0
        for q in qs:
            if q.kind not in ("hom", "blk"):
                continue
            pA, p3 = K.tables(q, d)
            t3, tA = K.targets(q)
            sc, _, _, ncol, nrow, _ = sm.one_pass(p3.astype(np.int32), None if pA is None else pA.astype(np.int32), t3, tA if pA is not None else None, q.go, q.ge, 16, True, detail=True)
            assert (sc < 32767).all()
            ncols += int(((ncol > 1) & (sc > 0)).sum()); nrows += int(((nrow > 1) & (sc > 0)).sum())
        assert ncols >= 1 and nrows >= 1, (R, aa, d, ncols, nrows)
    assert all((K.want(q, d)["word"] == 1).all() for q in qs for d in (0, 1))


@pytest.mark.parametrize("aa", AAS, ids=["aa", "3di"])
@pytest.mark.parametrize("R", K.CLASSES)
def test_b_int32_rerun_conditions(R, aa):
    qs = [q for q in K.section("b") if q.cls == R and q.aa == aa and q.kind != "long"]
    assert all(q.L == (K.BOTTOM[R] if q.kind == "hotbot" else 64 * R) for q in qs)
    if R > 1:
        w = K.want(next(q for q in qs if q.kind == "hotbot"), 0)
        assert (w["word"] == 2).any() and (w["word"] == 1).any()
    fwd_only = rev_only = both = 0
    for q in qs:
        f, r = K.want(q, 0), K.want(q, 1)
        fwd_only += int(((f["word"] == 2) & (r["word"] == 1)).sum()); rev_only += int(((f["word"] == 1) & (r["word"] == 2)).sum())
        both += int(((f["word"] == 2) & (r["word"] == 2)).sum())
        for w in (f, r):
            assert (w["score"][w["word"] == 2] >= 32767).all() and (w["score"][w["word"] == 1] < 32767).all() and int(w["score"].max()) < 2 ** 31
        if q.kind != "exact":
            # the re-run's subset and scatter: a saturated call also holds pairs that keep their int16 record, in either direction it saturates in
            for w in (f, r):
                assert not (w["word"] == 2).any() or ((w["word"] == 1).any() and (w["word"] == 2).any()), q.name
    assert fwd_only >= 2 and rev_only >= 2 and both >= 2, (R, aa, fwd_only, rev_only, both)
    kinds = {q.kind: q for q in qs if q.kind.startswith("hot")}
    f, r = K.want(kinds["hotF"], 0), K.want(kinds["hotF"], 1)
    assert (f["word"] == 2).any() and (r["word"] == 1).all()
    f, r = K.want(kinds["hotR"], 0), K.want(kinds["hotR"], 1)
    assert (r["word"] == 2).any() and (f["word"] == 1).all()
    # hot BIASES (what int8 holds) where the class allows it: with AA tables from 192 rows on, 3Di only from 384 rows on
    from_bias = max(int(np.abs(t).max()) for t in (kinds["hotB"].p3f, kinds["hotB"].p3r)) <= 127 + 18
    assert from_bias == (R >= (3 if aa else 6)), (R, aa)
    # class 1: no int8 material saturates 64 rows
    assert 64 * 508 < 32767 < 65 * 508
    ex = next(q for q in qs if q.kind == "exact")
    for d in (0, 1):
        k = list(ex.ids).index(K.db().tag["hom/63"])
        assert tuple(K.want(ex, d)[k]) == (32767, 62, 62, 2)
        pA, p3 = K.tables(ex, d)
        cells = p3[5, :63].astype(np.int64) + (0 if pA is None else pA[9, :63].astype(np.int64))
        assert cells.sum() == 32767 and (np.cumsum(cells)[:-1] < 32767).all()                # reached in the last cell, nothing clipped before
    # every register of lanes 0, 31, 63 ends an int32 record, in both directions
    need = {lane * R + rr for lane in K.LANES for rr in range(R)}
    seen = _rows_seen([q for q in qs if q.kind == "dom"], 2)
    assert need <= seen[0] and need <= seen[1], (R, aa, sorted(need - seen[0]), sorted(need - seen[1]))
    # rows tie in the int32 end cell: a homopolymer at 600 a cell against a shorter homopolymer
    hh = next(q for q in qs if q.kind == "homhot")
    pA, p3 = K.tables(hh, 0)
    t3, tA = K.targets(hh)
    sat = np.flatnonzero(K.want(hh, 0)["word"] == 2)
    assert len(sat)
    sc, qe, _, _, nrow, _ = sm.one_pass(p3.astype(np.int32), None if pA is None else pA.astype(np.int32), [t3[k] for k in sat], [tA[k] for k in sat] if pA is not None else None,
                                        10, 1, 8, False, detail=True)
    assert (nrow > 1).any() and (sc == K.want(hh, 0)["score"][sat]).all()
    if R > 1:                                          # ... among rows of ONE lane: the first of a lane's registers must win, not the last
        assert any(n > 1 and int(q_) % R != R - 1 for n, q_ in zip(nrow, qe)), (R, qe, nrow)


@pytest.mark.parametrize("aa", AAS, ids=["aa", "3di"])
def test_b_row_tiles_saturate(aa):
    for L in K.LONG:
        q = next(q for q in K.section("b") if q.kind == "long" and q.L == L and q.aa == aa)
        for d in (0, 1):
            w = K.want(q, d)
            assert (w["word"] == 2).sum() >= 3 and (w["word"] == 1).sum() >= 2 and int(w["score"].max()) < 2 ** 31
            assert (w["qEnd"][w["word"] == 2] >= 0).all()


@pytest.mark.parametrize("R", K.CLASSES)
def test_c_int16_range_conditions_and_decisiveness(R):
    differ = 0
    for q in [q for q in K.section("c") if q.cls == R and q.aa]:
        for d in (0, 1):
            pA, p3 = (t.astype(np.int32) for t in K.tables(q, d))
            s = pA + p3
            assert s.max() == 65534 and (s[0] == 40000).any()                                   # (i)
            assert s.min() == -65536 and (s[1] == -40000).all()                                 # (ii)
            legal = (s >= -32768) & (s <= 32767)
            if q.L > 1:
                assert (s[4] == 20000).sum() == 2 and legal[4].all() and legal[8].all() and (s[8] == 767).sum() == 1      # (iii): two legal sums on a diagonal
            assert max(int(np.abs(pA).max()), int(np.abs(p3).max())) == 32768
            live, wrap = K.want(q, d), K.wrapped(q, d)
            differ += int(sum(live[k].tobytes() != wrap[k].tobytes() for k in range(len(live))))
            k = list(q.ids).index(K.db().tag["c/iii"])
            if q.L > 1:
                assert tuple(live[k])[0] == 40000 and live[k]["word"] == 2 and wrap[k].tobytes() == live[k].tobytes()
            k = list(q.ids).index(K.db().tag["c/i"])
            assert tuple(live[k])[0] in (40000, 65534) and live[k]["word"] == 2 and wrap[k]["score"] < 32767
            k = list(q.ids).index(K.db().tag["c/ii alone"])
            assert tuple(live[k]) == (0, 0, 0, 1) and tuple(wrap[k]) == ((0, 0, 0, 2) if q.L > 1 else (25536, 0, 0, 1))      # two wrapped cells saturate: re-run, and the int32 pass finds nothing
            k = list(q.ids).index(K.db().tag["c/ii"])
            assert 0 < live[k]["score"] < 1000 and 25000 < wrap[k]["score"] < 32767
    assert differ >= 4, (R, differ)
    for q in [q for q in K.section("c") if q.cls == R and not q.aa]:                            # (iv): nothing to sum, H + s saturates
        for d in (0, 1):
            p3 = K.tables(q, d)[1].astype(np.int32)
            assert p3.max() == 20000 and p3.min() == -32768
            w = K.want(q, d)
            k = list(q.ids).index(K.db().tag["c/iii"])
            if q.L > 1:
                assert w[k]["score"] == 40000 and w[k]["word"] == 2
            k = list(q.ids).index(K.db().tag["c/i max"])
            assert w[k]["score"] == 20000 and w[k]["word"] == 1


@pytest.mark.parametrize("sec", ["b", "c"])
def test_model_against_the_c_oracle(sec):
    """every pair of the sections whose records saturation decides, both directions"""
    n = 0
    for q in K.section(sec):
        t3, tA = K.targets(q)
        for d in (0, 1):
            pA, p3 = K.tables(q, d)
            zero = np.zeros_like(p3)
            w = K.want(q, d)
            for k in range(len(t3)):
                o = helpers.o_sw(zero if pA is None else pA, p3, q.L, tA[k], t3[k], q.go, q.ge)
                assert tuple(int(o[f]) for f in FIELDS) == tuple(int(w[k][f]) for f in FIELDS), (q.name, d, k, len(t3[k]), o, w[k])
                n += 1
    assert n >= 400

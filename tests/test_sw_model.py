"""tests/sw_model.py held to what already stands (no GPU): (a) the frozen reference records of tests/golden/hotpath_v1.npz, (b) the C oracle's literal
emulation of the striped kernel, both passes, (c) the compiled reference where oracle/_ref is built, (d) a cell-by-cell textbook Gotoh for the model
with the segment quirk switched off, (e) counts of what the inputs of (b) reached, (f) the frozen answers of tests/golden/sw_v1 against the live model."""
import os

import numpy as np
import pytest

import helpers
import oracle_lib
import sw_cases as K
import sw_model as sm
from foldseek_amd import api, synth
from oracle_lib import SW_DT

GAP_COSTS = ((10, 1), (8, 2), (3, 1), (2, 1), (15, 3))
MUST_L = (1, 15, 16, 17, 127, 128, 129)


def _tiny(m):
    return np.ascontiguousarray(np.array(m.scores()).reshape(21, 21).astype(np.int8))


def _rec(r):
    return int(r["score"]), int(r["qEnd"]), int(r["dbEnd"]), int(r["word"])


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("atype", [2, 0])
def test_model_equals_the_frozen_reference_records(atype):
    G = np.load(os.path.join(K.HERE, "golden", "hotpath_v1.npz"))
    o = np.concatenate([[0], np.cumsum(G["q_lens"])])
    db = synth.PaddedDB(np.ascontiguousarray(G["db_data3di"]), np.ascontiguousarray(G["db_dataaa"]), G["db_offsets"], G["db_lengths"])
    mA, m3 = api.Matrix(1, 1.4 if atype == 2 else 0.0), api.Matrix(0, 2.1)
    tA, t3 = _tiny(mA), _tiny(m3)
    ids = list(range(db.n))
    targets = [K.target(db, i) for i in ids]
    for qi in range(len(G["q_lens"])):
        q3, qa = np.ascontiguousarray(G["q3"][o[qi]:o[qi + 1]]), np.ascontiguousarray(G["qa"][o[qi]:o[qi + 1]])
        for rev, key in ((False, "sw_fwd"), (True, "sw_rev")):
            # the reversed query's biases are those of the reversed sequence, indexed by the reversed position
            s3, sa = (q3[::-1].copy(), qa[::-1].copy()) if rev else (q3, qa)
            _, _, cbA, cb3 = api.align_profiles(mA, m3, sa, s3, True, 0.5)
            got = sm.align(t3, tA, q3, qa, cb3, cbA, rev, [t[0] for t in targets], [t[1] for t in targets])
            ref = G[f"{key}_t{atype}"][qi][ids]
            for k in range(len(ids)):
                assert _rec(got[k]) == _rec(ref[k]), (atype, qi, rev, ids[k])


# ---- (b), (e) ----------------------------------------------------------------------------------------------------------------------------------------
def _seq(rng, n, letters, style):
    """random / tandem repeat / homopolymer over an alphabet of `letters` letters, a few X"""
    if style == 0:
        s = rng.integers(0, letters, n)
    elif style == 1:
        s = np.resize(rng.integers(0, letters, int(rng.integers(2, 8))), n)
    else:
        s = np.full(n, rng.integers(0, letters))
    s = s.astype(np.uint8)
    if n > 6 and rng.random() < 0.3:
        s[rng.integers(0, n, 2)] = 20
    return s


def _oracle_cases():
    """260 queries x 4 targets = 1040 seeded cases: (L, go, ge, prof3, profA, [(t3, tA)])"""
    rng = np.random.default_rng(20261018)
    real3, realA = K.matrices()
    lens = list(MUST_L) * 4 + [int(x) for x in rng.integers(1, 301, 260 - 4 * len(MUST_L))]
    for n, L in enumerate(lens):
        go, ge = GAP_COSTS[n % 5]
        letters = (1, 2, 4, 20)[(n // 5) % 4]
        style = int(rng.integers(0, 3))
        q3, qa = _seq(rng, L, letters, style), _seq(rng, L, letters, style)
        if n % 3 == 0:
            m3, mA = real3, realA
        else:
            m3, mA = rng.integers(-7, 10, (21, 21)).astype(np.int8), rng.integers(-5, 8, (21, 21)).astype(np.int8)
            m3[20] = m3[:, 20] = 0; mA[20] = mA[:, 20] = -1
        if n % 6 == 5:
            m3 = m3.copy(); m3[np.arange(20), np.arange(20)] = 12          # strong diagonals: long gapped alignments
        big = n % 11
        cb3 = np.full(L, 100 if big == 0 else -100 if big == 1 else 0, np.int8) if big < 2 else rng.integers(-3, 4, L).astype(np.int8)
        cbA = np.full(L, 100 if big == 0 else 0, np.int8) if big < 2 else rng.integers(-3, 4, L).astype(np.int8)
        p3, pA = sm.profile(m3, q3, cb3, n % 2 == 1), sm.profile(mA, qa, cbA, n % 2 == 1)
        targets = []
        for k in range(4):
            T = int(rng.integers(1, 301)) if k else int(rng.choice(MUST_L + (L,)))
            if big == 0 and k >= 2:
                T = 300                                                          # +100 on every position: long enough to pass 32767
            if k == 1:                                                           # the query itself, shifted and cut: a shifted repeat
                sh = int(rng.integers(0, max(1, L // 2)))
                t3, ta = np.resize(np.roll(q3, sh), T), np.resize(np.roll(qa, sh), T)
                if T > 20:
                    cut = int(rng.integers(1, T - 8))
                    t3, ta = np.delete(t3, slice(cut, cut + 6)), np.delete(ta, slice(cut, cut + 6))
            else:
                t3, ta = _seq(rng, T, letters, int(rng.integers(0, 3))), _seq(rng, T, letters, int(rng.integers(0, 3)))
            targets.append((np.ascontiguousarray(t3, np.uint8), np.ascontiguousarray(ta, np.uint8)))
        yield L, go, ge, p3, pA, targets


# what the 1040 cases reached when this was written: 803 / 444 / 169 / 29 / 111; the floors are half of that
FLOORS = {"E fed from an H below the cell's": 400, "maximum again in a later column": 220, "maximum in another row of the best column": 85, "word 2": 15, "score 0": 55}


def test_model_equals_the_oracle_on_1040_cases_and_the_cases_reach_the_hard_parts():
    O = helpers.oracle()
    reach = dict.fromkeys(FLOORS, 0)
    n, seen_L = 0, set()
    for L, go, ge, p3, pA, targets in _oracle_cases():
        seen_L.add(L)
        t3, tA = [t[0] for t in targets], [t[1] for t in targets]
        got = sm.align_profiles(p3, pA, t3, tA, go, ge)
        wide = sm.one_pass(p3, pA, t3, tA, go, ge, 8, False)
        first = sm.one_pass(p3, pA, t3, tA, go, ge, 16, True, detail=True)
        plain = sm.one_pass(p3, pA, t3, tA, go, ge, 1, True)
        p3c, pAc = np.ascontiguousarray(p3, np.int16).ravel(), np.ascontiguousarray(pA, np.int16).ravel()
        for k in range(len(targets)):
            res = np.zeros(1, SW_DT)
            O.fso_sw_score_endpos(pAc, p3c, L, tA[k], t3[k], len(t3[k]), go, ge, res.ctypes.data)
            assert _rec(got[k]) == _rec(res[0]), ("alignScoreEndPos", n, L, len(t3[k]), go, ge, got[k], res[0])
            O.fso_sw_pass(pAc, p3c, L, tA[k], t3[k], len(t3[k]), go, ge, 8, 0, res.ctypes.data)
            assert (int(wide[0][k]), int(wide[1][k]), int(wide[2][k])) == _rec(res[0])[:3], ("int32 pass", n, L, len(t3[k]), go, ge)
            n += 1
        # the segment quirk: cases in which a vertical gap across a segment border set an H that E did not see.  It changes E alone: with
        # gapOpen > gapExtend no record depends on it (sw_model.py), so "the quirk changes the score" is counted, and has to stay at zero
        reach["E fed from an H below the cell's"] += int((first[5] > 0).sum())
        assert all((first[k] == plain[k]).all() for k in range(3)), ("one segment per column gives another record", n, L, go, ge)
        reach["maximum again in a later column"] += int((first[3] > 1).sum())
        reach["maximum in another row of the best column"] += int((first[4] > 1).sum())
        reach["word 2"] += int((got["word"] == 2).sum())
        reach["score 0"] += int((got["score"] == 0).sum())
    print(n, "cases;", reach)
    assert n >= 1000 and set(MUST_L) <= seen_L
    for what, floor in FLOORS.items():
        assert reach[what] >= floor, (what, reach)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("atype", [2, 0])
def test_model_equals_the_compiled_reference(atype):
    R = oracle_lib.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    from oracle_lib import REFSW_DT
    q3s, qas = synth.make_queries(3, seed=15)
    db = synth.make_db(150, (q3s, qas), seed=17, homologs_per_query=30)
    t3 = np.where(db.data3di >= 32, db.data3di - 32, db.data3di).astype(np.uint8)
    mA, m3 = api.Matrix(1, 1.4 if atype == 2 else 0.0), api.Matrix(0, 2.1)
    targets = [K.target(db, i) for i in range(db.n)]
    for qi in range(3):
        q3, qa = q3s[qi], qas[qi]
        fw, rv = np.zeros(db.n, REFSW_DT), np.zeros(db.n, REFSW_DT)
        R.ref_structure_align(qa, q3, len(q3), atype, 1, 0.5, 10, 1, db.dataaa, t3, db.offsets[:-1].copy(), db.lengths, db.n,
                              db.residues, 10.0, 0, 1, fw.ctypes.data, rv.ctypes.data, None, None, 0)
        for rev, ref in ((False, fw), (True, rv)):
            s3, sa = (q3[::-1].copy(), qa[::-1].copy()) if rev else (q3, qa)
            _, _, cbA, cb3 = api.align_profiles(mA, m3, sa, s3, True, 0.5)
            got = sm.align(_tiny(m3), _tiny(mA), q3, qa, cb3, cbA, rev, [t[0] for t in targets], [t[1] for t in targets])
            for k in range(db.n):
                assert _rec(got[k]) == _rec(ref[k]), (atype, qi, rev, k)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------
def _gotoh(p3, pA, t3, tA, go, ge):
    """textbook local alignment with affine gaps, cell by cell: gap(k) = go + (k - 1) ge; the end cell by the reference's rule"""
    L, T = p3.shape[1], len(t3)
    H = [[0] * (T + 1) for _ in range(L + 1)]
    E = [[0] * (T + 1) for _ in range(L + 1)]
    F = [[0] * (T + 1) for _ in range(L + 1)]
    best = (0, 0, 0)
    for c in range(1, T + 1):
        col_best, col_row = 0, 0
        for r in range(1, L + 1):
            E[r][c] = max(E[r][c - 1] - ge, H[r][c - 1] - go, 0)
            F[r][c] = max(F[r - 1][c] - ge, H[r - 1][c] - go, 0)
            s = int(p3[t3[c - 1]][r - 1]) + int(pA[tA[c - 1]][r - 1])
            H[r][c] = max(0, H[r - 1][c - 1] + s, E[r][c], F[r][c])
            if H[r][c] > col_best:
                col_best, col_row = H[r][c], r - 1
        if col_best > best[0]:
            best = (col_best, col_row, c - 1)
    return best


def test_model_without_the_segment_quirk_is_textbook_gotoh():
    rng = np.random.default_rng(7)
    real3, realA = K.matrices()
    differs = 0
    for n in range(160):
        L, T = int(rng.integers(1, 49)), int(rng.integers(1, 49))
        go, ge = GAP_COSTS[n % 5]
        letters = (2, 4, 20)[n % 3]
        q3, qa = _seq(rng, L, letters, n % 2), _seq(rng, L, letters, n % 2)
        t3, ta = (np.resize(np.roll(q3, 3), T), np.resize(np.roll(qa, 3), T)) if n % 4 == 0 else (_seq(rng, T, letters, 0), _seq(rng, T, letters, 0))
        p3, pA = sm.profile(real3, q3, rng.integers(-3, 4, L).astype(np.int8), n % 2 == 1), sm.profile(realA, qa, None, n % 2 == 1)
        want = _gotoh(p3, pA, t3, ta, go, ge)
        for sat in (False, True):
            got = sm.one_pass(p3, pA, [t3], [ta], go, ge, 1, sat)
            assert (int(got[0][0]), int(got[1][0]), int(got[2][0])) == want, (n, L, T, go, ge, sat)
        quirk = sm.one_pass(p3, pA, [t3], [ta], go, ge, 16, True, detail=True)
        assert (int(quirk[0][0]), int(quirk[1][0]), int(quirk[2][0])) == want            # gapOpen > gapExtend: the quirk stays inside E (sw_model.py)
        differs += int(quirk[5][0] > 0)
    assert differs >= 20, differs           # ... although it was at work in these inputs


# ---- (f) the frozen answers of tests/golden/sw_v1 ----------------------------------------------------------------------------------------------------
def _logged_lookups(calls):
    K.LOG = []
    try:
        for call in calls:
            for d in call.dirs:
                K.call_want(call, d)
        return K.LOG
    finally:
        K.LOG = None


def _live_equals_frozen(entries):
    """entries of K.LOG, grouped by query so that the model runs once per (query, direction)"""
    groups = {}
    for e in entries:
        d, m3, mA, q, rev, go, ge, t3, tA = e
        groups.setdefault((id(m3), id(mA), id(q), rev, go, ge), []).append(e)
    for es in groups.values():
        d, m3, mA, q, rev, go, ge = es[0][:7]
        got = K.live(m3, mA, q, rev, [(e[7], e[8]) for e in es], go, ge)
        for e, g in zip(es, got):
            assert _rec(g) == tuple(int(v) for v in K.store()[e[0]]), (len(q.q3), rev, go, ge, len(e[7]))
    return len(entries)


def test_every_ninth_frozen_answer_is_the_live_models():
    log = _logged_lookups(K.all_calls())
    uniq = list({e[0]: e for e in log}.values())
    assert len({e[0] for e in log}) + 4 == len(K.store()), "answers.npz holds pairs no call asks for (or misses some): regenerate it"
    assert _live_equals_frozen(uniq[::9]) >= 500


def test_sections_c_to_f_frozen_answers_are_the_live_models():
    log = _logged_lookups(K.live_sections())
    uniq = list({e[0]: e for e in log}.values())
    _live_equals_frozen(uniq)
    m3, mA, q, t3, tA = K.exact_32767()
    for rev in (False, True):
        got = K.live(m3, mA, q, rev, [(t3, tA)])
        assert _rec(got[0]) == (32767, 216, 216, 2) == _rec(K.want(m3, mA, q, rev, [(t3, tA)])[0])
        # the first pass reaches INT16_MAX without clipping an addition: the unsaturated pass gives the same number
        assert int(sm.one_pass(sm.profile(m3, q.q3, q.cb3f, rev), sm.profile(mA, q.qa, q.cbAf, rev), [t3], [tA], 10, 1, 16, False)[0][0]) == 32767


def test_cases_hold_what_the_sections_promise():
    """the database and the lists, checked where they are built: every length, the three kinds, the odd targets, relatives that score"""
    db = K.main_db()
    assert sorted(db.lengths.tolist()) == sorted(K.LENGTHS * 3 + [40, 50]) and 100 <= db.n <= 125
    assert {"random", "derived", "low", "allX", "masked"} == set(db.kind)
    assert (db.data3di[db.offsets[db.kind.index("masked")]:][:50] >= 32).all()
    for name, (HL, Rs) in K.A_CLASSES.items():
        qs = K.class_queries()[name]
        assert {(len(q.q3) + HL - 1) // HL for q in qs} == Rs
        for dw4 in range(4):                  # both ends of a class for every image layout
            ends = {len(q.q3) % HL == 0 for q in qs if ((len(q.q3) + HL - 1) // HL + 1) // 2 % 4 == dw4}
            assert ends == {True, False}, (name, dw4)
    K.LOG = None
    high = sum(int((w["score"] > 150).sum()) for c in K.section_a() for w in K.call_want(c, 0))
    assert high >= 60, high                   # gapped relatives among the pairs

"""fsgpu_diag_rescore (k_diag_rescore) called directly through Context.diag_rescore against the independent model (tests/diag_model.py, itself held to the
reference binary's output by tests/test_diag_model.py): all eight fields of every record, exactly.  Pairs with status UNDEFINED (the reference's reverse pass
reads past the query there) are compared in everything but revScore.  Which statuses, boundaries and tie situations a test covers is asserted from the
model's own output, not assumed."""
import ctypes as C

import numpy as np
import pytest

import diag_model as M
import helpers
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu


def _db(targets, mask3=()):
    """_manual_db-style resident DB (ascending length, entries padded with code 20 to a multiple of 4) of (AA, 3Di) code arrays; the 3Di residues of the
    targets named in mask3 are all soft-masked (+32).  Returns (PaddedDB, targets in DB order: what the model sees)."""
    lens = np.array([len(t[1]) for t in targets], np.int32)
    order = np.argsort(lens, kind="stable")
    lens = lens[order]
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens + 3) // 4 * 4)
    d3 = np.full(offsets[-1], 20, np.uint8)
    da = np.full(offsets[-1], 20, np.uint8)
    for new, old in enumerate(order):
        d3[offsets[new]:offsets[new] + lens[new]] = targets[old][1] + (32 if old in mask3 else 0)
        da[offsets[new]:offsets[new] + lens[new]] = targets[old][0]
    return synth.PaddedDB(d3, da, offsets, lens), [targets[old] for old in order]


def _ctx(db):
    c = api.Context(0)
    c.load_db(db)
    return c


def _real(aa_factor):
    m3 = helpers.o_submat("MAT3DI", 2.1)[0].reshape(21, 21).copy()
    mA = helpers.o_submat("BLOSUM62", aa_factor)[0].reshape(21, 21).copy()
    return m3, mA


def _model(queries, targets, pairs, m3, mA):
    l3, lA = np.asarray(m3).tolist(), np.asarray(mA).tolist()
    return [M.rescore_pair(queries, targets, p, l3, lA) for p in pairs]


def _check(got, want, pairs, what=""):
    assert len(got) == len(want) == len(pairs)
    for k, (g, w) in enumerate(zip(got, want)):
        skip = ("revScore",) if w["status"] == M.UNDEFINED else ()
        bad = [f for f in M.FIELDS if f not in skip and int(g[f]) != w[f]]
        assert not bad, f"{what} pair {k} (query, target, diagonal) = {tuple(int(x) for x in pairs[k])}: fields {bad}\ngot  {dict(zip(M.FIELDS, g.tolist()))}\nwant {w}"


def _run(ctx, queries, targets, pairs, m3, mA, what=""):
    got = ctx.diag_rescore([q[0] for q in queries], [q[1] for q in queries], m3, mA, pairs)
    want = _model(queries, targets, pairs, m3, mA)
    _check(got, want, pairs, what)
    return want


def _rand(rng, L, letters=20):
    return rng.integers(0, letters, size=L).astype(np.uint8), rng.integers(0, letters, size=L).astype(np.uint8)


def test_every_diagonal_of_small_sequences():
    """EVERY diagonal in [-(Lt + 2), Lq + 2] of 7 queries x 8 targets in one call: length-1 sequences, dist == Lq - 1 / Lq / Lt - 1 / Lt, dist + len == Lq
    against Lq + 1, an all-X target, a soft-masked target, X in the queries, a pair count that is no multiple of the 256-lane block; both alignment types"""
    rng = np.random.default_rng(20251101)
    queries = [_rand(rng, L) for L in (1, 2, 3, 7, 16, 33, 64)]
    for qa, q3 in queries[3:]:
        qa[rng.integers(0, len(qa))] = 20
        q3[rng.integers(0, len(q3), size=2)] = 20
    targets = [_rand(rng, L) for L in (1, 2, 5, 16, 40, 65)]
    targets.append((np.full(9, 20, np.uint8), np.full(9, 20, np.uint8)))          # all X
    targets.append(_rand(rng, 12))                                                # all 3Di residues soft-masked in the DB
    # relatives, so that runs longer than a residue or two occur: target 3 (16) and 4 (40) carry pieces of queries 4 (16) and 6 (64)
    targets[3][0][:], targets[3][1][:] = queries[4][0], queries[4][1]
    targets[3][1][5] = (targets[3][1][5] + 1) % 20
    targets[4][0][:], targets[4][1][:] = queries[6][0][10:50], queries[6][1][10:50]
    db, targets = _db(targets, mask3={7})
    assert (db.data3di >= 32).sum() == 12
    pairs = [(q, t, d) for q in range(len(queries)) for t in range(len(targets))
             for d in range(-(len(targets[t][1]) + 2), len(queries[q][1]) + 3)]
    assert len(pairs) > 2000 and len(pairs) % 256 != 0
    ctx = _ctx(db)
    for aa_factor in (1.4, 0.0):
        m3, mA = _real(aa_factor)
        want = _run(ctx, queries, targets, pairs, m3, mA, f"AA x {aa_factor}")
        st = np.array([w["status"] for w in want])
        assert min((st == M.OK).sum(), (st == M.NO_OVERLAP).sum(), (st == M.UNDEFINED).sum()) >= 100, np.bincount(st)
        assert sum(1 for w, p in zip(want, pairs) if w["status"] == M.OK and p[2] < 0) >= 100
        # both sides of every boundary, from the model's own records
        by = {p: w for p, w in zip(pairs, want)}
        for q in range(len(queries)):
            for t in range(len(targets)):
                Lq, Lt = len(queries[q][1]), len(targets[t][1])
                assert by[(q, t, Lq - 1)]["status"] == M.OK and by[(q, t, Lq - 1)]["diagonalLen"] == 1
                assert by[(q, t, Lq)]["status"] == M.NO_OVERLAP and by[(q, t, -Lt)]["status"] == M.NO_OVERLAP
                assert by[(q, t, -(Lt - 1))]["status"] in ((M.OK, M.UNDEFINED) if Lt > 1 else (M.OK,))
                assert by[(q, t, -(Lt - 1))]["diagonalLen"] == 1
                if Lt > 1:
                    assert by[(q, t, -1)]["status"] == (M.OK if Lt <= Lq else M.UNDEFINED)      # dist + len == Lq when Lt == Lq, Lq + 1 when Lt == Lq + 1
        assert any(len(queries[q][1]) == len(targets[t][1]) > 1 for q in range(len(queries)) for t in range(len(targets)))
        assert any(len(queries[q][1]) + 1 == len(targets[t][1]) for q in range(len(queries)) for t in range(len(targets)))
        assert max(w["endPos"] - w["startPos"] for w in want) >= 15 and max(w["identicalAA"] for w in want) >= 15
    ctx.close()


def test_tie_rules_with_crafted_matrices():
    """a +1 / -1 3Di matrix with a zero AA matrix on sequences over three letters: the running sum returns to exactly 0 (reset on <= 0) and equal maxima
    repeat (a new maximum only on >, so start and end are those of the FIRST); then entries of +-30 000 on 3 000 residues: sums far beyond int16"""
    rng = np.random.default_rng(7)
    m3 = np.where(np.eye(21, dtype=bool), 1, -1).astype(np.int16)
    mA = np.zeros((21, 21), np.int16)
    queries = [_rand(rng, L, 3) for L in (200, 200, 180, 150, 120, 90, 60, 37)]
    targets = [_rand(rng, L, 3) for L in (200, 170, 140, 100, 80, 50, 33, 200)]
    big_q = _rand(rng, 3000)
    big_t = (np.where(rng.random(3000) < 0.3, rng.integers(0, 20, 3000), big_q[0]).astype(np.uint8),
             np.where(rng.random(3000) < 0.3, rng.integers(0, 20, 3000), big_q[1]).astype(np.uint8))
    db, targets = _db(targets + [big_t])
    big = len(targets) - 1
    assert len(targets[big][1]) == 3000
    ctx = _ctx(db)
    pairs = []
    for q in range(len(queries)):
        for t in range(big):
            Lq, Lt = len(queries[q][1]), len(targets[t][1])
            ds = set(rng.integers(-(Lt // 2), Lq // 2 + 1, size=8).tolist()) | {0}
            pairs += [(q, t, d) for d in sorted(ds)]
    want = _run(ctx, queries, targets, pairs, m3, mA, "+-1")
    ok = [(p, w) for p, w in zip(pairs, want) if w["status"] == M.OK]
    assert len(ok) >= 200
    l3, lA = m3.tolist(), mA.tolist()
    zero = again = 0
    for (q, t, d), w in ok:
        z, times, first = M.forward_events(queries[q][0].tolist(), queries[q][1].tolist(), targets[t][0].tolist(), targets[t][1].tolist(), d, l3, lA)
        zero += z
        again += times > 1
        assert w["endPos"] == (first if times else 0) and w["startPos"] <= w["endPos"]      # the FIRST of the equal maxima
    assert 2 * zero >= len(ok) and 4 * again >= len(ok), (zero, again, len(ok))
    # int32 accumulation
    m3 = np.where(np.eye(21, dtype=bool), 30000, -30000).astype(np.int16)
    mA = np.where(np.eye(21, dtype=bool), 30000, -30000).astype(np.int16)
    pairs = [(0, big, d) for d in (0, 1, -1, 0)]
    want = _run(ctx, [big_q], targets, pairs, m3, mA, "+-30000")
    assert all(w["status"] == M.OK for w in want) and want[0]["score"] > 40_000_000 and want[0]["endPos"] - want[0]["startPos"] > 2000
    assert min(min(w["score"], w["revScore"]) for w in want) > 32767
    ctx.close()


def test_call_shapes():
    """n = 1, 255, 256, 257 and 0; a 3 000 x 3 000 pair on its main, first and last diagonals; diagonals +-32 767; 300 queries in one call, their data
    unpadded and back to back"""
    rng = np.random.default_rng(11)
    long_q = _rand(rng, 3000)
    targets = [_rand(rng, L) for L in (1, 6, 31, 77)] + [(long_q[0].copy(), long_q[1].copy())]
    targets[4][1][::7] = rng.integers(0, 20, size=len(targets[4][1][::7]))
    db, targets = _db(targets)
    ctx = _ctx(db)
    m3, mA = _real(1.4)
    queries = [long_q, _rand(rng, 77), _rand(rng, 5)]
    pool = [(q, t, int(d)) for q in (1, 2) for t in range(4) for d in rng.integers(-80, 80, size=40)]
    for n in (1, 255, 256, 257):
        _run(ctx, queries, targets, pool[:n], m3, mA, f"n = {n}")
    # n = 0: success, nothing written
    qa, q3 = np.ascontiguousarray(queries[2][0]), np.ascontiguousarray(queries[2][1])
    off, ln = np.array([0, 5], np.uint64), np.array([5], np.int32)
    out = np.full(4, -7, np.int32).view(np.int32)
    m3c, mAc = np.ascontiguousarray(m3, np.int16), np.ascontiguousarray(mA, np.int16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert api.lib().fsgpu_diag_rescore(ctx.h, vp(qa), vp(q3), vp(off), vp(ln), 1, vp(m3c), vp(mAc), None, 0, vp(out)) == 0
    assert api.lib().fsgpu_diag_rescore(ctx.h, vp(qa), vp(q3), vp(off), vp(ln), 1, vp(m3c), vp(mAc), None, 0, None) == 0
    assert (out == -7).all()
    assert len(ctx.diag_rescore([queries[2][0]], [queries[2][1]], m3, mA, [])) == 0
    # the long pair and the ends of the int16 diagonal range
    pairs = [(0, 4, d) for d in (0, 1, -1, 2999, -2999, 3000, -3000, 32767, -32767)] + [(1, 3, 32767), (2, 0, -32767), (1, 4, -2923), (1, 4, -2924)]
    want = _run(ctx, queries, targets, pairs, m3, mA, "3000 x 3000")
    assert [w["status"] for w in want[:9]] == [M.OK] * 5 + [M.NO_OVERLAP] * 4
    assert want[0]["diagonalLen"] == 3000 and want[0]["score"] > 3000 and want[3]["diagonalLen"] == want[4]["diagonalLen"] == 1
    # 300 queries
    many = [_rand(rng, int(L)) for L in rng.integers(1, 41, size=300)]
    starts = np.concatenate([[0], np.cumsum([len(q[1]) for q in many])])
    assert (starts[:-1] % 2 == 1).any() and (starts[:-1] % 4 != 0).sum() > 100
    pairs = [(q, int(t), int(d)) for q in range(300) for t, d in zip(rng.integers(0, 4, size=2), rng.integers(-20, 20, size=2))]
    pairs += [(299, 3, 0), (0, 3, 0), (298, 2, -1)]
    want = _run(ctx, many, targets, pairs, m3, mA, "300 queries")
    assert {w["status"] for w in want} == {M.OK, M.NO_OVERLAP, M.UNDEFINED}
    ctx.close()


def test_bad_ids_and_refused_arguments():
    """query == nq, target == db.n and 0xFFFFFFFF: status BAD_ID next to correct neighbours; bad query layouts, a context without a database and one
    without the AA half are refused; the same context answers the next good call"""
    rng = np.random.default_rng(5)
    targets = [_rand(rng, L) for L in (8, 20, 45)]
    db, targets = _db(targets)
    queries = [_rand(rng, 30), _rand(rng, 11)]
    qA, q3 = [q[0] for q in queries], [q[1] for q in queries]
    m3, mA = _real(1.4)
    good = [(0, 2, 3), (1, 0, -2), (1, 2, 0), (0, 1, -5)]
    pairs = [good[0], (2, 0, 0), good[1], (0, 3, 0), (0xFFFFFFFF, 0, 0), good[2], (0, 0xFFFFFFFF, 1), (0xFFFFFFFF, 0xFFFFFFFF, -1), good[3], (1, 3, -32767)]
    ctx = _ctx(db)
    want = _run(ctx, queries, targets, pairs, m3, mA, "bad ids")
    assert [w["status"] == M.BAD_ID for w in want] == [False, True, False, True, True, False, True, True, False, True]
    assert all(want[k]["status"] != M.NO_OVERLAP for k in (0, 2, 5, 8))
    for off, ln in (([0, 30, 41], [30, -1]), ([0, 30, 41], [-30, 11]), ([0, 31, 41], [30, 11]), ([0, 30, 41], [30, 12]), ([0, 42, 41], [30, 1])):
        with pytest.raises(api.FsgpuError):
            ctx.diag_rescore(qA, q3, m3, mA, good, offsets=off, lengths=ln)
        _run(ctx, queries, targets, good, m3, mA, "after a refused layout")
    # the same bytes under another, valid, layout: three queries, the middle one starting at an odd offset
    cat = (np.concatenate(qA), np.concatenate(q3))
    three = [(cat[0][o:o + l], cat[1][o:o + l]) for o, l in ((0, 7), (7, 20), (30, 11))]
    p3 = [(0, 0, 1), (1, 1, -1), (1, 2, 4), (2, 0, -3), (2, 2, 10), (1, 0, 19), (1, 0, 20)]
    got = ctx.diag_rescore(qA, q3, m3, mA, p3, offsets=[0, 7, 30, 41], lengths=[7, 20, 11])
    _check(got, _model(three, targets, p3, m3, mA), p3, "explicit layout")
    ctx.close()
    # no database at all, then one
    ctx = api.Context(0)
    with pytest.raises(api.FsgpuError):
        ctx.diag_rescore(qA, q3, m3, mA, good)
    ctx.load_db(db)
    _run(ctx, queries, targets, good, m3, mA, "after 'no database'")
    # 3Di only, then with AA
    ctx.load_db(synth.PaddedDB(db.data3di, None, db.offsets, db.lengths))
    with pytest.raises(api.FsgpuError):
        ctx.diag_rescore(qA, q3, m3, mA, good)
    ctx.load_db(db)
    _run(ctx, queries, targets, good, m3, mA, "after 'no AA'")
    ctx.close()


def test_scratch_shared_with_the_other_entries():
    """the entry borrows the context's SW staging, id and result buffers: interleaved with the SW entries and the gapless scan on ONE context, every call
    returns what it returns on a fresh context"""
    rng = np.random.default_rng(3)
    q3s, qas = synth.make_queries(3, seed=21, mean_len=120, lo=60, hi=200)
    db = synth.make_db(200, (q3s, qas), seed=22, homologs_per_query=10, lo=20, hi=400, mask_frac=0.02)
    mA_, m3_ = api.Matrix(1, 1.4), api.Matrix(0, 2.1)
    t3, tA = (np.ascontiguousarray(np.array(m.scores()).reshape(21, 21).astype(np.int8)) for m in (m3_, mA_))
    m3, mA = _real(1.4)
    ids = [rng.choice(db.n, size=n, replace=False).astype(np.uint32) for n in (13, 20, 9)]
    compact = []
    for i in range(3):
        _, _, cba_f, cb3_f = api.align_profiles(mA_, m3_, qas[i], q3s[i], True, 0.5)
        _, _, cba_r, cb3_r = api.align_profiles(mA_, m3_, qas[i][::-1].copy(), q3s[i][::-1].copy(), True, 0.5)
        compact.append((qas[i], q3s[i], cba_f, cb3_f, cba_r, cb3_r, ids[i]))
    pAf, p3f, _, _ = api.align_profiles(mA_, m3_, qas[1], q3s[1], True, 0.5)
    pAr, p3r, _, _ = api.align_profiles(mA_, m3_, qas[1][::-1].copy(), q3s[1][::-1].copy(), True, 0.5)
    expl = [helpers.target_seqs(db, int(t)) for t in rng.choice(db.n, size=7, replace=False)]
    pssm, cap = api.prefilter_profile(api.Matrix(0, 2.0), q3s[2], True, 0.15)
    pairs = [(int(q), int(t), int(d)) for q, t, d in zip(rng.integers(0, 3, 40), rng.integers(0, db.n, 40), rng.integers(-60, 60, 40))]
    pairs2 = pairs[::-1][:33]
    steps = [
        lambda c: [x.tobytes() for x in c.sw_multi_dir_c(t3, tA, compact, 0)],
        lambda c: c.diag_rescore(qas, q3s, m3, mA, pairs).tobytes(),
        lambda c: [x.tobytes() for x in c.sw_batch_seqs(pAf, p3f, pAr, p3r, [e[0] for e in expl], [e[1] for e in expl])],
        lambda c: [x.tobytes() for x in c.sw_multi_dir_c(t3, tA, compact, 1)],
        lambda c: [x.tobytes() for x in c.sw_batch(pAf, p3f, pAr, p3r, ids[1])],
        lambda c: c.gapless_scan(pssm, cap, min_score=20, max_res=50).tobytes(),
        lambda c: c.diag_rescore(qas, q3s, m3, mA, pairs2).tobytes(),
    ]
    fresh = []
    for step in steps:
        c = _ctx(db)
        fresh.append(step(c))
        c.close()
    ctx = _ctx(db)
    for k, step in enumerate(steps):
        assert step(ctx) == fresh[k], f"step {k} differs from the same call on a fresh context"
    ctx.close()
    # ... and the fresh answers of the entry under test are the model's
    targets = [helpers.target_seqs(db, t) for t in range(db.n)]
    queries = list(zip(qas, q3s))
    want = _model(queries, targets, pairs, m3, mA)
    _check(np.frombuffer(fresh[1], api.DIAG_RES_DT), want, pairs, "fresh context")
    assert sum(w["status"] == M.OK for w in want) >= 10

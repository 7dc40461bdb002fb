"""Pins oracle/fs_kmer_oracle.c (the C restatement of the k-mer prefilter) to the
reference's own classes compiled into oracle/_ref (ref_kmer_harness.cpp): index table, masked sequence lookup,
extended 3-mer matrix rows, similar-k-mer lists and complete per-query hit lists, including the
databaseHits-overflow path, every BINSIZE-dependent ordering and the score-255 rescoring path.
Skipped where oracle/_ref could not be built (no /root/reference)."""
import numpy as np
import pytest

import helpers as H
import kmer_lib as K
from foldseek_amd import synth

N, NQ = 1500, 5


@pytest.fixture(scope="module")
def world():
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    O = K.load_ora()
    q3, qa = synth.make_queries(NQ, seed=3)
    db = synth.make_db(N, (q3, qa), seed=11, homologs_per_query=25, mask_frac=0.02)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    # a few hand-made edge cases: leading run of code 0 (never masked), long repeats, all-X, too short for a k-mer
    targets[0] = np.array([0] * 12 + [3, 4, 5, 6, 7, 8, 9, 10, 11, 12] * 3, np.uint8)
    targets[1] = np.array([5] * 9 + [1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13] + [7] * 7 + [2, 3], np.uint8)
    targets[2] = np.full(40, 20, np.uint8)
    targets[3] = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9], np.uint8)
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    r = K.RefKpf(R, targets)
    o = K.OraKpf(O, ksub, pb, usub, targets)
    yield dict(r=r, o=o, q3=q3, targets=targets, ksub=ksub, usub=usub)
    r.close(); o.close()


def test_matrices(world):
    assert (world["r"].submat(0).ravel() == world["ksub"]).all()
    assert (world["r"].submat(1).ravel() == world["usub"]).all()


def test_index_and_lookup(world):
    r, o = world["r"], world["o"]
    ro, oo = r.offsets(), o.offsets()
    assert (ro == oo).all() and ro[-1] > 0
    for i in list(range(8)) + list(range(8, N, 37)):
        L = len(world["targets"][i])
        assert (r.masked(i, L) == o.masked(i, L)).all(), i
    rng = np.random.default_rng(5)
    nz = np.nonzero(np.diff(ro.astype(np.int64)))[0]
    for k in rng.choice(nz, 300):
        a, b = r.index_list(k), o.index_list(k)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), k


def test_extended_matrix_rows(world):
    r, o = world["r"], world["o"]
    for idx in [0, 1, 19, 20, 399, 400, 7999, 1234, 4321, 6789]:
        a, b = r.row(3, idx), o.row(3, idx)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), idx
    for idx in [0, 7, 399]:
        a, b = r.row(2, idx), o.row(2, idx)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), idx


def test_similar_kmer_lists(world):
    r, o = world["r"], world["o"]
    rng = np.random.default_rng(9)
    for t in range(40):
        km = rng.integers(0, 20, 6).astype(np.uint8)
        thr = int(rng.integers(30, 130)) if t else 0
        a, b = r.kmer_list(km, thr), o.kmer_list(km, thr)
        assert len(a) == len(b) and (a == b).all(), (km, thr)


VARIANTS = [
    dict(),
    dict(maxResListLen=40),
    dict(maxResListLen=40, bins=4),
    dict(maxResListLen=40, bins=32),
    dict(maxResListLen=4),                                        # >= maxHits hits at 255 -> rescoreHits path
    dict(maxResListLen=300, maxDbMatches=9000),                   # several databaseHits overflows
    dict(maxResListLen=60, maxDbMatches=4000, bins=8),
    dict(maxResListLen=300, maxDbMatches=3000, foundDiagonalsSize=2500),
    dict(compBias=0, maxResListLen=25, maxDbMatches=7000),
    dict(minDiagScoreThr=12, maxResListLen=1500),
]


@pytest.mark.parametrize("kw", VARIANTS)
def test_hit_lists(world, kw):
    r, o, q3 = world["r"], world["o"], world["q3"]
    base = dict(maxResListLen=1000, bins=0, maxDbMatches=0, foundDiagonalsSize=0, compBias=1, minDiagScoreThr=30)
    base.update(kw)
    r.set(**base); o.set(**base)
    ident = np.array([-1, 7, -1, 100, -1], np.int64)
    rr, rs, _ = r.run(q3, ident)
    orr, os_ = o.run(q3, ident)
    for q in range(NQ):
        assert orr[q] is not None
        assert len(rr[q]) == len(orr[q]) and (rr[q] == orr[q]).all(), (q, kw)
        assert np.allclose(rs[q], os_[q]), (q, rs[q], os_[q])
    assert sum(len(x) for x in rr) > 0
    if "maxDbMatches" in kw:
        assert rs[:, 2].sum() > 0     # the overflow path was really taken


@pytest.mark.parametrize("kw", [dict(maxResListLen=100, minDiagScoreThr=0), dict(maxResListLen=5, minDiagScoreThr=0, bins=16), dict(maxResListLen=1000, minDiagScoreThr=2, bins=4),
                                dict(maxResListLen=100, minDiagScoreThr=0, compBias=0)])
def test_hit_lists_without_diagonal_scoring(world, kw):
    """--diag-score 0 (QueryMatcher with diagonalScoring == false, the first prefilter call of the cluster workflow's cascade): the oracle's
    restatement of findDuplicates(computeTotalScore) + the KMER_SCORE result path == the compiled reference -- ids, counts as scores,
    diagonals, order, truncation at --max-seqs, the query's own entry with score 255"""
    r, o, q3 = world["r"], world["o"], world["q3"]
    base = dict(maxResListLen=1000, bins=0, maxDbMatches=0, foundDiagonalsSize=0, compBias=1, minDiagScoreThr=0, noDiagScore=1)
    base.update(kw)
    r.set(**base); o.set(**base)
    ident = np.array([-1, 7, -1, 100, -1], np.int64)
    rr, rs, _ = r.run(q3, ident)
    orr, os_ = o.run(q3, ident)
    for q in range(NQ):
        assert orr[q] is not None
        assert len(rr[q]) == len(orr[q]) and (rr[q] == orr[q]).all(), (q, kw)
    assert sum(len(x) for x in rr) > min(50, 4 * base["maxResListLen"]) and rr[1][0]["id"] == 7 and rr[1][0]["score"] == 255
    r.set(noDiagScore=0); o.set(noDiagScore=0)


@pytest.mark.parametrize("kw", [dict(maxResListLen=300, maxDbMatches=9000), dict(maxResListLen=60, maxDbMatches=4000, bins=8),
                                dict(maxResListLen=1000, maxDbMatches=3000, bins=2), dict(maxResListLen=25, maxDbMatches=7000, compBias=0, minDiagScoreThr=3),
                                dict(maxResListLen=2000, maxDbMatches=2500, bins=32)])
def test_hit_lists_without_diagonal_scoring_with_refills(world, kw):
    """--diag-score 0 with databaseHits refills: mergeElementsByScore as the reference EXECUTES it (CacheFriendlyOperations.cpp:150-180) --
    a target present in two per-refill lists comes out twice (the sum, then the low byte of a diagonal as its "count") and bytes left by
    one bin seed the sums of later bins.  The oracle restates exactly that; the device path replays it per (query, id >> shift) group
    (k_kmer_merge_heads: tests/test_kmer_merge_model.py without a device, tests/test_kmer_gpu.py against the compiled reference).
    Entries that share (score, id) -- possible only through that duplication -- compare equal under the reference's
    compareHitsByScoreAndId, so their relative order is whatever its std::sort leaves: the lists are compared with such ties
    put in diagonal order on both sides, and each side is checked to be ordered by (score desc, id asc)."""
    def canon(a):
        return a[np.lexsort((a["diag"], a["id"], -a["score"]))]

    def _ordered(a):
        s, i = a["score"].astype(np.int64), a["id"].astype(np.int64)
        return bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] <= i[1:]))).all())

    r, o, q3 = world["r"], world["o"], world["q3"]
    base = dict(maxResListLen=1000, bins=0, maxDbMatches=0, foundDiagonalsSize=0, compBias=1, minDiagScoreThr=0, noDiagScore=1)
    base.update(kw)
    r.set(**base); o.set(**base)
    ident = np.array([-1, 7, -1, 100, -1], np.int64)
    rr, rs, _ = r.run(q3, ident)
    orr, os_ = o.run(q3, ident)
    dup = 0
    try:
        for q in range(NQ):
            assert orr[q] is not None
            assert len(rr[q]) == len(orr[q]) and _ordered(rr[q]) and _ordered(orr[q]), (q, kw)
            assert (canon(rr[q]) == canon(orr[q])).all(), (q, kw)
            assert np.allclose(rs[q], os_[q]), (q, rs[q], os_[q])
            dup += len(rr[q]) - len(np.unique(rr[q]["id"]))
        assert rs[:, 2].sum() > 0     # refills really happened
        assert dup > 0 or base["maxResListLen"] < 100      # ... and the reference's duplicated targets are in the lists
    finally:
        r.set(noDiagScore=0, maxDbMatches=0, bins=0); o.set(noDiagScore=0, maxDbMatches=0, bins=0)


def _canon(a):
    return a[np.lexsort((a["diag"], a["id"], -a["score"].astype(np.int64)))]


def test_cut_zero_elements_oracle_equals_the_compiled_reference():
    """--min-ungapped-score 0 with diagonal scores: the score-0 elements keepMaxScoreElementOnly hands on (CacheFriendlyOperations.cpp:354-384: after a
    target's best element every later zero-score element of it, all of them when its best is 0) come out when a query's cut is 0.  Two k-mer matches on
    one diagonal score above 0 under the real matrix, so the reference's own ungapped matrix object is lowered (ref_kpf_shift_ungapped) and the oracle
    gets the same matrix: random settings with refills, 2 .. 64 bins and cuts inside the zero elements (what the device is then held to:
    tests/test_kmer_gpu.py::test_cut_zero_with_diagonal_scores_equals_the_compiled_reference)."""
    R = K.load_ref()
    if R is None or not hasattr(R, "ref_kpf_shift_ungapped"):
        pytest.skip("oracle/_ref not built")
    O = K.load_ora()
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    rng = np.random.default_rng(3)
    zeros = refills = 0
    for it in range(8):
        thr = int(rng.choice([78, 60, 96])); delta = int(rng.choice([-5, -7, -8, -9, -12])); mean = int(rng.choice([40, 100, 250])); n = int(rng.choice([300, 1500]))
        kw = dict(kmerThr=thr, maxResListLen=int(rng.choice([3, 20, 100, 5000])), minDiagScoreThr=0, compBias=int(rng.integers(0, 2)), bins=int(rng.choice([2, 4, 16, 64])),
                  maxDbMatches=int(rng.choice([0, 800, 3000, 9000])))
        q3, qa = synth.make_queries(5, seed=int(rng.integers(1 << 30)), mean_len=mean, lo=10, hi=int(mean * 3))
        db = synth.make_db(n, (q3, qa), seed=int(rng.integers(1 << 30)), homologs_per_query=int(rng.integers(0, 30)), mask_frac=0.1, mean_len=mean, lo=8, hi=mean * 4)
        targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
        o = K.OraKpf(O, ksub, pb, (usub + delta).astype(usub.dtype), targets, **kw)
        r = K.RefKpf(R, targets, threads=2, **kw)
        R.ref_kpf_shift_ungapped(r.h, delta)
        ident = np.array([-1, 3, -1, -1, 7], np.int64)
        rr, rs, _ = r.run(list(q3), ident)
        for i, q in enumerate(q3):
            b, st = o.query(q, int(ident[i]))
            if b is None:
                continue
            assert len(b) == len(rr[i]) and (_canon(b) == _canon(rr[i])).all() and np.allclose(st[:3], rs[i][:3]), (it, i, kw, delta)
            zeros += int((b["score"] == 0).sum())
        refills += int(rs[:, 2].sum())
        o.close(); r.close()
    assert zeros > 100 and refills >= 3, (zeros, refills)


def test_find_duplicates_cut_short_oracle_equals_the_compiled_reference():
    """foundDiagonals full: findDuplicates returns at the first bin whose candidates do not fit (CacheFriendlyOperations.cpp:217-219) and the query goes on
    with what fitted.  The oracle's restatement against the compiled reference with its buffer shrunk, on the database and the eight settings the device
    is held to (tests/test_kmer_gpu.py::test_find_duplicates_cut_short_equals_the_compiled_reference), with and without refills; counted: the queries
    whose answer differs from the one with the full-size buffer."""
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    O = K.load_ora()
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    q3, qa = synth.make_queries(6, seed=21, mean_len=200, lo=40, hi=600)
    db = synth.make_db(3000, (q3, qa), seed=22, homologs_per_query=60, mask_frac=0.05, mean_len=200, lo=20, hi=800, stay=0.5)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ident = np.array([-1, 3, -1, -1, 7, -1], np.int64)
    cut = cut_refilled = compared = 0
    for kw in [dict(foundDiagonalsSize=150, bins=16, maxDbMatches=3000), dict(foundDiagonalsSize=250, bins=4, maxDbMatches=9000), dict(foundDiagonalsSize=400, bins=2),
               dict(foundDiagonalsSize=200, bins=64, maxDbMatches=20000, maxResListLen=50), dict(foundDiagonalsSize=120, bins=8, maxDbMatches=1500, kmerThr=90),
               dict(foundDiagonalsSize=1500, bins=32, kmerThr=60), dict(foundDiagonalsSize=180, bins=2, maxDbMatches=2500, compBias=0),
               dict(foundDiagonalsSize=2500, bins=8, kmerThr=60, maxDbMatches=30000)]:
        full = dict(kmerThr=78, maxResListLen=1000, minDiagScoreThr=15, compBias=1)
        full.update(kw)
        o = K.OraKpf(O, ksub, pb, usub, targets, **full)
        r = K.RefKpf(R, targets, threads=4, **full)
        rr, rs, _ = r.run(list(q3), ident)
        r.close()
        r = K.RefKpf(R, targets, threads=4, **dict(full, foundDiagonalsSize=0))
        rr0, _, _ = r.run(list(q3), ident)
        r.close()
        for i, q in enumerate(q3):
            differs = not (len(rr[i]) == len(rr0[i]) and (rr[i] == rr0[i]).all())
            b, st = o.query(q, int(ident[i]))
            if b is None:
                continue                                 # std::sort branch: not modelled by the oracle (the device replays it, tests/test_kmer_gpu.py)
            compared += 1
            assert len(b) == len(rr[i]) and (b == rr[i]).all() and np.allclose(st[:3], rs[i][:3]), (i, kw)
            cut += differs
            cut_refilled += differs and st[2] > 0
        o.close()
    assert compared >= 25 and cut >= 15 and cut_refilled >= 5, (compared, cut, cut_refilled)


# ---- the shapes tests/test_kmer_edges_gpu.py holds the device to: the oracle is only as good as its pin ------------------------------------
def _pin(r, o, qs, ident, **kw):
    """reference and oracle with one parameter set: hit lists and statistics identical -> (lists, reference statistics, the oracle's refill counts)"""
    base = dict(maxResListLen=1000, bins=0, maxDbMatches=0, foundDiagonalsSize=0, compBias=1, minDiagScoreThr=30)
    base.update(kw)
    r.set(**base); o.set(**base)
    rr, rs, _ = r.run(qs, ident)
    refills = []
    for i, q in enumerate(qs):
        b, st = o.query(q, -1 if ident is None else int(ident[i]))
        refills.append(o.last_refills)
        assert b is not None and len(b) == len(rr[i]) and (b == rr[i]).all(), (i, kw, len(b), len(rr[i]))
        assert np.allclose(st[:3], rs[i][:3]), (i, kw, st, rs[i])
        assert (refills[-1] > 0) == (rs[i][2] > 0), (i, kw, refills[-1])
    return rr, rs, refills


@pytest.fixture(scope="module")
def small3000():
    """the 3000-target database of test_kmer_gpu.py / test_kmer_edges_gpu.py"""
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    q3, qa = synth.make_queries(6, seed=1)
    db = synth.make_db(3000, (q3, qa), homologs_per_query=30, mask_frac=0.02)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    r = K.RefKpf(R, targets)
    o = K.OraKpf(K.load_ora(), ksub, pb, usub, targets)
    yield dict(r=r, o=o, q3=q3, db=db)
    r.close(); o.close()


def test_long_queries(small3000):
    """2925 .. 20000 residues (beyond 2925 the device reads the profile from global memory); diagonals on both sides of 0"""
    r, o, db = small3000["r"], small3000["o"], small3000["db"]
    qs = [K.long_query(db, L, first) for L, first in K.LONG_QUERIES] + [small3000["q3"][0][:50]]
    rr, rs, refills = _pin(r, o, qs, None)
    assert all(len(x) > 0 for x in rr) and all((x["diag"] > 32767).any() for x in rr[:4]) and refills[3] >= 1


def test_longest_query():
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    db, q3, q = K.longest_query_world()
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    r = K.RefKpf(R, targets, kmerThr=100)
    o = K.OraKpf(K.load_ora(), ksub, pb, usub, targets, kmerThr=100)
    rr, _, _ = _pin(r, o, [q[:32767]] + list(q3), None, kmerThr=100, maxResListLen=50, minDiagScoreThr=15)
    assert len(rr[0]) == 50 and (rr[0]["diag"] > 32767).any()
    r.close(); o.close()


def test_more_than_255_refills(small3000):
    """the reference has no limit on databaseHits refills (the device replays 255): 9, 255, 256 and several hundred of them"""
    r, o, q3 = small3000["r"], small3000["o"], small3000["q3"]
    qs = [q3[0], q3[1][:60], q3[1], q3[2][:40], q3[4][:100]]
    ident = np.array([-1, -1, -1, 5, -1], np.int64)
    for m, want in ((4674, 9), (166, 255), (165, 256), (100, None)):
        rr, rs, refills = _pin(r, o, qs, ident, maxDbMatches=m, maxResListLen=300)
        assert (refills[0] == want if want else refills[0] > 400) and len(rr[0]) > 0, (m, refills)


def test_one_list_fills_database_hits(small3000):
    """a single index list of maxDbMatches entries or more: match() gives up (QueryMatcher.cpp:330-332) -- no hits but the identity, statistics cut short"""
    r, o, q3 = small3000["r"], small3000["o"], small3000["q3"]
    qs = [q3[0], q3[0], q3[0][:11], q3[3][5:18]]
    ident = np.array([-1, 7, -1, -1], np.int64)
    _, whole, _ = _pin(r, o, qs, ident, maxResListLen=100)
    for m in (4, 6, 8):
        rr, rs, refills = _pin(r, o, qs, ident, maxDbMatches=m, maxResListLen=100)
        assert len(rr[0]) == 0 and rs[0][1] < whole[0][1] and len(rr[1]) == 1 and rr[1][0]["id"] == 7 and len(rr[3]) == 0, (m, rs)
        assert len(rr[2]) > 0 and rs[2][1] == whole[2][1], (m, rs)                          # and a query that does not give up


@pytest.mark.parametrize("last_len", [8191, 8192])
def test_wide_database(last_len):
    """300 000 short targets and one of 8191 / 8192 residues as the last id (test_kmer_edges_gpu.py: index entries of 32 used bits / of 8 bytes)"""
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    db, q3 = K.wide_world(last_len)
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    r = K.RefKpf.from_padded(R, db)
    o = K.OraKpf.from_padded(K.load_ora(), ksub, pb, usub, db)
    assert (r.offsets() == o.offsets()).all()
    rr, _, _ = _pin(r, o, [q3[0], q3[2], q3[4]], np.array([-1, db.n - 1, -1], np.int64), minDiagScoreThr=15)
    assert db.n - 1 in rr[2]["id"] and rr[1][0]["id"] == db.n - 1
    r.close(); o.close()

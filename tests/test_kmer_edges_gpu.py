"""The k-mer prefilter on the paths the small shapes of test_kmer_gpu.py never take (fsgpu_kmer.hip / k_kmer.hpp), each against the C oracle
(oracle/fs_kmer_oracle.c, pinned to the compiled reference at these very shapes by test_kmer_oracle_vs_ref.py), bit-exact -- ids, scores,
diagonals, order, statistics:
  1  8-byte index entries (k_kmer_compact_entries, k_kmer_emit<uint64_t>): natural (id bits + position bits > 32) and forced (FSGPU_KMER_ENTRY64)
  2  4-byte entries that fill all 32 bits (19 id bits + 13 position bits, the long target is the last id: top bit set)
  3  k_kmer_scatter_stable<3..9> and the duplicate stage with more than 60 KB of LDS (a key of 65 536 ids)
  4  profiles read from global memory by k_kmer_score8 / k_kmer_score (queries of 2926 residues and more)
  5  one index list alone fills databaseHits: the query is answered empty, its statistics stop there
  6  255 refills are replayed, the 256th is FSGPU_KMER_E_CHUNKS; chunk tables of more than eight chunks in a batch of more than 64 queries
  7  FSGPU_KMER_E_OUTPUT stays a status with kmerScoreOnly
  8  the forced forms: k_kmer_score, k_kmer_walk<false> as the first walk, both LDS sizes of k_kmer_lists_w on rows they were not chosen for
  9  ids with all bits set in (query << tbits | target); queries of 32767 residues, refusal of 32768
Not reachable in seconds and left to test_kmer_fullsize_gpu.py: the block table of the emit stage in global memory (> 8.3 M targets), the
halving of a batch (> 4.8e8 hits), fewer than 1024 queries per batch (23 or more id bits)."""
import numpy as np
import pytest

import helpers as H
import kmer_lib as K
import test_kmer_gpu as T
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

E_OUTPUT, E_CHUNKS = -1, -2
BASE = dict(maxResListLen=1000, bins=0, maxDbMatches=0, foundDiagonalsSize=0, compBias=1, minDiagScoreThr=30)


def _mats():
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    return ksub, pb, usub


def _same(a, b):
    return len(a) == len(b) and bool((a["id"] == b["id"]).all() and (a["score"] == b["score"]).all() and (a["diag"] == b["diag"]).all())


def _search(w, qs, ident=None, thr=78, score_only=False, **kw):
    """one device call with the oracle's parameter names -> (hits, status, stats)"""
    p = dict(BASE, **kw)
    prep = [api.kmer_query_prepare(w["m8"], w["m2"], q, comp_bias=bool(p["compBias"]), scale=0.15, kmer_thr=thr) for q in qs]
    return w["ctx"].kmer_search(prep, identity=ident, max_res=p["maxResListLen"], min_diag=p["minDiagScoreThr"], bins=p["bins"],
                                max_db_matches=p["maxDbMatches"], found_diagonals_size=p["foundDiagonalsSize"], l2_cache_size=2 * 1024 * 1024,
                                want_stats=True, kmer_score_only=score_only)


def _oracle(o, qs, ident=None, **kw):
    """-> (hits, stats, refills) per query"""
    o.set(**dict(BASE, **kw))
    out = []
    for i, q in enumerate(qs):
        r, s = o.query(q, -1 if ident is None else int(ident[i]))
        assert r is not None
        out.append((r, s, o.last_refills))
    return out


def _equal(got, want, tag=()):
    """status 0, statistics and hit lists of one device call == the oracle's"""
    res, status, stats = got
    assert len(res) == len(want)
    for q, (r, s, _) in enumerate(want):
        assert status[q] == 0, tag + (q, int(status[q]))
        assert np.allclose(stats[q][:3], s[:3]), tag + (q, stats[q], s)
        assert _same(res[q], r), tag + (q, len(res[q]), len(r), res[q][:3], r[:3])


# ---- B1: the wide database ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(request):
    last_len, nbytes = dict(fit32=(8191, 4), nat64=(8192, 8))[request.param]
    db, q3 = K.wide_world(last_len)
    ksub, pb, usub = _mats()
    o = K.OraKpf.from_padded(K.load_ora(), ksub, pb, usub, db)
    ctx = api.Context(0)
    ctx.load_db(db)
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    ctx.kmer_index_build(m8, kmer_thr=78)
    ident = np.array([-1, -1, db.n - 1, -1, -1, -1], np.int64)
    kw = dict(minDiagScoreThr=15)
    yield dict(o=o, ctx=ctx, db=db, q3=q3, m8=m8, m2=m2, nbytes=nbytes, ident=ident, kw=kw, want=_oracle(o, q3, ident, **kw))
    o.close()
    ctx.close()


BOTH = pytest.mark.parametrize("wide", ["fit32", "nat64"], indirect=True)


@BOTH
def test_wide_database_is_what_the_tests_need(wide):
    """the oracle alone: every list non-empty, the hits spread over at least 128 of the 293 blocks of 1024 ids and reach the last one, two
    queries of more than three tiles of index hits, the long last target found by the query planted in it -- on a negative diagonal"""
    db, want = wide["db"], wide["want"]
    assert db.n == K.WIDE_N and int(db.lengths[-1]) == (8191 if wide["nbytes"] == 4 else 8192) and int(db.lengths[:-1].max()) == 24
    assert all(len(r) > 0 for r, _, _ in want)
    blocks = set()
    for r, _, _ in want:
        blocks |= set((r["id"] >> 10).tolist())
    assert len(blocks) >= 128 and ((db.n - 1) >> 10) in blocks, len(blocks)
    assert sum(s[1] >= 3 * 16384 for _, s, _ in want) >= 2
    last = want[4][0][want[4][0]["id"] == db.n - 1]
    assert len(last) == 1 and last[0]["diag"] > 32767 and last[0]["score"] > 255
    assert want[2][0][0]["id"] == db.n - 1 and want[2][0][0]["score"] == 65535              # the identity hit n - 1


@BOTH
def test_wide_index_equals_oracle(wide):
    o, ctx, db = wide["o"], wide["ctx"], wide["db"]
    assert ctx.kmer_index_entry_bytes == wide["nbytes"]
    ooff, oseq, opos = o.index()
    off, seq, pos, _ = ctx.kmer_index_reference_order(db.data3di.size)
    assert ctx.kmer_index_entries == int(ooff[-1])
    assert (off == ooff).all()
    assert (seq == oseq).all() and (pos == opos).all()
    assert (oseq == db.n - 1).sum() > 4000 and int(opos[oseq == db.n - 1].max()) > 8100         # the long target's entries, positions of 13 bits


@BOTH
def test_wide_hit_lists(wide):
    assert wide["ctx"].kmer_index_entry_bytes == wide["nbytes"]
    _equal(_search(wide, wide["q3"], wide["ident"], **wide["kw"]), wide["want"], (wide["nbytes"],))


@pytest.mark.parametrize("wide", ["fit32"], indirect=True)
def test_wide_every_key_width(wide, monkeypatch):
    """the eight coarse-key levels of 300 000 targets: 293 ... 5 keys, so the stable scatter runs with 9 ... 3 ballots per record, and the level of
    64 blocks per key gives the duplicate stage a key of 65 536 ids (65 540 bytes of LDS: the raised limit)"""
    ctx = wide["ctx"]
    bits, widest = set(), set()
    for level in range(8):
        monkeypatch.setenv("FSGPU_KMER_BIN_LEVEL", str(level))
        got = _search(wide, wide["q3"], wide["ident"], **wide["kw"])
        seg = ctx.kmer_segments()
        bits.add(int(np.ceil(np.log2(int(seg[5])))))
        widest.add(int(seg[6]))
        _equal(got, wide["want"], (level, seg))
    monkeypatch.delenv("FSGPU_KMER_BIN_LEVEL")
    assert bits >= {3, 4, 5, 6, 7, 8, 9}, bits
    assert 65536 in widest, widest


# ---- the 3000-target database of test_kmer_gpu.py ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    q3, qa = synth.make_queries(T.NQ, seed=1)
    db = synth.make_db(T.N, (q3, qa), homologs_per_query=30, mask_frac=0.02)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ksub, pb, usub = _mats()
    o = K.OraKpf(K.load_ora(), ksub, pb, usub, targets)
    ctx = api.Context(0)
    ctx.load_db(db)
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    ctx.kmer_index_build(m8, kmer_thr=78)
    assert ctx.kmer_index_entry_bytes == 4
    yield dict(o=o, ctx=ctx, db=db, q3=q3, m8=m8, m2=m2, targets=targets)
    o.close()
    ctx.close()


# ---- B2: 8-byte entries forced at the old shape ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small64(small):
    ctx = api.Context(0)
    ctx.load_db(small["db"])
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("FSGPU_KMER_ENTRY64", "1")
        ctx.kmer_index_build(small["m8"], kmer_thr=78)
    yield dict(small, ctx=ctx)
    ctx.close()


def test_forced_wide_entries_index(small64):
    o, ctx, db = small64["o"], small64["ctx"], small64["db"]
    assert ctx.kmer_index_entry_bytes == 8
    ooff, oseq, opos = o.index()
    off, seq, pos, _ = ctx.kmer_index_reference_order(db.data3di.size)
    assert ctx.kmer_index_entries == int(ooff[-1]) and (off == ooff).all() and (seq == oseq).all() and (pos == opos).all()


@pytest.mark.parametrize("kw", T.VARIANTS)
def test_forced_wide_entries_hit_lists(small64, kw):
    assert small64["ctx"].kmer_index_entry_bytes == 8
    ident = np.array([-1, 7, -1, 100, -1, -1], np.int64)
    want = _oracle(small64["o"], small64["q3"], ident, **kw)
    _equal(_search(small64, small64["q3"], ident, **kw), want, (kw,))
    assert "maxDbMatches" not in kw or sum(n for _, _, n in want) > 0


def test_forced_wide_entries_count_mode_with_refills_equals_the_compiled_reference(small64):
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    kw = dict(maxResListLen=300, minDiagScoreThr=2, bins=4, maxDbMatches=8000)
    ident = np.array([-1, 7, -1, 100, -1, -1], np.int64)
    res, status, stats = _search(small64, small64["q3"], ident, score_only=True, **kw)
    r = K.RefKpf(R, small64["targets"], threads=4, noDiagScore=1, compBias=1, **kw)
    rr, rs, _ = r.run(small64["q3"], ident)
    r.close()
    canon = lambda a: a[np.lexsort((a["diag"], a["id"], -a["score"].astype(np.int64)))]        # (score, id) ties: see test_kmer_gpu.py
    for q in range(T.NQ):
        assert status[q] == 0 and len(res[q]) == len(rr[q]) and (canon(res[q]) == canon(rr[q])).all(), q
        assert np.allclose(stats[q][:3], rs[q][:3]), (q, stats[q], rs[q])
    assert rs[:, 2].sum() >= 4 and sum(len(x) for x in rr) > 200


# ---- B3: long queries -----------------------------------------------------------------------------------------------------------------
def test_profiles_too_long_for_lds(small):
    """a profile of more than 61 440 bytes stays in global memory (k_kmer_score8: staged == false) -- 2925 residues is the last staged length,
    2926 the first unstaged one; short and long queries next to each other, so a workgroup's first query is staged and a later one is not, and
    the reverse; 20000 residues refill databaseHits on their own"""
    o, db, q3 = small["o"], small["db"], small["q3"]
    q2925, q2926, q6000, q20000 = (K.long_query(db, L, first) for L, first in K.LONG_QUERIES)
    q50 = q3[0][:50]
    for qs in ([q2925, q2926, q6000, q50], [q50, q6000], [q20000]):
        want = _oracle(o, qs)
        _equal(_search(small, qs), want, tuple(len(q) for q in qs))
        assert all(len(r) > 0 for r, _, _ in want)
        assert all((r["diag"] > 32767).any() for (r, _, _), q in zip(want, qs) if len(q) > 50)
    assert want[0][2] >= 1                                       # the 20000-residue query refilled


def test_longest_query_and_the_refusals():
    """32767 residues is the longest query (and target) the device takes; 32768 is refused by the argument checks, and the context goes on"""
    db, q3, q = K.longest_query_world()
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ksub, pb, usub = _mats()
    o = K.OraKpf(K.load_ora(), ksub, pb, usub, targets, kmerThr=100)
    ctx = api.Context(0)
    ctx.load_db(db)
    w = dict(ctx=ctx, m8=api.Matrix(0, 8.0, -0.2), m2=api.Matrix(0, 2.0, -0.2))
    ctx.kmer_index_build(w["m8"], kmer_thr=100)
    kw = dict(maxResListLen=50, minDiagScoreThr=15)
    want = _oracle(o, [q[:32767]], **kw)
    _equal(_search(w, [q[:32767]], thr=100, **kw), want)
    assert len(want[0][0]) > 0 and (want[0][0]["diag"] > 32767).any()
    seq, thr, prof = api.kmer_query_prepare(w["m8"], w["m2"], q[:32767], kmer_thr=100)
    assert len(q) == 32768
    too_long = (q, np.append(thr, thr[-1:]), np.vstack([prof, prof[-1:]]))
    with pytest.raises(api.FsgpuError, match="32768"):
        ctx.kmer_search([api.kmer_query_prepare(w["m8"], w["m2"], q3[0], kmer_thr=100), too_long], max_res=50, min_diag=15)
    want = _oracle(o, q3, **kw)
    _equal(_search(w, q3, thr=100, **kw), want)
    # a database with a target of 32768 residues loads, but gets no k-mer index; the index built before stays in use
    lens = np.array([40, 32768], np.int32)
    off = np.array([0, 40, 40 + 32768], np.int64)
    big = synth.PaddedDB(np.concatenate([q[:40], q]), None, off, lens)
    ctx2 = api.Context(0)
    ctx2.load_db(big)
    with pytest.raises(api.FsgpuError, match="32768"):
        ctx2.kmer_index_build(w["m8"], kmer_thr=100)
    assert ctx2.kmer_index_entry_bytes == 0
    ctx2.load_db(db)
    ctx2.kmer_index_build(w["m8"], kmer_thr=100)
    _equal(_search(dict(w, ctx=ctx2), q3, thr=100, **kw), want)
    o.close(); ctx.close(); ctx2.close()


# ---- B4: refill edges -----------------------------------------------------------------------------------------------------------------
# query 0 of the 3000-target database makes 42 060 index hits; the oracle's refill counter falls as maxDbMatches grows, these are the largest
# values that still give 9, 255 and 256 refills (searched with the oracle alone, asserted below)
MAXDB_9, MAXDB_255, MAXDB_256 = 4674, 166, 165


def _check_with_chunk_limit(got, want, tag):
    res, status, stats = got
    for q, (r, s, refills) in enumerate(want):
        if refills > 255:
            assert status[q] == E_CHUNKS and len(res[q]) == 0, tag + (q, refills, int(status[q]), len(res[q]))
        else:
            assert status[q] == 0 and np.allclose(stats[q][:3], s[:3]) and _same(res[q], r), tag + (q, refills, int(status[q]), stats[q], s)


def test_refills_up_to_255_are_replayed_and_the_256th_is_a_status(small):
    o, q3 = small["o"], small["q3"]
    qs = [q3[0], q3[1][:60], q3[1], q3[2][:40], q3[4][:100]]
    ident = np.array([-1, -1, -1, 5, -1], np.int64)
    seen = {}
    for m in (MAXDB_9, MAXDB_255, MAXDB_256):
        want = _oracle(o, qs, ident, maxDbMatches=m, maxResListLen=300)
        seen[m] = [n for _, _, n in want]
        _check_with_chunk_limit(_search(small, qs, ident, maxDbMatches=m, maxResListLen=300), want, (m,))
    assert seen[MAXDB_9][0] == 9 and seen[MAXDB_255][0] == 255 and seen[MAXDB_256][0] == 256, seen
    assert seen[MAXDB_255][2] == 256 and max(seen[MAXDB_256][1], seen[MAXDB_256][3], seen[MAXDB_256][4]) <= 255, seen   # both sides of the edge in one batch
    assert all(len(want[q][0]) > 0 for q in (1, 3, 4))


def test_more_than_eight_chunks_in_a_batch_of_more_than_64_queries(small):
    """batches of more than 64 queries fetch the head of every chunk table and the rest only when a query has more than eight chunks"""
    o, q3, ctx = small["o"], small["q3"], small["ctx"]
    qs = [q3[i % T.NQ][: len(q3[i % T.NQ]) - 3 * (i // T.NQ)] for i in range(70)]
    ident = np.array([(-1 if i % 3 else (i * 7) % T.N) for i in range(70)], np.int64)
    want = _oracle(o, qs, ident, maxDbMatches=MAXDB_9, maxResListLen=200)
    _search(small, qs[:6], None)                                                       # the context knows what a query costs: one batch of 70
    _equal(_search(small, qs, ident, maxDbMatches=MAXDB_9, maxResListLen=200), want)
    seg = ctx.kmer_segments()
    assert seg[4] >= 70 * seg[5], seg                                                  # all 70 in ONE device batch
    assert want[0][2] == 9 and max(n for _, _, n in want) > 9 and min(n for _, _, n in want) < 8


def test_one_list_fills_database_hits(small):
    """maxDbMatches no larger than one index list the query meets: match() leaves its loop there, the answer is empty (the identity hit apart) and the
    statistics stop at that list.  Queries that abort and queries that do not in one batch; with maxDbMatches = 8 the first such list of query 0
    comes after more than 255 refills, which the device declines as FSGPU_KMER_E_CHUNKS"""
    o, q3 = small["o"], small["q3"]
    qs = [q3[0], q3[0], q3[0][:11], q3[3][5:18]]
    ident = np.array([-1, 7, -1, -1], np.int64)
    for m, aborting in ((6, [0, 1, 3]), (4, [0, 1, 3])):
        whole = _oracle(o, qs, ident, maxResListLen=100)
        want = _oracle(o, qs, ident, maxDbMatches=m, maxResListLen=100)
        assert max(n for _, _, n in want) <= 255
        for q in range(len(qs)):
            assert (want[q][1][1] < whole[q][1][1]) == (q in aborting), (m, q)         # an abort is what cuts the index hits short
        assert len(want[0][0]) == 0 and len(want[3][0]) == 0 and len(want[2][0]) > 0
        assert len(want[1][0]) == 1 and want[1][0][0]["id"] == 7 and want[1][0][0]["score"] == 65535
        _equal(_search(small, qs, ident, maxDbMatches=m, maxResListLen=100), want, (m,))
    want = _oracle(o, qs, ident, maxDbMatches=8, maxResListLen=100)
    assert want[0][2] > 255 and len(want[0][0]) == 0
    _check_with_chunk_limit(_search(small, qs, ident, maxDbMatches=8, maxResListLen=100), want, (8,))


# ---- B5: count mode keeps its status ----------------------------------------------------------------------------------------------------
def test_count_mode_keeps_the_output_status():
    """--diag-score 0 with foundDiagonals nearly full: no truncation replay in this mode (the reference's next merge would read what the aborted bin
    left behind), so a query whose candidates may not have fitted is answered FSGPU_KMER_E_OUTPUT without hits; the others equal the compiled
    reference.  Data and bins of test_find_duplicates_cut_short_equals_the_compiled_reference's third setting (foundDiagonalsSize = 400, which flags
    every query in this mode), and larger buffers up to one that flags none"""
    q3, qa = synth.make_queries(6, seed=21, mean_len=200, lo=40, hi=600)
    db = synth.make_db(3000, (q3, qa), seed=22, homologs_per_query=60, mask_frac=0.05, mean_len=200, lo=20, hi=800, stay=0.5)
    ident = np.array([-1, 3, -1, -1, 7, -1], np.int64)
    w = dict(ctx=api.Context(0), m8=api.Matrix(0, 8.0, -0.2), m2=api.Matrix(0, 2.0, -0.2))
    w["ctx"].load_db(db)
    w["ctx"].kmer_index_build(w["m8"], kmer_thr=78)
    got = {}
    for size in (400, 1500, 5000, 20000, 100000):
        kw = dict(foundDiagonalsSize=size, bins=2, minDiagScoreThr=15)
        res, status, stats = got[size] = _search(w, q3, ident, score_only=True, **kw)
        print("count mode: foundDiagonalsSize", size, "status", status.tolist(), "hits", [len(r) for r in res])
        for q in range(6):
            assert status[q] == E_OUTPUT and len(res[q]) == 0 or status[q] >= 0, (size, q, int(status[q]), len(res[q]))
    w["ctx"].close()
    assert (got[400][1] == E_OUTPUT).all() and (got[100000][1] >= 0).all()
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    compared = 0
    for size, (res, status, stats) in got.items():
        if (status < 0).all():
            continue
        r = K.RefKpf(R, targets, threads=4, noDiagScore=1, kmerThr=78, **dict(BASE, foundDiagonalsSize=size, bins=2, minDiagScoreThr=15))
        rr, rs, _ = r.run(list(q3), ident)
        r.close()
        for q in range(6):
            if status[q] >= 0:
                assert _same(res[q], rr[q]) and np.allclose(stats[q][:3], rs[q][:3]), (size, q, int(status[q]), len(res[q]), len(rr[q]))
                compared += 1
    assert compared >= 6


# ---- B6: forced forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [130, 78, 0])
def test_forced_forms_of_lists_scoring_and_walk(thr, monkeypatch):
    """FSGPU_KMER_WAVE_SMALL / FSGPU_KMER_SCORE8 / FSGPU_KMER_WALK_FF are read per batch: the small LDS form of k_kmer_lists_w on rows with more than
    128 passing entries and the large one on rows with a handful, k_kmer_score (one lane per candidate) and k_kmer_walk<false> as the first walk --
    with real refill rounds (maxDbMatches = 3000) and with a 6000-residue query whose profile stays in global memory"""
    q3, qa = synth.make_queries(4, seed=77, mean_len=60, lo=40, hi=80)
    db = synth.make_db(400, (q3, qa), seed=78, homologs_per_query=10, mean_len=120, lo=30, hi=300)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ksub, pb, usub = _mats()
    o = K.OraKpf(K.load_ora(), ksub, pb, usub, targets, kmerThr=thr)
    w = dict(ctx=api.Context(0), m8=api.Matrix(0, 8.0, -0.2), m2=api.Matrix(0, 2.0, -0.2))
    w["ctx"].load_db(db)
    w["ctx"].kmer_index_build(w["m8"], kmer_thr=thr)
    q6000 = np.concatenate([db.seq(399)[100:]] + [db.seq(i) for i in range(398, 300, -1)])[:6000]
    assert len(q6000) == 6000
    qs = (list(q3) + [q3[0][:7], q3[1][3:9], q6000]) if thr else [q3[0][:16]]
    settings = [dict(maxResListLen=100), dict(maxResListLen=100, maxDbMatches=3000)]
    want = [_oracle(o, qs, **kw) for kw in settings]
    assert want[1][-1][2] >= (11 if thr == 78 else 1) and want[0][-1][2] == 0            # refill rounds of the last query: 1, 11 and 3
    forms = [dict(FSGPU_KMER_WAVE="1", FSGPU_KMER_WAVE_SMALL=s) for s in "01"] + \
            [dict(FSGPU_KMER_SCORE8=s, FSGPU_KMER_WALK_FF=f) for s in "01" for f in "01"]
    for env in forms:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for kw, wt in zip(settings, want):
            _equal(_search(w, qs, thr=thr, **kw), wt, (thr, env, kw))
        for k in env:
            monkeypatch.delenv(k)
    o.close()
    w["ctx"].close()


# ---- B7: ids with all bits set -------------------------------------------------------------------------------------------------------------
def _exact_db(n, q3, qa, seed):
    """exactly n targets of 24 .. 63 residues in ascending length; query k's homolog (15 % substitutions) overwrites id n - 1, 1023, 1024 for
    k = 0, 1, 2 where that id exists and is not taken -> (db, [(query, id)])"""
    rng = np.random.default_rng(seed)
    lens = np.sort(rng.integers(24, 64, n)).astype(np.int32)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum((lens + 3) // 4 * 4)
    d3, da = synth._draw(rng, int(offsets[-1]), synth.BACK_3DI), synth._draw(rng, int(offsets[-1]), synth.BACK_AA)
    planted = []
    for k, t in enumerate((n - 1, 1023, 1024)):
        if t >= n or t in [p[1] for p in planted]:
            continue
        L = min(int(lens[t]), len(q3[k]))
        h = np.where(rng.random(L) < 0.15, synth._draw(rng, L, synth.BACK_3DI), q3[k][:L])
        d3[offsets[t]:offsets[t] + L] = h
        planted.append((k, t))
    for t in range(n):
        d3[offsets[t] + lens[t]:offsets[t + 1]] = 20; da[offsets[t] + lens[t]:offsets[t + 1]] = 20
    return synth.PaddedDB(d3, da, offsets, lens), planted


@pytest.mark.parametrize("n", [1024, 1025, 4096, 4097])
def test_ids_with_all_bits_set(n):
    """n a power of two: target n - 1 is all ones in its tbits; four queries: query 3 | target n - 1 is all ones in the candidate key; one more
    target moves every id bit up by one"""
    q3, qa = synth.make_queries(3, seed=5, mean_len=60, lo=50, hi=70)
    db, planted = _exact_db(n, q3, qa, 100 + n)
    assert db.n == n
    q3 = list(q3) + [q3[0][2:]]
    planted = planted + [(3, n - 1)]
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    ksub, pb, usub = _mats()
    o = K.OraKpf(K.load_ora(), ksub, pb, usub, targets)
    w = dict(ctx=api.Context(0), m8=api.Matrix(0, 8.0, -0.2), m2=api.Matrix(0, 2.0, -0.2))
    w["ctx"].load_db(db)
    w["ctx"].kmer_index_build(w["m8"], kmer_thr=78)
    kw = dict(minDiagScoreThr=15, maxResListLen=n)
    want = _oracle(o, q3, **kw)
    for k, t in planted:
        assert t in want[k][0]["id"], (k, t)
    assert {t for _, t in planted} >= {n - 1} | ({1023} if n > 1024 else set()) | ({1024} if n > 1025 else set())
    _equal(_search(w, q3, **kw), want, (n,))
    o.close()
    w["ctx"].close()

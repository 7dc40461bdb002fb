"""Profile queries in the k-mer prefilter on the device (fsgpu_kmer_search_profile, k_kmer_profile.hpp):

1. the similar-k-mer lists, position by position through fsgpu_kmer_profile_list_copy, against tests/kmer_profile_model.py -- K_p of EVERY position
   (the model's count) and the content, in emission order, of a seeded share of them and of every special one;
2. the entry end to end against every frozen record of tests/golden/profile_kmer_v1 (the reference's `prefilter` with profile queries): ids, scores,
   diagonals, order, counts; the crafted world once as one batch and once one query per call;
3. the contract edges;
4. fshost_search_kmer_batch_profile on the 12 example structures.
"""
import functools
import json
import os

import numpy as np
import pytest

import kmer_profile_model as km
import profile_model as pm
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "profile_kmer_v1")
SRC = os.path.join(HERE, "golden", "profile_v1")
LETTERS = "ACDEFGHIKLMNPQRSTVWYX"
SLICE = 8192                      # kListSlice: similar k-mers of one position per workgroup of the list pass
L2 = 2 << 20


def read_db(path):
    data, out = open(path, "rb").read(), {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def where(name):
    return os.path.join(SRC if name in ("db", "db_ss", "profile_0", "profile_0_ss") else GOLD, name)


@functools.lru_cache(maxsize=None)
def manifest():
    return json.load(open(os.path.join(GOLD, "MANIFEST.json")))


def flag(par, name):
    return par[par.index(name) + 1]


def padded(t3, tA=None):
    keys = sorted(t3)
    lens = np.array([len(t3[k]) for k in keys], np.int32)
    off = np.zeros(len(keys) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
    for i, k in enumerate(keys):
        d3[off[i]:off[i] + lens[i]] = t3[k]
        da[off[i]:off[i] + lens[i]] = t3[k] if tA is None else tA[k]
    return keys, synth.PaddedDB(d3, da, off, lens)


def seq_db(name):
    return {k: np.array([LETTERS.index(chr(c).upper()) for c in v.rstrip(b"\n")], np.uint8) for k, v in read_db(where(name)).items()}


_CTX = {}


def context(target, spaced, kmer_thr=0):
    """one context per (target database, pattern, index threshold), kept for the module"""
    key = (target, spaced, kmer_thr)
    if key not in _CTX:
        keys, db = padded(seq_db(target), seq_db("db") if target == "db_ss" else None)
        ctx = api.Context(0)
        ctx.load_db(db)
        ctx.kmer_index_build(api.Matrix(0, 8.0, -0.2), kmer_thr=kmer_thr, spaced=spaced)
        _CTX[key] = (ctx, keys)
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for ctx, _ in _CTX.values():
        ctx.close()
    _CTX.clear()


def prepare(entries, thr, spaced):
    return [api.kmer_query_prepare_profile(e, thr, 6, spaced) for e in entries]


def check_lists(ctx, entries, thr, spaced, content_every, always=()):
    """every window of every query: K against the model's count; the list against the model's for every `content_every`-th window, for the queries in
    `always` and for every list of at most 64 k-mers"""
    nwin = checked = 0
    for q, e in enumerate(entries):
        s, l = km.sort_rows(km.raw_scores(e))
        t = km.window_threshold(thr)
        for start, has_x in km.windows(km.letters(e), spaced):
            rows_s, rows_l = km.position_rows(s, l, start, spaced)
            want_k = 0 if has_x else min(km.count_ge(rows_s, t), km.CAP)
            nwin += 1
            if q in always or nwin % content_every == 0 or want_k <= 64:
                k, got = ctx.kmer_profile_list(q, start)
                assert k == want_k, (q, start, k, want_k)
                want = km.generate_lex(rows_s, rows_l, t) if want_k else np.zeros(0, np.int64)
                assert len(got) == len(want) and (got.astype(np.int64) == want).all(), (q, start)
                checked += 1
            else:
                k, _ = ctx.kmer_profile_list(q, start, cap=0)
                assert k == want_k, (q, start, k, want_k)
        with pytest.raises(api.FsgpuError):
            ctx.kmer_profile_list(q, max(0, len(km.letters(e)) - km.pattern_size(spaced) + 1))          # one past the last window
    return nwin, checked


# ---- 1. lists against the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spaced", [1, 0])
def test_lists_of_the_crafted_queries(spaced):
    ctx, _ = context("ktarget_ss", spaced)
    db = read_db(where("kprof_ss"))
    entries = [db[k] for k in sorted(db)]
    note = manifest()["crafted"]["kprof_ss"]
    flat = [int(k) for k, v in note.items() if v.startswith("flat")]
    special = [int(k) for k, v in note.items() if v.startswith("length") or v.startswith("rows at") or v.startswith("two-valued")]
    res, status = ctx.kmer_search_profile(prepare(entries, 75, spaced), max_res=1000, min_diag=30, l2_cache_size=L2)
    assert (status == 0).all()
    # the flat query's windows are capped: one is read in full (8 388 607 k-mers), the others by count
    nwin, checked = check_lists(ctx, entries, 75, spaced, 29 if spaced else 61, always=set(special if spaced else special[:6]))
    k, got = ctx.kmer_profile_list(flat[0], 0)
    s, l = km.sort_rows(km.raw_scores(entries[flat[0]]))
    assert k == km.CAP and (got.astype(np.int64) == km.generate_lex(*km.position_rows(s, l, 0, spaced), 75)).all()
    assert nwin > 500 and checked > 40
    assert int(ctx.kmer_counts()[0]) == sum(min(km.count_ge(km.position_rows(*km.sort_rows(km.raw_scores(e)), st, spaced)[0], 75), km.CAP)
                                            for e in entries for st, x in km.windows(km.letters(e), spaced) if not x)


def test_lists_of_a_seeded_batch_of_short_profiles():
    ctx, _ = context("ktarget_ss", 1)
    rng = np.random.default_rng(20261104)
    entries = []
    for q in range(32):
        L = int(rng.integers(10, 61))
        codes = rng.integers(0, 20, L)
        sc = np.full((20, L), -50) + rng.integers(-10, 11, (20, L))
        sc[codes, np.arange(L)] = 45 + rng.integers(-10, 11, L)
        sc[:, rng.random(L) < 0.1] = rng.choice(np.array([-128, 127]), 20)[:, None]          # a tenth of the positions at the extremes
        codes[rng.random(L) < 0.03] = 20                                                     # and a few X query letters
        entries.append(pm.encode(np.clip(sc, -128, 127).astype(np.int8), codes))
    for thr in (110, 75):
        _, status = ctx.kmer_search_profile(prepare(entries, thr, 1), l2_cache_size=L2)
        assert (status == 0).all()
        nwin, checked = check_lists(ctx, entries, thr, 1, 5 if thr == 110 else 37)
        assert nwin == sum(len(e) // 25 - 9 for e in entries) and checked > 30


def crafted_single(rows_vals, seed, spaced):
    """one window: row i of the window holds rows_vals[i] on seeded letters and -128 elsewhere"""
    rng = np.random.default_rng(seed)
    L = km.pattern_size(spaced)
    sc = np.full((20, L), -128)
    for i, o in enumerate(km.pattern(spaced)):
        sc[rng.permutation(20)[:len(rows_vals[i])], o] = rows_vals[i]
    return pm.encode(sc.astype(np.int8), rng.integers(0, 20, L))


SIZED = {   # list size -> (viable scores per row, threshold): found by search, asserted through the model below
    8191: ([[5, 2, 2, 1], [5, 3, 2, 0], [4, 3, 2, 0], [5, 5, 4, 2], [5, 4, 4, 4, 3, 2, 2, 0], [5, 2, 1, 0]], 4),
    8192: ([[4, 4, 3, 2, 2, 2, 2, 1], [5, 4, 3, 1], [3, 2, 2, 0], [5, 4, 4, 3, 2, 0, 0, 0], [5, 5, 1, 0], [5, 2]], 4),
    8193: ([[4, 3, 3, 2, 2, 1, 0], [5, 3, 3, 2, 1, 1, 0], [5, 5, 5, 2], [5, 5, 5, 3, 3, 2, 1, 0], [5, 4, 2], [4, 2, 0]], 17),
}


@pytest.mark.parametrize("spaced", [1, 0])
def test_lists_at_the_edges_of_size_and_threshold(spaced):
    """an empty, a one-element and a capped list; lists of exactly one slice of the list pass, one more and one fewer; a negative and a huge kmerThr"""
    ctx, _ = context("ktarget_ss", spaced)
    for size, (vals, thr) in SIZED.items():
        e = crafted_single(vals, size, spaced)
        s, l = km.sort_rows(km.raw_scores(e))
        assert km.count_ge(km.position_rows(s, l, 0, spaced)[0], thr) == size and size in (SLICE - 1, SLICE, SLICE + 1)
        # alone, and behind a query whose lists shift the slice grid
        for entries in ([e], [crafted_single(SIZED[8193][0], 77, spaced), e, e]):
            _, status = ctx.kmer_search_profile(prepare(entries, thr, spaced), l2_cache_size=L2)
            assert (status == 0).all()
            check_lists(ctx, entries, thr, spaced, 1)
    one = crafted_single([[9, 3], [9, 1], [9], [9, 8], [9], [9, 0]], 5, spaced)
    flat = pm.encode(np.full((20, km.pattern_size(spaced)), -3, np.int8), np.zeros(km.pattern_size(spaced), np.uint8))
    for thr, sizes in ((54, (1, 0)), (55, (0, 0)), (0, (16, 0)), (-7, (16, 0)), (1000, (0, 0)), (30000, (0, 0)), (32767, (0, 0))):
        _, status = ctx.kmer_search_profile(prepare([one, flat], thr, spaced), l2_cache_size=L2)
        check_lists(ctx, [one, flat], thr, spaced, 1)
        assert [ctx.kmer_profile_list(q, 0, cap=0)[0] for q in (0, 1)] == list(sizes), thr
    # all scores equal and negative: nothing at thr 0; all equal at 0: everything, capped
    zero = pm.encode(np.zeros((20, km.pattern_size(spaced)), np.int8), np.zeros(km.pattern_size(spaced), np.uint8))
    ctx.kmer_search_profile(prepare([zero], -1, spaced), l2_cache_size=L2)
    check_lists(ctx, [zero], -1, spaced, 1)
    assert ctx.kmer_profile_list(0, 0, cap=0)[0] == km.CAP


@pytest.mark.parametrize("spaced", [1, 0])
def test_an_x_at_every_pattern_offset(spaced):
    ctx, _ = context("ktarget_ss", spaced)
    db = read_db(where("ksmall_ss"))
    entries = [db[k] for k in sorted(db)]
    for thr in (75, -5):
        ctx.kmer_search_profile(prepare(entries, thr, spaced), l2_cache_size=L2)
        nwin, checked = check_lists(ctx, entries, thr, spaced, 1 if thr == 75 else 5)
        assert nwin == sum(max(0, len(e) // 25 - km.pattern_size(spaced) + 1) for e in entries)
    skipped = sum(x for e in entries for _, x in km.windows(km.letters(e), spaced))
    # spaced: the one window of the six queries whose X sits on a used offset; contiguous: offset o lies in min(o, 9 - o, 4) + 1 of the five windows
    assert skipped == (6 if spaced else sum(min(o, 9 - o, 4) + 1 for o in range(10))) and (spaced or skipped == 30)


# ---- 2. end to end against the frozen reference records -------------------------------------------------------------------------------------------
def frozen(name):
    return {k: [tuple(int(x) for x in l.split("\t")) for l in v.decode().splitlines()] for k, v in read_db(where(name)).items()}


def run_search(ctx, entries, r, one_by_one=False):
    par = r["parameters"]
    spaced = int(flag(par, "--spaced-kmer-mode"))
    kw = dict(max_res=int(flag(par, "--max-seqs")), min_diag=int(flag(par, "--min-ungapped-score")), kmer_score_only=flag(par, "--diag-score") == "0",
              l2_cache_size=L2)
    prep = prepare(entries, r["kmer_threshold"], spaced)
    if not one_by_one:
        return ctx.kmer_search_profile(prep, **kw)
    out = [ctx.kmer_search_profile([p], **kw) for p in prep]
    return [o[0][0] for o in out], np.array([o[1][0] for o in out])


@pytest.mark.parametrize("name", sorted(manifest()["runs"]) if os.path.exists(os.path.join(GOLD, "MANIFEST.json")) else [])
def test_search_equals_every_frozen_record(name):
    r = manifest()["runs"][name]
    qdb, tdb = r["positional"]
    spaced = int(flag(r["parameters"], "--spaced-kmer-mode"))
    ctx, keys = context(tdb, spaced)
    db = read_db(where(qdb))
    qkeys = sorted(db)
    want = frozen(name)
    assert sum(len(v) for v in want.values()) == r["lines"]
    for one_by_one in ((False, True) if name.startswith("c_") else (False,)):
        res, status = run_search(ctx, [db[k] for k in qkeys], r, one_by_one)
        assert (status == 0).all(), status
        for k, hits in zip(qkeys, res):
            got = [(keys[int(h["id"])], int(h["score"]), int(np.int16(h["diag"]))) for h in hits]
            assert got == want[k], (name, k, one_by_one)
    if not r["expect_empty"]:
        assert sum(len(h) for h in res) > 0


# ---- 3. contract edges ---------------------------------------------------------------------------------------------------------------------------
def test_an_index_with_a_kmer_threshold_is_refused():
    ctx, _ = context("db_ss", 1, kmer_thr=78)
    e = read_db(where("profile_0_ss"))[0]
    with pytest.raises(api.FsgpuError) as err:
        ctx.kmer_search_profile(prepare([e], 75, 1))
    assert "Prefiltering.cpp:555" in str(err.value) and "78" in str(err.value) and getattr(err.value, "rc", api.FSGPU_E_ARG) == api.FSGPU_E_ARG
    # the context still serves sequence queries
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    res, status = ctx.kmer_search([api.kmer_query_prepare(m8, m2, seq_db("db_ss")[0])], l2_cache_size=L2)
    assert status[0] == 0 and len(res[0]) > 0


def test_sequence_calls_between_profile_calls_a_clone_and_empty_input():
    ctx, keys = context("ktarget_ss", 1)
    db = read_db(where("kprof_ss"))
    entries = [db[k] for k in sorted(db)][:8]
    prep = prepare(entries, 75, 1)
    first, st1 = ctx.kmer_search_profile(prep, l2_cache_size=L2)
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    targets = seq_db("ktarget_ss")
    sq = [api.kmer_query_prepare(m8, m2, targets[k], kmer_thr=78) for k in (0, 10, 11)]
    seq1, sst1 = ctx.kmer_search(sq, l2_cache_size=L2)
    with pytest.raises(api.FsgpuError):                                    # the last batch was a sequence batch: nothing to inspect
        ctx.kmer_profile_list(0, 0)
    second, st2 = ctx.kmer_search_profile(prep, l2_cache_size=L2)
    seq2, sst2 = ctx.kmer_search(sq, l2_cache_size=L2)
    assert (st1 == 0).all() and (st2 == 0).all() and (sst1 == sst2).all()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)) and all(a.tobytes() == b.tobytes() for a, b in zip(seq1, seq2))
    assert all(len(a) for a in seq1)
    want = frozen("c_s95")
    assert [[(keys[int(h["id"])], int(h["score"]), int(np.int16(h["diag"]))) for h in hits] for hits in second] == [want[k] for k in sorted(db)[:8]]
    clone = ctx.clone()
    try:
        third, st3 = clone.kmer_search_profile(prep, l2_cache_size=L2)
        assert (st3 == 0).all() and all(a.tobytes() == b.tobytes() for a, b in zip(first, third))
        k, got = clone.kmer_profile_list(0, 0)
        s0, l0 = km.sort_rows(km.raw_scores(entries[0]))
        assert k == len(got) > 0 and (got.astype(np.int64) == km.generate_lex(*km.position_rows(s0, l0, 0, 1), 75)).all()
        with pytest.raises(api.FsgpuError):                                # the clone's batch is the clone's: this context's last one was a sequence batch
            ctx.kmer_profile_list(0, 0)
    finally:
        clone.close()
    # nq = 0, and queries of no position among others
    res, status = ctx.kmer_search_profile([], l2_cache_size=L2)
    assert res == [] and len(status) == 0
    empty = (np.zeros(0, np.uint8), np.zeros((0, 20), np.int8), np.zeros((0, 21), np.int8), 75)
    res, status = ctx.kmer_search_profile([empty, prep[0], empty], l2_cache_size=L2)
    assert (status == 0).all() and len(res[0]) == 0 and len(res[2]) == 0 and res[1].tobytes() == first[0].tobytes()
    res, status = ctx.kmer_search_profile([empty], l2_cache_size=L2)
    assert status[0] == 0 and len(res[0]) == 0
    assert api.lib().fsgpu_kmer_batch_hint(ctx.h) >= 32 and len(ctx.kmer_stage_ms()) == 11 and ctx.kmer_stage_ms()[0] >= 0


# ---- 4. the fused per-batch body on the 12 structures ---------------------------------------------------------------------------------------------
def test_the_fused_batch_body_on_the_example_structures():
    ctx, keys = context("db_ss", 1)
    par = api.default_params()
    par.minDiagScoreThr, par.maxResListLen, par.evalThr, par.addBacktrace, par.alignmentType = 30, 1000, 10.0, 1, 2
    s = api.Search(ctx, par, keys=np.array(keys, np.uint32))
    try:
        pA, p3 = read_db(where("profile_0")), read_db(where("profile_0_ss"))
        qkeys = sorted(p3)
        r = manifest()["runs"]["e_s95"]
        out = s.kmer_batch_profile([(pA[k], p3[k]) for k in qkeys], r["kmer_threshold"], 1, max_res=1000, min_diag=30)
        want = frozen("e_s95")
        lists = []
        for i, k in enumerate(qkeys):
            hits = out["hits"][i, :out["nhits"][i]]
            assert out["status"][i] == 0
            assert [(keys[int(h["id"])], int(h["score"]), int(np.int16(h["diag"]))) for h in hits] == want[k], k
            assert (out["kept"][i, :out["nkept"][i]] == hits["id"]).all()                     # no coverage threshold: every hit goes to the aligner
            lists.append(hits["id"].astype(np.uint32).copy())
        fused = [out["results"][i, :out["nres"][i]].copy() for i in range(len(qkeys))]
        res, _ = s.align_batch_profile([(pA[k], p3[k]) for k in qkeys], lists)
        assert sum(len(x) for x in res) > 12
        for i in range(len(qkeys)):
            assert len(res[i]) == len(fused[i])
            for f in ("dbKey", "score", "qStartPos", "qEndPos", "qLen", "dbStartPos", "dbEndPos", "dbLen", "eval"):
                assert (res[i][f] == fused[i][f]).all(), (i, f)
        with pytest.raises(api.FsgpuError) as err:
            s.kmer_batch_profile([(pA[qkeys[0]], p3[qkeys[0]])], 75, 0)
        assert "spaced = 0" in str(err.value) and "spaced = 1" in str(err.value)
    finally:
        s.close()

"""The device k-mer prefilter at EVERY index parameter against the C oracle (oracle/fs_kmer_oracle.c, pinned to the compiled reference at these very
settings by tests/test_kmer_params_model.py): spaced / contiguous k-mers, lower-case masking on / off, repeat limits 0, 1, 2, 6 and 50, all three
off, contiguous k-mers at threshold 110 (tests/kmer_param_cases.py: 622 targets, 13 queries).  Everything is compared for exact equality.

* per setting: the whole index in reference order, the masked lookup of every target, statistics and complete hit lists at three search settings
  (defaults, --max-seqs 50 with databaseHits refills, --diag-score 0); with contiguous k-mers also both forced forms of the similar-k-mer passes and
  two levels of the hit-stream partition
* one context rebuilt default -> contiguous -> repeat limit 1 -> default, and a clone that keeps the index it was taken with
* Search.kmer_batch (fshost_search_kmer_batch) against its parts: Context.kmer_search, Util::canBeCovered restated in numpy, Search.align_batch
* fshost_search_kmer_batch refuses a `spaced` that is not the resident index's (fsgpu_kmer_index_get_params)"""
import ctypes as C

import numpy as np
import pytest

import kmer_param_cases as P
from foldseek_amd import api

pytestmark = pytest.mark.gpu

CONTIGUOUS = ("contiguous", "alloff")          # the settings whose pattern is 6 residues long and that get the forced-form runs


@pytest.fixture(scope="module")
def worlds():
    """name -> (context with the database and that setting's index, the oracle's answers per search setting, the oracle); built on first use, kept
    for the module: an index is half a GiB of HBM, all nine stay far below one card"""
    w = P.world()
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    ksub, _, usub = P.matrices()
    assert (m8.scores().ravel() == ksub).all() and (m2.scores().ravel() == usub).all()
    made = {}

    def get(name):
        if name not in made:
            o = P.make_oracle(name)
            ctx = api.Context(0)
            ctx.load_db(w.db)
            build(ctx, name)
            made[name] = dict(ctx=ctx, o=o, answers={s: P.oracle_answers(o, name, s) for s in P.SEARCHES})
        return made[name]

    def build(ctx, name):
        ip = P.index_params(name)
        ctx.kmer_index_build(m8, kmer_thr=ip["kmerThr"], spaced=ip["spaced"], mask_lower_case=ip["maskLowerCase"], mask_n_repeats=ip["maskNrepeats"])

    def prepare(name, queries=None):
        ip = P.index_params(name)
        return [api.kmer_query_prepare(m8, m2, q, comp_bias=True, scale=0.15, kmer_thr=ip["kmerThr"], spaced=ip["spaced"]) for q in (w.queries if queries is None else queries)]

    def search(ctx, name, which, **kw):
        sp = P.search_params(name, which)
        return ctx.kmer_search(prepare(name), identity=w.identity, max_res=sp["maxResListLen"], min_diag=sp["minDiagScoreThr"], bins=sp["bins"],
                               max_db_matches=sp["maxDbMatches"], found_diagonals_size=sp["foundDiagonalsSize"], l2_cache_size=2 * 1024 * 1024,
                               kmer_score_only=bool(sp["noDiagScore"]), want_stats=True, **kw)

    yield dict(w=w, m8=m8, m2=m2, get=get, build=build, prepare=prepare, search=search)
    for v in made.values():
        v["o"].close()
        v["ctx"].close()


@pytest.fixture
def x(worlds, name):
    """the world of the test's setting; built here, so that a test's own time is what it compares"""
    return worlds["get"](name)


def _check(w, res, status, stats, answers, where):
    """status 0, statistics and complete hit lists of every query equal the oracle's; the query without residues has no hit"""
    for qi, (want, st, _) in enumerate(answers):
        if want is None:
            assert len(res[qi]) == 0, (where, w.qnames[qi])
            continue
        assert status[qi] == 0, (where, w.qnames[qi], status[qi])
        assert len(res[qi]) == len(want) and (res[qi] == want).all(), (where, w.qnames[qi], len(res[qi]), len(want))
        if stats is not None:
            assert np.allclose(stats[qi], st, rtol=0, atol=0, equal_nan=True), (where, w.qnames[qi], stats[qi], st)


def _check_segments(seg, nq):
    assert seg[1] == seg[4] and seg[4] % seg[5] == 0 and seg[4] // seg[5] >= nq and 1 <= seg[6] <= 65536, seg


@pytest.mark.parametrize("name", P.NAMES)
def test_index_equals_oracle(worlds, x, name):
    w = worlds["w"]
    ctx, o = x["ctx"], x["o"]
    assert ctx.kmer_index_params() == P.index_params(name)
    ooff, oseq, opos = o.index()
    off, seq, pos, msk = ctx.kmer_index_reference_order(w.db.data3di.size)
    print(f"{name}: {ctx.kmer_index_entries} index entries on the device, {int(ooff[-1])} in the oracle")
    assert ctx.kmer_index_entries == int(ooff[-1]) > 0 and ctx.kmer_index_entry_bytes == 4           # 10 id bits + 9 position bits
    assert (off == ooff).all()
    assert len(seq) == len(oseq) and (seq == oseq).all() and (pos == opos).all()
    for i in range(w.db.n):
        L, a = int(w.db.lengths[i]), int(w.db.offsets[i])
        assert (msk[a:a + L] == o.masked(i, L)).all(), (name, i)
        assert (msk[a + L:int(w.db.offsets[i + 1])] == P.X).all(), (name, i)                          # the padding behind an entry stays X


@pytest.mark.parametrize("which", tuple(P.SEARCHES))
@pytest.mark.parametrize("name", P.NAMES)
def test_hits_equal_oracle(worlds, x, name, which):
    w = worlds["w"]
    res, status, stats = worlds["search"](x["ctx"], name, which)
    _check(w, res, status, stats, x["answers"][which], (name, which))
    _check_segments(x["ctx"].kmer_segments(), sum(1 for q in w.queries if len(q)))
    if which == "refill":
        assert max(r for _, _, r in x["answers"][which]) > 0 and stats[:, 2].sum() > 0              # refills happened, in the oracle and on the device


@pytest.mark.parametrize("name", CONTIGUOUS)
def test_forced_forms_and_bin_levels_with_contiguous_kmers(worlds, x, name, monkeypatch):
    """every search kernel takes the pattern by value: the workgroup and the wave form of k_kmer_count / k_kmer_lists, and two granularities of the
    hit-stream partition, with a pattern of 6 residues"""
    w = worlds["w"]
    ctx = x["ctx"]
    nq = sum(1 for q in w.queries if len(q))
    forms = {}
    for form in ("0", "1"):
        monkeypatch.setenv("FSGPU_KMER_WAVE", form)
        for which in P.SEARCHES:
            res, status, stats = worlds["search"](ctx, name, which)
            _check(w, res, status, stats, x["answers"][which], (name, which, "wave", form))
        h = ctx.history_counters()
        forms[form] = (h["kmer_count_form"], h["kmer_list_form"])
    monkeypatch.delenv("FSGPU_KMER_WAVE")
    assert forms == {"0": (1, 1), "1": (2, 2)}, forms
    for level in ("0", "2"):
        monkeypatch.setenv("FSGPU_KMER_BIN_LEVEL", level)
        for which in ("defaults", "refill"):
            res, status, stats = worlds["search"](ctx, name, which)
            _check(w, res, status, stats, x["answers"][which], (name, which, "level", level))
            _check_segments(ctx.kmer_segments(), nq)
    monkeypatch.delenv("FSGPU_KMER_BIN_LEVEL")


def test_rebuild_on_one_context_and_a_clone_keeps_its_index(worlds):
    """default -> contiguous -> repeat limit 1 -> default on ONE context: after each build the hits are that setting's; the first and the last index
    agree byte for byte; a clone taken under the contiguous index answers with it after the parent went on (the snapshot rule of include/fsgpu.h)"""
    w = worlds["w"]
    ctx = api.Context(0)
    ctx.load_db(w.db)
    clone = None
    try:
        copies = []
        for step, name in enumerate(("default", "contiguous", "rep1", "default")):
            worlds["build"](ctx, name)
            assert ctx.kmer_index_params() == P.index_params(name)
            res, status, stats = worlds["search"](ctx, name, "defaults")
            _check(w, res, status, stats, worlds["get"](name)["answers"]["defaults"], (step, name))
            if name == "default":
                copies.append(ctx.kmer_index_copy(w.db.data3di.size))
            if name == "contiguous":
                clone = ctx.clone()
            if clone is not None:
                assert clone.kmer_index_params() == P.index_params("contiguous")
                assert clone.kmer_index_entries == worlds["get"]("contiguous")["ctx"].kmer_index_entries
                res, status, stats = worlds["search"](clone, "contiguous", "defaults")
                _check(w, res, status, stats, worlds["get"]("contiguous")["answers"]["defaults"], (step, name, "clone"))
        for a, b in zip(*copies):
            assert a.tobytes() == b.tobytes()
        assert ctx.kmer_index_entries == worlds["get"]("default")["ctx"].kmer_index_entries != clone.kmer_index_entries
    finally:
        if clone is not None:
            clone.close()
        ctx.close()


# ---- Search.kmer_batch ------------------------------------------------------------------------------------------------------------------
def _batch_inputs(w):
    """the queries as fshost_search_kmer_batch takes them: plain codes (the aligner reads them too), the one without residues as a null pointer"""
    q3 = [np.ascontiguousarray(q % 32, np.uint8) for q in w.queries]
    qa = [np.ascontiguousarray(q % 32, np.uint8) for q in w.queries_aa]
    p3 = np.array([q.ctypes.data if len(q) else 0 for q in q3], np.uint64)
    pa = np.array([q.ctypes.data if len(q) else 0 for q in qa], np.uint64)
    return q3, qa, p3, pa, np.array([len(q) for q in q3], np.int32)


def _can_be_covered(thr, mode, q, t):
    """Util::canBeCovered (Util.cpp:542-559) over float32, as the reference computes it"""
    q, t, thr = np.float32(q), t.astype(np.float32), np.float32(thr)
    if mode == 0:
        return (q / t >= thr) & (t / q >= thr)
    if mode == 2:
        return t / q >= thr
    if mode == 5:
        return np.minimum(t, q) / np.maximum(t, q) >= thr
    raise AssertionError(mode)


MAX_RES = 200


@pytest.mark.parametrize("cov", [(0.0, 0), (0.7, 0), (0.7, 2), (0.7, 5)], ids=lambda c: f"cov{c[0]}mode{c[1]}")
@pytest.mark.parametrize("name", ["default", "contiguous"])
def test_search_kmer_batch_equals_its_parts(worlds, x, name, cov):
    w = worlds["w"]
    ctx, ip = x["ctx"], P.index_params(name)
    q3, qa, p3, pa, lens = _batch_inputs(w)
    nq = len(q3)
    par = api.default_params()
    par.covThr, par.covMode = cov
    s = api.Search(ctx, par)
    try:
        out = s.kmer_batch(worlds["m8"], worlds["m2"], ip["kmerThr"], ip["spaced"], pa, p3, lens, pref_identity=w.identity, aln_identity=w.identity,
                           max_res=MAX_RES, rows=nq + 1)
        # the prefilter: a direct search of the same queries with the same settings
        res, status = ctx.kmer_search(worlds["prepare"](name, q3), identity=w.identity, max_res=MAX_RES, min_diag=30)
        want_kept = []
        for k in range(nq):
            assert out["status"][k] == status[k] == 0 and out["nhits"][k] == len(res[k]), (k, out["status"][k], out["nhits"][k], len(res[k]))
            assert (out["hits"][k, :len(res[k])] == res[k]).all(), k
            ids = res[k]["id"]
            keep = ids if cov[0] == 0 else ids[_can_be_covered(cov[0], cov[1], lens[k], w.db.lengths[ids])] if len(ids) else ids
            want_kept.append(np.asarray(keep, np.uint32))
            assert out["nkept"][k] == len(keep) and (out["kept"][k, :len(keep)] == keep).all(), (k, cov)
        if cov[0] > 0:
            assert sum(len(a) for a in want_kept) < sum(len(r) for r in res)                     # the coverage filter really dropped hits
        assert sum(len(a) for a in want_kept) > 0
        # the alignment: align_batch over the queries that kept a hit, in their order
        live = [k for k in range(nq) if len(want_kept[k]) and lens[k] > 0]
        aligned = s.align_batch([qa[k] for k in live], [q3[k] for k in live], [want_kept[k] for k in live], identity=w.identity[live])
        total = 0
        for k in range(nq):
            a = aligned[live.index(k)] if k in live else np.zeros(0, api.RESULT_DT)
            assert out["nres"][k] == len(a), (k, out["nres"][k], len(a))
            assert out["results"][k, :len(a)].tobytes() == a.tobytes(), k
            total += len(a)
        assert total > 0
        # a query without residues and a query without a hit: no result, and nothing written into their rows or behind the last one
        canary = lambda a: (a.view(np.uint8) == 0xA5).all()
        for k in (w.qnames.index("prefix0"), w.qnames.index("allx")):
            assert out["nhits"][k] == 0 and out["nkept"][k] == 0 and out["nres"][k] == 0, k
            assert canary(out["results"][k]) and canary(out["kept"][k]), k
        assert w.qnames[-2] == "allx" and canary(out["results"][nq]) and canary(out["kept"][nq]) and canary(out["hits"][nq])
        assert canary(out["nres"][nq:]) and canary(out["nkept"][nq:]) and canary(out["nhits"][nq:]) and canary(out["status"][nq:])
        for k in range(nq):                                                                       # ... nor behind a query's own results
            assert canary(out["results"][k, out["nres"][k]:]) or k in live, k
            assert canary(out["kept"][k, out["nkept"][k]:]), k
    finally:
        s.close()


@pytest.mark.parametrize("name,other", [("contiguous", "default"), ("default", "contiguous")])
def test_search_kmer_batch_refuses_another_pattern_than_the_index(worlds, x, name, other):
    """the host prepares L - patternSize + 1 thresholds and the device reads as many as ITS pattern gives: a `spaced` that is not the resident index's
    is refused before anything is prepared or launched, with both values in the message; the next call with the index's own value is correct"""
    w = worlds["w"]
    ctx, ip, op = x["ctx"], P.index_params(name), P.index_params(other)
    q3, qa, p3, pa, lens = _batch_inputs(w)
    s = api.Search(ctx)
    try:
        with pytest.raises(api.FsgpuError) as e:
            s.kmer_batch(worlds["m8"], worlds["m2"], ip["kmerThr"], op["spaced"], pa, p3, lens, pref_identity=w.identity, aln_identity=w.identity, max_res=MAX_RES)
        msg = str(e.value)
        assert "rc=-1" in msg and f"spaced = {op['spaced']} " in msg and f"built with spaced = {ip['spaced']}" in msg, msg
        out = s.kmer_batch(worlds["m8"], worlds["m2"], ip["kmerThr"], ip["spaced"], pa, p3, lens, pref_identity=w.identity, aln_identity=w.identity, max_res=MAX_RES)
        res, status = ctx.kmer_search(worlds["prepare"](name, q3), identity=w.identity, max_res=MAX_RES, min_diag=30)
        for k in range(len(q3)):
            assert out["status"][k] == status[k] == 0 and out["nhits"][k] == len(res[k]) and (out["hits"][k, :len(res[k])] == res[k]).all(), k
        assert out["nres"].sum() > 0
    finally:
        s.close()


def test_index_params_without_an_index():
    ctx = api.Context(0)
    try:
        ctx.load_db(P.world().db)
        with pytest.raises(api.FsgpuError):
            ctx.kmer_index_params()
        p = api.KmerIndexParams(-7, -7, -7, -7, -7)
        assert api.lib().fsgpu_kmer_index_get_params(ctx.h, C.byref(p)) == -3 and p.spaced == -7          # FSGPU_E_NODB, *out untouched
        assert api.lib().fsgpu_kmer_index_get_params(ctx.h, None) == -1 and api.lib().fsgpu_kmer_index_get_params(None, C.byref(p)) == -1
    finally:
        ctx.close()

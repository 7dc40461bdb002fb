"""The k-mer prefilter's checkers at EVERY index parameter (no GPU): spaced / contiguous k-mers, lower-case masking on / off, repeat limits 0, 1, 2, 6
and 50, all three off, and contiguous k-mers at a high threshold (tests/kmer_param_cases.py).

* Counted conditions on the inputs, so that no axis is vacuous: every setting changes the index and at least one full query's hit list, the hand-made
  runs are masked exactly where the rule says, the short windows are hits only with contiguous k-mers, the soft-masked homolog only without
  lower-case masking, every index has a search setting with databaseHits refills, and no query takes the oracle's unmodelled std::sort branch.
* oracle/fs_kmer_oracle.c against the reference's own classes compiled into oracle/_ref, at every setting: offsets table, every entry, the masked
  lookup of every target, complete hit lists (ids, scores, diagonals, order) and statistics at three search settings.  tests/test_kmer_params_gpu.py
  holds the device to the oracle at these settings; the oracle is only as good as this pin.  Skipped where oracle/_ref could not be built.
* fshost_kmer_query_prepare with spaced = 0 against the threshold rule restated in numpy over the oracle's composition bias."""
import numpy as np
import pytest

import helpers as H
import kmer_lib as K
import kmer_param_cases as P
from foldseek_amd import api


@pytest.fixture(scope="module")
def model():
    """per setting: the oracle, its entry count, its masked lookup and its answers at every search setting"""
    w = P.world()
    m = {}
    for name in P.NAMES:
        o = P.make_oracle(name)
        m[name] = dict(o=o, entries=int(o.offsets()[-1]), masked=[o.masked(i, len(t)) for i, t in enumerate(w.targets)],
                       answers={s: P.oracle_answers(o, name, s) for s in P.SEARCHES})
    yield m
    for v in m.values():
        v["o"].close()


def _same(a, b):
    return len(a) == len(b) and bool((a == b).all())


def _hit_of(model, name, target):
    """the queries whose default-search hit list at a setting holds a target"""
    return [qi for qi, (r, _, _) in enumerate(model[name]["answers"]["defaults"]) if r is not None and target in r["id"]]


def test_every_setting_changes_the_index_and_the_hits(model):
    base = model["default"]
    for name in P.NAMES[1:]:
        m = model[name]
        changed = [qi for qi in range(4) if not _same(m["answers"]["defaults"][qi][0], base["answers"]["defaults"][qi][0])]
        print(f"{name}: {m['entries']} index entries (default {base['entries']}), full queries with another hit list: {changed}")
        assert m["entries"] != base["entries"], name
        assert changed, name
    for name in P.NAMES:
        refills = [r for _, _, r in model[name]["answers"]["refill"]]
        print(f"{name}: databaseHits refills per query at maxDbMatches = {P.REFILL_MATCHES[name]}: {refills}")
        assert max(refills) > 0, name
        assert all(r == 0 for _, _, r in model[name]["answers"]["defaults"]), name
        assert sum(len(r) for r, _, _ in model[name]["answers"]["scoreonly"] if r is not None) > 0, name


def test_runs_are_masked_where_the_rule_says(model):
    w = P.world()
    counted = {}
    for name in P.NAMES:
        ip = P.index_params(name)
        kept = masked = 0
        for run in w.runs:
            got = model[name]["masked"][run.id][run.start:run.start + run.length]
            raw = w.targets[run.id][run.start:run.start + run.length]
            if P.run_masked(run, ip["maskNrepeats"]):
                assert (got == P.X).all(), (name, run)
                masked += 1
            else:
                want = np.where((raw >= 32) & (ip["maskLowerCase"] != 0), P.X, raw % 32)       # only the soft-masked part of a border run goes
                assert (got == want).all(), (name, run, got)
                kept += 1
        counted[name] = (kept, masked)
        x = model[name]["masked"][w.ids["xrun"]]
        assert (x == P.X).sum() == 8, name                                                     # the run of X stays X and takes nothing with it
    print("runs kept / masked per setting:", counted)
    # the conditions by name: at its own limit each n-run survives, each n + 1-run is X; the leading run of code 0 survives; c | c + 32 is one run
    for n, name in ((1, "rep1"), (2, "rep2"), (6, "default")):
        mine = [r for r in w.runs if r.id in (w.ids[f"run{n}a"], w.ids[f"run{n}b"])]
        assert sorted(r.length for r in mine) == [n] * 3 + [n + 1] * 3
        assert {r.start == 0 for r in mine if r.length == n} == {True, False} and {r.start == 0 for r in mine if r.length == n + 1} == {True, False}
        for r in mine:
            assert (model[name]["masked"][r.id][r.start:r.start + r.length] == P.X).all() == (r.length == n + 1), (name, r)
        b = next(r for r in w.runs if r.id == w.ids[f"border{n}"])
        raw = w.targets[b.id][b.start:b.start + b.length]
        assert (raw < 32).any() and (raw >= 32).any() and (raw < 32).sum() <= n and (raw >= 32).sum() <= n      # neither part passes the limit alone
        assert (model[name]["masked"][b.id][b.start:b.start + b.length] == P.X).all(), (name, b)
    zero = model["default"]["masked"][w.ids["zero"]]
    lead, mid = [r for r in w.runs if r.id == w.ids["zero"]]
    assert lead.leading_zero and (zero[:8] == 0).all() and (zero[mid.start:mid.start + 8] == P.X).all()
    nolc = model["nomasklc"]["masked"][w.ids["border6"]]
    b = next(r for r in w.runs if r.id == w.ids["border6"])
    assert (nolc[b.start:b.start + b.length] == P.X).all()          # masked by the repeat rule alone: lower-case masking is off here


def test_short_windows_and_the_soft_masked_homolog(model):
    w = P.world()
    seen = {}
    for name in P.NAMES:
        ip = P.index_params(name)
        wins = {k: _hit_of(model, name, w.ids[f"win{k}"]) for k in P.WINDOWS}
        soft = _hit_of(model, name, w.ids["softhom"])
        seen[name] = ({k: v for k, v in wins.items() if v}, soft)
        assert not wins[5], name
        for k in (7, 8, 9, 10):
            assert bool(wins[k]) == (ip["spaced"] == 0), (name, k, wins[k])
        assert bool(soft) == (ip["maskLowerCase"] == 0), (name, soft)
    assert seen["default"][0].keys() == {11} and seen["contiguous"][0].keys() == {7, 8, 9, 10, 11}
    print("queries that hit the window targets / the soft-masked homolog:", seen)
    # the 9-residue prefix: hits with contiguous k-mers, none with the spaced pattern (too short for one k-mer)
    q9 = w.qnames.index("prefix9")
    assert len(model["contiguous"]["answers"]["defaults"][q9][0]) > 0 and len(model["default"]["answers"]["defaults"][q9][0]) == 0


@pytest.mark.parametrize("name", P.NAMES)
def test_oracle_equals_compiled_reference(model, name):
    R = K.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    w = P.world()
    o = model[name]["o"]
    r = K.RefKpf(R, w.targets, threads=4, **P.SETTINGS[name])
    try:
        ooff, oseq, opos = o.index()
        roff = r.offsets()
        assert (roff == ooff).all() and int(roff[-1]) == model[name]["entries"]
        sizes = np.diff(roff.astype(np.int64))
        for k in np.nonzero(sizes)[0]:
            s, p = r.index_list(int(k), cap=int(sizes[k]))
            a = int(roff[k])
            assert (s == oseq[a:a + len(s)]).all() and (p == opos[a:a + len(p)]).all(), (name, k)
        for i, t in enumerate(w.targets):
            assert (r.masked(i, len(t)) == model[name]["masked"][i]).all(), (name, i)
        live = [qi for qi, q in enumerate(w.queries) if len(q)]
        for search in P.SEARCHES:
            r.set(**P.search_params(name, search))
            rr, rs, _ = r.run([w.queries[qi] for qi in live], w.identity[live], threads=2)
            for k, qi in enumerate(live):
                b, st, refills = model[name]["answers"][search][qi]
                assert len(b) == len(rr[k]) and (b == rr[k]).all(), (name, search, w.qnames[qi], len(b), len(rr[k]))
                assert np.allclose(st, rs[k], equal_nan=True), (name, search, w.qnames[qi], st, rs[k])
                assert (refills > 0) == (rs[k][2] > 0), (name, search, w.qnames[qi], refills)
    finally:
        r.close()


@pytest.mark.parametrize("kmer_thr", [78, 110])
def test_host_query_preparation_with_contiguous_kmers(kmer_thr):
    """fshost_kmer_query_prepare(spaced = 0): max(0, L - 5) thresholds, each max(kmerThr - round(sum of the composition bias over p .. p + 5), 0) with
    the bias in float32 as the oracle computes it against the k-mer matrix (QueryMatcher.cpp:262-270: summed in float, rounded half away from zero);
    the ungapped profile is the one of spaced = 1"""
    w = P.world()
    ksub, pb, usub = P.matrices()
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    assert (m8.scores().ravel() == ksub).all() and (m2.scores().ravel() == usub).all()
    nonzero = 0
    for q in w.queries:
        L = len(q)
        seq0, thr0, prof0 = api.kmer_query_prepare(m8, m2, q, comp_bias=True, scale=0.15, kmer_thr=kmer_thr, spaced=0)
        seq1, thr1, prof1 = api.kmer_query_prepare(m8, m2, q, comp_bias=True, scale=0.15, kmer_thr=kmer_thr, spaced=1)
        assert len(thr0) == max(0, L - 5) and len(thr1) == max(0, L - 9)
        assert (prof0 == prof1).all() and prof0.shape == (L, 21)
        if L < 6:
            continue
        cbf, _ = H.o_round_bias(ksub, pb, (q % 32).astype(np.uint8), 0.15)
        acc = np.zeros(L - 5, np.float32)
        for z in range(6):
            acc = acc + cbf[z:z + L - 5]                      # float32 + float32: the reference's running float sum, in its order
        assert acc.dtype == np.float32
        rounded = np.trunc(acc.astype(np.float64) + np.where(acc < 0, -0.5, 0.5)).astype(np.int64)
        want = np.maximum(kmer_thr - rounded, 0)
        assert (thr0.astype(np.int64) == want).all(), (L, thr0[:8], want[:8])
        nonzero += int((rounded != 0).sum())
    assert nonzero > 50          # the bias really moves thresholds

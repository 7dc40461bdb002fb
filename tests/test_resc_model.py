"""The model of structurerescorediagonal's per-query body (tests/resc_model.py) held to the REFERENCE BINARY's frozen output, without a GPU, and the census of
what the GPU test runs (tests/resc_cases.py, answers frozen in tests/golden/resc_v1).

1. The three runs of tests/golden/scop_v1 (resc_t2_clu, resc_t2_a, resc_t0_a_sid1) and every run of tests/golden/resc_v1/MANIFEST.json -- coverage modes 0, 1,
   3, 4, 5, identity thresholds under --seq-id-mode 0 and 2, --min-aln-len, --max-accept, --max-rejected, both together, -e 1e-3 with both alignment types,
   -a 0, and the same database under one path and under two with --add-self-matches 0 and 1; thresholds that sit AT a named line's value -- on the frozen
   prefilter lists: the model writes every entry byte for byte -- which lines exist, their order, every column.  Over the new runs every outcome name but the
   two `skipped` ones occurs.
2. The frozen answers of the seeded world are the live model's, for every parameter set and both alignment types; the parameter sets are the derived ones;
   each pair of sets AT a threshold and one representable number beyond it differs in the named hit and in hits at the same value only.
3. What the world contains, asserted on the model's own outcomes (resc_cases.census), so that a change to the cases cannot hollow the GPU test out.
tests/test_diag_model.py keeps holding the pair fields on their own."""
import functools
import json
import os

import numpy as np
import pytest

import diag_model as D
import resc_cases as K
import resc_model as R

SCOP_RUNS = ("resc_t2_clu", "resc_t2_a", "resc_t0_a_sid1")
MANIFEST = json.load(open(os.path.join(K.GOLD, "MANIFEST.json")))
SCOP_MANIFEST = json.load(open(os.path.join(K.SCOP, "MANIFEST.json")))


@functools.lru_cache(maxsize=None)
def pref(name):
    return K.read_pref(os.path.join(K.SCOP if name == "pref_kmer_defined" else K.GOLD, name))


@functools.lru_cache(maxsize=None)
def check_run(fixture, name):
    """-> the model's outcome counts of the run, after its result DB was found equal to the frozen one"""
    run = (SCOP_MANIFEST if fixture == "scop_v1" else MANIFEST)["runs"][name]
    assert run["module"] == "structurerescorediagonal"
    got, res = K.model_db(run, pref(run["positional"][2]))
    want = D.read_db(os.path.join(K.SCOP if fixture == "scop_v1" else K.GOLD, name))
    assert sorted(got) == sorted(want)
    for q in sorted(want):
        assert got[q] == want[q], f"{name}: entry {q}\nwant {want[q][:300]!r}\ngot  {got[q][:300]!r}"
    assert sum(len(v) for v in want.values()) > 0
    if "threshold_at" in run:                                  # the named line still sits at equality, and is accepted there
        at = run["threshold_at"]
        _, P, _ = K.run_params(run)
        value = {"seqId": P["seqIdThr"], "alnLength": P["alnLenThr"], "eval": P["evalThr"]}[at["field"]]
        assert any(int(x["dbKey"]) == at["target"] and float(x[at["field"]]) == float(value) for x in res[at["query"]].records), (name, at)
    return R.count_outcomes(res.values())


@pytest.mark.parametrize("fixture,name", [("scop_v1", n) for n in SCOP_RUNS] + [("resc_v1", n) for n in sorted(MANIFEST["runs"])])
def test_model_reproduces_the_reference_binary(fixture, name):
    assert check_run(fixture, name)["accepted"] > 0


def test_reference_runs_reach_every_outcome():
    assert len(MANIFEST["runs"]) >= 16 and sum("threshold_at" in r for r in MANIFEST["runs"].values()) == 4
    total = {}
    for name in MANIFEST["runs"]:
        for o, n in check_run("resc_v1", name).items():
            total[o] = total.get(o, 0) + n
    assert [o for o in R.OUTCOMES if o not in total] == ["skipped: undefined", "skipped: no overlap"], total
    # no identity under a second path without --add-self-matches, identity through either of the two conditions otherwise (:321)
    c = {n: check_run("resc_v1", n) for n in ("e_sid05_noself", "e_sid05_2path_noself", "e_sid05_2path_self")}
    assert c["e_sid05_noself"] == c["e_sid05_2path_self"] and c["e_sid05_noself"]["accepted as identity"] >= 20
    assert "accepted as identity" not in c["e_sid05_2path_noself"]
    assert c["e_sid05_2path_noself"]["seq id"] == c["e_sid05_noself"]["seq id"] + c["e_sid05_noself"]["accepted as identity"]
    census = open(os.path.join(K.GOLD, "CENSUS.md")).read()
    for name in MANIFEST["runs"]:
        row = [l for l in census.splitlines() if l.startswith(f"| {name} |")]
        assert len(row) == 1 and [int(x) for x in row[0].split("|")[2:-1]] == [check_run("resc_v1", name).get(o, 0) for o in R.OUTCOMES], name


def test_the_crafted_prefilter_lists():
    """pref_resc_edges: defined pairs only; per query the self hit on diagonal 0, on a far diagonal with four cells and on a near one, one target on two
    diagonals, two runs of at least three lines the default gates reject between accepted ones, and an order that is not score order"""
    keys, seqs = K.scop_sequences()
    run = dict(positional=["db", "db"], parameters=MANIFEST["runs"]["e_cov0"]["parameters"])
    run["parameters"] = [("0" if i and run["parameters"][i - 1] == "-c" else x) for i, x in enumerate(run["parameters"])]
    _, res = K.model_db(run, pref("pref_resc_edges"))
    for q, lines in pref("pref_resc_edges").items():
        L = len(seqs[q][0])
        assert all(K.defined(L, len(seqs[t][0]), d) for t, d in lines)
        self_d = [d for t, d in lines if t == q]
        assert 0 in self_d and L - 4 in self_d and any(0 < d <= 12 for d in self_d)
        ts = [t for t, _ in lines if t != q]
        assert len(ts) > len(set(ts))
        out = res[q].outcomes
        assert out[lines.index((q, L - 4))] == "e-value" and out[lines.index((q, 0))] == "accepted"
        pattern = "".join("r" if o == "e-value" else "a" for o in out)
        assert pattern.count("rrra") >= 2 and "a" in pattern[:pattern.index("rrra")], (q, pattern)
        assert res[q].hit_of_record != sorted(res[q].hit_of_record)


# ---- the seeded world ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def live(atype):
    lv = K.Live(atype)
    sets, extra = K.derive(lv)
    return lv, sets, extra, K.answers(lv, sets)


@pytest.mark.parametrize("atype", K.ATYPES)
def test_frozen_answers_are_the_live_models(atype):
    lv, sets, extra, ans = live(atype)
    F = K.Frozen(atype)
    assert sorted(F.names) == sorted(sets) and sorted(F.extra) == sorted(extra)
    for n in extra:
        assert extra[n][0] == F.extra[n][0] and (extra[n][1] == F.extra[n][1]).all() and (extra[n][2] == F.extra[n][2]).all()
    for name, S in sets.items():
        fs = F.set(name)
        assert (fs["P"], fs["identity"], fs["skip"], fs["lists"]) == (S["P"], S["identity"], S["skip"], S["lists"]), name
        for k, r in enumerate(ans[name]):
            if isinstance(r, R.Undefined):
                assert F.records(name, k) is None and fs["error"] == dict(list=S["lists"][k], key=r.key, diagonal=r.diagonal, kind=r.kind)
                assert str(r.key) in str(r) and str(r.diagonal) in str(r) and S["lists"][k] in str(r)      # the refusal names query, target key and diagonal
                continue
            rec, bts, hit = F.records(name, k)
            assert rec.tobytes() == r.records.tobytes() and bts == r.backtraces and list(hit) == r.hit_of_record, (atype, name, k)
            assert F.outcomes(name, k) == r.outcomes, (atype, name, k)


@pytest.mark.parametrize("atype", K.ATYPES)
def test_census_of_the_seeded_world(atype):
    lv, sets, extra, ans = live(atype)
    w = K.world()
    lens = [len(a) for a, _ in w["queries"]]
    assert sorted(lens) == [1, 2, 24, 47, 80, 129, 200, 257, 320, 1025] and sum(n % 4 != 0 for n in lens) >= 5
    tl = [len(a) for a, k in zip([t[0] for t in w["targets"]], w["kinds"]) if k != "identity"]
    assert min(tl) == 1 and max(tl) == 420 and (np.diff(w["keys"].astype(np.int64)) < 0).any()
    assert all(20 <= len(w["lists"][n][1]) <= 110 for n in K.DEFINED)
    assert all(K.defined(lens[q], len(w["targets"][int(t)][0]), int(d)) for n in K.DEFINED for q, ts, ds, _ in [w["lists"][n]] for t, d in zip(ts, ds))
    assert any(int(d) < 0 for n in K.DEFINED for d in w["lists"][n][2])
    assert K.check_pairs(lv, sets) == 16                      # six canBeCovered modes, five coverages, the e-value, three identity modes, the length
    K.census(lv, sets, ans)
    for f in os.listdir(K.GOLD):
        assert os.path.getsize(os.path.join(K.GOLD, f)) < 400000, f


def test_a_reached_undefined_pair_is_an_error_without_the_skip_rule():
    lv, sets, extra, ans = live(2)
    w = K.world()
    q, ts, ds, kinds = w["lists"]["mixed"]
    first = kinds.index("undefined")
    with pytest.raises(R.Undefined) as e:
        R.rescore_query(lv.W, *w["queries"][q], list(zip(ts.tolist(), ds.tolist())), R.params(), identity=w["identity"][q], skip=False, qname="mixed")
    assert (e.value.key, e.value.diagonal, e.value.kind) == (int(w["keys"][int(ts[first])]), int(ds[first]), "undefined")
    r = R.rescore_query(lv.W, *w["queries"][q], list(zip(ts.tolist(), ds.tolist())), R.params(), identity=w["identity"][q], skip=True)
    assert r.outcomes.count("skipped: undefined") == 3 and r.outcomes.count("skipped: no overlap") == 4
    # the skipped pairs left out of the list: the same records
    keep = [k for k, o in enumerate(r.outcomes) if not o.startswith("skipped")]
    r2 = R.rescore_query(lv.W, *w["queries"][q], [(int(ts[k]), int(ds[k])) for k in keep], R.params(), identity=w["identity"][q])
    assert r2.records.tobytes() == r.records.tobytes()

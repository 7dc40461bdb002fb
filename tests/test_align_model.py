"""The model of structurealign's accept loop (tests/align_model.py) held to the REFERENCE BINARY's frozen output, without a GPU, and the census of the seeded
world the GPU test runs (tests/align_cases.py, answers frozen in tests/golden/align_v1).

1. Every `aln_*` run of tests/golden/scop_v1 (both alignment types, -e 0.001 -c 0.8, coverage modes 1..5, both other seq-id modes, --min-aln-len,
   --max-accept / --max-rejected, --alt-ali 2, other gap costs, no / scaled composition bias, the ungapped prefilter's lists, the padded target DB) and
   every thresholded / structure-bits run of tests/golden/ca_v1 and tm_v1 (LDDT 0.5 / 0.7 / 0.8, the three TM modes, structure bits alone, with both
   thresholds, with --alt-ali, with --max-rejected, padded): the live model on the frozen prefilter lists gives every line the reference wrote -- all
   fields at the precision it printed, CIGARs included, in its order.  The per-pair LDDT averages and TM-scores are the frozen answers of
   tests/lddt_model.py / tests/tm_model.py for the records of ca_v1's aln_l0, taken only after the model's own start cells and CIGAR were found equal to
   that record.
   THE SAMPLE.  The Python block aligner needs about 0.1 s per pair, so the suite runs queries 3, 13 and 23 of scop_v1's 30 and queries 1, 5 and 9 of
   ca_v1's 12 for EVERY run; tests/golden/make_align_golden.py scop runs all queries of all runs (check_reference_runs(sample=None)).
2. The frozen answers of the seeded world are the live model's: queries 0, 3 and 8 (3Di + AA) and 1 and 3 (3Di only) re-run for every parameter set.
3. What the world contains, asserted on the model's own outcomes, so that a change to the cases cannot hollow the GPU test out."""
import functools
import json
import os

import numpy as np
import pytest

import align_cases as K
import align_model as A
import diag_model as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SAMPLE = {"scop_v1": (3, 13, 23), "ca_v1": (1, 5, 9)}


# ---- the reference's frozen runs -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _manifest(fixture):
    return json.load(open(os.path.join(GOLDEN, fixture, "MANIFEST.json")))


def _db(fixture, name):
    return D.read_db(os.path.join(GOLDEN, fixture, name))


@functools.lru_cache(maxsize=None)
def _sequences(fixture, padded):
    """-> (keys in index order, {key: (AA codes, 3Di codes)}, {key: key of the same entry in the source DB}).  A padded DB (makepaddedseqdb) renumbers the
    entries by length; its AA index points into the source DB's data, which is how an entry is traced back."""
    g = os.path.join(GOLDEN, fixture)
    aa, ss = _db(fixture, "db"), _db(fixture, "db_ss")
    seqs = {k: (D.encode(aa[k].decode().rstrip("\n")), D.encode(ss[k].decode().rstrip("\n"))) for k in aa}
    if not padded:
        return sorted(seqs), seqs, {k: k for k in seqs}
    src_at = {int(l.split()[1]): int(l.split()[0]) for l in open(os.path.join(g, "db.index"))}
    back = {int(l.split()[0]): src_at[int(l.split()[1])] for l in open(os.path.join(g, "db_pad.index"))}
    return sorted(back), {k: seqs[s] for k, s in back.items()}, back


@functools.lru_cache(maxsize=None)
def _world(fixture, padded, atype, comp_bias, scale, go, ge):
    keys, seqs, _ = _sequences(fixture, padded)
    return A.World([seqs[k] for k in keys], keys=np.array(keys, np.uint32), alignment_type=atype, comp_bias=comp_bias, scale=scale, go=go, ge=ge)


def _flags(par):
    return {par[i]: par[i + 1] for i in range(len(par) - 1) if par[i].startswith("-") and not par[i + 1].startswith("--")}


def run_setup(fixture, name):
    """the frozen parameter string of a run -> (world, model parameters, backtraces written, prefilter DB, padded)"""
    man = _manifest(fixture)
    run = man["runs"][name]
    f = _flags(run["parameters"])
    padded = run["positional"][1] == "db_pad"
    go, ge = int(f["--gap-open"].split(",")[0].split(":")[1]), int(f["--gap-extend"].split(",")[0].split(":")[1])
    W = _world(fixture if fixture != "tm_v1" else "ca_v1", padded, int(f["--alignment-type"]), f["--comp-bias-corr"] == "1", float(f["--comp-bias-corr-scale"]), go, ge)
    f32 = lambda x: float(np.float32(float(x)))  # noqa: E731  float parameters of the reference; -e is a double
    P = A.params(evalThr=float(f["-e"]), covThr=f32(f["-c"]), covMode=int(f["--cov-mode"]), seqIdThr=f32(f["--min-seq-id"]), seqIdMode=int(f["--seq-id-mode"]),
                 alnLenThr=int(f["--min-aln-len"]), maxAccept=int(f["--max-accept"]), maxRejected=int(f["--max-rejected"]), altAlignment=int(f["--alt-ali"]),
                 tmThr=f32(f["--tmscore-threshold"]), tmMode=int(f["--tmscore-threshold-mode"]), lddtThr=f32(f["--lddt-threshold"]),
                 structureBits=int(f["--sort-by-structure-bits"]))
    return W, P, f["-a"] == "1", run["positional"][2], padded


def _callbacks(W, back, qkey, hits, P):
    return K.ca_callbacks(qkey, [back[int(W.keys[h])] for h in hits], P)


def check_run(fixture, name, sample):
    W, P, with_bt, pref_name, padded = run_setup(fixture, name)
    src = fixture if fixture != "tm_v1" else "ca_v1"
    keys, seqs, back = _sequences(src, padded)
    qkeys, qseqs, _ = _sequences(src, False)
    idx = {k: i for i, k in enumerate(keys)}
    pref = {q: [int(l.split()[0]) for l in e.decode().splitlines()] for q, e in _db(src, pref_name).items()}
    want = _db(fixture, name)
    lines = 0
    for n, q in enumerate(qkeys):
        if sample is not None and n not in sample:
            continue
        hits = [idx[t] for t in pref.get(q, [])]
        identity = -1 if padded else idx[q]                # isIdentity needs the same database on both sides (structurealign.cpp:168, :356)
        lddt, tm = _callbacks(W, back, q, hits, P)
        r = A.align_query(W, qseqs[q][0], qseqs[q][1], hits, P, identity=identity, lddt=lddt, tm=tm)
        got = [A.line(rec, c if with_bt else None) for rec, c in zip(r.records, r.cigars)]
        exp = want.get(q, b"").decode().splitlines()
        # two records equal in every key of the comparator (an alternative alignment with the score of its primary): std::sort leaves their order open
        cmp_ = A.compare_structure_bits if P["structureBits"] else A.compare_hits
        i = 0
        while i < len(got):
            j = i + 1
            while j < len(got) and cmp_(r.records[i], r.records[j]) == 0:
                j += 1
            got[i:j], exp[i:j] = sorted(got[i:j]), sorted(exp[i:j])
            i = j
        assert got == exp, (fixture, name, q, [(a, b) for a, b in zip(got, exp) if a != b][:2], len(got), len(exp))
        assert "e-value crit" not in r.outcomes
        lines += len(exp)
    return lines


def reference_runs():
    out = [("scop_v1", n) for n in sorted(_manifest("scop_v1")["runs"]) if n.startswith("aln_")]
    out += [("ca_v1", n) for n in sorted(_manifest("ca_v1")["runs"]) if n.startswith("aln_")]
    out += [("tm_v1", n) for n in sorted(_manifest("tm_v1")["runs"]) if n.startswith("aln_")]
    return out


def check_reference_runs(sample):
    for fixture, name in reference_runs():
        n = check_run(fixture, name, None if sample is None else sample[fixture if fixture != "tm_v1" else "ca_v1"])
        print(f"{fixture}/{name}: {n} lines equal", flush=True)


@pytest.mark.parametrize("fixture,name", reference_runs())
def test_model_reproduces_the_reference_binary(fixture, name):
    assert check_run(fixture, name, SAMPLE[fixture if fixture != "tm_v1" else "ca_v1"]) > 0


def test_every_kind_of_reference_run_is_there():
    names = {n for _, n in reference_runs()}
    assert len(names) == 36, sorted(names)
    for n in ("aln_t0_a", "aln_t2_a_e001_c08", "aln_t2_a_cov1", "aln_t2_a_cov5", "aln_t2_a_sid1", "aln_t2_a_sid2", "aln_t2_a_minlen", "aln_t2_a_maxacc",
              "aln_t2_a_altali", "aln_t0_a_gap", "aln_t2_a_nocb", "aln_t2_a_cbs", "aln_l05", "aln_l07", "aln_l08", "aln_l07_maxrej", "aln_sb0_t07_m0",
              "aln_sb0_t07_m1", "aln_sb0_t07_m2", "aln_sb1", "aln_sb1_t07_maxrej"):
        assert n in names, n


# ---- the seeded world ----------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frozen(atype):
    return K.Frozen(atype)


@pytest.mark.parametrize("atype,queries", [(2, (0, 3, 8)), (0, (1, 3))])
def test_frozen_answers_are_the_live_models(atype, queries):
    F, live = frozen(atype), K.Live(atype)
    for name in F.names:
        P = F.params(name)
        for q in queries:
            r = live.query(q, P)
            want, cigars, hit = F.records(name, q)
            assert r.records.tobytes() == want.tobytes() and r.cigars == cigars and list(hit) == r.hit_of_record, (atype, name, q)
            assert r.outcomes == F.outcomes(name, q) and r.reversed == F.looked(name)[q], (atype, name, q)
            assert (r.fwd.view(np.int32).reshape(-1, 4) == F.fwd(q)).all() and (r.rev.view(np.int32).reshape(-1, 4) == F.rev(name, q)).all(), (atype, name, q)
            assert [tuple(e) for e in F.alt_ends(name) if e[0] == q] == [(q, k, n, why) for k, n, why in r.alt_ends], (atype, name, q)


def test_parameter_sets_are_the_derived_ones():
    """the thresholds in the frozen files are what derive() reads off the live model's records of the named query (3Di + AA)"""
    live = K.Live(2)
    Q = K.NAMED_QUERY
    sets = K.derive(lambda P: [live.query(q, P) if q == Q or q == 0 else None for q in range(len(K.world()["queries"]))], live.evalue_fwd)
    F = frozen(2)
    assert sorted(sets) == sorted(F.names)
    for name in sets:
        assert sets[name] == F.params(name), name


@pytest.mark.parametrize("atype", K.ATYPES)
def test_census_of_the_seeded_world(atype):
    F, w = frozen(atype), K.world()
    assert len(w["queries"]) == 9 and 1025 in [len(a) for a, _ in w["queries"]] and 300 <= len(w["targets"]) <= 400
    assert min(len(a) for a, _ in w["targets"]) == 1 and max(len(a) for a, k in zip([t[0] for t in w["targets"]], w["kinds"]) if k != "identity") == 420
    assert sorted(F.n)[0] == 1 and sorted(F.n)[1] >= 20 and max(F.n) <= 150
    c = {name: F.count(name) for name in F.names}
    has = lambda name, o, n=1: c[name].get(o, 0) >= n  # noqa: E731
    # every reject reason; a hit that passes the end-based coverage gate and fails checkCriteria's start-based coverage
    for mode in (0, 1, 2):
        for v in ("eq", "next"):
            assert has(f"cov{mode}_{v}", "end coverage") and has(f"cov{mode}_{v}", "start coverage") and has(f"cov{mode}_{v}", "accepted"), (mode, v)
            assert has(f"cov{mode}_{v}", "not coverable")
        # AT equality the named hit is accepted, one float above it fails the start-based coverage
        assert c[f"cov{mode}_next"]["accepted"] < c[f"cov{mode}_eq"]["accepted"] and c[f"cov{mode}_next"]["start coverage"] > c[f"cov{mode}_eq"]["start coverage"]
    for side in "qt":          # each comparison of the bidirectional mode decided at equality on its own
        assert c[f"cov0{side}_next"]["accepted"] < c[f"cov0{side}_eq"]["accepted"] and c[f"cov0{side}_next"]["start coverage"] > c[f"cov0{side}_eq"]["start coverage"]
    for mode in (3, 4, 5):
        assert c[f"cov{mode}_next"]["not coverable"] > c[f"cov{mode}_eq"]["not coverable"] and has(f"cov{mode}_next", "accepted")
        assert "end coverage" not in c[f"cov{mode}_eq"] and "start coverage" not in c[f"cov{mode}_eq"]
    for mode in (0, 1, 2):
        assert c[f"sid{mode}_next"]["seq id"] > c[f"sid{mode}_eq"]["seq id"] >= 1
    assert c["len_next"]["aln length"] > c["len_eq"]["aln length"] >= 1
    assert c["ediff_below"]["accepted"] == c["ediff_eq"]["accepted"] - 1
    assert c["efwd_below"]["e-value fwd"] == c["efwd_eq"]["e-value fwd"] + 1
    assert has("default", "e-value fwd") and has("default", "e-value diff")
    # the identity target: failing a criterion and accepted anyway; failing a score gate and NOT accepted
    assert has("len_eq", "accepted as identity") and has("alt_len", "accepted as identity")
    pos = [k for k, t in enumerate(w["lists"][0]) if int(t) == w["identity"][0]][0]
    assert F.outcomes("default", 0)[pos] == "accepted" and F.outcomes("ident_below", 0)[pos] in ("e-value diff", "e-value fwd")
    # limits: the rejected count reaches maxRejected - 1, is reset by an accepted hit, and trips later
    Q = K.NAMED_QUERY
    out, m = F.outcomes("rej_reset", Q), F.params("rej_reset")["maxRejected"]
    runs, n = [], 0
    for o in out:
        if o.startswith("accepted"):
            runs.append(n); n = 0
        elif not o.startswith("not reached"):
            n += 1
    assert m - 1 in runs and n == m and out[-1] == "not reached: max-rejected", (runs, n, m)
    assert "not reached: max-accept" not in F.outcomes("acc_last", Q) and F.outcomes("acc_last", Q)[-1] == "accepted"      # met exactly at the last hit
    tail = F.outcomes("acc_before", Q)
    assert tail[-1] == "not reached: max-accept" and sum(o == "not reached: max-accept" for o in tail) >= 1                # ... and one before it
    assert has("acc_rej_mix", "not reached: max-accept") and has("acc_rej_mix", "not reached: max-rejected")
    assert has("both_1", "not reached: max-accept") and has("both_1", "not reached: max-rejected")
    # --alt-ali: two further alignments of the repeat target (cumulative masking), the capacity of the ninth list, every way a search for more ends
    _, _, hit = F.records("alt2", 8)
    assert len(hit) == 3 == F.n[8] * 3
    ends = {name: {} for name in F.names}
    for name in F.names:
        for _q, _k, _n, why in F.alt_ends(name):
            ends[name][why] = ends[name].get(why, 0) + 1
    assert ends["alt1"].get("count reached", 0) >= 1 and ends["alt3"].get("e-value diff", 0) >= 1 and ends["alt1"].get("e-value fwd", 0) >= 1
    assert ends["alt_len"].get("criteria", 0) >= 1 and ends["alt_cov"].get("end coverage", 0) >= 1 and ends["alt_cov_end"].get("end coverage", 0) >= 1
    assert any(n == 2 for _q, _k, n, _w in F.alt_ends("alt3"))
    # ties: two byte-identical targets whose key order is the reverse of their id order; a target and the same target with a tail: dbLen decides
    by_key = by_len = 0
    for q in range(len(F.n)):
        rec, _, hit = F.records("default", q)
        for i in range(len(rec) - 1):
            a, b = rec[i], rec[i + 1]
            if a["eval"] == b["eval"] and a["score"] == b["score"]:
                ia, ib = int(w["lists"][q][hit[i]]), int(w["lists"][q][hit[i + 1]])
                if a["dbLen"] == b["dbLen"]:
                    assert a["dbKey"] < b["dbKey"]
                    by_key += ia > ib
                else:
                    assert a["dbLen"] < b["dbLen"]
                    by_len += 1
    assert by_key >= 1 and by_len >= 1, (by_key, by_len)
    # a block alignment that fails (start -1): the model produces none in this world
    for name in F.names:
        for q in range(len(F.n)):
            assert (F.records(name, q)[0]["qStartPos"] >= 0).all()
    for f in os.listdir(K.GOLD):
        assert os.path.getsize(os.path.join(K.GOLD, f)) < 400000, f


def test_frozen_answers_of_the_example_structures_are_the_live_models():
    """queries 1, 5 and 9 of ca_v1 for every LDDT / TM / structure-bits parameter set"""
    F, live = K.Frozen("ca"), K.LiveCa()
    assert K.ca_sets() == {name: F.params(name) for name in F.names}
    for name in F.names:
        for q in SAMPLE["ca_v1"]:
            r = live.query(q, F.params(name))
            want, cigars, hit = F.records(name, q)
            assert r.records.tobytes() == want.tobytes() and r.cigars == cigars and r.outcomes == F.outcomes(name, q), (name, q)
            assert r.reversed == F.looked(name)[q] and (r.rev.view(np.int32).reshape(-1, 4) == F.rev(name, q)).all(), (name, q)


def test_census_of_the_example_structures():
    """hits drop under every threshold; with a reject limit the rule `a dropped hit counts neither as accepted nor as rejected` decides where a list stops:
    counting a drop as a rejection would stop at least three lists of every such set before a hit they accept"""
    F = K.Frozen("ca")
    c = {name: F.count(name) for name in F.names}
    for m in (0, 1, 2):
        assert c[f"tm07_m{m}"]["tm drop"] >= 10
    assert c["tm07_m0"]["tm drop"] < c["tm07_m1"]["tm drop"] != c["tm07_m2"]["tm drop"]
    assert c["lddt07"]["lddt drop"] >= 10 and c["lddt07_tm07_m1"]["tm drop"] >= 10 and c["lddt07_tm07_m1"]["lddt drop"] >= 10
    assert c["sb"] == {"accepted": 144} and c["sb_lddt07_tm07_m1"] == c["lddt07_tm07_m1"]
    for name in F.names:
        if not name.endswith("_e_rej2"):
            continue
        m = F.params(name)["maxRejected"]
        changed = 0
        for q in range(len(F.n)):
            out = F.outcomes(name, q)
            stop = next((k for k, o in enumerate(out) if o.startswith("not reached")), len(out))
            rejected, stop_wrong = 0, None
            for k, o in enumerate(out[:stop]):          # the wrong rule: everything that is not accepted counts
                rejected = 0 if o.startswith("accepted") else rejected + 1
                if rejected >= m:
                    stop_wrong = k + 1
                    break
            changed += stop_wrong is not None and any(o.startswith("accepted") for o in out[stop_wrong:stop])
        print(name, "lists that would lose accepted hits if a drop counted as a rejection:", changed)
        assert changed >= 3, name
    # the matrix of what the entries are run with
    assert any(n.endswith("_acc3") for n in F.names) and sum(c[n].get("not reached: max-accept", 0) for n in F.names) > 0

"""Profile queries at module level, on REFERENCE-WRITTEN profile databases (tests/golden/profile_v1, generator tests/golden/make_profile_golden.py:
`result2profile` after round 0 on the 12 example structures, and a crafted profile database).  `fsgpu-modules` runs with the positional arguments and
the complete parameter strings the reference binary was run with, and every result DB must be the reference's byte for byte: data, index and type."""
import json
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "profile_v1")
BIN = os.path.join(ROOT, "foldseek_amd", "bin", "fsgpu-modules")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))
RUNS = MANIFEST["runs"]
_PREF = sorted(n for n, r in RUNS.items() if r["module"] == "ungappedprefilter")
_ALIGN = sorted(n for n, r in RUNS.items() if r["module"] == "structurealign")


@pytest.fixture()
def work(tmp_path):
    w = tmp_path / "profile"
    shutil.copytree(GOLD, w)
    return w


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _same_files(got, want):
    """data, index and dbtype, byte for byte; on a difference the first differing entry"""
    for ext in ("", ".index", ".dbtype"):
        g, w = open(got + ext, "rb").read(), open(want + ext, "rb").read()
        if g != w and ext == "":
            for i, (a, b) in enumerate(zip(w.split(b"\n"), g.split(b"\n"))):
                assert a == b, f"{os.path.basename(want)}: line {i + 1}\nwant {a[:300]!r}\ngot  {b[:300]!r}"
        assert g == w, (os.path.basename(want) + ext, len(g), len(w))


def _with(par, **kw):
    par = list(par)
    for flag, v in kw.items():
        par[par.index(flag) + 1] = str(v)
    return par


@pytest.mark.parametrize("threads", (1, 4))
@pytest.mark.parametrize("name", _PREF)
def test_ungappedprefilter_equals_reference_result_db(work, name, threads):
    run = RUNS[name]
    out = str(work / f"mine_{name}")
    r = _run([BIN, "ungappedprefilter"] + [str(work / p) for p in run["positional"]] + [out] + _with(run["parameters"], **{"--threads": threads}) + ["--gpus", "1"])
    assert r.returncode == 0, r.stderr
    _same_files(out, str(work / name))


@pytest.mark.parametrize("threads", (1, 4))
@pytest.mark.parametrize("name", _ALIGN)
def test_structurealign_equals_reference_result_db(work, name, threads):
    """alignment types 0 and 2 (the reference reads the AA profile either way: the two frozen results are the same bytes), with and without -a, the
    coverage and e-value thresholds, the accept / reject limits, and the crafted profiles: one position, the extremes, the saturating one, 1025 positions"""
    run = RUNS[name]
    out = str(work / f"mine_{name}")
    r = _run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + _with(run["parameters"], **{"--threads": threads}) + ["--gpus", "1"])
    assert r.returncode == 0, r.stderr
    _same_files(out, str(work / name))


def test_alignment_type_does_not_reach_a_profile_query():
    for a, b in (("paln_t0_a", "paln_t2_a"), ("paln_t0", "paln_t2")):
        assert open(os.path.join(GOLD, a), "rb").read() == open(os.path.join(GOLD, b), "rb").read()


@pytest.mark.parametrize("threads", (1, 4))
@pytest.mark.parametrize("name, query, target, pref", (("paln_t2_a", "profile_0", "db", "ppref"), ("caln_t2_a", "cprof", "ctarget", "cpref")))
def test_search_with_the_ungapped_prefilter_equals_the_two_reference_modules(work, name, query, target, pref, threads):
    """`search --prefilter-mode 1` is ungappedprefilter + structurealign in one process: both result DBs are the reference's.  The argument vector is
    written here, not recorded by the generator: the reference's `search` is a shell workflow over the two modules, and no run of it is frozen."""
    out, outp = str(work / f"mine_search_{name}"), str(work / f"mine_search_{name}_pref")
    r = _run([BIN, "search", str(work / query), str(work / target), out, outp, "--prefilter-mode", "1", "--min-ungapped-score", "15", "-a", "1", "--alignment-type", "2",
              "--sort-by-structure-bits", "0", "--threads", str(threads), "--gpus", "1", "--max-seqs", "1000", "-e", "10"])
    assert r.returncode == 0, r.stderr
    _same_files(outp, str(work / pref))
    _same_files(out, str(work / name))


# ---- the C-alpha flags: a profile query database has no _ca, so they behave as for a sequence query without one ------------------------------------------
def _structurealign(work, out, **kw):
    run = RUNS["paln_t2_a"]
    return _run([BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [str(work / out)] + _with(run["parameters"], **kw))


def test_structure_bits_without_ca_warns_and_turns_itself_off(work):
    r = _structurealign(work, "mine_bits", **{"--sort-by-structure-bits": 1})
    assert r.returncode == 0, r.stderr
    assert "C-alpha database\nDisabling --sort-by-structure-bits\n" in r.stderr
    _same_files(str(work / "mine_bits"), str(work / "paln_t2_a"))


def test_lddt_threshold_without_ca_warns_and_runs_without_the_filter(work):
    r = _structurealign(work, "mine_lddt", **{"--lddt-threshold": 0.5})
    assert r.returncode == 0, r.stderr
    assert "Cannot use --lddt-threshold with --sort-by-structure-bits 0\nDisabling --lddt-threshold\n" in r.stderr
    _same_files(str(work / "mine_lddt"), str(work / "paln_t2_a"))


def test_tmscore_threshold_without_ca_is_refused_by_name(work):
    r = _structurealign(work, "mine_tm", **{"--tmscore-threshold": 0.5})
    assert r.returncode != 0 and "structurealign: --tmscore-threshold 0.5 is not implemented on the device path" in r.stderr, r.stderr
    assert not os.path.exists(work / "mine_tm")


# ---- a damaged entry: the decoder's refusal, with the entry's key, and nothing written -------------------------------------------------------------------
@pytest.mark.parametrize("module", ("ungappedprefilter", "structurealign"))
def test_a_damaged_profile_entry_is_refused_by_name(work, module):
    data = open(work / "profile_0_ss", "rb").read()
    key, off, _ = open(work / "profile_0_ss.index").readline().split()
    off = int(off)
    open(work / "profile_0_ss", "wb").write(data[:off + 25 * 3 + 20] + bytes([33]) + data[off + 25 * 3 + 21:])          # the query letter of position 3
    if module == "ungappedprefilter":
        r = _run([BIN, module, str(work / "profile_0_ss"), str(work / "db_ss"), str(work / "out"), "--threads", "1"])
    else:
        r = _run([BIN, module, str(work / "profile_0"), str(work / "db"), str(work / "ppref"), str(work / "out"), "--threads", "1"])
    assert r.returncode != 0
    assert f"{module} failed: query profile {key}: profile entry: query letter at position 3 is 33, above 20" in r.stderr, r.stderr
    assert not os.path.exists(work / "out.index")


# ---- the library's four search bodies, directly: one query at a time == the batch == the reference's lines ------------------------------------------------
def test_single_query_bodies_equal_the_batch_bodies_and_the_reference():
    import numpy as np
    import align_model
    from foldseek_amd import api, synth
    letters = "ACDEFGHIKLMNPQRSTVWYX"

    def read_db(name):
        data, out = open(os.path.join(GOLD, name), "rb").read(), {}
        for line in open(os.path.join(GOLD, name + ".index")):
            k, off, ln = line.split()
            out[int(k)] = data[int(off):int(off) + int(ln) - 1]
        return out

    def seq_db(name):
        return {k: np.array([letters.index(chr(c).upper()) for c in v.rstrip(b"\n")], np.uint8) for k, v in read_db(name).items()}
    tA, t3 = seq_db("db"), seq_db("db_ss")
    keys = sorted(t3)                                                      # reader order, as the modules load a plain database: ties go by it
    lens = np.array([len(t3[k]) for k in keys], np.int32)
    off = np.zeros(len(keys) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
    for i, k in enumerate(keys):
        d3[off[i]:off[i] + lens[i]] = t3[k]; da[off[i]:off[i] + lens[i]] = tA[k]
    index_of = {k: i for i, k in enumerate(keys)}
    ctx = api.Context(0)
    ctx.load_db(synth.PaddedDB(d3, da, off, lens))
    par = api.default_params()
    par.minDiagScoreThr, par.maxResListLen, par.evalThr, par.addBacktrace, par.alignmentType = 15, 1000, 10.0, 1, 2
    s = api.Search(ctx, par, keys=np.array(keys, np.uint32))
    try:
        pA, p3 = read_db("profile_0"), read_db("profile_0_ss")
        pref, aln = read_db("ppref"), read_db("paln_t2_a")
        qkeys = sorted(p3)
        batch_hits = s.prefilter_batch_profile([p3[k] for k in qkeys])
        lists = []
        for k, bh in zip(qkeys, batch_hits):
            one = s.prefilter_profile(p3[k])
            assert one.tobytes() == bh.tobytes(), k
            assert "".join(api.format_prefilter_hit(keys[int(h["id"])], int(h["score"])) for h in one) == pref[k].decode(), k
            lists.append(np.array([index_of[int(l.split("\t")[0])] for l in pref[k].decode().splitlines()], np.uint32))
        b_res, b_bt = s.align_batch_profile([(pA[k], p3[k]) for k in qkeys], lists)
        for i, k in enumerate(qkeys):
            res, bt = s.align_profile(pA[k], p3[k], lists[i])
            assert len(res) == len(b_res[i]) and bt == b_bt[i], k
            rows = [l.split("\t") for l in aln[k].decode().splitlines()]
            assert len(rows) == len(res), k
            for r, one, many, cig in zip(rows, res, b_res[i], bt):
                got = tuple(int(one[f]) for f in ("dbKey", "score", "qStartPos", "qEndPos", "qLen", "dbStartPos", "dbEndPos", "dbLen"))
                assert got == tuple(int(many[f]) for f in ("dbKey", "score", "qStartPos", "qEndPos", "qLen", "dbStartPos", "dbEndPos", "dbLen"))
                assert got == (int(r[0]), int(r[1]), int(r[4]), int(r[5]), int(r[6]), int(r[7]), int(r[8]), int(r[9])), (k, r)
                assert "%.3E" % float(one["eval"]) == r[3] and align_model.compress(cig) == r[10], (k, r)
        par.altAlignment = 1
        s2 = api.Search(ctx, par, keys=np.array(keys, np.uint32))
        with pytest.raises(api.FsgpuError) as e:
            s2.align_profile(pA[qkeys[0]], p3[qkeys[0]], lists[0])
        assert e.value.rc == api.FSGPU_E_UNSUPPORTED and "--alt-ali with a profile query" in str(e.value)
        s2.close()
    finally:
        s.close()
        ctx.close()


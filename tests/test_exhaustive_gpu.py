"""The exhaustive search -- fshost_search_exhaustive_batch (Search.exhaustive_batch) and `fsgpu-modules search --prefilter-mode 2` / `--exhaustive-search 1`
-- against (a) the frozen answers of tests/align_model.py over ALL targets of tests/align_cases.py's world (tests/golden/exh_v1, tests/exh_cases.py),
record by record and CIGAR by CIGAR; against Search.align_batch over range(n), byte for byte; the survivor counts against the model's count of
first-gate passers; and (b) the reference binary's own `search --exhaustive-search 1` result databases on the frozen SCOP databases, data and index
byte for byte.  No tolerance anywhere."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import align_cases as AC
import exh_cases as E
from foldseek_amd import api
from test_align_entries_gpu import INT_MAX, make_params, pack, same_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "foldseek_amd", "bin", "fsgpu-modules")
SCOP = os.path.join(ROOT, "tests", "golden", "scop_v1")
SCOP_MANIFEST = json.load(open(os.path.join(SCOP, "MANIFEST.json")))
REF_RUNS = json.load(open(os.path.join(E.GOLD, "REF_RUNS.json")))
SET_NAMES = ("default", "efwd_eq", "efwd_below", "e1e300", "c08", "acc3", "alt2")


@pytest.fixture(scope="module")
def env():
    w = AC.world()
    ctx = api.Context(0)
    ctx.load_db(pack(w["targets"]))
    assert ctx.residues == sum(len(a) for a, _ in w["targets"])          # what the model's e-values were computed with
    yield dict(w=w, ctx=ctx, frozen={t: E.Frozen(t) for t in E.ATYPES})
    ctx.close()


@pytest.mark.parametrize("atype", E.ATYPES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_exhaustive_batch_equals_the_model_and_align_batch(env, atype, name):
    w, F = env["w"], env["frozen"][atype]
    assert sorted(F.names) == sorted(SET_NAMES)
    P = F.params(name)
    nq, n = E.n_queries(), len(w["targets"])
    qa, q3 = [x[0] for x in w["queries"][:nq]], [x[1] for x in w["queries"][:nq]]
    ident = w["identity"][:nq]
    s = api.Search(env["ctx"], make_params(atype, P), keys=w["keys"])
    try:
        res, bts = s.exhaustive_batch(qa, q3, identity=ident, with_backtrace=True)
        for q in range(nq):
            want, cigars = F.records(name, q)
            same_records(res[q], bts[q], want, cigars, (atype, name, "exhaustive_batch", q))
        assert s.last_survivors == F.survivors(name), (atype, name, "targets the first e-value gate lets through")
        if name == "e1e300":
            assert s.last_survivors == [n] * nq                           # cutoff 0: everything survives
        elif name == "default":
            assert all(0 < x < n for x in s.last_survivors)               # the selection keeps some and drops some
        # the only way to the same answer without the entry: every target in every list
        ref, rbts = s.align_batch(qa, q3, [E.all_targets()] * nq, identity=ident, with_backtrace=True)
        for q in range(nq):
            assert res[q].tobytes() == ref[q].tobytes() and bts[q] == rbts[q], (atype, name, "align_batch over range(n)", q)
    finally:
        s.close()


def test_efwd_pair_moves_the_named_hit_across_the_cutoff(env):
    """-e AT a hit's forward e-value keeps it, the next double below drops it on the device: one survivor fewer for the named query (and its ties)"""
    for atype in E.ATYPES:
        F = env["frozen"][atype]
        a, b = F.survivors("efwd_eq")[E.NAMED_QUERY], F.survivors("efwd_below")[E.NAMED_QUERY]
        assert a > b >= 1, (atype, a, b)


def test_max_rejected_is_refused_by_name_and_a_good_call_follows(env):
    w = env["w"]
    par = make_params(2, env["frozen"][2].params("default"))
    par.maxRejected = 5
    s = api.Search(env["ctx"], par, keys=w["keys"])
    try:
        with pytest.raises(api.FsgpuError) as e:
            s.exhaustive_batch([w["queries"][0][0]], [w["queries"][0][1]])
        assert e.value.rc == api.FSGPU_E_UNSUPPORTED and "--max-rejected" in str(e.value)
    finally:
        s.close()
    par.maxRejected = INT_MAX
    s = api.Search(env["ctx"], par, keys=w["keys"])
    try:
        res, bts = s.exhaustive_batch([w["queries"][0][0]], [w["queries"][0][1]], identity=[w["identity"][0]], with_backtrace=True)
        want, cigars = env["frozen"][2].records("default", 0)
        same_records(res[0], bts[0], want, cigars, "after the refusal")
        assert s.exhaustive_batch([], []) == []
    finally:
        s.close()


# ---- the module against the reference binary's own exhaustive search --------------------------------------------------------------------------------------
@pytest.fixture()
def scop(tmp_path):
    work = tmp_path / "scop"
    work.mkdir()
    for f in os.listdir(SCOP):
        if f.startswith("db"):
            shutil.copy(os.path.join(SCOP, f), work / f)
    for link, target in SCOP_MANIFEST["links"].items():
        if not os.path.lexists(work / link):
            os.symlink(str(work / target), str(work / link))
    return work


# both spellings on every frozen run; that the flag wins over the mode, and the bare flag, once
_MODULE_RUNS = [(n, how) for n in sorted(REF_RUNS["runs"]) if n not in REF_RUNS["target"] for how in ("--prefilter-mode 2", "--exhaustive-search 1")] + \
               [("ref_t2_e10", "--exhaustive-search 1 --prefilter-mode 0"), ("ref_t0_e1e-3", "--exhaustive-search")]


@pytest.mark.parametrize("name,how", _MODULE_RUNS)
def test_module_equals_the_reference_binary(scop, name, how):
    out = str(scop / "mine")
    cmd = [BIN, "search", str(scop / "db"), str(scop / "db"), out] + how.split() + ["-a", "1", "--sort-by-structure-bits", "0", "--threads", "1", "-v", "1"] + REF_RUNS["runs"][name]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    for ext in ("", ".index", ".dbtype"):
        assert open(out + ext, "rb").read() == open(os.path.join(E.GOLD, name + ext), "rb").read(), (name, how, ext or "data")
    assert os.path.getsize(out) > 1000


def test_module_on_the_padded_target_and_two_threads(scop):
    """the branch feeds the same align path as the other modes: the padded target (the reference's own run against it: makepaddedseqdb renumbers the
    keys) and several host threads"""
    name = "ref_t2_e10_pad"
    assert REF_RUNS["target"][name] == "db_pad"
    out = str(scop / "mine_pad")
    cmd = [BIN, "search", str(scop / "db"), str(scop / "db_pad"), out, "--exhaustive-search", "1", "-a", "1", "--sort-by-structure-bits", "0", "--threads", "2", "-v", "1"] + REF_RUNS["runs"][name]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    from test_scop_golden import read_db
    assert read_db(out) == read_db(os.path.join(E.GOLD, name))


@pytest.mark.parametrize("args,needle", [
    (["--prefilter-mode", "2", "--max-rejected", "5"], "--max-rejected is not supported in the exhaustive mode"),
    (["--exhaustive-search", "1", "--max-rejected", "2147483647"], "--max-rejected is not supported in the exhaustive mode"),
    (["--prefilter-mode", "2", "PREF"], "<outPrefDB> is not written in the exhaustive mode"),
    (["--exhaustive-search", "1", "PREF"], "<outPrefDB> is not written in the exhaustive mode"),
])
def test_module_refusals_print_their_messages(scop, args, needle):
    args = [str(scop / "pref") if a == "PREF" else a for a in args]
    pos = [a for a in args if not a.startswith("-") and os.sep in a]
    flags = [a for a in args if a not in pos]
    r = subprocess.run([BIN, "search", str(scop / "db"), str(scop / "db"), str(scop / "out")] + pos + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 1 and needle in r.stderr, r.stderr
    assert not os.path.exists(scop / "out.index")

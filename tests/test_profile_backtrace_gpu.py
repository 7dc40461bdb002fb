"""fsgpu_profile_backtrace (k_pbtrace.hpp: the reverse pass and the banded trace-back of profile-query hits on the device) and the host path that uses it
(fshost_search_align_batch_profile, FSGPU_PROFILE_BACKTRACE).  The entry is held to the frozen answers of the independent model on the task set of
tests/pbt_cases.py (tests/golden/profile_bt_v1): status, start cell, identity count, M / I / D string and final band width of every task, exactly, under
shuffling, duplication and splitting, under a byte budget that forces several launches and under one that is too small for the largest task.  The host
path is held to the frozen answers of tests/profile_cases.py (tests/golden/profile_align_v1) for every parameter set with the switch unset, 1 and 0, and
the modules to the reference's result DBs of tests/golden/profile_v1 both ways.  Nothing here runs the model."""
import functools
import os

import numpy as np
import pytest

import pbt_cases as B
import profile_cases as K
import test_profile_modules_gpu as M
from foldseek_amd import api, synth
from test_align_entries_gpu import make_params as _align_params, pack, same_records

pytestmark = pytest.mark.gpu
FIELDS = ("status", "qStart", "dbStart", "identicalAA", "band", "backtrace")
E_ARG, E_NODB = -1, -3


@functools.lru_cache(maxsize=None)
def frozen():
    return B.Frozen()


@functools.lru_cache(maxsize=None)
def align_frozen():
    return K.Frozen()


def want(k):
    a = frozen().answer(k)
    return dict(status=a["status"], qStart=a["qStart"], dbStart=a["dbStart"], identicalAA=a["ids"], band=a["band"], backtrace=a["path"])


def need(k):
    """scratch bytes of task k (include/fsgpu.h): one direction byte per cell of the band it ends with, qLen x min(2 band + 1, dbLen), and 8 bytes per line
    cell for lines beyond 1024 cells (the reverse pass's line is the prefix qEnd + 1, the banded pass's the rectangle's width), in 256-byte units"""
    up = lambda x: (int(x) + 255) // 256 * 256  # noqa: E731
    t, a = frozen().tasks[k], frozen().answer(k)
    rev = up(8 * (int(t[2]) + 1)) if int(t[2]) + 1 > 1024 else 0
    if a["status"] == 2:
        return rev
    q_len, db_len = int(t[2]) - a["qStart"] + 1, int(t[3]) - a["dbStart"] + 1
    return max(rev, up(q_len * min(2 * a["band"] + 1, db_len)) + (up(8 * db_len) if db_len > 1024 else 0))


@pytest.fixture(scope="module")
def env():
    w = B.world()
    ctx = api.Context(0)
    ctx.load_db(pack(w["raw"]))
    queries = []
    for ea, e3 in w["entries"]:
        codes, _, prof_a, _ = api.profile_decode(ea)
        _, _, prof_3, _ = api.profile_decode(e3)
        queries.append((prof_a, prof_3, codes))
    yield dict(w=w, ctx=ctx, queries=queries)
    ctx.close()


def call(env, idx, gaps):
    F = frozen()
    return env["ctx"].profile_backtrace(env["queries"], [tuple(int(x) for x in F.tasks[k][:5]) for k in idx], gaps[0], gaps[1])


def same(got, idx, what):
    for g, k in zip(got, idx):
        w = want(k)
        assert {f: g[f] for f in FIELDS} == w, (what, k, frozen().names[k], frozen().tasks[k].tolist(), {f: g[f] for f in FIELDS[:5]}, {f: w[f] for f in FIELDS[:5]})


@pytest.mark.parametrize("gaps", sorted(frozen().by_gaps()))
def test_every_frozen_task(env, gaps, monkeypatch):
    monkeypatch.delenv("FSGPU_PBT_BYTES", raising=False)
    idx = frozen().by_gaps()[gaps]
    got = call(env, idx, gaps)
    assert not any(g["status"] == 0 for g in got)
    same(got, idx, "one call")
    last = env["ctx"].profile_backtrace_last()
    st = np.bincount([want(k)["status"] for k in idx], minlength=4)
    assert last["status"] == st.tolist() and last["launches"] >= 2 and last["band_launches"] >= 1 and last["device_ms"] > 0 and last["scratch_bytes"] > 0, last


def test_shuffled_duplicated_and_split(env, monkeypatch):
    monkeypatch.delenv("FSGPU_PBT_BYTES", raising=False)
    gaps = (10, 1)
    idx = frozen().by_gaps()[gaps]
    rng = np.random.default_rng(7)
    mixed = [idx[i] for i in rng.permutation(len(idx))] + [idx[i] for i in rng.integers(0, len(idx), 40)]
    cut = len(mixed) // 3
    same(call(env, mixed[:cut], gaps), mixed[:cut], "first part")
    same(call(env, mixed[cut:], gaps), mixed[cut:], "second part")
    assert call(env, [], gaps) == [] and env["ctx"].profile_backtrace_last()["launches"] == 0
    same(call(env, idx[:5], gaps), idx[:5], "after an empty call")


def test_refusals_launch_nothing_and_leave_the_results(env):
    F, ctx, q = frozen(), env["ctx"], env["queries"]
    k = F.names.index("piece")
    good = tuple(int(x) for x in F.tasks[k][:5])
    qi, ti, L, T = good[0], good[1], len(q[good[0]][2]), len(env["w"]["raw"][good[1]][0])
    n_targets = len(env["w"]["raw"])
    bad = {"query index": ((len(q),) + good[1:], (10, 1)), "query index -1": ((-1,) + good[1:], (10, 1)),
           "qEnd == L": ((qi, ti, L, good[3], good[4]), (10, 1)), "qEnd < 0": ((qi, ti, -1, good[3], good[4]), (10, 1)),
           "dbEnd == length": ((qi, ti, good[2], T, good[4]), (10, 1)), "dbEnd < 0": ((qi, ti, good[2], -1, good[4]), (10, 1)),
           "target id": ((qi, n_targets) + good[2:], (10, 1)), "open == extend": (good, (3, 3)), "open < extend": (good, (1, 2)), "extend 0": (good, (10, 0))}
    for what, (task, gaps) in bad.items():
        with pytest.raises(api.FsgpuError) as e:
            ctx.profile_backtrace(q, [good, task, good], gaps[0], gaps[1])
        assert e.value.rc == E_ARG and set(e.value.res) == {0xF9}, (what, e.value.rc, str(e.value))
    with pytest.raises(api.FsgpuError, match="below 32768") as e:          # the limit of the SW entries the tasks come from
        ctx.profile_backtrace(q, [good], 32768, 1)
    assert e.value.rc == api.FSGPU_E_UNSUPPORTED and set(e.value.res) == {0xF9}
    same(call(env, [k], (10, 1)), [k], "after the refusals")
    # a database loaded without AA sequences
    w = env["w"]
    db = pack(w["raw"][:40])
    other = api.Context(0)
    try:
        other.load_db(synth.PaddedDB(db.data3di, None, db.offsets, db.lengths))
        with pytest.raises(api.FsgpuError, match="without AA sequences") as e:
            other.profile_backtrace(q, [(0, 1, 0, 0, 1)])
        assert e.value.rc == E_NODB and set(e.value.res) == {0xF9}
    finally:
        other.close()


def test_a_small_budget_takes_several_launches(env, monkeypatch):
    gaps = (10, 1)
    idx = frozen().by_gaps()[gaps]
    monkeypatch.delenv("FSGPU_PBT_BYTES", raising=False)
    call(env, idx, gaps)
    plain = env["ctx"].profile_backtrace_last()
    monkeypatch.setenv("FSGPU_PBT_BYTES", str(max(need(k) for k in idx)))
    got = call(env, idx, gaps)
    assert not any(g["status"] == 0 for g in got)
    same(got, idx, "one launch's budget = the largest task's need")
    last = env["ctx"].profile_backtrace_last()
    assert last["band_launches"] > max(plain["band_launches"], 1) and last["launches"] > plain["launches"] and last["scratch_bytes"] <= max(need(k) for k in idx), (plain, last)


def test_a_budget_below_the_largest_task_hands_it_back(env, monkeypatch):
    gaps = (10, 1)
    idx = frozen().by_gaps()[gaps]
    top = max(need(k) for k in idx)
    monkeypatch.setenv("FSGPU_PBT_BYTES", str(top - 1))
    got = call(env, idx, gaps)
    big = [i for i, k in enumerate(idx) if need(k) == top]
    assert big and all(got[i]["status"] == 0 and got[i]["backtrace"] == "" for i in big)
    rest = [i for i in range(len(idx)) if i not in set(big)]
    same([got[i] for i in rest], [idx[i] for i in rest], "the others")
    assert env["ctx"].profile_backtrace_last()["status"][0] == len(big)


# ---- the host path -------------------------------------------------------------------------------------------------------------------------------------------------
def make_params(P):
    par = _align_params(2, P)
    par.gapOpen, par.gapExtend, par.addBacktrace = P["gapOpen"], P["gapExtend"], P["addBacktrace"]
    return par


@pytest.fixture(scope="module")
def world_env():
    w = K.world()
    ctx = api.Context(0)
    ctx.load_db(pack(w["targets"]))
    yield dict(w=w, ctx=ctx)
    ctx.close()


GATES = ("not coverable", "end coverage", "e-value fwd", "e-value diff", "not reached: max-accept", "not reached: max-rejected")


def batch_equals_frozen(env, s, name, what):
    w, F = env["w"], align_frozen()
    res, bts = s.align_batch_profile(w["entries"], w["lists"], identity=w["identity"])
    for q in range(len(F.n)):
        recs, cigars, _ = F.records(name, q)
        same_records(res[q], bts[q], recs, cigars, (name, what, q))


@pytest.mark.parametrize("name", align_frozen().names)
def test_batch_entry_equals_the_model_with_the_switch_unset_on_and_off(world_env, name, monkeypatch):
    F = align_frozen()
    P = F.params(name)
    limited = P["maxAccept"] != K.INT_MAX or P["maxRejected"] != K.INT_MAX
    passing = sum(o not in GATES for q in range(len(F.n)) for o in F.outcomes(name, q))
    monkeypatch.delenv("FSGPU_PBT_BYTES", raising=False)
    s = api.Search(world_env["ctx"], make_params(P), keys=world_env["w"]["keys"])
    try:
        for mode in (None, "1", "0"):
            if mode is None:
                monkeypatch.delenv("FSGPU_PROFILE_BACKTRACE", raising=False)
            else:
                monkeypatch.setenv("FSGPU_PROFILE_BACKTRACE", mode)
            batch_equals_frozen(world_env, s, name, mode)
            assert s.backtrace_counts() == ((0, 0) if mode == "0" or limited else (passing, passing)), (name, mode, s.backtrace_counts(), passing)
            if mode != "0" and not limited and passing:
                assert world_env["ctx"].profile_backtrace_last()["status"][0] == 0
    finally:
        s.close()


@pytest.mark.parametrize("name", ["default", "e_all", "gap8_2"])
def test_tasks_the_device_hands_back_reach_the_host_path(world_env, name, monkeypatch):
    """a budget of 16 KiB: the wide rectangles come back with status 0, gateAlign answers them one by one, the records do not change"""
    F = align_frozen()
    monkeypatch.delenv("FSGPU_PROFILE_BACKTRACE", raising=False)
    monkeypatch.setenv("FSGPU_PBT_BYTES", "16384")
    s = api.Search(world_env["ctx"], make_params(F.params(name)), keys=world_env["w"]["keys"])
    try:
        batch_equals_frozen(world_env, s, name, "small budget")
        on_device, everything = s.backtrace_counts()
        handed_back = world_env["ctx"].profile_backtrace_last()
        assert 0 < on_device < everything and everything - on_device == handed_back["status"][0], (on_device, everything, handed_back)
    finally:
        s.close()


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------------------------------
def _run(cmd, mode):
    env = dict(os.environ, FSGPU_PROFILE_BACKTRACE=mode)
    env.pop("FSGPU_PBT_BYTES", None)
    return M.subprocess.run(cmd, stdout=M.subprocess.PIPE, stderr=M.subprocess.PIPE, text=True, env=env)


@pytest.fixture()
def work(tmp_path):
    w = tmp_path / "profile"
    M.shutil.copytree(M.GOLD, w)
    return w


@pytest.mark.parametrize("mode", ("0", "1"))
@pytest.mark.parametrize("name", M._ALIGN)
def test_structurealign_equals_the_reference_both_ways(work, name, mode):
    run = M.RUNS[name]
    out = str(work / f"mine_{name}")
    r = _run([M.BIN, "structurealign"] + [str(work / p) for p in run["positional"]] + [out] + M._with(run["parameters"], **{"--threads": 4}) + ["--gpus", "1"], mode)
    assert r.returncode == 0, r.stderr
    M._same_files(out, str(work / name))


@pytest.mark.parametrize("mode", ("0", "1"))
@pytest.mark.parametrize("name, query, target, pref", (("paln_t2_a", "profile_0", "db", "ppref"), ("caln_t2_a", "cprof", "ctarget", "cpref")))
def test_search_equals_the_reference_both_ways(work, name, query, target, pref, mode):
    out, outp = str(work / f"mine_search_{name}"), str(work / f"mine_search_{name}_pref")
    r = _run([M.BIN, "search", str(work / query), str(work / target), out, outp, "--prefilter-mode", "1", "--min-ungapped-score", "15", "-a", "1", "--alignment-type", "2",
              "--sort-by-structure-bits", "0", "--threads", "4", "--gpus", "1", "--max-seqs", "1000", "-e", "10"], mode)
    assert r.returncode == 0, r.stderr
    M._same_files(outp, str(work / pref))
    M._same_files(out, str(work / name))

"""fshost_search_align_profile / _align_batch_profile and fshost_search_prefilter_profile / _prefilter_batch_profile on the seeded world of
tests/profile_cases.py, whose gates are decided at their edges.  Everything expected of the alignment entries was frozen by
tests/golden/make_profile_align_golden.py (tests/golden/profile_align_v1): the answers of tests/align_model.py's accept loop over tests/profile_model.py's
ProfileWorld, which tests/test_profile_cases.py holds to the reference binary's runs on this very world.  Compared exactly, for every parameter set and in both
branches of the batch body (one submission for both directions; forward pass, needsReversePass, reversed pass over the selection): count, order and every
record field as bit patterns, every CIGAR, the forward and reversed Smith-Waterman records of every pair, the number of pairs whose reversed score was
looked at (stats()[6]), the reverse selection (stats()[7]) and what the last device call planned.  The prefilter entries are held to tests/gapless_model.py,
computed here on the CPU.  Nothing goes through a device transcendental: no tolerance anywhere."""
import functools
import types

import numpy as np
import pytest

import gapless_model as gm
import profile_cases as K
import profile_model as pm
from foldseek_amd import api
from test_align_entries_gpu import FIELDS, as_rows, make_params as _align_params, pack, same_records

pytestmark = pytest.mark.gpu
BRANCHES = {"one submission": "1000000000", "two passes": "0"}          # FSGPU_SW_ONEPASS_PAIRS, read per call


@functools.lru_cache(maxsize=None)
def frozen():
    return K.Frozen()


def make_params(P):
    par = _align_params(2, P)
    par.gapOpen, par.gapExtend, par.addBacktrace = P["gapOpen"], P["gapExtend"], P["addBacktrace"]
    return par


@pytest.fixture(scope="module")
def env():
    w = K.world()
    ctx = api.Context(0)
    ctx.load_db(pack(w["targets"]))
    assert ctx.residues == sum(len(a) for a, _ in w["targets"])          # what the model's e-values were computed with
    yield dict(w=w, ctx=ctx)
    ctx.close()


def plan_of(ctx):
    p = ctx.sw3_last_plan()
    return sum(p["pairs"].values()), p["profile_pairs"], p["rerun_pairs"]


def check_batch(env, s, name, branch, monkeypatch):
    """one align_batch_profile call of all eight lists against the frozen answers of set `name`; -> (records, backtraces) per query"""
    w, F = env["w"], frozen()
    monkeypatch.setenv("FSGPU_SW_ONEPASS_PAIRS", BRANCHES[branch])
    before = s.stats()[6]
    res, bts = s.align_batch_profile(w["entries"], w["lists"], identity=w["identity"])
    st, (k3_pairs, long_pairs, _) = s.stats(), plan_of(env["ctx"])
    total = int(sum(F.n))
    fwd, rev = s.last_sw(total)
    for q in range(len(F.n)):
        want, cigars, _ = F.records(name, q)
        same_records(res[q], bts[q], want, cigars, (name, branch, "align_batch_profile", q))
    assert (as_rows(fwd) == F.fwd(name)).all(), (name, branch, "forward records")
    assert (as_rows(rev) == F.rev(name)).all(), (name, branch, "reversed records, all zero where the reference does not reverse")
    assert st[6] - before == F.looked(name).sum(), (name, branch, "pairs whose reversed score was looked at")
    assert st[7] == F.selection(name), (name, branch, "reverse selection")
    # what the last multi-query call ran: every pair in both directions, or the reversed pass over the selection; the 1025-position query's pairs take
    # the profile-based path (the trace-backs' reverse passes are single-pair calls of another entry and leave the plan alone)
    long_q = K.Q_LENGTHS.index(1025)
    if branch == "one submission":
        assert (k3_pairs, long_pairs) == (total - F.n[long_q], F.n[long_q]), (name, branch, k3_pairs, long_pairs)
    elif F.selection(name):
        assert long_pairs == F.selection(name, long_q) and k3_pairs == F.selection(name) - long_pairs, (name, branch, k3_pairs, long_pairs)
    return res, bts


@pytest.mark.parametrize("name", frozen().names)
def test_batch_entry_equals_the_model_in_both_branches(env, name, monkeypatch):
    """every parameter set: thresholds AT a hit's value and one representable number beyond, the three coverage and identity modes, the no-cigar rule
    (the covi sets: the identity hit keeps its start cell and loses its cigar), the limits, -a 0, gap costs 8 / 2, and every pair backtraced (e_all)"""
    F = frozen()
    s = api.Search(env["ctx"], make_params(F.params(name)), keys=env["w"]["keys"])
    try:
        out = {b: check_batch(env, s, name, b, monkeypatch) for b in BRANCHES}
        a, b = out["one submission"], out["two passes"]
        assert [r.tobytes() for r in a[0]] == [r.tobytes() for r in b[0]] and a[1] == b[1]
        if name == "default":
            assert 0 < F.selection(name) < sum(F.n)                          # the two-pass branch has something to leave out
    finally:
        s.close()


@pytest.mark.parametrize("name", ["default", "covi0_next", "sid1_eq", "rej2"])
def test_single_entry_is_the_batch_member(env, name, monkeypatch):
    """fshost_search_align_profile, one query at a time: byte-equal to the batch call's member, and the model's"""
    w, F = env["w"], frozen()
    monkeypatch.delenv("FSGPU_SW_ONEPASS_PAIRS", raising=False)
    s = api.Search(env["ctx"], make_params(F.params(name)), keys=w["keys"])
    try:
        res, bts = s.align_batch_profile(w["entries"], w["lists"], identity=w["identity"])
        for q in range(len(F.n)):
            before = s.stats()[6]
            one, one_bt = s.align_profile(w["entries"][q][0], w["entries"][q][1], w["lists"][q], identity=w["identity"][q])
            assert b"".join(np.ascontiguousarray(one[f]).tobytes() for f in FIELDS) == b"".join(np.ascontiguousarray(res[q][f]).tobytes() for f in FIELDS), (name, q)
            assert one_bt == bts[q], (name, q)
            want, cigars, _ = F.records(name, q)
            same_records(one, one_bt, want, cigars, (name, "align_profile", q))
            assert s.stats()[6] - before == F.looked(name)[q] and s.stats()[7] == F.selection(name, q), (name, q)
            fwd, rev = s.last_sw(F.n[q])
            assert (as_rows(fwd) == F.fwd(name, q)).all() and (as_rows(rev) == F.rev(name, q)).all(), (name, q)
    finally:
        s.close()


@pytest.mark.parametrize("branch", sorted(BRANCHES))
@pytest.mark.parametrize("name", ["default", "e_all"])
def test_saturating_list(env, name, branch, monkeypatch):
    """600 positions of the constant maximum against the 1025-residue target: 37200 in both directions, the int16 pass saturates and the int32 re-run
    decides -- in the two multi-query passes, and (e_all) in the reverse pass of the trace-back, whose 600 x 600 rectangle gives 600M"""
    w, F = env["w"], frozen()
    q = K.SAT_QUERY
    monkeypatch.setenv("FSGPU_SW_ONEPASS_PAIRS", BRANCHES[branch])
    s = api.Search(env["ctx"], make_params(F.params(name)), keys=w["keys"])
    try:
        res, bts = s.align_batch_profile([w["entries"][q]], [w["lists"][q]], identity=[-1])
        assert plan_of(env["ctx"]) == (2 if branch == "one submission" else F.selection(name, q), 0, 1)
        want, cigars, _ = F.records(name, q)
        same_records(res[0], bts[0], want, cigars, (name, branch, "saturating"))
        fwd, rev = s.last_sw(2)
        assert (as_rows(fwd) == F.fwd(name, q)).all() and (as_rows(rev) == F.rev(name, q)).all()
        assert as_rows(fwd)[0].tolist() == [37200, 599, 599, 2] and as_rows(rev)[0].tolist()[::3] == [37200, 2] and F.selection(name, q) == 2
    finally:
        s.close()


def test_refusals_leave_context_and_handle_usable(env, monkeypatch):
    """gap costs 1 / 1 and --alt-ali are refused by name, in both entries, before anything runs; a target id past the database is refused per call.  The
    handle that refused the call and a default handle on the same context then equal the model."""
    w, F = env["w"], frozen()
    q = K.NAMED_QUERY
    ea, e3 = w["entries"][q]
    for change, rc, words in ((dict(gapOpen=1, gapExtend=1), api.FSGPU_E_UNSUPPORTED, "gapOpen > gapExtend >= 1 (got 1 / 1)"),
                              (dict(altAlignment=1), api.FSGPU_E_UNSUPPORTED, "--alt-ali with a profile query")):
        s = api.Search(env["ctx"], make_params(dict(F.params("default"), **change)), keys=w["keys"])
        try:
            with pytest.raises(api.FsgpuError) as e:
                s.align_profile(ea, e3, w["lists"][q], identity=w["identity"][q])
            assert e.value.rc == rc and words in str(e.value)
            with pytest.raises(api.FsgpuError, match="--alt-ali|gapOpen"):
                s.align_batch_profile(w["entries"], w["lists"], identity=w["identity"])
        finally:
            s.close()
    s = api.Search(env["ctx"], make_params(F.params("default")), keys=w["keys"])
    try:
        bad = w["lists"][q].copy()
        bad[1] = len(w["targets"])
        for branch in BRANCHES:
            monkeypatch.setenv("FSGPU_SW_ONEPASS_PAIRS", BRANCHES[branch])
            with pytest.raises(api.FsgpuError, match="target id out of range"):
                s.align_profile(ea, e3, bad, identity=w["identity"][q])
            with pytest.raises(api.FsgpuError, match="target id out of range"):
                s.align_batch_profile([w["entries"][0], (ea, e3)], [w["lists"][0], bad], identity=[w["identity"][0], w["identity"][q]])
            check_batch(env, s, "default", branch, monkeypatch)
    finally:
        s.close()


# ---- the prefilter entries ---------------------------------------------------------------------------------------------------------------------------------------------
def _gapless_db():
    t = [x[1] for x in K.world()["targets"]]
    lens = np.array([len(x) for x in t], np.int64)
    return types.SimpleNamespace(data3di=np.concatenate(t), offsets=np.concatenate([[0], np.cumsum(lens)])[:-1], lengths=lens)


def _gapless_scores():
    packed = gm.pack(_gapless_db())
    return [gm.scores(prof, pm.cap(prof), packed) for prof in (pm.decode(e[1])[2] for e in K.world()["entries"])]


GAPLESS = _gapless_scores()                                # expected values: tests/gapless_model.py on the CPU, once, on this small database
MIN_SCORE = 15


def _tie_cut():
    """a list length that cuts the named query's list inside a run of equal scores (the order inside it is by id)"""
    full = gm.select(GAPLESS[K.NAMED_QUERY], MIN_SCORE, K.world()["identity"][K.NAMED_QUERY], len(GAPLESS[K.NAMED_QUERY]))
    cuts = [k for k in range(3, len(full) - 1) if full["score"][k - 1] == full["score"][k] and full["score"][k - 2] == full["score"][k]]
    assert cuts, full["score"]
    return cuts[len(cuts) // 2]


@pytest.mark.parametrize("min_score, max_res", [(MIN_SCORE, 1000), (MIN_SCORE, _tie_cut()), (230, 1000)], ids=["all", "cut inside a tie", "identity alone"])
def test_prefilter_entries_with_identity_ids(env, min_score, max_res):
    """the hit lists of both entries: score above the threshold or the identity id, by (score descending, id ascending), cut at maxResListLen.  With the
    threshold above the cap of a profile that holds a negative score (255 - 32) the identity id is all that is left."""
    w = env["w"]
    par = api.default_params()
    par.minDiagScoreThr, par.maxResListLen = min_score, max_res
    s = api.Search(env["ctx"], par, keys=w["keys"])
    try:
        want = [gm.select(GAPLESS[q], min_score, w["identity"][q], max_res) for q in range(len(w["entries"]))]
        if max_res < 1000:
            full = gm.select(GAPLESS[K.NAMED_QUERY], min_score, w["identity"][K.NAMED_QUERY], 1000)
            assert len(want[K.NAMED_QUERY]) == max_res < len(full) and full["score"][max_res - 1] == full["score"][max_res]
        if min_score == 230:
            assert all(want[q]["id"].tolist() == [w["identity"][q]] for q in range(7)) and all(GAPLESS[q].max() <= 223 for q in range(7))
        got = s.prefilter_batch_profile([e[1] for e in w["entries"]], identity=w["identity"])
        for q, e in enumerate(w["entries"]):
            assert len(got[q]) == len(want[q]) and (got[q]["id"] == want[q]["id"]).all() and (got[q]["score"] == want[q]["score"]).all(), ("batch", q, got[q][:6], want[q][:6])
            one = s.prefilter_profile(e[1], identity=w["identity"][q])
            assert one.tobytes() == got[q].tobytes(), ("single", q)
        # without the identity ids the lists lose exactly that hit where its score does not carry it
        if min_score == 230:
            plain = s.prefilter_batch_profile([e[1] for e in w["entries"]])
            assert all(len(plain[q]) == 0 for q in range(7))
    finally:
        s.close()

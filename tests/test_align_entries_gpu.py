"""fshost_search_align and fshost_search_align_batch against the independent model of structurealign's accept loop (tests/align_model.py), on the seeded world
of tests/align_cases.py whose gates are decided at their edges.  Everything expected here was frozen by tests/golden/make_align_golden.py
(tests/golden/align_v1); the model is held to the reference binary's frozen runs by tests/test_align_model.py, which also pins what the world contains.
Compared exactly, for every parameter set and both alignment types: count, order and every record field as bit patterns, every CIGAR, the forward and
reversed Smith-Waterman records of every pair, the number of pairs whose reversed score was looked at (stats()[6]) and the reverse selection (stats()[7]).
Nothing here goes through a device transcendental: no tolerance anywhere."""
import numpy as np
import pytest

import align_cases as K
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

FIELDS = ("dbKey", "score", "qcov", "dbcov", "seqId", "eval", "alnLength", "qStartPos", "qEndPos", "qLen", "dbStartPos", "dbEndPos", "dbLen")
BACKTRACED = ("accepted", "accepted as identity", "seq id", "start coverage", "aln length", "e-value crit", "tm drop", "lddt drop")
INT_MAX = 2147483647


def pack(targets):
    """PaddedDB in id order, every entry padded to a multiple of four with X"""
    lens = np.array([len(a) for a, _ in targets], np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
    for k, (a, s) in enumerate(targets):
        d3[off[k]:off[k] + lens[k]] = s
        da[off[k]:off[k] + lens[k]] = a
    return synth.PaddedDB(d3, da, off, lens)


@pytest.fixture(scope="module")
def env():
    w = K.world()
    db = pack(w["targets"])
    ctx = api.Context(0)
    ctx.load_db(db)
    assert ctx.residues == sum(len(a) for a, _ in w["targets"])          # what the model's e-values were computed with
    frozen = {t: K.Frozen(t) for t in K.ATYPES}
    yield dict(w=w, ctx=ctx, frozen=frozen, db=db)
    ctx.close()


def make_params(atype, P):
    par = api.default_params()
    par.alignmentType, par.addBacktrace = atype, 1
    par.evalThr, par.covThr, par.covMode = P["evalThr"], P["covThr"], P["covMode"]
    par.seqIdThr, par.seqIdMode, par.alnLenThr = P["seqIdThr"], P["seqIdMode"], P["alnLenThr"]
    par.maxAccept, par.maxRejected, par.altAlignment = P["maxAccept"], P["maxRejected"], P["altAlignment"]
    assert np.float32(par.covThr) == np.float32(P["covThr"]) and np.float32(par.seqIdThr) == np.float32(P["seqIdThr"]) and par.evalThr == P["evalThr"]
    return par


def compress(bt):
    """run-length text of a backtrace ('MMI' -> '2M1I'); a text that already carries counts is left alone"""
    if any(ch.isdigit() for ch in bt):
        return bt
    out, k = "", 0
    while k < len(bt):
        e = k
        while e < len(bt) and bt[e] == bt[k]:
            e += 1
        out += f"{e - k}{bt[k]}"
        k = e
    return out


def same_records(got, bts, want, cigars, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for f in FIELDS:
        g, x = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert g.dtype == x.dtype, (where, f)
        if g.tobytes() != x.tobytes():
            k = int(np.flatnonzero(g != x)[0]) if (g != x).any() else 0
            raise AssertionError(f"{where}: field {f} of record {k}: got {got[k]}, want {want[k]}")
    assert [compress(b) for b in bts] == list(cigars), where


def as_rows(sw):
    return np.ascontiguousarray(sw).view(np.int32).reshape(-1, 4)


def check_set(env, atype, name, setup=None, before_call=None):
    """both entries against the frozen model for one parameter set; -> backtrace_counts() of the batch call.  setup(search, P): once, after the handle is
    made; before_call(search, query indices): before every align / align_batch call"""
    w, F = env["w"], env["frozen"][atype]
    P = F.params(name)
    s = api.Search(env["ctx"], make_params(2 if atype == "ca" else atype, P), keys=w["keys"])
    before_call = before_call or (lambda search, qs: None)
    try:
        if setup:
            setup(s, P)
        nq = len(w["queries"])
        # ---- one query at a time
        for q in range(nq):
            qa, q3 = w["queries"][q]
            before = s.stats()[6]
            before_call(s, [q])
            res, bts = s.align(qa, q3, w["lists"][q], identity=w["identity"][q], with_backtrace=True)
            want, cigars, _ = F.records(name, q)
            same_records(res, bts, want, cigars, (atype, name, "align", q))
            assert s.stats()[6] - before == F.looked(name)[q], (atype, name, "align", q, "pairs whose reversed score was looked at")
            fwd, rev = s.last_sw(len(w["lists"][q]))
            assert (as_rows(fwd) == F.fwd(q)).all(), (atype, name, "align", q, "forward records")
            sel = F.rev(name, q)[:, 3] != 0                    # this entry reverses every pair: compared where the reference reverses
            assert (as_rows(rev)[sel] == F.rev(name, q)[sel]).all(), (atype, name, "align", q, "reversed records")
        # ---- all queries in one call
        before = s.stats()[6]
        before_call(s, list(range(nq)))
        res, bts = s.align_batch([x[0] for x in w["queries"]], [x[1] for x in w["queries"]], w["lists"], identity=w["identity"], with_backtrace=True)
        counts = s.backtrace_counts()
        st = s.stats()
        for q in range(nq):
            want, cigars, _ = F.records(name, q)
            same_records(res[q], bts[q], want, cigars, (atype, name, "align_batch", q))
        assert st[6] - before == F.looked(name).sum(), (atype, name, "align_batch", "pairs whose reversed score was looked at")
        fwd, rev = s.last_sw(int(sum(F.n)))
        assert (as_rows(fwd) == F.z["fwd"]).all(), (atype, name, "align_batch", "forward records")
        assert (as_rows(rev) == F.z[f"{name}/rev"]).all(), (atype, name, "align_batch", "reversed records, all zero where the reference does not reverse")
        assert st[7] == (F.z[f"{name}/rev"][:, 3] != 0).sum(), (atype, name, "align_batch", "reverse selection")
        # the result capacity n * (1 + alt) of the ninth list
        if name == "alt2":
            assert len(res[nq - 1]) == len(w["lists"][nq - 1]) * 3
        return counts
    finally:
        s.close()


def _set_names():
    return K.Frozen(2).names


@pytest.mark.parametrize("atype", K.ATYPES)
@pytest.mark.parametrize("name", _set_names())
def test_entries_equal_the_model(env, atype, name, monkeypatch):
    """every parameter set: thresholds AT a hit's value and one representable number beyond, all coverage and identity modes, accept / reject limits, --alt-ali"""
    monkeypatch.delenv("FSGPU_DEVICE_BACKTRACE", raising=False)
    F = env["frozen"][atype]
    P = F.params(name)
    on_dev, total = check_set(env, atype, name)
    backtraced = sum(c for o, c in F.count(name).items() if o in BACKTRACED)
    if P["maxAccept"] != INT_MAX or P["maxRejected"] != INT_MAX:
        # a list that can be cut short computes its backtraces hit by hit, where the loop reaches them: nothing is computed ahead
        assert (on_dev, total) == (0, 0), (on_dev, total)
    else:
        assert total == backtraced and 0 <= on_dev <= total, (on_dev, total, backtraced)


@pytest.mark.parametrize("atype", K.ATYPES)
@pytest.mark.parametrize("name", ["default", "alt2"])
@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_three_backtrace_answerers(env, atype, name, mode, monkeypatch):
    """host aligner, device aligner, both sharing one list (from a lowered number of hits on): identical records and CIGARs, backtrace_counts() says who answered"""
    monkeypatch.setenv("FSGPU_DEVICE_BACKTRACE", mode)
    if mode == "2":
        monkeypatch.setenv("FSGPU_BT_SHARE_MIN", "128")
    else:
        monkeypatch.delenv("FSGPU_BT_SHARE_MIN", raising=False)
    F = env["frozen"][atype]
    on_dev, total = check_set(env, atype, name)
    backtraced = sum(c for o, c in F.count(name).items() if o in BACKTRACED)
    assert total == backtraced >= 128
    if mode == "0":
        assert on_dev == 0
    elif mode == "1":
        assert 0.9 * total <= on_dev <= total, (on_dev, total)          # blocks beyond the device's passes go back to the host: a handful at most
    else:
        assert 0 <= on_dev <= total


# ---- the two-pass branch ---------------------------------------------------------------------------------------------------------------------------------------------
def fillers(w, n_pairs):
    """short seeded queries (24 .. 64 residues) against the world's targets of at most 64 residues, enough of them for n_pairs pairs"""
    rng = np.random.default_rng(K.SEED + 1)
    short = np.array([i for i, (a, _) in enumerate(w["targets"]) if len(a) <= 64], np.uint32)
    assert len(short) >= 30
    qs, lists, left = [], [], n_pairs
    while left > 0:
        L = int(rng.integers(24, 65))
        if len(qs) % 3 == 0:                                   # a relative of a short target, so that the selection is not empty
            t = w["targets"][int(short[rng.integers(0, len(short))])]
            a, s = np.resize(t[0], L).copy(), np.resize(t[1], L).copy()
        else:
            a, s = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
        ids = short[:min(left, len(short))]
        qs.append((a, s)); lists.append(ids.copy()); left -= len(ids)
    return qs, lists


def _plan_pairs(ctx):
    p = ctx.sw3_last_plan()
    return sum(p["pairs"].values()) + p["profile_pairs"]


def _two_pass_set(F):
    """a coverage gate that empties the reverse selection of at least one model-held query while others keep theirs"""
    for name in F.names:
        P = F.params(name)
        if P["covThr"] > 0 and P["maxAccept"] == INT_MAX and P["maxRejected"] == INT_MAX and P["altAlignment"] == 0:
            per_q = [(F.rev(name, q)[:, 3] != 0).sum() for q in range(len(F.n))]
            if min(per_q) == 0 and sum(x > 0 for x in per_q) >= 2:
                return name
    raise AssertionError("no parameter set empties one query's selection")


@pytest.mark.parametrize("atype,which", [(2, "default"), (0, "default"), (2, "gate")])
def test_two_pass_branch_at_its_threshold(env, atype, which, monkeypatch):
    """one align_batch call of 16 385 pairs: forward pass over all of them, reversed pass over the needsReversePass selection only.  The first nine queries are
    the model's, the rest fillers that must equal the same fillers submitted in calls of at most 16 384 pairs (one submission for both directions)."""
    monkeypatch.delenv("FSGPU_SW_ONEPASS_PAIRS", raising=False)
    w, F = env["w"], env["frozen"][atype]
    name = "default" if which == "default" else _two_pass_set(F)
    P = F.params(name)
    held = int(sum(F.n))
    fq, fl = fillers(w, 16385 - held)
    total = held + sum(len(x) for x in fl)
    assert total == 16385
    qa = [x[0] for x in w["queries"]] + [x[0] for x in fq]
    q3 = [x[1] for x in w["queries"]] + [x[1] for x in fq]
    lists = list(w["lists"]) + fl
    ident = list(w["identity"]) + [-1] * len(fq)
    s = api.Search(env["ctx"], make_params(atype, P), keys=w["keys"])
    try:
        res, bts = s.align_batch(qa, q3, lists, identity=ident, with_backtrace=True)
        plan, sel = _plan_pairs(env["ctx"]), s.stats()[7]
        fwd, rev = s.last_sw(total)
        assert 0 < sel < total and plan == sel, (plan, sel, total)          # the last compact call was the reversed pass over the selection
        nq = len(w["queries"])
        for q in range(nq):
            want, cigars, _ = F.records(name, q)
            same_records(res[q], bts[q], want, cigars, (atype, name, "two-pass", q))
        assert (as_rows(fwd)[:held] == F.z["fwd"]).all() and (as_rows(rev)[:held] == F.z[f"{name}/rev"]).all()
        if which == "gate":
            per_q = [(F.rev(name, q)[:, 3] != 0).sum() for q in range(nq)]
            assert min(per_q) == 0 and max(per_q) > 0
        # the fillers once more, in calls that take the one-pass branch
        half = len(fq) // 2
        got, got_bt, sw_f, sw_r, sel_small = [], [], [], [], 0
        for a, b in ((0, half), (half, len(fq))):
            r2, b2 = s.align_batch([x[0] for x in fq[a:b]], [x[1] for x in fq[a:b]], fl[a:b], with_backtrace=True)
            n = sum(len(x) for x in fl[a:b])
            assert 0 < n <= 16384 and _plan_pairs(env["ctx"]) == n          # one submission, every pair
            f2, v2 = s.last_sw(n)
            got += r2; got_bt += b2; sw_f.append(as_rows(f2)); sw_r.append(as_rows(v2)); sel_small += s.stats()[7]
        for k in range(len(fq)):
            same_records(res[nq + k], bts[nq + k], got[k], [compress(b) for b in got_bt[k]], (atype, name, "filler", k))
        assert (as_rows(fwd)[held:] == np.concatenate(sw_f)).all() and (as_rows(rev)[held:] == np.concatenate(sw_r)).all()
        assert sel_small + (F.z[f"{name}/rev"][:, 3] != 0).sum() == sel
        assert sum(len(r) for r in got) > 0
    finally:
        s.close()


@pytest.mark.parametrize("atype", K.ATYPES)
def test_each_branch_forced_on_the_same_small_call(env, atype, monkeypatch):
    """FSGPU_SW_ONEPASS_PAIRS is read per call: 0 (never one submission) and a huge value (always) on the model's nine lists, byte for byte the same and
    both the model's"""
    w, F = env["w"], env["frozen"][atype]
    name = "cov0_eq"
    s = api.Search(env["ctx"], make_params(atype, F.params(name)), keys=w["keys"])
    try:
        out = {}
        for limit in ("0", "1000000000"):
            monkeypatch.setenv("FSGPU_SW_ONEPASS_PAIRS", limit)
            res, bts = s.align_batch([x[0] for x in w["queries"]], [x[1] for x in w["queries"]], w["lists"], identity=w["identity"], with_backtrace=True)
            total = int(sum(F.n))
            fwd, rev = s.last_sw(total)
            out[limit] = (b"".join(np.ascontiguousarray(r[f]).tobytes() for r in res for f in FIELDS), bts, as_rows(fwd).tobytes(), as_rows(rev).tobytes(), s.stats()[7], _plan_pairs(env["ctx"]))
            for q in range(len(w["queries"])):
                want, cigars, _ = F.records(name, q)
                same_records(res[q], bts[q], want, cigars, (atype, name, limit, q))
            assert as_rows(rev).tobytes() == F.z[f"{name}/rev"].tobytes()
        assert out["0"][:5] == out["1000000000"][:5]
        assert out["0"][5] == out["0"][4] and 0 < out["0"][4] < total and out["1000000000"][5] == total
    finally:
        s.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limits", [False, True])
def test_target_id_out_of_range_is_refused_and_the_handle_lives_on(env, limits):
    """a target id past the database in either entry: the error and its message; the next valid call on the same handle equals the model"""
    w, F = env["w"], env["frozen"][2]
    name = "acc_rej_mix" if limits else "default"
    s = api.Search(env["ctx"], make_params(2, F.params(name)), keys=w["keys"])
    try:
        q = K.NAMED_QUERY
        qa, q3 = w["queries"][q]
        bad = w["lists"][q].copy()
        bad[1] = len(w["targets"])
        with pytest.raises(api.FsgpuError, match="target id out of range"):
            s.align(qa, q3, bad, identity=w["identity"][q])
        with pytest.raises(api.FsgpuError, match="target id out of range"):
            s.align_batch([qa, qa], [q3, q3], [w["lists"][q], bad], identity=[w["identity"][q]] * 2)
        res, bts = s.align(qa, q3, w["lists"][q], identity=w["identity"][q], with_backtrace=True)
        want, cigars, _ = F.records(name, q)
        same_records(res, bts, want, cigars, (name, "align after a refusal"))
        res, bts = s.align_batch([qa], [q3], [w["lists"][q]], identity=[w["identity"][q]], with_backtrace=True)
        same_records(res[0], bts[0], want, cigars, (name, "align_batch after a refusal"))
    finally:
        s.close()


# ---- LDDT / TM thresholds and structure bits at the library level -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env_ca():
    w = K.ca_world()
    ctx = api.Context(0)
    ctx.load_db(pack(w["targets"]))
    yield dict(w=w, ctx=ctx, frozen={"ca": K.Frozen("ca")})
    ctx.close()


def _bind(w):
    def setup(s, P):
        s.set_tm(P["tmThr"], P["tmMode"], bool(P["structureBits"]))
        s.bind_ca(P["lddtThr"], w["ca"])
    return setup


def _query_ca(w):
    return lambda s, qs: s.set_query_ca([w["ca"][q] for q in qs])


@pytest.mark.parametrize("name", K.Frozen("ca").names)
def test_lddt_and_tm_thresholds_and_structure_bits(env_ca, name, monkeypatch):
    """the twelve example structures, every one against every one: the TM threshold in its three modes, the LDDT threshold (dbcov replaced by the average),
    both, structure bits (score rescaled, ordered by score, length, key) -- through the single entry and the batch entry, whose values come from one
    device call per batch, and with an accept / reject limit, where they are computed hit by hit and a dropped hit counts neither way.  TM values go
    through tm_finish on raw device scores, the LDDT average through the ordered float sum: exact equality, as for the fixture tasks of test_tm_gpu.py."""
    monkeypatch.delenv("FSGPU_DEVICE_BACKTRACE", raising=False)
    w, F = env_ca["w"], env_ca["frozen"]["ca"]
    P = F.params(name)
    on_dev, total = check_set(env_ca, "ca", name, setup=_bind(w), before_call=_query_ca(w))
    if P["maxAccept"] != INT_MAX or P["maxRejected"] != INT_MAX:
        assert (on_dev, total) == (0, 0)
    else:
        assert total == sum(c for o, c in F.count(name).items() if o in BACKTRACED)


def test_calpha_refusals_leave_the_handle_usable(env_ca):
    """set_query_ca missing while C-alpha data is bound, and a query entry too short for its sequence: the error and its message; the next valid call on
    the same handle equals the model"""
    w, F = env_ca["w"], env_ca["frozen"]["ca"]
    name = "lddt07_tm07_m1"
    P = F.params(name)
    s = api.Search(env_ca["ctx"], make_params(2, P), keys=w["keys"])
    try:
        _bind(w)(s, P)
        qa, q3 = w["queries"][1]
        with pytest.raises(api.FsgpuError, match="query C-alpha entries of this call were not set"):
            s.align(qa, q3, w["lists"][1], identity=1)
        with pytest.raises(api.FsgpuError, match="query C-alpha entries of this call were not set"):
            s.align_batch([qa], [q3], [w["lists"][1]], identity=[1])
        s.set_query_ca([w["ca"][1][:40]])
        with pytest.raises(api.FsgpuError, match="shorter than its sequence needs"):
            s.align(qa, q3, w["lists"][1], identity=1)
        s.set_query_ca([w["ca"][1], w["ca"][2][:40]])
        with pytest.raises(api.FsgpuError, match="shorter than its sequence needs"):
            s.align_batch([qa, w["queries"][2][0]], [q3, w["queries"][2][1]], [w["lists"][1], w["lists"][2]], identity=[1, 2])
        want, cigars, _ = F.records(name, 1)
        s.set_query_ca([w["ca"][1]])
        res, bts = s.align(qa, q3, w["lists"][1], identity=1, with_backtrace=True)
        same_records(res, bts, want, cigars, "align after the refusals")
        s.set_query_ca([w["ca"][1]])
        res, bts = s.align_batch([qa], [q3], [w["lists"][1]], identity=[1], with_backtrace=True)
        same_records(res[0], bts[0], want, cigars, "align_batch after the refusals")
    finally:
        s.close()

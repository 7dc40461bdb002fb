"""fsgpu_sw_scan_c (Context.sw_scan_c) -- the whole-database forward Smith-Waterman pass with the selection on the device -- against tests/sw_model.py,
exactly: for every query the ascending ids of the targets whose score reaches the cutoff, and score, qEnd, dbEnd and word of each.  Inputs and the model's
frozen records come from tests/scan_cases.py; what the cases must contain for these tests to mean something is asserted in tests/test_scan_cases.py."""
import threading

import numpy as np
import pytest

import scan_cases as S
import sw_cases as K
import sw_model as sm
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu
ENV = ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT", "FSGPU_SCAN_BYTES")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.load_db(S.db())
    yield c
    c.close()


def set_env(monkeypatch, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def same(got, want, what):
    """one query: (ids, records) against the model's; on a mismatch the ids that differ and the first differing records"""
    gi, gr = got
    wi, wr = want
    assert gi.tolist() == wi.tolist(), (what, "ids", sorted(set(gi.tolist()) ^ set(wi.tolist()))[:8], len(gi), len(wi))
    bad = [k for k in range(len(wi)) if any(int(gr[k][f]) != int(wr[k][f]) for f in S.FIELDS)]
    assert not bad, (what, [(int(wi[k]), "device", tuple(int(gr[k][f]) for f in S.FIELDS), "model", tuple(int(wr[k][f]) for f in S.FIELDS)) for k in bad[:6]])


def scan_and_check(ctx, cfg, kind, what):
    atype, go, ge = cfg
    m3, mA = S.matrices(atype)
    recs = S.records(cfg)
    cuts = [S.cutoffs(r)[kind] for r in recs]
    got = ctx.sw_scan_c(m3, mA, S.api_queries(atype), cuts, gap_open=go, gap_extend=ge)
    assert len(got) == len(recs)
    for i, r in enumerate(recs):
        same(got[i], S.expected(r, cuts[i]), (what, S.config_name(cfg), kind, f"L={S.Q_LENGTHS[i]}", f"cutoff={cuts[i]}"))
    return got


# ---- the contract, every configuration and cutoff ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", S.CONFIGS, ids=S.config_name)
def test_scan_equals_the_model_filter(ctx, monkeypatch, cfg):
    set_env(monkeypatch)
    N = S.db().n
    for kind in S.CUTOFF_KINDS:
        scan_and_check(ctx, cfg, kind, "auto")
        plan = ctx.sw3_last_plan()
        # the 513-residue query with AA is the plain k_sw3 launch of test_sw3_model_gpu.py::test_split_boundaries at that shape
        assert plan["pairs"][32] > 0 and plan["pairs"][64] > 0 and plan["pairs"][16] == 0, plan
        assert plan["profile_pairs"] == N * sum(1 for L in S.Q_LENGTHS if L > 1024), plan
        assert sum(plan["pairs"].values()) == N * sum(1 for L in S.Q_LENGTHS if L <= 1024), plan
        assert -(-513 // 64) in plan["classes"][64] and -(-200 // 32) in plan["classes"][32], plan
    last = ctx.sw_scan_last()
    assert last["sub_batches"] == 1 and last["survivors"] == sum(int((r["score"] >= 32767).sum()) for r in S.records(cfg)), last      # the last kind: cutoff 32767
    set_env(monkeypatch, FSGPU_SW3_MID=512)
    scan_and_check(ctx, cfg, "median", "mid512")
    plan = ctx.sw3_last_plan()
    assert plan["pairs"][16] > 0 and plan["pairs"][32] > 0 and plan["pairs"][64] > 0, plan
    passes = ctx.sw_last_passes()
    assert passes[0][0] > 0 and passes[0][2] >= N * sum(1 for L in S.Q_LENGTHS if L <= 1024), passes       # every k_sw3 pair of the call (and what the profile path counts)


def test_one_query_per_sub_batch_gives_the_same_answer(ctx, monkeypatch):
    cfg = S.CONFIGS[0]
    set_env(monkeypatch)
    one = scan_and_check(ctx, cfg, "median", "one sub-batch")
    assert ctx.sw_scan_last()["sub_batches"] == 1
    set_env(monkeypatch, FSGPU_SCAN_BYTES=20 * S.db().n)
    split = scan_and_check(ctx, cfg, "median", "one query per sub-batch")
    last = ctx.sw_scan_last()
    assert last["sub_batches"] == sum(1 for L in S.Q_LENGTHS if L <= 1024), last
    for a, b in zip(one, split):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    plan = ctx.sw3_last_plan()                                                            # the counters add up over the sub-batches
    assert sum(plan["pairs"].values()) == S.db().n * last["sub_batches"] and plan["images_built"] >= last["sub_batches"], plan


def test_saturated_pairs_are_decided_by_their_int32_score(ctx, monkeypatch):
    set_env(monkeypatch)
    m3, mA, q = S.sat_case()
    recs = S.sat_records()
    for cut in S.SAT_CUTOFFS:
        got = ctx.sw_scan_c(m3, mA, S.api_queries(2, [q]), [cut])
        same(got[0], S.expected(recs, cut), ("saturation", cut))
        assert ctx.sw3_last_plan()["rerun_pairs"] == int((recs["word"] == 2).sum())
    assert (got[0][1]["word"] == 2).any() and (got[0][1]["word"] == 1).any()


def test_more_than_one_selection_chunk(monkeypatch):
    """a database of more than two chunks of 4096 slots: the survivors of a query come from several workgroups of the selection kernels"""
    set_env(monkeypatch)
    d, q = S.wide_db(), S.wide_query()
    assert d.n > 2 * 4096 and d.n % 4096 not in (0, 1)
    m3, mA = S.matrices(2)
    recs = S.wide_records()
    c = api.Context(0)
    try:
        c.load_db(d)
        cuts = [S.cutoffs(recs)["median"], S.cutoffs(recs)["occurs"], 0]
        for bytes_ in (None, 20 * d.n):
            set_env(monkeypatch, **({} if bytes_ is None else {"FSGPU_SCAN_BYTES": bytes_}))
            got = c.sw_scan_c(m3, mA, S.api_queries(2, [q, q, q]), cuts)
            for k, cut in enumerate(cuts):
                want = S.expected(recs, cut)
                assert 0 < len(want[0]) and (cut == 0 or len(want[0]) < d.n)
                same(got[k], want, ("wide", cut))
        assert len(got[2][0]) == d.n
    finally:
        c.close()


# ---- output capacity ---------------------------------------------------------------------------------------------------------------------------------
def test_cap_too_small_reports_the_needed_counts_and_writes_nothing_behind_cap(ctx, monkeypatch):
    set_env(monkeypatch)
    cfg = S.CONFIGS[0]
    atype, go, ge = cfg
    m3, mA = S.matrices(atype)
    recs = S.records(cfg)
    cuts = [S.cutoffs(r)["median"] for r in recs]
    want = [S.expected(r, c) for r, c in zip(recs, cuts)]
    total = sum(len(w[0]) for w in want)
    cap = total // 2
    assert cap > 0
    with pytest.raises(api.FsgpuError) as e:
        ctx.sw_scan_c(m3, mA, S.api_queries(atype), cuts, gap_open=go, gap_extend=ge, cap=cap)
    assert e.value.rc == api.FSGPU_E_OUTPUT == -6
    rc, base, ids, out = ctx.last_scan
    assert base.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()
    assert len(ids) == cap + 1 and ids[cap] == api.SCAN_GUARD and (out[cap:].view(np.uint32) == api.SCAN_GUARD).all()
    flat_ids = np.concatenate([w[0] for w in want])
    assert ids[:cap].tolist() == flat_ids[:cap].tolist()                                   # what fits is the head of the answer
    got = ctx.sw_scan_c(m3, mA, S.api_queries(atype), cuts, gap_open=go, gap_extend=ge, cap=int(base[-1]))
    for i in range(len(recs)):
        same(got[i], want[i], ("repeat with the reported size", i))
    rc, base, ids, out = ctx.last_scan
    assert rc == 0 and ids[total] == api.SCAN_GUARD
    got = ctx.sw_scan_c(m3, mA, S.api_queries(atype), cuts, gap_open=go, gap_extend=ge)   # the binding's own repeat: starts at 4096 records
    for i in range(len(recs)):
        same(got[i], want[i], ("binding repeat", i))


# ---- neighbours: images, databases, clones -----------------------------------------------------------------------------------------------------------
def test_reversed_pass_after_a_scan_answers_the_model(ctx, monkeypatch):
    """the scan builds the images of the same queries a compact call would: the reversed call after it must not take them for its own unless they are"""
    set_env(monkeypatch)
    cfg = S.CONFIGS[0]
    atype, go, ge = cfg
    m3, mA = S.matrices(atype)
    scan_and_check(ctx, cfg, "occurs", "before the reversed pass")
    d = S.db()
    ids = np.array([i for i in range(d.n) if d.lengths[i] <= 40][:6], np.uint32)
    assert len(ids) == 6
    qs = S.queries()
    got = ctx.sw_multi_dir_c(m3, mA, [t + (ids,) for t in S.api_queries(atype)], 1, gap_open=go, gap_extend=ge)
    ts = [K.target(d, int(i)) for i in ids]
    for i, q in enumerate(qs):
        want = sm.align(m3, mA, q.q3, q.qa, q.cb3r, q.cbAr, True, [t[0] for t in ts], [t[1] for t in ts], go, ge)
        assert [tuple(int(r[f]) for f in S.FIELDS) for r in got[i]] == [tuple(int(r[f]) for f in S.FIELDS) for r in want], (i, len(q.q3))
    scan_and_check(ctx, cfg, "occurs", "after the reversed pass")


def test_reload_of_a_different_database_drops_the_cached_order(monkeypatch):
    set_env(monkeypatch)
    cfg = S.CONFIGS[0]
    atype, go, ge = cfg
    m3, mA = S.matrices(atype)
    c = api.Context(0)
    try:
        c.load_db(S.db())
        scan_and_check(c, cfg, "median", "first database")
        other = S.other_db()
        c.load_db(other)
        # the other database's entries are entries 0..39 of the first: their records are known
        src = {K.target(S.db(), i)[0].tobytes() + b"|" + K.target(S.db(), i)[1].tobytes(): i for i in range(40)}
        back = np.array([src[K.target(other, j)[0].tobytes() + b"|" + K.target(other, j)[1].tobytes()] for j in range(other.n)], np.int64)
        recs = [r[back] for r in S.records(cfg)]
        cuts = [S.cutoffs(r)["median"] for r in recs]
        got = c.sw_scan_c(m3, mA, S.api_queries(atype), cuts, gap_open=go, gap_extend=ge)
        for i, r in enumerate(recs):
            same(got[i], S.expected(r, cuts[i]), ("second database", i))
        c.load_db(S.db())
        scan_and_check(c, cfg, "median", "first database again")
    finally:
        c.close()


def test_a_clone_scans_at_the_same_time_as_its_source(monkeypatch):
    set_env(monkeypatch)
    src = api.Context(0)
    src.load_db(S.db())
    clone = src.clone()                                   # before either has scanned: whichever comes first builds the order both use
    errors = []

    def work(c, cfg, kinds):
        try:
            for kind in kinds:
                scan_and_check(c, cfg, kind, "concurrent")
        except BaseException as e:                        # noqa: BLE001 -- reported by the main thread
            errors.append(e)
    try:
        ts = [threading.Thread(target=work, args=(src, S.CONFIGS[0], ("median", "occurs", "zero"))),
              threading.Thread(target=work, args=(clone, S.CONFIGS[2], ("occurs+1", "median", "max")))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
    finally:
        clone.close()
        src.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_a_good_call_follows(ctx, monkeypatch):
    set_env(monkeypatch)
    cfg = S.CONFIGS[0]
    atype, go, ge = cfg
    m3, mA = S.matrices(atype)
    qs = S.api_queries(atype)[:3]
    L = api.lib()

    def refused(rc, text, **kw):
        args = dict(mat3di=m3, matAA=mA, queries=qs, cutoffs=[5, 5, 5], gap_open=go, gap_extend=ge)
        args.update(kw)
        with pytest.raises(api.FsgpuError) as e:
            ctx.sw_scan_c(**args)
        assert e.value.rc == rc and text in str(e.value), (rc, text, str(e.value))

    refused(api.FSGPU_E_ARG, "cutoff outside 0..32767", cutoffs=[5, -1, 5])
    refused(api.FSGPU_E_ARG, "cutoff outside 0..32767", cutoffs=[5, 5, 32768])
    refused(api.FSGPU_E_UNSUPPORTED, "gapOpen > gapExtend", gap_open=1, gap_extend=1)
    bad = list(qs)
    bad[1] = (bad[1][0], np.full(len(bad[1][1]), 21, np.uint8)) + bad[1][2:]
    refused(api.FSGPU_E_ARG, "fsgpu_sw_scan_c: residue code out of range", queries=bad)
    empty = list(qs)
    empty[2] = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), None, None, None, None)
    refused(api.FSGPU_E_ARG, "fsgpu_sw_scan_c: bad query", queries=empty)
    # a query that brings a target list, through the C entry itself (the binding never passes one)
    class Q(api.C.Structure):
        _fields_ = [("qAA", api.C.c_void_p), ("q3Di", api.C.c_void_p), ("cbAA_fwd", api.C.c_void_p), ("cb3Di_fwd", api.C.c_void_p), ("cbAA_rev", api.C.c_void_p),
                    ("cb3Di_rev", api.C.c_void_p), ("L", api.C.c_int32), ("n", api.C.c_int32), ("targetIds", api.C.c_void_p)]
    q3, qa = np.ascontiguousarray(qs[0][1]), np.ascontiguousarray(qs[0][0])
    tid = np.zeros(1, np.uint32)
    one = (Q * 1)()
    one[0].qAA, one[0].q3Di, one[0].L, one[0].n, one[0].targetIds = qa.ctypes.data, q3.ctypes.data, len(q3), 1, tid.ctypes.data
    cut, base = np.array([5], np.int32), np.zeros(2, np.uint64)
    ids, out = np.zeros(8, np.uint32), np.zeros(8, api.SWRES_DT)
    rc = L.fsgpu_sw_scan_c(ctx.h, m3.ctypes.data, mA.ctypes.data, api.C.cast(one, api.C.c_void_p), 1, go, ge, cut.ctypes.data, ids.ctypes.data, out.ctypes.data, 8, base.ctypes.data)
    assert rc == api.FSGPU_E_ARG and b"must be 0 / NULL" in L.fsgpu_last_error(ctx.h)
    assert L.fsgpu_sw_scan_c(ctx.h, m3.ctypes.data, mA.ctypes.data, api.C.cast(one, api.C.c_void_p), 1, go, ge, cut.ctypes.data, ids.ctypes.data, out.ctypes.data, 8, None) == api.FSGPU_E_ARG
    assert L.fsgpu_sw_scan_c(ctx.h, m3.ctypes.data, mA.ctypes.data, api.C.cast(one, api.C.c_void_p), 1, go, ge, cut.ctypes.data, None, None, 8, base.ctypes.data) == api.FSGPU_E_ARG
    # no database; a database without AA and an AA matrix
    c = api.Context(0)
    try:
        with pytest.raises(api.FsgpuError) as e:
            c.sw_scan_c(m3, mA, qs, [5, 5, 5])
        assert e.value.rc == api.FSGPU_E_NODB
        d = S.db()
        c.load_db(synth.PaddedDB(d.data3di, None, d.offsets, d.lengths))
        with pytest.raises(api.FsgpuError) as e:
            c.sw_scan_c(m3, mA, qs, [5, 5, 5])
        assert e.value.rc == api.FSGPU_E_NODB and "without AA" in str(e.value)
        cfg0 = S.CONFIGS[2]                                   # 3Di only: that context serves it
        scan_and_check(c, cfg0, "median", "3Di-only database")
    finally:
        c.close()
    assert ctx.sw_scan_c(m3, mA, [], []) == []               # no queries: no lists
    scan_and_check(ctx, cfg, "median", "after the refusals")

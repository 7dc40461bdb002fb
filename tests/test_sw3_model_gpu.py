"""The compact-query Smith-Waterman path (fsgpu_sw_multi_dir_c / fsgpu_sw_multi_c: k_sw3, k_sw3_image and the planner of fsgpu_sw3_multi.hip) and its
siblings against tests/sw_model.py, exactly: score, qEnd, dbEnd and word of every pair, no pair skipped.  Inputs and the model's frozen answers come from
tests/sw_cases.py; which shape and rows-per-lane class a pair ran with is asserted from Context.sw3_last_plan()."""
import numpy as np
import pytest

import sw_cases as K
import sw_model as sm
from foldseek_amd import api

pytestmark = pytest.mark.gpu
FIELDS = ("score", "qEnd", "dbEnd", "word")


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.load_db(K.main_db())
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_tiny():
    c = api.Context(0)
    c.load_db(K.tiny_db())
    yield c
    c.close()


def set_env(monkeypatch, env):
    for k in ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def same(got, want, what, L, tlens):
    """every pair of one query: on a mismatch the class, L, the target's length and both records"""
    bad = [k for k in range(len(want)) if any(int(got[k][f]) != int(want[k][f]) for f in FIELDS)]
    assert len(got) == len(want) and not bad, \
        (what, f"L={L} R16/32/64={-(-L // 16)}/{-(-L // 32)}/{-(-L // 64)}", f"{len(bad)} of {len(want)} pairs differ",
         [(k, int(tlens[k]), "device", tuple(int(got[k][f]) for f in FIELDS), "model", tuple(int(want[k][f]) for f in FIELDS)) for k in bad[:6]])


def check(call, direction, got, sel=None):
    db = K.DBS[call.db]()
    want = K.call_want(call, direction)
    for i, q in enumerate(call.queries):
        tl = db.lengths[np.asarray(call.ids[i], np.int64)]
        if sel is None:
            same(got[i], want[i], (call.name, "rev" if direction else "fwd", i), len(q.q3), tl)
        else:
            m = np.zeros(len(call.ids[i]), bool); m[np.asarray(sel[i], np.int64)] = True
            same(got[i][m], want[i][m], (call.name, "selected", i), len(q.q3), tl[m])
            assert not got[i][~m].tobytes().strip(b"\0"), (call.name, "unselected entries written", i)
    return want


def run(ctx, monkeypatch, call, sel=None):
    """the call's directions through sw_multi_dir_c, each compared with the model; returns ([results per direction], [plan per direction])"""
    set_env(monkeypatch, call.env)
    res, plans = [], []
    for d in call.dirs:
        got = ctx.sw_multi_dir_c(call.m3, call.mA, K.api_queries(call), d, selections=sel, gap_open=call.go, gap_extend=call.ge)
        plans.append(ctx.sw3_last_plan())
        check(call, d, got, sel)
        res.append(got)
    return res, plans


def assert_split(call, plan, sel=None):
    exp = K.expected_split(call, sel)
    assert plan["pairs"] == {16: exp[16], 32: exp[32], 64: exp[64]} and plan["profile_pairs"] == exp["profile"], (call.name, plan, exp)
    assert plan["classes"] == exp["classes"], (call.name, plan, exp)
    return exp


# ---- (a) every class of every shape ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6), ids=lambda k: K.section_a()[k].name)
def test_every_class_of_every_shape(ctx, monkeypatch, which):
    call = K.section_a()[which]
    HL, Rs = K.A_CLASSES[call.name.split("/")[1]]
    _, plans = run(ctx, monkeypatch, call)
    total = sum(len(x) for x in call.ids)
    for plan in plans:
        assert plan["classes"] == {hl: (Rs if hl == HL else set()) for hl in (16, 32, 64)}, plan
        assert plan["pairs"] == {hl: (total if hl == HL else 0) for hl in (16, 32, 64)} and plan["profile_pairs"] == 0 and plan["rerun_pairs"] == 0, plan
        assert_split(call, plan)
    assert plans[0]["images_built"] == len(call.queries) and plans[1]["images_built"] == 0, plans      # the reversed call finds the forward call's images


# ---- (b) wave and workgroup packing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(3), ids=lambda k: K.section_b()[k].name)
def test_wave_and_workgroup_packing(ctx, monkeypatch, which):
    call = K.section_b()[which]
    _, _, HL, L = K.B_CLASSES[which]
    R = -(-L // HL)
    ppw, ppb = K.pairs_per_wave(HL), K.pairs_per_workgroup(R, HL, True)
    sizes = [len(x) for x in call.ids]
    assert sizes == [1, 2, 3, ppw - 1, ppw, ppw + 1, ppb, ppb + 1] and ppb % ppw == 0
    _, plans = run(ctx, monkeypatch, call)
    for plan in plans:
        assert plan["pairs"][HL] == sum(sizes) and plan["classes"][HL] == {R} and plan["groups"] == 1, plan
        assert plan["workgroups"] == sum(-(-n // ppb) for n in sizes) == len(sizes) + 1, (plan, ppb)


def test_packing_every_length_in_one_list(ctx, monkeypatch):
    call = K.section_b()[3]
    assert len(call.ids[0]) == K.main_db().n
    _, plans = run(ctx, monkeypatch, call)
    for plan in plans:
        exp = assert_split(call, plan)
        assert exp[64] > 0 and exp[32] > 0 and exp[16] == 0


@pytest.mark.parametrize("which", range(4, 7), ids=lambda k: K.section_b()[k].name)
def test_packing_longest_target_shares_a_register_with_a_one_column_target(ctx, monkeypatch, which):
    """two pairs, one shape, one workgroup: sorted longest first they are targets A and B of the first lane group, the two halves of every register"""
    call = K.section_b()[which]
    HL = int(call.name.split("/")[2])
    lens = K.main_db().lengths[call.ids[0].astype(np.int64)].tolist()
    assert sorted(lens) == [1, 1300 if HL == 64 else 896]
    _, plans = run(ctx, monkeypatch, call)
    for plan in plans:
        assert plan["pairs"] == {hl: (2 if hl == HL else 0) for hl in (16, 32, 64)} and plan["workgroups"] == 1 and plan["groups"] == 1, plan
        assert_split(call, plan)


# ---- (c) the split's boundaries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(5), ids=lambda k: K.section_c()[k].name)
def test_split_boundaries(ctx, monkeypatch, which):
    call = K.section_c()[which]
    _, plans = run(ctx, monkeypatch, call)
    for plan in plans:
        exp = assert_split(call, plan)
    n1025 = len(call.ids[-1])
    assert exp["profile"] == n1025 and len(call.queries[-1].q3) == 1025
    compact = sum(len(x) for x in call.ids) - n1025
    # what each setting is there for, stated on the derived counts so that a change of the cases cannot hollow it out
    if call.name == "c/auto":
        assert exp[16] == 0 and exp[64] == 2 * 17 + 3 and exp[32] == compact - exp[64]                  # 513 and 1024 rows; the 897-column target of the others
    elif call.name == "c/mid512":
        assert exp[16] == 17 - 3 and exp[64] == 2 * 17 + 3 and exp["classes"][16] == {24}                  # 384 rows: up to 512 columns
    elif call.name == "c/mid896 short0":
        assert exp[16] == 16 and exp[32] == 2 * 16
    elif call.name == "c/16 per query":
        assert compact == 16 * 5 and exp[64] == compact
    else:
        assert compact == 16 * 5 + 1 and exp[32] > 0


# ---- (d) image reuse ---------------------------------------------------------------------------------------------------------------------------------
def test_image_reuse(monkeypatch):
    steps = K.section_d()
    ctx = api.Context(0)
    ctx.load_db(K.main_db())
    try:
        def go(name, sel=None, built=None):
            res, plans = run(ctx, monkeypatch, steps[name], sel)
            if built is not None:
                assert (plans[0]["images_built"] > 0) == built, (name, plans[0])
            return res[0], plans[0]
        first, p1 = go("short", built=True)                                     # 1
        assert p1["pairs"][32] > 0 and p1["classes"][64] == {10}
        _, p2 = go("long", built=True)                                          # 2: the 897-column targets need the 64-lane images of the short queries
        assert p2["classes"][64] == {1, 4, 6, 10} and p2["images_built"] == 7, p2
        again, _ = go("short", built=False)                                     # 3
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        base = K.call_want(steps["short"], 0)
        for name in ("bias", "matrix"):                                         # 4, 5: one byte of what the images are made of
            go(name, built=True)
            assert any((a != b).any() for a, b in zip(K.call_want(steps[name], 0), base)), name + ": the change must show in the model's records"
        assert (K.call_want(steps["bias"], 0)[0] == base[0]).all()              # ... and the other queries keep theirs
        go("3di", built=True)                                                   # 6
        full = [np.arange(len(x), dtype=np.int32) for x in steps["short"].ids]
        sel = [full[0], full[1], np.zeros(0, np.int32), full[3]]
        _, p = go("short", sel, built=True)                                     # 7: built without query 2, which the full lists then miss
        assert p["images_built"] == 3, p
        _, p = go("short", built=True)
        assert p["images_built"] == 4, p
        go("short", sel, built=False)
        go("swapped", built=True)                                               # 8
        first, _ = go("short", built=True)                                      # 9: the profile-path entries in between leave the images alone
        c = steps["short"]
        profs = [[sm.profile(m, s, b, rev).astype(np.int16) for m, s, b, rev in ((c.mA, q.qa, q.cbAf, False), (c.m3, q.q3, q.cb3f, False), (c.mA, q.qa, q.cbAr, True), (c.m3, q.q3, q.cb3r, True))]
                 for q in c.queries]
        f, r = ctx.sw_batch(*profs[2], c.ids[2])
        same(f, base[2], "sw_batch between compact calls", 380, K.main_db().lengths[c.ids[2].astype(np.int64)])
        multi = ctx.sw_multi_dir([(p[0], p[1], p[2], p[3], len(q.q3), ids) for p, q, ids in zip(profs, c.queries, c.ids)], 0)
        for i in range(len(multi)):
            same(multi[i], base[i], "sw_multi_dir between compact calls", len(c.queries[i].q3), K.main_db().lengths[c.ids[i].astype(np.int64)])
        again, _ = go("short", built=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    finally:
        ctx.close()


# ---- (e) saturation ----------------------------------------------------------------------------------------------------------------------------------
def test_saturation_in_one_direction_only(ctx, monkeypatch):
    call = K.section_e()[0]
    wf, wr = K.call_want(call, 0)[0], K.call_want(call, 1)[0]
    assert (wf["word"] == 2).all() and (wf["score"] > 32767).all() and (wr["word"] == 1).all() and (wr["score"] < 32767).all()
    n = len(call.ids[0])
    _, plans = run(ctx, monkeypatch, call)
    assert plans[0]["rerun_pairs"] == n and plans[1]["rerun_pairs"] == 0, plans
    set_env(monkeypatch, call.env)
    f, r = ctx.sw_multi_c(call.m3, call.mA, K.api_queries(call))
    assert ctx.sw3_last_plan()["rerun_pairs"] == n
    tl = K.main_db().lengths[call.ids[0].astype(np.int64)]
    same(f[0], wf, "one submission, forward (saturated)", 400, tl)
    same(r[0], wr, "one submission, reversed (not saturated: its int16 record stands)", 400, tl)


def test_saturation_all_biases_100(ctx, monkeypatch):
    call = K.section_e()[1]
    wf, wr = K.call_want(call, 0)[0], K.call_want(call, 1)[0]
    assert (wf["word"] == 2).any() and (wf["word"] == 1).any()
    _, plans = run(ctx, monkeypatch, call)
    assert plans[0]["rerun_pairs"] == int((wf["word"] == 2).sum()) and plans[1]["rerun_pairs"] == int((wr["word"] == 2).sum())
    f, r = ctx.sw_multi_c(call.m3, call.mA, K.api_queries(call))
    assert ctx.sw3_last_plan()["rerun_pairs"] == int(((wf["word"] == 2) | (wr["word"] == 2)).sum())
    tl = K.main_db().lengths[call.ids[0].astype(np.int64)]
    same(f[0], wf, "one submission, forward", 400, tl)
    same(r[0], wr, "one submission, reversed", 400, tl)


def test_score_of_exactly_32767_unclipped(monkeypatch):
    """217 positions of 151 each: INT16_MAX reached without clipping is still re-run (word 2), as alignScoreEndPos does"""
    m3, mA, q, t3, tA = K.exact_32767()
    db = K.exact_db()
    hom = int(np.flatnonzero(db.lengths == 217)[0])
    ids = np.array([hom, 1 - hom], np.uint32)
    ctx = api.Context(0)
    ctx.load_db(db)
    try:
        set_env(monkeypatch, {})
        for d in (0, 1):
            want = K.want(m3, mA, q, bool(d), [K.target(db, int(i)) for i in ids])
            assert tuple(want[0]) == (32767, 216, 216, 2)
            got = ctx.sw_multi_dir_c(m3, mA, [(q.qa, q.q3, q.cbAf, q.cb3f, q.cbAr, q.cb3r, ids)], d)
            same(got[0], want, ("exactly 32767", d), 217, db.lengths[ids.astype(np.int64)])
            assert ctx.sw3_last_plan()["rerun_pairs"] == 1
    finally:
        ctx.close()


# ---- (f) score zero and tiny inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(6), ids=lambda k: K.section_f()[k].name)
def test_score_zero_and_tiny_inputs(ctx, ctx_tiny, monkeypatch, which):
    call = K.section_f()[which]
    HL = int(call.name.split("/")[2])
    res, plans = run(ctx if call.db == "main" else ctx_tiny, monkeypatch, call)
    total = sum(len(x) for x in call.ids)
    for plan in plans:
        assert plan["pairs"] == {hl: (total if hl == HL else 0) for hl in (16, 32, 64)}, plan
    if call.db == "main":
        want = K.call_want(call, 0)
        assert not want[0].view(np.int32).reshape(-1, 4)[:, :3].any()                 # the all-X query: (0, 0, 0) everywhere
        allx = K.main_db().kind.index("allX")
        k = list(call.ids[2]).index(allx)                                             # the L = 1 query without biases against the all-X target
        assert len(call.queries[2].q3) == 1 and tuple(want[2][k]) == (0, 0, 0, 1) and tuple(res[0][2][k]) == (0, 0, 0, 1)


# ---- (g) the siblings, directly ----------------------------------------------------------------------------------------------------------------------
def _profiles(call, q):
    return [sm.profile(m, s, b, rev).astype(np.int16) for m, s, b, rev in ((call.mA, q.qa, q.cbAf, False), (call.m3, q.q3, q.cb3f, False), (call.mA, q.qa, q.cbAr, True), (call.m3, q.q3, q.cb3r, True))]


def _siblings(ctx, call):
    db = K.main_db()
    want = [K.call_want(call, 0), K.call_want(call, 1)]
    profs = [_profiles(call, q) for q in call.queries]
    for d in (0, 1):
        multi = ctx.sw_multi_dir([(p[0], p[1], p[2], p[3], len(q.q3), ids) for p, q, ids in zip(profs, call.queries, call.ids)], d, gap_open=call.go, gap_extend=call.ge)
        for i, q in enumerate(call.queries):
            same(multi[i], want[d][i], (call.name, "sw_multi_dir", d, i), len(q.q3), db.lengths[call.ids[i].astype(np.int64)])
    for i, q in enumerate(call.queries):
        tl = db.lengths[call.ids[i].astype(np.int64)]
        f, r = ctx.sw_batch(*profs[i], call.ids[i], call.go, call.ge)
        same(f, want[0][i], (call.name, "sw_batch fwd", i), len(q.q3), tl)
        same(r, want[1][i], (call.name, "sw_batch rev", i), len(q.q3), tl)
        ts = [K.target(db, int(t)) for t in call.ids[i]]
        f, r = ctx.sw_batch_seqs(*profs[i], [t[1] for t in ts], [t[0] for t in ts], call.go, call.ge)
        same(f, want[0][i], (call.name, "sw_batch_seqs fwd", i), len(q.q3), tl)
        same(r, want[1][i], (call.name, "sw_batch_seqs rev", i), len(q.q3), tl)


@pytest.mark.parametrize("which", range(3), ids=lambda k: K.section_g()[0][k].name)
def test_siblings_on_the_class_queries(ctx, which):
    _siblings(ctx, K.section_g()[0][which])


@pytest.mark.parametrize("which", range(12), ids=lambda k: K.section_g()[1][k].name)
def test_other_gap_costs_compact_and_siblings(ctx, monkeypatch, which):
    call = K.section_g()[1][which]
    run(ctx, monkeypatch, call)
    _siblings(ctx, call)

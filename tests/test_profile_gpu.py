"""Profile queries on the device: fsgpu_sw_multi_dir_p / fsgpu_sw_multi_p (k_sw3 over the images k_sw3_image_profile builds; the int16 path above 1024
positions) against tests/profile_model.py -> tests/sw_model.py, exactly: score, qEnd, dbEnd and word of every pair.  Which shape and rows-per-lane
class a pair ran with is asserted from Context.sw3_last_plan(), as in tests/test_sw3_model_gpu.py.  The gapless scan takes a decoded profile as its
pssm (fsgpu_gapless_scan, fsgpu_gapless_scan_multi) and is held to tests/gapless_model.py.

The profiles are seeded: the substitution-matrix columns of a master sequence (so that the database's relatives of it align) plus noise, clipped to
what an entry can hold after the division by four (-32 .. 31), X row zero; every tenth position carries the extremes.  The model's records are
computed once per (tables, gap costs, direction) and shared by the cases."""
import functools

import numpy as np
import pytest

import gapless_model as gm
import profile_model as pm
import sw_cases as K
from foldseek_amd import api

pytestmark = pytest.mark.gpu
FIELDS = ("score", "qEnd", "dbEnd", "word")
# the borders of k_sw3's shapes (16 lanes: 1 row per lane up to 16, 32 lanes: up to 32; 32 -> 64 lanes at 512; the end of k_sw3 at 1024) and the hand-over
LENGTHS = (1, 2, 16, 17, 32, 33, 511, 512, 513, 1023, 1024, 1025)
ENVS = {"16": K.ENV_16, "32": K.ENV_32, "auto": K.ENV_AUTO}


@functools.lru_cache(maxsize=None)
def tables(L, seed=0):
    """(p3 fwd, pA fwd, p3 rev, pA rev) int8 [21, L] through the entry format: encode -> profile_model.decode"""
    rng = np.random.default_rng(31000 + 17 * L + seed)
    m3, mA = K.matrices()
    out = []
    for mat, master in zip((m3, mA), K._master()):
        stored = 4 * mat[:20, master[:L]].astype(np.int32) + rng.integers(-9, 10, (20, L))
        stored[:, ::10] = rng.choice(np.array([-128, 127]), (20, len(range(0, L, 10))))
        codes = master[:L].copy()
        _, _, prof, rev = pm.decode(pm.encode(np.clip(stored, -128, 127).astype(np.int8), codes))
        assert not prof[20].any() and prof.min() >= -32 and prof.max() <= 31
        out.append((prof, rev))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@functools.lru_cache(maxsize=None)
def lists():
    """per length a dozen targets of up to 257 columns, the relative nearest in length (up to 257 columns), a 1-column target and one of 897 columns,
    which the 16- and 32-lane settings hand to the 64-lane shape"""
    db = K.main_db()
    rng = np.random.default_rng(2718)
    pool = K.ids_where(db, 2, 257)
    out = []
    for L in LENGTHS:
        ids = list(rng.choice(pool, size=12, replace=False)) + [K.first_of_length(db, 1)]
        cand = K.ids_where(db, 1, 257, "derived")
        ids.append(int(cand[np.argmin(np.abs(db.lengths[cand].astype(np.int64) - L))]))
        ids.append(K.first_of_length(db, 897, "derived"))
        out.append(np.array(sorted(set(int(i) for i in ids)), np.uint32))
    return out


@functools.lru_cache(maxsize=None)
def want(L, ids_key, aa, go, ge, direction, seed=0):
    """the model's records of the profile of length L in one direction; ids_key: the target ids as a tuple"""
    db = K.main_db()
    p3f, pAf, p3r, pAr = tables(L, seed)
    return pm.sw_records(p3r if direction else p3f, (pAr if direction else pAf) if aa else None, [K.target(db, i) for i in ids_key], go, ge)


def queries(aa, id_lists, lengths=LENGTHS, seed=0):
    out = []
    for L, ids in zip(lengths, id_lists):
        p3f, pAf, p3r, pAr = tables(L, seed)
        out.append((pAf if aa else None, p3f, pAr if aa else None, p3r, ids))
    return out


def same(got, wanted, what, L, tlens):
    bad = [k for k in range(len(wanted)) if any(int(got[k][f]) != int(wanted[k][f]) for f in FIELDS)]
    assert len(got) == len(wanted) and not bad, \
        (what, f"L={L}", f"{len(bad)} of {len(wanted)} pairs differ",
         [(k, int(tlens[k]), "device", tuple(int(got[k][f]) for f in FIELDS), "model", tuple(int(wanted[k][f]) for f in FIELDS)) for k in bad[:6]])


def set_env(monkeypatch, env):
    for k in ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def expected_plan(env, id_lists, sel=None, lengths=LENGTHS):
    """the planner's documented split (sw_cases.expected_split) for queries of these lengths: it reads only len(q.q3), the lists and the setting"""
    stand_in = [K.Query(np.zeros(L, np.uint8), None, None, None, None, None) for L in lengths]
    return K.expected_split(K.Call("profile", env, None, None, stand_in, id_lists, (0,), 10, 1, "main"), sel)


def assert_plan(plan, exp):
    assert plan["pairs"] == {16: exp[16], 32: exp[32], 64: exp[64]} and plan["profile_pairs"] == exp["profile"] and plan["classes"] == exp["classes"], (plan, exp)


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    c.load_db(K.main_db())
    yield c
    c.close()


def check_dir(ctx, aa, go, ge, direction, id_lists, sel, what):
    db = K.main_db()
    got = ctx.sw_multi_dir_p(queries(aa, id_lists), direction, selections=sel, gap_open=go, gap_extend=ge)
    for i, L in enumerate(LENGTHS):
        w = want(L, tuple(int(t) for t in id_lists[i]), aa, go, ge, direction)
        tl = db.lengths[id_lists[i].astype(np.int64)]
        if sel is None:
            same(got[i], w, (what, direction, i), L, tl)
        else:
            m = np.zeros(len(id_lists[i]), bool); m[np.asarray(sel[i], np.int64)] = True
            same(got[i][m], w[m], (what, "selected", direction, i), L, tl[m])
            assert not got[i][~m].tobytes().strip(b"\0"), (what, "unselected entries written", i)
    return ctx.sw3_last_plan()


# ---- every border length, in every shape --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(ENVS))
@pytest.mark.parametrize("direction", (0, 1))
def test_border_lengths_in_every_shape(ctx, monkeypatch, setting, direction):
    set_env(monkeypatch, ENVS[setting])
    ids = lists()
    plan = check_dir(ctx, True, 10, 1, direction, ids, None, setting)
    exp = expected_plan(ENVS[setting], ids)
    assert_plan(plan, exp)
    n1025 = len(ids[-1])
    assert exp["profile"] == n1025 and plan["rerun_pairs"] == 0
    # what each setting is there for: the classes on both sides of every border
    if setting == "16":
        assert {1, 2, 3} <= exp["classes"][16] and {8, 9, 16} <= exp["classes"][64] and exp["classes"][32] == {16}       # 16 | 17, 32 | 33 rows; 511 / 512: 32 lanes
    elif setting == "32":
        assert exp["classes"][32] == {1, 2, 16} and {1, 8, 9, 16} <= exp["classes"][64] and exp[16] == 0                   # 32 | 33; 512 | 513; 897 columns
    else:
        assert exp[16] == 0 and exp[32] == 0 and exp["classes"][64] == {1, 8, 9, 16}                                    # short lists: 64 lanes throughout


@pytest.mark.parametrize("aa", (True, False), ids=("aa", "3di"))
@pytest.mark.parametrize("gaps", ((10, 1), (8, 2)), ids=("10-1", "8-2"))
def test_variants_both_directions_and_selections(ctx, monkeypatch, aa, gaps):
    set_env(monkeypatch, K.ENV_32)
    ids = lists()
    rng = np.random.default_rng(5)
    sel = [np.sort(rng.choice(len(x), size=max(1, len(x) // 2), replace=False)).astype(np.int32) for x in ids]
    sel[3] = np.zeros(0, np.int32)                                           # a query without a selected pair
    for direction in (0, 1):
        plan = check_dir(ctx, aa, gaps[0], gaps[1], direction, ids, None, ("all pairs", aa, gaps))
        assert_plan(plan, expected_plan(K.ENV_32, ids))
        plan = check_dir(ctx, aa, gaps[0], gaps[1], direction, ids, sel, ("selection", aa, gaps))
        assert_plan(plan, expected_plan(K.ENV_32, ids, sel))
    # one submission for both directions
    db = K.main_db()
    f, r = ctx.sw_multi_p(queries(aa, ids), gap_open=gaps[0], gap_extend=gaps[1])
    for i, L in enumerate(LENGTHS):
        key, tl = tuple(int(t) for t in ids[i]), db.lengths[ids[i].astype(np.int64)]
        same(f[i], want(L, key, aa, gaps[0], gaps[1], 0), ("sw_multi_p forward", aa, gaps, i), L, tl)
        same(r[i], want(L, key, aa, gaps[0], gaps[1], 1), ("sw_multi_p reversed", aa, gaps, i), L, tl)


def test_reversed_call_finds_the_forward_calls_images(ctx, monkeypatch):
    set_env(monkeypatch, K.ENV_32)
    ids = lists()
    other = queries(True, ids, seed=1)
    ctx.sw_multi_dir_p(other, 0)                                             # something else in the context first
    q = queries(True, ids)
    ctx.sw_multi_dir_p(q, 0)
    built = ctx.sw3_last_plan()["images_built"]
    ctx.sw_multi_dir_p(q, 1)
    assert built > 0 and ctx.sw3_last_plan()["images_built"] == 0
    # one byte of one table: the images are rebuilt, and the record that depends on it follows
    p3f = tables(512)[0].copy()
    p3f[3, 100] = -32 if p3f[3, 100] > 0 else 31
    k = LENGTHS.index(512)
    q2 = list(q); q2[k] = (q[k][0], p3f, q[k][2], q[k][3], q[k][4])
    got = ctx.sw_multi_dir_p(q2, 0)
    assert ctx.sw3_last_plan()["images_built"] > 0
    db = K.main_db()
    w = pm.sw_records(p3f, tables(512)[1], [K.target(db, int(i)) for i in ids[k]])
    same(got[k], w, "one byte changed", 512, db.lengths[ids[k].astype(np.int64)])


def test_refusals(ctx):
    ids = lists()
    q = queries(True, ids)
    for go, ge in ((1, 1), (1, 2)):
        with pytest.raises(api.FsgpuError) as e:
            ctx.sw_multi_dir_p(q, 0, gap_open=go, gap_extend=ge)
        assert "gapOpen > gapExtend" in str(e.value)
    mixed = [q[0], (None, q[1][1], None, q[1][3], q[1][4])]                  # one query with AA tables, one without
    with pytest.raises(api.FsgpuError):
        ctx.sw_multi_dir_p(mixed, 0)
    plan = check_dir(ctx, True, 10, 1, 0, ids, None, "after the refusals")
    assert plan["images_built"] > 0


# ---- saturation: the int16 pass returns 32767, the int32 re-run decides -------------------------------------------------------------------------------
def test_saturating_profile(ctx, monkeypatch):
    """600 positions of the largest score an entry can hold (31 after the division) in both tables: 62 a column, 32767 is passed after 529 columns"""
    set_env(monkeypatch, {})
    db = K.main_db()
    stored = np.full((20, 600), 127, np.int8)
    codes = np.zeros(600, np.uint8)
    _, _, prof, rev = pm.decode(pm.encode(stored, codes))
    assert (prof[:20] == 31).all() and (rev == prof).all()
    ids = np.concatenate([K.ids_where(db, 511, 513, "random"), K.ids_where(db, 895, 897, "random"), K.ids_where(db, 1300, 1300), K.ids_where(db, 100, 130, "random")]).astype(np.uint32)
    targets = [K.target(db, int(i)) for i in ids]
    w = pm.sw_records(prof, prof, targets)
    n_sat = int((w["word"] == 2).sum())
    assert n_sat >= 4 and (w["word"] == 1).any() and w["score"].max() > 32767 and (w["score"][w["word"] == 2] > 32767).all()
    for direction in (0, 1):
        got = ctx.sw_multi_dir_p([(prof, prof, rev, rev, ids)], direction)
        same(got[0], w, ("saturating", direction), 600, db.lengths[ids.astype(np.int64)])
        assert ctx.sw3_last_plan()["rerun_pairs"] == n_sat
    f, r = ctx.sw_multi_p([(prof, prof, rev, rev, ids)])
    same(f[0], w, "saturating, one submission, forward", 600, db.lengths[ids.astype(np.int64)])
    same(r[0], w, "saturating, one submission, reversed", 600, db.lengths[ids.astype(np.int64)])


# ---- state: compact, profile, compact on one context at the same lengths ------------------------------------------------------------------------------
def test_profile_call_between_two_compact_calls(monkeypatch):
    call = K.section_d()["short"]
    set_env(monkeypatch, call.env)
    db = K.main_db()
    lengths = tuple(len(q.q3) for q in call.queries)
    ctx = api.Context(0)
    ctx.load_db(db)
    try:
        def compact(step):
            got = ctx.sw_multi_dir_c(call.m3, call.mA, K.api_queries(call), 0)
            plan = ctx.sw3_last_plan()
            for i, (q, w) in enumerate(zip(call.queries, K.call_want(call, 0))):
                same(got[i], w, (step, i), len(q.q3), db.lengths[call.ids[i].astype(np.int64)])
            return plan
        first = compact("compact, first")
        assert first["images_built"] == len(call.queries)
        got = ctx.sw_multi_dir_p(queries(True, call.ids, lengths), 0)
        plan = ctx.sw3_last_plan()
        assert plan["images_built"] == len(call.queries), plan              # same lengths, same lists, same shapes: yet nothing of the compact call fits
        assert plan["pairs"] == first["pairs"] and plan["classes"] == first["classes"]
        for i, L in enumerate(lengths):
            same(got[i], want(L, tuple(int(t) for t in call.ids[i]), True, 10, 1, 0), ("profile, between", i), L, db.lengths[call.ids[i].astype(np.int64)])
        again = compact("compact, after the profile call")
        assert again["images_built"] == len(call.queries), again
        got = ctx.sw_multi_dir_p(queries(False, call.ids, lengths), 1)      # and a 3Di-only reversed profile call after a compact one with AA
        for i, L in enumerate(lengths):
            same(got[i], want(L, tuple(int(t) for t in call.ids[i]), False, 10, 1, 1), ("profile 3Di, after", i), L, db.lengths[call.ids[i].astype(np.int64)])
    finally:
        ctx.close()


# ---- the gapless scan with a decoded profile as its pssm ----------------------------------------------------------------------------------------------
def _same_hits(got, wanted, what):
    assert len(got) == len(wanted) and (got["id"] == wanted["id"]).all() and (got["score"] == wanted["score"]).all(), (what, got[:8], wanted[:8])


@pytest.mark.parametrize("L", (1, 33, 300, 1025))
def test_gapless_scan_of_a_profile_between_two_sequence_queries(ctx, L):
    db = K.main_db()
    m3, _ = K.matrices()
    packed = gm.pack(db)
    entry = pm.encode(np.clip(4 * tables(L)[0][:20].astype(np.int32) + 1, -128, 127).astype(np.int8), K._master()[0][:L])
    codes, _, prof, _ = api.profile_decode(entry)
    assert (prof == pm.decode(entry)[2]).all() and api.profile_bias(prof) == pm.bias(prof)
    seqs = [K.make_query(n, 400 + n, "related") for n in (120, 260)]
    seq_q = [(np.ascontiguousarray(m3[:, s.q3] + s.cb3f[None, :]).astype(np.int8), 255 - int(-min(0, int(m3.min()) + int(s.cb3f.min())))) for s in seqs]
    trio = [seq_q[0], (prof, pm.cap(prof)), seq_q[1]]
    wants = [gm.scores(p, c, packed) for p, c in trio]
    assert wants[1].max() > 30
    for k, (p, c) in enumerate(trio):                                        # one after the other on one context
        hits = ctx.gapless_scan(p, c, min_score=15, identity=-1, max_res=60)
        assert (ctx.gapless_scores().astype(np.int32) == wants[k]).all(), ("scan, scores", L, k)
        _same_hits(hits, gm.select(wants[k], 15, -1, 60), ("scan, hits", L, k))
    got = ctx.gapless_scan_multi([(p, c, -1) for p, c in trio], min_score=15, max_res=60)
    for k in range(3):
        if trio[k][0].shape[1] <= 896:                                       # the batched score vector is kept for queries of up to 896 rows (fsgpu.h)
            assert (ctx.gapless_scores_multi(k).astype(np.int32) == wants[k]).all(), ("scan_multi, scores", L, k)
        _same_hits(got[k], gm.select(wants[k], 15, -1, 60), ("scan_multi, hits", L, k))

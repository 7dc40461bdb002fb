"""k_gapless HALVES (classes 17 .. 36 of fsgpu_gapless_scan_multi: two queries in the halves of every register, 16 lanes a target, a stripe in two
passes of four targets) held to tests/gapless_model.py: whole score slices and hit lists, exact equality everywhere.  Profiles that come from
prefilter_profile meet the C oracle as well.  The pairing rule itself: tests/test_gapless_pairing.py."""
import ctypes as C

import numpy as np
import pytest

import gapless_model as gm
import helpers
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

PAIR_MAX_CLASS = 16            # classes up to this one: the PAIRED kernels, a launch of their own for an odd member out


def _db_from(seqs3):
    lens = np.array([len(x) for x in seqs3], np.int32)
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3 = np.full(int(offsets[-1]), 20, np.uint8)
    for k, s in enumerate(seqs3):
        d3[offsets[k]:offsets[k] + lens[k]] = s
    return synth.PaddedDB(d3, None, offsets, lens)


def _klass(L):
    return max(1, (L + 15) // 16)


def _expected_launches(lengths):
    """the launches of one call, unchanged by HALVES: classes up to 16 with two members or more one paired launch and one more for an odd member
    out, every other class present one launch"""
    members = {}
    for L in lengths:
        members[_klass(L)] = members.get(_klass(L), 0) + 1
    return sum((1 + m % 2) if (c <= PAIR_MAX_CLASS and m >= 2) else 1 for c, m in members.items())


def _segments(db, klass, waves):
    """column segments among the items the scan's planner makes of this database for a class"""
    lens = np.sort(np.asarray(db.lengths, np.int64), kind="stable")
    sl = np.array([(int(lens[a:a + 8].max()) + 15) // 16 for a in range(0, len(lens), 8)], np.uint32)
    items = np.zeros(4 * len(sl) + 4096, np.uint64)
    n = api.lib().fsgpu_gapless_plan_items(sl.ctypes.data_as(C.c_void_p), len(sl), klass, float(waves), items.ctypes.data_as(C.c_void_p), len(items), None)
    assert 0 < n <= len(items)
    return int(((items[:n] >> np.uint64(31)) & np.uint64(1)).sum())


def _placement(lengths):
    cls = np.array([_klass(L) for L in lengths], np.int32)
    lc, rec, half = (np.zeros(len(cls), np.int32) for _ in range(3))
    assert api.lib().fsgpu_gapless_pair_halves(cls.ctypes.data, len(cls), lc.ctypes.data, rec.ctypes.data, half.ctypes.data) >= 0
    return lc, rec, half


@pytest.fixture(scope="module", autouse=True)
def cus():
    """CUs of the device.  autouse: torch asks before the library opens the device, whichever test of the file is selected (as bench.py does)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class Query:
    """a profile, its uncapped model scores against one database (computed once), a cap"""

    def __init__(self, pssm, cap, packed, raw=None):
        self.pssm, self.cap, self.L = pssm, cap, pssm.shape[1]
        self.raw = gm.best_runs(pssm, packed) if raw is None else raw
        self.want = np.minimum(self.raw, gm.clamp(cap)).astype(np.int32)

    def capped(self, cap):
        return Query(self.pssm, cap, None, self.raw)


def _real(m, q3, packed, db):
    pssm, cap = api.prefilter_profile(m, q3, True, 0.15)
    q = Query(pssm, cap, packed)
    assert (helpers.o_ungapped_scores(q3, db, True) == q.want).all()       # the model and the C oracle agree before the device is asked
    return q


def _crafted(rng, L, p):
    return rng.choice(np.array([-128, -1, 0, 1, 127], np.int8), size=(21, L), p=p)


PAIR_CLASSES = (17, 36, 19, 29, 18)           # even R at both ends of the range, odd R (the Keep / Both fold of the last register), R % 4 == 2
REAL_LENGTHS = [L for R in PAIR_CLASSES for L in (16 * R - 15, 16 * R)] + [16 * 19 + 1, 312, 320, 321, 330, 336,      # classes 20 and 21, three each
                                                                           340, 353, 360, 368, 241, 256, 577, 592]    # 22; 23 x 3; 16 x 2; 37 x 2


@pytest.fixture(scope="module")
def world(cus):
    rng = np.random.default_rng(20260)
    q3 = [rng.choice(20, size=L).astype(np.uint8) for L in REAL_LENGTHS]
    qa = [rng.choice(20, size=L).astype(np.uint8) for L in REAL_LENGTHS]
    # short background targets keep the model's loop in seconds; the planted homologs are as long as their queries
    base = synth.make_db(588, (q3, qa), seed=29, homologs_per_query=1, mask_frac=0.02, mean_len=25, lo=2, hi=900)
    seqs = [base.seq(i, unmask=False) for i in range(base.n)]
    seqs += [rng.choice(20, size=L).astype(np.uint8) for L in (1, 15, 16, 17, 1, 17, 901, 1357, 999, 1203, 2100, 2300, 2500, 2700)]
    # a stripe of more than 2 * 37 chunks: the planner cuts column segments for every class used here
    seqs += [np.concatenate([q3[3], rng.choice(20, size=50).astype(np.uint8), q3[-1], q3[1]])[:1811]]
    db = _db_from(sorted(seqs, key=len))
    assert db.n == 603 and db.n % 8 and db.lengths.min() == 1 and (db.lengths > 896).sum() >= 8 and (db.data3di >= 32).any()
    assert {1, 15, 16, 17} <= set(db.lengths.tolist())
    for R in set(_klass(L) for L in REAL_LENGTHS):
        assert _segments(db, R, cus * 3 * 4) > 0, R
    packed = gm.pack(db)
    m = api.Matrix(0, 2.0)
    queries = {L: _real(m, q, packed, db) for L, q in zip(REAL_LENGTHS, q3)}
    ctx = api.Context(0)
    ctx.load_db(db)
    yield dict(db=db, packed=packed, q=queries, ctx=ctx, m=m, rng=rng)
    ctx.close()


def _check_batch(ctx, batch, what, idents=None, min_score=0, max_res=10, launches=True):
    """one fsgpu_gapless_scan_multi call: the launch count of the standing rule, every member's slice and hit list against its own model"""
    idents = [-1] * len(batch) if idents is None else idents
    hits = ctx.gapless_scan_multi([(q.pssm, q.cap, i) for q, i in zip(batch, idents)], min_score, max_res)
    assert len(hits) == len(batch)
    if launches:
        assert ctx.gapless_last_batch() == (_expected_launches([q.L for q in batch]), len(batch)), what
    for k, (q, ident) in enumerate(zip(batch, idents)):
        got = ctx.gapless_scores_multi(k).astype(np.int32)
        assert (got == q.want).all(), (what, k, q.L, np.flatnonzero(got != q.want)[:10])
        want = gm.select(q.want, min_score, ident, max_res)
        assert len(hits[k]) == len(want) and (hits[k]["id"] == want["id"]).all() and (hits[k]["score"] == want["score"]).all(), (what, k, q.L)
    return hits


def test_pairs_of_every_fold_both_orders(world):
    """lengths 16R - 15 and 16R share the registers of class R, for R = 17 and 36 (even), 19 and 29 (odd: Keep / Both fold), 18; both orders, the
    two members with different caps; one launch per class"""
    ctx, q = world["ctx"], world["q"]
    batch = []
    for R in PAIR_CLASSES:
        batch += [q[16 * R - 15].capped(37 + R), q[16 * R]]
    lc, rec, half = _placement([x.L for x in batch])
    assert half.tolist() == [0, 1] * len(PAIR_CLASSES)
    assert all(a.cap != b.cap and (a.want == a.cap).any() and (a.want < a.cap).any() and b.want.max() > a.cap for a, b in zip(batch[::2], batch[1::2]))
    _check_batch(ctx, batch, "A short, B full")
    assert ctx.gapless_last_batch()[0] == len(PAIR_CLASSES)
    swapped = [batch[k ^ 1] for k in range(len(batch))]
    _check_batch(ctx, swapped, "A full, B short")
    # one class at a time: the same slices whatever else the call holds
    for R in (19, 36):
        _check_batch(ctx, [q[16 * R].capped(255), q[16 * R - 15].capped(21)], ("alone", R))
        assert ctx.gapless_last_batch()[0] == 1


def test_a_saturated_half_leaves_the_other_alone(world):
    """127 everywhere drives one half of every register to the FP16 ceiling (2048) on every target of 17 residues or more; the other half holds
    a sparse real profile or a crafted one of {-128, -1, 0, 1, 127}.  Both orders."""
    ctx, q, packed, rng = world["ctx"], world["q"], world["packed"], world["rng"]
    R = 19
    full = Query(np.full((21, 16 * R - 3), 127, np.int8), 255, packed)
    assert (full.raw > 2048).sum() == (world["db"].lengths >= 17).sum() > 50 and full.want.max() == 255
    mixed = Query(_crafted(rng, 16 * R, [0.25, 0.35, 0.1, 0.25, 0.05]), 200, packed)
    real = q[16 * R]
    assert real.raw.max() < 2048 and (real.want != full.want).any() and (mixed.want != full.want).any()
    for batch in ([full, real], [real, full], [mixed, full], [full, mixed], [full, full.capped(100)]):
        _check_batch(ctx, batch, "saturated")
        assert ctx.gapless_last_batch()[0] == 1


def test_three_of_one_class_alone(world):
    """one launch; the last record runs without a B"""
    ctx, q = world["ctx"], world["q"]
    batch = [q[353], q[360].capped(33), q[368]]
    lc, rec, half = _placement([x.L for x in batch])
    assert lc.tolist() == [23] * 3 and rec.tolist() == [0, 0, 1] and half.tolist() == [0, 1, 0]
    _check_batch(ctx, batch, "three of class 23")
    assert ctx.gapless_last_batch() == (1, 3)


def test_odd_member_out_moves_up_a_class(world):
    """three members each of classes 20 and 21: two launches, the third of class 20 -- 320 residues, every row of its class in use -- rides as B
    of class 21's last record; all six slices exact.  In both orders of the classes in the call."""
    ctx, q = world["ctx"], world["q"]
    batch = [q[16 * 19 + 1], q[312].capped(50), q[320], q[321].capped(44), q[330], q[336]]
    lc, rec, half = _placement([x.L for x in batch])
    assert lc.tolist() == [20, 20, 21, 21, 21, 21] and rec.tolist() == [0, 0, 1, 0, 0, 1] and half.tolist() == [0, 1, 1, 0, 1, 0]
    _check_batch(ctx, batch, "20 + 21")
    assert ctx.gapless_last_batch() == (2, 6)
    mixed = [batch[k] for k in (5, 0, 3, 2, 4, 1)]                              # now 312 residues move up, beside 330
    lc, rec, half = _placement([x.L for x in mixed])
    assert (lc[5], rec[5], half[5]) == (21, 1, 1) and (lc[4], rec[4], half[4]) == (21, 1, 0)
    _check_batch(ctx, mixed, "20 + 21 interleaved")
    assert ctx.gapless_last_batch() == (2, 6)


def test_single_member_and_the_neighbouring_kernels(world):
    """one member of class 22: the unpaired kernel, one launch.  Classes 16 (PAIRED) and 37 (8-wave workgroups, unpaired) beside classes of the
    range: the launch counts of the standing rule, every slice exact."""
    ctx, q = world["ctx"], world["q"]
    _check_batch(ctx, [q[340]], "class 22 alone")
    assert ctx.gapless_last_batch() == (1, 1)
    # the single member of class 22 as the host of class 20's odd member out (320 residues, two classes below): still one launch per class
    guest = [q[16 * 19 + 1], q[340].capped(61), q[312], q[320].capped(48)]
    lc, rec, half = _placement([x.L for x in guest])
    assert lc.tolist() == [20, 22, 20, 22] and rec.tolist() == [0, 0, 0, 0] and half.tolist() == [0, 0, 1, 1]
    _check_batch(ctx, guest, "a guest of a single member")
    assert ctx.gapless_last_batch() == (2, 4)
    batch = [q[241], q[577], q[340], q[16 * 17], q[256], q[592], q[16 * 17 - 15], q[353], q[360], q[368], q[16 * 36]]
    _check_batch(ctx, batch, "16, 37 and the range")
    assert ctx.gapless_last_batch() == (1 + 1 + 1 + 1 + 1 + 1, len(batch))       # classes 16, 37, 22, 17, 23, 36
    _check_batch(ctx, [q[241], q[256], q[241].capped(9), q[577], q[592]], "16 x 3, 37 x 2")
    assert ctx.gapless_last_batch() == (2 + 1, 5)


def test_hit_lists_of_an_a_and_a_b_member(world):
    """min_score and identity ids: a query A whose identity target fails the score filter, a query B whose identity target is its best"""
    ctx, q = world["ctx"], world["q"]
    batch = [q[16 * 29 - 15], q[16 * 29], q[353], q[360], q[368]]
    lc, rec, half = _placement([x.L for x in batch])
    assert half.tolist() == [0, 1, 0, 1, 0]
    idents = [int(np.argmin(batch[0].want)), int(np.argmax(batch[1].want)), -1, int(np.argmin(batch[3].want)), 7]
    assert batch[0].want[idents[0]] <= 15 and batch[3].want[idents[3]] <= 15
    hits = _check_batch(ctx, batch, "hit lists", idents, min_score=15, max_res=50)
    assert hits[1]["id"][0] == idents[1]
    hits = _check_batch(ctx, batch, "long lists", idents, min_score=15, max_res=600)        # long enough for the identity targets below the filter
    assert idents[0] in hits[0]["id"] and idents[3] in hits[3]["id"]
    # max_res cuts inside a tie
    _check_batch(ctx, batch, "short lists", idents, min_score=0, max_res=3)


@pytest.mark.parametrize("n", [3, 5])
def test_tiny_databases(n):
    """3 targets: the second pass of the only stripe is empty and is skipped; 5 targets: it holds one target"""
    rng = np.random.default_rng(40 + n)
    seqs = [rng.choice(20, size=L).astype(np.uint8) for L in (9, 33, 300, 17, 290)[:n]]
    db = _db_from(sorted(seqs, key=len))
    packed = gm.pack(db)
    ctx = api.Context(0)
    ctx.load_db(db)
    try:
        p = [np.ascontiguousarray(_crafted(rng, L, [0.05, 0.4, 0.1, 0.3, 0.15])) for L in (16 * 19 - 15, 16 * 19, 16 * 19 - 7, 16 * 17, 16 * 17 - 1)]
        batch = [Query(x, c, packed) for x, c in zip(p, (255, 90, 40, 255, 120))]
        assert all(x.want.max() > 0 for x in batch)
        _check_batch(ctx, batch, ("tiny", n))
        assert ctx.gapless_last_batch() == (2, 5)
    finally:
        ctx.close()

"""Every k_gapless instantiation the library holds, run on the probe world of tests/gapless_sweep_cases.py and held to tests/gapless_model.py: whole
score vectors and hit lists, exact equality.  Which kernel a length runs in is read from fsgpu_gapless_shape and fsgpu_gapless_pair_halves; what the
probes are built to meet is asserted without a GPU in tests/test_gapless_sweep_cases.py.

  untiled   R = 1..56 through fsgpu_gapless_scan (no pairing rule can turn a lone query into anything else)
  PAIRED    2R registers, R = 1..16: two members per fsgpu_gapless_scan_multi call, both orders
  HALVES    R = 17..36: two members per call, both orders, and three (the last record without a B)
  tiled     R = 22..32 at the first lengths of 2, 3 and 4 tiles, alone and beside two short queries in one batched call
One context per test; the classes of a test are visited in descending order with every member and again in ascending order with a few."""
import ctypes as C

import numpy as np
import pytest

import gapless_model as gm
import gapless_sweep_cases as W
from foldseek_amd import api

pytestmark = pytest.mark.gpu

TILED_R = list(range(22, 33))


@pytest.fixture(scope="module", autouse=True)
def cus():
    """CUs of the device.  autouse: torch asks before the library opens the device, whichever test of the file is selected (as bench.py does)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def world(cus):
    db = W.DB(W.TARGETS)
    sl = np.array(W.STRIPE_CHUNKS, np.uint32)
    items = np.zeros(4096, np.uint64)
    for R in range(1, W.UNTILED_MAX + 1):               # column segments for every class on this device
        n = api.lib().fsgpu_gapless_plan_items(sl.ctypes.data_as(C.c_void_p), len(sl), R, float(cus * 3 * 4), items.ctypes.data_as(C.c_void_p), len(items), None)
        assert 0 < n <= len(items) and ((items[:n] >> np.uint64(31)) & np.uint64(1)).sum() > 0, R
    return dict(db=db, packed=gm.pack(db))


@pytest.fixture
def ctx(world):
    c = api.Context(0)
    c.load_db(world["db"])
    yield c
    c.close()


def _same_hits(hits, want, what):
    assert len(hits) == len(want) and (hits["id"] == want["id"]).all() and (hits["score"] == want["score"]).all(), what


def _single(ctx, p, what, ident=-1, min_score=30, max_res=12):
    hits = ctx.gapless_scan(p.pssm, p.cap, min_score=min_score, identity=ident, max_res=max_res)
    got = ctx.gapless_scores().astype(np.int32)
    assert (got == p.want).all(), (what, p.L, np.flatnonzero(got != p.want)[:10], got[got != p.want][:10], p.want[got != p.want][:10])
    _same_hits(hits, gm.select(p.want, min_score, ident, max_res), (what, p.L))


def _batch(ctx, members, launches, what, min_score=30, max_res=12):
    idents = [(7 * k + 3) % W.N_SHORT for k in range(len(members))]
    hits = ctx.gapless_scan_multi([(p.pssm, p.cap, i) for p, i in zip(members, idents)], min_score, max_res)
    assert ctx.gapless_last_batch() == (launches, len(members)), what
    for k, (p, ident) in enumerate(zip(members, idents)):
        got = ctx.gapless_scores_multi(k).astype(np.int32)
        assert (got == p.want).all(), (what, k, p.L, np.flatnonzero(got != p.want)[:10], got[got != p.want][:10], p.want[got != p.want][:10])
        _same_hits(hits[k], gm.select(p.want, min_score, ident, max_res), (what, k, p.L))


_MEMBERS = {}               # class -> its probe members with their model scores: computed once, shared by the tests of the file, never changed


def _members(R, packed):
    if R in _MEMBERS:
        return _MEMBERS[R]
    full, short, sat = W.class_probes(R)
    members = _MEMBERS[R] = full + [short, sat]
    for p in members:
        p.model(packed)
        assert api.gapless_shape(p.L) == (1, R)
    assert sat.want.max() == 255 and all(0 < p.want.max() < p.cap for p in members[:-1])
    return members


UNTILED_GROUPS = [(1, 8), (9, 16), (17, 24), (25, 32), (33, 38), (39, 44), (45, 50), (51, 56)]


@pytest.mark.parametrize("lo,hi", UNTILED_GROUPS)
def test_untiled_alone(lo, hi, world, ctx):
    members = {R: _members(R, world["packed"]) for R in range(lo, hi + 1)}
    for R in range(hi, lo - 1, -1):
        for k, p in enumerate(members[R]):
            _single(ctx, p, ("down", R, k), ident=(5 * k + R) % W.N_SHORT)
    for R in range(lo, hi + 1):
        for k in (0, -2, -1):
            _single(ctx, members[R][k], ("up", R, k), min_score=0, max_res=200)


@pytest.mark.parametrize("lo,hi", [(1, 8), (9, 16)])
def test_paired(lo, hi, world, ctx):
    """both queries of a PAIRED kernel: every member of a class once as query A (lanes 0..3) and once as query B (lanes 4..7)"""
    members = {R: _members(R, world["packed"]) for R in range(lo, hi + 1)}
    for R in range(hi, lo - 1, -1):
        m = members[R]
        pairs = [(m[-2], m[0])] + [(m[k], m[(k + 1) % len(m)]) for k in range(0, len(m), 2)]
        for a, b in pairs + [(b, a) for a, b in pairs]:
            _batch(ctx, [a, b], 1, ("paired", R, a.L, b.L))
    for R in range(lo, hi + 1):
        m = members[R]
        _batch(ctx, [m[0], m[-1]], 1, ("up", R))
        _batch(ctx, [m[-2], m[0], m[-1]], 2, ("up, three", R))                 # the third member alone in the unpaired kernel


def _placement(lengths):
    cls = np.array([api.gapless_shape(L)[1] for L in lengths], np.int32)
    lc, rec, half = (np.zeros(len(cls), np.int32) for _ in range(3))
    assert api.lib().fsgpu_gapless_pair_halves(cls.ctypes.data, len(cls), lc.ctypes.data, rec.ctypes.data, half.ctypes.data) >= 0
    return lc.tolist(), rec.tolist(), half.tolist()


@pytest.mark.parametrize("lo,hi", [(17, 23), (24, 30), (31, 36)])
def test_halves(lo, hi, world, ctx):
    """both halves of every register: every member of a class once as query A (low) and once as query B (high); the member of 16R - 15 residues
    beside one of 16R under another cap, both orders; three members, the last record without a B"""
    members = {R: _members(R, world["packed"]) for R in range(lo, hi + 1)}
    for R in range(hi, lo - 1, -1):
        m = members[R]
        full, short, sat = m[:-2], m[-2], m[-1]
        assert short.L == 16 * R - 15 and full[0].L == 16 * R and short.cap != full[0].cap
        pairs = [(short, full[0]), (sat, full[-1])] + [(m[k], m[(k + 1) % len(m)]) for k in range(0, len(m), 2)]
        for a, b in pairs + [(b, a) for a, b in pairs]:
            assert _placement([a.L, b.L]) == ([R, R], [0, 0], [0, 1])
            _batch(ctx, [a, b], 1, ("halves", R, a.L, b.L))
        three = [full[0], short, full[-1]]
        assert _placement([p.L for p in three]) == ([R] * 3, [0, 0, 1], [0, 1, 0])
        _batch(ctx, three, 1, ("no B", R))
    for R in range(lo, hi + 1):
        m = members[R]
        _batch(ctx, [m[-2], m[0]], 1, ("up", R))
        _batch(ctx, [m[1], m[-1], m[-2]], 1, ("up, no B", R))


@pytest.mark.parametrize("lo,hi", [(22, 24), (25, 27), (28, 30), (31, 32)])
def test_tiled(lo, hi, world, ctx):
    """row tiles: the single entry at every length, and the first profile of every length as the middle member of a batched call (the entry runs it
    through the single path; the two short members share a PAIRED launch)"""
    packed = world["packed"]
    lengths = W.tiled_lengths(api.gapless_shape, TILED_R)
    probes = {}
    for R in range(lo, hi + 1):
        assert [n for L, n in lengths[R]] == ([2] if R >= 29 else []) + [3] + ([4] if R >= 25 else [])
        for L, n in lengths[R]:
            assert api.gapless_shape(L) == (n, R)
            probes[R, L] = [p.model(packed) for p in W.tiled_probes(R, L, n, full=(n == 3))]
    short = [p.model(packed) for p in W.class_probes(3)[0][:2]]
    n_all = world["db"].n
    for (R, L), ps in sorted(probes.items(), reverse=True):
        for k, p in enumerate(ps):
            assert 0 < p.want.max() < p.cap
            _single(ctx, p, ("down", R, L, k), ident=(3 * k + R) % W.N_SHORT)
        # beside two short queries; min_score -1 and max_res = n make the hit list of the tiled member its whole score vector
        batch = [short[0], ps[0], short[1]]
        hits = ctx.gapless_scan_multi([(p.pssm, p.cap, -1) for p in batch], -1, n_all)
        assert ctx.gapless_last_batch() == (2, 3)
        for k, p in enumerate(batch):
            _same_hits(hits[k], gm.select(p.want, -1, -1, n_all), ("batched", R, L, k))
            if k != 1:
                assert (ctx.gapless_scores_multi(k).astype(np.int32) == p.want).all(), ("batched", R, L, k)
        with pytest.raises(api.FsgpuError, match="no batched scan results for this query"):
            ctx.gapless_scores_multi(1)
    for (R, L), ps in sorted(probes.items()):
        _single(ctx, ps[0], ("up", R, L), min_score=0, max_res=200)

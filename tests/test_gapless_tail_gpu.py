"""The last chunk of a stripe in k_gapless: only its real columns run (a loop over single columns behind the unrolled 16-column body), and an odd
register class folds its last register across two columns.  Every target's score, from the batched scan (fsgpu_gapless_scan_multi +
fsgpu_gapless_scores_multi) and from the single-query scan (fsgpu_gapless_scan + fsgpu_gapless_scores), equals tests/gapless_model.py exactly.

Two databases.  "residues": 2400 targets whose stripes' longest members cover every residue mod 16, among them, for every query, a target that ends
with a copy of the query's last residues and is the longest of its stripe: the best diagonal ends in the stripe's very last real column.
"split": 2000 short targets and one of 2000 columns, whose stripe the planner cuts into column segments for every class of the queries; it ends
with the same planted tails."""
import ctypes as C

import numpy as np
import pytest

import gapless_model as gm
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

# query lengths: class R = ceil(L / 16).  9 and 16 share a launch of the paired kernel (k_gapless<2, false, true>), 11 is the odd one out of class 1
# (k_gapless<1>); 331 / 366 are R = 21 / 23 (odd, both residues mod 4), 352 / 375 R = 22 / 24, 589 R = 37 (8-wave workgroups), 900 runs as two row
# tiles of R = 29 (the tiled instantiations, which run every padded column as before)
LENGTHS = (9, 16, 11, 331, 366, 352, 375, 589, 900)
CLASSES = {1: 3, 21: 1, 23: 1, 22: 1, 24: 1, 37: 1}
TAIL = 10                      # planted residues: few enough for the diagonal to stay below the score cap


def _db_from(seqs3):
    lens = np.array([len(x) for x in seqs3], np.int32)
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3 = np.full(int(offsets[-1]), 20, np.uint8)
    for k, s in enumerate(seqs3):
        d3[offsets[k]:offsets[k] + lens[k]] = s
    return synth.PaddedDB(d3, None, offsets, lens)


def _stripe_columns(db):
    """real columns per 8-target stripe, stripes along the length order (fsgpu_db_load)"""
    lens = np.sort(np.asarray(db.lengths, np.int64), kind="stable")
    return np.array([int(lens[a:a + 8].max()) for a in range(0, len(lens), 8)], np.int64)


def _segments(db, klass, waves):
    """column segments among the items the scan's planner makes of this database for a class"""
    sl = ((_stripe_columns(db) + 15) // 16).astype(np.uint32)
    items = np.zeros(4 * len(sl) + 4096, np.uint64)
    n = api.lib().fsgpu_gapless_plan_items(sl.ctypes.data_as(C.c_void_p), len(sl), klass, float(waves), items.ctypes.data_as(C.c_void_p), len(items), None)
    assert 0 < n <= len(items)
    return int(((items[:n] >> np.uint64(31)) & np.uint64(1)).sum())


class World:
    pass


@pytest.fixture(scope="module")
def world():
    import torch
    w = World()
    w.cus = torch.cuda.get_device_properties(0).multi_processor_count            # torch asks before the library opens the device (as bench.py does)
    rng = np.random.default_rng(20261018)
    w.q3 = [rng.choice(20, size=L).astype(np.uint8) for L in LENGTHS]
    m = api.Matrix(0, 2.0)
    w.profiles = [api.prefilter_profile(m, q, True, 0.15) for q in w.q3]
    noise = lambda T: rng.choice(21, size=T).astype(np.uint8)
    tails = [q[-min(TAIL, len(q)):] for q in w.q3]

    # "residues": background of 1..40 columns; 16 stripes' worth of longer targets, 8 of one length each, lengths 64 + 17 k (every residue mod 16);
    # then one stripe per query whose longest member (alone at its length) ends with the query's tail
    seqs = [noise(int(rng.integers(1, 41))) for _ in range(2400 - 16 * 8 - 8 * len(LENGTHS))]
    for k in range(16):
        seqs += [noise(64 + 17 * k) for _ in range(8)]
    w.planted = []
    for k, t in enumerate(tails):
        T = 400 + 21 * k + (1 if (400 + 21 * k) % 16 == 0 else 0)                 # distinct, never a multiple of 16
        seqs += [noise(T - 1) for _ in range(7)]
        seqs.append(np.concatenate([noise(T - len(t)), t]))
        w.planted.append(len(seqs) - 1)
    w.residues = _db_from(seqs)
    cols = _stripe_columns(w.residues)
    assert w.residues.n == 2400 and set((cols % 16).tolist()) == set(range(16))
    for k, p in enumerate(w.planted):
        T = int(w.residues.lengths[p])
        assert T % 16 != 0 and (cols == T).sum() == 1 and (w.residues.lengths == T).sum() == 1      # the longest of its stripe, alone at that length

    # "split": 2000 background targets and one of 2000 columns that ends with all the tails, the R = 23 query's last
    long_one = np.concatenate([noise(2000 - sum(len(t) for t in tails))] + [tails[k] for k in (0, 1, 2, 3, 5, 6, 7, 8, 4)])
    w.split = _db_from([noise(int(rng.integers(1, 41))) for _ in range(2000)] + [long_one])
    assert w.split.n == 2001 and int(w.split.lengths.max()) == 2000 == len(long_one)
    w.want = {}
    for name in ("residues", "split"):
        packed = gm.pack(getattr(w, name))
        w.want[name] = [gm.scores(pssm, cap, packed) for pssm, cap in w.profiles]
    w.ctx = {}
    for name in ("residues", "split"):
        w.ctx[name] = api.Context(0)
        w.ctx[name].load_db(getattr(w, name))
    yield w
    for c in w.ctx.values():
        c.close()


def test_inputs_are_what_the_cases_need(world):
    """the planted diagonals end in the last real column, below the cap: without that column the model itself gives less.  The long target's stripe
    is cut into column segments for every class the queries run in."""
    for k in (3, 4):                                                                # the R = 21 and R = 23 queries
        pssm, cap = world.profiles[k]
        t = world.residues.seq(world.planted[k], unmask=False)
        full, short = gm.scores_brute(pssm.tolist(), cap, [t[-3 * TAIL:], t[-3 * TAIL:-1]])
        assert short < full < gm.clamp(cap), (k, short, full, cap)
        assert world.want["residues"][k][world.planted[k]] >= full
    pssm, cap = world.profiles[4]
    t = world.split.seq(2000, unmask=False)
    full, short = gm.scores_brute(pssm.tolist(), cap, [t[-3 * TAIL:], t[-3 * TAIL:-1]])
    assert short < full < gm.clamp(cap) and world.want["split"][4][2000] >= full
    for R in CLASSES:
        assert _segments(world.split, R, world.cus * 3 * 4) >= 2, R
    spread = np.unique(np.concatenate(world.want["residues"]))
    assert spread.min() == 0 and len(spread) > 40


@pytest.mark.parametrize("name", ["residues", "split"])
def test_batched_scan_equals_the_model(world, name):
    ctx, want = world.ctx[name], world.want[name]
    hits = ctx.gapless_scan_multi([(pssm, cap, -1) for pssm, cap in world.profiles], 15, 40)
    # one launch per class, one more for the pair of class 1, one for the row-tiled query
    assert ctx.gapless_last_batch() == (len(CLASSES) + 1 + 1, len(LENGTHS))
    for k, L in enumerate(LENGTHS):
        if L <= 896:
            got = ctx.gapless_scores_multi(k).astype(np.int32)
            assert (got == want[k]).all(), (name, L, np.flatnonzero(got != want[k])[:10], got[got != want[k]][:10], want[k][got != want[k]][:10])
        sel = gm.select(want[k], 15, -1, 40)
        assert len(hits[k]) == len(sel) and (hits[k]["id"] == sel["id"]).all() and (hits[k]["score"] == sel["score"]).all(), (name, L)


@pytest.mark.parametrize("name", ["residues", "split"])
def test_single_query_scan_equals_the_model(world, name):
    ctx, want = world.ctx[name], world.want[name]
    for k, (pssm, cap) in enumerate(world.profiles):
        hits = ctx.gapless_scan(pssm, cap, min_score=15, identity=-1, max_res=40)
        got = ctx.gapless_scores().astype(np.int32)
        assert (got == want[k]).all(), (name, LENGTHS[k], np.flatnonzero(got != want[k])[:10], got[got != want[k]][:10], want[k][got != want[k]][:10])
        sel = gm.select(want[k], 15, -1, 40)
        assert len(hits) == len(sel) and (hits["id"] == sel["id"]).all() and (hits["score"] == sel["score"]).all(), (name, LENGTHS[k])

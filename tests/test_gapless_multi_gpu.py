"""The batched gapless scan (fsgpu_gapless_scan_multi: PAIRED instantiations of k_gapless, per-query records / queues / score slices, the
blockIdx.y form of the k_select passes) and what small databases never reach in the single-query path (selection over several chunks, the atomic
work queue, crafted profiles), held to tests/gapless_model.py: full score vectors and hit lists, exact equality everywhere.  Profiles that come
from prefilter_profile meet the C oracle as well."""
import ctypes as C

import numpy as np
import pytest

import gapless_model as gm
import helpers
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

SEL_CHUNK = 4096               # k_select.hpp kSelChunk: targets per workgroup of the selection passes
PAIR_MAX_CLASS = 16            # classes (16-row register counts) up to this one run two queries to a kernel


def _db_from(seqs3):
    """PaddedDB of 3Di code strings in the order given (no AA: prefilter only)"""
    lens = np.array([len(x) for x in seqs3], np.int32)
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3 = np.full(int(offsets[-1]), 20, np.uint8)
    for k, s in enumerate(seqs3):
        d3[offsets[k]:offsets[k] + lens[k]] = s
    return synth.PaddedDB(d3, None, offsets, lens)


def _sorted_db(seqs3):
    return _db_from(sorted(seqs3, key=len))


def _klass(L):
    return max(1, (L + 15) // 16)


def _expected_launches(lengths):
    """the pairing rule of fsgpu_gapless_scan_multi: per class of one-piece queries one launch of the paired kernel when it has two members or
    more (classes up to 16), one more for an odd one out; every other class one launch; a row-tiled query (> 896 residues) counts one"""
    members = {}
    for L in lengths:
        if L <= 896:
            members[_klass(L)] = members.get(_klass(L), 0) + 1
    return sum((1 + m % 2) if (c <= PAIR_MAX_CLASS and m >= 2) else 1 for c, m in members.items()) + sum(1 for L in lengths if L > 896)


def _stripe_chunks(db):
    """16-column chunks per 8-target stripe, stripes along the length order (fsgpu_db_load)"""
    lens = np.sort(np.asarray(db.lengths, np.int64), kind="stable")
    return np.array([(int(lens[a:a + 8].max()) + 15) // 16 for a in range(0, len(lens), 8)], np.uint32)


def _plan(db, klass, waves):
    """(items, items that are column segments) the scan's planner makes of this database for a class"""
    sl = _stripe_chunks(db)
    items = np.zeros(4 * len(sl) + 4096, np.uint64)
    n = api.lib().fsgpu_gapless_plan_items(sl.ctypes.data_as(C.c_void_p), len(sl), klass, float(waves), items.ctypes.data_as(C.c_void_p), len(items), None)
    assert 0 < n <= len(items)
    return int(n), int(((items[:n] >> np.uint64(31)) & np.uint64(1)).sum())


@pytest.fixture(scope="module", autouse=True)
def cus():
    """CUs of the device.  autouse: torch asks before the library opens the device, whichever test of the file is selected (as bench.py does)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _same_hits(hits, want, what=None):
    key = "id" if "id" in want.dtype.names else "key"
    assert len(hits) == len(want), (what, len(hits), len(want))
    assert (hits["id"] == want[key]).all() and (hits["score"] == want["score"]).all(), what


def _crafted(rng, L, p):
    return rng.choice(np.array([-128, -1, 0, 1, 127], np.int8), size=(21, L), p=p)


# ---- the database and the queries of 4a / 4b / 4f ---------------------------------------------------------------------------------------------
class Query:
    def __init__(self, q3, pssm, cap, packed, db, comp_bias=True):
        self.q3, self.pssm, self.cap, self.L = q3, pssm, cap, pssm.shape[1]
        self.want = gm.scores(pssm, cap, packed)
        if q3 is not None:                           # a profile of prefilter_profile: the model and the C oracle agree before the device is asked
            assert (helpers.o_ungapped_scores(q3, db, comp_bias) == self.want).all()


@pytest.fixture(scope="module")
def world(cus):
    rng = np.random.default_rng(20251)
    lens = []
    for R in range(1, 17):
        lens += [16 * R - 15, 16 * R] + ([16 * R - 7] if R % 2 else [])            # the pair, and for odd classes the odd one out
    lens += [16 * 17 - 9, 512, 513, 576, 577, 896, 897]                             # classes 17, 32, 33, 36, 37 (8-wave workgroups), 56; row tiles
    q3 = [rng.choice(20, size=L).astype(np.uint8) for L in lens]
    qa = [rng.choice(20, size=L).astype(np.uint8) for L in lens]
    # short background targets keep the model's loop in seconds; the planted homologs are as long as their queries
    base = synth.make_db(590, (q3, qa), seed=23, homologs_per_query=1, mask_frac=0.02, mean_len=25, lo=2, hi=900)
    seqs = [base.seq(i, unmask=False) for i in range(base.n)]
    seqs += [np.array([k], np.uint8) for k in (3, 17, 20)] + [rng.choice(20, size=L).astype(np.uint8) for L in (5, 6, 7, 901, 1357, 999)]
    # a stripe of more than 2 * 56 chunks: the planner cuts column segments for every class
    seqs += [np.concatenate([q3[-2], rng.choice(20, size=50).astype(np.uint8), q3[-1]])[:1811]]
    db = _sorted_db(seqs)
    assert db.n == 600 and db.lengths.min() == 1 and (db.lengths % 4 != 0).any() and (db.lengths > 16 * 56).sum() >= 4 and (db.data3di >= 32).any()
    packed = gm.pack(db)
    m = api.Matrix(0, 2.0)
    queries = [Query(q, *api.prefilter_profile(m, q, True, 0.15), packed, db) for q in q3]
    ctx = api.Context(0)
    ctx.load_db(db)
    yield dict(db=db, packed=packed, queries=queries, ctx=ctx, m=m)
    ctx.close()


def _check_batch(ctx, batch, idents, min_score, max_res, what):
    """one fsgpu_gapless_scan_multi call; every member's score slice and hit list against its own model (and the oracle's selection)"""
    hits = ctx.gapless_scan_multi([(q.pssm, q.cap, i) for q, i in zip(batch, idents)], min_score, max_res)
    assert len(hits) == len(batch)
    for k, (q, ident) in enumerate(zip(batch, idents)):
        if q.L <= 896:
            got = ctx.gapless_scores_multi(k).astype(np.int32)
            assert (got == q.want).all(), (what, k, q.L, np.flatnonzero(got != q.want)[:10])
        _same_hits(hits[k], gm.select(q.want, min_score, ident, max_res), (what, k, q.L))
        if q.q3 is not None:
            _same_hits(hits[k], helpers.o_prefilter_select(q.want, min_score, ident, max_res), (what, k, q.L))
    return hits


def test_every_paired_class_in_one_batch(world, cus):
    """4a: classes 1..16 as pairs of different length (16R - 15 in lanes 0..3, 16R in lanes 4..7), an unpaired third for the odd classes, the
    unpaired classes 17 / 32 / 33 / 36 / 37 / 56 and a row-tiled query, one call"""
    ctx, db, qs = world["ctx"], world["db"], world["queries"]
    for R in list(range(1, 17)) + [17, 32, 33, 36, 37, 56]:
        assert _plan(db, R, cus * 3 * 4)[1] > 0, R                                  # condition on the inputs: column segments occur for this class
    idents = [-1] * len(qs)
    # batch order inside a class is the call's order: the first two members are queries A and B of the pair, the third runs unpaired
    a3, b5, u7 = [[i for i, q in enumerate(qs) if _klass(q.L) == R] for R in (3, 5, 7)]
    idents[a3[0]] = int(np.argmin(qs[a3[0]].want))                                  # fails the score filter
    idents[b5[1]] = int(np.argmax(qs[b5[1]].want))
    idents[u7[2]] = int(np.argmin(qs[u7[2]].want))
    idents[len(qs) - 2] = 7
    assert qs[a3[0]].want[idents[a3[0]]] <= 15 and qs[u7[2]].want[idents[u7[2]]] <= 15
    _check_batch(ctx, qs, idents, 15, 50, "4a")
    launches, batched = ctx.gapless_last_batch()
    # the row-tiled member has no slice in the batch: its score vector through a scan of its own
    tiled = qs[-1]
    _same_hits(ctx.gapless_scan(tiled.pssm, tiled.cap, min_score=15, identity=-1, max_res=50), gm.select(tiled.want, 15, -1, 50), "row-tiled")
    assert tiled.L == 897 and (ctx.gapless_scores().astype(np.int32) == tiled.want).all()
    assert batched == len(qs) == 47
    assert launches == _expected_launches([q.L for q in qs]) == 8 * 2 + 8 * 1 + 6 + 1
    spread = np.unique(np.concatenate([q.want for q in qs]))
    assert spread.min() == 0 and spread.max() == max(q.cap for q in qs) and len(spread) > 50       # scores spread over 0..cap, the cap binds


def test_pairs_that_differ_where_a_bug_would_swap_them(world):
    """4b: the two members of a pair differ in cap and in profile (crafted against real), both orders; a one-residue query beside a 16-residue one,
    both orders.  Each slice equals its own model."""
    ctx, db, packed, m = world["ctx"], world["db"], world["packed"], world["m"]
    rng = np.random.default_rng(8)
    crafted = Query(None, _crafted(rng, 40, [0.25, 0.35, 0.1, 0.25, 0.05]), 255, packed, db)
    q3 = rng.choice(20, size=45).astype(np.uint8)
    pssm, cap = api.prefilter_profile(m, q3, True, 0.15)
    assert cap > 40
    real = Query(None, pssm, 40, packed, db)
    assert (real.want == np.minimum(helpers.o_ungapped_scores(q3, db, True), 40)).all()
    assert crafted.want.max() > 40 and (crafted.want != real.want).any()
    q16 = Query(None, _crafted(rng, 16, [0.1, 0.3, 0.1, 0.3, 0.2]), 200, packed, db)
    q1 = Query(None, np.arange(21, dtype=np.int8).reshape(21, 1) * 5 - 20, 77, packed, db)
    assert (q16.want != q1.want).any()
    for k, batch in enumerate(([crafted, real], [real, crafted], [q16, q1], [q1, q16])):
        _check_batch(ctx, batch, [-1, 3], 10, 60, ("4b", k))
        assert ctx.gapless_last_batch() == (1, 2)                                   # one launch for both: the paired kernel ran


# ---- 4c: crafted profiles --------------------------------------------------------------------------------------------------------------------
EXPECTED_CLAMP = {255: 255, 1: 1, 0: 0, -5: 0, 300: 255}                          # scoreCap -> what the entry makes of it: max(0, min(cap, 255))


def test_crafted_profiles_single_and_batched():
    """4c: entries from {-128, -1, 0, 1, 127} and a profile that is 127 everywhere, L = 1 / 16 / 17 / 300 / 896, targets of up to 2400 residues (sums run
    far past the 2048 the packed FP16 recurrence saturates at), every clamp of scoreCap"""
    rng = np.random.default_rng(77)
    tl = [1, 2, 3, 5, 7, 15, 16, 17, 31, 33, 64, 100, 129, 255, 300, 301, 600, 897, 1200, 2047, 2049, 2400, 2399, 1000]
    db = _sorted_db([rng.choice(21, size=T).astype(np.uint8) + (32 * (rng.random(T) < 0.03)).astype(np.uint8) for T in tl])
    packed = gm.pack(db)
    kinds = {"sparse": [0.25, 0.35, 0.1, 0.25, 0.05], "rich": [0.1, 0.1, 0.1, 0.1, 0.6], "flat": [0.2] * 5}
    profiles = []
    for L in (1, 16, 17, 300, 896):
        profiles += [_crafted(rng, L, p) for p in kinds.values()] + [np.full((21, L), 127, np.int8)]
    raw = [gm.best_runs(p, packed) for p in profiles]
    assert max(r.max() for r in raw) > 4 * 2048 and any(((r > 0) & (r < 255)).any() for r in raw)
    ctx = api.Context(0)
    ctx.load_db(db)
    for cap, clamp in EXPECTED_CLAMP.items():
        assert gm.clamp(cap) == clamp
        wants = [np.minimum(r, clamp).astype(np.int32) for r in raw]
        min_score = -1 if clamp == 0 else 0
        for p, want in zip(profiles, wants):
            hits = ctx.gapless_scan(p, cap, min_score=min_score, identity=2, max_res=10)
            got = ctx.gapless_scores().astype(np.int32)
            assert (got == want).all(), (cap, p.shape[1], got, want)
            _same_hits(hits, gm.select(want, min_score, 2, 10), (cap, p.shape[1]))
        hits = ctx.gapless_scan_multi([(p, cap, 2) for p in profiles], min_score, 10)
        assert ctx.gapless_last_batch()[0] == _expected_launches([p.shape[1] for p in profiles])
        for k, want in enumerate(wants):
            got = ctx.gapless_scores_multi(k).astype(np.int32)
            assert (got == want).all(), (cap, k, got, want)
            _same_hits(hits[k], gm.select(want, min_score, 2, 10), (cap, k))
    # one batch in which the two members of every pair carry different caps
    caps = [list(EXPECTED_CLAMP)[k % 5] for k in range(len(profiles))]
    hits = ctx.gapless_scan_multi([(p, c, -1) for p, c in zip(profiles, caps)], 0, 10)
    for k, (r, c) in enumerate(zip(raw, caps)):
        want = np.minimum(r, EXPECTED_CLAMP[c]).astype(np.int32)
        assert (ctx.gapless_scores_multi(k).astype(np.int32) == want).all(), (k, c)
        _same_hits(hits[k], gm.select(want, 0, -1, 10), (k, c))
    ctx.close()


# ---- 4d: selection over several chunks, chosen scores ----------------------------------------------------------------------------------------
def _column(values):
    """one-residue profile: letter k scores values[k], every other letter (X included) nothing"""
    p = np.full((21, 1), -128, np.int8)
    p[:len(values), 0] = values
    return p


@pytest.mark.parametrize("n", [4096, 4097, 8193])
def test_selection_over_chunks_with_chosen_scores(n):
    """4d: one-residue query against n one-residue targets, letters interleaved by id: the score vector is the one written down here.  n = 8193 is three
    chunks of the selection passes with one target in the last, 4097 two, 4096 one."""
    letters = (np.arange(n) % 4).astype(np.uint8)
    db = _db_from([letters[i:i + 1] for i in range(n)])
    packed = gm.pack(db)
    tie = (n - 1) % 4                                                               # the last id belongs to the tie group: the group reaches every chunk
    role = lambda hi, t, mid, lo: [dict(zip([(tie + 1) % 4, tie, (tie + 2) % 4, (tie + 3) % 4], (hi, t, mid, lo)))[k] for k in range(4)]
    vectors = {"equal": (_column([50] * 4), 30), "tie": (_column(role(90, 60, 40, 10)), 30), "tie2": (_column(role(35, 127, 31, 30)), 30),
               "none": (_column(role(30, 10, 0, -7)), 30), "zeros": (_column(role(0, -128, 5, 0)), -1)}
    ctx = api.Context(0)
    ctx.load_db(db)
    nchunks = (n + SEL_CHUNK - 1) // SEL_CHUNK
    wants, sizes, inside_second = {}, {}, {}
    for name, (col, min_score) in vectors.items():
        written = np.maximum(col[:, 0].astype(np.int32), 0)[letters]
        want = wants[name] = gm.scores(col, 255, packed)
        assert (want == written).all()
        sizes[name] = [1, n - 1, n, n + 5]
        if name in ("tie", "tie2"):
            # a cut inside the tie group, so that the ties kept (mTies) end inside the second chunk
            above = int((want > want[n - 1]).sum())
            members = np.flatnonzero(want == want[n - 1])
            in0, in1 = int((members < SEL_CHUNK).sum()), int(((members >= SEL_CHUNK) & (members < 2 * SEL_CHUNK)).sum())
            if nchunks > 1:
                sizes[name] += [above + in0, above + in0 + max(1, in1 // 2)]        # the ties kept end with the first chunk / inside the second
                inside_second[name] = sizes[name][-1] if in1 >= 2 else None
        identity = n - 1 if name == "none" else -1
        for max_res in sizes[name]:
            hits = ctx.gapless_scan(col, 255, min_score=min_score, identity=identity, max_res=max_res)
            got = ctx.gapless_scores().astype(np.int32)
            assert (got == written).all(), name
            sel = gm.select(want, min_score, identity, max_res)
            _same_hits(hits, sel, (name, max_res))
            if name == "none":
                assert sel.tolist() == [(n - 1, int(want[n - 1]))] and (n - 1) // SEL_CHUNK == nchunks - 1       # the identity id alone, from the last chunk
            elif len(sel) and (nchunks == 3 or (nchunks == 2 and sel["score"][-1] == want[n - 1])):
                # condition on the inputs: the tie group at the cut score spans at least two chunks (with two chunks the second holds the last id
                # alone, so there only the group of that id does)
                group = np.flatnonzero((want == sel["score"][-1]) & (want > min_score))
                assert len(np.unique(group // SEL_CHUNK)) >= 2, (name, max_res)
                if max_res == inside_second.get(name):
                    kept = sel["id"][sel["score"] == sel["score"][-1]]
                    assert kept.max() // SEL_CHUNK == 1 and len(kept) < len(group)
    # the same vectors as the four queries of one batch (two pairs): blockIdx.y form, another cut for every query
    for names, min_score in ((("equal", "tie", "none", "tie2"), 30), (("zeros", "tie", "equal", "tie2"), -1)):
        for max_res in sorted(set(sum((sizes[k] for k in names), []))):
            idents = [n - 1 if k == "none" else -1 for k in names]
            hits = ctx.gapless_scan_multi([(vectors[k][0], 255, i) for k, i in zip(names, idents)], min_score, max_res)
            assert ctx.gapless_last_batch() == (1, 4)
            for k, name in enumerate(names):
                assert (ctx.gapless_scores_multi(k).astype(np.int32) == wants[name]).all(), (name, max_res)
                _same_hits(hits[k], gm.select(wants[name], min_score, idents[k], max_res), (name, min_score, max_res))
    ctx.close()


# ---- 4e: the atomic work queue ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", ["4 waves", "8 waves"])
def test_waves_take_later_items_from_the_queue(block, monkeypatch, cus):
    """4e: with one workgroup per CU a launch has CUs * 4 waves (classes up to 36) or CUs * 8 (the 512-thread workgroups above); a database of more
    stripes than that makes every wave go to the queue for its later items.  12 500 targets of 1..60 residues are 1563 stripes, more than the 1024
    waves of the small workgroups on 256 CUs; the large ones have 2048 waves there, so their classes (40, 56) meet 20 000 targets of 1..20 residues,
    2500 stripes."""
    n, hi, classes, waves_per_block = (12500, 60, (1, 8, 16, 20), 4) if block == "4 waves" else (20000, 20, (40, 56), 8)
    stripes = (n + 7) // 8
    if stripes <= cus * waves_per_block:
        pytest.skip(f"{stripes} stripes do not exceed the {cus * waves_per_block} waves of a launch on {cus} CUs: no wave would reach the queue")
    rng = np.random.default_rng(n)
    q3 = [rng.choice(20, size=16 * R - int(rng.integers(0, 16))).astype(np.uint8) for R in classes]
    if block == "4 waves":
        q3.append(rng.choice(20, size=120).astype(np.uint8))                        # a second member of class 8: the paired kernel meets the queue too
    seqs = []
    for t in range(n):                                                              # half of the targets are pieces of the queries: scores spread
        T = int(rng.integers(1, hi + 1))
        q = q3[t % len(q3)]
        if t % 2 and len(q) >= T:
            a = int(rng.integers(0, len(q) - T + 1))
            s = np.where(rng.random(T) < 0.15, rng.integers(0, 20, T), q[a:a + T]).astype(np.uint8)
        else:
            s = rng.integers(0, 21, T).astype(np.uint8)
        seqs.append(s)
    db = _sorted_db(seqs)
    assert db.n == n and db.residues < 400000 and len(_stripe_chunks(db)) == stripes
    for R in classes:
        assert _plan(db, R, cus * 3 * 4)[0] >= stripes > cus * waves_per_block      # every stripe is at least one item
    monkeypatch.setenv("FSGPU_GAPLESS_BLOCKS_PER_CU", "1")                          # read when the context is created
    ctx = api.Context(0)
    ctx.load_db(db)
    m = api.Matrix(0, 2.0)
    packed = gm.pack(db) if block == "4 waves" else None
    profiles, wants = [], []
    for q in q3:
        pssm, cap = api.prefilter_profile(m, q, True, 0.15)
        # the model itself where its loop over the rows stays short, the C oracle for the longer queries
        want = gm.scores(pssm, cap, packed) if packed is not None and len(q) < 120 else helpers.o_ungapped_scores(q, db, True)
        profiles.append((pssm, cap)); wants.append(want)
        hits = ctx.gapless_scan(pssm, cap, min_score=20, identity=-1, max_res=300)
        got = ctx.gapless_scores().astype(np.int32)
        assert (got == want).all(), (len(q), np.flatnonzero(got != want)[:10])
        _same_hits(hits, gm.select(want, 20, -1, 300), len(q))
    assert len(np.unique(np.concatenate(wants))) > 40
    hits = ctx.gapless_scan_multi([(p, c, -1) for p, c in profiles], 20, 300)
    assert ctx.gapless_last_batch() == (len(classes), len(q3))
    for k, want in enumerate(wants):
        got = ctx.gapless_scores_multi(k).astype(np.int32)
        assert (got == want).all(), (k, np.flatnonzero(got != want)[:10])
        _same_hits(hits[k], gm.select(want, 20, -1, 300), k)
        _same_hits(hits[k], helpers.o_prefilter_select(want, 20, -1, 300), k)
    ctx.close()


# ---- 4f: state between calls -----------------------------------------------------------------------------------------------------------------
def test_state_between_calls_on_one_context(world):
    """4f: batches of 12, 3 and 20 queries on one fresh context (slices, queues and buffers regrown and reused), refused calls in between, single scans
    before and after batches"""
    db, qs = world["db"], world["queries"]
    ctx = api.Context(0)
    ctx.load_db(db)
    tiled = len(qs) - 1
    assert qs[tiled].L == 897
    pick = lambda idx: [qs[i] for i in idx]
    b12 = pick([40, 0, 1, 17, 18, 19, 41, 5, 6, 7, 44, 30])
    b3 = pick([45, 2, 3])
    b20 = pick([tiled, 10, 11, 12, 13, 14, 20, 21, 22, 23, 24, 42, 43, 45, 8, 9, 33, 34, 35, 0])
    _check_batch(ctx, b12, [-1] * 12, 15, 50, "12")
    assert ctx.gapless_last_batch() == (_expected_launches([q.L for q in b12]), 12)
    _check_batch(ctx, b3, [5, -1, -1], 15, 50, "3")
    assert ctx.gapless_scan_multi([], 15, 50) == []                                 # nq = 0: no error
    # refused queries leave the context usable
    for bad in ((np.zeros((21, 0), np.int8), 100, -1), (None, 100, -1)):
        with pytest.raises(api.FsgpuError, match="bad query"):
            ctx.gapless_scan_multi([(b3[0].pssm, b3[0].cap, -1), bad], 15, 50)
        _check_batch(ctx, b3, [-1, -1, 9], 15, 50, "after a refusal")
    _check_batch(ctx, b20, [-1] * 20, 15, 50, "20")
    assert ctx.gapless_last_batch() == (_expected_launches([q.L for q in b20]), 20)
    with pytest.raises(api.FsgpuError, match="no batched scan results for this query"):
        ctx.gapless_scores_multi(0)                                                 # the row-tiled member ran on its own
    for index in (-1, 20, 1000):
        with pytest.raises(api.FsgpuError, match="no batched scan results for this query"):
            ctx.gapless_scores_multi(index)
    # a single scan after a batch, a batch after a single scan
    for q in (qs[4], qs[tiled], qs[44]):
        hits = ctx.gapless_scan(q.pssm, q.cap, min_score=15, identity=-1, max_res=50)
        assert (ctx.gapless_scores().astype(np.int32) == q.want).all(), q.L
        _same_hits(hits, gm.select(q.want, 15, -1, 50), q.L)
        _check_batch(ctx, b3, [-1] * 3, 15, 50, ("after a single scan", q.L))
    ctx.close()

"""The device block aligner (k_block_backtrace, all three launch forms) against the INDEPENDENT model of the crate (tests/ba_model.py) instead of the host
restatement it was written from: every 3di case of oracle/ba_kat/cases.txt and every long case of tests/golden/ba_long/long_cases.txt.gz becomes one task of a direct
fsgpu_block_backtrace call (Context.block_backtrace: no host path behind it that could quietly recompute a hit), and status, start position, backtrace,
identical-residue count and the number of block sizes tried must be the model's frozen answer -- or, for the cases the model says the device cannot hold
(a block beyond 512 rows), exactly a hand-back.  Integer and string equality throughout.

What this still does not pin: the model and the restatement are two readings of scan_block.rs; the crate itself has never run here (no Rust toolchain)."""
import os

import numpy as np
import pytest

import btrace_cases as B
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu


def _edge_cases():
    """handcrafted pairs whose answers the model computes now (milliseconds each): end cells on the first row / column, one-residue query, prefixes exactly
    at and around the block sizes 32 and 128 on each axis"""
    rng = np.random.default_rng(20261018)
    _, sA = B.matrix_text(os.path.join(B.KAT, "mat_aa.txt"))
    _, s3 = B.matrix_text(os.path.join(B.KAT, "mat_3di.txt"))
    W, D, A = B.CODE["W"], B.CODE["D"], B.CODE["A"]
    one = int(sA[W, W] + s3[D, D])                       # a single strong match: the whole alignment when an end coordinate is 0
    assert one > 0
    u8 = lambda *x: np.array(x, np.uint8)  # noqa: E731
    out = []

    def add(name, qa, q3, ta, t3, score, bias=None, whole_query=False):
        bias = np.zeros(len(qa), np.int64) if bias is None else bias
        out.append((B.model_case(name, qa, q3, bias, ta, t3, score), whole_query))

    ta10, t310 = np.concatenate([np.full(9, A, np.uint8), u8(W)]), np.concatenate([np.full(9, A, np.uint8), u8(D)])
    add("edge_qEnd0", u8(W), u8(D), ta10, t310, one)
    add("edge_dbEnd0", ta10, t310, u8(W), u8(D), one)
    add("edge_both0", u8(W), u8(D), u8(W), u8(D), one)
    add("edge_query1", u8(W), u8(D), ta10, t310, one, whole_query=True)
    s8a, s83 = rng.integers(0, 20, 8).astype(np.uint8), rng.integers(0, 20, 8).astype(np.uint8)
    add("edge_same8", s8a, s83, s8a.copy(), s83.copy(), int(sum(sA[a, a] + s3[b, b] for a, b in zip(s8a, s83))))
    for n in (32, 33, 127, 128, 129):
        for axis in (0, 1):
            # a mutated copy with one 3-residue gap; the score requested is what the path "copy, gap, copy" is worth, recomputed here -- the model decides
            # whether the aligner reaches, overshoots or misses it, and the device must do the same
            a3, aa = rng.integers(0, 20, n).astype(np.uint8), rng.integers(0, 20, n).astype(np.uint8)
            cut = n // 2
            b3, ba = np.concatenate([a3[:cut], a3[cut + 3:]]), np.concatenate([aa[:cut], aa[cut + 3:]])
            score = int(sum(sA[x, x] + s3[y, y] for x, y in zip(ba, b3))) - 10 - 2
            bias = rng.integers(-3, 4, n)
            if axis == 0:                               # the query prefix is exactly n long
                score += int(bias[:cut].sum() + bias[cut + 3:].sum())
                add(f"edge_q{n}", aa, a3, ba, b3, score, bias)
            else:                                       # ... the target prefix
                bb = bias[:len(ba)]
                add(f"edge_t{n}", ba, b3, aa, a3, score + int(bb.sum()), bb)
    return out


def _inputs():
    """cases -> (cases, queries, padded database sorted by length, one task per case, end cells)"""
    rng = np.random.default_rng(20261017)
    cases = [(c, False) for c in B.short_cases() + B.long_cases()] + _edge_cases()
    queries, t3s, tas, ends = [], [], [], []
    for c, whole_query in cases:
        codes = lambda s: np.array([B.CODE[ch] for ch in s[::-1]], np.uint8)  # noqa: E731
        qa, q3, ta, t3 = codes(c.rqa), codes(c.rq3), codes(c.rta), codes(c.rt3)
        bias = np.array(c.rbias[::-1], np.int64)
        # residues BEHIND the end cell of both sequences (with X among them), bias values behind it on the query: a kernel that indexed from the sequence
        # end instead of from qEnd / dbEnd reads these
        nq, nt = (0 if whole_query else int(rng.integers(0, 41))), int(rng.integers(0, 41))
        qa, q3 = np.concatenate([qa, rng.integers(0, 21, nq).astype(np.uint8)]), np.concatenate([q3, rng.integers(0, 21, nq).astype(np.uint8)])
        ta, t3 = np.concatenate([ta, rng.integers(0, 21, nt).astype(np.uint8)]), np.concatenate([t3, rng.integers(0, 21, nt).astype(np.uint8)])
        bias = np.concatenate([bias, rng.integers(-30, 31, nq)])
        # the bias reaches the device as two int8 arrays that are added there
        lo, hi = np.maximum(-128, bias - 127), np.minimum(127, bias + 128)
        cbA = np.clip(rng.integers(-100, 101, len(bias)), lo, hi)
        cbS = bias - cbA
        assert (cbS >= -128).all() and (cbS <= 127).all() and (cbA + cbS == bias).all()
        queries.append((qa, q3, cbA.astype(np.int8), cbS.astype(np.int8)))
        # soft-masked (+32) residues in the target, inside the aligned prefix too: the aligner must see them unmasked
        for s in (ta, t3):
            m = rng.integers(0, len(s), size=1 + len(s) // 25)
            s[m] += 32
        tas.append(ta); t3s.append(t3)
        ends.append((len(c.rqa) - 1, len(c.rta) - 1))
    lens = np.array([len(x) for x in t3s], np.int32)
    order = np.argsort(lens, kind="stable")
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens[order] + 3) // 4 * 4)
    d3, da = np.full(offsets[-1], 20, np.uint8), np.full(offsets[-1], 20, np.uint8)
    target_of = np.zeros(len(lens), np.int64)
    for new, old in enumerate(order):
        d3[offsets[new]:offsets[new] + lens[old]] = t3s[old]
        da[offsets[new]:offsets[new] + lens[old]] = tas[old]
        target_of[old] = new
    db = synth.PaddedDB(d3, da, offsets, lens[order])
    tasks = [(k, int(target_of[k]), ends[k][0], ends[k][1], c.target) for k, (c, _w) in enumerate(cases)]
    return [c for c, _w in cases], queries, db, tasks, ends


@pytest.fixture(scope="module")
def world():
    os.environ.pop("FSGPU_BT_SPREAD", None)              # read once per process: the form is picked by the size of a call
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count          # (before the library opens the device, as bench.py does)
    cases, queries, db, tasks, ends = _inputs()
    ctx = api.Context(0)
    ctx.load_db(db)
    tables = B.device_tables()
    # a call has one pair of gap costs: the cases of each pair (10/1, 8/2, 3/1, 15/3) form a call of their own
    groups = {}
    for k, c in enumerate(cases):
        groups.setdefault((c.go, c.ge), []).append(k)

    def run(ks, pass2):
        """one fsgpu_block_backtrace call per gap-cost pair over the tasks ks (an index may occur several times); (records in the order of ks, tasks of
        the smallest and of the largest call)"""
        out, sizes = [None] * len(ks), []
        os.environ["FSGPU_BT_PASS2"] = "1" if pass2 else "0"
        try:
            for (go, ge), members in groups.items():
                members = set(members)
                pos = [p for p, k in enumerate(ks) if k in members]
                got = ctx.block_backtrace(*tables, queries, [tasks[ks[p]] for p in pos], go, ge)
                sizes.append(len(pos))
                for p, r in zip(pos, got):
                    out[p] = r
        finally:
            os.environ.pop("FSGPU_BT_PASS2", None)
        return out, min(sizes), max(sizes)

    yield dict(ctx=ctx, cases=cases, ends=ends, run=run, cus=cus, groups=groups, tables=tables, queries=queries)
    ctx.close()


def _check(world, ks, got, pass2):
    """every record against the model's frozen answer"""
    bad, seen = [], {"A": 0, "B": 0, "C": 0, 2: 0}
    for k, r in zip(ks, got):
        c = world["cases"][k]
        want = c.expected(*world["ends"][k])
        if c.cls == "B" and not pass2:
            want = dict(status=0, qStart=-1, dbStart=-1, identicalAA=0, backtrace="")
        sizes_ok = True
        if c.cls == "A":
            sizes_ok = r["blockSizes"] == c.attempts
        elif c.cls == "B" and pass2:
            sizes_ok = r["blockSizes"] >= c.attempts
        got_r = {x: r[x] for x in want}
        if got_r != want or not sizes_ok:
            bad.append((c.name, c.cls, c.attempts, {x: (str(v)[:60]) for x, v in r.items()}, {x: (str(v)[:60]) for x, v in want.items()}))
        seen[c.cls] += 1
        seen[2] += want["status"] == 2
    assert not bad, (len(bad), bad[:6])
    return seen


def test_one_alignment_per_wave_and_second_pass_follow_the_model(world):
    """every case once: at most 12 tasks per compute unit in a call, the one-alignment-per-wave form <128, 4, true>; the second pass <512, 4, true> takes
    what the first hands back"""
    ks = list(range(len(world["cases"])))
    got, _least, most = world["run"](ks, True)
    assert most <= 12 * world["cus"]
    seen = _check(world, ks, got, True)
    assert seen["A"] >= 850 and seen["B"] >= 50 and seen["C"] >= 8 and seen[2] >= 20, seen
    world["once"] = got


def test_four_alignments_per_wave_follow_the_model_in_any_order(world):
    """the same tasks repeated in a seeded shuffle until every call holds more than 12 per compute unit: the form <128, 16> with four alignments to a
    wave, neighbours of every size; each copy of a case must come back identical to the others and to the single call's"""
    n = len(world["cases"])
    rng = np.random.default_rng(5)
    ks = []
    for members in world["groups"].values():
        ks += list(np.repeat(members, (12 * world["cus"]) // len(members) + 1))
    ks = [int(k) for k in rng.permutation(ks)]
    got, least, _most = world["run"](ks, True)
    assert least > 12 * world["cus"]
    _check(world, ks, got, True)
    once = world.get("once") or world["run"](list(range(n)), True)[0]
    for k, r in zip(ks, got):
        assert r == once[k], (world["cases"][k].name, r, once[k])


def test_without_the_second_pass_class_b_comes_back_and_class_a_is_unchanged(world):
    n = len(world["cases"])
    ks = list(range(n))
    got = world["run"](ks, False)[0]
    _check(world, ks, got, False)
    once = world.get("once") or world["run"](ks, True)[0]
    nb = 0
    for k, r in zip(ks, got):
        c = world["cases"][k]
        if c.cls == "B":
            assert r["status"] == 0 and once[k]["status"] in (1, 2), c.name
            nb += 1
        elif c.cls == "A":
            assert r == once[k], c.name
    assert nb >= 50


def test_footprint_of_one_workgroup_per_cu_and_empty_call(world):
    """fsgpu_block_backtrace_footprint(ctx, 1) changes the grid, never an answer; a call without tasks is fine"""
    ctx, n = world["ctx"], len(world["cases"])
    ks = list(range(n))
    once = world.get("once") or world["run"](ks, True)[0]
    ctx.block_backtrace_footprint(1)
    try:
        got = world["run"](ks, True)[0]
    finally:
        ctx.block_backtrace_footprint(0)
    assert got == once
    assert ctx.block_backtrace(*world["tables"], world["queries"][:1], [], 10, 1) == []
    assert ctx.block_backtrace(*world["tables"], [], [], 10, 1) == []

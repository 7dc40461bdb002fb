"""The shapes fsgpu_gapless_shape gives every query length, and the conditions the probe world of tests/gapless_sweep_cases.py meets for every
k_gapless instantiation those shapes (and the pairing of fsgpu_gapless_scan_multi) can run -- all on the CPU, with tests/gapless_model.py alone.
Conditions on inputs, not measurements: every one is decided by the model's brute-force best cell (gm.best_cells) of an asserted (profile, target)
pair, whose score is the one the device sweep (tests/test_gapless_sweep_gpu.py) compares.

(a) every register, both halves, first / interior / last lane of a target group (A and B where two queries share a kernel): some pair has its one
    best cell in that row, and the score falls when the model's profile loses that row;
(b) a best cell in the last column of a stripe in a row of the last register, for stripes whose last chunk holds 1, 15 and 16 columns: column
    index in the chunk 0, 14 (even) and 15 (odd).  What this can and cannot reach in the kernel: a stripe's last chunk runs in the single-column
    loop (every column folds the last register alone) unless it is full, and then its last column has the odd index 15, which completes a Keep /
    Both pair; no item ends on a kept register.  The even and odd columns of an unrolled chunk are met by the targets that hold their run inside
    the first chunk (asserted below: both parities, for every class);
(c) a member of 16R - 15 residues beside those of 16R, and one that is 127 everywhere (uncapped score above 2048 where the class has the 17 rows
    that takes);
(d) row tiles: runs that cross every tile border and enter at a column = 0 mod 16, an odd one, an even one; 2 tiles where R allows, 3, 4;
(e) the planner cuts column segments for the class, and a best run starts before a segment's first own column and ends at or behind it."""
import ctypes as C

import numpy as np
import pytest

import gapless_model as gm
import gapless_sweep_cases as W
from foldseek_amd import api

TILED_R = list(range(22, 33))
WAVES = 256 * 3 * 4            # what fsgpu_gapless_scan plans for on the 256 CUs of an MI355X; the cut length does not depend on it while work / waves < 2R


@pytest.fixture(scope="module")
def shapes():
    """(row tiles, registers) of every length an entry takes"""
    return [None] + [api.gapless_shape(L) for L in range(1, api.FSGPU_MAX_SEQ_LEN + 1)]


def test_shape_of_every_length(shapes):
    """one piece of ceil(L / 16) = 1..56 registers up to 896 residues; beyond that ceil(L / 512) tiles of equal height, and exactly the register
    counts 22..32: the tiled kernels the library holds"""
    for L in range(1, 897):
        assert shapes[L] == (1, (L + 15) // 16), L
    assert {R for n, R in shapes[1:897]} == set(range(1, 57))
    tiled = shapes[897:]
    assert all(n == -(-L // 512) and n >= 2 for L, (n, R) in zip(range(897, 65536), tiled))
    assert all(16 * R * (n - 1) < L <= 16 * R * n for L, (n, R) in zip(range(897, 65536), tiled))        # the last tile is not empty, no row is left over
    assert {R for n, R in tiled} == set(TILED_R)
    first = {}
    for L, (n, R) in zip(range(897, 65536), tiled):
        first.setdefault(R, L)
    assert [first[R] for R in TILED_R] == [1025, 1057, 1105, 1153, 1201, 1249, 1297, 897, 929, 961, 993]
    assert {R for n, R in tiled if n == 2} == {29, 30, 31, 32} and {R for n, R in tiled if n == 3} == set(TILED_R)
    assert min(R for n, R in tiled if n >= 4) == 25 and shapes[65535] == (128, 32)
    for bad in (0, -1, 65536):
        with pytest.raises(api.FsgpuError):
            api.gapless_shape(bad)
    n = C.c_int(0)
    assert api.lib().fsgpu_gapless_shape(100, None, C.byref(n)) == -1 and api.lib().fsgpu_gapless_shape(100, C.byref(n), None) == -1


# ---- the database -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    return W.DB(W.TARGETS)


def _segments(klass):
    """the planner's items for the probe database: {stripe: sorted end chunks of its column segments}"""
    sl = np.array(W.STRIPE_CHUNKS, np.uint32)
    items = np.zeros(4096, np.uint64)
    n = api.lib().fsgpu_gapless_plan_items(sl.ctypes.data_as(C.c_void_p), len(sl), klass, float(WAVES), items.ctypes.data_as(C.c_void_p), len(items), None)
    assert 0 < n <= len(items)
    out = {}
    for it in items[:n]:
        if (int(it) >> 31) & 1:
            out.setdefault(int(it) >> 32, []).append(int(it) & 0xffff)
    return {s: sorted(e) for s, e in out.items()}


def test_database(db):
    lens = db.lengths.tolist()
    assert db.n == 136 <= 150 and lens == sorted(lens) and {1, 15, 16, 17} <= set(lens)
    assert {c % 16 for c in W.STRIPE_COLS} == set(range(16))                                  # every trim 1..16 of the single-column loop
    assert (db.lengths > 896).sum() >= 8 and 1790 <= max(lens) <= 1811 and (db.data3di >= 32).any()
    single = [x for x in W.TARGETS if len(set(x.codes.tolist())) == 1]
    assert {3, 15} <= {x.length for x in single} and all(3 <= x.length <= 40 for x in W.TARGETS[1:W.N_SHORT])
    for code in range(W.ROW_CODES):
        ids = W.targets_of(code)
        assert len(ids) >= 3
        for k in ids:                                                                           # one run of exactly the code's width, nowhere else
            x = W.TARGETS[k]
            assert (np.flatnonzero(x.codes == code) == np.arange(x.end - code, x.end + 1)).all()
    # both parities of a column inside an unrolled chunk, for condition (b)'s second half
    inner = [x.end % 16 for x in W.TARGETS[:W.N_SHORT] if x.end < 16 * (W.STRIPE_COLS[W.TARGETS.index(x) // 8] // 16)]
    assert {e % 2 for e in inner} == {0, 1}
    assert [W.STRIPE_COLS[k // 8] - 16 * (W.STRIPE_CHUNKS[k // 8] - 1) for k, _ in W.EDGE] == [1, 15, 16]
    for R in range(1, 57):
        assert len(W.STRIPE_CHUNKS) - 1 in _segments(R), R                                    # (e), first half: segments for every class


# ---- per instantiation --------------------------------------------------------------------------------------------------------------------------
def _best(probe, pairs, zero_rows=None):
    """gm.best_cells for (target id) pairs of one probe; zero_rows[k]: the row pair k's profile loses"""
    pssms = np.repeat(probe.pssm[None].astype(np.int32), len(pairs), axis=0)
    if zero_rows is not None:
        for k, row in enumerate(zero_rows):
            pssms[k, :, row] = 0
    return gm.best_cells(pssms, [W.TARGETS[t].codes for t in pairs])


def _covered(probes, packed):
    """rows in which an asserted pair of these probes has its one best cell, the score the model's, lost with the row: {row: [(probe, target)]}"""
    out = {}
    for p in probes:
        if not p.entries:
            continue
        p.model(packed)
        ids = [W.targets_of(code)[0] for _, code in p.entries]
        full = _best(p, ids)
        cut = _best(p, ids, [row for row, _ in p.entries])
        for (row, code), t, (score, cells, start), (less, _, _) in zip(p.entries, ids, full, cut):
            x = W.TARGETS[t]
            assert cells == [(row, x.end)] and score == W.WIDTH[code] * W.VALUE[code] == p.raw[t] < p.cap, (p.L, row, code, t)
            assert start == (row - code, x.end - code) and less < score
            out.setdefault(row, []).append((p, t))
    return out


def _check_edge(probes, layout_register, R, packed):
    """(b): the three stripe-end targets have their best cell in the stripe's last column, in a row of register R - 1"""
    seen = set()
    for p in probes:
        for (t, code), row in zip(W.EDGE, W.last_register_rows(R if layout_register != "paired" else R // 2)):
            if (row, code) in p.entries:
                (score, cells, _), = _best(p, [t])
                assert cells == [(row, W.STRIPE_COLS[t // 8] - 1)] and score == p.model(packed).raw[t]
                if layout_register == "halves":
                    assert row % R == R - 1
                else:
                    assert row % (2 * R) % R == R - 1
                seen.add(cells[0][1] % 16)
    assert seen == {0, 14, 15}


def _check_class(R, packed):
    full, short, sat = W.class_probes(R)
    got = _covered(full + [short], packed)
    # (a) per kernel of the class
    assert set(W.rows_untiled(R)) <= set(got) and len(W.rows_untiled(R)) == 6 * R
    _check_edge(full, "untiled", R, packed)
    if R <= W.PAIR_MAX_CLASS:
        need = W.rows_paired(R)                       # A in lanes 0, 1, 3; B the same rows in lanes 4, 5, 7: every member runs as both
        assert set(need) <= set(got) and {(h, r) for g, h, r in need.values()} == {(h, r) for h in (0, 1) for r in range(2 * R)}
        _check_edge(full, "paired", 2 * R, packed)
    if W.HALVES_MIN <= R <= W.HALVES_MAX:
        need = W.rows_halves(R)                       # A low, B high: every member runs as both
        assert set(need) <= set(got) and sorted(r for g, h, r in need.values()) == sorted(list(range(R)) * 3)
        _check_edge(full, "halves", R, packed)
    # (b), second half: best cells inside an unrolled chunk at even and at odd columns, in a row of the last register
    cols = set()
    for row in sorted(row for row in got if row % R == R - 1):
        p, first = got[row][0]
        inner = [t for t in W.targets_of(W.TARGETS[first].code) if W.TARGETS[t].end < 16 * (W.STRIPE_COLS[t // 8] // 16)]
        for t, (score, cells, _) in zip(inner, _best(p, inner) if inner else []):
            assert cells == [(row, W.TARGETS[t].end)] and score == p.raw[t]
            cols.add(cells[0][1] % 2)
        if cols == {0, 1}:
            break
    assert cols == {0, 1}, (R, cols)
    # (c)
    assert short.L == 16 * R - 15 and all(p.L == 16 * R for p in full) and short.cap != full[0].cap
    sat.model(packed)
    assert (sat.pssm == 127).all() and sat.cap == 255 and sat.raw.max() == 127 * 16 * R and sat.want.max() == 255
    assert sat.raw.max() > 2048 or R == 1                                                      # 16 rows reach 2032 at most
    # (e): the long targets' best run against a member that carries the long code
    ends = _segments(R)[len(W.STRIPE_CHUNKS) - 1]
    starts = [16 * e for e in ends[:-1]]
    p = next(p for p in full if p.long_row is not None)
    p.model(packed)
    hit = [t for t in range(W.N_SHORT, len(W.TARGETS)) if any(W.TARGETS[t].end - W.LONG_WIDTH + 1 < s <= W.TARGETS[t].end for s in starts)]
    assert hit, (R, starts)
    (score, cells, start), = _best(p, hit[:1])
    assert len(cells) == 1 and score == W.LONG_WIDTH * W.LONG_VALUE == p.raw[hit[0]] and any(start[1] < s <= cells[0][1] for s in starts)
    assert all(q.model(packed).raw[W.N_SHORT:].min() == score for q in full if q.long_row is not None)   # every long target's score is such a run


@pytest.fixture(scope="module")
def packed(db):
    return gm.pack(db)


@pytest.mark.parametrize("lo", range(1, 57, 8))
def test_conditions_untiled_paired_halves(lo, packed):
    for R in range(lo, lo + 8):
        _check_class(R, packed)


@pytest.mark.parametrize("R", TILED_R)
def test_conditions_tiled(R, shapes, packed):
    lengths = W.tiled_lengths(lambda L: shapes[L], TILED_R)[R]
    assert [n for L, n in lengths] == ([2] if R >= 29 else []) + [3] + ([4] if R >= 25 else [])
    rows = set()
    for L, n in lengths:
        assert shapes[L] == (n, R)
        probes = W.tiled_probes(R, L, n, full=(n == 3))
        got = _covered(probes, packed)
        rows |= {row % (16 * R) for row in got}
        if n == 3:
            _check_edge(probes, "untiled", R, packed)
        # (d) per border: entering columns 0 mod 16, odd, even
        p = probes[0]
        for t in range(1, n):
            base, kinds = t * 16 * R, set()
            for row, code in p.entries:
                if not base <= row < base + code:
                    continue
                ids = W.targets_of(code)
                for tid, (score, cells, start) in zip(ids, _best(p, ids)):
                    assert cells == [(row, W.TARGETS[tid].end)] and start[0] < base and score == p.raw[tid]
                    col = cells[0][1] - (row - base)
                    kinds.add("zero" if col % 16 == 0 else "odd" if col % 2 else "even")
            assert kinds == {"zero", "odd", "even"}, (R, L, t, kinds)
    assert set(W.rows_untiled(R)) <= rows                                                      # (a) over the tiles of the instantiation

"""fsgpu_gapless_pair_halves (host only, no GPU): which queries of one fsgpu_gapless_scan_multi call share the registers of the classes 17 .. 36
(k_gapless HALVES: query A in the low halves, query B in the high halves).  Held to the rule as include/fsgpu.h states it, over random class
histograms and the corner cases around the range's ends and the two-class reach of an odd member out."""
import numpy as np
import pytest

from foldseek_amd import api

LO, HI, REACH = 17, 36, 2


def _pair(classes):
    cls = np.asarray(classes, np.int32)
    lc, rec, half = (np.full(len(cls), -7, np.int32) for _ in range(3))
    n = api.lib().fsgpu_gapless_pair_halves(cls.ctypes.data, len(cls), lc.ctypes.data, rec.ctypes.data, half.ctypes.data)
    return int(n), lc, rec, half


def _fewest_dead(odd):
    """the fewest records without a B any choice of moves leaves.  odd: sorted (class, members) of the classes of the range with an odd member
    count; the odd member out of a class of three or more may take the free seat of a class c < c' <= c + REACH of this list, a seat is taken
    once, and who has given their seat away stays.  Plain recursion over the classes that can move, every choice tried."""
    movers = [c for c, m in odd if m >= 3]

    def go(k, used):
        if k == len(movers):
            return 0
        c = movers[k]
        if c in used:                                               # has a guest: no dead half, and does not move
            return go(k + 1, used)
        best = 1 + go(k + 1, used)
        for r, _ in odd:
            if c < r <= c + REACH and r not in used:
                best = min(best, go(k + 1, used | {r}))
        return best
    return go(0, frozenset())


def _check(classes):
    cls = [int(c) for c in classes]
    n, lc, rec, half = _pair(cls)
    members = {}
    for c in cls:
        members[c] = members.get(c, 0) + 1
    placed = [i for i in range(len(cls)) if rec[i] >= 0]
    # who is placed: the members of the classes of the range with two members or more and a single member that has a guest; everybody else
    # runs as before under their own class
    hosts = {int(lc[i]) for i in range(len(cls)) if lc[i] != cls[i]}
    for i, c in enumerate(cls):
        if LO <= c <= HI and (members[c] >= 2 or c in hosts):
            assert rec[i] >= 0 and half[i] in (0, 1), (cls, i)
        else:
            assert (lc[i], rec[i], half[i]) == (c, -1, -1), (cls, i)
    # every placed query exactly once: no two in one half of one record, every record has its A, records count up from 0
    seats = [(int(lc[i]), int(rec[i]), int(half[i])) for i in placed]
    assert len(set(seats)) == len(seats), cls
    records = sorted({(c, r) for c, r, _ in seats})
    assert n == len(records), cls
    for c, r in records:
        assert (c, r, 0) in seats, (cls, c, r)
    per_class = {}
    for c, r in records:
        per_class.setdefault(c, []).append(r)
    for c, rs in per_class.items():
        assert rs == list(range(len(rs))), (cls, c)
    # launches: one per class present, as before -- the unpaired kernel for a single member without a guest, else one launch over the class's
    # records (the loop above: no member of such a class is left to the unpaired kernel)
    for c, m in members.items():
        if LO <= c <= HI:
            assert (c in per_class) == (m >= 2 or c in hosts), (cls, c)
    assert set(per_class) <= set(members), cls
    # inside a class two by two in the call's order; only the odd member out of a class of three or more may leave, upward, REACH at most,
    # as the B of the record that class's own odd member out, or its single member, opens
    moved = []
    for c, m in members.items():
        if not (LO <= c <= HI and m >= 2):
            continue
        mine = [i for i in range(len(cls)) if cls[i] == c]
        for p, i in enumerate(mine[:m - m % 2]):
            assert (lc[i], rec[i], half[i]) == (c, p // 2, p % 2), (cls, i)
        if m % 2:
            i = mine[-1]
            if lc[i] == c:
                assert (rec[i], half[i]) == (m // 2, 0), (cls, i)
            else:
                up = int(lc[i])
                assert m >= 3 and c < up <= min(c + REACH, HI) and half[i] == 1, (cls, i)
                assert members.get(up, 0) % 2 == 1 and rec[i] == members[up] // 2, (cls, i)
                moved.append((c, up))
    for c in hosts:
        if members[c] == 1:
            assert (int(lc[cls.index(c)]), int(rec[cls.index(c)]), int(half[cls.index(c)])) == (c, 0, 0), (cls, c)
    assert len({up for _, up in moved}) == len(moved) and not ({c for c, _ in moved} & {up for _, up in moved}), cls
    # dead halves: only the last record of an odd class, and never two that could have met
    dead = [c for c, r in records if (c, r, 1) not in seats]
    assert len(set(dead)) == len(dead), cls
    for c in dead:
        assert members[c] % 2 == 1, (cls, c)
        assert members[c] >= 3 and c not in hosts, (cls, c)
        # no legal partner was left: neither another record without a B nor a single member on its own within reach above
        for up in range(c + 1, min(c + REACH, HI) + 1):
            assert up not in dead and not (members.get(up, 0) == 1 and up not in hosts), (cls, c, up)
    odd = sorted((c, m) for c, m in members.items() if LO <= c <= HI and m % 2 == 1)
    if len(odd) <= 14:
        assert len(dead) == _fewest_dead(odd), (cls, dead, moved)
    return n, lc, rec, half, moved


def test_corner_cases():
    assert _pair([])[0] == 0
    assert api.lib().fsgpu_gapless_pair_halves(None, 3, None, None, None) == -1
    assert _pair([20, 0])[0] == -1
    assert _check([22])[0] == 0                                          # one member: the unpaired kernel
    assert _check([22, 22])[0] == 1
    n, lc, rec, half, moved = _check([23, 23, 23])                       # three alone: the last record without a B
    assert n == 2 and moved == [] and (lc[2], rec[2], half[2]) == (23, 1, 0)
    n, lc, rec, half, moved = _check([20, 21, 20, 21, 20, 21])           # the benchmark's case: both counts odd
    assert n == 3 and moved == [(20, 21)] and (lc[4], rec[4], half[4]) == (21, 1, 1) and (lc[5], rec[5], half[5]) == (21, 1, 0)
    assert _check([20] * 3 + [21] * 2 + [22] * 3)[4] == [(20, 22)]       # the next class is full: one further
    assert _check([20] * 3 + [21] * 2 + [23] * 3)[4] == []               # three up is out of reach
    n, lc, rec, half, moved = _check([20, 21, 20, 20, 22])               # a single member takes a guest: its launch is one record
    assert n == 2 and moved == [(20, 21)] and (lc[1], rec[1], half[1]) == (21, 0, 0) and (lc[3], rec[3], half[3]) == (21, 0, 1) and rec[4] == -1
    assert _check([20] * 1 + [21] * 3)[4] == []                          # a single member does not move itself: its class keeps its launch
    assert _check([20] * 1 + [21] * 1)[0] == 0
    assert _check([20] * 3 + [21] * 1 + [22] * 3)[4] == [(20, 22)]       # two odd members out that meet save two dead halves, a guest of a single one
    assert sorted(_check([20] * 3 + [21] * 1 + [22] * 3 + [23] * 3)[4]) == [(20, 21), (22, 23)]
    assert len(_check([20] * 3 + [21] * 3 + [22] * 3)[4]) == 1           # a chain: one pair, one record without a B
    assert len(_check([20] * 3 + [21] * 3 + [22] * 3 + [23] * 5)[4]) == 2
    assert _check([36] * 3 + [37] * 3 + [38] * 3)[4] == []               # the range ends at 36
    assert _check([35] * 3 + [37] * 3)[4] == []
    assert _check([35] * 3 + [36] * 5)[4] == [(35, 36)]
    assert _check([16] * 3 + [17] * 3 + [15] * 3)[4] == []               # and begins at 17: the paired short classes are not placed here
    assert _check([16] * 3 + [17] * 3 + [18] * 7)[4] == [(17, 18)]
    assert _check([60, 3, 57, 1000])[0] == 0


@pytest.mark.parametrize("seed", range(6))
def test_random_histograms(seed):
    rng = np.random.default_rng(seed)
    for _ in range(150):
        lo, hi = (10, 42) if rng.random() < 0.5 else (17, 29)            # beyond the range on both sides / the benchmark's classes
        n = int(rng.integers(1, 70))
        dense = rng.integers(lo, hi + 1, size=n)
        few = rng.choice(rng.integers(lo, hi + 1, size=int(rng.integers(1, 7))), size=n)
        _check(dense if rng.random() < 0.5 else few)

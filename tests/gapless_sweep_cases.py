"""The probe world of the k_gapless sweep (tests/test_gapless_sweep_cases.py holds it to its conditions on the CPU, tests/test_gapless_sweep_gpu.py
runs it on the device).  Nothing here calls into foldseek_amd: the shape of a query (row tiles, registers) comes in as a function, expectations come
from tests/gapless_model.py.

Database (136 targets, sorted by length: ids are the load order, stripe s = ids 8s .. 8s + 7).  A probe target is filler (X, every fourth residue
written soft-masked with some other letter, which the scan reads as X too) around ONE run of one code: code c = 0..18 always as c + 1 residues
(WIDTH), code 19 -- the long targets' -- as 8.  Single-code targets of 1 and 3..15 residues; sixteen stripes whose longest target has every length
mod 16; from 16 residues on all eight targets of a stripe are equally long, every second one ends in its run (best cell in the stripe's last
column), the others hold it inside the first chunk.  The last stripe holds eight targets of 897 .. 1811 residues whose run straddles column 16 m,
m = LONG_BORDERS: with 114 chunks the planner cuts this stripe for every class R = 1..56 into segments of ceil(114 / ceil(114 / R)) chunks, and
every one of these segment lengths divides one m.

Profiles: -1 everywhere, and per entry (row i, code c) the rows i - c .. i of code c hold VALUE[c]: against a target of code c the one best cell is
(i, end of the run) with score WIDTH[c] * VALUE[c] <= 152.  A profile may carry the long code as well: 8 rows of 25 ending in `long_row`, 200 against
every long target -- the best cell of those, in a run that starts before a segment's first own column and ends behind it."""
import numpy as np

import gapless_model as gm

FILL = 20
ROW_CODES = 19
WIDTH = [c + 1 for c in range(ROW_CODES)]
VALUE = [100 // (c + 1) + 3 for c in range(ROW_CODES)]
LONG_CODE, LONG_WIDTH, LONG_VALUE = 19, 8, 25
CAP, OTHER_CAP, SHORT_CAP = 255, 230, 210  # above every total (152, 200): no probe score is cut
STRIPE_MAX = [9, 15, 16, 17, 18, 19, 20, 21, 22, 23, 26, 27, 28, 29, 30, 40]
LONG_LENGTHS = [897, 901, 999, 1040, 1203, 1357, 1500, 1811]
LONG_BORDERS = [38, 52, 58, 60, 68, 69, 72, 77]          # 38 | 38, 19; 58 | 29; 69 | 23; 68 | 17; 60 | 15, 12, 10, 6, 5, 4, 3, 2; 52 | 13; 72 | 9, 8; 77 | 11, 7
PAIR_MAX_CLASS, HALVES_MIN, HALVES_MAX, UNTILED_MAX = 16, 17, 36, 56


class Target:
    def __init__(self, length, code, end):
        self.length, self.code, self.end = length, code, end
        self.width = LONG_WIDTH if code == LONG_CODE else WIDTH[code]
        assert 0 <= end - self.width + 1 and end < length
        j = np.arange(length)
        self.codes = np.where(j % 4 == 1, 32 + j * 7 % 21, FILL).astype(np.uint8)
        self.codes[end - self.width + 1:end + 1] = code


def _targets():
    t = [Target(n, n - 1, n - 1) for n in (1, 3, 4, 5, 6, 7, 8, 9)]                  # stripe 0: single-code
    t += [Target(n, n - 1, n - 1) for n in range(10, 16)] + [Target(15, 1, 14), Target(15, 0, 14)]
    for k, T in enumerate(STRIPE_MAX[2:]):
        for j in range(8):
            n = 8 * k + j
            c = n % ROW_CODES if n % ROW_CODES < T else n % 16
            t.append(Target(T, c, T - 1 if j % 2 == 0 else max(c, 5 * n % 16)))
    t += [Target(n, LONG_CODE, 16 * m + 3) for n, m in zip(LONG_LENGTHS, LONG_BORDERS)]
    assert [x.length for x in t] == sorted(x.length for x in t) and len(t) % 8 == 0
    return t


TARGETS = _targets()
N_SHORT = len(TARGETS) - len(LONG_LENGTHS)
STRIPE_COLS = [max(x.length for x in TARGETS[s:s + 8]) for s in range(0, len(TARGETS), 8)]
STRIPE_CHUNKS = [(c + 15) // 16 for c in STRIPE_COLS]


class DB:
    """what gapless_model and api.Context.load_db read of a synth.PaddedDB"""

    def __init__(self, targets):
        self.lengths = np.array([x.length for x in targets], np.int32)
        self.offsets = np.zeros(len(targets) + 1, np.int64)
        self.offsets[1:] = np.cumsum((self.lengths.astype(np.int64) + 3) // 4 * 4)
        self.data3di = np.full(int(self.offsets[-1]), FILL, np.uint8)
        for k, x in enumerate(targets):
            self.data3di[self.offsets[k]:self.offsets[k] + x.length] = x.codes
        self.n, self.dataaa = len(targets), None


def targets_of(code):
    return [k for k, x in enumerate(TARGETS) if x.code == code]


def stripe_end_target(trim, taken=()):
    """(id, code) of the narrowest-run target (of a code not taken) that ends in its run and is the longest of a stripe whose last chunk holds `trim`
    columns"""
    best = None
    for k, x in enumerate(TARGETS[:N_SHORT]):
        if x.code not in taken and x.length == STRIPE_COLS[k // 8] and x.end == x.length - 1 and (x.length - 1) % 16 + 1 == trim:
            if best is None or x.width < TARGETS[best].width:
                best = k
    return best, TARGETS[best].code


# the last-register probes: the stripe's last chunk holds 1 column (index 0 in its chunk), 15 (index 14) and 16 (index 15, the unrolled loop)
EDGE = []
for _trim in (1, 15, 16):
    EDGE.append(stripe_end_target(_trim, [c for _, c in EDGE]))


# ---- rows of the kernels' layouts ---------------------------------------------------------------------------------------------------------------
def rows_untiled(R, lanes=(0, 3, 7)):
    """untiled and row tiles: row g 2R + r in the low half of register r of lane g, + R in the high half; {row: (lane, half, register)}"""
    return {g * 2 * R + h * R + r: (g, h, r) for g in lanes for h in (0, 1) for r in range(R)}


def rows_paired(c, lanes=(0, 1, 3)):
    """PAIRED of class c: 2c registers, query A in lanes 0..3, query B the same rows in lanes 4..7"""
    return rows_untiled(2 * c, lanes)


def rows_halves(R, lanes=(0, 7, 15)):
    """HALVES: row g R + r in register r of lane g, A low, B high"""
    return {g * R + r: (g, 0, r) for g in lanes for r in range(R)}


def last_register_rows(R):
    """rows 16R - 1, 14R - 1, 12R - 1: in the last register of k_gapless<R> (lanes 7, 6, 5, high half), of HALVES<R> (lanes 15, 13, 11) and of
    PAIRED<2R> (lanes 3, 2 high, 2 low)"""
    return [16 * R - 1, 14 * R - 1, 12 * R - 1]


# ---- profiles -----------------------------------------------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, L, entries, cap=CAP, long_row=None, pssm=None):
        self.L, self.cap, self.entries, self.long_row = L, cap, sorted(entries), long_row
        if pssm is None:
            pssm = np.full((21, L), -1, np.int8)
            for row, code in entries:
                assert code <= row < L
                pssm[code, row - code:row + 1] = VALUE[code]
            if long_row is not None:
                assert LONG_WIDTH - 1 <= long_row < L
                pssm[LONG_CODE, long_row - LONG_WIDTH + 1:long_row + 1] = LONG_VALUE
        self.pssm = np.ascontiguousarray(pssm, np.int8)
        self.raw = self.want = None

    def model(self, packed):
        if self.raw is None:
            self.raw = gm.best_runs(self.pssm, packed)
            self.want = np.minimum(self.raw, gm.clamp(self.cap)).astype(np.int32)
        return self


def plan(rows, demands=()):
    """entry lists that between them put a code on every row: demands[k] = the (row, code) entries profile k starts from; then row by row the
    widest code that is free in the profile and whose window fits above the row"""
    left = sorted(set(rows) - {r for d in demands for r, _ in d})
    out, k = [], 0
    while left or k < len(demands):
        entries = list(demands[k]) if k < len(demands) else []
        free = sorted(set(range(ROW_CODES)) - {c for _, c in entries})
        later = []
        for row in left:
            fit = [c for c in free if c <= row]
            if fit:
                entries.append((row, fit[-1]))
                free.remove(fit[-1])
            else:
                later.append(row)
        left = later
        out.append(entries)
        k += 1
    return out


def _long_row(L, k):
    return LONG_WIDTH - 1 + (53 * k + L - LONG_WIDTH) % (L - LONG_WIDTH + 1) if L >= LONG_WIDTH else None


def class_rows(R):
    """the rows condition (a) names for the kernels a query of class R can run in"""
    rows = set(rows_untiled(R))
    if R <= PAIR_MAX_CLASS:
        rows |= set(rows_paired(R))
    if HALVES_MIN <= R <= HALVES_MAX:
        rows |= set(rows_halves(R))
    return rows


def class_probes(R):
    """the probe members of class R = 1..56: (full-length profiles, the member of 16R - 15 residues, the saturating member)"""
    L = 16 * R
    edge = [(row, code) for row, (_, code) in zip(last_register_rows(R), EDGE)]
    full = [Probe(L, e, OTHER_CAP if k % 2 else CAP, _long_row(L, k)) for k, e in enumerate(plan(class_rows(R), [edge]))]
    Ls = L - 15
    # the short member: the rows it has among those of the second profile (the first where that is the only one)
    src = full[min(1, len(full) - 1)]
    short = Probe(Ls, [(row, code) for row, code in src.entries if row < Ls], SHORT_CAP, _long_row(Ls, R))
    return full, short, Probe(L, [], CAP, None, np.full((21, L), 127, np.int8))


def tiled_lengths(shape, r_values):
    """per tiled register count the first length that runs as 2 (where there is one), 3 and 4 or more row tiles: {R: [(L, nTiles)]}"""
    found = {R: {} for R in r_values}
    for L in range(16 * UNTILED_MAX + 1, 2200):
        n, R = shape(L)
        if n > 1:
            found[R].setdefault(min(n, 4), (L, n))
    return {R: [found[R][n] for n in sorted(found[R])] for R in r_values}


def border_demands(R, n_tiles, used=()):
    """condition (d): per tile border three entries whose run crosses it and enters the new tile at a column = 0 mod 16, an odd one, an even one"""
    used, out = set(used), []
    for t in range(1, n_tiles):
        base = t * 16 * R
        for want in (lambda col: col % 16 == 0, lambda col: col % 2 == 1, lambda col: col % 2 == 0 and col % 16 != 0):
            hit = None
            for code in range(ROW_CODES - 1, 0, -1):
                if code in used:
                    continue
                for d in range(0, code):                    # d rows into the new tile: at least one row of the window lies above the border
                    if any(want(TARGETS[k].end - d) for k in targets_of(code)):
                        hit = (base + d, code)
                        break
                if hit:
                    break
            assert hit, (R, n_tiles, t)
            used.add(hit[1])
            out.append(hit)
    return out


def tiled_probes(R, L, n_tiles, full):
    """full: the rows of condition (a), dealt over the tiles, behind the border and last-register entries; else one profile of the border entries
    and as many more rows as it has codes for"""
    tile = 16 * R
    rows = []
    for k, u in enumerate(sorted(rows_untiled(R))):
        t = k % n_tiles
        rows.append(t * tile + u if t * tile + u < L else u)
    borders = border_demands(R, n_tiles)
    edge = [(row, code) for row, (_, code) in zip(last_register_rows(R), EDGE)]
    entries = plan(rows, [borders, edge])
    if not full:
        entries = entries[:1]
    return [Probe(L, e, CAP if k % 2 == 0 else SHORT_CAP, _long_row(L, k)) for k, e in enumerate(entries)]

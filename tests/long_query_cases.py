"""tests/long_query_cases.py -- the seeded inputs of the long-query tests (TEST INFRASTRUCTURE: of the project only synth.PaddedDB, a plain container, and
the host-side profile builders of foldseek_amd.api are used; nothing is read outside tests/golden).

include/fsgpu.h takes a query of 1 .. FSGPU_MAX_SEQ_LEN = 65535 residues on every entry.  Per query length of LQ one seeded query (3Di and AA) and one
small resident database are built here, for the CPU test of the models (tests/test_long_query_model.py) and the GPU tests (tests/test_long_query_gpu.py):

* planted scan targets: query[p - w : p + w] for every row p that is a border between two row tiles of the gapless scan at that length, and for the
  rows 0, 32768 (where the query has it) and L - 1.  w is chosen so that the window scores below the query's cap and above each half alone: a diagonal
  that the scan cut at the border would score what one half scores.
* planted Smith-Waterman targets: windows of 40 .. 200 query residues with 3 residues taken out of the middle, lying across a multiple of 512 query
  rows (the row tile of k_sw): the first, the 63rd / 64th and the last multiple, 8 seeded others, one window from row 0, one up to row L - 1; the same
  windows of the REVERSED query; a window of SAT_LEN residues up to row L - 1 whose self-match passes 32767 (the int32 re-run), and for L >= 32769 one
  across row 32768 (at L = 32769 that is the same window).
* plain targets: 60 unrelated ones of 1 .. 300 residues, some with soft-masked stretches, one all X.

The models run live; what they return is kept per process, so that tests of one file share it."""
import collections
import functools

import numpy as np

import gapless_model as gm
import sw_cases as K
import sw_model as sm
from foldseek_amd import api, synth

LQ = (8193, 32767, 32768, 32769, 65534, 65535)
SW_TILE = 512                       # query rows of one row tile of k_sw (64 lanes x 8 rows)
SCAN_UNTILED = 896                  # the scan runs queries up to here in one piece
SCAN_TILE = 512                     # ... and longer ones in row tiles of at most this many rows
SAT_LEN = 3200                      # a self-match of 3000 residues averages 32 800 at these matrices, too close to 32767 to pass it for every seed

Entry = collections.namedtuple("Entry", "t3 ta kind info")           # t3 as stored (soft-masked letters + 32), info: what the kind needs


def scan_tiles(L):
    """(number of row tiles, rows per tile) of the gapless scan, from the rule stated at fsgpu_gapless_launch: one piece up to 896 rows; beyond that
    ceil(L / 512) tiles of EQUAL height, the height rounded up to whole 16-row strips: L = 1025 runs as 3 x 352 rows, not as 512 + 512 + 1"""
    if L <= SCAN_UNTILED:
        return 1, L
    n = -(-L // SCAN_TILE)
    return n, 16 * -(-(-(-L // n)) // 16)


def scan_borders(L):
    n, rows = scan_tiles(L)
    return [t * rows for t in range(1, n) if t * rows < L]


@functools.lru_cache(maxsize=None)
def query(L):
    """(3Di codes, AA codes): seeded, uniform over the 20 letters, an X every 1000 residues or so"""
    rng = np.random.default_rng(20261019 + L)
    q3, qa = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
    q3[rng.integers(0, L, max(1, L // 1000))] = 20
    qa[rng.integers(0, L, max(1, L // 1000))] = 20
    return q3, qa


@functools.lru_cache(maxsize=None)
def scan_profile(L):
    """(pssm int8 [21, L], cap) of the prefilter: 3Di at bit factor 2.0, composition bias on"""
    return api.prefilter_profile(api.Matrix(0, 2.0), query(L)[0], True, 0.15)


def tiny(m):
    return np.ascontiguousarray(np.array(m.scores()).reshape(21, 21).astype(np.int8))


@functools.lru_cache(maxsize=None)
def host_matrices(atype):
    """(AA, 3Di) api.Matrix of structurealign for an alignment type: BLOSUM62 at 1.4 (type 2) or 0.0 (type 0), 3Di at 2.1"""
    return api.Matrix(1, 1.4 if atype == 2 else 0.0), api.Matrix(0, 2.1)


@functools.lru_cache(maxsize=None)
def sw_query(L, atype=2):
    """sw_cases.Query with the composition biases of both directions (the reversed query's are those of the reversed sequence, indexed by the
    reversed position)"""
    q3, qa = query(L)
    mA, m3 = host_matrices(atype)
    _, _, cbAf, cb3f = api.align_profiles(mA, m3, qa, q3, True, 0.5)
    _, _, cbAr, cb3r = api.align_profiles(mA, m3, qa[::-1].copy(), q3[::-1].copy(), True, 0.5)
    return K.Query(q3, qa, cb3f, cbAf, cb3r, cbAr)


@functools.lru_cache(maxsize=None)
def sw_matrices(atype):
    mA, m3 = host_matrices(atype)
    return tiny(m3), tiny(mA)


def sw_profiles(L, atype):
    """(pAA fwd, p3Di fwd, pAA rev, p3Di rev) int16 [21, L], stated by sw_model.profile"""
    q = sw_query(L, atype)
    m3, mA = sw_matrices(atype)
    return [np.ascontiguousarray(sm.profile(m, s, b, rev).astype(np.int16))
            for m, s, b, rev in ((mA, q.qa, q.cbAf, False), (m3, q.q3, q.cb3f, False), (mA, q.qa, q.cbAr, True), (m3, q.q3, q.cb3r, True))]


# ---- the planted targets ---------------------------------------------------------------------------------------------------------------------------------
def _diag_sum(pssm, codes, lo):
    """best run of the target `codes` on the diagonal that puts its first residue on query row lo"""
    best = s = 0
    for k, c in enumerate(codes):
        s = max(0, s + int(pssm[int(c), lo + k]))
        best = max(best, s)
    return best


def _scan_window(L, p):
    """query[p - w : p + w] (moved inside the query at its ends) with the w, 12 first, at which the window's own diagonal stays below the cap and
    above both halves; the CPU test asserts the same of the model's score over all diagonals"""
    pssm, cap = scan_profile(L)
    q3 = query(L)[0]
    for w in (12, 10, 14, 8, 16, 6, 18, 20):
        lo = min(max(0, p - w), L - 2 * w)
        t = q3[lo:lo + 2 * w]
        whole, a, b = _diag_sum(pssm, t, lo), _diag_sum(pssm, t[:w], lo), _diag_sum(pssm, t[w:], lo + w)
        if whole < gm.clamp(cap) - 8 and whole > max(a, b) + 8 and whole > 40:
            return lo, w
    raise AssertionError(("no window width serves row", L, p))


def _cut3(seq):
    h = len(seq) // 2
    return np.concatenate([seq[:h], seq[h + 3:]])


def _sw_windows(L):
    """[(first row, length, the multiple of 512 it lies across or None)] in the rows of one direction"""
    rng = np.random.default_rng(77 + L)
    mult = list(range(SW_TILE, L, SW_TILE))
    must = {mult[0], mult[-1]} | {m for m in (63 * SW_TILE, 64 * SW_TILE) if m in mult}
    rest = [m for m in mult if m not in must]
    chosen = sorted(must | set(int(x) for x in rng.choice(rest, size=min(8, len(rest)), replace=False)))
    out = []
    for m in chosen:
        n = int(rng.integers(40, 201))
        before = int(rng.integers(n // 2 + 8, n - 8))       # the border lies behind the 3 residues taken out: first row and end row on two sides of it
        s = max(0, m - before)
        out.append((s, min(n, L - s), m))
    out.append((0, int(rng.integers(40, 201)), None))
    n = int(rng.integers(40, 201))
    out.append((L - n, n, None))
    return out


@functools.lru_cache(maxsize=None)
def entries(L):
    q3, qa = query(L)
    rng = np.random.default_rng(4000 + L)
    out = []
    for p in sorted(set(scan_borders(L)) | {0, L - 1} | ({32768} if L > 32768 else {32767} if L == 32768 else set())):
        lo, w = _scan_window(L, p)
        out.append(Entry(q3[lo:lo + 2 * w].copy(), qa[lo:lo + 2 * w].copy(), "scan", dict(p=p, lo=lo, w=w)))
    for rev in (False, True):
        s3, sa = (q3[::-1], qa[::-1]) if rev else (q3, qa)
        for s, n, m in _sw_windows(L):
            out.append(Entry(_cut3(s3[s:s + n]), _cut3(sa[s:s + n]), "sw_rev" if rev else "sw_fwd", dict(s=s, n=n, m=m, end=s + n - 1)))
    # up to row L - 1, and across row 32768 (at L = 32769 the first one is both)
    sat = sorted({L - SAT_LEN} | ({min(32768 - SAT_LEN // 2, L - SAT_LEN)} if L >= 32769 else set()))
    for s in sat:
        out.append(Entry(q3[s:s + SAT_LEN].copy(), qa[s:s + SAT_LEN].copy(), "sat", dict(s=s, end=s + SAT_LEN - 1)))
    for k in range(60):
        n = 1 if k == 0 else 300 if k == 1 else int(rng.integers(2, 300))
        t3, ta = rng.integers(0, 20, n).astype(np.uint8), rng.integers(0, 20, n).astype(np.uint8)
        if k == 2:
            t3[:] = 20; ta[:] = 20
        elif k % 6 == 3 and n > 8:
            a = int(rng.integers(0, n - 4)); b = int(rng.integers(a + 1, n + 1))
            t3[a:b] += 32                                    # a soft-masked stretch: X to the scan, the letter itself to the aligner
        out.append(Entry(t3, ta, "allX" if k == 2 else "plain", {}))
    return out


class World:
    """the database of one query length (ascending length, every target padded to a multiple of 4 with X), .kind / .info per target"""

    def __init__(self, L):
        es = sorted(entries(L), key=lambda e: len(e.t3))
        lens = np.array([len(e.t3) for e in es], np.int32)
        off = np.zeros(len(lens) + 1, np.int64)
        off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
        d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
        for k, e in enumerate(es):
            d3[off[k]:off[k] + lens[k]] = e.t3
            da[off[k]:off[k] + lens[k]] = e.ta
        self.L, self.db = L, synth.PaddedDB(d3, da, off, lens)
        self.kind, self.info = [e.kind for e in es], [e.info for e in es]
        self._scan, self._sw = None, {}

    def ids(self, *kinds):
        return [i for i, k in enumerate(self.kind) if k in kinds]

    def plain_sample(self):
        return self.ids("plain", "allX")[::5]

    def sw_ids(self):
        """the targets of the SW tests: every planted SW target, every 5th plain one, every 8th scan target"""
        return np.array(sorted(self.ids("sw_fwd", "sw_rev", "sat") + self.plain_sample() + self.ids("scan")[::8]), np.uint32)

    def scan_want(self):
        if self._scan is None:
            self._scan = gm.scores(*scan_profile(self.L), self.db)
        return self._scan

    def sw_want(self, atype, rev, ids, go=10, ge=1, L=None):
        """sw_model's records of the query of length L (this world's own by default), one direction, for targets `ids` of this database; each pair
        is computed once per process"""
        L = self.L if L is None else L
        q = sw_query(L, atype)
        m3, mA = sw_matrices(atype)
        have = self._sw.setdefault((L, atype, bool(rev), go, ge), {})
        todo = sorted({int(i) for i in ids} - set(have), key=lambda i: int(self.db.lengths[i]))
        cb3, cbA = (q.cb3r, q.cbAr) if rev else (q.cb3f, q.cbAf)
        for a in range(0, len(todo), 8):                     # targets of similar length together: one_pass pads to the longest
            part = todo[a:a + 8]
            ts = [K.target(self.db, i) for i in part]
            got = sm.align(m3, mA, q.q3, q.qa, cb3, cbA, bool(rev), [t[0] for t in ts], [t[1] for t in ts], go, ge)
            for i, g in zip(part, got):
                have[i] = g.copy()
        out = np.zeros(len(ids), sm.REC_DT)
        for k, i in enumerate(ids):
            out[k] = have[int(i)]
        return out


@functools.lru_cache(maxsize=None)
def world(L):
    return World(L)


def first_aligned_row(L, atype, rev, target3, targetA, rec, margin=64):
    """the first query row of an optimal alignment that ends in the model's end cell: the same model over the reversed rows [end - span, qEnd] and
    the reversed target columns [0, dbEnd] finds that alignment from its end; returns (row, score found there)"""
    q = sw_query(L, atype)
    m3, mA = sw_matrices(atype)
    cb3, cbA = (q.cb3r, q.cbAr) if rev else (q.cb3f, q.cbAf)
    qe, de = int(rec["qEnd"]), int(rec["dbEnd"])
    lo = max(0, qe - len(target3) - margin)
    p3 = sm.profile(m3, q.q3, cb3, rev)[:, lo:qe + 1][:, ::-1]
    pA = sm.profile(mA, q.qa, cbA, rev)[:, lo:qe + 1][:, ::-1]
    got = sm.align_profiles(np.ascontiguousarray(p3), np.ascontiguousarray(pA), [target3[:de + 1][::-1].copy()], [targetA[:de + 1][::-1].copy()])[0]
    return qe - int(got["qEnd"]), int(got["score"])

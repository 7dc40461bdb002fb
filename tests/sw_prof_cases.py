"""The world of the profile-path sweep: every instantiation of k_sw<R, HAS_AA, Pk16 | I32> and k_sw2<R, HAS_AA>, R in {1, 2, 3, 4, 6, 8}
(tests/test_sw_prof_cases.py holds the world to its conditions on the CPU, tests/test_sw_prof_gpu.py runs it on the device).  Nothing here calls
into foldseek_amd.  A query IS its four ready-made int16 tables [21, L] (AA forward, 3Di forward, AA reversed, 3Di reversed; the AA pair None: 3Di
only), so ordinary tables (matrix entry + bias) and tables no matrix could give share one route; the answers are sw_model.align_profiles of those
tables, frozen in tests/golden/sw_prof_v1/answers.npz by tests/golden/make_sw_prof_golden.py.

Query lengths are the bottom and the top of every register class: 1, 64 | 65, 128 | 129, 192 | 193, 256 | 257, 384 | 385, 512; every query exists
with AA tables and 3Di only.  Sections:

(a) ordinary tables.  `rand`: residues 0..15 drawn at random, rows 0, 1, L - 2, L - 1 hold the letters 16..19, which the query holds only there;
    per class the member of 64 R rows has planted targets: for every register rr and each of the lanes 0, 31, 63 the copy of the query's rows
    r - 24 .. r, r = lane * R + rr, of the forward and of the reversed query.  `hom` (one letter) and `blk` (ten rows of one letter, then another)
    are the low-complexity members whose records the two tie rules decide.  Gap costs 10 / 1; class 3 again at 8 / 2 and class 6 at 3 / 1.
(b) the int32 re-run.  Why class 1 needs ready-made tables: a cell of int8 material holds at most 127 + 127 per table, 508 with both, and
    64 * 508 = 32512 < 32767; from 65 rows on 65 * 508 = 33020 passes.  `dom0` / `dom1`: -5 everywhere, and per probed row r one letter that holds
    17000 in the rows r - 1 and r (row 0: 32767 in row 0 alone): the target (X, X, X, letter, letter) saturates and its int32 record ends in r.
    `hotF` / `hotR` / `hotB`: the `rand` tables plus a bonus on the forward, the reversed, both directions' tables -- 100, which a bias can hold,
    wherever the longest target then saturates, else 600.  `homhot`: one letter at 600 a cell, so that the int32 end cell is chosen among tied rows.
    `exact`: 63 cells that sum to 32767 with no addition clipped.  `hotbot`: the class's shortest member, bonus 600.  `long`: 513 and 1025 rows (two and three row tiles), bonus 600.
(c) the int16 range.  Letters of one target stand for the conditions: 0 the AA + 3Di sum 20000 + 20000 (i), 6 the sum 32767 + 32767 (i), 1 the
    sum -20000 - 20000 in every row (ii), 7 the sum -32768 - 32768 in every row (ii), 4 two cells of 10000 + 10000 on one diagonal (iii),
    8 the legal sum 32767 - 32000, 3 a plain 60 + 40 in every row; 3Di only the tables hold the sums' halves, which only (iii) / (iv) can touch.
    The targets of this section hold the same letter in both tracks, so the column score is a function of one letter and `wrapped` below can state
    what a wrapping int16 sum would give."""
import collections
import functools
import hashlib
import os

import numpy as np

import sw_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sw_prof_v1")
ANSWERS = os.path.join(GOLD, "answers.npz")

CLASSES = (1, 2, 3, 4, 6, 8)
BOTTOM = {1: 1, 2: 65, 3: 129, 4: 193, 6: 257, 8: 385}
LANES = (0, 31, 63)
LONG = (513, 1025)
X = 20
GAP_VARIANTS = {3: (8, 2), 6: (3, 1)}

# one query of the world: tables (pAf / pAr None: 3Di only), gap costs, ids of its targets in the database
Q = collections.namedtuple("Q", "name sec kind cls aa L pAf p3f pAr p3r go ge ids")


def class_of(L):
    return next((R for R in CLASSES if 64 * R >= L), 8)


@functools.lru_cache(maxsize=None)
def matrices():
    """(3Di at bit factor 2.1, BLOSUM62 at 1.4) as int32 [21, 21], read from the frozen reference fixture"""
    g = np.load(os.path.join(HERE, "golden", "hotpath_v1.npz"))
    return g["sub_mat3di_2.1"].reshape(21, 21).astype(np.int32), g["sub_blosum62_1.4"].reshape(21, 21).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _master():
    rng = np.random.default_rng(20261021)
    return rng.integers(0, 16, 1025).astype(np.uint8), rng.integers(0, 16, 1025).astype(np.uint8)


def rand_codes(L):
    """(3Di, AA) codes of the `rand` member of L rows"""
    out = []
    for m in _master():
        q = m[:L].copy()
        for row, letter in ((0, 16), (1, 17), (L - 2, 18), (L - 1, 19)):
            if 0 <= row < L:
                q[row] = letter
        out.append(q)
    return out


def ordinary(codes3, codesA, seed, bias=3):
    """matrix entry + bias: the four tables [21, L] int16 of sw_model.profile, the letters 16..19 with the largest bias"""
    rng = np.random.default_rng(seed)
    m3, mA = matrices()
    out = []
    for mat, codes, rev in ((mA, codesA, False), (m3, codes3, False), (mA, codesA, True), (m3, codes3, True)):
        c = codes[::-1] if rev else codes
        cb = rng.integers(-bias, bias + 1, len(c)).astype(np.int32) if bias else np.zeros(len(c), np.int32)
        cb[c >= 16] = bias
        out.append((mat[:, c.astype(np.int64)] + cb[None, :]).astype(np.int16))
    return out


# ---- the database -----------------------------------------------------------------------------------------------------------------------------------
class DB:
    """what api.Context.load_db reads of a synth.PaddedDB; .t3 / .tA: the codes as the aligner reads them (soft-masking removed)"""

    def __init__(self, entries):
        order = sorted(range(len(entries)), key=lambda k: len(entries[k][1]))
        self.tag = {entries[k][0]: i for i, k in enumerate(order)}
        assert len(self.tag) == len(entries)
        entries = [entries[k] for k in order]
        self.lengths = np.array([len(e[1]) for e in entries], np.int32)
        self.offsets = np.zeros(len(entries) + 1, np.int64)
        self.offsets[1:] = np.cumsum((self.lengths.astype(np.int64) + 3) // 4 * 4)
        self.data3di, self.dataaa = np.full(int(self.offsets[-1]), X, np.uint8), np.full(int(self.offsets[-1]), X, np.uint8)
        self.t3, self.tA = [], []
        for k, (_, t3, tA) in enumerate(entries):
            o, n = int(self.offsets[k]), len(t3)
            self.data3di[o:o + n], self.dataaa[o:o + n] = t3, tA
            self.t3.append((np.asarray(t3) % 32).astype(np.uint8)); self.tA.append((np.asarray(tA) % 32).astype(np.uint8))
        self.n = len(entries)

    def ids(self, *tags):
        return np.array([self.tag[t] for t in tags], np.uint32)


def planted_rows(R):
    return [lane * R + rr for lane in LANES for rr in range(R)]


def _window(q, r):
    return q[max(0, r - 24):r + 1]


C_TARGETS = {"c/i": [X, 0, X], "c/i max": [6], "c/ii": [3, 3, 3, 1, 3, 3, 3], "c/ii min": [3, 3, 3, 7, 3, 3, 3], "c/ii alone": [1, 1], "c/iii": [X, 4, 4],
             "c/legal": [8], "c/plain": [3] * 5, "c/all": [3, 3, 0, 3, 4, 4, 3, 7, 3, 6, 8, 1, 3]}


@functools.lru_cache(maxsize=None)
def db():
    rng = np.random.default_rng(1021)
    e = []
    for n in (1, 2, 63, 64, 65, 130, 400):
        e.append((f"random/{n}", rng.integers(0, 20, n).astype(np.uint8), rng.integers(0, 20, n).astype(np.uint8)))
    m3, mA = _master()
    rel3, relA = m3[3:133].copy(), mA[3:133].copy()                 # a relative of every `rand` query: one residue in ten redrawn
    sub = rng.random(130) < 0.1
    rel3[sub] = rng.integers(0, 16, int(sub.sum())); relA[sub] = rng.integers(0, 16, int(sub.sum()))
    e.append(("relative/130", rel3, relA))
    e.append(("relative/400", np.concatenate([m3[:140], m3[150:410]]), np.concatenate([mA[:140], mA[150:410]])))
    e.append(("allX", np.full(40, X, np.uint8), np.full(40, X, np.uint8)))
    e.append(("masked", rng.integers(0, 20, 50).astype(np.uint8) + 32, rng.integers(0, 20, 50).astype(np.uint8)))
    for n in (1, 2, 5, 63, 130):
        e.append((f"hom/{n}", np.full(n, 5, np.uint8), np.full(n, 9, np.uint8)))
    for R in CLASSES:
        q3, qA = rand_codes(64 * R)
        for r in planted_rows(R):
            e.append((f"plant/{R}/fwd/{r}", _window(q3, r), _window(qA, r)))
            e.append((f"plant/{R}/rev/{r}", _window(q3[::-1], r), _window(qA[::-1], r)))
        L = BOTTOM[R]
        q3, qA = rand_codes(L)
        e.append((f"plant/{R}/bottom/fwd", _window(q3, L - 1), _window(qA, L - 1)))
        e.append((f"plant/{R}/bottom/rev", _window(q3[::-1], L - 1), _window(qA[::-1], L - 1)))
    for c in range(20):
        e.append((f"dom/{c}", np.array([X, X, X, c, c], np.uint8), np.array([X, X, X, c, c], np.uint8)))
    for tag, t in C_TARGETS.items():
        e.append((tag, np.array(t, np.uint8), np.array(t, np.uint8)))
    return DB(e)


GENERIC = ("random/1", "random/2", "random/63", "random/64", "random/65", "random/130", "relative/130", "allX", "masked", "hom/5")
HOMS = ("hom/1", "hom/2", "hom/5", "hom/63", "hom/130")


# ---- queries ----------------------------------------------------------------------------------------------------------------------------------------
def _q(name, sec, kind, aa, tables, ids, go=10, ge=1):
    pAf, p3f, pAr, p3r = [np.ascontiguousarray(t, np.int16) for t in tables]
    L = p3f.shape[1]
    assert p3f.shape == p3r.shape == pAf.shape == pAr.shape == (21, L)
    return Q(name, sec, kind, class_of(L), aa, L, pAf if aa else None, p3f, pAr if aa else None, p3r, go, ge, ids)


def _low(L, kind):
    c3, cA = np.full(L, 5, np.uint8), np.full(L, 9, np.uint8)
    if kind == "blk":
        c3[10:], cA[10:] = 11, 2
    return c3, cA


def dom_rows(R):
    """rows probed by dom0 (lanes 0 and 31) and dom1 (lane 63) of the class's member of 64 R rows"""
    return [lane * R + rr for lane in LANES[:2] for rr in range(R)], [LANES[2] * R + rr for rr in range(R)]


def dom_tables(L, rows, aa, shift):
    """-5 everywhere; letter (k + shift) % 20 holds 17000 in the rows r - 1 and r of the k-th probed row r (row 0: 32767 in row 0); with AA tables
    the value is split between the two.  Returns (tables of one direction as (pA, p3), {letter: row})"""
    pA, p3 = np.full((21, L), -5 if aa else 0, np.int32), np.full((21, L), -5, np.int32)
    where = {}
    for k, r in enumerate(rows):
        c = (k + shift) % 20
        assert c not in where
        where[c] = r
        v, lo = (32767, r) if r == 0 else (17000, r - 1)
        if aa:
            p3[c, lo:r + 1], pA[c, lo:r + 1] = v // 2, v - v // 2
        else:
            p3[c, lo:r + 1] = v
    return (pA, p3), where


def hot_bonus(L, aa):
    """100 where the `rand` tables + 100 saturate against the 400-column targets (every cell then about 100 per table), else 600"""
    return 100 if min(L, 400) * (200 if aa else 100) * 0.9 > 32767 else 600


def exact_tables(L, aa):
    """the rows 0..62 of the hom targets' letters (3Di 5, AA 9) sum to 32767 along the diagonal, -1000 a cell elsewhere"""
    n = 63
    v = np.full(n, 32767 // n, np.int32); v[:32767 - int(v.sum())] += 1
    assert v.sum() == 32767
    pA, p3 = np.full((21, L), -500 if aa else 0, np.int32), np.full((21, L), -500 if aa else -1000, np.int32)
    p3[5, :n] = v - (1 if aa else 0)
    pA[9, :n] = 1 if aa else 0
    return pA, p3


def c_tables(L, rows):
    """section (c): the AA and 3Di tables of one direction; rows = (row of i, of i max, of iii's first cell, of legal)"""
    ri, rmax, riii, rleg = rows
    pA, p3 = np.full((21, L), -5, np.int32), np.full((21, L), -5, np.int32)
    pA[3], p3[3] = 40, 60
    pA[1], p3[1] = -20000, -20000
    pA[7], p3[7] = -32768, -32768
    pA[0, ri], p3[0, ri] = 20000, 20000
    pA[6, rmax], p3[6, rmax] = 32767, 32767
    pA[4, riii:riii + 2], p3[4, riii:riii + 2] = 10000, 10000
    pA[8, rleg], p3[8, rleg] = 32767, -32000
    return pA, p3


def c_rows(L, reverse):
    if L == 1:
        return 0, 0, 0, 0
    rows = (L - 1, 0, L // 2 - 1, L // 3) if not reverse else (0, L - 1, L // 3, L // 2)
    return rows


def c_single(pA, p3):
    """3Di only (iv): one table holding the two tables' sums, cut to -32768 .. 20000: nothing is left to sum, only H + s can saturate"""
    return np.clip(pA + p3, -32768, 20000)


@functools.lru_cache(maxsize=None)
def world():
    d = db()
    out = []
    for R in CLASSES:
        top, bot = 64 * R, BOTTOM[R]
        plants = [f"plant/{R}/{dr}/{r}" for dr in ("fwd", "rev") for r in planted_rows(R)]
        for aa in (True, False):
            s = f"{R}/{'aa' if aa else '3di'}"
            # (a)
            t_top, t_bot = ordinary(*rand_codes(top), seed=100 + R), ordinary(*rand_codes(bot), seed=200 + R)
            out.append(_q(f"a/rand top/{s}", "a", "rand", aa, t_top, d.ids(*GENERIC, *plants)))
            out.append(_q(f"a/rand bottom/{s}", "a", "rand", aa, t_bot, d.ids(*GENERIC, f"plant/{R}/bottom/fwd", f"plant/{R}/bottom/rev")))
            for kind, L in (("hom", top), ("blk", bot if bot > 10 else top)):
                out.append(_q(f"a/{kind}/{s}", "a", kind, aa, ordinary(*_low(L, kind), seed=0, bias=0), d.ids(*HOMS, "random/65")))
            if R in GAP_VARIANTS:
                go, ge = GAP_VARIANTS[R]
                out.append(_q(f"a/rand top {go}-{ge}/{s}", "a", "rand", aa, t_top, d.ids(*GENERIC, *plants), go, ge))
                out.append(_q(f"a/blk {go}-{ge}/{s}", "a", "blk", aa, ordinary(*_low(top, "blk"), seed=0, bias=0), d.ids(*HOMS), go, ge))
            # (b)
            for k, rows in enumerate(dom_rows(R)):
                (fA, f3), wf = dom_tables(top, rows, aa, 0)
                (rA, r3), wr = dom_tables(top, rows, aa, 7)
                letters = sorted(set(wf) | set(wr))
                out.append(_q(f"b/dom{k}/{s}", "b", "dom", aa, (fA, f3, rA, r3), d.ids(*[f"dom/{c}" for c in letters], "random/1", "random/65", "allX")))
            bonus = hot_bonus(top, aa)
            for kind, (bf, br) in (("hotF", (bonus, 0)), ("hotR", (0, bonus)), ("hotB", (bonus, bonus))):
                t = [x.astype(np.int32) + b for x, b in zip(t_top, (bf, bf, br, br))]
                out.append(_q(f"b/{kind}/{s}", "b", kind, aa, t, d.ids("random/1", "random/2", "random/63", "random/130", "random/400", "relative/400", "masked", "hom/5")))
            if bot > 1:                                                                      # the class's shortest member: one row in its last live lane
                t = [x.astype(np.int32) + 600 for x in t_bot]
                out.append(_q(f"b/hotB bottom/{s}", "b", "hotbot", aa, t, d.ids("random/1", "random/2", "random/63", "random/130", "masked", f"plant/{R}/bottom/fwd", f"plant/{R}/bottom/rev")))
            homA, hom3 = np.full((21, top), -50, np.int32), np.full((21, top), -50, np.int32)
            homA[9], hom3[5] = 300, (300 if aa else 600)                                      # the hom targets' letters
            out.append(_q(f"b/homhot/{s}", "b", "homhot", aa, (homA, hom3, homA, hom3), d.ids(*HOMS, "random/65")))
            ex = exact_tables(top, aa)
            out.append(_q(f"b/exact/{s}", "b", "exact", aa, (ex[0], ex[1], ex[0], ex[1]), d.ids("hom/63", "hom/5", "random/64")))
            # (c)
            for L in sorted({top, bot}):
                fA, f3 = c_tables(L, c_rows(L, False))
                rA, r3 = c_tables(L, c_rows(L, True))
                t = (fA, f3, rA, r3) if aa else (fA, c_single(fA, f3), rA, c_single(rA, r3))
                out.append(_q(f"c/{L}/{s}", "c", "range", aa, t, d.ids(*C_TARGETS)))
    for L in LONG:
        for aa in (True, False):
            t = [x.astype(np.int32) + 600 for x in ordinary(*rand_codes(L), seed=300 + L)]
            out.append(_q(f"b/long/{L}/{'aa' if aa else '3di'}", "b", "long", aa, t, d.ids("random/1", "random/2", "random/65", "random/130", "relative/130", "relative/400")))
    assert len({q.name for q in out}) == len(out)
    return out


def section(sec):
    return [q for q in world() if q.sec == sec]


def targets(q):
    d = db()
    return [d.t3[int(i)] for i in q.ids], [d.tA[int(i)] for i in q.ids]


def tables(q, reverse):
    return (q.pAr, q.p3r) if reverse else (q.pAf, q.p3f)


# ---- the model's answers ----------------------------------------------------------------------------------------------------------------------------
def live(q, reverse):
    pA, p3 = tables(q, reverse)
    t3, tA = targets(q)
    return sm.align_profiles(p3.astype(np.int32), None if pA is None else pA.astype(np.int32), t3, tA if pA is not None else None, q.go, q.ge)


def wrapped(q, reverse):
    """section (c) only (targets hold one letter in both tracks): the records if the int16 pass summed the two tables with a WRAPPING int16 add --
    the column score is then a function of the one letter, so the wrapped sum is a table of its own; the int32 pass adds without a limit"""
    pA, p3 = tables(q, reverse)
    t3, tA = targets(q)
    assert pA is not None and all((a == b).all() for a, b in zip(t3, tA))
    w = ((pA.astype(np.int32) + p3.astype(np.int32) + 32768) % 65536 - 32768).astype(np.int32)
    sc, qe, de = sm.one_pass(w, None, t3, None, q.go, q.ge, 16, True)
    out = np.zeros(len(t3), sm.REC_DT)
    out["score"], out["qEnd"], out["dbEnd"], out["word"] = sc, qe, de, 1
    again = np.flatnonzero(sc == 32767)
    if len(again):
        s2, q2, d2 = sm.one_pass(p3.astype(np.int32), pA.astype(np.int32), [t3[k] for k in again], [tA[k] for k in again], q.go, q.ge, 8, False)
        out["score"][again], out["qEnd"][again], out["dbEnd"][again], out["word"][again] = s2, q2, d2, 2
    return out


def digest(q):
    h = hashlib.blake2b(digest_size=8)
    d = db()
    for part in (q.pAf, q.p3f, q.pAr, q.p3r):
        h.update(b"-" if part is None else part.tobytes()); h.update(b"|")
    h.update(np.array([q.go, q.ge, q.L], np.int32).tobytes())
    for i in q.ids:
        h.update(d.t3[int(i)].tobytes()); h.update(b"/"); h.update(d.tA[int(i)].tobytes()); h.update(b"|")
    return int.from_bytes(h.digest(), "little")


def compute_all():
    """{name: (digest, forward records, reversed records)} from the live model"""
    return {q.name: (digest(q), live(q, False), live(q, True)) for q in world()}


def save(ans):
    os.makedirs(GOLD, exist_ok=True)
    names = sorted(ans)
    np.savez_compressed(ANSWERS, names=np.array(names), keys=np.array([ans[n][0] for n in names], np.uint64), counts=np.array([len(ans[n][1]) for n in names], np.int32),
                        fwd=np.concatenate([ans[n][1] for n in names]).view(np.int32).reshape(-1, 4), rev=np.concatenate([ans[n][2] for n in names]).view(np.int32).reshape(-1, 4))


@functools.lru_cache(maxsize=None)
def frozen():
    """{name: (forward records, reversed records)} from tests/golden/sw_prof_v1; a query whose inputs changed since has no frozen answer"""
    z = np.load(ANSWERS)
    out, b = {}, 0
    by_name = {q.name: q for q in world()}
    assert sorted(by_name) == [str(n) for n in z["names"]], "the world changed: run tests/golden/make_sw_prof_golden.py"
    for name, key, n in zip(z["names"], z["keys"], z["counts"]):
        q = by_name[str(name)]
        if int(key) != digest(q) or n != len(q.ids):
            raise KeyError(f"{name}: inputs changed since the answers were frozen: run tests/golden/make_sw_prof_golden.py")
        out[str(name)] = tuple(np.ascontiguousarray(z[k][b:b + n]).view(sm.REC_DT).reshape(-1) for k in ("fwd", "rev"))
        b += int(n)
    return out


def want(q, reverse):
    return frozen()[q.name][1 if reverse else 0]

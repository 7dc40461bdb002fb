"""The database, the queries and the expected hit lists `class Marv` (include/marv.h, foldseek_amd/csrc/host/marv_shim.cpp) is held to.

Nothing here asks the shim or fshost_prefilter_profile for an expectation:
    profile    pssm[a][i] = matrix[a][q_i] + cb[i], matrix from helpers.o_submat, cb from helpers.o_round_bias (the C oracle, which the CPU suite pins
               to the reference's own translation units)
    cap        255 - fso_ungapped_bias(tinyMatrix, 21, cb, L): |min(matrix)| + |min(0, min(cb))|, the matrix-WIDE minimum
    scores     gapless_model.scores(pssm, cap, db)
    hit list   gapless_model.select(scores, -1, -1, maxSeqs): every target qualifies, (score descending, id ascending), the first min(maxSeqs, n)
One case is the documented exception: a profile of a matrix the shim does not carry (3Di at 1.0 bits) whose query holds no column with the matrix's
minimum.  The shim reads the minimum off the profile there, so its cap is 255 - (|min(pssm[a][i] - pssm[X][i])| + |min(0, min pssm[X][i])|), which is
higher than the CPU path's; tests/test_marv_cases.py asserts that the two differ.

tests/test_marv_cases.py checks the conditions that make these cases worth running; tests/test_marv_direct_gpu.py runs them."""
import functools

import numpy as np

import gapless_model as gm
import helpers
from foldseek_amd import synth

X = 20
SEED = 20261
# --comp-bias-corr-scale: the prefilter's own 0.15 rounds to a bias of zero on most 3Di queries, so the long queries run at 1.0 as well
SCALE_3DI, SCALE_FULL, SCALE_AA = 0.15, 1.0, 1.0
SHARDS = (1, 2, 3, 7)
TIE_MAX_SEQS = 5                         # a cut strictly inside the group of targets at the cap (at least ten by construction)
L_LONG, L_AA, L_POLY = 897, 150, 160     # the long 3Di query (the first row-tiled length), the BLOSUM62 query, the one-letter targets
COPIES = 10


class Case:
    def __init__(self, name, matrix, seq, comp_bias, saturating, profile_cap=False):
        """matrix: (name in fs_params.h, bit factor, composition-bias scale)"""
        self.name, self.matrix, self.saturating, self.comp_bias, self.profile_cap = name, matrix, saturating, comp_bias, profile_cap
        self.seq = np.ascontiguousarray(seq, np.uint8)
        self.L = len(self.seq)
        sub, pb = helpers.o_submat(matrix[0], matrix[1])
        self.tiny = np.ascontiguousarray(sub, np.int16).astype(np.int8)
        self.cb = helpers.o_round_bias(sub, pb, self.seq, matrix[2])[1] if comp_bias else np.zeros(self.L, np.int8)
        m = sub.reshape(21, 21).astype(np.int32)
        p = m[:, self.seq] + self.cb.astype(np.int32)[None, :]
        assert np.abs(p).max() <= 127
        self.pssm = np.ascontiguousarray(p.astype(np.int8))
        self.matrix_min = int(m.min())
        self.matrix_cap = 255 - int(helpers.oracle().fso_ungapped_bias(self.tiny, 21, self.cb, self.L))
        # what the shim can know of an unknown matrix: its X row is zero, so pssm[X] is the bias and pssm[a] - pssm[X] the matrix entry
        self.derived_cap = 255 - (abs(int(min(0, (p - p[X]).min()))) + abs(int(min(0, p[X].min()))))
        self.cap = self.derived_cap if profile_cap else self.matrix_cap


def _background(rng, n, back):
    return rng.choice(20, size=n, p=back / back.sum()).astype(np.uint8)


def _poly_letter():
    """a letter whose column holds the minimum of neither 3Di matrix (2.0 and 1.0 bits) and that scores most against itself"""
    ok = None
    for bits in (2.0, 1.0):
        m = helpers.o_submat("MAT3DI", bits)[0].reshape(21, 21).astype(np.int32)
        lacks = m[:, :20].min(axis=0) > m.min()
        ok = lacks if ok is None else ok & lacks
    m = helpers.o_submat("MAT3DI", 1.0)[0].reshape(21, 21).astype(np.int32)
    cand = np.flatnonzero(ok)
    assert len(cand)
    return int(cand[np.argmax(m[cand, cand])])


def _padded(seqs):
    """PaddedDB of the code strings in the order given: every entry padded with X to a multiple of 4"""
    lens = np.array([len(s) for s in seqs], np.int32)
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    data = np.full(int(offsets[-1]), X, np.uint8)
    for k, s in enumerate(seqs):
        data[offsets[k]:offsets[k] + lens[k]] = s
    return synth.PaddedDB(data, None, offsets, lens)


def subset(db, ids):
    """the entries ids of db, in that order, as a database of their own (shard k of N is subset(db, range(k, n, N)))"""
    return _padded([db.seq(int(i), unmask=False) for i in ids])


def unpadded(db):
    """(data, offsets) of the same entries in a buffer that ends with the last entry's last residue"""
    end = int(db.offsets[db.n - 1]) + int(db.lengths[db.n - 1])
    off = db.offsets.copy()
    off[db.n] = end
    return db.data3di[:end].copy(), off


@functools.lru_cache(maxsize=None)
def world():
    """-> dict(db, packed, queries Q / QB, letter, copies of each planted query); seeded, built once per process"""
    rng = np.random.default_rng(SEED)
    Q = _background(rng, L_LONG, synth.BACK_3DI)
    QB = _background(rng, L_AA, synth.BACK_AA)
    letter = _poly_letter()
    seqs, kind = [], []
    for T in (1, 1, 2, 2, 3, 3, 5, 5, 15, 16, 17, 63, 64, 65, 4, 8, 700, 699):
        seqs.append(_background(rng, T, synth.BACK_3DI)); kind.append("edge")
    for k in range(190):
        T = int(rng.integers(6, 640))
        s = _background(rng, T, synth.BACK_3DI if k % 2 else synth.BACK_AA)
        if k % 3 == 0:                                  # a mutated piece of a query: scores between the background's and the cap
            src = Q if k % 2 else QB
            n = int(rng.integers(4, min(T, len(src), 120) + 1))
            a, b = int(rng.integers(0, len(src) - n + 1)), int(rng.integers(0, T - n + 1))
            piece = src[a:a + n].copy()
            hit = rng.random(n) < rng.choice([0.05, 0.2, 0.4])
            piece[hit] = rng.integers(0, 20, int(hit.sum()))
            s[b:b + n] = piece
        if k % 5 == 0:                                  # soft-masked residues, some of them X
            mask = rng.random(T) < 0.08
            s[mask] += 32
            if k % 10 == 0:
                s[int(rng.integers(0, T))] = 32 + X
        seqs.append(s); kind.append("random")
    for T, fill in ((3, X), (16, X), (65, X), (30, 32 + X)):
        seqs.append(np.full(T, fill, np.uint8)); kind.append("allx")
    for what, s in (("Q", Q), ("QB", QB), ("poly", np.full(L_POLY, letter, np.uint8))):
        for _ in range(COPIES):
            seqs.append(s.copy()); kind.append(what)
    order = np.argsort([len(s) for s in seqs], kind="stable")      # the padded layout is sorted by length
    db = _padded([seqs[i] for i in order])
    kind = np.array(kind)[order]
    return dict(db=db, packed=gm.pack(db), Q=Q, QB=QB, letter=letter, copies={w: np.flatnonzero(kind == w) for w in ("Q", "QB", "poly")},
                allx=np.flatnonzero(kind == "allx"))


MAT_3DI, MAT_3DI_FULL, MAT_AA, MAT_OTHER = ("MAT3DI", 2.0, SCALE_3DI), ("MAT3DI", 2.0, SCALE_FULL), ("BLOSUM62", 2.0, SCALE_AA), ("MAT3DI", 1.0, SCALE_FULL)
MAT_OTHER_LOW = ("MAT3DI", 1.0, SCALE_3DI)     # a one-letter query's bias at the full scale is beyond what the shim accepts in an X row


@functools.lru_cache(maxsize=None)
def cases():
    w = world()
    Q, QB, c = w["Q"], w["QB"], w["letter"]
    out = [Case(f"3di_L{L}", MAT_3DI, Q[:L], True, L >= 64) for L in (1, 5, 64)]
    out += [Case(f"3di_L{L}", MAT_3DI_FULL, Q[:L], True, True) for L in (300, L_LONG)]
    out += [Case("3di_L300_nobias", MAT_3DI, Q[:300], False, True),
            Case("blosum62", MAT_AA, QB, True, True),
            Case("3di_one_letter", MAT_3DI, np.full(100, c), True, True),           # branch (1), no column holds the matrix's minimum
            Case("all_x", MAT_3DI, np.full(33, X), True, False),
            Case("other_matrix_with_min", MAT_OTHER, Q[:300], True, True),          # branch (2), the profile holds the matrix's minimum
            Case("other_matrix_without_min", MAT_OTHER_LOW, np.full(L_POLY, c), True, True, profile_cap=True)]
    return {q.name: q for q in out}


@functools.lru_cache(maxsize=None)
def scores(name):
    """the expected score of every target (int32), read-only"""
    q = cases()[name]
    s = gm.scores(q.pssm, q.cap, world()["packed"])
    s.setflags(write=False)
    return s


def expected(name, max_seqs, want=None):
    return gm.select(scores(name) if want is None else want, -1, -1, max_seqs)


@functools.lru_cache(maxsize=None)
def other_db():
    """database B of the handle tests: the entries of the first with every letter moved on by seven (masked letters stay masked, X stays X)"""
    db = world()["db"]
    d = db.data3di.copy()
    low, masked = d < 20, (d >= 32) & (d < 52)
    d[low] = (d[low] + 7) % 20
    d[masked] = 32 + (d[masked] - 32 + 7) % 20
    return synth.PaddedDB(d, None, db.offsets, db.lengths)


@functools.lru_cache(maxsize=None)
def scores_on(name, which):
    """expected scores of case `name` on another database: "B", or ("first", k) = the first k entries... see small_db"""
    q = cases()[name]
    db = other_db() if which == "B" else small_db(which)
    s = gm.scores(q.pssm, q.cap, db)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def small_db(k):
    """k entries taken from the large database: a copy of the long query first in id order is not possible in a sorted layout, so a mid-length
    target that scores and, for k = 2, a copy of the long query after it"""
    w = world()
    mid = int(np.argmax(np.where(w["db"].lengths < 600, scores("3di_L300"), -1)))
    return subset(w["db"], [mid, int(w["copies"]["Q"][0])][:k])

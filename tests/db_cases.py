"""tests/db_cases.py -- the table shapes the database entry (fsgpu_db_load, fsgpu_db_adopt_device, fsgpu_db_broadcast) is held to, with the answers of
the independent models for them (TEST INFRASTRUCTURE: of the project only synth.PaddedDB, a plain container, and the host-side profile builder are used).

A shape is one table: seeded residues laid out in a byte buffer by offsets and lengths.  shapes() names them all; tests/test_db_table_host.py runs
every one through fsgpu_db_check_table, tests/test_db_entry_gpu.py loads every one and compares the scan with tests/gapless_model.py, the three
Smith-Waterman kernels with tests/sw_model.py, the diagonal rescoring with tests/diag_model.py, the k-mer index and search with the C oracle and the block
aligner with tests/ba_model.py.  The models read a target through the loader's documented rule for its bytes, stated here once (scan_bytes, aligner_bytes,
kmer_bytes): three lines of numpy, applied BEFORE the models.

What the models need more than about a second for -- everything on `longest`, whose targets reach FSGPU_MAX_SEQ_LEN -- is frozen in
tests/golden/db_v1/answers.npz by tests/golden/make_db_golden.py; tests/test_db_table_host.py re-runs the live model on every ninth frozen case.
refusals() are the tables the entries must refuse, with the index fsgpu_db_check_table has to name."""
import collections
import functools
import os

import numpy as np

import diag_model as dm
import gapless_model as gm
import sw_cases as K
import sw_model as sm
from foldseek_amd import api, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "db_v1")
ANSWERS = os.path.join(GOLD, "answers.npz")
MAX_LEN = 65535                      # FSGPU_MAX_SEQ_LEN
LIVE = False                         # the generator sets this: nothing is read from the frozen answers
GO, GE = 10, 1
SW_FIELDS = ("score", "qEnd", "dbEnd", "word")

Shape = collections.namedtuple("Shape", "name db pool note")          # pool[i]: identity of entry i in the pool its table was laid out from (or None)


# ---- the loader's rule for the bytes of an entry ----------------------------------------------------------------------------------------------------
def scan_bytes(raw):
    """the scan copy: every byte above 20 is X (soft-masked residues and anything unknown)"""
    return np.where(np.asarray(raw) > 20, 20, raw).astype(np.uint8)


def aligner_bytes(raw):
    """the aligner copies: 32 off a byte of 32 or more, then everything above 20 is X"""
    c = np.where(np.asarray(raw) >= 32, np.asarray(raw).astype(np.int64) - 32, raw)
    return np.where(c > 20, 20, c).astype(np.uint8)


def kmer_bytes(raw):
    """what the k-mer oracle is given: legal bytes as they are (the mask flag kept), every other byte X -- below 32 by the aligner rule, from 53 on because
    a byte of 32 or more is masked (maskLowerCase) whatever is left of it"""
    raw = np.asarray(raw)
    return np.where((raw <= 20) | ((raw >= 32) & (raw <= 52)), raw, 20).astype(np.uint8)


def entry(db, i, which="3di"):
    d = db.data3di if which == "3di" else db.dataaa
    return np.asarray(d[int(db.offsets[i]):int(db.offsets[i]) + int(db.lengths[i])])


def aligner_target(db, i):
    """(3Di, AA) codes as the aligner reads entry i; AA all X for a table without AA data (never read then)"""
    t3 = aligner_bytes(entry(db, i))
    return t3, (aligner_bytes(entry(db, i, "aa")) if db.dataaa is not None else np.full(len(t3), 20, np.uint8))


def scan_db(db):
    """the table as the scan model takes it: the same layout with the scan rule applied to every byte"""
    return synth.PaddedDB(scan_bytes(db.data3di), None, db.offsets, db.lengths)


# ---- queries ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query(L):
    """K.Query of L residues: codes 0..19 with one X from 5 residues on, biases in -3..3 for both directions"""
    rng = np.random.default_rng(7700 + L)
    q3, qa = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
    if L > 4:
        q3[int(rng.integers(0, L))] = 20
    return K.Query(q3, qa, *[rng.integers(-3, 4, L).astype(np.int8) for _ in range(4)])


@functools.lru_cache(maxsize=None)
def scan_profile(L):
    """(pssm int8 [21, L], cap) of query(L) as the prefilter builds it"""
    return api.prefilter_profile(api.Matrix(0, 2.0), query(L).q3, True, 0.15)


SCAN_LENGTHS = (1, 17, 300)
SW_LENGTHS = (17, 300)
LONG_SCAN_LENGTHS = (1, 17, 300, 897)        # 897: the first row-tiled query
LONG_SW_LENGTHS = (40, 300)


def scan_lengths(shape):
    """the row-tiled query also meets the tables with a stripe that holds no column: the tiled path stores its scores through another buffer"""
    return LONG_SCAN_LENGTHS if shape.name in ("longest", "empty_stripe", "all_empty") else SCAN_LENGTHS


def sw_lengths(shape):
    return LONG_SW_LENGTHS if shape.name == "longest" else SW_LENGTHS


# ---- residues ----------------------------------------------------------------------------------------------------------------------------------------
def make_entry(rng, L):
    """(3Di bytes, AA bytes) of L residues: i.i.d. letters around a mutated piece of query(300) or query(17), now and then an X and a soft-masked stretch
    (+32, in both strings: the aligner has to take it off again)"""
    t3, ta = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
    if L >= 6:
        q = query(300) if rng.random() < 0.7 else query(17)
        n = int(min(L, len(q.q3), rng.integers(6, 120)))
        a, b = int(rng.integers(0, len(q.q3) - n + 1)), int(rng.integers(0, L - n + 1))
        keep = rng.random(n) >= 0.12
        t3[b:b + n] = np.where(keep, q.q3[a:a + n], t3[b:b + n])
        ta[b:b + n] = np.where(keep, q.qa[a:a + n], ta[b:b + n])
    if L >= 3 and rng.random() < 0.4:
        t3[int(rng.integers(0, L))] = 20
    if L >= 2 and rng.random() < 0.4:
        a = int(rng.integers(0, L - 1))
        b = int(min(L, a + rng.integers(1, 12)))
        t3[a:b] += 32
        ta[a:b] += 32
    return t3, ta


def lay_out(entries, offsets, nbytes, fill=None, aa=True):
    """entries [(3Di bytes, AA bytes)] at the byte offsets given, in a buffer of nbytes; every other byte is 20, or fill[i] (values that would score)"""
    d3 = np.full(nbytes, 20, np.uint8) if fill is None else np.asarray(fill, np.uint8).copy()
    da = d3.copy()
    for (t3, ta), o in zip(entries, offsets):
        d3[o:o + len(t3)] = t3
        da[o:o + len(ta)] = ta
    off = np.array(list(offsets) + [nbytes], np.int64)
    return synth.PaddedDB(d3, da if aa else None, off, np.array([len(e[0]) for e in entries], np.int32))


def padded(entries, aa=True):
    """the layout of a padded database: the entries in the order given, each padded with X to a multiple of 4"""
    lens = np.array([len(e[0]) for e in entries], np.int64)
    off = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
    return lay_out(entries, [int(x) for x in off[:-1]], int(off[-1]), aa=aa)


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 7, 8, 9, 16, 17)               # the last stripe with 1, 7, 0 (full), 1, 0 and 1 live slots
COUNT_LENGTHS = (33, 1, 15, 16, 17, 31, 32, 5, 48, 2, 64, 100, 3, 65, 7, 129, 20)
EMPTY_LENGTHS = (0, 5, 0, 0, 40, 0, 17, 0, 0)
# by length: six empty entries share a stripe with the 5 and the 17, the 40 is alone in the second
EMPTY_STRIPE_LENGTHS = (0, 0, 12, 0, 0, 0, 0, 30, 0, 0, 0)          # nine empty entries: a whole stripe without a single column, and one more
ORDER_POOL = (24,) * 10 + (57,) * 8 + (1, 2, 9, 33, 64, 100, 130, 257)
BYTES_POOL = (1, 5, 16, 17, 33, 40, 64, 65, 100, 129, 257, 300)


def _pool(seed, lengths):
    rng = np.random.default_rng(seed)
    return [make_entry(rng, L) for L in lengths]


def _counts(n):
    pool = _pool(100 + n, sorted(COUNT_LENGTHS[:n]))
    return Shape(f"counts{n}", padded(pool), None, f"{n} entries in ascending length")


def _empty(name, lengths):
    pool = _pool(200 + len(lengths), lengths)
    return Shape(name, padded(pool), None, f"lengths {lengths} in this order")


def _all_empty():
    n = 9
    db = synth.PaddedDB(np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(n + 1, np.int64), np.zeros(n, np.int32))
    return Shape("all_empty", db, None, "nine entries without residues, bytes == 0")


def _order(which):
    pool = _pool(300, ORDER_POOL)
    asc = sorted(range(len(pool)), key=lambda k: len(pool[k][0]))
    rng = np.random.default_rng(301)
    ids = dict(ascending=asc, descending=asc[::-1], equal=[k for k in range(len(pool)) if len(pool[k][0]) == 24],
               strict=[k for k in asc[::-1] if ORDER_POOL.count(len(pool[k][0])) == 1], ties=[int(k) for k in rng.permutation(len(pool))])[which]
    return Shape(f"order_{which}", padded([pool[k] for k in ids]), ids, "the pool of order_* by length: " + which)


def _bytes(which):
    pool = _pool(400, BYTES_POOL)
    rng = np.random.default_rng(401)
    lens = [len(e[0]) for e in pool]
    if which == "odd":                      # no padding at all, the first entry at byte 1
        off = [1 + sum(lens[:k]) for k in range(len(pool))]
        nbytes, fill = 1 + sum(lens), None
    elif which == "gaps":                   # 1..70 bytes between entries (and before the first, behind the last), holding residues that would score
        gaps = rng.integers(1, 71, len(pool) + 1)
        off = [int(gaps[:k + 1].sum()) + sum(lens[:k]) for k in range(len(pool))]
        nbytes = off[-1] + lens[-1] + int(gaps[-1])
        fill = rng.integers(0, 20, nbytes)
    else:                                   # descending memory order: entry 0 last in the buffer, padded to 4
        pad = [(x + 3) // 4 * 4 for x in lens]
        nbytes, fill = sum(pad), None
        off = [nbytes - sum(pad[:k + 1]) for k in range(len(pool))]
    return Shape(f"bytes_{which}", lay_out(pool, off, nbytes, fill), list(range(len(pool))), "the pool of bytes_*: " + which)


def _codes():
    rng = np.random.default_rng(500)
    legal = np.concatenate([np.arange(21), np.arange(32, 53)]).astype(np.uint8)
    illegal = np.concatenate([np.arange(21, 32), np.arange(53, 256)]).astype(np.uint8)
    masked = make_entry(rng, 30)
    masked = ((masked[0] % 32) + 32).astype(np.uint8), ((masked[1] % 32) + 32).astype(np.uint8)
    x = make_entry(rng, 25)
    x[0][:] %= 32
    x[0][12] = 52
    x[1][3] = 52
    pool = [(legal, legal[::-1].copy()), masked, x, (illegal, np.roll(illegal, 77)), (np.tile(illegal[:11], 3), make_entry(rng, 33)[1])]
    pool += [make_entry(rng, L) for L in (8, 41, 120)]
    return Shape("codes", padded(pool), None, "every legal code, a fully soft-masked entry, a soft-masked X, two entries of illegal bytes")


LONG_LENGTHS = (65535, 65534, 32769, 32768, 32767, 1)
LONG_SHORT = (3, 17, 40, 64, 129, 300, 640, 1000)
# (query length, first column) of the planted copies per long target: end cells at the final column, around column 32767 and at column 39
LONG_PLANTS = {0: ((300, 65535 - 300), (40, 32771 - 40)), 1: ((40, 65534 - 40), (300, 32776 - 300)), 2: ((300, 32769 - 300), (40, 0)),
               3: ((40, 32768 - 40), (300, 0)), 4: ((300, 32767 - 300), (40, 20000))}


def _longest():
    rng = np.random.default_rng(600)
    pool = []
    for k, L in enumerate(LONG_LENGTHS):
        t3, ta = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
        for qL, at in LONG_PLANTS.get(k, ()):
            t3[at:at + qL], ta[at:at + qL] = query(qL).q3, query(qL).qa
        pool.append((t3, ta))
    pool += [make_entry(rng, L) for L in LONG_SHORT]
    order = sorted(range(len(pool)), key=lambda k: len(pool[k][0]))
    return Shape("longest", padded([pool[k] for k in order]), order, "targets of 65535, 65534, 32769, 32768, 32767 and 1 residues and eight short ones")


def _no_aa():
    s = _counts(9)
    return Shape("no_aa", synth.PaddedDB(s.db.data3di, None, s.db.offsets, s.db.lengths), None, "counts9 without AA data")


_BUILDERS = collections.OrderedDict(
    [(f"counts{n}", functools.partial(_counts, n)) for n in COUNTS] +
    [("empty_entries", functools.partial(_empty, "empty_entries", EMPTY_LENGTHS)), ("empty_stripe", functools.partial(_empty, "empty_stripe", EMPTY_STRIPE_LENGTHS)),
     ("all_empty", _all_empty)] +
    [(f"order_{w}", functools.partial(_order, w)) for w in ("ascending", "equal", "descending", "strict", "ties")] +
    [(f"bytes_{w}", functools.partial(_bytes, w)) for w in ("odd", "gaps", "descending")] +
    [("codes", _codes), ("longest", _longest), ("no_aa", _no_aa)])
NAMES = tuple(_BUILDERS)
BACKTRACE_NAMES = ("empty_entries", "bytes_odd", "bytes_gaps", "bytes_descending", "longest")


@functools.lru_cache(maxsize=None)
def shape(name):
    return _BUILDERS[name]()


def long_id(sh, k):
    """id of pool entry k of `longest` (k = 0..5: the long targets in the order of LONG_LENGTHS) in its table"""
    return sh.pool.index(k)


# ---- frozen answers ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frozen():
    return dict(np.load(ANSWERS)) if os.path.exists(ANSWERS) else {}


def _frozen_or(key, compute):
    if not LIVE and key in frozen():
        return frozen()[key]
    if not LIVE and key.startswith("longest"):
        raise KeyError(f"{key}: no frozen model answer, run tests/golden/make_db_golden.py")
    return compute()


# ---- the models' answers ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_want(name, L):
    """gapless_model's score of query(L) for every target of the shape"""
    def compute():
        pssm, cap = scan_profile(L)
        return gm.scores(pssm, cap, scan_db(shape(name).db))
    return np.asarray(_frozen_or(f"{name}/scan/{L}", compute), np.int32)


def sw_ids(sh, L):
    """the targets a Smith-Waterman query of L residues is paired with: all of them, except that on `longest` the 300-residue query meets only two of the
    five long targets (65535 and 32768 residues; a 65535-column target runs on a single wave)"""
    if sh.name == "longest" and L == 300:
        return np.array([i for i in range(sh.db.n) if sh.pool[i] in (0, 3) or sh.pool[i] >= 5], np.uint32)
    return np.arange(sh.db.n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def sw_want(name, L, reverse, with_aa):
    """sw_model's records of query(L) in one direction against sw_ids, with both matrices or 3Di only"""
    sh = shape(name)

    def compute():
        m3, mA = K.matrices()
        r = K.live(m3, mA if with_aa else None, query(L), bool(reverse), [aligner_target(sh.db, int(i)) for i in sw_ids(sh, L)], GO, GE)
        return np.array([[int(x[f]) for f in SW_FIELDS] for x in r], np.int32).reshape(-1, 4)
    rec = np.asarray(_frozen_or(f"{name}/sw/{L}/{int(reverse)}/{int(with_aa)}", compute), np.int32).reshape(-1, 4)
    out = np.zeros(len(rec), sm.REC_DT)
    for k, f in enumerate(SW_FIELDS):
        out[f] = rec[:, k]
    return out


def diag_queries(sh):
    """[(AA codes, 3Di codes)] of the rescoring call: query(17), query(300) and, on `longest`, a 65535-residue relative of its longest target"""
    qs = [(query(L).qa, query(L).q3) for L in SW_LENGTHS]
    if sh.name == "longest":
        rng = np.random.default_rng(601)
        t3, ta = aligner_target(sh.db, long_id(sh, 0))
        hit = rng.random(len(t3)) < 0.3
        qs.append((np.where(hit, rng.integers(0, 20, len(ta)), ta).astype(np.uint8), np.where(hit, rng.integers(0, 20, len(t3)), t3).astype(np.uint8)))
    return qs


def diag_pairs(sh):
    """(query, target, diagonal): diagonals 0 and +-1 of every target with the first two queries; on `longest` the long query against the longest target
    on 0, +-1, +-32767, +-32768 and the last legal diagonals +-65534 (and one beyond), the 300-residue query on its own last ones"""
    pairs = [(q, t, d) for q in range(2) for t in range(sh.db.n) for d in (0, 1, -1)]
    if sh.name == "longest":
        t0, t1 = long_id(sh, 0), long_id(sh, 1)
        pairs += [(2, t0, d) for d in (0, 1, -1, 32767, -32767, 32768, -32768, 65534, -65534, 65535, -65535)]
        pairs += [(2, t1, d) for d in (0, -1, 65533, -65533)] + [(1, t0, d) for d in (299, 300, -65234, -65235, -65534)]
    return pairs


@functools.lru_cache(maxsize=None)
def diag_want(name):
    """diag_model's eight fields per pair of diag_pairs, int32 [pairs, 8].  A target without residues has no cell on any diagonal and the reference would
    look at the byte behind it: the entry answers NO_OVERLAP for it (include/fsgpu.h), stated here, not taken from the model"""
    sh = shape(name)

    def compute():
        m3, mA = (np.asarray(m, np.int64).tolist() for m in K.matrices())
        targets = [aligner_target(sh.db, i)[::-1] for i in range(sh.db.n)]           # (AA, 3Di)
        out = []
        for q, t, d in diag_pairs(sh):
            if len(targets[t][0]) == 0:
                r = dict(score=0, startPos=-1, endPos=-1, revScore=0, diagonalLen=0, identicalAA=0, status=dm.NO_OVERLAP, reserved=0)
            else:
                r = dm.rescore_pair(diag_queries(sh), targets, (q, t, d), m3, mA)
            out.append([r[f] for f in dm.FIELDS])
        return np.array(out, np.int32).reshape(-1, 8)
    return np.asarray(_frozen_or(f"{name}/diag", compute), np.int32).reshape(-1, 8)


def frozen_keys():
    """every key tests/golden/make_db_golden.py freezes, with the call that computes it live"""
    keys = [(f"longest/scan/{L}", functools.partial(scan_want, "longest", L)) for L in LONG_SCAN_LENGTHS]
    keys += [(f"longest/sw/{L}/{r}/{a}", functools.partial(sw_want, "longest", L, r, a)) for L in LONG_SW_LENGTHS for r in (0, 1) for a in (1, 0)]
    keys.append(("longest/diag", functools.partial(diag_want, "longest")))
    return keys


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
Refusal = collections.namedtuple("Refusal", "name db index")          # index: what fsgpu_db_check_table returns; None: refused before the table is looked at


@functools.lru_cache(maxsize=None)
def refusals():
    base = shape("counts9").db

    def variant(name, index, offsets=None, lengths=None, data=None):
        d3, da = (base.data3di, base.dataaa) if data is None else data
        return Refusal(name, synth.PaddedDB(d3, da, base.offsets.copy() if offsets is None else offsets, base.lengths.copy() if lengths is None else lengths), index)

    nbytes = int(base.data3di.size)
    out = []
    off = base.offsets.copy(); off[4] = nbytes + 1
    out.append(variant("offset_past_bytes", 4, offsets=off))
    off = base.offsets.copy(); off[8] = nbytes - int(base.lengths[8]) + 1
    out.append(variant("last_residue_past_bytes_by_one", 8, offsets=off))
    off = base.offsets.astype(np.uint64); off[2] = np.uint64(2 ** 64 - 3)            # + 15 residues = 12: a sum that wraps into the buffer
    out.append(variant("offset_wraps", 2, offsets=off))
    off = base.offsets.copy(); off[9] = nbytes + 1
    out.append(variant("end_past_bytes", 9, offsets=off))
    ln = base.lengths.copy(); ln[3] = -1
    out.append(variant("negative_length", 3, lengths=ln))
    big = np.full(MAX_LEN + 1, 7, np.uint8)
    out.append(Refusal("longer_than_max", synth.PaddedDB(big, big, np.array([0, 0, MAX_LEN + 1], np.int64), np.array([0, MAX_LEN + 1], np.int32)), 1))
    out.append(Refusal("no_entries", synth.PaddedDB(base.data3di, base.dataaa, np.array([nbytes], np.int64), np.zeros(0, np.int32)), None))
    # refused by name: two entries over one byte.  Entry 5 begins on the last residue of entry 4; in the second table entry 2 begins where entry 6 does
    # (the later of the two is named); in the third the table is in descending memory order and entry 1 reaches into entry 0
    off = base.offsets.copy(); off[5] = off[4] + int(base.lengths[4]) - 1
    out.append(variant("overlap_by_one", 5, offsets=off))
    off = base.offsets.copy(); off[2] = off[6]
    out.append(variant("overlap_same_start", 6, offsets=off))
    d = shape("bytes_descending").db
    off = d.offsets.copy(); off[1] = off[0] - int(d.lengths[1]) + 1
    out.append(Refusal("overlap_descending", synth.PaddedDB(d.data3di, d.dataaa, off, d.lengths.copy()), 0))
    # several bad entries: the first one is named, whatever its kind
    off = base.offsets.copy(); off[7] = nbytes + 5; off[5] = off[4] + 1; ln = base.lengths.copy(); ln[8] = -4
    out.append(variant("several_overlap_first", 5, offsets=off, lengths=ln))
    off = base.offsets.copy(); off[1] = nbytes; off[5] = off[4] + 1
    out.append(variant("several_outside_first", 1, offsets=off))
    return out


def check_table_model(offsets, lengths, nbytes):
    """fsgpu_db_check_table from its definition, in Python integers and quadratic: the lowest index of an entry whose length is out of range, which lies
    outside the buffer, or which begins inside another entry (of two that begin at one address, the later in the table)"""
    off, ln, n = [int(x) for x in np.asarray(offsets, np.uint64)], [int(x) for x in lengths], len(lengths)
    inside = [0 <= ln[t] <= MAX_LEN and off[t] + ln[t] <= nbytes for t in range(n)]
    for t in range(n):
        if not inside[t]:
            return t
        for u in range(n):
            if u != t and inside[u] and ln[t] > 0 and ln[u] > 0 and off[u] <= off[t] < off[u] + ln[u] and (off[u] < off[t] or u < t):
                return t
    return -1 if off[n] <= nbytes else n

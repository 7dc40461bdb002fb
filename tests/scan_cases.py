"""tests/scan_cases.py -- the seeded inputs of the whole-database Smith-Waterman scan (fsgpu_sw_scan_c) and the frozen records of tests/sw_model.py for
them (TEST INFRASTRUCTURE: of the project only synth.PaddedDB, a plain container, is used; nothing is read outside tests/golden).

One database of a few hundred targets at most -- the lengths at which k_sw3's shapes and the planner's thresholds change, some sixty random ones, mutated
pieces of the queries -- in a SHUFFLED order of entries, so that the longest-first order the scan runs in is unrelated to the id order it answers in.
Queries at the borders of the rows-per-lane classes and of the compact path.  Every record of every (query, target) pair comes from sw_model.align and is
frozen in tests/golden/scan_v1/answers.npz by tests/golden/make_scan_golden.py; tests/test_scan_cases.py re-runs a sample live and asserts, from the
model alone, what makes the GPU test mean something."""
import functools
import hashlib
import os

import numpy as np

import sw_cases as K
import sw_model as sm
from foldseek_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "scan_v1")
ANSWERS = os.path.join(GOLD, "answers.npz")

FIXED_LENGTHS = [0, 1, 15, 16, 17, 511, 512, 513, 895, 896, 897, 1300]
N_RANDOM = 60
Q_LENGTHS = [1, 31, 32, 33, 200, 512, 513, 1024, 1025]
CONFIGS = [(2, 10, 1), (2, 12, 2), (0, 10, 1), (0, 12, 2)]          # (alignment type: 2 = 3Di + AA, 0 = 3Di; gap open; gap extend)
CUTOFF_KINDS = ("zero", "occurs", "occurs+1", "median", "max")
FIELDS = ("score", "qEnd", "dbEnd", "word")
SAT_CUTOFFS = (32767, 1000)


def config_name(cfg):
    return "t%d_%d_%d" % cfg


@functools.lru_cache(maxsize=None)
def queries():
    return [K.make_query(L, 7000 + L, "related") for L in Q_LENGTHS]


def _mutated(rng, s3, sa, rate=0.1):
    s3, sa = s3.copy(), sa.copy()
    m = rng.random(len(s3)) < rate
    s3[m] = rng.integers(0, 20, int(m.sum())); sa[m] = rng.integers(0, 20, int(m.sum()))
    return s3, sa


@functools.lru_cache(maxsize=None)
def db():
    """PaddedDB with .kind per entry; entries in a seeded random order, padded to multiples of 4 with X"""
    rng = np.random.default_rng(20261020)
    entries = []
    for L in FIXED_LENGTHS:
        entries.append((rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8), "fixed"))
    for L in rng.integers(20, 421, N_RANDOM):
        entries.append((rng.integers(0, 20, int(L)).astype(np.uint8), rng.integers(0, 20, int(L)).astype(np.uint8), "random"))
    for q in queries():
        L = len(q.q3)
        if L < 31:
            continue
        for _ in range(3):                                        # a piece of the query, one residue in ten redrawn, between random flanks
            n = int(rng.integers(min(20, L), min(L, 400) + 1))
            a = int(rng.integers(0, L - n + 1))
            p3, pa = _mutated(rng, q.q3[a:a + n], q.qa[a:a + n])
            f0, f1 = int(rng.integers(0, 11)), int(rng.integers(0, 11))
            t3 = np.concatenate([rng.integers(0, 20, f0), p3, rng.integers(0, 20, f1)]).astype(np.uint8)
            ta = np.concatenate([rng.integers(0, 20, f0), pa, rng.integers(0, 20, f1)]).astype(np.uint8)
            entries.append((t3, ta, "piece"))
    order = rng.permutation(len(entries))
    entries = [entries[k] for k in order]
    lens = np.array([len(e[0]) for e in entries], np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(max(int(off[-1]), 1), 20, np.uint8), np.full(max(int(off[-1]), 1), 20, np.uint8)
    for k, (t3, ta, _) in enumerate(entries):
        d3[off[k]:off[k] + lens[k]] = t3
        da[off[k]:off[k] + lens[k]] = ta
    out = synth.PaddedDB(d3, da, off, lens)
    out.kind = [e[2] for e in entries]
    return out


def other_db():
    """a different database (other entries, other n) for the reload test: the first forty entries of db(), reversed"""
    d = db()
    ts = [K.target(d, i) for i in range(40)][::-1]
    return K.pack([(t3, ta, "other") for t3, ta in ts])


def targets(d=None):
    d = d or db()
    return [K.target(d, i) for i in range(d.n)]


def matrices(atype):
    m3, mA = K.matrices()
    return m3, (mA if atype == 2 else None)


@functools.lru_cache(maxsize=None)
def sat_case():
    """(m3, mA, query): matrices inflated as far as int8 goes and a forward bias of +100 per position: the long targets saturate the int16 pass, the
    short ones do not"""
    m3, mA = K.matrices()
    f = min(127 // int(m3.max()), 128 // -int(m3.min()), 127 // int(mA.max()), 128 // -int(mA.min()))
    assert f >= 2
    q = K.make_query(200, 7777, "random")
    hot = np.full(200, 100, np.int8)
    return (m3.astype(np.int32) * f).astype(np.int8), (mA.astype(np.int32) * f).astype(np.int8), q._replace(cb3f=hot, cbAf=hot)


def digest():
    """of everything the frozen records depend on"""
    h = hashlib.blake2b(digest_size=16)
    d = db()
    parts = [d.data3di, d.dataaa, d.offsets, d.lengths, *K.matrices()]
    for q in queries() + [sat_case()[2]]:
        parts += list(q)
    parts += [sat_case()[0], sat_case()[1], np.array(CONFIGS, np.int32)]
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes()); h.update(b"|")
    return h.hexdigest()


def live_records(cfg, qi, ids=None):
    """sw_model's forward records of query qi against the targets `ids` (None: all) under a configuration"""
    atype, go, ge = cfg
    m3, mA = matrices(atype)
    q = queries()[qi]
    ts = targets()
    if ids is not None:
        ts = [ts[int(i)] for i in ids]
    return sm.align(m3, mA, q.q3, q.qa, q.cb3f, q.cbAf, False, [t[0] for t in ts], [t[1] for t in ts], go, ge)


def live_sat(ids=None):
    m3, mA, q = sat_case()
    ts = targets()
    if ids is not None:
        ts = [ts[int(i)] for i in ids]
    return sm.align(m3, mA, q.q3, q.qa, q.cb3f, q.cbAf, False, [t[0] for t in ts], [t[1] for t in ts], 10, 1)


@functools.lru_cache(maxsize=None)
def frozen():
    z = np.load(ANSWERS)
    if str(z["digest"]) != digest():
        raise KeyError("tests/golden/scan_v1/answers.npz was made for other inputs: run tests/golden/make_scan_golden.py")
    return {k: z[k] for k in z.files}


def records(cfg):
    """[queries][N] records of a configuration (frozen)"""
    a = frozen()[config_name(cfg)]
    return [np.ascontiguousarray(a[i]).view(sm.REC_DT).reshape(-1) for i in range(a.shape[0])]


def sat_records():
    return np.ascontiguousarray(frozen()["sat"]).view(sm.REC_DT).reshape(-1)


def cutoffs(recs):
    """the five cutoffs of one query from its N model records: 0; a score that occurs (the second largest distinct one, so that something survives
    score + 1 too) and that score + 1; the median; 32767"""
    s = recs["score"].astype(np.int64)
    distinct = np.unique(s)
    occurs = int(distinct[-2]) if len(distinct) > 1 else int(distinct[-1])
    return {"zero": 0, "occurs": min(occurs, 32767), "occurs+1": min(occurs + 1, 32767), "median": int(min(np.median(s), 32767)), "max": 32767}


def expected(recs, cutoff):
    """(ids ascending, records) of the pairs with score >= cutoff"""
    ids = np.flatnonzero(recs["score"] >= cutoff).astype(np.uint32)
    return ids, recs[ids.astype(np.int64)]


def api_queries(atype, qs=None):
    """the query tuples Context.sw_scan_c takes"""
    aa = atype == 2
    return [(q.qa if aa else None, q.q3, q.cbAf if aa else None, q.cb3f, q.cbAr if aa else None, q.cb3r) for q in (qs if qs is not None else queries())]


def longest_first(d=None):
    """all ids, longest first, equal lengths by ascending id: the order the scan runs the targets in"""
    d = d or db()
    return np.array(sorted(range(d.n), key=lambda i: (-int(d.lengths[i]), i)), np.uint32)


# ---- more targets than a selection chunk holds: short targets, one short query, the model live (a second or so) --------------------------------------
@functools.lru_cache(maxsize=None)
def wide_db():
    rng = np.random.default_rng(99)
    lens = rng.integers(0, 13, 2 * 4096 + 811)
    return K.pack([(rng.integers(0, 20, int(L)).astype(np.uint8), rng.integers(0, 20, int(L)).astype(np.uint8), "wide") for L in lens])


def wide_query():
    return K.make_query(33, 4242, "random")


@functools.lru_cache(maxsize=None)
def wide_records():
    m3, mA = K.matrices()
    q, d = wide_query(), wide_db()
    ts = [K.target(d, i) for i in range(d.n)]
    return sm.align(m3, mA, q.q3, q.qa, q.cb3f, q.cbAf, False, [t[0] for t in ts], [t[1] for t in ts], 10, 1)

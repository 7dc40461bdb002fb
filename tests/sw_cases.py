"""tests/sw_cases.py -- the seeded inputs of the Smith-Waterman model tests and the model's frozen answers for them (TEST INFRASTRUCTURE: of the project only
synth.PaddedDB, a plain container, is used; nothing is read outside tests/golden).

One small database, the query lists and target lists of every section of tests/test_sw3_model_gpu.py are built here from seeds, as plain data
("calls"), so that the generator tests/golden/make_sw_golden.py, the CPU test of the model and the GPU tests all see the same inputs.  tests/sw_model.py
needs about 0.1 ms per target column and query, too slow to run live in every GPU test: its records are frozen in tests/golden/sw_v1/answers.npz, keyed by
a digest of everything a record depends on (matrices, query codes, the direction's biases, direction, gap costs, target codes).  A pair whose inputs
changed has no frozen answer and the lookup raises; tests/test_sw_model.py re-runs the live model on every ninth frozen pair and on whole sections.
"""
import collections
import functools
import hashlib
import os

import numpy as np

import sw_model as sm
from foldseek_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "sw_v1")
ANSWERS = os.path.join(GOLD, "answers.npz")

Query = collections.namedtuple("Query", "q3 qa cb3f cbAf cb3r cbAr")
# one compact call: the environment that picks the shapes, the matrices (mA None: 3Di only), queries, target ids per query, directions to run
Call = collections.namedtuple("Call", "name env m3 mA queries ids dirs go ge db")

LENGTHS = [1, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 130, 255, 256, 257, 511, 512, 513, 895, 896, 897, 1025, 1300,
           7, 23, 100, 191, 377]                 # the last five: "a few random ones", drawn once and written down
ENV_16 = {"FSGPU_SW3_MID": "896", "FSGPU_SW3_SHORT": "0"}          # the short-list rule off: lists of a dozen pairs would all take 64 lanes
ENV_32 = {"FSGPU_SW3_MID": "0", "FSGPU_SW3_SHORT": "0"}
ENV_AUTO = {}
GAPS = ((8, 2), (15, 3), (3, 1), (2, 1))


@functools.lru_cache(maxsize=None)
def matrices():
    """(3Di at bit factor 2.1, BLOSUM62 at 1.4) as int8 [21, 21]: the structurealign defaults, read from the frozen reference fixture"""
    g = np.load(os.path.join(HERE, "golden", "hotpath_v1.npz"))
    return (np.ascontiguousarray(g["sub_mat3di_2.1"].reshape(21, 21).astype(np.int8)), np.ascontiguousarray(g["sub_blosum62_1.4"].reshape(21, 21).astype(np.int8)))


@functools.lru_cache(maxsize=None)
def _master():
    rng = np.random.default_rng(20261018)
    return rng.integers(0, 20, 1500).astype(np.uint8), rng.integers(0, 20, 1500).astype(np.uint8)


def low_complexity(rng, n, variant):
    """homopolymer / two-letter string / tandem repeat of period 2..7"""
    if variant % 3 == 0:
        return np.full(n, rng.integers(0, 20), np.uint8)
    if variant % 3 == 1:
        return rng.choice(rng.choice(20, size=2, replace=False), size=n).astype(np.uint8)
    unit = rng.integers(0, 20, int(rng.integers(2, 8)))
    return np.resize(unit, n).astype(np.uint8)


def make_query(L, seed, kind="related", bias=3):
    """related: the first L residues of the master sequence, one in twenty redrawn, an X somewhere; low: low complexity; random.  Biases in -bias..bias."""
    rng = np.random.default_rng(seed)
    if kind == "related":
        q3, qa = (m[:L].copy() for m in _master())
        redraw = rng.random(L) < 0.05
        q3[redraw] = rng.integers(0, 20, int(redraw.sum())); qa[redraw] = rng.integers(0, 20, int(redraw.sum()))
        if L > 4:
            q3[rng.integers(0, L)] = 20
    elif kind == "low":
        v = int(rng.integers(0, 3))
        q3, qa = low_complexity(rng, L, v), low_complexity(rng, L, v + 1)
    else:
        q3, qa = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
    cb = [rng.integers(-bias, bias + 1, L).astype(np.int8) for _ in range(4)]
    return Query(q3, qa, *cb)


def _derived(rng, L):
    """a relative of the master's start, exactly L residues: one residue in ten substituted, one to three indels of 1..40 residues"""
    out = []
    for m in _master():
        s = m[:L + 130].copy()
        out.append(s)
    sub = rng.random(L + 130) < 0.1
    for s in out:
        s[sub] = rng.integers(0, 20, int(sub.sum()))
    for _ in range(int(rng.integers(1, 4))):
        n, at = int(rng.integers(1, 41)), int(rng.integers(0, max(1, L)))
        if rng.random() < 0.5:
            out = [np.concatenate([s[:at], s[at + n:]]) for s in out]
        else:
            ins = [rng.integers(0, 20, n).astype(np.uint8) for _ in out]
            out = [np.concatenate([s[:at], i, s[at:]]) for s, i in zip(out, ins)]
    return [np.ascontiguousarray(s[:L]) for s in out]


def pack(entries):
    """[(3Di codes, AA codes, kind)] -> PaddedDB (ascending length, padded to multiples of 4 with X) with .kind per entry"""
    order = sorted(range(len(entries)), key=lambda k: len(entries[k][0]))
    entries = [entries[k] for k in order]
    lens = np.array([len(e[0]) for e in entries], np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
    for k, (t3, ta, _) in enumerate(entries):
        d3[off[k]:off[k] + lens[k]] = t3
        da[off[k]:off[k] + lens[k]] = ta
    db = synth.PaddedDB(d3, da, off, lens)
    db.kind = [e[2] for e in entries]
    return db


@functools.lru_cache(maxsize=None)
def main_db():
    """every length of LENGTHS three times: random, a relative of the queries' master sequence, low complexity; an all-X and an entirely soft-masked
    target; X at both ends of every tenth"""
    rng = np.random.default_rng(4711)
    entries = []
    for kind in ("random", "derived", "low"):
        for k, L in enumerate(LENGTHS):
            if kind == "random":
                t3, ta = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
            elif kind == "derived":
                t3, ta = _derived(rng, L)
            else:
                t3, ta = low_complexity(rng, L, k), low_complexity(rng, L, k + 1)
            if k % 10 == 3 and L >= 3:
                t3[0] = t3[-1] = 20; ta[0] = ta[-1] = 20
            entries.append((t3, ta, kind))
    entries.append((np.full(40, 20, np.uint8), np.full(40, 20, np.uint8), "allX"))
    entries.append((rng.integers(0, 20, 50).astype(np.uint8) + 32, rng.integers(0, 20, 50).astype(np.uint8), "masked"))
    return pack(entries)


@functools.lru_cache(maxsize=None)
def tiny_db():
    """the database of test_gpu_parity.py::test_ragged_and_tiny_database"""
    rng = np.random.default_rng(4)
    lens = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89]
    entries = [[rng.integers(0, 20, l).astype(np.uint8), rng.integers(0, 20, l).astype(np.uint8), "random"] for l in lens]
    entries[5][0][:] = 20
    entries[6][0] += 32
    return pack([tuple(e) for e in entries])


DBS = {"main": main_db, "tiny": tiny_db}


def target(db, i):
    """(3Di, AA) codes of entry i as the aligner reads them: soft-masking removed"""
    o, l = int(db.offsets[i]), int(db.lengths[i])
    t3, ta = db.data3di[o:o + l], db.dataaa[o:o + l]
    return np.where(t3 >= 32, t3 - 32, t3).astype(np.uint8), np.where(ta >= 32, ta - 32, ta).astype(np.uint8)


def ids_where(db, lo=1, hi=1 << 30, kind=None):
    return np.array([i for i in range(db.n) if lo <= db.lengths[i] <= hi and (kind is None or db.kind[i] == kind)], np.uint32)


def first_of_length(db, L, kind="random"):
    return int(ids_where(db, L, L, kind)[0])


# ---- the model's answers: frozen, or live for the generator ------------------------------------------------------------------------------------------
_STORE = None
LIVE = False          # the generator and the live checks set this: a pair without a frozen answer is computed instead of refused
LOG = None            # a list: every lookup is appended as (digest, m3, mA, query, reverse, go, ge, t3, tA)


def store():
    global _STORE
    if _STORE is None:
        _STORE = {}
        if os.path.exists(ANSWERS):
            z = np.load(ANSWERS)
            _STORE = {int(k): r for k, r in zip(z["keys"], z["recs"])}
    return _STORE


def save_store():
    os.makedirs(GOLD, exist_ok=True)
    keys = np.array(sorted(store()), np.uint64)
    np.savez_compressed(ANSWERS, keys=keys, recs=np.array([store()[int(k)] for k in keys], np.int32).reshape(-1, 4))


def _query_hash(m3, mA, q, reverse, go, ge):
    h = hashlib.blake2b(digest_size=8)
    cb3, cbA = (q.cb3r, q.cbAr) if reverse else (q.cb3f, q.cbAf)
    zeros = np.zeros(len(q.q3), np.int8)
    parts = [np.ascontiguousarray(m3, np.int8), q.q3, zeros if cb3 is None else cb3, np.array([int(reverse), go, ge, len(q.q3)], np.int32)]
    if mA is not None:
        parts += [np.ascontiguousarray(mA, np.int8), q.qa, zeros if cbA is None else cbA]
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes()); h.update(b"|")
    return h


def want(m3, mA, q, reverse, targets, go=10, ge=1):
    """the model's records of one query in one direction against targets = [(3Di codes, AA codes)]"""
    st = store()
    qh = _query_hash(m3, mA, q, reverse, go, ge)
    digs = []
    for t3, ta in targets:
        h = qh.copy()
        h.update(np.ascontiguousarray(t3, np.uint8).tobytes())
        if mA is not None:
            h.update(b"|"); h.update(np.ascontiguousarray(ta, np.uint8).tobytes())
        digs.append(int.from_bytes(h.digest(), "little"))
    if LOG is not None:
        LOG.extend((d, m3, mA, q, reverse, go, ge, t[0], t[1]) for d, t in zip(digs, targets))
    miss = [k for k, d in enumerate(digs) if d not in st]
    if miss:
        if not LIVE:
            raise KeyError(f"{len(miss)} pairs without a frozen model answer: run tests/golden/make_sw_golden.py")
        recs = live(m3, mA, q, reverse, [targets[k] for k in miss], go, ge)
        for k, r in zip(miss, recs):
            st[digs[k]] = np.array([r["score"], r["qEnd"], r["dbEnd"], r["word"]], np.int32)
    out = np.zeros(len(digs), sm.REC_DT)
    for k, d in enumerate(digs):
        out[k] = tuple(int(v) for v in st[d])
    return out


def live(m3, mA, q, reverse, targets, go=10, ge=1):
    cb3, cbA = (q.cb3r, q.cbAr) if reverse else (q.cb3f, q.cbAf)
    return sm.align(m3, mA, q.q3, q.qa, cb3, cbA, reverse, [t[0] for t in targets], [t[1] for t in targets], go, ge)


def call_want(call, direction):
    """model records per query of a call"""
    db = DBS[call.db]()
    return [want(call.m3, call.mA, q, bool(direction), [target(db, int(i)) for i in ids], call.go, call.ge) for q, ids in zip(call.queries, call.ids)]


def api_queries(call):
    """the query tuples Context.sw_multi_dir_c takes"""
    aa = call.mA is not None
    return [(q.qa if aa else None, q.q3, q.cbAf if aa else None, q.cb3f, q.cbAr if aa else None, q.cb3r, np.asarray(ids, np.uint32)) for q, ids in zip(call.queries, call.ids)]


# ---- the planner's documented rules, written down a second time (fsgpu_sw3_multi.hip: the comment above sw3SortAndSplit; k_sw3.hpp: the LDS layout) ----
def expected_split(call, selections=None):
    """{16: pairs, 32: pairs, 64: pairs, 'profile': pairs, 'classes': {16: set of R, 32: ..., 64: ...}} of a call under its environment"""
    db = DBS[call.db]()
    mid_env = call.env.get("FSGPU_SW3_MID")
    mid = int(mid_env) if mid_env is not None else 512
    short = int(call.env.get("FSGPU_SW3_SHORT", 16))
    lists = [np.asarray(ids)[np.asarray(selections[k], np.int64)] if selections is not None else np.asarray(ids) for k, ids in enumerate(call.ids)]
    out = {16: 0, 32: 0, 64: 0, "profile": 0, "classes": {16: set(), 32: set(), 64: set()}}
    compact = [(q, ids) for q, ids in zip(call.queries, lists) if len(q.q3) <= 1024]
    out["profile"] = sum(len(ids) for q, ids in zip(call.queries, lists) if len(q.q3) > 1024)
    total = sum(len(ids) for _, ids in compact)
    active = sum(1 for _, ids in compact if len(ids))
    call_short = short > 0 and active > 0 and total <= short * active
    for q, ids in compact:
        L, ns = len(q.q3), len(ids)
        if ns == 0:
            continue
        lt = db.lengths[np.asarray(ids, np.int64)]
        n_long = ns if (L > 512 or call_short) else int((lt > 896).sum())
        shape16 = L <= 384 and mid > 0 and (mid_env is not None or total >= 100000)
        n_mid = 0 if n_long == ns else int(((lt > mid) & (lt <= 896)).sum()) if shape16 else ns - n_long
        for hl, n in ((64, n_long), (32, n_mid), (16, ns - n_long - n_mid)):
            if n:
                out[hl] += n
                out["classes"][hl].add((L + hl - 1) // hl)
    return out


def _dw(R):
    return (R + 1) // 2


def lds_bytes(R, HL, has_aa, waves):
    """dynamic LDS of a workgroup: one direction's image (22 profile rows per table; per row 16-byte planes of HL lanes, an 8-byte remainder plane of
    max(HL, 32) lanes or a 4-byte one of 64), then one ring of target columns per target pair, aligned to its size"""
    planes16 = _dw(R) // 4 + (1 if _dw(R) % 4 == 3 else 0)
    row = planes16 * HL * 16 + (max(HL, 32) * 8 if _dw(R) % 4 == 2 else 0) + (256 if _dw(R) % 4 == 1 else 0)
    img = (2 if has_aa else 1) * 22 * row
    ring = (64 if HL < 32 else 2 * HL) * (16 if has_aa else 8)
    return (img + ring - 1) // ring * ring + waves * (64 // HL) * ring


def pairs_per_wave(HL):
    return 2 * (64 // HL)


def pairs_per_workgroup(R, HL, has_aa):
    """four waves where three such workgroups fit the 160 KB of LDS of a compute unit, eight otherwise"""
    waves = 4 if (160 * 1024) // lds_bytes(R, HL, has_aa, 4) >= 3 else 8
    return waves * pairs_per_wave(HL)


# ---- section (a): every class of every shape --------------------------------------------------------------------------------------------------------
def _class_length(HL, R):
    """alternately the bottom of the class (most padding) and its top (none): both occur for every ceil(R / 2) % 4"""
    return HL * R if ((R - 1) // 2 + R) % 2 == 0 else HL * (R - 1) + 1


@functools.lru_cache(maxsize=None)
def class_queries():
    """{setting: [Query]}: 16 lanes R = 1..24, 32 lanes R = 1..16, 64 lanes R = 1..8 (short lists) and 9..16; every third query low-complexity"""
    out = {}
    for name, HL, Rs in (("16", 16, range(1, 25)), ("32", 32, range(1, 17)), ("64", 64, range(1, 17))):
        out[name] = [make_query(_class_length(HL, R), 1000 * HL + R, "low" if R % 3 == 0 else "related") for R in Rs]
    return out


def _relative(db, q, rng, cap):
    """the query's relative: the target derived from the master sequence that is nearest to its length, at most cap columns"""
    cand = ids_where(db, 1, cap, "derived")
    return int(cand[np.argmin(np.abs(db.lengths[cand].astype(np.int64) - len(q.q3)))])


def _lists(db, queries, seed, n=12, hi=257, cap=896):
    rng = np.random.default_rng(seed)
    pool = ids_where(db, 1, hi)
    out = []
    for q in queries:
        ids = list(rng.choice(pool, size=n, replace=False))
        rel = _relative(db, q, rng, cap)
        if rel not in ids:
            ids.append(rel)
        out.append(np.array(ids, np.uint32))
    return out


@functools.lru_cache(maxsize=None)
def section_a():
    db, (m3, mA) = main_db(), matrices()
    calls = []
    for name, env, cap in (("16", ENV_16, 896), ("32", ENV_32, 896), ("64", ENV_AUTO, 1300)):
        qs = class_queries()[name]
        ids = _lists(db, qs, 77 + len(qs), cap=cap)
        for aa in (True, False):
            calls.append(Call(f"a/{name}/{'aa' if aa else '3di'}", env, m3, mA if aa else None, qs, ids, (0, 1), 10, 1, "main"))
    return calls


A_CLASSES = {"16": (16, set(range(1, 25))), "32": (32, set(range(1, 17))), "64": (64, set(range(1, 17)))}


# ---- section (b): wave and workgroup packing --------------------------------------------------------------------------------------------------------
B_CLASSES = (("16", ENV_16, 16, 100), ("32", ENV_32, 32, 200), ("64", ENV_AUTO, 64, 600))


@functools.lru_cache(maxsize=None)
def section_b():
    """per shape one query length with lists of 1, 2, 3, ppw - 1, ppw, ppw + 1, ppb, ppb + 1 pairs (one query each: a list is cut into workgroups by
    itself); then, under the automatic rule, every target of the database in one list; then two-pair lists of the longest target a shape takes and a
    1-column one"""
    db, (m3, mA) = main_db(), matrices()
    rng = np.random.default_rng(808)
    calls = []
    for name, env, HL, L in B_CLASSES:
        R = (L + HL - 1) // HL
        ppw, ppb = pairs_per_wave(HL), pairs_per_workgroup(R, HL, True)
        q = make_query(L, 5000 + HL, "related")
        pool = ids_where(db, 1, 896)
        sizes = [1, 2, 3, ppw - 1, ppw, ppw + 1, ppb, ppb + 1]
        ids = [rng.choice(pool, size=n, replace=False).astype(np.uint32) for n in sizes]
        calls.append(Call(f"b/{name}", env, m3, mA, [q] * len(sizes), ids, (0, 1), 10, 1, "main"))
    q = make_query(200, 5999, "related")
    calls.append(Call("b/every length", ENV_AUTO, m3, mA, [q], [np.arange(db.n, dtype=np.uint32)], (0, 1), 10, 1, "main"))
    # a call of its own each, so that both targets take ONE shape and, longest first, the two int16 halves of one register
    for name, env, long_ in (("64", ENV_AUTO, 1300), ("32", ENV_32, 896), ("16", ENV_16, 896)):       # 64 lanes: by the short-list rule (2 <= 16 * 1)
        two = np.array([first_of_length(db, 1), first_of_length(db, long_)], np.uint32)
        calls.append(Call(f"b/{long_} with 1 column/{name}", env, m3, mA, [q], [two], (0, 1), 10, 1, "main"))
    return calls


# ---- section (c): the split's boundaries ------------------------------------------------------------------------------------------------------------
C_QUERY_LENGTHS = (384, 385, 512, 513, 1024, 1025)
C_TARGET_LENGTHS = (512, 513, 896, 897)


@functools.lru_cache(maxsize=None)
def section_c():
    """the boundary targets plus 13 short ones per query (17 pairs: the short-list rule stays out of the first three settings), then lists of 16 -- the
    call holds exactly 16 pairs per active query -- and one pair more"""
    db, (m3, mA) = main_db(), matrices()
    rng = np.random.default_rng(33)
    qs = [make_query(L, 7000 + L, "related") for L in C_QUERY_LENGTHS]
    edge = [first_of_length(db, L, "derived") for L in C_TARGET_LENGTHS]
    pool = np.setdiff1d(ids_where(db, 1, 257), edge)
    extra = [rng.choice(pool, size=13, replace=False) for _ in qs]
    ids17 = [np.array(edge + list(e), np.uint32) for e in extra]
    ids16 = [x[:16] for x in ids17]
    ids16p = [x[:16] for x in ids17[:-2]] + [ids17[-2][:17], ids17[-1][:16]]          # one pair more, in the last compact query
    calls = [Call("c/auto", ENV_AUTO, m3, mA, qs, ids17, (0, 1), 10, 1, "main"),
             Call("c/mid512", {"FSGPU_SW3_MID": "512"}, m3, mA, qs, ids17, (0, 1), 10, 1, "main"),
             Call("c/mid896 short0", ENV_16, m3, mA, qs, ids17, (0, 1), 10, 1, "main"),
             Call("c/16 per query", ENV_AUTO, m3, mA, qs, ids16, (0,), 10, 1, "main"),
             Call("c/16 per query + 1", ENV_AUTO, m3, mA, qs, ids16p, (0,), 10, 1, "main")]
    return calls


# ---- section (d): image reuse -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def section_d():
    """{step name: Call}; all under the 32-lane setting, so that a target of 897 columns needs a shape (64 lanes) the short lists did not build"""
    db, (m3, mA) = main_db(), matrices()
    rng = np.random.default_rng(99)
    qs = [make_query(L, 9000 + L, kind) for L, kind in ((60, "related"), (200, "low"), (380, "related"), (600, "related"))]
    pool = ids_where(db, 1, 257)
    short = [rng.choice(pool, size=6, replace=False).astype(np.uint32) for _ in qs]
    long_ = [np.concatenate([s[:3], ids_where(db, 897, 897)[:2]]).astype(np.uint32) for s in short]
    mk = lambda name, queries, ids, dirs, m3_=m3, mA_=mA: Call("d/" + name, ENV_32, m3_, mA_, queries, ids, dirs, 10, 1, "main")
    steps = {"short": mk("short", qs, short, (0,)), "long": mk("long", qs, long_, (1,))}
    cb = qs[1].cb3f.copy(); cb[17] = 100                    # one bias byte of one query
    steps["bias"] = mk("bias", [qs[0], qs[1]._replace(cb3f=cb), qs[2], qs[3]], short, (0,))
    letter = int(np.bincount(qs[2].qa, minlength=21)[:20].argmax())
    mA2 = mA.copy(); mA2[letter, letter] += 20              # one entry of the AA matrix
    steps["matrix"] = mk("matrix", qs, short, (0,), m3, mA2)
    steps["3di"] = mk("3di", qs, short, (0,), m3, None)
    steps["swapped"] = mk("swapped", [qs[0], qs[2], qs[1], qs[3]], [short[0], short[2], short[1], short[3]], (0,))
    return steps


# ---- section (e): saturation ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def section_e():
    db, (m3, mA) = main_db(), matrices()
    rng = np.random.default_rng(55)
    L = 400
    q = make_query(L, 555, "random")
    hot, zero = np.full(L, 100, np.int8), np.zeros(L, np.int8)
    ids = np.concatenate([ids_where(db, 255, 257, "random"), ids_where(db, 511, 513, "low"), ids_where(db, 897, 897, "random"), ids_where(db, 1300, 1300, "derived")]).astype(np.uint32)
    one = Call("e/forward only", ENV_AUTO, m3, mA, [q._replace(cb3f=hot, cbAf=hot, cb3r=zero, cbAr=zero)], [ids], (0, 1), 10, 1, "main")
    mixed = np.concatenate([ids, ids_where(db, 1, 3, "random"), ids_where(db, 63, 65, "random")]).astype(np.uint32)
    both = Call("e/all +100", ENV_AUTO, m3, mA, [q._replace(cb3f=hot, cbAf=hot, cb3r=hot, cbAr=hot)], [mixed], (0, 1), 10, 1, "main")
    return one, both


@functools.lru_cache(maxsize=None)
def exact_32767():
    """217 matching positions of 151 each: 60 + 60 on the diagonals of both matrices, biases 15 and 16, every mismatch -100 -- a homopolymer query of 217
    rows against a homopolymer target of 217 columns reaches 217 * 151 = 32767 = INT16_MAX with no addition clipped.  Returns (m3, mA, query, t3, tA)."""
    m = np.full((21, 21), -100, np.int8)
    m[np.arange(21), np.arange(21)] = 60
    q = Query(np.full(217, 7, np.uint8), np.full(217, 11, np.uint8), np.full(217, 15, np.int8), np.full(217, 16, np.int8), np.full(217, 15, np.int8), np.full(217, 16, np.int8))
    return m, m.copy(), q, np.full(217, 7, np.uint8), np.full(217, 11, np.uint8)


@functools.lru_cache(maxsize=None)
def exact_db():
    """that homopolymer target and a random one of 30 residues"""
    rng = np.random.default_rng(1)
    _, _, _, t3, tA = exact_32767()
    return pack([(t3, tA, "homopolymer"), (rng.integers(0, 20, 30).astype(np.uint8), rng.integers(0, 20, 30).astype(np.uint8), "random")])


# ---- section (f): score zero and tiny inputs --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def section_f():
    db, (m3, mA) = main_db(), matrices()
    rng = np.random.default_rng(66)
    allx = Query(np.full(70, 20, np.uint8), np.full(70, 20, np.uint8), *[np.zeros(70, np.int8) for _ in range(4)])
    qs = [allx, make_query(1, 1, "random"), make_query(1, 2, "random", bias=0), make_query(45, 3, "random"), make_query(130, 4, "related")]
    special = [i for i in range(db.n) if db.kind[i] in ("allX", "masked")]
    ids = [np.array(special + list(rng.choice(ids_where(db, 1, 130), size=8, replace=False)), np.uint32) for _ in qs]
    calls = [Call(f"f/main/{n}", env, m3, mA, qs, ids, (0, 1), 10, 1, "main") for n, env in (("16", ENV_16), ("32", ENV_32), ("64", ENV_AUTO))]
    tq = [make_query(45, 45, "random"), make_query(1, 46, "random"), make_query(13, 47, "low")]
    tids = [np.arange(tiny_db().n, dtype=np.uint32)] * len(tq)
    calls += [Call(f"f/tiny/{n}", env, m3, mA, tq, tids, (0, 1), 10, 1, "tiny") for n, env in (("16", ENV_16), ("32", ENV_32), ("64", ENV_AUTO))]
    return calls


# ---- section (g): the siblings ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def section_g():
    """the AA calls of (a), and six classes (two per shape) under the other gap costs"""
    base = [c for c in section_a() if c.mA is not None]
    gaps = []
    for c in base:
        pick = [1, len(c.queries) - 2]
        for go, ge in GAPS:
            gaps.append(c._replace(name=f"g/{c.name}/{go}-{ge}", queries=[c.queries[k] for k in pick], ids=[c.ids[k] for k in pick], go=go, ge=ge))
    return base, gaps


def all_calls():
    calls = list(section_a()) + list(section_b()) + list(section_c())
    d = section_d()
    calls += [d[k] for k in ("short", "long", "bias", "matrix", "3di", "swapped")]
    calls += list(section_e()) + list(section_f()) + list(section_g()[1])
    return calls


def live_sections():
    """(c) to (f): re-run live in full by tests/test_sw_model.py"""
    d = section_d()
    return list(section_c()) + [d[k] for k in d] + list(section_e()) + list(section_f())

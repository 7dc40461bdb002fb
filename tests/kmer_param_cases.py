"""tests/kmer_param_cases.py -- the seeded inputs of the k-mer index-parameter tests (TEST INFRASTRUCTURE: of the project only foldseek_amd.synth, a
generator, is used, and the test-only C oracle through kmer_lib; nothing is read outside the repository).

fsgpu_kmer_index_build takes five parameters (include/fsgpu.h, fsgpu_kmer_index_params).  The other k-mer tests vary kmerThr alone; here one small
database, one set of queries and the index settings of SETTINGS are built for the CPU test of the checkers (tests/test_kmer_params_model.py: the C
oracle against the compiled reference at EVERY setting, and counted conditions that keep the axes from being vacuous) and the device tests
(tests/test_kmer_params_gpu.py).

The database is 600 seeded targets of 4 .. 300 residues with runs (stay = 0.4), soft-masked stretches (10 %) and 20 planted homologs per query, and
behind them hand-made targets, each with a name in World.ids:

* win5 .. win11: 5 .. 11 residues of query WINDOW_QUERY from its residue WINDOW_AT on.  Two k-mer starts on one diagonal need 7 residues with
  contiguous k-mers and 11 with the spaced pattern 1101010011: win7 .. win10 can be hits only under spaced = 0, win5 never, win11 under both.
* runs: per repeat limit n of RUN_LIMITS two targets with runs of a non-zero letter of exactly n (kept under maskNrepeats = n) and n + 1 (masked) at
  position 0, in the middle and at the end; a run of n + 1 that continues across a plain / soft-masked border (codes c and c + 32: the repeat rule
  compares unmasked codes, so it is ONE run); a run of 8 of code 0 at position 0 (never masked: Masker.cpp:83-115 starts with previousChar = 0 and
  startOfRepeat = -1) and the same run in the middle (masked); a run of X.  World.runs lists every one as (id, start, length, leading code 0?), so a
  test can say for any setting which of them must be X.
* softhom: 40 residues of query 1 between unrelated letters, the +32 flags laid over the whole copy: a hit only with maskLowerCase = 0.

Queries: the four full queries, prefixes of 0, 5, 6, 7, 9, 10 and 11 residues of query WINDOW_QUERY, an all-X query and a database member that carries
soft-mask flags, searched with its own id as identity."""
import collections
import functools

import numpy as np

import helpers as H
import kmer_lib as K
from foldseek_amd import synth

N_SEEDED = 600
WINDOW_QUERY = 0
WINDOW_AT = 20                          # not 0: a first match on diagonal 0 meets the zeroed byte of findDuplicates and counts as a second one
WINDOWS = (5, 6, 7, 8, 9, 10, 11)
PREFIXES = (0, 5, 6, 7, 9, 10, 11)
RUN_LIMITS = (1, 2, 6, 50)              # 50: a limit no seeded target reaches, so that maskNrepeats = 50 and 0 differ by the hand-made runs alone
X = 20

# index settings: oracle / reference parameter names (kmer_lib.default_params); all k = 6
SETTINGS = collections.OrderedDict([
    ("default", dict()),
    ("contiguous", dict(spaced=0)),
    ("nomasklc", dict(maskLowerCase=0)),
    ("rep0", dict(maskNrepeats=0)),
    ("rep1", dict(maskNrepeats=1)),
    ("rep2", dict(maskNrepeats=2)),
    ("rep50", dict(maskNrepeats=50)),
    ("alloff", dict(spaced=0, maskLowerCase=0, maskNrepeats=0)),
    ("contiguous_thr110", dict(spaced=0, kmerThr=110)),
])
NAMES = tuple(SETTINGS)


def index_params(name):
    """the five index parameters of a setting, defaults filled in"""
    p = dict(kmerSize=6, spaced=1, kmerThr=78, maskLowerCase=1, maskNrepeats=6)
    p.update(SETTINGS[name])
    return p


# search settings per index: oracle parameter names.  `refill`: maxDbMatches comes from REFILL_MATCHES (small enough for databaseHits refills at
# that setting's index: the lists of maskNrepeats = 1 hold a tenth of the default's entries)
SEARCHES = collections.OrderedDict([
    ("defaults", dict(maxResListLen=1000, minDiagScoreThr=30, maxDbMatches=0, noDiagScore=0)),
    ("refill", dict(maxResListLen=50, minDiagScoreThr=30, noDiagScore=0)),
    ("scoreonly", dict(maxResListLen=100, minDiagScoreThr=0, maxDbMatches=0, noDiagScore=1)),
])
REFILL_MATCHES = dict(default=2000, contiguous=2000, nomasklc=2000, rep0=2000, rep1=300, rep2=800, rep50=2000, alloff=2000, contiguous_thr110=400)


def search_params(setting, search):
    p = dict(bins=0, foundDiagonalsSize=0, compBias=1)
    p.update(SEARCHES[search])
    if search == "refill":
        p["maxDbMatches"] = REFILL_MATCHES[setting]
    return p


Run = collections.namedtuple("Run", "id start length leading_zero")
World = collections.namedtuple("World", "db targets q3 qa queries queries_aa identity ids runs qnames")


def _filler(rng, n, avoid):
    """n letters of 1 .. 19 without `avoid`, no two neighbours equal: nothing in it is a repeat at any limit"""
    out, prev = [], avoid
    for _ in range(n):
        c = int(rng.integers(1, 20))
        while c == prev or c == avoid:
            c = int(rng.integers(1, 20))
        out.append(c); prev = c
    return out


def _run_targets(rng, n, ids, runs, entries):
    """the two run targets of limit n and its border target"""
    c = 3 + RUN_LIMITS.index(n)                                   # a non-zero letter per limit
    for which, lens in (("a", (n, n + 1, n)), ("b", (n + 1, n, n + 1))):
        t, tid = [], len(entries)
        for k, r in enumerate(lens):
            if k:
                t += _filler(rng, 14, c)
            runs.append(Run(tid, len(t), r, False))
            t += [c] * r
        ids[f"run{n}{which}"] = tid
        entries.append(np.array(t, np.uint8))
    # n + 1 residues of one letter, the first `plain` of them plain and the others soft-masked: neither part alone passes the limit
    plain = (n + 2) // 2
    tid = len(entries)
    head = _filler(rng, 14, c)
    t = head + [c] * plain + [c + 32] * (n + 1 - plain) + _filler(rng, 14, c)
    runs.append(Run(tid, len(head), n + 1, False))
    ids[f"border{n}"] = tid
    entries.append(np.array(t, np.uint8))


def _padded(entries3, entriesa):
    lens = np.array([len(e) for e in entries3], np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3 = np.full(int(off[-1]), X, np.uint8); da = np.full(int(off[-1]), X, np.uint8)
    for e3, ea, o in zip(entries3, entriesa, off[:-1]):
        d3[o:o + len(e3)] = e3; da[o:o + len(ea)] = ea
    return synth.PaddedDB(d3, da, off, lens)


@functools.lru_cache(maxsize=None)
def world():
    q3, qa = synth.make_queries(4, seed=3, mean_len=120, lo=30, hi=300)
    seeded = synth.make_db(N_SEEDED, (q3, qa), seed=5, homologs_per_query=20, mask_frac=0.1, mean_len=80, lo=4, hi=300, stay=0.4)
    e3 = [seeded.seq(i, "3di", unmask=False).copy() for i in range(seeded.n)]
    ea = [seeded.seq(i, "aa", unmask=False).copy() for i in range(seeded.n)]
    rng = np.random.default_rng(20261019)
    ids, runs = {}, []
    wq = q3[WINDOW_QUERY]
    for w in WINDOWS:
        ids[f"win{w}"] = len(e3)
        e3.append(wq[WINDOW_AT:WINDOW_AT + w].copy())
    for n in RUN_LIMITS:
        _run_targets(rng, n, ids, runs, e3)
    # code 0: a leading run (never masked) and the same run in the middle
    head = [0] * 8
    t = head + _filler(rng, 14, 0)
    runs.append(Run(len(e3), 0, 8, True)); runs.append(Run(len(e3), len(t), 8, False))
    ids["zero"] = len(e3)
    e3.append(np.array(t + [0] * 8 + _filler(rng, 14, 0), np.uint8))
    # a run of X
    ids["xrun"] = len(e3)
    e3.append(np.array(_filler(rng, 14, X) + [X] * 8 + _filler(rng, 14, X), np.uint8))
    # the soft-masked homolog
    piece = q3[1][10:50]
    ids["softhom"] = len(e3)
    e3.append(np.concatenate([np.array(_filler(rng, 20, X), np.uint8), piece + 32, np.array(_filler(rng, 20, X), np.uint8)]).astype(np.uint8))
    while len(ea) < len(e3):
        ea.append(rng.integers(0, 20, len(e3[len(ea)])).astype(np.uint8))
    db = _padded(e3, ea)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    member = next(i for i in range(N_SEEDED) if (targets[i] >= 32).any() and len(targets[i]) > 100)
    queries = list(q3) + [wq[:k].copy() for k in PREFIXES] + [np.full(40, X, np.uint8), targets[member].copy()]
    qnames = [f"full{i}" for i in range(4)] + [f"prefix{k}" for k in PREFIXES] + ["allx", "member"]
    queries_aa = list(qa) + [qa[WINDOW_QUERY][:k].copy() for k in PREFIXES] + [np.full(40, X, np.uint8), db.seq(member, "aa").copy()]
    identity = np.full(len(queries), -1, np.int64)
    identity[-1] = member
    ids["member"] = member
    return World(db, targets, q3, qa, queries, queries_aa, identity, ids, tuple(runs), tuple(qnames))


@functools.lru_cache(maxsize=None)
def matrices():
    """(k-mer matrix at 8 bits, background, ungapped matrix at 2 bits) as the oracle builds them"""
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    return ksub, pb, usub


def make_oracle(name):
    """kmer_lib.OraKpf over the targets with the index parameters of a setting (the caller closes it)"""
    ksub, pb, usub = matrices()
    return K.OraKpf(K.load_ora(), ksub, pb, usub, world().targets, **SETTINGS[name])


def oracle_answers(o, setting, search):
    """[(hits, statistics, refills)] of every query at one search setting; the query without residues is not put to the oracle (hits None)"""
    w = world()
    o.set(**search_params(setting, search))
    out = []
    for q, ident in zip(w.queries, w.identity):
        if len(q) == 0:
            out.append((None, None, 0))
            continue
        r, st = o.query(q, int(ident))
        assert o.last_rc >= 0, (setting, search, "the unmodelled std::sort branch")
        out.append((r, st, o.last_refills))
    return out


def run_masked(run, maskNrepeats):
    """whether the repeat rule turns a listed run into X at a limit (0: the rule is off)"""
    return maskNrepeats > 0 and run.length > maskNrepeats and not run.leading_zero

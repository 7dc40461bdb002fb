"""tests/tm_cases.py -- the TM-score fixtures of tests/golden/tm_v1 (generator: tests/golden/make_tm_golden.py) as Python objects, the seeded task lists the
GPU tests run, and the model's raw answers for all of them (TEST INFRASTRUCTURE: no project code in here).

The model (tests/tm_model.py) needs 0.01 - 1 s per task, so its answers for the fixed task lists below are computed ONCE, by the generator, and frozen next to
the reference's outputs as uint32 arrays [tasks, 4] = (pairs, bits of score_max of standard_TMscore's search, of detailed_search_standard's, of the rmsd):
model_fixture_raw.npy, model_corpus_raw.npy, model_edge_raw.npy.  test_tm_model.py runs the LIVE model on the whole fixture list (every
field the reference printed, every threshold decision) and on a spread sample of the corpus and edge lists, so the frozen answers cannot drift from it.
"""
import functools
import json
import os

import numpy as np

import lddt_cases as K
import lddt_model as M
import tm_model as T

ROOT = K.ROOT
GOLD = os.path.join(ROOT, "tests", "golden", "tm_v1")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json"))) if os.path.exists(os.path.join(GOLD, "MANIFEST.json")) else {}


def read_db(name):
    """{key: entry bytes without the terminator} of a DB frozen in tm_v1"""
    data = open(os.path.join(GOLD, name), "rb").read()
    out = {}
    for line in open(os.path.join(GOLD, name + ".index")):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def result_records(path_reader, name):
    """[(query key, [fields])] of a result DB, queries in key order, records in file order"""
    out = []
    for q, entry in sorted(path_reader(name).items()):
        for line in entry.decode().splitlines():
            out.append((q, line.split("\t")))
    return out


def norm_lengths(qs, ts, bt, q_len, t_len):
    """the normalisation lengths of alntmscore / qtmscore / ttmscore = --tmscore-threshold-mode 0 / 1 / 2"""
    qe = qs + sum(ch in "MI" for ch in bt) - 1
    te = ts + sum(ch in "MD" for ch in bt) - 1
    return min(qe - qs, te - ts), q_len, t_len


@functools.lru_cache(maxsize=None)
def crafted_coords():
    L = {int(l.split()[0]): int(l.split()[2]) - 2 for l in open(os.path.join(GOLD, "tmdb.index"))}
    return {k: M.decode(e, L[k]) for k, e in read_db("tmdb_ca").items()}


def crafted_records():
    """[(query key, target key, qStart, dbStart, cigar)] of the crafted alignment DB in the order convertalis prints them"""
    return [(q, int(c[0]), int(c[4]), int(c[7]), c[10]) for q, c in result_records(read_db, "tmaln")]


@functools.lru_cache(maxsize=None)
def fixture_tasks():
    """-> (coords list, tasks): the 144 pairs of ca_v1's aln_l0 and the crafted records, each with its three normalisation lengths, in the order of the
    frozen .m8 files (task 3 * r + m = record r, mode m).  tasks: (query index, target index, qStart, dbStart, backtrace, normLen)"""
    coords, tasks = [], []
    for C, recs in ((K.coords("db"), K.records("aln_l0")), (crafted_coords(), crafted_records())):
        keys = sorted(C)
        base = len(coords)
        coords += [C[k] for k in keys]
        for q, t, qs, ts, cig in recs:
            bt = M.expand(cig)
            for nl in norm_lengths(qs, ts, bt, C[q].shape[1], C[t].shape[1]):
                tasks.append((base + keys.index(q), base + keys.index(t), qs, ts, bt, nl))
    return coords, tasks


# ---- seeded synthetic tasks -------------------------------------------------------------------------------------------------------------------------
def _walk(rng, L, step=3.8):
    v = rng.normal(size=(L, 3))
    v = v / np.linalg.norm(v, axis=1)[:, None] * step
    return np.ascontiguousarray(np.cumsum(v, axis=0).T, np.float32)


def _backtrace(rng, n_m, gaps=True, head="", tail=""):
    """n_m aligned columns with short I / D runs sprinkled in between"""
    out = [head]
    for k in range(n_m):
        out.append("M")
        if gaps and k + 1 < n_m and rng.random() < 0.06:
            out.append(("I", "D")[int(rng.integers(2))] * int(rng.integers(1, 4)))
    out.append(tail)
    return "".join(out)


def _rotation(rng):
    q = rng.normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _fit(rng, bt, q_start, t_start):
    """a query and a target just long enough for the backtrace from the given start cells, with a few residues behind its end.  The target is the query's
    ALIGNED residues under a random rigid motion plus noise (small, medium, large, or large on a tail only), or an unrelated walk"""
    nq = q_start + sum(ch in "MI" for ch in bt) + int(rng.integers(0, 5))
    nt = t_start + sum(ch != "I" for ch in bt) + int(rng.integers(0, 5))
    q, t = _walk(rng, max(nq, 1)), _walk(rng, max(nt, 1))
    kind = int(rng.integers(0, 6))
    if kind < 5:
        R, shift = _rotation(rng), rng.normal(scale=20.0, size=(3, 1))
        qi, ti = q_start, t_start
        for k, ch in enumerate(bt):
            if ch == "M":
                p = R @ q[:, qi].astype(np.float64)[:, None] + shift
                scale = (0.3, 1.5, 4.0, 0.0, 1.0)[kind]
                if kind == 4 and k > len(bt) * 0.6:
                    scale = 8.0
                t[:, ti] = (p[:, 0] + rng.normal(scale=scale, size=3)).astype(np.float32)
                qi += 1; ti += 1
            elif ch == "I":
                qi += 1
            else:
                ti += 1
    return q, t


CORPUS_COUNTS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 39, 40, 41, 63, 64, 65, 79, 80, 81, 127, 128, 129, 159, 160, 161]


@functools.lru_cache(maxsize=None)
def corpus():
    """-> (queries, targets, tasks): 66 tasks of every pair count of CORPUS_COUNTS and 30 of about 300 pairs, every task on coordinates of its own"""
    rng = np.random.default_rng(20261018)
    queries, targets, tasks = [], [], []
    counts = CORPUS_COUNTS * 66 + [int(v) for v in rng.integers(290, 311, 30)]
    for n in counts:
        head = ("", "II", "D", "IDD")[int(rng.integers(0, 4))] if rng.random() < 0.3 else ""
        bt = _backtrace(rng, n, rng.random() < 0.7, head, "")
        qs, ts = (0, 0) if rng.random() < 0.3 else (int(rng.integers(0, 9)), int(rng.integers(0, 9)))
        q, t = _fit(rng, bt, qs, ts)
        nl = norm_lengths(qs, ts, bt, q.shape[1], t.shape[1])[int(rng.integers(0, 3))]
        queries.append(q); targets.append(t)
        tasks.append((len(queries) - 1, len(targets) - 1, qs, ts, bt, nl))
    return queries, targets, tasks


LDS_PAIRS = 1024          # kTmLdsPairs of k_tm.hpp: hits with more pairs keep their pairs and masks in global memory


@functools.lru_cache(maxsize=None)
def edge():
    """-> (queries, targets, tasks): one hit AT the LDS limit and one just past it (with gaps, start cells > 0), then 60 short hits that share one query
    and one target (different windows, all three normalisations)"""
    rng = np.random.default_rng(20261019)
    queries, targets, tasks = [], [], []
    for n in (LDS_PAIRS, LDS_PAIRS + 1):
        bt = _backtrace(rng, n, True, "I", "")
        q, t = _fit(rng, bt, 2, 3)
        queries.append(q); targets.append(t)
        tasks.append((len(queries) - 1, len(targets) - 1, 2, 3, bt, q.shape[1]))
    bt = "M" * 200
    q, t = _fit(rng, bt, 0, 0)
    queries.append(q); targets.append(t)
    for k in range(60):
        n = int(rng.integers(5, 45))
        qs = int(rng.integers(0, 150))
        sub = _backtrace(rng, n, True)
        sub = sub[:min(len(sub), 45)]
        ts = min(max(qs + int(rng.integers(-3, 4)), 0), 150)
        tasks.append((2, 2, qs, ts, sub, norm_lengths(qs, ts, sub, q.shape[1], t.shape[1])[k % 3]))
    return queries, targets, tasks


def model_raw(coords_q, coords_t, tasks, only=None):
    """the live model on a task list -> uint32 [tasks, 4]; only: indices to compute (the other rows stay 0)"""
    out = np.zeros((len(tasks), 4), np.uint32)
    for k, (q, t, qs, ts, bt, nl) in enumerate(tasks):
        if only is not None and k not in only:
            continue
        xtm, ytm = T.pairs(coords_q[q], coords_t[t], qs, ts, bt)
        n, s1, s2, rmsd = T.tm_raw(xtm, ytm, nl)
        out[k] = (n, np.float32(s1).view(np.uint32), np.float32(s2).view(np.uint32), np.float32(rmsd).view(np.uint32))
    return out


@functools.lru_cache(maxsize=None)
def live_fixture_raw():
    """the live model on every fixture task, once per test session"""
    coords, tasks = fixture_tasks()
    return model_raw(coords, coords, tasks)


def frozen_raw(which):
    return np.load(os.path.join(GOLD, f"model_{which}_raw.npy"))


def raw_of_device(res):
    """what Context.tm_batch returns -> uint32 [tasks, 4]"""
    out = np.zeros((len(res), 4), np.uint32)
    for k, (n, s1, s2, rmsd) in enumerate(res):
        out[k] = (n, np.float32(s1).view(np.uint32), np.float32(s2).view(np.uint32), np.float32(rmsd).view(np.uint32))
    return out


def as_floats(row):
    return int(row[0]), row[1:2].view(np.float32)[0], row[2:3].view(np.float32)[0], row[3:4].view(np.float32)[0]


def text_fields(raw_rows, norm_lens):
    """the alntmscore / qtmscore / ttmscore / rmsd text of one record from its three raw rows"""
    out = []
    for row, nl in zip(raw_rows, norm_lens):
        n, s1, s2, _ = as_floats(row)
        out.append(T.sstr(T.tm_finish(n, s1, s2, nl)))
    out.append(T.sstr(float(as_floats(raw_rows[2])[3])))
    return out

"""tests/pbt_cases.py -- a seeded task set for fsgpu_profile_backtrace (start cell, identity count and M / I / D string of profile-query hits on the device:
k_pbtrace.hpp) and the frozen answers of the independent model for it: tests/profile_model.py's start_cell and banded_path (tests/golden/profile_bt_v1,
generator tests/golden/make_profile_bt_golden.py).  TEST INFRASTRUCTURE: nothing of the project is imported here; the GPU test
(tests/test_profile_backtrace_gpu.py) builds queries and targets from the seed, reads tasks and answers from the frozen files and never runs the model;
the CPU test (tests/test_profile_backtrace_cases.py) re-runs the live model on a sample and holds the frozen files to it.

The set:
* every pair of the tests/profile_cases.py world under gap costs 10 / 1 (its e_all set: forward records of all pairs) and the pairs of its gap8_2 set whose
  reversed score the reference looks at, under 8 / 2: the edge, xhead, xmid, longgap, row / col and slot kinds, the 1025-position query, the saturating list;
* one more query of 200 positions (rows 10 and 20 share their letters) and crafted targets, each under 10 / 1, 8 / 2 and 2 / 1:
    prefix     copies of the master's first 63, 64, 65, 127, 128, 129 positions: qEnd + 1 and the rectangle's height on both sides of the 64-lane chunk
    ins40/70   a stretch with 40 / 70 random residues inserted: first band 41 / 71, a band line of 83 / 143 cells (crosses 64 / 128)
    both12     the whole master with 12 residues deleted and 12 inserted further on: square, first band 1, the band doubles four times
    small8     the same in a 17 x 17 rectangle with 8 residues: the band grows until it is the rectangle
    masked     a mutated stretch whose database copy holds soft-masked codes (+ 32), codes 21 .. 31 and codes beyond 52 (all read as X by the aligner)
  and tasks that no forward pass hands out but the entry must answer like the source (the reverse pass is a LOCAL alignment from the end cell):
    one_by_n   [m, X, X, X, X] with the end cell on the last X: a 1 x 5 rectangle, the path runs along the row (MDDDD)
    n_by_one   the single residue m against rows 0 .. 24 of which 10 and 20 reach the score: a reverse-pass tie inside ONE column (the smallest reversed
               row wins: row 20), a 5 x 1 rectangle whose last column is the one the `edge` slot clears: with the quirk the trace-back fails (status 3)
    no_path    found by search over the query's tables (gap costs 2 / 1): a single column whose end cell came from the diagonal, so the trace-back leaves
               the rectangle with rows still to go -- banded_sw's "Trace back error": start cell, no path (status 3)
* for the named tasks the score raised by one: the reverse pass cannot reach it (status 2)."""
import functools
import json
import os

import numpy as np

import profile_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "profile_bt_v1")
SEED = 20261103
GAPS = ((10, 1), (8, 2), (2, 1))
CRAFT_L = 200
X = 20
PREFIXES = (63, 64, 65, 127, 128, 129)
TIE_ROWS = (10, 20)


def normalise(codes):
    """what the aligner reads for a database code: the soft-mask flag dropped, anything above 20 is X"""
    c = np.asarray(codes, np.uint8).astype(np.int64)
    c = np.where(c >= 32, c - 32, c)
    return np.where(c > 20, 20, c).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def world():
    """-> dict(entries [(AA entry, 3Di entry)], raw [(AA, 3Di)] database codes, targets [(AA, 3Di)] as the aligner reads them, kinds [str], craft_query,
    craft {name: target id}): the profile_cases world with the crafted query and targets appended"""
    w = K.world()
    rng = np.random.default_rng(SEED)
    m3, mA = K.matrices()
    qa, q3 = K._rand(rng, CRAFT_L)
    qa[TIE_ROWS[1]], q3[TIE_ROWS[1]] = qa[TIE_ROWS[0]], q3[TIE_ROWS[0]]
    entries = list(w["entries"]) + [(K._entry(rng, mA, qa), K._entry(rng, m3, q3))]
    raw, kinds, craft = list(w["targets"]), list(w["kinds"]), {}

    def add(name, a, s):
        raw.append((np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8))); kinds.append(name)
        craft[name] = len(raw) - 1

    for h in PREFIXES:
        add(f"prefix{h}", qa[:h], q3[:h])
    for g, lo, mid, hi in ((40, 20, 80, 140), (70, 10, 90, 170)):
        ia, is_ = K._rand(rng, g)
        add(f"ins{g}", np.concatenate([qa[lo:mid], ia, qa[mid:hi]]), np.concatenate([q3[lo:mid], is_, q3[mid:hi]]))
    ia, is_ = K._rand(rng, 12)
    add("both12", np.concatenate([qa[:60], qa[72:130], ia, qa[130:]]), np.concatenate([q3[:60], q3[72:130], is_, q3[130:]]))
    ia, is_ = K._rand(rng, 8)
    add("small8", np.concatenate([qa[100:104], qa[112:113], ia, qa[113:117]]), np.concatenate([q3[100:104], q3[112:113], is_, q3[113:117]]))
    a, s = qa[30:120].copy(), q3[30:120].copy()
    m = rng.random(len(a)) < 0.1
    a[m] = rng.integers(0, 20, int(m.sum())); s[m] = rng.integers(0, 20, int(m.sum()))
    a[5:40:7] += 32; s[8:60:9] += 32                       # soft-masked: the same letter
    a[50], s[50], a[51], s[52] = 25, 31, 60, 53            # X by value: 21 .. 31, and 32 + 21 .. : what is left after the flag is still above 20
    add("masked", a, s)
    r = TIE_ROWS[1]
    add("one_by_n", np.concatenate([qa[r:r + 1], np.full(4, X, np.uint8)]), np.concatenate([q3[r:r + 1], np.full(4, X, np.uint8)]))
    add("n_by_one", qa[r:r + 1], q3[r:r + 1])
    # every pair of letters as a one-residue target: what the no_path search picks from
    for x in range(20):
        for y in range(20):
            raw.append((np.array([x], np.uint8), np.array([y], np.uint8))); kinds.append("letter")
    craft["letters"] = len(raw) - 400
    targets = [(normalise(a), normalise(s)) for a, s in raw]
    return dict(entries=entries, raw=raw, targets=targets, kinds=kinds, craft_query=len(entries) - 1, craft=craft)


@functools.lru_cache(maxsize=None)
def tables(q):
    """(AA profile, 3Di profile) int8 [21, L] of query q and its AA query letters, by the model's decoder"""
    import profile_model as pm
    ea, e3 = world()["entries"][q]
    ca, _, aF, _ = pm.decode(ea)
    _, _, sF, _ = pm.decode(e3)
    return aF, sF, ca


def forward(q, t, go, ge):
    """the forward record (score, qEnd, dbEnd) of a pair, by the model"""
    import profile_model as pm
    aF, sF, _ = tables(q)
    ta, t3 = world()["targets"][t]
    r = pm.sw_records(sF, aF, [(t3, ta)], go, ge)[0]
    return int(r["score"]), int(r["qEnd"]), int(r["dbEnd"])


def find_no_path():
    """tasks (target, qEnd, dbEnd, score) under gap costs 2 / 1 on the crafted query against one-residue targets: the column's maximum s0 sits n - 1 >= 2
    rows above the end row, whose own score v is at least what the vertical gap brings down (s0 - 2 - (n - 2)) and below s0: the end cell of the n x 1
    rectangle comes from the diagonal, the trace-back steps to column -1 with rows to go.  (n = 2 is left out: there the source's loop ends and its identity count reads past the target.)"""
    w = world()
    q = w["craft_query"]
    aF, sF, _ = tables(q)
    M = aF.astype(np.int64)[:20][:, None, :] + sF.astype(np.int64)[None, :20, :]          # [AA letter, 3Di letter, row]
    out = []
    for r in range(0, 60):
        for n in (3, 4):
            end = r + n - 1
            for x in range(20):
                for y in range(20):
                    col = M[x, y, :end + 1]
                    s0, v = int(col[r]), int(col[end])
                    if s0 <= 0 or not (s0 - 2 - (n - 2) <= v < s0) or v <= 0:
                        continue
                    if (col[:r] >= s0).any() or (col[r + 1:end] >= s0 - 2).any():
                        continue
                    out.append((w["craft"]["letters"] + 20 * x + y, end, 0, s0))
                    break
                else:
                    continue
                break
    return out[:3]


def build_tasks():
    """-> (tasks int32 [n, 7]: query, target, qEnd, dbEnd, score, gapOpen, gapExtend; names [str])  (generator only: runs the model's forward pass)"""
    w, F = world(), K.Frozen()
    rows, names = [], []
    for q in range(len(F.n)):
        for k, t in enumerate(w_list(q)):
            sc, qe, de, _ = (int(x) for x in F.fwd("e_all", q)[k])
            rows.append((q, int(t), qe, de, sc, 10, 1)); names.append(w["kinds"][int(t)])
            if F.rev("gap8_2", q)[k][3] != 0:
                sc, qe, de, _ = (int(x) for x in F.fwd("gap8_2", q)[k])
                rows.append((q, int(t), qe, de, sc, 8, 2)); names.append(w["kinds"][int(t)] + "/8-2")
    cq = w["craft_query"]
    aF, sF, _ = tables(cq)
    r = TIE_ROWS[1]
    peak = int(aF[w["targets"][w["craft"]["n_by_one"]][0][0], r]) + int(sF[w["targets"][w["craft"]["n_by_one"]][1][0], r])
    for go, ge in GAPS:
        for name, t in w["craft"].items():
            if name in ("letters", "one_by_n", "n_by_one"):
                continue
            sc, qe, de = forward(cq, t, go, ge)
            rows.append((cq, t, qe, de, sc, go, ge)); names.append(f"{name}/{go}-{ge}")
            if name in ("prefix64", "both12", "masked"):
                rows.append((cq, t, qe, de, sc + 1, go, ge)); names.append(f"{name}/{go}-{ge}/raised")
        rows.append((cq, w["craft"]["one_by_n"], r, 4, peak, go, ge)); names.append(f"one_by_n/{go}-{ge}")
        rows.append((cq, w["craft"]["n_by_one"], r + 4, 0, peak, go, ge)); names.append(f"n_by_one/{go}-{ge}")
    for t, qe, de, sc in find_no_path():
        rows.append((cq, t, qe, de, sc, 2, 1)); names.append("no_path/2-1")
    # a hit of the world with its score raised
    first = next(i for i, n in enumerate(names) if n == "piece")
    rows.append(rows[first][:4] + (rows[first][4] + 1,) + rows[first][5:]); names.append("piece/raised")
    return np.array(rows, np.int32), names


def w_list(q):
    return K.world()["lists"][q]


def reverse_ties(q, t, q_end, db_end, score, go, ge):
    """cells of the first reversed column that reaches the score which hold it (plain integers, every cell: small prefixes only)"""
    aF, sF, _ = tables(q)
    ta, t3 = world()["targets"][t]
    s = (sF.astype(np.int64)[:, :q_end + 1][t3[:db_end + 1].astype(np.int64)].T + aF.astype(np.int64)[:, :q_end + 1][ta[:db_end + 1].astype(np.int64)].T)[::-1, ::-1]
    n, m = s.shape
    up_h, up_e = [0] * n, [0] * n                          # per row: H and the horizontal gap state of the previous column
    for j in range(m):
        col, f, above, diag_src = [0] * n, 0, 0, 0
        for i in range(n):
            e = max(up_h[i] - go, up_e[i] - ge) if j else 0
            f = max(above - go, f - ge) if i else 0
            h = max(0, (diag_src if i and j else 0) + int(s[i, j]), e, f)
            diag_src = up_h[i]
            up_e[i] = e
            col[i] = above = h
        up_h = col
        if max(col) >= score:
            return sum(1 for x in col if x == max(col))
    return 0


def answer(task):
    """the model's answer: dict(status, qStart, dbStart, ids, band, doublings, path, edge_differs)"""
    import profile_model as pm
    q, t, q_end, db_end, score, go, ge = (int(x) for x in task)
    aF, sF, letters = tables(q)
    ta, t3 = world()["targets"][t]
    out = dict(status=2, qStart=-1, dbStart=-1, ids=0, band=0, doublings=0, path="", edge_differs=False)
    try:
        qs, ds = pm.start_cell(sF, aF, t3, ta, q_end, db_end, score, go, ge)
    except AssertionError:
        return out
    tt3, tta = t3[ds:db_end + 1].astype(np.int64), ta[ds:db_end + 1].astype(np.int64)
    match = sF.astype(np.int64)[:, qs:q_end + 1][tt3].T + aF.astype(np.int64)[:, qs:q_end + 1][tta].T
    q_len, db_len = q_end - qs + 1, db_end - ds + 1
    widths = []
    path = pm.banded_path(match, q_len, db_len, score, go, ge, doublings=widths)
    out.update(status=3, qStart=qs, dbStart=ds, doublings=len(widths), band=(abs(db_len - q_len) + 1) << len(widths))
    out["edge_differs"] = pm.banded_path(match, q_len, db_len, score, go, ge, edge_slot=False) != path
    if path is None:
        return out
    qp, tp, ids = qs, ds, 0
    for op in path:
        if op == "M":
            ids += int(ta[tp]) == int(letters[qp]); qp += 1; tp += 1
        elif op == "I":
            qp += 1
        else:
            tp += 1
    assert (qp, tp) == (q_end + 1, db_end + 1), (task, path)
    out.update(status=1, ids=ids, path=path)
    return out


# ---- the frozen files ---------------------------------------------------------------------------------------------------------------------------------------------
def save(tasks, names, answers, ties):
    os.makedirs(GOLD, exist_ok=True)
    ans = np.array([[a["status"], a["qStart"], a["dbStart"], a["ids"], a["band"], a["doublings"], int(a["edge_differs"]), ties[k]] for k, a in enumerate(answers)], np.int32)
    np.savez_compressed(os.path.join(GOLD, "tasks.npz"), tasks=tasks, answers=ans, paths=np.frombuffer("\n".join(a["path"] for a in answers).encode(), np.uint8))
    json.dump(dict(seed=SEED, world_seed=K.SEED, names=names), open(os.path.join(GOLD, "names.json"), "w"), indent=0)


class Frozen:
    def __init__(self):
        j = json.load(open(os.path.join(GOLD, "names.json")))
        assert j["seed"] == SEED and j["world_seed"] == K.SEED, "the world changed: run tests/golden/make_profile_bt_golden.py"
        z = np.load(os.path.join(GOLD, "tasks.npz"))
        self.names = j["names"]
        self.tasks, self.ans = z["tasks"], z["answers"]
        self.paths = bytes(z["paths"]).decode().split("\n")
        assert len(self.names) == len(self.tasks) == len(self.ans) == len(self.paths)

    def answer(self, k):
        a = self.ans[k]
        return dict(status=int(a[0]), qStart=int(a[1]), dbStart=int(a[2]), ids=int(a[3]), band=int(a[4]), doublings=int(a[5]), path=self.paths[k],
                    edge_differs=bool(a[6]))

    def by_gaps(self):
        """{(gapOpen, gapExtend): [task indices]}: one device call takes one pair of gap costs"""
        out = {}
        for k, t in enumerate(self.tasks):
            out.setdefault((int(t[5]), int(t[6])), []).append(k)
        return out


def conditions(F):
    """what keeps the set honest; asserted by the generator on what it wrote and by tests/test_profile_backtrace_cases.py on the frozen files"""
    w = world()
    st = F.ans[:, 0]
    assert (st == 1).sum() >= 200 and (st == 2).sum() >= 4 and (st == 3).sum() >= 1, np.bincount(st)          # the model CAN produce a status 3: no_path
    assert all(F.names[k].endswith("raised") for k in np.flatnonzero(st == 2))
    assert {F.names[k].split("/")[0] for k in np.flatnonzero(st == 3)} == {"no_path", "n_by_one"}
    assert F.ans[:, 6].sum() >= 1, "no rectangle whose path the edge slot decides"
    assert (F.ans[:, 5] > 0).sum() >= 5, "band doublings"
    assert (F.ans[:, 7] > 1).sum() >= 1, "no reverse-pass tie inside one column"
    ok = np.flatnonzero(st == 1)
    q_len = F.tasks[ok, 2] - F.ans[ok, 1] + 1
    db_len = F.tasks[ok, 3] - F.ans[ok, 2] + 1
    shapes = set(zip(q_len.tolist(), db_len.tolist()))
    assert (1, 1) in shapes and any(a == 1 and b > 1 for a, b in shapes)
    # n x 1: a single column is the last column, which the edge slot clears in every row above: no vertical gap survives and the model finds no path
    tall = [k for k in np.flatnonzero(st == 3) if F.tasks[k, 3] - F.ans[k, 2] == 0 and F.tasks[k, 2] - F.ans[k, 1] >= 2]
    assert tall and all(F.ans[k, 6] for k in tall if F.names[k].startswith("n_by_one"))
    assert set(PREFIXES) <= set(q_len.tolist()) and set(PREFIXES) <= set((F.tasks[ok, 2] + 1).tolist())
    line = np.minimum(2 * F.ans[ok, 4] + 1, db_len)
    assert ((line > 64) & (line <= 128)).any() and (line > 128).any(), "band lines beyond one and two 64-lane chunks"
    assert (F.tasks[:, 2] + 1 == 1025).any() and (F.tasks[ok, 2] + 1 > 1024).any(), "the 1025-position query, and a prefix beyond the LDS line"
    assert (db_len > 1024).any() and (q_len > 1024).any(), "a band line beyond the LDS line"
    square = (np.abs(q_len - db_len) <= 1) & (F.ans[ok, 5] >= 3)
    assert square.any(), "a near-square rectangle whose band doubles three times"
    whole = (F.ans[ok, 5] > 0) & (2 * F.ans[ok, 4] + 1 >= db_len)
    assert whole.any(), "a band that grows to the rectangle"
    masked = w["craft"]["masked"]
    assert (w["raw"][masked][0] >= 32).any() and ((w["raw"][masked][0] > 20) & (w["raw"][masked][0] < 32)).any() and (F.tasks[ok, 1] == masked).any()
    assert {(10, 1), (8, 2), (2, 1)} <= set(F.by_gaps())
    kinds = {F.names[k] for k in ok}
    assert {"edge", "xhead", "xmid", "longgap", "row", "col", "slot", "identity", "piece"} <= kinds, kinds

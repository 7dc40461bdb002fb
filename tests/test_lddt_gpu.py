"""fsgpu_lddt_batch (k_lddt_norm + k_lddt_pairs) called directly through Context.lddt_batch against the independent float32 model (tests/lddt_model.py, itself held
to the reference binary's output by tests/test_lddt_model.py): alignLength and every per-column value, compared with float BIT equality (a NaN column is a
NaN column; its payload is not read by anything).  There is no host path behind the entry that could recompute a value."""
import numpy as np
import pytest

import lddt_cases as K
import lddt_model as M
from foldseek_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _check(got, want_cols, what=""):
    assert len(got) == len(want_cols)
    for k, ((n, cols), want) in enumerate(zip(got, want_cols)):
        assert n == len(want), f"{what} task {k}: alignLength {n}, model {len(want)}"
        assert K.same_bits(cols, want), f"{what} task {k}: first differing column {np.flatnonzero(~((cols == want) | (np.isnan(cols) & np.isnan(want))))[:5]}"


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


def _fit(rng, bt, q_start, t_start):
    """a query and a target just long enough for the backtrace from the given start cells, with a few residues behind its end"""
    nq = q_start + sum(ch in "MI" for ch in bt) + int(rng.integers(0, 5))
    nt = t_start + sum(ch in "MD" for ch in bt) + int(rng.integers(0, 5))
    q = _walk(rng, max(nq, 1))
    t = _walk(rng, max(nt, 1))
    m = min(q.shape[1], t.shape[1])
    t[:, :m] = q[:, :m] + rng.normal(scale=1.2, size=(3, m)).astype(np.float32)      # a perturbed copy: every quarter count occurs
    return q, t


def test_all_fixture_pairs_in_one_call(ctx):
    """the 144 pairs of the 12 example structures (compressed entries) and the 14 crafted records (raw-float entry, NaN columns, exact cutoffs, fused-vs-unfused
    pairs) as ONE call; the coordinates come from fshost_ca_decode"""
    queries, targets, tasks, want = [], [], [], []
    for db, aln in (("db", "aln_l0"), ("cdb", "caln")):
        L, entries = K.lengths(db), K.read_db(db + "_ca")
        keys = sorted(entries)
        base = len(queries)
        for k in keys:
            c = api.ca_decode(entries[k], L[k])
            queries.append(c)
            targets.append(c)
        for q, t, qs, ts, cig in K.records(aln):
            tasks.append((base + keys.index(q), base + keys.index(t), qs, ts, M.expand(cig)))
        want += K.model_columns(db, aln)
    assert len(tasks) == 144 + 14
    _check(ctx.lddt_batch(queries, targets, tasks), want, "fixtures")


def test_synthetic_lengths_gaps_offsets_and_shared_targets(ctx):
    """alignment lengths around the wave (64) and the workgroup (256), backtraces that begin and end with I / D runs, start cells > 0, a query of one residue,
    two tasks on one target; then an EMPTY call and a SMALLER call on the same context (stale workspace, stale lengths)"""
    rng = np.random.default_rng(20251018)
    queries, targets, tasks = [], [], []
    for n_m in (1, 2, 63, 64, 65, 255, 256, 257):
        bt = _backtrace(rng, n_m)
        qs, ts = (0, 0) if n_m in (1, 64) else (int(rng.integers(1, 9)), int(rng.integers(1, 9)))
        q, t = _fit(rng, bt, qs, ts)
        queries.append(q); targets.append(t)
        tasks.append((len(queries) - 1, len(targets) - 1, qs, ts, bt))
    for head, tail in (("III", "DD"), ("DDDD", "I"), ("IID", "DII"), ("D", "")):
        bt = _backtrace(rng, 40, True, head, tail)
        qs, ts = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        q, t = _fit(rng, bt, qs, ts)
        queries.append(q); targets.append(t)
        tasks.append((len(queries) - 1, len(targets) - 1, qs, ts, bt))
    # a query of one residue: its only column has no neighbour
    queries.append(_walk(rng, 1))
    tasks.append((len(queries) - 1, 2, 0, 3, "M"))
    # two more tasks on target 5 (and one of them on another query's coordinates)
    tasks.append((5, 5, 2, 7, "M" * 30 + "DD" + "M" * 20))
    tasks.append((6, 5, 0, 0, "II" + "M" * 100))
    want = [M.columns(queries[q], targets[t], qs, ts, bt) for q, t, qs, ts, bt in tasks]
    assert np.isnan(want[12]).all() and len(want[12]) == 1
    _check(ctx.lddt_batch(queries, targets, tasks), want, "synthetic")
    assert ctx.lddt_batch(queries, targets, []) == []
    assert ctx.lddt_batch([], [], []) == []
    small = [tasks[3], tasks[9], tasks[1]]
    _check(ctx.lddt_batch(queries, targets, small), [want[3], want[9], want[1]], "second, smaller call")


def test_alignment_longer_than_an_lds_tile(ctx):
    """4 500 aligned columns: more than four LDS tiles of k_lddt_pairs and 18 column blocks per workgroup, next to a short task in the same call"""
    rng = np.random.default_rng(7)
    bt = _backtrace(rng, 4500, True, "II", "D")
    q, t = _fit(rng, bt, 3, 5)
    tasks = [(0, 0, 0, 0, "M" * 10), (0, 0, 3, 5, bt)]
    want = [M.columns(q, t, qs, ts, b) for _, _, qs, ts, b in tasks]
    assert len(want[1]) == 4500
    _check(ctx.lddt_batch([q], [t], tasks), want, "long")


def test_bad_tasks_are_refused_not_run(ctx):
    """a backtrace that runs past a sequence end, a start cell outside the sequence: an error from the entry, nothing launched"""
    rng = np.random.default_rng(3)
    q, t = _walk(rng, 20), _walk(rng, 20)
    for task in ((0, 0, 0, 0, "M" * 21), (0, 0, 5, 0, "M" * 16), (0, 0, 0, 18, "MMD"), (0, 0, -1, 0, "M")):
        with pytest.raises(api.FsgpuError):
            ctx.lddt_batch([q], [t], [task])
    _check(ctx.lddt_batch([q], [t], [(0, 0, 0, 0, "M" * 20)]), [M.columns(q, t, 0, 0, "M" * 20)], "after refusals")

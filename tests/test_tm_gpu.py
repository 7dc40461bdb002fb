"""fsgpu_tm_batch (k_tm_pairs + k_tm_search) called directly through Context.tm_batch against the independent model (tests/tm_model.py, itself held to the
reference binary's output by the fixture generator and tests/test_tm_model.py): the pair count, the raw score_max of both searches and the rmsd, compared as
float BIT patterns.  The model's answers for the fixed task lists are frozen (tests/tm_cases.py); there is no host path behind the entry that could
recompute a value.

Tolerated: on the seeded corpus at most 2 tasks may differ, and those must still print the same %.3E text.  The only operations whose results cannot be
argued from IEEE rules are the double-precision atan2 / cos / sin of the eigen step (device library here, glibc in the model and the reference); a
last-place difference there survives the cast to float only rarely.  The fixture tasks allow no difference."""
import numpy as np
import pytest

import tm_cases as TC
import tm_model as T
from foldseek_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _differing(got, want):
    return [k for k in range(len(want)) if got[k].tobytes() != want[k].tobytes()]


def _describe(k, task, got, want):
    return f"task {k} (pairs {want[0]}, normLen {task[5]}): device {TC.as_floats(got)} model {TC.as_floats(want)}"


def test_all_fixture_tasks_in_one_call(ctx):
    """the 144 pairs of the 12 example structures and the crafted records, each with its three normalisations, as ONE call: zero mismatches"""
    coords, tasks = TC.fixture_tasks()
    want = TC.frozen_raw("fixture")
    assert len(tasks) == len(want) == 3 * (144 + len(TC.crafted_records()))
    got = TC.raw_of_device(ctx.tm_batch(coords, coords, tasks))
    bad = _differing(got, want)
    for k in bad:
        print(_describe(k, tasks[k], got[k], want[k]))
    assert not bad
    assert ctx.kernel_ms(16) >= 0 and ctx.kernel_ms(17) > 0


def test_seeded_corpus(ctx):
    """2 010 tasks: 66 of every pair count 1-9, 15-17, 31-33, 39-41, 63-65, 79-81, 127-129, 159-161 and 30 of about 300, gaps, start cells, random rigid
    motions, noise from 0 to unrelated"""
    queries, targets, tasks = TC.corpus()
    want = TC.frozen_raw("corpus")
    assert len(tasks) == len(want) >= 2000
    got = TC.raw_of_device(ctx.tm_batch(queries, targets, tasks))
    assert (got[:, 0] == want[:, 0]).all()
    bad = _differing(got, want)
    for k in bad:
        print(_describe(k, tasks[k], got[k], want[k]))
    assert len(bad) <= 2
    for k in bad:
        g, w, nl = TC.as_floats(got[k]), TC.as_floats(want[k]), tasks[k][5]
        assert T.sstr(T.tm_finish(g[0], g[1], g[2], nl)) == T.sstr(T.tm_finish(w[0], w[1], w[2], nl))
        assert T.sstr(float(g[3])) == T.sstr(float(w[3]))


def test_lds_limit_shared_coordinates_and_growing_workspace(ctx):
    """a hit AT the LDS limit and one just past it (pairs and masks in global memory), 60 hits on one query and one target; called as a small batch
    first and then as a whole, so that the pair and mask workspaces grow between two calls on one context"""
    queries, targets, tasks = TC.edge()
    want = TC.frozen_raw("edge")
    assert [int(w[0]) for w in want[:2]] == [TC.LDS_PAIRS, TC.LDS_PAIRS + 1]
    small = tasks[2:12]
    got = TC.raw_of_device(ctx.tm_batch(queries, targets, small))
    assert not _differing(got, want[2:12])
    got = TC.raw_of_device(ctx.tm_batch(queries, targets, tasks))
    bad = _differing(got, want)
    for k in bad:
        print(_describe(k, tasks[k], got[k], want[k]))
    assert not bad
    got = TC.raw_of_device(ctx.tm_batch(queries, targets, small))          # and a smaller call again: stale workspace behind it
    assert not _differing(got, want[2:12])


def test_empty_call_and_zero_pair_task(ctx):
    rng = np.random.default_rng(11)
    q, t = TC._walk(rng, 20), TC._walk(rng, 20)
    assert ctx.tm_batch([q], [t], []) == []
    assert ctx.tm_batch([], [], []) == []
    res = ctx.tm_batch([q], [t], [(0, 0, 2, 3, "IIDDD", 20), (0, 0, 0, 0, "M" * 20, 20), (0, 0, 0, 0, "", 0)])
    for k in (0, 2):                                   # score_max keeps its initial -1, the rmsd its initial 0
        n, s1, s2, rmsd = res[k]
        assert (n, float(s1), float(s2), float(rmsd)) == (0, -1.0, -1.0, 0.0)
    xtm, ytm = T.pairs(q, t, 0, 0, "M" * 20)
    assert TC.raw_of_device(res[1:2]).tobytes() == TC.model_raw([q], [t], [(0, 0, 0, 0, "M" * 20, 20)]).tobytes()
    assert T.tm_finish(0, -1.0, -1.0, 20) == api.tm_finish(0, -1.0, -1.0, 20) == 0.0


def test_bad_tasks_are_refused_not_run(ctx):
    """a backtrace that runs past a sequence end (every character that is neither M nor I advances the target), a start cell outside the sequence, a
    query index out of range, a search parameter that is not a positive finite number: an error from the entry, nothing launched"""
    rng = np.random.default_rng(3)
    q, t = TC._walk(rng, 20), TC._walk(rng, 20)
    for task in ((0, 0, 0, 0, "M" * 21, 20), (0, 0, 5, 0, "M" * 16, 20), (0, 0, 0, 18, "MMD", 20), (0, 0, 0, 18, "MMX", 20), (0, 0, -1, 0, "M", 20),
                 (1, 0, 0, 0, "M", 20)):
        with pytest.raises(api.FsgpuError):
            ctx.tm_batch([q], [t], [task])
    # search parameters that fshost_tm_params cannot produce (they drive loops in the kernel): NaN, infinity, zero, negative
    good = [float(v) for v in api.tm_params(20)]
    for slot in range(4):
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            par = list(good)
            par[slot] = bad
            with pytest.raises(api.FsgpuError):
                ctx.tm_batch([q], [t], [(0, 0, 0, 0, "M" * 20, 20)], params=[par])
    got = TC.raw_of_device(ctx.tm_batch([q], [t], [(0, 0, 0, 0, "M" * 20, 20)]))
    assert got.tobytes() == TC.model_raw([q], [t], [(0, 0, 0, 0, "M" * 20, 20)]).tobytes()

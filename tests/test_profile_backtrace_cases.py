"""The task set of tests/pbt_cases.py and its frozen answers (tests/golden/profile_bt_v1), held to the live model on the CPU: the conditions that keep the set
honest, the tasks as the model's forward pass hands them out today, and the answers of start_cell / banded_path for a sample that holds every crafted
case.  The frozen answers are what tests/test_profile_backtrace_gpu.py holds fsgpu_profile_backtrace to."""
import functools

import numpy as np
import pytest

import pbt_cases as B


@functools.lru_cache(maxsize=None)
def frozen():
    return B.Frozen()


def test_conditions_of_the_set():
    """at least one rectangle whose path the edge slot decides, five whose band doubles, a reverse-pass tie inside one column, every status the model can
    produce -- 1, 2 (the score raised by one) and 3 (it can: a single-column rectangle of more than one row, pbt_cases.conditions says why) -- the shapes
    1 x 1, 1 x n and n x 1, heights and prefixes of 63 .. 129, band lines beyond 64 and 128 cells, lines beyond 1024 cells, a band that grows to its
    rectangle, masked and out-of-alphabet database codes, three pairs of gap costs"""
    B.conditions(frozen())


def test_the_tasks_are_what_the_model_hands_out():
    tasks, names = B.build_tasks()
    F = frozen()
    assert names == F.names and (tasks == F.tasks).all()


def _sample():
    F = frozen()
    crafted = [k for k, n in enumerate(F.names) if "/" in n and not n.endswith("/8-2")]
    rest = [k for k in range(len(F.names)) if k not in set(crafted)]
    return crafted + rest[::7]


@pytest.mark.parametrize("part", range(4))
def test_frozen_answers_are_the_live_models(part):
    F = frozen()
    for k in _sample()[part::4]:
        got, want = B.answer(F.tasks[k]), F.answer(k)
        assert got == want, (k, F.names[k], F.tasks[k].tolist())
        if want["status"] != 2 and (int(F.tasks[k][2]) + 1) * (int(F.tasks[k][3]) + 1) <= 5000:
            assert B.reverse_ties(*(int(x) for x in F.tasks[k])) == int(F.ans[k][7]), (k, F.names[k])


def test_database_codes_are_read_as_the_host_reads_them():
    raw = np.array([0, 19, 20, 21, 31, 32, 51, 52, 53, 60, 255], np.uint8)
    assert B.normalise(raw).tolist() == [0, 19, 20, 20, 20, 0, 19, 20, 20, 20, 20]


def test_the_entry_is_bound():
    from foldseek_amd import api
    assert {"fsgpu_profile_backtrace", "fsgpu_profile_backtrace_last"} <= set(api.exported_symbols())
    assert hasattr(api.Context, "profile_backtrace") and api.PbtQuery._fields_[3][0] == "L"

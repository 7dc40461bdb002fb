#!/usr/bin/env python3
"""tests/golden/make_profile_bt_golden.py -- writes tests/golden/profile_bt_v1 (TEST INFRASTRUCTURE): the task set of tests/pbt_cases.py and the answers
of tests/profile_model.py's start_cell and banded_path for it (status, start cell, identity count, final band width, M / I / D string), then asserts the
set's conditions (pbt_cases.conditions) on what it wrote.  Our own model's output: nothing of the reference goes in, and nothing outside the repository
is read.

usage: make_profile_bt_golden.py            (about a minute)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import pbt_cases as B  # noqa: E402


def main():
    tasks, names = B.build_tasks()
    answers, ties = [], []
    for k, t in enumerate(tasks):
        a = B.answer(t)
        answers.append(a)
        small = (int(t[2]) + 1) * (int(t[3]) + 1) <= 60000
        ties.append(B.reverse_ties(*(int(x) for x in t)) if a["status"] != 2 and small else 0)
        if k % 50 == 0:
            print(k, len(tasks), names[k], a["status"], a["band"], flush=True)
    B.save(tasks, names, answers, ties)
    B.conditions(B.Frozen())
    for f in sorted(os.listdir(B.GOLD)):
        print(f, os.path.getsize(os.path.join(B.GOLD, f)))


if __name__ == "__main__":
    main()

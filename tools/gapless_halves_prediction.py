#!/usr/bin/env python3
"""Host-only: the VALU wave-instructions per query k_gapless issues on the benchmark's database, before and after queries of the classes 17 .. 36
share registers two by two (k_gapless HALVES), and the records that run with a dead half.  Counted from the stripe table, the
queries' lengths and the pairing rule (fsgpu_gapless_pair_halves) alone, to set beside a `rocprofv3 --pmc SQ_INSTS_VALU` pass of the same bench.py
arguments.

Per stripe column a wave issues, for a query alone, R + R / 2 + 3 instructions in the unrolled body (R adds, R / 2 max3, row address, dpp move,
hand-off perm) and R + ceil(R / 2) + 3 + 5 in the last-chunk loop.  A HALVES record of class R runs every stripe column twice (slots 0..3, then
4..7) at one instruction less (no hand-off perm), whether its B is a query of the class, one moved up from a class below, or dead.
usage: gapless_halves_prediction.py [--targets N] [--steps K] [--warmup W] [--group G]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foldseek_amd import api, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--targets", type=int, default=1000000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--group", type=int, default=64)
ap.add_argument("--fullrange-steps", type=int, default=8)
ap.add_argument("--homologs", type=int, default=50)
ap.add_argument("--host-threads", type=int, default=3)
args = ap.parse_args()

G = args.group
n_timed, n_warm = args.steps * G, args.warmup * G
q3, qa = synth.make_queries(n_timed + n_warm, seed=1000, lo=250, hi=450)           # bench.py: timed queries first, then the warm-up ones
f3, fa = synth.make_queries(args.fullrange_steps * G, seed=3000, lo=30, hi=2000)   # planted in every run
db = synth.make_db_fast(args.targets, (q3 + f3, qa + fa), seed=20260923, homologs_per_query=args.homologs)
lens = np.sort(np.asarray(db.lengths, np.int64), kind="stable")
pad = (-len(lens)) % 8
mx = np.concatenate([lens, np.zeros(pad, np.int64)]).reshape(-1, 8).max(axis=1)
tail_cols = int((mx % 16).sum())                                                  # columns of the last-chunk loops
body_cols = int(mx.sum()) - tail_cols


def column_loop(R, other):
    """wave-instructions of one pass over every stripe: `other` = the instructions of a column that do not depend on R"""
    return body_cols * (R + R / 2.0 + other) + tail_cols * (R + (R + 1) // 2 + other + 5)


def pair(classes):
    cls = np.asarray(classes, np.int32)
    lc, rec, half = (np.zeros(len(cls), np.int32) for _ in range(3))
    assert api.lib().fsgpu_gapless_pair_halves(cls.ctypes.data, len(cls), lc.ctypes.data, rec.ctypes.data, half.ctypes.data) >= 0
    return lc, rec, half


def step_cost(batch):
    """(before, after, records, dead halves, moved up) of one multi-query call; classes up to 16 run two queries to a kernel of 2 R registers"""
    cls = [max(1, (L + 15) // 16) for L in batch]
    lc, rec, half = pair(cls)
    before = after = 0.0
    count = {}
    for R in cls:
        count[R] = count.get(R, 0) + 1
    for R, m in count.items():
        short = (R <= 16 and m >= 2)
        alone = m * column_loop(R, 3) if not short else (m // 2) * column_loop(2 * R, 3) + (m % 2) * column_loop(R, 3)
        before += alone
        if not any(r >= 0 for r, c in zip(rec, cls) if c == R):
            after += alone
    records = sorted({(int(c), int(r)) for c, r in zip(lc, rec) if r >= 0})
    for c, r in records:
        after += 2 * column_loop(c, 2)
    full = {(int(c), int(r)) for c, r, h in zip(lc, rec, half) if h == 1}
    moved = sum(1 for c, l, r in zip(cls, lc, rec) if r >= 0 and c != l)
    return before, after, len(records), len(records) - len(full), moved


def report(name, calls):
    before = after = 0.0
    records = dead = moved = nq = 0
    weight = 0.0
    for call in calls:
        batch = [len(q3[i]) for i in call]
        b, a, r, d, mv = step_cost(batch)
        before += b; after += a; records += r; dead += d; moved += mv; nq += len(batch)
        weight += sum(1.0 / (1.5 * max(1, (L + 15) // 16) + 3.19) for L in batch) / len(batch)
    steps = len(calls)
    print(f"{name}: {nq} queries in {steps} calls, {records} HALVES records, {dead} of them with a dead half ({100.0 * dead / max(1, records):.2f} %), {moved} queries moved up a class;\n"
          f"    column loops per query {before / nq:.4e} -> {after / nq:.4e} wave-instructions: {100.0 * (before - after) / before:.3f} % fewer "
          f"(every query paired in its own class at one instruction in 1.5 R + 3.19 would give {100.0 * weight / steps:.3f} %)")


print(f"stripes {len(mx)}: {body_cols} columns in unrolled bodies, {tail_cols} in last-chunk loops")
# bench.py: the timed queries in length order, 64 to a call; the warm-up steps in the order drawn; one query of every class per feeder thread
timed = sorted(range(n_timed), key=lambda i: len(q3[i]))
timed = [timed[k:k + G] for k in range(0, n_timed, G)]
warm = [list(range(k, min(k + G, n_timed + n_warm))) for k in range(n_timed, n_timed + n_warm, G)]
first = {}
for i in list(range(n_timed, n_timed + n_warm)) + list(range(n_timed)):
    first.setdefault((len(q3[i]) + 15) // 16, i)
report("timed steps", timed)
report("warm-up + timed steps (what a counter pass sees of the batched calls)", warm + [sorted(first.values())] * args.host_threads + timed)

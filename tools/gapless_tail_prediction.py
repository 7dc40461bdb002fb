#!/usr/bin/env python3
"""Host-only: the VALU wave-instructions per query k_gapless issues on the benchmark's database, before and after the stripe's last chunk is cut to
its real columns and odd register classes fold their last register across two columns.  Counted from the stripe table and the
queries' lengths alone, to set beside a `rocprofv3 --pmc SQ_INSTS_VALU` pass of the same bench.py arguments.

Per target column a lane issues R packed adds, ceil(R / 2) max3 and 3 others (row address, dpp move, hand-off perm).  After the change a column of
the unrolled body issues R + R / 2 + 3 (odd R: half a max3 less), a column of the last-chunk loop R + ceil(R / 2) + 3 + 5 (the codes move down
through the four residue words: 3 alignbit + 1 shift, and one copy of the row address), and the padding columns are gone.
usage: gapless_tail_prediction.py [--targets N] [--steps K] [--warmup W] [--group G]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foldseek_amd import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--targets", type=int, default=1000000)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--group", type=int, default=64)
ap.add_argument("--fullrange-steps", type=int, default=8)
ap.add_argument("--homologs", type=int, default=50)
args = ap.parse_args()

G = args.group
n_timed, n_warm = args.steps * G, args.warmup * G
q3, qa = synth.make_queries(n_timed + n_warm, seed=1000, lo=250, hi=450)           # bench.py: timed queries first, then the warm-up ones
f3, fa = synth.make_queries(args.fullrange_steps * G, seed=3000, lo=30, hi=2000)   # planted in every run
db = synth.make_db_fast(args.targets, (q3 + f3, qa + fa), seed=20260923, homologs_per_query=args.homologs)
lens = np.sort(np.asarray(db.lengths, np.int64), kind="stable")
pad = (-len(lens)) % 8
mx = np.concatenate([lens, np.zeros(pad, np.int64)]).reshape(-1, 8).max(axis=1)
real = int(mx.sum())
padded = int(((mx + 15) // 16 * 16).sum())
tail = mx % 16                                                                    # columns the last-chunk loop runs (0: the last chunk is full)
tail_cols = int(tail.sum())
print(f"stripes {len(mx)}: {padded} columns processed before, {real} real ({100.0 * (padded - real) / padded:.3f} % padding), "
      f"{tail_cols} of them in last-chunk loops ({100.0 * tail_cols / real:.3f} %)")


def launches(batch):
    """(R, queries) per kernel of one multi-query call: classes up to 16 run two queries to a kernel of 2 R registers"""
    out = []
    cls = {}
    for L in batch:
        R = max(1, (L + 15) // 16)
        cls[R] = cls.get(R, 0) + 1
    for R, m in cls.items():
        if R <= 16 and m >= 2:
            out += [(2 * R, 2)] * (m // 2) + [(R, 1)] * (m % 2)
        else:
            out += [(R, 1)] * m
    return out


order = list(range(n_timed, n_timed + n_warm)) + list(range(n_timed))              # warm-up steps first: the counters see them too
before = after = 0.0
nq = 0
odd = 0
for s in range(0, len(order), G):
    batch = [len(q3[i]) for i in order[s:s + G]]
    for R, m in launches(batch):
        half = (R + 1) // 2
        before += padded * (R + half + 3)
        after += (real - tail_cols) * (R + R / 2.0 + 3) + tail_cols * (R + half + 3 + 5)
        nq += m
        odd += m * (R % 2)
per_wave_column = 1.0                                                             # a wave serves the 8 targets of a stripe: one wave-instruction per stripe column
print(f"{nq} query slots ({odd} in odd classes): predicted SQ_INSTS_VALU per query {before * per_wave_column / nq:.4e} -> {after * per_wave_column / nq:.4e} "
      f"({100.0 * (before - after) / before:.3f} % fewer; column loop only: LDS image build, epilogue and column-segment warm-up not counted)")

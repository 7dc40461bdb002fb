#!/usr/bin/env python3
"""tools/tm_superpose_timing.py -- the driver behind profiles/tm_superpose.txt (needs an MI355X and the built library).

On the fixture task list of tests/test_tm_exact_gpu.py (144 records x 3 normalisations and the crafted records, 495 tasks): kernel ms (HIP events inside the
entries, fsgpu_last_kernel_ms) and caller-seen wall time of fsgpu_tm_batch (slots 16 / 17) and of fsgpu_tm_superpose_batch (slots 18 / 19 / 20),
approximate and exact.  --lib-root DIR imports foldseek_amd from another checkout (one that may not have the new entry yet: then only fsgpu_tm_batch is
timed), so that two builds can be timed in one session.
Usage: python3 tools/tm_superpose_timing.py [--lib-root DIR] [--out FILE]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
arg = lambda name, d=None: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else d
OUT, LIB_ROOT = arg('--out'), os.path.abspath(arg('--lib-root', ROOT))
sys.path.insert(0, LIB_ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
from foldseek_amd import api
import tm_cases as TC

out = []
def say(s):
    print(s, flush=True); out.append(s)

def timed(ctx, call, slots, warm=3, reps=10):
    for _ in range(warm):
        call()
    wall, ks = [], [[] for _ in slots]
    for _ in range(reps):
        t0 = time.perf_counter(); call(); wall.append(time.perf_counter() - t0)
        for i, s in enumerate(slots):
            ks[i].append(ctx.kernel_ms(s))
    return wall, ks

def report(names, wall, ks, nt):
    for name, k in zip(names, ks):
        say(f"  {name:<15} median {statistics.median(k):.3f} ms (min {min(k):.3f}, max {max(k):.3f})")
    w = statistics.median(wall)
    say(f"  caller-seen     median {w * 1e3:.3f} ms (min {min(wall) * 1e3:.3f}, max {max(wall) * 1e3:.3f}) -> {nt / w:,.0f} tasks/s")

ctx = api.Context(0)
coords, tasks = TC.fixture_tasks()
say(f"library: {os.path.relpath(api.LIB_PATH, ROOT)}; one MI355X, one context, one host thread (3 warm-up calls, 10 timed; Python staging is in the wall time)")
say(f"the fixture call: {len(tasks)} tasks, {sum(t[4].count('M') for t in tasks) / len(tasks):.0f} pairs on average")
say("fsgpu_tm_batch:")
wall, ks = timed(ctx, lambda: ctx.tm_batch(coords, coords, tasks), (16, 17))
report(("k_tm_pairs", "k_tm_search"), wall, ks, len(tasks))
if hasattr(ctx, "tm_superpose_batch"):
    for exact in (False, True):
        say(f"fsgpu_tm_superpose_batch, exact = {int(exact)}:")
        wall, ks = timed(ctx, lambda: ctx.tm_superpose_batch(coords, coords, tasks, exact=exact), (18, 19, 20))
        report(("k_tm_pairs", "k_tm_sp_search", "k_tm_sp_finish"), wall, ks, len(tasks))
ctx.close()
if OUT:
    open(OUT, "w").write("\n".join(out) + "\n")

#!/usr/bin/env python3
"""tools/tm_timing.py -- the driver behind profiles/tm_batch.txt (needs an MI355X and the built library).

fsgpu_tm_batch: kernel ms (HIP events inside the entry, fsgpu_last_kernel_ms 16 / 17) and caller-seen wall time for two inputs -- the fixture call of
tests/test_tm_gpu.py (144 pairs x 3 normalisations and the crafted records) and 3 200 synthetic hits of about 300 pairs on 64 queries, the accepted hits
of one 64-query align batch -- with fsgpu_lddt_batch on the same synthetic hits next to it.
Usage: python3 tools/tm_timing.py [--out FILE]"""
import ctypes as C
import os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from foldseek_amd import api

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
        say(f"  {name:<12} median {statistics.median(k):.3f} ms (min {min(k):.3f}, max {max(k):.3f})")
    w = statistics.median(wall)
    say(f"  caller-seen  median {w * 1e3:.3f} ms (min {min(wall) * 1e3:.3f}, max {max(wall) * 1e3:.3f}) -> {nt / w:,.0f} tasks/s")

def walk(rng, L):
    v = rng.normal(size=(L, 3)); v = v / np.linalg.norm(v, axis=1)[:, None] * 3.8
    return np.ascontiguousarray(np.cumsum(v, axis=0).T, np.float32)

ctx = api.Context(0)
say("fsgpu_tm_batch on one MI355X, one context, one host thread (3 warm-up calls, 10 timed)")

import tm_cases as TC
coords, tasks = TC.fixture_tasks()
say(f"the fixture call: {len(tasks)} tasks, {sum(t[4].count('M') for t in tasks) / len(tasks):.0f} pairs on average (through Context.tm_batch: Python staging is in the wall time)")
wall, ks = timed(ctx, lambda: ctx.tm_batch(coords, coords, tasks), (16, 17))
report(("k_tm_pairs", "k_tm_search"), wall, ks, len(tasks))

# 3 200 hits of about 300 pairs on 64 queries, both entries on the same hits, C entries called directly on prebuilt inputs
rng = np.random.default_rng(2)
nq, nt, cols = 64, 3200, 300
L = cols + 50
queries = [walk(rng, L) for _ in range(nq)]
targets = [q + rng.normal(scale=1.5, size=q.shape).astype(np.float32) for q in queries]
qs = (api.LddtQuery * nq)()
for i, q in enumerate(queries):
    qs[i].ca, qs[i].L, qs[i].reserved = q.ctypes.data, L, 0
tc = np.concatenate([t.reshape(-1) for t in targets])
lt, tt = (api.LddtTask * nt)(), (api.TmTask * nt)()
bts, boff, ooff, total = [], 0, 0, 0
par = {}
for k in range(nt):
    n = int(rng.integers(cols - 30, cols + 31))
    bt = ("M" * (n // 2) + "ID" + "M" * (n - n // 2)).encode()
    q = k % nq
    start = (int(rng.integers(0, 5)), int(rng.integers(0, 5)))
    for t in (lt[k], tt[k]):
        t.query, t.tLen, t.tOff, t.qStart, t.dbStart, t.btOff, t.btLen, t.reserved = q, L, q * 3 * L, start[0], start[1], boff, len(bt), 0
    lt[k].outOff = ooff
    if n not in par:
        par[n] = api.tm_params(n)
    tt[k].scoreD8, tt[k].d0Std, tt[k].d0, tt[k].d0Search = (float(v) for v in par[n])
    bts.append(bt); boff += len(bt); ooff += n; total += n
bt = np.frombuffer(b"".join(bts), np.uint8)
aln = np.zeros(nt, np.int32); o = np.zeros(ooff, np.float32)
npairs = np.zeros(nt, np.int32); scores = np.zeros(2 * nt, np.float32); rmsd = np.zeros(nt, np.float32)
lib = api.lib()
vp = lambda a: a.ctypes.data_as(C.c_void_p)
def call_tm():
    assert lib.fsgpu_tm_batch(ctx.h, qs, nq, tt, nt, vp(tc), tc.size, vp(bt), bt.size, vp(npairs), vp(scores), vp(rmsd)) == 0
def call_lddt():
    assert lib.fsgpu_lddt_batch(ctx.h, qs, nq, lt, nt, vp(tc), tc.size, vp(bt), bt.size, vp(aln), vp(o), ooff) == 0
say(f"{nt} tasks, {total / nt:.0f} pairs on average, {nq} queries of {L} residues, the target a perturbed copy (1.5 A) of the query:")
wall, ks = timed(ctx, call_tm, (16, 17))
report(("k_tm_pairs", "k_tm_search"), wall, ks, nt)
say("fsgpu_lddt_batch on the same hits:")
wall, ks = timed(ctx, call_lddt, (14, 15))
report(("k_lddt_norm", "k_lddt_pairs"), wall, ks, nt)
ctx.close()
if OUT:
    open(OUT, "w").write("\n".join(out) + "\n")

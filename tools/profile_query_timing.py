#!/usr/bin/env python3
"""tools/profile_query_timing.py -- the driver behind profiles/profile_queries.txt (needs an MI355X and the built library).

The forward pass of 64 profile queries of about 300 positions against 1000 targets each, three ways on one context, alternating, each after warm-up
calls: fsgpu_sw_multi_dir_p (k_sw3 over the images k_sw3_image_profile builds), the same tables widened to int16 through fsgpu_sw_multi_dir (k_sw2),
and -- the yardstick -- fsgpu_sw_multi_dir_c on the sequences the profiles were made from.  The profile of a query is its matrix column per position
(clipped to -32 .. 31, X row zero), so wherever nothing is clipped the three answers are the same records: compared here.
Kernel ms: fsgpu_last_kernel_ms(1), HIP events around the launches of the pass (image build and copies are outside; they are in the wall time).
Usage: python3 tools/profile_query_timing.py [--out FILE]"""
import os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from foldseek_amd import api, synth
import sw_cases as K

out = []
def say(s):
    print(s, flush=True); out.append(s)

NQ, NT, WARM, REPS = 64, 1000, 3, 10
m3, mA = K.matrices()
q3, qa = synth.make_queries(NQ, seed=12, mean_len=300, lo=250, hi=350)
db = synth.make_db(NT, (q3, qa), seed=13, homologs_per_query=10)
ids = np.arange(db.n, dtype=np.uint32)

def table(mat, codes, reverse):
    c = np.asarray(codes, np.int64)[::-1] if reverse else np.asarray(codes, np.int64)
    t = np.clip(mat[:, c].astype(np.int32), -32, 31).astype(np.int8)
    t[20] = 0
    return np.ascontiguousarray(t)

tabs = [(table(mA, a, False), table(m3, s, False), table(mA, a, True), table(m3, s, True)) for s, a in zip(q3, qa)]
clipped = sum(int((np.abs(m[:20][:, np.asarray(c, np.int64)].astype(np.int32)) > 31).sum()) for m, cs in ((m3, q3), (mA, qa)) for c in cs)
pq = [(t[0], t[1], t[2], t[3], ids) for t in tabs]
wq = [(t[0].astype(np.int16), t[1].astype(np.int16), t[2].astype(np.int16), t[3].astype(np.int16), t[1].shape[1], ids) for t in tabs]
cq = [(a, s, None, None, None, None, ids) for s, a in zip(q3, qa)]
ctx = api.Context(0)
ctx.load_db(db)
calls = {"fsgpu_sw_multi_dir_p (int8 tables, k_sw3)": lambda: ctx.sw_multi_dir_p(pq, 0),
         "fsgpu_sw_multi_dir (tables widened, k_sw2)": lambda: ctx.sw_multi_dir(wq, 0),
         "fsgpu_sw_multi_dir_c (sequences, k_sw3)": lambda: ctx.sw_multi_dir_c(m3, mA, cq, 0)}
say(f"forward pass, {NQ} queries of {min(map(len, q3))}..{max(map(len, q3))} positions (mean {np.mean([len(x) for x in q3]):.0f}) x {db.n} targets "
    f"(mean {db.lengths.mean():.0f} columns), 3Di + AA, gap costs 10 / 1; one MI355X, one context, {WARM} warm-up calls each, {REPS} timed, alternating")
res = {}
for name, f in calls.items():
    for _ in range(WARM):
        res[name] = f()
ms = {n: [] for n in calls}; wall = {n: [] for n in calls}
for _ in range(REPS):
    for name, f in calls.items():
        t0 = time.perf_counter(); f(); wall[name].append((time.perf_counter() - t0) * 1e3)
        ms[name].append(ctx.kernel_ms(1))
for name in calls:
    k, w = ms[name], wall[name]
    say(f"  {name:<44} kernel median {statistics.median(k):.3f} ms (min {min(k):.3f}, max {max(k):.3f}); caller-seen median {statistics.median(w):.1f} ms (Python staging included)")
ctx.sw_multi_dir_p(pq, 0)
say(f"  plan of the profile call: {ctx.sw3_last_plan()}")
ctx.sw_multi_dir_c(m3, mA, cq, 0)
say(f"  plan of the compact call: {ctx.sw3_last_plan()}")
names = list(calls)
same_w = all(a.tobytes() == b.tobytes() for a, b in zip(res[names[0]], res[names[1]]))
same_c = all(a.tobytes() == b.tobytes() for a, b in zip(res[names[0]], res[names[2]]))
say(f"  records: int8 tables == widened tables: {same_w}; == compact queries: {same_c} ({clipped} matrix entries of the queries' columns were clipped to -32 .. 31)")
p, w, c = (statistics.median(ms[n]) for n in names)
say(f"  profile entry / widened = {p / w:.2f}, profile entry / compact = {p / c:.2f}")
ctx.close()
if OUT:
    open(OUT, "w").write("\n".join(out) + "\n")

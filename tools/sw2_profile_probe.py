"""k_sw2 alone on the device (tools/sw2_probe.py has moved on to k_sw3): one batch of 32 queries x 1000 random targets of a 100k-target synthetic DB
through fsgpu_sw_multi_dir with ready-made profiles, forward pass, 3Di and 3Di + AA.  Prints per setting the device ms of the pass (HIP events around
the k_sw2 launches, best of 5) and one JSON line.  An optional first argument names another libfsgpu.so to load instead of the package's, so that
two builds can be timed against each other from one tree: python tools/sw2_profile_probe.py [path/to/libfsgpu.so]"""
import json, os, sys, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foldseek_amd import api, synth
if len(sys.argv) > 1:
    api.LIB_PATH = os.path.abspath(sys.argv[1])
NQ, NP = 32, 1000
q3, qa = synth.make_queries(NQ, seed=5000, lo=250, hi=450)
db = synth.make_db(100000, synth.make_queries(8, seed=1000, lo=250, hi=450))
ctx = api.Context(0); ctx.load_db(db)
rng = np.random.default_rng(1)
hits = [rng.choice(db.n, NP, replace=False).astype(np.uint32) for _ in range(NQ)]
m3, mA = api.Matrix(0, 2.1, 0.0), api.Matrix(1, 1.4, 0.0)
prof = []
for a, s in zip(qa, q3):
    pAf, p3f, _, _ = api.align_profiles(mA, m3, a, s)
    pAr, p3r, _, _ = api.align_profiles(mA, m3, a[::-1], s[::-1])
    prof.append((pAf, p3f, pAr, p3r))
out = {"lib": api.LIB_PATH}
for name, aa in (("3di", False), ("3di+aa", True)):
    queries = [(p[0] if aa else None, p[1], p[2] if aa else None, p[3], p[1].shape[1], h) for p, h in zip(prof, hits)]
    ms = []
    for rep in range(5):
        r = ctx.sw_multi_dir(queries, 0)
        ms.append(float(ctx.sw_last_passes()[0][0]))
    cells = float(ctx.sw_last_passes()[0][1])
    out[name] = min(ms)
    print("%s: k_sw2 forward pass %.4f ms (runs %s), %.3e cells -> %.3f Tcell/s; checksum %d" %
          (name, min(ms), " ".join("%.4f" % x for x in ms), cells, cells / min(ms) / 1e9, int(sum(int(x["score"].sum()) for x in r))), flush=True)
print(json.dumps(out))
ctx.close()

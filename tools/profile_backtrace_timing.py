"""profile backtrace: caller-seen time of fshost_search_align_batch_profile with FSGPU_PROFILE_BACKTRACE = 0 and = 1, alternating in one process, on one
module-sized batch (64 profile queries of 250..350 positions, about 50 accepted hits each).  usage: profile_backtrace_timing.py [cores]: the process is held to
that many cores (affinity, FSGPU_CORES_PER_GPU) first.  Output: profiles/profile_backtrace.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
cores = int(sys.argv[1]) if len(sys.argv) > 1 else 0
if cores:
    os.sched_setaffinity(0, set(sorted(os.sched_getaffinity(0))[:cores]))
    os.environ["FSGPU_CORES_PER_GPU"] = str(cores)
    os.environ["OMP_NUM_THREADS"] = str(cores)
from foldseek_amd import api, synth  # noqa: E402


def entry(mat, master):
    L = len(master)
    rec = np.zeros((L, 25), np.uint8)
    rec[:, :20] = np.clip(4 * mat[:20, master], -128, 127).astype(np.int8).T.view(np.uint8)
    rec[:, 20] = master; rec[:, 21] = master
    return rec.tobytes()


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hotpath_v1.npz"))
    m3, mA = g["sub_mat3di_2.1"].reshape(21, 21).astype(np.int32), g["sub_blosum62_1.4"].reshape(21, 21).astype(np.int32)
    q3, qa = synth.make_queries(64, seed=11, mean_len=300.0, lo=250, hi=350)
    db = synth.make_db(20000, (q3, qa), seed=12, homologs_per_query=50, mean_len=313.0, lo=30, hi=700)
    entries = [(entry(mA, a), entry(m3, s)) for a, s in zip(qa, q3)]
    ctx = api.Context(0)
    ctx.load_db(db)
    par = api.default_params()
    par.alignmentType, par.addBacktrace, par.maxResListLen = 2, 1, 60
    s = api.Search(ctx, par)
    hits = s.prefilter_batch_profile([e[1] for e in entries])
    lists = [np.ascontiguousarray(h["id"], np.uint32) for h in hits]
    keep, arr = s._pqueries(entries)
    nq = len(entries)
    res = [np.zeros(max(1, len(t)), api.RESULT_DT) for t in lists]
    P = C.c_void_p * nq
    pt, pr = P(*[x.ctypes.data for x in lists]), P(*[x.ctypes.data for x in res])
    ns = np.array([len(x) for x in lists], np.int32)
    nres = np.zeros(nq, np.int32)
    L = api.lib()

    def once(mode):
        os.environ["FSGPU_PROFILE_BACKTRACE"] = mode
        t0 = time.perf_counter()
        rc = L.fshost_search_align_batch_profile(s.h, nq, C.cast(arr, C.c_void_p), None, C.cast(pt, C.c_void_p), ns.ctypes.data_as(C.c_void_p), C.cast(pr, C.c_void_p),
                                                 nres.ctypes.data_as(C.c_void_p))
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, (rc, L.fshost_search_error(s.h))
        snap = b"".join(res[i][:nres[i]].tobytes() for i in range(nq)) + b"".join(x.encode() for i in range(nq) for x in s._bts(res[i][:nres[i]]))
        return ms, s.stats()[5] * 1e3, ctx.profile_backtrace_last() if mode == "1" else None, s.backtrace_counts(), snap

    out = {"0": [], "1": []}
    for _ in range(3):
        for mode in ("0", "1"):
            once(mode)
    for _ in range(12):
        for mode in ("0", "1"):
            out[mode].append(once(mode))
    assert out["0"][0][4] == out["1"][0][4], "records or backtraces differ between the two settings"
    lens = [len(x) for x in q3]
    print(f"cores {len(os.sched_getaffinity(0))}: 64 profile queries of {min(lens)}..{max(lens)} positions (mean {np.mean(lens):.0f}), {int(ns.sum())} listed pairs, "
          f"{int(nres.sum())} accepted hits, backtrace tasks (device answered, all) = {out['1'][0][3]}; 3 warm-up calls each, 12 timed, alternating")
    for mode in ("0", "1"):
        call = np.array([x[0] for x in out[mode]]); bt = np.array([x[1] for x in out[mode]])
        print(f"  FSGPU_PROFILE_BACKTRACE={mode}: caller-seen median {np.median(call):.2f} ms (min {call.min():.2f}, max {call.max():.2f}); "
              f"backtrace share (stats slot 5) median {np.median(bt):.2f} ms (min {bt.min():.2f}, max {bt.max():.2f})")
    k = np.array([x[2]["device_ms"] for x in out["1"]])
    print(f"  fsgpu_profile_backtrace kernels: median {np.median(k):.3f} ms (min {k.min():.3f}, max {k.max():.3f}); last call: {out['1'][-1][2]}")
    print("  records and backtraces of the two settings are the same bytes")
    s.close(); ctx.close()


main()

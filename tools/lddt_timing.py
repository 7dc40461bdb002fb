#!/usr/bin/env python3
"""tools/lddt_timing.py -- the driver behind profiles/lddt_batch.txt (needs an MI355X and the built library).

fsgpu_lddt_batch: kernel ms (HIP events inside the entry) and caller-seen tasks/s (wall time of the C call, inputs prebuilt and already decoded) for two batch
shapes, and the hit-by-hit form of the --max-accept / --max-rejected path (one task per call on one query); then the wall time of the structurealign module at
--lddt-threshold 0.7 against 0 on the 12 example structures with every prefilter line repeated 100 times, batched and with --max-rejected set.
Usage: python3 tools/lddt_timing.py [--out FILE]"""
import ctypes as C
import os, shutil, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
sys.path.insert(0, ROOT)
from foldseek_amd import api

out = []
def say(s):
    print(s, flush=True); out.append(s)

def walk(rng, L):
    v = rng.normal(size=(L, 3)); v = v / np.linalg.norm(v, axis=1)[:, None] * 3.8
    return np.ascontiguousarray(np.cumsum(v, axis=0).T, np.float32)

def shape(ctx, nt, cols, nq, seed):
    rng = np.random.default_rng(seed)
    L = cols + 20
    queries = [walk(rng, L) for _ in range(nq)]
    targets = [q + rng.normal(scale=1.0, size=q.shape).astype(np.float32) for q in queries]
    qs = (api.LddtQuery * nq)()
    for i, q in enumerate(queries):
        qs[i].ca, qs[i].L, qs[i].reserved = q.ctypes.data, L, 0
    tc = np.concatenate([t.reshape(-1) for t in targets])
    ts = (api.LddtTask * nt)()
    bts, boff, ooff, total = [], 0, 0, 0
    for k in range(nt):
        n = int(rng.integers(cols - 30, cols + 31)); n = min(n, L - 10)
        bt = ("M" * (n // 2) + "ID" + "M" * (n - n // 2)).encode()
        q = k % nq
        ts[k].query, ts[k].tLen, ts[k].tOff, ts[k].qStart, ts[k].dbStart = q, L, q * 3 * L, int(rng.integers(0, 5)), int(rng.integers(0, 5))
        ts[k].btOff, ts[k].btLen, ts[k].reserved, ts[k].outOff = boff, len(bt), 0, ooff
        bts.append(bt); boff += len(bt); ooff += n; total += n
    bt = np.frombuffer(b"".join(bts), np.uint8)
    aln = np.zeros(nt, np.int32); o = np.zeros(ooff, np.float32)
    lib = api.lib()
    call = lambda: lib.fsgpu_lddt_batch(ctx.h, qs, nq, ts, nt, tc.ctypes.data_as(C.c_void_p), tc.size, bt.ctypes.data_as(C.c_void_p), bt.size,
                                        aln.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), ooff)
    for _ in range(5):
        assert call() == 0
    wall, kn, kp = [], [], []
    for _ in range(20):
        t0 = time.perf_counter(); rc = call(); wall.append(time.perf_counter() - t0)
        assert rc == 0
        kn.append(ctx.kernel_ms(14)); kp.append(ctx.kernel_ms(15))
    w = statistics.median(wall)
    say(f"{nt} tasks, {total / nt:.0f} aligned columns on average, {nq} queries of {L} residues (5 warm-up calls, 20 timed):")
    say(f"  k_lddt_norm  median {statistics.median(kn):.3f} ms (min {min(kn):.3f}, max {max(kn):.3f})")
    say(f"  k_lddt_pairs median {statistics.median(kp):.3f} ms (min {min(kp):.3f}, max {max(kp):.3f})")
    say(f"  caller-seen  median {w * 1e3:.3f} ms (min {min(wall) * 1e3:.3f}, max {max(wall) * 1e3:.3f}) -> {nt / w:,.0f} tasks/s; input {(tc.nbytes + bt.nbytes) / 1e6:.1f} MB staged per call")

def one_by_one(ctx, cols, seed):
    """what gateAlign does with --max-accept / --max-rejected: one task per call, the same query every time (its norms stay on the device)"""
    rng = np.random.default_rng(seed)
    L = cols + 20
    q = walk(rng, L)
    tc = (q + rng.normal(scale=1.0, size=q.shape).astype(np.float32)).reshape(-1)
    qs = (api.LddtQuery * 1)(); qs[0].ca, qs[0].L, qs[0].reserved = q.ctypes.data, L, 0
    bt = np.frombuffer(("M" * cols).encode(), np.uint8)
    ts = (api.LddtTask * 1)()
    ts[0].query, ts[0].tLen, ts[0].tOff, ts[0].qStart, ts[0].dbStart, ts[0].btOff, ts[0].btLen, ts[0].reserved, ts[0].outOff = 0, L, 0, 2, 3, 0, cols, 0, 0
    aln = np.zeros(1, np.int32); o = np.zeros(cols, np.float32)
    lib = api.lib()
    call = lambda: lib.fsgpu_lddt_batch(ctx.h, qs, 1, ts, 1, tc.ctypes.data_as(C.c_void_p), tc.size, bt.ctypes.data_as(C.c_void_p), bt.size,
                                        aln.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), cols)
    for _ in range(20):
        assert call() == 0
    wall = []
    for _ in range(200):
        t0 = time.perf_counter(); rc = call(); wall.append(time.perf_counter() - t0)
        assert rc == 0
    w = statistics.median(wall)
    say(f"one task of {cols} aligned columns per call, same query of {L} residues (20 warm-up calls, 200 timed): caller-seen median {w * 1e6:.1f} us "
        f"(min {min(wall) * 1e6:.1f}, max {max(wall) * 1e6:.1f}) -> {1 / w:,.0f} tasks/s")

ctx = api.Context(0)
say("fsgpu_lddt_batch on one MI355X, one context, one host thread")
shape(ctx, 3000, 150, 1024, 1)
shape(ctx, 3200, 330, 64, 2)
one_by_one(ctx, 150, 3)
one_by_one(ctx, 330, 4)
ctx.close()

# ---- module wall time: structurealign on the 12 example structures with every prefilter line repeated 100 times (14 400 pairs)
G = os.path.join(ROOT, "tests", "golden", "ca_v1")
BIN = os.path.join(ROOT, "foldseek_amd", "bin", "fsgpu-modules")
w = tempfile.mkdtemp()
for f in os.listdir(G):
    if f.startswith("db") and not f.startswith("db_pad"):
        shutil.copy(os.path.join(G, f), os.path.join(w, f))
data = open(os.path.join(G, "pref"), "rb").read()
blob, idx, off = b"", [], 0
for line in open(os.path.join(G, "pref.index")):
    k, o_, l = line.split()
    body = data[int(o_):int(o_) + int(l) - 1] * 100 + b"\0"
    idx.append(f"{k}\t{off}\t{len(body)}\n"); blob += body; off += len(body)
open(os.path.join(w, "pref"), "wb").write(blob); open(os.path.join(w, "pref.index"), "w").write("".join(idx))
shutil.copy(os.path.join(G, "pref.dbtype"), os.path.join(w, "pref.dbtype"))
say("")
say("structurealign module, 12 queries x 1 200 prefilter lines (14 400 pairs, all accepted at threshold 0), -a 1, --threads 1, wall time of the process (3 runs each);")
say("with --max-rejected 1000000 the module takes its hit-by-hit path (backtrace and LDDT of a hit when the loop reaches it):")
for thr, extra in (("0", []), ("0.7", []), ("0", ["--max-rejected", "1000000"]), ("0.7", ["--max-rejected", "1000000"])):
    ts = []
    for r in range(4):
        outdb = os.path.join(w, f"o_{thr}_{len(extra)}_{r}")
        t0 = time.perf_counter()
        p = subprocess.run([BIN, "structurealign", os.path.join(w, "db"), os.path.join(w, "db"), os.path.join(w, "pref"), outdb, "--sort-by-structure-bits", "0",
                            "-a", "1", "-e", "10", "--threads", "1", "--lddt-threshold", thr] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        ts.append(time.perf_counter() - t0)
        assert p.returncode == 0, p.stderr
    n = sum(1 for _ in open(outdb, "rb").read().split(b"\n")) - 1
    say(f"  --lddt-threshold {thr}{' ' + ' '.join(extra) if extra else ''}: " + ", ".join(f"{t:.3f}" for t in ts[1:]) + f" s (first run {ts[0]:.3f} s not counted), {n} result lines")
shutil.rmtree(w)
if OUT:
    open(OUT, "w").write("\n".join(out) + "\n")

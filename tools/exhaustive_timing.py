#!/usr/bin/env python3
"""tools/exhaustive_timing.py -- the exhaustive search on a synthetic database, timed.

(i)  Search.exhaustive_batch: one database-wide forward pass with the selection on the device (fsgpu_sw_scan_c), the survivors through the align body.
(ii) The same answer the only way it could be had before: Search.align_batch with every target in every query's list.  --baseline-lib names the
     libfsgpu.so to run (ii) with (a build of the commit before the exhaustive entry); without it (ii) runs on this tree's library, whose align_batch
     is the same code.

Every measurement runs in a child process of its own (one library per process), (ii) and (i) alternating, --rounds times; a child builds the seeded
database, warms up --warmup calls and times --reps calls with a host clock around calls that end in a device synchronise.  Reported per variant: the
median and the spread (min .. max) over all timed calls of all rounds; for (i) also the device ms of the Smith-Waterman launches and of the two
selection kernels (fsgpu_last_kernel_ms 21 / 22 / 23), the host ms spent planning, the sub-batches, the records the selection handed over and the
survivors per query.  The two answers are compared by digest.

    python tools/exhaustive_timing.py --targets 100000 --queries 16 --out profiles/exhaustive_scan.txt
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np
    from foldseek_amd import api, synth
    if args.lib:
        # an older library lacks the entries the binding has learnt since: they are bound to a stub that raises when called, (ii) calls none of them
        class Baseline(api.C.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith(("fsgpu_", "fshost_")):
                        raise

                    def missing(*_):
                        raise RuntimeError(f"{name} is not in the baseline library")
                    return missing
        api.LIB_PATH = os.path.abspath(args.lib)
        api.C.CDLL = Baseline
    q3, qa = synth.make_queries(args.queries, seed=11, mean_len=350.0, lo=200, hi=600)
    db = synth.make_db_fast(args.targets, (q3, qa), seed=12, homologs_per_query=20)
    ctx = api.Context(0)
    ctx.load_db(db)
    par = api.default_params()
    par.alignmentType, par.addBacktrace = 2, 1
    s = api.Search(ctx, par, nn_path=os.path.join(ROOT, "foldseek_amd", "data", "evalue_nn.bin"))     # a baseline library elsewhere looks for it next to itself
    every = np.arange(db.n, dtype=np.uint32)

    def run():
        if args.child == "exhaustive":
            return s.exhaustive_batch(qa, q3)
        return s.align_batch(qa, q3, [every] * len(q3))
    for _ in range(args.warmup):
        res = run()
    times, extra = [], {}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = run()                                  # returns after the last device wait of the call
        times.append((time.perf_counter() - t0) * 1e3)
    if args.child == "exhaustive":
        last = ctx.sw_scan_last()
        extra = dict(sw_ms=ctx.kernel_ms(21), count_ms=ctx.kernel_ms(22), emit_ms=ctx.kernel_ms(23), plan_ms=last["plan_ms"], scan_call_ms=last["call_ms"],
                     sub_batches=last["sub_batches"], device_selected=last["device_selected"], survivors=s.last_survivors)
    h = hashlib.blake2b(digest_size=8)
    for r in res:
        h.update(np.ascontiguousarray(r).tobytes())
    print(json.dumps(dict(variant=args.child, ms=times, accepted=[len(r) for r in res], digest=h.hexdigest(), targets=int(db.n), residues=int(db.residues),
                          query_lengths=[len(x) for x in q3], **extra)), flush=True)
    s.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("exhaustive", "align"), default=None)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"align": [], "exhaustive": []}
    for _ in range(args.rounds):
        for variant in ("align", "exhaustive"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--targets", str(args.targets), "--queries", str(args.queries),
                   "--reps", str(args.reps), "--warmup", str(args.warmup)]
            if variant == "align" and args.baseline_lib:
                cmd += ["--lib", args.baseline_lib]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit(f"{variant} child ended with status {p.returncode}")
            runs[variant].append(json.loads(p.stdout.strip().splitlines()[-1]))
    lines = []

    def say(x=""):
        lines.append(x)
        print(x, flush=True)
    a, e = runs["align"], runs["exhaustive"]
    say(f"exhaustive search, synthetic database: {e[0]['targets']} targets, {e[0]['residues']} residues, {args.queries} queries of {min(e[0]['query_lengths'])}..{max(e[0]['query_lengths'])} residues, 3Di + AA")
    say(f"{args.rounds} rounds, alternating; per child {args.warmup} warm-up calls, {args.reps} timed calls; host clock around calls that end in a device wait")
    for name, rs, what in (("(ii) align_batch over range(N)", a, "baseline library: " + (args.baseline_lib or "this tree's")), ("(i) exhaustive_batch", e, "")):
        ms = [x for r in rs for x in r["ms"]]
        say(f"{name}: median {statistics.median(ms):.1f} ms per call, min {min(ms):.1f}, max {max(ms):.1f} over {len(ms)} calls  {what}")
    for r in e:
        say(f"  (i) last call of a round: SW launches {r['sw_ms']:.2f} ms, k_sw_scan_count + offsets {r['count_ms']:.3f} ms, k_sw_scan_emit {r['emit_ms']:.3f} ms on the device; "
            f"host planning {r['plan_ms']:.2f} ms ({r['plan_ms'] / args.queries:.3f} per query), scan call {r['scan_call_ms']:.1f} ms, {r['sub_batches']} sub-batch(es), "
            f"{r['device_selected']} records handed to the host")
    say(f"  survivors per query: {e[0]['survivors']}")
    say(f"  accepted per query:  {e[0]['accepted']}")
    same = len({r["digest"] for r in a + e}) == 1
    say(f"answers of (i) and (ii) identical in every round: {same}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not same:
        sys.exit("the two answers differ")


if __name__ == "__main__":
    main()

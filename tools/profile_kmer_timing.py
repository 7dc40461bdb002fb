#!/usr/bin/env python3
"""tools/profile_kmer_timing.py -- the driver behind profiles/profile_kmer_queries.txt (needs an MI355X and the built library).

The k-mer prefilter with PROFILE queries (fsgpu_kmer_search_profile) next to the sequence form (fsgpu_kmer_search) on the profiles' consensus
sequences: 32 queries of 250..350 positions against the bench's synthetic database, -s 9.5 (k-mer threshold 75 for a profile, 78 for a sequence).
A profile's stored scores are the seeding matrix's column of its consensus letter (3di.out at bit factor 8, what the sequence form scores k-mers
with) plus noise of +-6, clipped to a byte; the profile index is built with kmerThr = 0, the sequence index with 78, on one context one after the other.
Times are the stage timers of the last batch (HIP events on the context's stream): count pass + scan, list pass + chunk tables, whole device part.
Usage: python3 tools/profile_kmer_timing.py [--targets N] [--out FILE]"""
import os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
NT = int(sys.argv[sys.argv.index('--targets') + 1]) if '--targets' in sys.argv else 100000
sys.path.insert(0, ROOT)
from foldseek_amd import api, synth

out = []
def say(s):
    print(s, flush=True); out.append(s)

NQ, WARM, REPS = 32, 2, 7
m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
q3, qa = synth.make_queries(NQ, seed=12, mean_len=300, lo=250, hi=350)
db = synth.make_db_fast(NT, (q3, qa), seed=13, homologs_per_query=20)
sub = np.asarray(m8.scores(), np.int32).reshape(21, 21)
rng = np.random.default_rng(14)
prof = []
for s in q3:
    c = np.minimum(np.asarray(s, np.int64) % 32, 19)
    raw = np.clip(sub[:20][:, c].T + rng.integers(-6, 7, (len(c), 20)), -128, 127).astype(np.int8)          # [L, 20]
    ung = np.zeros((len(c), 21), np.int8); ung[:, :20] = np.sign(raw.astype(np.int32)) * (np.abs(raw.astype(np.int32)) // 4)
    prof.append((c.astype(np.uint8), raw, ung, api.kmer_threshold_profile(9.5, 6, False)))
positions = sum(max(0, len(s) - 9) for s in q3)
ctx = api.Context(0)
ctx.load_db(db)
say(f"k-mer prefilter, {NQ} queries of {min(map(len, q3))}..{max(map(len, q3))} positions ({positions} k-mer starts) x {db.n} targets "
    f"({int(db.lengths.sum())} residues), spaced k-mers, -s 9.5; one MI355X, one context, {WARM} warm-up calls, {REPS} timed, medians")

def measure(name, call):
    rows = []
    for i in range(WARM + REPS):
        res, status = call()
        if i >= WARM:
            ms = ctx.kmer_stage_ms()
            rows.append((ms[1], ms[2], ms[10], ms[0]))
    cnt = [int(x) for x in ctx.kmer_counts()]
    c, l, k, tot = (statistics.median(r[j] for r in rows) for j in range(4))
    say(f"  {name}")
    say(f"    similar k-mers {cnt[0]} ({cnt[0] / positions:.0f} per position), index hits {cnt[1]}, candidates {cnt[2]}, hits returned {sum(len(r) for r in res)}, "
        f"statuses {sorted(set(int(s) for s in status))}")
    say(f"    count pass + scan {c:.3f} ms, list pass + chunk tables {l:.3f} ms (list kernel alone {k:.3f} ms), whole batch on the device {tot:.3f} ms")
    say(f"    stage 1 = {c + l:.3f} ms = {100 * (c + l) / tot:.0f} % of the batch, {(c + l) * 1e6 / max(cnt[0], 1):.3f} ns per similar k-mer")
    return (c + l) * 1e6 / max(cnt[0], 1), (c + l) / tot

ctx.kmer_index_build(m8, kmer_thr=0)
p_ns, p_share = measure("profile queries (fsgpu_kmer_search_profile, index kmerThr 0, threshold 75)", lambda: ctx.kmer_search_profile(prof, l2_cache_size=2 << 20))
ctx.kmer_index_build(m8, kmer_thr=78)
seqs = [api.kmer_query_prepare(m8, m2, p[0], kmer_thr=78) for p in prof]
s_ns, s_share = measure("their consensus sequences (fsgpu_kmer_search, index kmerThr 78, threshold 78 - composition bias)", lambda: ctx.kmer_search(seqs, l2_cache_size=2 << 20))
say(f"  stage-1 ns per similar k-mer, profile form / sequence form = {p_ns / s_ns:.2f}; stage 1's share of the batch {100 * p_share:.0f} % / {100 * s_share:.0f} %")
ctx.close()
if OUT:
    open(OUT, "w").write("\n".join(out) + "\n")

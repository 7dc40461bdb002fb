#!/usr/bin/env python3
"""tests/golden/make_profile_kmer_golden.py -- generator of tests/golden/profile_kmer_v1 (TEST INFRASTRUCTURE).

Runs the WHOLE reference binary (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu): its `prefilter` module (the k-mer prefilter,
--prefilter-mode 0 of the search workflow) with PROFILE queries, and freezes the result databases the device path is held to.

(a) the 12 example structures: `prefilter profile_0_ss db_ss` -- both databases are the reference-written ones of tests/golden/profile_v1, read from
    there and not copied -- with the workflow's parameter string at -s 9.5 and -s 4, with contiguous k-mers, with --diag-score 0 and with --max-seqs 5.
(b) a crafted world: 300 synthetic 3Di targets and profile queries written with tests/profile_model.py's encoder -- relatives of targets; a profile with
    all 20 scores equal at every position (ties everywhere, and the cap of 8 388 607 similar k-mers); two-valued rows; rows at -128 / 127; an X query
    letter at each of the ten offsets of the spaced pattern (six used, four unused); lengths 5, 6, 9, 10, 11; a family of near-identical targets that
    saturate the 8-bit diagonal score, so that with --max-seqs 5 the truncated-score rescoring runs; --k-score's profile half set to 60, to 1000 (above
    every possible sum: 6 x 127 = 762) and to -5; a copy of the queries whose dbtype carries the context-pseudo-count bit (the other threshold formula).

The manifest records, per run, what the reference printed (k-mer threshold, k-mers per position, overflows) and what the conditions of
tests/test_kmer_profile_model.py read.  The run with --k-score 1000 can have no hit (no k-mer reaches the threshold): it is recorded as `expect_empty`
and is the one setting the "every setting has hits" condition does not apply to.

Needs the built reference binary only; it reads nothing else outside this repository.
"""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import profile_model as pm  # noqa: E402

FS = os.path.join(ROOT, "oracle", "_ref", "bin", "foldseek")
SRC = os.path.join(HERE, "profile_v1")
OUT = os.path.join(HERE, "profile_kmer_v1")
SUBMAT = "aa:3di.out,nucl:3di.out"
LETTERS = "ACDEFGHIKLMNPQRSTVWYX"
CONTEXT_DBTYPE = 2 | (4 << 16)          # DBTYPE_HMM_PROFILE with DBTYPE_EXTENDED_CONTEXT_PSEUDO_COUNTS

# F/data/structuresearch.sh ${PREFILTER_PAR} as the search workflow composes it; -v 3: the module prints its threshold and statistics
PREFILTER_PAR = ["--sub-mat", SUBMAT, "--seed-sub-mat", SUBMAT, "-s", "9.5", "-k", "6", "--target-search-mode", "0",
                 "--k-score", "seq:2147483647,prof:2147483647", "--alph-size", "aa:21,nucl:5", "--max-seq-len", "65535",
                 "--max-seqs", "1000", "--split", "0", "--split-mode", "2", "--split-memory-limit", "0", "-c", "0",
                 "--cov-mode", "0", "--comp-bias-corr", "1", "--comp-bias-corr-scale", "0.15", "--diag-score", "1",
                 "--exact-kmer-matching", "0", "--mask", "0", "--mask-prob", "0.999995", "--mask-lower-case", "1",
                 "--mask-n-repeat", "6", "--min-ungapped-score", "30", "--add-self-matches", "0", "--spaced-kmer-mode", "1",
                 "--db-load-mode", "0", "--pca", "substitution:1.100,context:1.400", "--pcb", "substitution:4.100,context:5.800",
                 "--threads", "1", "--compressed", "0", "-v", "3"]


def par(**kw):
    p = list(PREFILTER_PAR)
    for flag, v in kw.items():
        p[p.index(flag) + 1] = str(v)
    return p


def kscore(v):
    return f"seq:2147483647,prof:{v}"


# name -> (query db, target db, parameters, expect_empty)
RUNS = {
    "e_s95": ("profile_0_ss", "db_ss", par(), False),
    "e_s4": ("profile_0_ss", "db_ss", par(**{"-s": 4}), False),
    "e_nospace": ("profile_0_ss", "db_ss", par(**{"--spaced-kmer-mode": 0}), False),
    "e_diag0": ("profile_0_ss", "db_ss", par(**{"--diag-score": 0, "--min-ungapped-score": 0}), False),
    "e_max5": ("profile_0_ss", "db_ss", par(**{"--max-seqs": 5}), False),
    "c_s95": ("kprof_ss", "ktarget_ss", par(), False),
    "c_s4": ("kprof_ss", "ktarget_ss", par(**{"-s": 4}), False),
    "c_nospace": ("kprof_ss", "ktarget_ss", par(**{"--spaced-kmer-mode": 0}), False),
    "c_diag0": ("kprof_ss", "ktarget_ss", par(**{"--diag-score": 0, "--min-ungapped-score": 0}), False),
    "c_max5": ("kprof_ss", "ktarget_ss", par(**{"--max-seqs": 5}), False),
    "c_k60": ("kprof_ss", "ktarget_ss", par(**{"--k-score": kscore(60)}), False),
    "c_khuge": ("kprof_ss", "ktarget_ss", par(**{"--k-score": kscore(1000)}), True),
    "c_kneg": ("ksmall_ss", "ktarget_ss", par(**{"--k-score": kscore(-5)}), False),
    "c_kneg_nospace": ("ksmall_ss", "ktarget_ss", par(**{"--k-score": kscore(-5), "--spaced-kmer-mode": 0}), False),
    "c_small": ("ksmall_ss", "ktarget_ss", par(), False),
    "c_small_nospace": ("ksmall_ss", "ktarget_ss", par(**{"--spaced-kmer-mode": 0}), False),
    "c_ctx": ("kctx_ss", "ktarget_ss", par(), False),
}


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise SystemExit(f"FAILED: {' '.join(cmd)}")
    return r.stdout


def read_db(path):
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def write_db(path, entries, dbtype):
    blob, index, off = b"", [], 0
    for k in sorted(entries):
        body = entries[k] + b"\0"
        index.append(f"{k}\t{off}\t{len(body)}\n")
        blob += body
        off += len(body)
    open(path, "wb").write(blob)
    open(path + ".index", "w").write("".join(index))
    open(path + ".dbtype", "wb").write(int(dbtype).to_bytes(4, "little"))


def crafted(work):
    rng = np.random.default_rng(20261101)
    n = 300
    targets = [rng.integers(0, 20, int(rng.integers(60, 200))) for _ in range(n)]
    # a family of near-identical targets (ids 10..17): one base of 140 letters, 6 % of the letters changed per member
    base = rng.integers(0, 20, 140)
    for t in range(10, 18):
        m = base.copy()
        hit = rng.random(140) < 0.06
        m[hit] = rng.integers(0, 20, int(hit.sum()))
        targets[t] = m
    text = lambda c: ("".join(LETTERS[int(x)] for x in c) + "\n").encode()
    write_db(os.path.join(work, "ktarget_ss"), {k: text(v) for k, v in enumerate(targets)}, 0)

    def matching(codes, lo=-40, hi=60, noise=8):
        L = len(codes)
        s = np.full((20, L), lo, np.int32) + rng.integers(-noise, noise + 1, (20, L))
        s[np.asarray(codes, np.int64), np.arange(L)] = hi + rng.integers(-noise, noise + 1, L)
        return np.clip(s, -128, 127).astype(np.int8)

    q, note = {}, {}

    def add(entry, what):
        q[len(q)] = entry; note[str(len(q) - 1)] = what
    for t in (0, 1, 2, 3):                                                   # relatives of a target's consensus
        add(pm.encode(matching(targets[t]), targets[t]), f"relative of target {t}")
    # all 20 scores 20: every one of the 20^6 rank tuples sums to 120, above the threshold of every setting but --k-score 1000
    add(pm.encode(np.full((20, 10), 20, np.int8), targets[4][:10]), "flat: all scores equal, one spaced window, capped")
    two = np.where(rng.random((20, 90)) < 0.2, 30, -30); two[targets[5][:90], np.arange(90)] = 30
    add(pm.encode(two.astype(np.int8), targets[5][:90]), "two-valued rows, relative of target 5")
    ext = np.full((20, 80), -128, np.int8); ext[targets[6][:80], np.arange(80)] = 127
    add(pm.encode(ext, targets[6][:80]), "rows at -128 / 127, relative of target 6")
    add(pm.encode(matching(base, lo=-60, hi=120), base), "relative of the family 10..17: saturates the 8-bit diagonal score on each member")
    big = {k: v for k, v in q.items()}
    small, snote = {}, {}

    def adds(entry, what):
        small[len(small)] = entry; snote[str(len(small) - 1)] = what
    frag = targets[7]
    for L in (5, 6, 9, 10, 11):
        adds(pm.encode(matching(frag[:L]), frag[:L]), f"length {L}")
    for o in range(10):                                                      # an X query letter at every offset of the spaced pattern
        codes = frag[20:30].copy(); codes[o] = 20
        adds(pm.encode(matching(frag[20:30]), codes), f"length 10, X query letter at offset {o}")
    for k, v in small.items():
        big[len(q) + k] = v; note[str(len(q) + k)] = snote[str(k)]
    write_db(os.path.join(work, "kprof_ss"), big, 2)
    write_db(os.path.join(work, "kctx_ss"), big, CONTEXT_DBTYPE)
    write_db(os.path.join(work, "ksmall_ss"), small, 2)
    return {"targets": n, "family": list(range(10, 18)), "kprof_ss": note, "ksmall_ss": snote}


def main():
    if not os.path.exists(FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    work = os.path.join(ROOT, "oracle", "_ref_full", "profile_kmer_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for f in os.listdir(SRC):
        if f.split(".")[0] in ("db_ss", "profile_0_ss"):
            shutil.copy(os.path.join(SRC, f), work)
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu", "example_inputs": "tests/golden/profile_v1: profile_0_ss, db_ss",
                "crafted": crafted(work), "runs": {}}
    for name, (qdb, tdb, p, expect_empty) in RUNS.items():
        log = run([FS, "prefilter", qdb, tdb, name] + p, work)
        res = read_db(os.path.join(work, name))
        n_targets = len(read_db(os.path.join(work, tdb)))
        rows = {k: [l.split("\t") for l in v.decode().splitlines()] for k, v in res.items()}
        manifest["runs"][name] = {
            "module": "prefilter", "positional": [qdb, tdb], "parameters": p, "expect_empty": expect_empty, "targets": n_targets,
            "kmer_threshold": int(re.search(r"k-mer similarity threshold: (-?\d+)", log).group(1)),
            "kmers_per_pos": float(re.search(r"([0-9.]+) k-mers per position", log).group(1)),
            "overflows": int(re.search(r"(\d+) overflows", log).group(1)),
            "index_kmer_threshold": int(re.search(r"Index table k-mer threshold: (-?\d+)", log).group(1)),
            "lines": sum(len(r) for r in rows.values()), "queries_with_hits": sum(1 for r in rows.values() if r),
            "hits_at_255": {str(k): sum(1 for x in r if int(x[1]) >= 255) for k, r in rows.items() if any(int(x[1]) >= 255 for x in r)},
        }
    runs = manifest["runs"]
    # --max-seqs M: computeScoreThreshold stops in the 255 bucket, and rescoreHits runs, when at least min(M, targets) targets reach 255 -- counted
    # in the same run without the limit
    for limited, free in (("e_max5", "e_s95"), ("c_max5", "c_s95")):
        m = min(5, runs[limited]["targets"])
        runs[limited]["truncated_queries"] = sorted(int(k) for k, c in runs[free]["hits_at_255"].items() if c >= m)
    # the flat query alone: k-mers per position x L = the similar k-mers of its one window
    flat_key = next(int(k) for k, v in manifest["crafted"]["kprof_ss"].items() if v.startswith("flat"))
    write_db(os.path.join(work, "kflat_ss"), {0: read_db(os.path.join(work, "kprof_ss"))[flat_key]}, 2)
    log = run([FS, "prefilter", "kflat_ss", "ktarget_ss", "c_flat"] + par(), work)
    manifest["flat"] = {"query": flat_key, "length": 10, "kmers_per_pos": float(re.search(r"([0-9.]+) k-mers per position", log).group(1)),
                        "overflows": int(re.search(r"(\d+) overflows", log).group(1))}
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    keep = set(runs) | {"ktarget_ss", "kprof_ss", "kctx_ss", "ksmall_ss"}
    for f in sorted(os.listdir(work)):
        stem = f.split(".")[0]
        if os.path.isfile(os.path.join(work, f)) and stem in keep and f.split(".")[-1] in (stem, "index", "dbtype"):
            shutil.copy(os.path.join(work, f), os.path.join(OUT, f))
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    size = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(os.listdir(OUT))} files, {size} bytes -> {OUT}")
    for k, v in runs.items():
        print(k, {x: v[x] for x in ("kmer_threshold", "kmers_per_pos", "overflows", "lines", "queries_with_hits", "hits_at_255")}, v.get("truncated_queries"))
    print("flat", manifest["flat"])


if __name__ == "__main__":
    main()

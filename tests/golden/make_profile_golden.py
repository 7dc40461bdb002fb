#!/usr/bin/env python3
"""tests/golden/make_profile_golden.py -- generator of tests/golden/profile_v1 (TEST INFRASTRUCTURE).

Runs the WHOLE reference binary (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu) on the 12 committed structures of
tests/golden/example_structures and freezes what profile queries -- the later rounds of an iterative search -- are held to:

  * round 0: `createdb`, `ungappedprefilter`, `structurealign -a 1`, then `result2profile`, which writes profile_0 (AA) and profile_0_ss (3Di),
    both of type DBTYPE_HMM_PROFILE;
  * with those profiles as the query: `ungappedprefilter profile_0_ss db_ss`, and `structurealign profile_0 db <pref>` for --alignment-type 0 and 2,
    each with and without -a, with -e 0.001 -c 0.8 --cov-mode 0 (and with -e 1e-08 -c 0.97, which on these 12 relatives is what drops hits), and with
    --max-accept 3 --max-rejected 2;
  * a CRAFTED profile database (written here with tests/profile_model.py's encoder, no structure behind it) through the same two reference modules:
    one position; every score byte at an extreme (-128 / 127: -32 / 31 after the division by four); 600 positions of the constant maximum, whose
    int16 pass saturates against the 600-residue target written next to it; 1025 positions, which takes the long path.  (An entry stores 20 scores per
    position: there is no X score in it that a decoder could fail to zero; the X ROW of the alignment profile exists only in memory.)

Needs the built reference binary only; it reads nothing else outside this repository.
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import profile_model as pm  # noqa: E402

FS = os.path.join(ROOT, "oracle", "_ref", "bin", "foldseek")
EXAMPLE = os.path.join(HERE, "example_structures")
OUT = os.path.join(HERE, "profile_v1")
SUBMAT = "aa:3di.out,nucl:3di.out"
LETTERS = "ACDEFGHIKLMNPQRSTVWYX"

UNGAPPED_PAR = ["--sub-mat", SUBMAT, "-c", "0", "-e", "1.79769e+308", "--cov-mode", "0", "--comp-bias-corr", "1",
                "--comp-bias-corr-scale", "0.15", "--min-ungapped-score", "15", "--max-seqs", "1000", "--db-load-mode", "0",
                "--gpu", "0", "--gpu-server", "0", "--gpu-server-wait-timeout", "600", "--prefilter-mode", "1",
                "--threads", "1", "--compressed", "0", "-v", "1"]


def align_par(**kw):
    par = ["--tmscore-threshold", "0", "--tmscore-threshold-mode", "0", "--lddt-threshold", "0", "--sort-by-structure-bits", "0",
           "--alignment-type", "2", "--exact-tmscore", "0", "--sub-mat", SUBMAT, "-a", "1", "--alignment-mode", "3",
           "--alignment-output-mode", "0", "--wrapped-scoring", "0", "-e", "10", "--min-seq-id", "0", "--min-aln-len", "0",
           "--seq-id-mode", "0", "--alt-ali", "0", "-c", "0", "--cov-mode", "0", "--max-seq-len", "65535", "--comp-bias-corr", "1",
           "--comp-bias-corr-scale", "0.5", "--max-rejected", "2147483647", "--max-accept", "2147483647", "--add-self-matches", "0",
           "--db-load-mode", "0", "--pca", "substitution:1.100,context:1.400", "--pcb", "substitution:4.100,context:5.800",
           "--score-bias", "0", "--realign", "0", "--realign-score-bias", "-0.2", "--realign-max-seqs", "2147483647",
           "--corr-score-weight", "0", "--gap-open", "aa:10,nucl:10", "--gap-extend", "aa:1,nucl:1", "--zdrop", "40",
           "--threads", "1", "--compressed", "0", "-v", "1"]
    for flag, v in kw.items():
        par[par.index(flag) + 1] = str(v)
    return par


# name -> (positional args, parameters)
PROFILE_ALIGN_RUNS = {
    "paln_t2_a": (["profile_0", "db", "ppref"], align_par()),
    "paln_t2": (["profile_0", "db", "ppref"], align_par(**{"-a": 0})),
    "paln_t0_a": (["profile_0", "db", "ppref"], align_par(**{"--alignment-type": 0})),
    "paln_t0": (["profile_0", "db", "ppref"], align_par(**{"--alignment-type": 0, "-a": 0})),
    "paln_cov": (["profile_0", "db", "ppref"], align_par(**{"-e": 0.001, "-c": 0.8})),
    "paln_cov_strict": (["profile_0", "db", "ppref"], align_par(**{"-e": 1e-08, "-c": 0.97})),      # the 12 structures are one family: 0.001 / 0.8 drops nothing
    "paln_limits": (["profile_0", "db", "ppref"], align_par(**{"--max-accept": 3, "--max-rejected": 2})),
    "caln_t2_a": (["cprof", "ctarget", "cpref"], align_par()),
    "caln_t0": (["cprof", "ctarget", "cpref"], align_par(**{"--alignment-type": 0, "-a": 0})),
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
    """entries: {key: bytes without the terminator}"""
    blob, index, off = b"", [], 0
    for k in sorted(entries):
        body = entries[k] + b"\0"
        index.append(f"{k}\t{off}\t{len(body)}\n")
        blob += body
        off += len(body)
    open(path, "wb").write(blob)
    open(path + ".index", "w").write("".join(index))
    open(path + ".dbtype", "wb").write(int(dbtype).to_bytes(4, "little"))


def count_lines(path):
    return sum(len(v.decode().splitlines()) for v in read_db(path).values())


def crafted(work):
    """the crafted query profiles cprof / cprof_ss and their targets ctarget / ctarget_ss"""
    rng = np.random.default_rng(20261021)
    t3 = {0: rng.integers(0, 20, 600), 1: rng.integers(0, 20, 300), 2: rng.integers(0, 20, 1100), 3: rng.integers(0, 20, 40), 4: rng.integers(0, 20, 5)}
    tA = {k: rng.integers(0, 20, len(v)) for k, v in t3.items()}
    text = lambda c: ("".join(LETTERS[int(x)] for x in c) + "\n").encode()
    write_db(os.path.join(work, "ctarget"), {k: text(v) for k, v in tA.items()}, 0)
    write_db(os.path.join(work, "ctarget_ss"), {k: text(v) for k, v in t3.items()}, 0)
    write_db(os.path.join(work, "ctarget_h"), {k: f"target{k}\n".encode() for k in t3}, 12)

    def matching(codes, L, lo=-40, hi=60):
        """stored scores that favour `codes` position by position: hi on the letter, lo elsewhere, noise on both"""
        s = np.full((20, L), lo, np.int32) + rng.integers(-8, 9, (20, L))
        s[np.asarray(codes[:L], np.int64), np.arange(L)] = hi + rng.integers(-8, 9, L)
        return np.clip(s, -128, 127).astype(np.int8)

    q3, qA = {}, {}
    # 0: one position
    q3[0] = pm.encode(matching(t3[4], 1), t3[4][:1]); qA[0] = pm.encode(matching(tA[4], 1), tA[4][:1])
    # 1: every score byte at an extreme, the high one on the letters of target 3
    ext3 = np.full((20, 40), -128, np.int8); ext3[t3[3], np.arange(40)] = 127
    extA = np.full((20, 40), -128, np.int8); extA[tA[3], np.arange(40)] = 127
    q3[1] = pm.encode(ext3, t3[3]); qA[1] = pm.encode(extA, tA[3])
    # 2: 600 positions of the constant maximum: 62 a column against anything, 37200 > 32767 against the 600 residues of target 0
    q3[2] = pm.encode(np.full((20, 600), 127, np.int8), t3[0]); qA[2] = pm.encode(np.full((20, 600), 127, np.int8), tA[0])
    # 3: 1025 positions, a relative of target 2
    q3[3] = pm.encode(matching(t3[2], 1025), t3[2][:1025]); qA[3] = pm.encode(matching(tA[2], 1025), tA[2][:1025])
    # 4: 300 positions, a relative of target 1, consensus letters that differ from the query letters
    q3[4] = pm.encode(matching(t3[1], 300), t3[1], consensus=rng.integers(0, 21, 300), neff=77)
    qA[4] = pm.encode(matching(tA[1], 300), tA[1], consensus=rng.integers(0, 21, 300), neff=77)
    write_db(os.path.join(work, "cprof"), qA, 2)
    write_db(os.path.join(work, "cprof_ss"), q3, 2)
    write_db(os.path.join(work, "cprof_h"), {k: f"profile{k}\n".encode() for k in q3}, 12)
    return {"targets": {str(k): len(v) for k, v in t3.items()}, "queries": {str(k): len(v) // pm.RECORD for k, v in q3.items()}}


def main():
    if not os.path.exists(FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    work = os.path.join(ROOT, "oracle", "_ref_full", "profile_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu", "runs": {}}
    run([FS, "createdb", EXAMPLE, "db", "--threads", "1", "-v", "1"], work)
    run([FS, "ungappedprefilter", "db_ss", "db_ss", "pref0"] + UNGAPPED_PAR, work)
    run([FS, "structurealign", "db", "db", "pref0", "aln0"] + align_par(), work)
    run([FS, "result2profile", "db", "db", "aln0", "profile_0", "--threads", "1", "-v", "1"], work)
    for f in ("profile_0", "profile_0_ss"):
        assert int.from_bytes(open(os.path.join(work, f + ".dbtype"), "rb").read()[:2], "little") == 2, f
    manifest["round0"] = ["createdb", "ungappedprefilter db_ss db_ss pref0", "structurealign db db pref0 aln0", "result2profile db db aln0 profile_0"]
    manifest["crafted"] = crafted(work)
    for name, pos in (("ppref", ["profile_0_ss", "db_ss"]), ("cpref", ["cprof_ss", "ctarget_ss"])):
        run([FS, "ungappedprefilter"] + pos + [name] + UNGAPPED_PAR, work)
        manifest["runs"][name] = {"module": "ungappedprefilter", "positional": pos, "parameters": UNGAPPED_PAR, "lines": count_lines(os.path.join(work, name))}
    for name, (pos, par) in PROFILE_ALIGN_RUNS.items():
        run([FS, "structurealign"] + pos + [name] + par, work)
        manifest["runs"][name] = {"module": "structurealign", "positional": pos, "parameters": par, "lines": count_lines(os.path.join(work, name))}
    # the runs do what they are there for
    lines = {k: v["lines"] for k, v in manifest["runs"].items()}
    assert lines["ppref"] > 12 and lines["paln_t2_a"] > 12 and lines["paln_cov"] <= lines["paln_t2_a"] and 0 < lines["paln_cov_strict"] < lines["paln_t2_a"] and lines["paln_limits"] < lines["paln_t2_a"], lines
    assert lines["cpref"] >= 5 and lines["caln_t2_a"] >= 5, lines
    sat = [l.split("\t") for l in read_db(os.path.join(work, "caln_t2_a"))[2].decode().splitlines()]
    # forward and reversed profile are the same constant: both passes saturate in int16, the int32 re-runs give 37200 each, the record's score is
    # their difference, and its end cell (599, 599) is the int32 pass's (the int16 pass stops rising after 529 columns)
    assert any(int(r[0]) == 0 and int(r[1]) == 0 and (r[4], r[5], r[7], r[8]) == ("0", "599", "0", "599") and r[10] == "600M" for r in sat), sat
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    keep = ("db", "db_ss", "db_h", "profile_0", "profile_0_ss", "profile_0_h", "cprof", "cprof_ss", "cprof_h", "ctarget", "ctarget_ss", "ctarget_h", "pref0", "aln0")
    for f in sorted(os.listdir(work)):
        p = os.path.join(work, f)
        stem = f.split(".")[0]
        if os.path.isdir(p) or os.path.islink(p) or not (stem in keep or stem in manifest["runs"]) or f.endswith(".sh"):
            continue
        if f.split(".")[-1] not in (stem, "index", "dbtype"):
            continue
        shutil.copy(p, os.path.join(OUT, f))
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    n = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(os.listdir(OUT))} files, {n} bytes -> {OUT}", {k: v["lines"] for k, v in manifest["runs"].items()})


if __name__ == "__main__":
    main()

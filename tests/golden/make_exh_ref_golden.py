#!/usr/bin/env python3
"""Generator of tests/golden/exh_v1/ref_* (TEST INFRASTRUCTURE): the reference binary's own `search ... --exhaustive-search 1` (oracle/_ref/bin/foldseek,
CPU only, built by oracle/build_ref_full.sh) on the frozen SCOP databases of tests/golden/scop_v1, for both alignment types and two e-values.  The
result databases (data, .index, .dbtype; a few KB each) are frozen; tests/test_exhaustive_gpu.py holds `fsgpu-modules search --prefilter-mode 2` and
`--exhaustive-search 1` to them byte for byte.  --sort-by-structure-bits 0: there is no C-alpha database in scop_v1.
Run from the repository root where the reference binary exists: python tests/golden/make_exh_ref_golden.py"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FS = os.path.join(ROOT, "oracle", "_ref", "bin", "foldseek")
SCOP = os.path.join(HERE, "scop_v1")
OUT = os.path.join(HERE, "exh_v1")

# name -> flags on top of `search db db res tmp --exhaustive-search 1 -a 1 --sort-by-structure-bits 0 --threads 1`
RUNS = {
    "ref_t2_e10": ["--alignment-type", "2", "-e", "10"],
    "ref_t2_e1e-3": ["--alignment-type", "2", "-e", "0.001"],
    "ref_t0_e10": ["--alignment-type", "0", "-e", "10"],
    "ref_t0_e1e-3": ["--alignment-type", "0", "-e", "0.001"],
    "ref_t2_e10_pad": ["--alignment-type", "2", "-e", "10"],            # against the padded target (makepaddedseqdb renumbers the keys by length)
}
TARGET = {"ref_t2_e10_pad": "db_pad"}
COMMON = ["--exhaustive-search", "1", "-a", "1", "--sort-by-structure-bits", "0", "--threads", "1", "-v", "1"]


def main():
    if not os.path.exists(FS):
        sys.exit(f"{FS} not built (oracle/build_ref_full.sh)")
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as work:
        for f in os.listdir(SCOP):
            if f.startswith("db"):
                shutil.copy(os.path.join(SCOP, f), os.path.join(work, f))
        for link, target in json.load(open(os.path.join(SCOP, "MANIFEST.json")))["links"].items():      # what makepaddedseqdb links instead of copying
            os.symlink(os.path.join(work, target), os.path.join(work, link))
        for name, flags in RUNS.items():
            res, tmp = os.path.join(work, name), os.path.join(work, "tmp_" + name)
            subprocess.check_call([FS, "search", os.path.join(work, "db"), os.path.join(work, TARGET.get(name, "db")), res, tmp] + COMMON + flags, cwd=work)
            for ext in ("", ".index", ".dbtype"):
                shutil.copy(res + ext, os.path.join(OUT, name + ext))
            print(name, os.path.getsize(res), "bytes")
    json.dump({"common": COMMON, "runs": RUNS, "target": TARGET}, open(os.path.join(OUT, "REF_RUNS.json"), "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    main()

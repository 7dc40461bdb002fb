#!/usr/bin/env python3
"""tests/golden/make_tm_exact_golden.py -- generator of tests/golden/tm_exact_v1 (TEST INFRASTRUCTURE).

Runs the WHOLE reference binary (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu) on the databases frozen in tests/golden/ca_v1 (db, aln_l0)
and on the crafted database frozen in tests/golden/tm_v1 (tmdb, tmaln: tm_cases.crafted_records()), and freezes

  (a) the result DBs of the reference's `aln2tmscore` (a2t_ca, a2t_crafted: data, index, dbtype), --threads 1;
  (b) `convertalis --format-output query,target,alntmscore,qtmscore,ttmscore,rmsd,u,t` with --exact-tmscore 0 and 1 (conv_x0.m8, conv_x1.m8,
      conv_x0_crafted.m8, conv_x1_crafted.m8).

Before anything is frozen the LIVE model (tests/tm_exact_model.py) is asserted against every field of (a) and (b).  Its raw answers for the task lists of
tests/tm_exact_cases.py (these fixtures, the seeded corpus, the hits at the LDS limit), approximate and exact, are frozen as model_*_raw.npy, and for the
corpus how many starts reach the exact search's maximum, with how many distinct superpositions, in how many blocks of starts
(model_corpus_exact_ties.npy); that takes minutes on a process pool.  Running the generator twice gives identical files.  Needs the built reference binary only.
"""
import json
import multiprocessing
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import tm_cases as TC  # noqa: E402
import tm_exact_cases as XC  # noqa: E402
import tm_exact_model as X  # noqa: E402
from make_ca_golden import FS, read_db, run  # noqa: E402

CA = os.path.join(HERE, "ca_v1")
TM = os.path.join(HERE, "tm_v1")
OUT = os.path.join(HERE, "tm_exact_v1")
SUBMAT = "aa:3di.out,nucl:3di.out"
A2T_PAR = ["--threads", "1", "--compressed", "0", "-v", "1"]


def convert_par(exact):
    return ["--sub-mat", SUBMAT, "--format-mode", "0", "--format-output", "query,target,alntmscore,qtmscore,ttmscore,rmsd,u,t",
            "--translation-table", "1", "--gap-open", "aa:10,nucl:10", "--gap-extend", "aa:1,nucl:1", "--db-output", "0", "--db-load-mode", "0",
            "--search-type", "0", "--threads", "1", "--compressed", "0", "-v", "1", "--exact-tmscore", str(exact)]


def pool_raw(pool, lists, is_exact):
    cq, ct, tasks = lists
    rows = np.array(pool.map(XC.model_row, XC.task_args(cq, ct, tasks, is_exact), chunksize=4), np.uint32).reshape(len(tasks), X.RAW_COLS + 3)
    return np.ascontiguousarray(rows[:, :X.RAW_COLS]), np.ascontiguousarray(rows[:, X.RAW_COLS:])


def main():
    if not os.path.exists(FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    work = os.path.join(ROOT, "oracle", "_ref_full", "tm_exact_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for src, prefixes in ((CA, ("db", "aln_l0")), (TM, ("tmdb", "tmaln"))):
        for f in sorted(os.listdir(src)):
            if f.startswith(prefixes) and not f.startswith("db_pad") and (not f.startswith("aln_l0") or f.split(".")[0] == "aln_l0"):
                shutil.copy(os.path.join(src, f), os.path.join(work, f))
    inputs = set(os.listdir(work))
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu",
                "inputs": "tests/golden/ca_v1: db*, aln_l0; tests/golden/tm_v1: tmdb*, tmaln", "runs": {}}
    sets = (("ca", "db", "aln_l0", ""), ("crafted", "tmdb", "tmaln", "_crafted"))
    for name, db, aln, suffix in sets:
        run([FS, "aln2tmscore", db, db, aln, "a2t_" + name] + A2T_PAR, work)
        manifest["runs"]["a2t_" + name] = {"module": "aln2tmscore", "positional": [db, db, aln], "parameters": A2T_PAR}
        for ex in (0, 1):
            out = f"conv_x{ex}{suffix}.m8"
            run([FS, "convertalis", db, db, aln, out] + convert_par(ex), work)
            manifest["runs"][out] = {"module": "convertalis", "positional": [db, db, aln], "parameters": convert_par(ex)}

    # ---- the live model on every fixture task, both modes, against every field the reference printed
    coords, tasks = XC.fixture_tasks()
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        raw = {ex: pool_raw(pool, (coords, coords, tasks), bool(ex))[0] for ex in (0, 1)}
        # (b): the .m8 rows are in task order, three tasks a record
        for ex in (0, 1):
            text = [l.rstrip("\n").split("\t") for suffix in ("", "_crafted") for l in open(os.path.join(work, f"conv_x{ex}{suffix}.m8"))]
            assert len(text) * 3 == len(tasks), (len(text), len(tasks))
            for r, row in enumerate(text):
                got = X.convertalis_fields(raw[ex][3 * r:3 * r + 3], [t[5] for t in tasks[3 * r:3 * r + 3]], bool(ex))
                assert got == row[2:8], (ex, r, row, got)
        # (a): mode 0, approximate; the lines of a query in record order
        r = 0
        lines = 0
        for name, _, aln, _ in sets:
            src = CA if name == "ca" else TM
            recs = TC.result_records(lambda n, s=src: read_db(os.path.join(s, n)), aln)
            got = read_db(os.path.join(work, "a2t_" + name))
            per_q = {}
            for q, c in recs:
                per_q.setdefault(q, []).append(X.aln2tmscore_line(int(c[0]), raw[0][3 * r], tasks[3 * r][5], False))
                r += 1
            assert sorted(per_q) == sorted(got)
            for q in per_q:
                assert got[q].decode().splitlines() == per_q[q], (name, q, got[q].decode().splitlines(), per_q[q])
                lines += len(per_q[q])
        assert 3 * r == len(tasks)
        manifest["a2t_lines"] = lines
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        for f in sorted(os.listdir(work)):
            p = os.path.join(work, f)
            if f in inputs or os.path.islink(p) or os.path.isdir(p) or "_tmp" in f or ".idx" in f:
                continue
            shutil.copy(p, os.path.join(OUT, f))
        for ex in (0, 1):
            np.save(os.path.join(OUT, f"model_fixture_{'exact' if ex else 'approx'}_raw.npy"), raw[ex])
        # ---- the model's raw answers for the seeded lists
        for which in ("corpus", "edge"):
            lists = XC.LISTS[which]()
            for ex in (0, 1):
                rows, ties = pool_raw(pool, lists, bool(ex))
                np.save(os.path.join(OUT, f"model_{which}_{'exact' if ex else 'approx'}_raw.npy"), rows)
                if which == "corpus" and ex:
                    # self-alignments and rigid copies: the maximum is reached by many starts with bit-distinct rotations in several blocks of starts, so
                    # the first-maximum rule and the reduction across workgroups are visible in t / u
                    assert int(((ties[:, 0] >= 2) & (ties[:, 1] >= 2) & (ties[:, 2] >= 2)).sum()) >= 10, ties
                    np.save(os.path.join(OUT, "model_corpus_exact_ties.npy"), ties)
    json.dump(manifest, open(os.path.join(OUT, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    n = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(os.listdir(OUT))} files, {n} bytes -> {OUT}")


if __name__ == "__main__":
    main()

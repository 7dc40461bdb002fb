#!/usr/bin/env python3
"""tests/golden/make_profile_align_golden.py -- writes tests/golden/profile_align_v1 (TEST INFRASTRUCTURE).

1. The model's answers: tests/align_model.py's accept loop over tests/profile_model.py's ProfileWorld on the seeded world of tests/profile_cases.py, for the
   parameter sets profile_cases.derive() reads off the model's own records (answers.npz, sets.json).
2. The world's conditions (profile_cases.conditions): asserted here on what was just written, and again by tests/test_profile_cases.py.
3. The reference binary's `structurealign` (oracle/_ref/bin/foldseek, built by oracle/build_ref_full.sh cpu) on the same world written as databases, with a
   hand-written prefilter result in list order, for six of the sets (profile_cases.REFERENCE_SETS): the result DBs and a MANIFEST of positional arguments
   and full parameter strings.  The databases themselves are not kept: the tests write them again from the seed.

usage: make_profile_align_golden.py            (about a minute; needs the built reference binary for step 3 only, reads nothing else outside the repository)"""
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, HERE)
import make_profile_golden as G  # noqa: E402  the reference binary's path, its full parameter string, the database helpers
import profile_cases as K  # noqa: E402


def reference_par(P):
    """the parameter string of a set; -c and --min-seq-id are floats in the reference: nine digits name one exactly"""
    return G.align_par(**{"-e": repr(float(P["evalThr"])), "-c": "%.9g" % np.float32(P["covThr"]), "--cov-mode": P["covMode"],
                          "--min-seq-id": "%.9g" % np.float32(P["seqIdThr"]), "--seq-id-mode": P["seqIdMode"], "--min-aln-len": P["alnLenThr"],
                          "--max-accept": P["maxAccept"], "--max-rejected": P["maxRejected"], "-a": P["addBacktrace"],
                          "--gap-open": f"aa:{P['gapOpen']},nucl:{P['gapOpen']}", "--gap-extend": f"aa:{P['gapExtend']},nucl:{P['gapExtend']}"})


def model_answers():
    import align_model as A
    live = K.Live()
    sets = K.derive(live)
    answers = {}
    for name, P in sets.items():
        answers[name] = live.run(P)
        print(f"{name}: {A.count_outcomes(answers[name])}", flush=True)
        for q, r in enumerate(answers[name]):              # the order of two records that compare equal in every key is not defined (std::sort)
            assert all(A.compare_hits(r.records[i], r.records[i + 1]) < 0 for i in range(len(r.records) - 1)), (name, q)
            assert "e-value crit" not in r.outcomes
    K.save(sets, answers, {})
    F = K.Frozen()
    K.save(sets, answers, K.measure_facts(F))
    K.conditions(K.Frozen())


def reference_runs():
    if not os.path.exists(G.FS):
        raise SystemExit("build the reference first: bash oracle/build_ref_full.sh cpu")
    F = K.Frozen()
    work = os.path.join(ROOT, "oracle", "_ref_full", "profile_align_work")
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    K.write_world(work)
    manifest = {"reference": "steineggerlab/foldseek, binary from oracle/build_ref_full.sh cpu", "seed": K.SEED,
                "databases": "written by tests/profile_cases.py write_world() from the seed", "runs": {}}
    for name in K.REFERENCE_SETS:
        par = reference_par(F.params(name))
        pos = ["qprof", "tdb", "pref"]
        G.run([G.FS, "structurealign"] + pos + ["aln_" + name] + par, work)
        manifest["runs"]["aln_" + name] = {"module": "structurealign", "positional": pos, "parameters": par, "set": name,
                                           "lines": G.count_lines(os.path.join(work, "aln_" + name))}
    for name in manifest["runs"]:
        for ext in ("", ".index", ".dbtype"):
            shutil.copy(os.path.join(work, name + ext), os.path.join(K.GOLD, name + ext))
    json.dump(manifest, open(os.path.join(K.GOLD, "MANIFEST.json"), "w"), indent=1, sort_keys=True)
    print({k: v["lines"] for k, v in manifest["runs"].items()})


def main():
    if "ref-only" not in sys.argv[1:]:
        model_answers()
    reference_runs()
    for f in sorted(os.listdir(K.GOLD)):
        print(f, os.path.getsize(os.path.join(K.GOLD, f)))


if __name__ == "__main__":
    main()

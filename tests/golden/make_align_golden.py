#!/usr/bin/env python3
"""tests/golden/make_align_golden.py -- writes tests/golden/align_v1 (TEST INFRASTRUCTURE).

For both alignment types: runs the independent model of structurealign's accept loop (tests/align_model.py) on the seeded world of tests/align_cases.py
with the default parameters, derives the parameter sets from the model's own records (align_cases.derive: thresholds AT a named hit's value and one
representable number beyond), runs the model for every set and freezes records, CIGARs, outcomes, Smith-Waterman records and the sets themselves
(answers_t<type>.npz, sets_t<type>.json).  With `scop` it first holds the model to EVERY query of every frozen structurealign run of the reference binary
(tests/golden/scop_v1, ca_v1, tm_v1: the lists of tests/test_align_model.py, of which the CPU suite re-runs a stated sample).

usage: make_align_golden.py [scop]        (pure Python; about ten minutes, the two alignment types in parallel)"""
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))


def one(atype):
    import align_cases as K
    import align_model as A
    live = K.Live(atype)
    sets = K.derive(live.run, live.evalue_fwd)
    answers = {}
    for name, P in sets.items():
        answers[name] = live.run(P)
        print(f"t{atype} {name}: {A.count_outcomes(answers[name])} alt {sorted((why, sum(1 for r in answers[name] for e in r.alt_ends if e[2] == why)) for why in A.ALT_ENDS)}", flush=True)
        for q, r in enumerate(answers[name]):          # the order of two records that compare equal in every key is not defined (std::sort)
            cmp_ = A.compare_structure_bits if P["structureBits"] else A.compare_hits
            assert all(cmp_(r.records[i], r.records[i + 1]) < 0 for i in range(len(r.records) - 1)), (name, q)
    K.save(atype, sets, answers)
    return atype


def ca(_):
    import align_cases as K
    import align_model as A
    live = K.LiveCa()
    sets = K.ca_sets()
    answers = {}
    for name, P in sets.items():
        answers[name] = live.run(P)
        print(f"ca {name}: {A.count_outcomes(answers[name])}", flush=True)
        for q, r in enumerate(answers[name]):
            cmp_ = A.compare_structure_bits if P["structureBits"] else A.compare_hits
            assert all(cmp_(r.records[i], r.records[i + 1]) < 0 for i in range(len(r.records) - 1)), (name, q)
    K.save("ca", sets, answers, seed=K.CA_SEED)
    return "ca"


def main():
    if "scop" in sys.argv[1:]:
        import test_align_model as T
        T.check_reference_runs(sample=None)
    with Pool(3) as pool:
        r = [pool.apply_async(one, (2,)), pool.apply_async(one, (0,)), pool.apply_async(ca, (0,))]
        print([x.get() for x in r])
    import align_cases as K
    # the census as a document: per parameter set what ended how many hits of the lists, and how the searches for alternative alignments ended
    with open(os.path.join(K.GOLD, "CENSUS.md"), "w") as f:
        f.write("# Outcome counts of the model per parameter set (written by make_align_golden.py)\n")
        for tag, title in ((2, "seeded world, 3Di + AA"), (0, "seeded world, 3Di only"), ("ca", "twelve example structures, 3Di + AA")):
            F = K.Frozen(tag)
            f.write(f"\n## {title}: {len(F.n)} lists, {sum(F.n)} pairs\n\n")
            for name in F.names:
                ends = {}
                for _q, _k, _n, why in F.alt_ends(name):
                    ends[why] = ends.get(why, 0) + 1
                c = F.count(name)
                f.write(f"- `{name}`: " + ", ".join(f"{o} {c[o]}" for o in F.outcome_names if o in c)
                        + ("; alternatives ended by: " + ", ".join(f"{w} {n}" for w, n in sorted(ends.items())) if ends else "") + "\n")
    for f in sorted(os.listdir(K.GOLD)):
        print(f, os.path.getsize(os.path.join(K.GOLD, f)))


if __name__ == "__main__":
    main()

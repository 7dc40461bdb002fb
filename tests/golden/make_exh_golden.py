"""Generator of tests/golden/exh_v1/{answers,sets}_t{2,0}: tests/align_model.py over ALL targets of tests/align_cases.py's world for the parameter
sets of tests/exh_cases.py.  No GPU (needs oracle/libfso.so for the e-value network and the matrices, as the model always does).  The reference binary's
result databases in the same directory (ref_*) are written by tests/golden/make_exh_ref_golden.py.
Run from the repository root: python tests/golden/make_exh_golden.py"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import exh_cases as E  # noqa: E402


def main():
    t0 = time.time()
    for atype in E.ATYPES:
        live = E.Live(atype)
        sets = E.derive(live)
        for name, P in sets.items():
            for q in range(E.n_queries()):
                live.query(q, P)
            print(f"t{atype} {name}: {time.time() - t0:.0f} s", flush=True)
        E.save(atype, sets, live)
    print("done", flush=True)


if __name__ == "__main__":
    main()

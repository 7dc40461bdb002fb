"""Generator of tests/golden/sw_v1/answers.npz: the records of tests/sw_model.py for every pair of every call of tests/sw_cases.py (inputs are rebuilt
from seeds; only digests and records are stored).  No GPU, no reference needed.  Run from the repository root: python tests/golden/make_sw_golden.py"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sw_cases as K  # noqa: E402


def main():
    K.LIVE = True
    K.store().clear()
    t0 = time.time()
    for call in K.all_calls():
        for d in call.dirs:
            K.call_want(call, d)
        print(f"{call.name}: {len(K.store())} pairs, {time.time() - t0:.0f} s", flush=True)
    m3, mA, q, t3, tA = K.exact_32767()
    for rev in (False, True):
        K.want(m3, mA, q, rev, [K.target(K.exact_db(), i) for i in range(K.exact_db().n)])
    K.save_store()
    print(f"{len(K.store())} records -> {K.ANSWERS} ({os.path.getsize(K.ANSWERS)} bytes)")


if __name__ == "__main__":
    main()

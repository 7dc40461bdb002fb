"""Generator of tests/golden/db_v1/answers.npz: what the independent models (tests/gapless_model.py, tests/sw_model.py, tests/diag_model.py) answer on the
`longest` shape of tests/db_cases.py, whose targets reach FSGPU_MAX_SEQ_LEN -- a Smith-Waterman pass of the model over 65535 columns takes several seconds.
Inputs are rebuilt from seeds; only the answers are stored.  No GPU, no reference needed.  Run from the repository root:
python tests/golden/make_db_golden.py"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import db_cases as D  # noqa: E402


def main():
    D.LIVE = True
    out, t0 = {}, time.time()
    for key, compute in D.frozen_keys():
        r = compute()
        out[key] = np.array([[int(x[f]) for f in D.SW_FIELDS] for x in r], np.int32) if "/sw/" in key else np.asarray(r, np.int32)
        print(f"{key}: {out[key].shape}, {time.time() - t0:.0f} s", flush=True)
    os.makedirs(D.GOLD, exist_ok=True)
    np.savez_compressed(D.ANSWERS, **out)
    print(f"{len(out)} arrays -> {D.ANSWERS} ({os.path.getsize(D.ANSWERS)} bytes)")


if __name__ == "__main__":
    main()

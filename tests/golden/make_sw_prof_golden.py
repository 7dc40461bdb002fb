"""Freezes the answers of tests/sw_model.py for the world of tests/sw_prof_cases.py into tests/golden/sw_prof_v1/answers.npz.
Run from the repository root: python tests/golden/make_sw_prof_golden.py.  Needs numpy alone; nothing of foldseek_amd is called."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import sw_prof_cases as K  # noqa: E402

if __name__ == "__main__":
    t0 = time.time()
    ans = K.compute_all()
    K.save(ans)
    pairs = sum(len(v[1]) for v in ans.values())
    print(f"{len(ans)} queries, {pairs} pairs per direction, {time.time() - t0:.1f} s -> {K.ANSWERS} ({os.path.getsize(K.ANSWERS)} bytes)")

"""Generator of tests/golden/scan_v1/answers.npz: the records of tests/sw_model.py for every (query, target) pair of tests/scan_cases.py under every
configuration, and for the saturation case.  No GPU, no reference needed.  Run from the repository root: python tests/golden/make_scan_golden.py"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scan_cases as S  # noqa: E402


def main():
    t0 = time.time()
    out = {"digest": np.array(S.digest())}
    for cfg in S.CONFIGS:
        recs = [S.live_records(cfg, qi) for qi in range(len(S.Q_LENGTHS))]
        out[S.config_name(cfg)] = np.array([[[int(r[f]) for f in S.FIELDS] for r in rs] for rs in recs], np.int32)
        print(f"{S.config_name(cfg)}: {time.time() - t0:.0f} s", flush=True)
    out["sat"] = np.array([[int(r[f]) for f in S.FIELDS] for r in S.live_sat()], np.int32)
    os.makedirs(S.GOLD, exist_ok=True)
    np.savez_compressed(S.ANSWERS, **out)
    print(f"{S.db().n} targets -> {S.ANSWERS} ({os.path.getsize(S.ANSWERS)} bytes)")


if __name__ == "__main__":
    main()

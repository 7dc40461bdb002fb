"""Diagonal rescoring without a GPU: the independent model (tests/diag_model.py) against what the REFERENCE BINARY's structurerescorediagonal wrote on
the example structures (tests/golden/scop_v1: resc_t2_a, resc_t0_a_sid1, resc_t2_clu from the prefilter lines of pref_kmer_defined).  For every prefilter
line that survived the run's e-value / coverage gates the model gives exactly the printed score (forward - reversed), the four positions and, where the run
wrote backtraces, the alignment length.  The kernel is held to this model by tests/test_diag_gpu.py."""
import os

import numpy as np
import pytest

import diag_model as M
import helpers
from foldseek_amd import api

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scop_v1")


@pytest.fixture(scope="module")
def scop():
    aa, ss = M.read_db(os.path.join(GOLD, "db")), M.read_db(os.path.join(GOLD, "db_ss"))
    assert sorted(aa) == sorted(ss)
    seqs = {k: (M.encode(aa[k].decode().rstrip("\n")), M.encode(ss[k].decode().rstrip("\n"))) for k in aa}
    assert all(len(a) == len(s) > 0 for a, s in seqs.values())
    pref = {}
    for q, entry in M.read_db(os.path.join(GOLD, "pref_kmer_defined")).items():
        pref[q] = [(int(f[0]), int(f[2])) for f in (l.split() for l in entry.decode().splitlines())]
    return seqs, pref


# run -> (bit factor of the AA matrix, backtraces written, lines the reference alone is known to provide)
RUNS = {"resc_t2_a": (1.4, True, 560), "resc_t0_a_sid1": (0.0, True, 454), "resc_t2_clu": (1.4, False, 138)}


@pytest.mark.parametrize("run", sorted(RUNS))
def test_model_reproduces_reference_rescorediagonal(scop, run):
    seqs, pref = scop
    aa_factor, has_bt, at_least = RUNS[run]
    m3 = helpers.o_submat("MAT3DI", 2.1)[0].reshape(21, 21).tolist()
    mA = helpers.o_submat("BLOSUM62", aa_factor)[0].reshape(21, 21).tolist()
    out = M.read_db(os.path.join(GOLD, run))
    compared = negative = 0
    for q in sorted(pref):
        lines = {}
        for l in out.get(q, b"").decode().splitlines():
            f = l.split()
            assert int(f[0]) not in lines
            lines[int(f[0])] = f
        assert len({t for t, _ in pref[q]}) == len(pref[q])
        for t, d in pref[q]:
            if t not in lines:
                continue                                   # dropped by the run's e-value / coverage / sequence identity gates
            f = lines[t]
            r = M.rescore(seqs[q][0], seqs[q][1], seqs[t][0], seqs[t][1], d, m3, mA)
            assert r["status"] == M.OK, (run, q, t, d, r)
            score, qs, qe, ds, de, aln = M.module_columns(r, d)
            want = (int(f[1]), int(f[4]), int(f[5]), int(f[7]), int(f[8]))
            assert (score, qs, qe, ds, de) == want, (run, q, t, d, (score, qs, qe, ds, de), want)
            assert (int(f[6]), int(f[9])) == (len(seqs[q][0]), len(seqs[t][0]))
            if has_bt:
                assert f[10] == "%dM" % aln, (run, q, t, d, aln, f[10])
            compared += 1
            negative += d < 0
    print(f"{run}: {compared} lines compared, {negative} on negative diagonals")
    assert compared >= at_least
    if run == "resc_t2_a":
        assert negative >= 80


def test_scan_tie_rules():
    """the reference loop on hand-made cells: reset on <= 0, a new maximum only on >"""
    assert M.scan([]) == (0, 0, 0)
    assert M.scan([-1, -2]) == (0, 0, 0)
    assert M.scan([1, -1, 1]) == (1, 0, 0)                 # back to exactly 0, the equal second maximum is not taken
    assert M.scan([1, -1, 2]) == (2, 2, 2)                 # ... and the run restarts AFTER the zero
    assert M.scan([2, -1, 1, -2, 3]) == (3, 4, 4)
    assert M.scan([2, -1, 1]) == (2, 0, 0)                 # 2 reached twice: the first stays
    assert M.scan([0, 0, 3, 0]) == (3, 2, 2)
    assert M.scan_events([1, -1, 1]) == (True, 2, 0)
    assert M.scan_events([2, -3, 1]) == (False, 1, 0)
    assert M.scan_events([-1, -1]) == (False, 0, -1)


def test_api_binds_the_two_entries():
    names = api.exported_symbols()
    assert "fsgpu_diag_rescore" in names and "fsgpu_sw_batch_seqs" in names
    L = api.lib()
    assert hasattr(L, "fsgpu_diag_rescore") and hasattr(L, "fsgpu_sw_batch_seqs")
    assert api.DIAG_PAIR_DT.itemsize == 12 and api.DIAG_PAIR_DT.names == ("query", "target", "diagonal")
    assert api.DIAG_RES_DT.itemsize == 32 and api.DIAG_RES_DT.names == M.FIELDS
    assert (api.FSGPU_DIAG_OK, api.FSGPU_DIAG_NO_OVERLAP, api.FSGPU_DIAG_UNDEFINED, api.FSGPU_DIAG_BAD_ID) == (M.OK, M.NO_OVERLAP, M.UNDEFINED, M.BAD_ID)
    assert hasattr(api.Context, "diag_rescore") and hasattr(api.Context, "sw_batch_seqs")

"""fshost_evalue_score_cutoff -- the first e-value gate of alignStructure (structurealign.cpp:55-59) as a score cutoff -- against a brute-force scan of
fshost_evalue_corr over ALL 32768 scores, on a grid of (lambda, mu, threshold) whose cutoffs fall into each of computePvalue's three branches (h > 10,
h < -2.5, between), with threshold 0, a threshold so large that the cutoff is 0, and thresholds no score passes.  No GPU."""
import math
import subprocess

import numpy as np
import pytest

from foldseek_amd import api

RESIDUES = 5_000_000


@pytest.fixture(scope="module")
def evaluer():
    return api.Evaluer(RESIDUES)


def brute(ev, lam, mu):
    """the e-value of every score 0 .. 32767, one library call each"""
    return np.array([ev.evalue_corr(s, lam, mu) for s in range(32768)], np.float64)


def cutoff_of(e, thr):
    """the smallest score the gate `e-value > thr -> reject` lets through (a NaN is let through), 32767 when there is none"""
    ok = ~(e > thr)
    return int(np.argmax(ok)) if ok.any() else 32767


def branch_of(lam, mu, s):
    h = lam * (s - mu)
    return "linear" if h > 10 else "double exponential" if h < -2.5 else "between"


# (lambda, mu): the network's range for real queries is lambda 0.1 .. 0.25, mu -3 .. 60; the others push a cutoff into every branch
GRID = [(0.175, 10.0), (0.12, 55.0), (0.25, -2.5), (0.05, 300.0), (0.9, 20.0), (0.0004, 100.0), (0.175, 20000.0)]


@pytest.mark.parametrize("lam,mu", GRID)
def test_cutoff_equals_the_brute_force_scan(evaluer, lam, mu):
    e = brute(evaluer, lam, mu)
    # thresholds: 0, the defaults, a threshold so large that every score passes, one no score reaches (negative), and the e-values of scores picked from
    # each branch of computePvalue -- AT the value and one representable number below it (the named score then just fails)
    picks = {}
    for s in (0, 1, 2, 5, 17, 40, 77, 150, 333, 1000, 5000, 20000, 32766, 32767):
        picks.setdefault(branch_of(lam, mu, s), []).append(s)
    thresholds = [0.0, 10.0, 1e-3, 1e-30, 1e300, -1.0, float("inf")]
    for ss in picks.values():
        for s in ss[:3] + ss[-1:]:
            if math.isfinite(e[s]):
                thresholds += [float(e[s]), float(np.nextafter(e[s], -np.inf))]
    seen = set()
    for thr in thresholds:
        want = cutoff_of(e, thr)
        got = evaluer.score_cutoff(lam, mu, thr)
        assert got == want, (lam, mu, thr, got, want)
        # what the cutoff is for: every score below it is rejected by the gate, the cutoff itself is not (unless nothing passes)
        assert (e[:got] > thr).all()
        if (~(e > thr)).any():
            assert not e[got] > thr
            seen.add(branch_of(lam, mu, got))
    assert seen, "no threshold of this pair had a passing score"
    assert evaluer.score_cutoff(lam, mu, 1e300) == 0                      # a threshold so large the cutoff is 0
    assert evaluer.score_cutoff(lam, mu, -1.0) == 32767                   # no passing score


def test_cutoffs_of_the_grid_reach_all_three_branches(evaluer):
    seen = set()
    for lam, mu in GRID:
        e = brute(evaluer, lam, mu)
        # the usual thresholds, and the e-value of score 5, which for the pairs with a large mu lies in the double-exponential branch
        for thr in (10.0, 1e-3, 1e-30, float(e[5])):
            c = evaluer.score_cutoff(lam, mu, thr)
            assert c == cutoff_of(e, thr)
            if c < 32767:
                seen.add(branch_of(lam, mu, c))
    assert seen == {"linear", "double exponential", "between"}, seen


def test_cutoff_with_the_networks_own_parameters(evaluer):
    rng = np.random.default_rng(5)
    for L in (30, 150, 700):
        lam, mu = evaluer.mu_lambda(rng.integers(0, 20, L).astype(np.uint8))
        e = brute(evaluer, lam, mu)
        for thr in (10.0, 1e-3):
            assert evaluer.score_cutoff(lam, mu, thr) == cutoff_of(e, thr)
            assert 0 < cutoff_of(e, thr) < 2000


def test_symbol_resolves():
    L = api.lib()
    assert L.fshost_evalue_score_cutoff.argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", api.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert " T fshost_evalue_score_cutoff\n" in out
    assert callable(api.Evaluer.score_cutoff)

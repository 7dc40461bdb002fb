"""tests/gapless_model.py held to what already stands (no GPU): the C oracle's striped uint8 scan and selection, the compiled reference's
ungapped alignment where oracle/_ref is built, and -- for profiles no matrix produces -- a second brute-force form of its own."""
import numpy as np
import pytest

import gapless_model as gm
import helpers
import oracle_lib
from foldseek_amd import api, synth


def _db_with_edges(n=160, seed=31):
    """a seeded database with planted homologs, masked stretches, an all-X target, an all-masked target and targets of 1..3 residues"""
    q3, qa = synth.make_queries(4, seed=seed, mean_len=90, lo=1, hi=200)
    q3[0], qa[0] = q3[0][:1], qa[0][:1]
    q3[1], qa[1] = np.resize(q3[1], 17), np.resize(qa[1], 17)
    db = synth.make_db(n, (q3, qa), seed=seed + 1, homologs_per_query=10, mask_frac=0.05, mean_len=80, lo=1, hi=300)
    d3 = db.data3di.copy()
    for t, fill in ((db.n - 1, 20), (db.n - 2, 32 + 7), (db.n // 2, 52)):          # all X, all masked, all masked X
        d3[db.offsets[t]:db.offsets[t] + db.lengths[t]] = fill
    return synth.PaddedDB(d3, db.dataaa, db.offsets, db.lengths), q3


@pytest.fixture(scope="module")
def world():
    db, q3 = _db_with_edges()
    return db, q3, gm.pack(db)


@pytest.mark.parametrize("comp_bias", [True, False])
def test_scores_equal_the_oracle(world, comp_bias):
    db, q3, packed = world
    assert int(db.lengths.min()) == 1 and (db.data3di >= 32).any()
    m = api.Matrix(0, 2.0)
    spread = set()
    for q in q3:
        pssm, cap = api.prefilter_profile(m, q, comp_bias, 0.15)
        got = gm.scores(pssm, cap, packed)
        want = helpers.o_ungapped_scores(q, db, comp_bias)
        assert (got == want).all(), (len(q), np.flatnonzero(got != want)[:10])
        assert (gm.scores(pssm, cap, db) == got).all()                             # packed or not: the same
        spread |= set(got.tolist())
    assert len(spread) > 20 and max(spread) > 100                                  # homologs score, background does not


@pytest.mark.parametrize("comp_bias", [True, False])
def test_scores_equal_the_compiled_reference(world, comp_bias):
    ref = oracle_lib.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    db, q3, packed = world
    m = api.Matrix(0, 2.0)
    for q in q3:
        pssm, cap = api.prefilter_profile(m, q, comp_bias, 0.15)
        want = np.zeros(db.n, np.int32)
        ref.ref_ungapped(np.ascontiguousarray(q, np.uint8), len(q), int(comp_bias), 0.15, db.data3di, np.ascontiguousarray(db.offsets[:-1], np.int64),
                         np.ascontiguousarray(db.lengths, np.int32), db.n, 1, want)
        got = gm.scores(pssm, cap, packed)
        assert (got == want).all(), (len(q), np.flatnonzero(got != want)[:10])


def test_select_equals_the_oracle():
    rng = np.random.default_rng(5)
    n = 500
    vectors = [rng.integers(0, 6, n) * 40,                       # six values: every cut falls into a tie group
               np.full(n, 77), np.zeros(n, np.int64),
               rng.integers(0, 256, n)]
    for s in vectors:
        s = s.astype(np.int32)
        low = int(np.argmin(s))
        for min_score in (-1, 30, 119, 255):
            for identity in (-1, low, n - 1):
                for max_res in (1, n - 1, n, n + 7):
                    got = gm.select(s, min_score, identity, max_res)
                    want = helpers.o_prefilter_select(s, min_score, identity, max_res)
                    assert len(got) == len(want) and (got["id"] == want["key"]).all() and (got["score"] == want["score"]).all(), \
                        (min_score, identity, max_res)
    # an identity id that fails the score filter is kept, after everything that passed
    s = np.array([50, 10, 50, 31], np.int32)
    assert gm.select(s, 30, 1, 10).tolist() == [(0, 50), (2, 50), (3, 31), (1, 10)]
    assert gm.select(s, 30, 1, 3).tolist() == [(0, 50), (2, 50), (3, 31)]
    assert gm.select(s, 30, -1, 10).tolist() == [(0, 50), (2, 50), (3, 31)]


def _crafted(rng, L, kind):
    if kind == "all127":
        return np.full((21, L), 127, np.int8)
    return rng.choice(np.array([-128, -1, 0, 1, 127], np.int8), size=(21, L), p=[0.3, 0.2, 0.1, 0.2, 0.2] if kind == "mixed" else None)


@pytest.mark.parametrize("kind", ["mixed", "uniform", "all127", "int8"])
def test_crafted_profiles_equal_the_brute_force_form(kind):
    """arbitrary int8 entries, which no substitution matrix gives and the oracle's biased uint8 profile cannot hold: the vectorised form against
    the whole DP matrix in Python integers, every clamp of the cap"""
    rng = np.random.default_rng(len(kind))
    lens = [1, 2, 3, 5, 16, 17, 23, 40, 40, 37]
    targets = [rng.integers(0, 21, T).astype(np.uint8) for T in lens]
    targets[4][::3] += 32                                                          # masked letters read as X
    targets[8][:] = 20
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((np.array(lens) + 3) // 4 * 4)
    d3 = np.full(off[-1], 20, np.uint8)
    for k, t in enumerate(targets):
        d3[off[k]:off[k] + len(t)] = t
    db = synth.PaddedDB(d3, None, off, np.array(lens, np.int32))
    for L in (1, 7, 16, 17, 40):
        pssm = rng.integers(-128, 128, (21, L)).astype(np.int8) if kind == "int8" else _crafted(rng, L, kind)
        raw = gm.best_runs(pssm, db)
        for cap in (255, 40, 1, 0, -5, 300):
            got = gm.scores(pssm, cap, db)
            assert (got == gm.scores_brute(pssm, cap, targets)).all(), (L, cap)
            assert (got == np.minimum(raw, max(0, min(cap, 255)))).all()
        if kind == "all127":
            assert (raw == 127 * np.minimum(L, np.array(lens))).all()               # the longest diagonal, every cell 127

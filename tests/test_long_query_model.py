"""The inputs of the long-query tests and the models at those lengths (no GPU).  tests/long_query_cases.py plants targets where a query of up to 65535
residues makes the kernels do what they do at no shorter length; here (a) the conditions those inputs must meet are asserted on the models alone, with the
counts of every kind, (b) gapless_model and sw_model are held to the C oracle and, where oracle/_ref is built, to the compiled reference at L = 32769 and
65535, (c) the host's profile builders equal the oracle's arrays at L = 32768 and 65535."""
import numpy as np
import pytest

import gapless_model as gm
import helpers
import long_query_cases as LC
import oracle_lib
import sw_cases as K
from foldseek_amd import api, synth

MODEL_L = (32769, 65535)


def _rec(r):
    return int(r["score"]), int(r["qEnd"]), int(r["dbEnd"]), int(r["word"])


def _db_of(seqs3):
    lens = np.array([len(x) for x in seqs3], np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3 = np.full(int(off[-1]), 20, np.uint8)
    for k, s in enumerate(seqs3):
        d3[off[k]:off[k] + lens[k]] = s
    return synth.PaddedDB(d3, None, off, lens)


# ---- (a) conditions and counts ---------------------------------------------------------------------------------------------------------------------------
def test_the_tile_rule_gives_the_shapes_the_lengths_were_chosen_for():
    assert LC.scan_tiles(1025) == (3, 352) and LC.scan_tiles(896) == (1, 896) and LC.scan_tiles(897) == (2, 464)
    assert [LC.scan_tiles(L) for L in LC.LQ] == [(17, 496), (64, 512), (64, 512), (65, 512), (128, 512), (128, 512)]
    # k_sw: tiles of 512 rows; the rows of the last one
    assert [(-(-L // 512), L - (-(-L // 512) - 1) * 512) for L in LC.LQ] == [(17, 1), (64, 511), (64, 512), (65, 1), (128, 510), (128, 511)]


@pytest.mark.parametrize("L", LC.LQ)
def test_scan_targets_meet_their_conditions(L):
    w = LC.world(L)
    pssm, cap = LC.scan_profile(L)
    cap = gm.clamp(cap)
    want = w.scan_want()
    scan = w.ids("scan")
    planted_rows = {w.info[i]["p"] for i in scan}
    assert planted_rows == set(LC.scan_borders(L)) | {0, L - 1} | ({32768} if L > 32768 else set())
    assert len(LC.scan_borders(L)) == LC.scan_tiles(L)[0] - 1 and len(scan) == len(planted_rows)
    halves = []
    for i in scan:
        t, half = gm.target_codes(w.db, i), w.info[i]["w"]
        assert len(t) == 2 * half and (t == LC.query(L)[0][w.info[i]["lo"]:][:2 * half]).all()
        assert w.info[i]["lo"] <= w.info[i]["p"] < w.info[i]["lo"] + 2 * half
        halves += [t[:half], t[half:]]
    alone = gm.scores(pssm, cap, _db_of(halves))
    for k, i in enumerate(scan):
        assert want[i] < cap, ("a planted scan target reaches the cap", L, w.info[i], int(want[i]), cap)
        assert want[i] > max(alone[2 * k], alone[2 * k + 1]), ("a half alone scores as much", L, w.info[i], int(want[i]), alone[2 * k:2 * k + 2])
    plain = w.ids("plain", "allX")
    assert len(plain) == 60 and len(w.ids("allX")) == 1
    assert sum(int(want[i] >= cap) for i in plain) <= len(plain) // 10
    lens = w.db.lengths[plain]
    assert lens.min() == 1 and lens.max() == 300 and (w.db.data3di >= 32).any()
    assert w.db.n == len(scan) + len(w.ids("sw_fwd", "sw_rev", "sat")) + 60
    hits = gm.select(want, 30, -1, 1000)
    assert set(scan) <= set(hits["id"].tolist()) and 0 < len(hits) < w.db.n           # the planted ones pass the filter, not everything does


@pytest.mark.parametrize("L", LC.LQ)
def test_sw_targets_meet_their_conditions(L):
    w = LC.world(L)
    mult = list(range(512, L, 512))
    must = {mult[0], mult[-1]} | ({63 * 512, 64 * 512} & set(mult))
    n_sat = 2 if L > 32769 else 1                        # at 32769 the window up to row L - 1 is the one across row 32768
    for rev, kind in ((False, "sw_fwd"), (True, "sw_rev")):
        ids = w.ids(kind)
        across = {w.info[i]["m"] for i in ids} - {None}
        assert must <= across and len(across) == len(must) + 8 and len(ids) == len(across) + 2
        assert sum(w.info[i]["s"] == 0 for i in ids) == 1 and sum(w.info[i]["end"] == L - 1 and w.info[i]["m"] is None for i in ids) == 1
        recs = w.sw_want(2, rev, ids)
        for i, r in zip(ids, recs):
            info = w.info[i]
            assert 40 <= info["n"] <= 200 or info["m"] == mult[-1], info              # a window across the last multiple ends with the query
            assert int(w.db.lengths[i]) == info["n"] - 3 and _rec(r)[1:] == (info["end"], info["n"] - 4, 1), (L, rev, info, r)
            first, score = LC.first_aligned_row(L, 2, rev, *K.target(w.db, i), r)
            assert score == int(r["score"]) and abs(first - info["s"]) <= 8, (L, rev, info, r, first, score)     # the whole window: the gap is part of it
            if info["m"] is not None:                         # (the windows at row 0 and up to row L - 1 are too short to reach a second tile)
                assert first // 512 + 1 == int(r["qEnd"]) // 512 == info["m"] // 512, (L, rev, info, r, first)
        assert any(int(r["qEnd"]) == L - 1 for r in recs)
    sat = w.ids("sat")
    assert len(sat) == n_sat
    recs = w.sw_want(2, False, sat)
    ends = set()
    for i, r in zip(sat, recs):
        assert int(w.db.lengths[i]) == LC.SAT_LEN
        assert _rec(r)[1:] == (w.info[i]["end"], LC.SAT_LEN - 1, 2) and int(r["score"]) > 32767, (L, w.info[i], r)
        ends.add(int(r["qEnd"]))
    assert L - 1 in ends and (L < 32769 or any(w.info[i]["s"] < 32768 <= w.info[i]["end"] for i in sat))


# ---- (b) the models at these lengths ---------------------------------------------------------------------------------------------------------------------
def _model_ids(w):
    return sorted(w.ids("scan", "sw_fwd", "sw_rev", "sat") + w.plain_sample())


@pytest.mark.parametrize("L", MODEL_L)
def test_models_equal_the_oracle(L):
    w = LC.world(L)
    ids = _model_ids(w)
    assert len(ids) >= w.db.n - 60 + 12
    q3, qa = LC.query(L)
    want = helpers.o_ungapped_scores(q3, w.db, True)
    got = w.scan_want()
    assert (got[ids] == want[ids]).all(), (L, [i for i in ids if got[i] != want[i]][:10])
    for rev in (False, True):
        s3, sa = (q3[::-1].copy(), qa[::-1].copy()) if rev else (q3, qa)
        pA, p3, _, _ = helpers.o_align_profiles(sa, s3, 2)
        recs = w.sw_want(2, rev, ids)
        for i, r in zip(ids, recs):
            ta, t3 = helpers.target_seqs(w.db, i)
            assert _rec(r) == _rec(helpers.o_sw(pA, p3, L, ta, t3)), (L, rev, i, w.kind[i], w.info[i])


@pytest.mark.parametrize("L", MODEL_L)
def test_models_equal_the_compiled_reference(L):
    R = oracle_lib.load_ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    from oracle_lib import REFSW_DT
    w = LC.world(L)
    db, ids = w.db, _model_ids(w)
    q3, qa = LC.query(L)
    want = np.zeros(db.n, np.int32)
    R.ref_ungapped(np.ascontiguousarray(q3, np.uint8), L, 1, 0.15, db.data3di, np.ascontiguousarray(db.offsets[:-1], np.int64),
                   np.ascontiguousarray(db.lengths, np.int32), db.n, 1, want)
    got = w.scan_want()
    assert (got[ids] == want[ids]).all(), (L, [i for i in ids if got[i] != want[i]][:10])
    t3 = np.where(db.data3di >= 32, db.data3di - 32, db.data3di).astype(np.uint8)
    fw, rv = np.zeros(db.n, REFSW_DT), np.zeros(db.n, REFSW_DT)
    R.ref_structure_align(qa, q3, L, 2, 1, 0.5, 10, 1, db.dataaa, t3, db.offsets[:-1].copy(), db.lengths, db.n, db.residues, 10.0, 0, 1, fw.ctypes.data,
                          rv.ctypes.data, None, None, 0)
    for rev, ref in ((False, fw), (True, rv)):
        recs = w.sw_want(2, rev, ids)
        for i, r in zip(ids, recs):
            assert _rec(r) == _rec(ref[i]), (L, rev, i, w.kind[i], w.info[i])


# ---- (c) the host's profile builders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [32768, 65535])
def test_host_profiles_equal_the_oracle(L):
    O = helpers.oracle()
    q3, qa = LC.query(L)
    for which, name, bf, scale, seq in ((0, "MAT3DI", 2.0, 0.15, q3), (1, "BLOSUM62", 1.4, 1.0, qa), (1, "BLOSUM62", 1.4, 0.5, q3)):
        sub, pb = helpers.o_submat(name, bf)
        assert (api.Matrix(which, bf).comp_bias(seq, scale) == helpers.o_round_bias(sub, pb, seq, scale)[0]).all(), (L, name, scale)
    sub, pb = helpers.o_submat("MAT3DI", 2.0)
    pssm, cap = LC.scan_profile(L)
    cb = helpers.o_round_bias(sub, pb, q3, 0.15)[1]
    assert cap == 255 - O.fso_ungapped_bias(sub.astype(np.int8), 21, cb, L)
    assert (pssm.astype(np.int32) == sub.reshape(21, 21)[:, q3].astype(np.int32) + cb.astype(np.int32)[None, :]).all()
    for atype in (2, 0):
        mA, m3 = LC.host_matrices(atype)
        for rev in (False, True):
            s3, sa = (q3[::-1].copy(), qa[::-1].copy()) if rev else (q3, qa)
            pA, p3, cbA, cbS = api.align_profiles(mA, m3, sa, s3, True, 0.5)
            oA, o3, ocA, ocS = helpers.o_align_profiles(sa, s3, atype)
            assert (pA.ravel() == oA).all() and (p3.ravel() == o3).all() and (cbA == ocA).all() and (cbS == ocS).all(), (L, atype, rev)
            # ... and sw_model.profile states the same tables from the matrix and the bias vector
            have = LC.sw_profiles(L, atype)
            assert (have[2 if rev else 0] == pA).all() and (have[3 if rev else 1] == p3).all(), (L, atype, rev)

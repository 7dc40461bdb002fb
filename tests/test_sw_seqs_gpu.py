"""fsgpu_sw_batch_seqs (the structure SW on EXPLICIT target sequences, what structurealign --alt-ali re-aligns) called directly through
Context.sw_batch_seqs against the C oracle (helpers.o_sw) on the same profiles and sequences: score, qEnd, dbEnd and word of both directions.  The targets
of one call lie unpadded and back to back, so most of them start at offsets that are no multiple of 4."""
import numpy as np
import pytest

import helpers
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

FIELDS = ("score", "qEnd", "dbEnd", "word")
TARGET_LENGTHS = (1, 2, 3, 63, 64, 65, 500, 1500, 7, 33, 100, 129, 255, 257, 301, 17, 90, 777, 5, 41, 640)      # + all-X, X in the middle, two relatives


@pytest.fixture(scope="module")
def env():
    """a context with a small resident DB (the entry needs one loaded, and the state tests go back to it) and the two matrices"""
    q3, qa = synth.make_queries(2, seed=31, mean_len=150, lo=100, hi=220)
    db = synth.make_db(120, (q3, qa), seed=32, homologs_per_query=15, lo=10, hi=600, mask_frac=0.03)
    ctx = api.Context(0)
    ctx.load_db(db)
    yield ctx, db, q3, qa
    ctx.close()


def _profiles(qa, q3, atype=2, comp_bias=True):
    mAA, m3 = api.Matrix(1, 1.4 if atype == 2 else 0.0), api.Matrix(0, 2.1)
    pAf, p3f, _, _ = api.align_profiles(mAA, m3, qa, q3, comp_bias, 0.5)
    pAr, p3r, _, _ = api.align_profiles(mAA, m3, qa[::-1].copy(), q3[::-1].copy(), comp_bias, 0.5)
    return pAf, p3f, pAr, p3r


def _noisy(rng, s, rate):
    return np.where(rng.random(len(s)) < rate, rng.integers(0, 20, size=len(s)), s).astype(np.uint8)


def _redrawn(rng, s, n):
    out = s.copy()
    out[rng.choice(len(s), size=n, replace=False)] = rng.integers(0, 20, size=n)
    return out


def _oracle(prof, L, tA, t3, go=10, ge=1):
    """(fwd, rev) SW_DT arrays of helpers.o_sw, the AA half zero where the call runs without AA"""
    pAf, p3f, pAr, p3r = prof
    zero = np.zeros_like(p3f)
    fwd, rev = np.zeros(len(t3), api.SW_DT), np.zeros(len(t3), api.SW_DT)
    for k in range(len(t3)):
        ta = tA[k] if tA is not None else np.zeros(len(t3[k]), np.uint8)
        for out, pA, p3 in ((fwd, pAf, p3f), (rev, pAr, p3r)):
            w = helpers.o_sw(pA if pA is not None else zero, p3, L, ta, t3[k], go, ge)
            out[k] = tuple(int(w[f]) for f in FIELDS)
    return fwd, rev


def _same(got, want, what):
    for d, (g, w) in enumerate(zip(got, want)):
        for f in FIELDS:
            bad = np.flatnonzero(g[f] != w[f])
            assert len(bad) == 0, f"{what}, {'forward' if d == 0 else 'reversed'}: target {bad[0]} field {f}: got {g[bad[0]]}, oracle {w[bad[0]]}"


def _targets(rng, qa, q3):
    tA = [rng.integers(0, 20, size=L).astype(np.uint8) for L in TARGET_LENGTHS]
    t3 = [rng.integers(0, 20, size=L).astype(np.uint8) for L in TARGET_LENGTHS]
    tA.append(np.full(50, 20, np.uint8)); t3.append(np.full(50, 20, np.uint8))                  # all X
    for part in (12, 8):                                                                        # relatives of the query: every 12th / 8th residue redrawn
        tA.append(_redrawn(rng, qa, max(1, len(qa) // part))); t3.append(_redrawn(rng, q3, max(1, len(q3) // part)))
    a, s = _noisy(rng, qa, 0.1), _noisy(rng, q3, 0.1)                                           # the --alt-ali shape: the middle third overwritten with X
    a[len(a) // 3:2 * len(a) // 3] = 20; s[len(s) // 3:2 * len(s) // 3] = 20
    tA.insert(4, a); t3.insert(4, s)
    assert len(t3) == 25
    return tA, t3


@pytest.mark.parametrize("L", [20, 100, 130, 230, 260, 350, 390, 512, 700, 1300])
def test_every_register_class_against_unpadded_targets(env, L):
    """one query per register class of k_sw (R = 1, 2, 3, 4, 6, 8) and two row-tiled ones (borders in HBM, their stride from the explicit lengths) against 25
    targets stored back to back: lengths around the 64-column chunk, 1 .. 1 500, all X, X in the middle, relatives; with AA and without"""
    ctx = env[0]
    rng = np.random.default_rng(1000 + L)
    qa, q3 = rng.integers(0, 20, size=L).astype(np.uint8), rng.integers(0, 20, size=L).astype(np.uint8)
    tA, t3 = _targets(rng, qa, q3)
    starts = np.concatenate([[0], np.cumsum([len(t) for t in t3])])[:-1]
    assert (starts % 4 != 0).sum() >= 10 and (starts % 2 == 1).any()
    for atype in (2, 0):
        prof = _profiles(qa, q3, atype)
        want = _oracle(prof, L, tA, t3)
        if atype == 2:
            assert (want[0]["score"] > 100).sum() >= 2, want[0]["score"]
        _same(ctx.sw_batch_seqs(*prof, tA, t3), want, f"L = {L}, alignment type {atype}, AA given")
        if atype == 0:
            want = _oracle((None, prof[1], None, prof[3]), L, None, t3)
            _same(ctx.sw_batch_seqs(None, prof[1], None, prof[3], None, t3), want, f"L = {L}, no AA")


def test_explicit_copies_of_db_entries_equal_the_db_call(env):
    """entries copied out of the resident DB (unmasked) and passed explicitly in shuffled order == fsgpu_sw_batch on their ids, byte for byte"""
    ctx, db, q3, qa = env
    rng = np.random.default_rng(8)
    ids = rng.permutation(db.n)[:60].astype(np.uint32)
    ids[:3] = [db.n - 1, 0, db.n - 2]
    seqs = [helpers.target_seqs(db, int(t)) for t in ids]
    for qi in range(2):
        for atype in (2, 0):
            prof = _profiles(qa[qi], q3[qi], atype)
            if atype == 0:
                prof = (None, prof[1], None, prof[3])
            want = ctx.sw_batch(*prof, ids)
            got = ctx.sw_batch_seqs(*prof, [s[0] for s in seqs] if atype == 2 else None, [s[1] for s in seqs])
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (qi, atype)
            assert (want[0]["score"] > 100).any()


def test_int16_saturation_rerun_reads_the_explicit_lengths():
    """the 3 000-residue self-scoring query of test_sw_int16_saturation_rerun: its copy and its [100:2900] slice as explicit targets among random ones; the
    int32 re-run of the saturated pairs looks their lengths up in the explicit list, not in the (short) resident DB"""
    rng = np.random.default_rng(9)
    L = 3000
    q3 = np.where(rng.random(L) < 0.1, rng.choice(20, size=L), 10).astype(np.uint8)
    qa = np.where(rng.random(L) < 0.1, rng.choice(20, size=L), 18).astype(np.uint8)
    t3 = [rng.choice(20, size=int(l)).astype(np.uint8) for l in rng.integers(50, 2500, size=6)]
    tA = [rng.choice(20, size=len(x)).astype(np.uint8) for x in t3]
    t3[2:2] = [q3[100:2900].copy()]; tA[2:2] = [qa[100:2900].copy()]
    t3.append(q3.copy()); tA.append(qa.copy())
    t3.append(rng.choice(20, size=77).astype(np.uint8)); tA.append(rng.choice(20, size=77).astype(np.uint8))
    tiny = [rng.choice(20, size=l).astype(np.uint8) for l in (5, 9, 30)]
    lens = np.array([5, 9, 30], np.int32)
    offs = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)]).astype(np.int64)
    d = np.full(offs[-1], 20, np.uint8)
    for i in range(3):
        d[offs[i]:offs[i] + lens[i]] = tiny[i]
    ctx = api.Context(0)
    ctx.load_db(synth.PaddedDB(d, d.copy(), offs, lens))                 # three short entries: ids and lengths of the explicit list mean nothing here
    prof = _profiles(qa, q3, 2, comp_bias=False)
    want = _oracle(prof, L, tA, t3)
    assert (want[0]["word"] == 2).sum() >= 1 and (want[1]["word"] == 2).sum() >= 1
    assert ((want[0]["word"] == 2) & (want[0]["score"] > 32767)).any()
    _same(ctx.sw_batch_seqs(*prof, tA, t3), want, "saturated")
    ctx.close()


def test_other_gap_costs(env):
    ctx = env[0]
    rng = np.random.default_rng(12)
    qa, q3 = rng.integers(0, 20, size=260).astype(np.uint8), rng.integers(0, 20, size=260).astype(np.uint8)
    tA, t3 = _targets(rng, qa, q3)
    prof = _profiles(qa, q3)
    seen = []
    for go, ge in ((8, 2), (15, 3)):
        want = _oracle(prof, 260, tA, t3, go, ge)
        _same(ctx.sw_batch_seqs(*prof, tA, t3, gap_open=go, gap_extend=ge), want, f"gaps {go}/{ge}")
        seen.append(want[0]["score"].copy())
    assert (seen[0] != seen[1]).any()


def test_state_after_success_failures_and_empty_calls(env):
    """after an explicit call, and after each refused one, fsgpu_sw_batch reads the resident DB again; the refusals: a length of 0, an offset past the end,
    AA profiles without AA targets, gap costs the device refuses; n = 0 returns empty arrays"""
    ctx, db, q3, qa = env
    rng = np.random.default_rng(4)
    prof = _profiles(qa[0], q3[0])
    ids = np.arange(0, db.n, 5, dtype=np.uint32)
    want_db = ctx.sw_batch(*prof, ids)
    seqs = [helpers.target_seqs(db, int(t)) for t in ids]
    for k, fld in ((0, "score"), (0, "dbEnd"), (1, "score")):
        assert (want_db[k][fld] == np.array([helpers.o_sw(prof[2 * k], prof[2 * k + 1], len(q3[0]), a, s)[fld] for a, s in seqs])).all()

    def db_again(what):
        got = ctx.sw_batch(*prof, ids)
        assert got[0].tobytes() == want_db[0].tobytes() and got[1].tobytes() == want_db[1].tobytes(), what

    # explicit targets that are NOT the DB's: as many as ids, other lengths
    tA = [rng.integers(0, 20, size=int(l)).astype(np.uint8) for l in rng.integers(1, 300, size=len(ids))]
    t3 = [rng.integers(0, 20, size=len(a)).astype(np.uint8) for a in tA]
    want = _oracle(prof, len(q3[0]), tA, t3)
    _same(ctx.sw_batch_seqs(*prof, tA, t3), want, "explicit")
    db_again("after an explicit call")
    total = sum(len(a) for a in tA)
    nat = np.concatenate([[0], np.cumsum([len(a) for a in tA])])
    lens = [len(a) for a in tA]
    bad_len, bad_off, neg_len = list(lens), nat.copy(), list(lens)
    bad_len[3] = 0
    neg_len[0] = -1
    bad_off[5] = total - lens[5] + 1
    refused = [dict(lengths=bad_len), dict(lengths=neg_len), dict(offsets=bad_off), dict(gap_open=1, gap_extend=1), dict(gap_open=5, gap_extend=7)]
    for kw in refused:
        with pytest.raises(api.FsgpuError):
            ctx.sw_batch_seqs(*prof, tA, t3, **kw)
        db_again(f"after a refused call {sorted(kw)}")
    with pytest.raises(api.FsgpuError):
        ctx.sw_batch_seqs(*prof, None, t3)                     # AA profiles, no AA targets
    db_again("after 'AA profiles without AA targets'")
    _same(ctx.sw_batch_seqs(*prof, tA, t3), want, "explicit, after the refusals")
    fwd, rev = ctx.sw_batch_seqs(*prof, [], [])
    assert len(fwd) == 0 and len(rev) == 0 and fwd.dtype == api.SW_DT
    db_again("after an empty call")

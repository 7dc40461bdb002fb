"""tests/marv_cases.py held to the conditions that make its cases find something (no GPU): the caps bind, the cut of the tie case falls inside a group
that spans shards, the one-letter queries really lack the matrix's minimum, and the model's scores are the C oracle's and the compiled reference's on
every target of every case.  A later edit of the cases that hollows the device tests out fails here."""
import numpy as np
import pytest

import gapless_model as gm
import helpers
import marv_cases as MC
import oracle_lib

NAMES = ["3di_L1", "3di_L5", "3di_L64", "3di_L300", "3di_L897", "3di_L300_nobias", "blosum62", "3di_one_letter", "all_x", "other_matrix_with_min",
         "other_matrix_without_min"]
SATURATING = [n for n in NAMES if n not in ("3di_L1", "3di_L5", "all_x")]


def test_the_cases_are_the_ones_listed():
    cases = MC.cases()
    assert list(cases) == NAMES and [n for n in NAMES if cases[n].saturating] == SATURATING
    assert [cases[n].L for n in NAMES[:5]] == [1, 5, 64, 300, 897]
    assert [n for n in NAMES if cases[n].profile_cap] == ["other_matrix_without_min"]
    assert not cases["3di_L300_nobias"].cb.any() and all(cases[n].comp_bias for n in NAMES if n != "3di_L300_nobias")
    for n in ("3di_L300", "3di_L897", "blosum62", "other_matrix_with_min"):               # a bias that is not the same number everywhere
        assert cases[n].cb.min() < 0 < cases[n].cb.max(), n
    for n in NAMES:                                                                       # the profile is matrix column + bias, nothing else
        q = cases[n]
        m = q.tiny.reshape(21, 21).astype(np.int32)
        assert (q.pssm.astype(np.int32) == m[:, q.seq] + q.cb.astype(np.int32)).all() and q.pssm.shape == (21, q.L)
        assert q.matrix_cap == 255 - (abs(min(0, int(m.min()))) + abs(min(0, int(q.cb.min()))))
        assert q.cap == (q.derived_cap if q.profile_cap else q.matrix_cap)


def test_the_database_holds_what_the_shim_has_to_handle():
    w = MC.world()
    db = w["db"]
    lens = db.lengths
    assert 230 <= db.n <= 250 and (np.diff(lens) >= 0).all()
    assert set([1, 2, 3, 5, 15, 16, 17, 63, 64, 65]) <= set(lens.tolist()) and 690 <= np.sort(lens)[-MC.COPIES - 1] <= 700
    assert (lens % 4 != 0).mean() > 0.6 and int(lens[-1]) % 4 != 0                        # the last entry has padding for the second buffer to lack
    assert ((db.data3di >= 32) & (db.data3di < 52)).sum() > 50 and (db.data3di == 52).sum() > 5
    assert len(w["allx"]) == 4
    for t in w["allx"]:
        assert (gm.target_codes(db, t) == MC.X).all()
    for what, q in (("Q", w["Q"]), ("QB", w["QB"])):
        ids = w["copies"][what]
        assert len(ids) == MC.COPIES
        for t in ids:
            assert (db.seq(int(t), unmask=False) == q).all()
        for N in (2, 3, 7):
            assert len(set((ids % N).tolist())) >= min(N, 3), (what, N)
    data, off = MC.unpadded(db)
    assert len(data) == int(db.offsets[db.n - 1]) + int(lens[-1]) < len(db.data3di) and (off[:-1] == db.offsets[:-1]).all()
    assert (data == db.data3di[:len(data)]).all()
    B = MC.other_db()
    assert (B.lengths == lens).all() and (B.data3di != db.data3di).mean() > 0.8 and ((B.data3di >= 32) == (db.data3di >= 32)).all()


@pytest.mark.parametrize("name", SATURATING)
def test_the_cap_binds(name):
    """a wrong cap shows only where some target's uncapped run exceeds it"""
    q, w = MC.cases()[name], MC.world()
    raw = gm.best_runs(q.pssm, w["packed"])
    s = MC.scores(name)
    assert raw.max() > q.cap + 50 and (s == q.cap).sum() >= 10 and s.max() == q.cap
    assert (s == np.minimum(raw, q.cap)).all()
    assert ((s > 0) & (s < q.cap)).sum() > 20                                             # and the rest of the list is not all one number


@pytest.mark.parametrize("name", NAMES)
def test_the_cut_of_the_tie_case_falls_inside_a_group_that_spans_shards(name):
    s = MC.scores(name)
    hits = MC.expected(name, MC.TIE_MAX_SEQS)
    assert len(hits) == MC.TIE_MAX_SEQS
    last = int(hits["score"][-1])
    group = np.flatnonzero(s == last)
    kept = hits["id"][hits["score"] == last]
    assert 0 < len(kept) < len(group), name                                              # strictly inside
    assert (kept == group[:len(kept)]).all()                                              # the lowest ids of the group
    for N in (2, 3, 7):
        assert len(set((group % N).tolist())) >= 2 and len(set((kept % N).tolist())) >= 2, (name, N)
    if MC.cases()[name].saturating:
        assert last == MC.cases()[name].cap


def test_the_other_sizes_of_the_list():
    n = MC.world()["db"].n
    for name in NAMES:
        s = MC.scores(name)
        assert MC.expected(name, 1).tolist() == [(int(np.argmax(s)), int(s.max()))]
        full = MC.expected(name, n)
        assert len(full) == n and sorted(full["id"].tolist()) == list(range(n)) and MC.expected(name, n + 9).tolist() == full.tolist()
        key = list(zip((-full["score"]).tolist(), full["id"].tolist()))
        assert key == sorted(key)
    assert not MC.scores("all_x").any() and MC.expected("all_x", 7)["id"].tolist() == list(range(7))


def test_the_one_letter_queries_lack_the_minimum_of_their_matrix():
    cases = MC.cases()
    for name in ("3di_one_letter", "other_matrix_without_min"):
        q = cases[name]
        m = q.tiny.reshape(21, 21).astype(np.int32)
        assert len(set(q.seq.tolist())) == 1 and q.seq[0] == MC.world()["letter"] < 20
        a, b = np.unravel_index(np.argmin(m), m.shape)
        assert q.seq[0] not in (a, b)
        assert m[:, q.seq].min() > m.min() == q.matrix_min                                # min over its own columns > the matrix minimum
        assert q.derived_cap > q.matrix_cap                                               # reading the minimum off the profile gives another cap
    # branch (1) must not do that; branch (2) does, and the expectation says so
    assert cases["3di_one_letter"].cap == cases["3di_one_letter"].matrix_cap
    assert cases["other_matrix_without_min"].cap == cases["other_matrix_without_min"].derived_cap != cases["other_matrix_without_min"].matrix_cap
    q = cases["other_matrix_with_min"]
    m = q.tiny.reshape(21, 21).astype(np.int32)
    assert m[:, q.seq].min() == m.min() and q.derived_cap == q.matrix_cap and not m[MC.X].any()
    # between the two caps the divergent case has targets: the difference shows in the hit list
    raw = gm.best_runs(cases["other_matrix_without_min"].pssm, MC.world()["packed"])
    assert (raw >= cases["other_matrix_without_min"].derived_cap).sum() >= 10


def _oracle_scores(q, db):
    O = helpers.oracle()
    out = np.zeros(db.n, np.int32)
    for i in range(db.n):
        t = np.ascontiguousarray(gm.target_codes(db, i).astype(np.uint8))
        out[i] = O.fso_ungapped_score(q.seq, q.L, q.tiny, 21, q.cb, t, len(t))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_scores_equal_the_oracle_on_every_target(name):
    """the CPU path's cap is the matrix-wide one: the model under that cap is the oracle everywhere, the divergent case included"""
    q, w = MC.cases()[name], MC.world()
    want = _oracle_scores(q, w["db"])
    got = gm.scores(q.pssm, q.matrix_cap, w["packed"])
    assert (got == want).all(), np.flatnonzero(got != want)[:10]
    if q.profile_cap:
        assert (MC.scores(name) != want).sum() >= 10 and (np.minimum(MC.scores(name), q.matrix_cap) == want).all()
    else:
        assert (MC.scores(name) == want).all()


@pytest.mark.parametrize("which", ["B", 1, 2])
def test_scores_on_the_other_databases_equal_the_oracle(which):
    db = MC.other_db() if which == "B" else MC.small_db(which)
    assert db.n == (MC.world()["db"].n if which == "B" else which)
    for name in ("3di_L300", "blosum62", "3di_L5"):
        want = _oracle_scores(MC.cases()[name], db)
        assert (MC.scores_on(name, which) == want).all(), name
    if which == "B":
        assert (MC.scores_on("3di_L300", "B") != MC.scores("3di_L300")).mean() > 0.5
    else:
        assert MC.scores_on("3di_L300", which).min() > 30


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("3di") or n == "all_x"])
def test_scores_equal_the_compiled_reference(name):
    ref = oracle_lib.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref not built")
    q, db = MC.cases()[name], MC.world()["db"]
    want = np.zeros(db.n, np.int32)
    ref.ref_ungapped(q.seq, q.L, int(q.comp_bias), q.matrix[2], db.data3di, np.ascontiguousarray(db.offsets[:-1], np.int64),
                     np.ascontiguousarray(db.lengths, np.int32), db.n, 1, want)
    assert (MC.scores(name) == want).all(), np.flatnonzero(MC.scores(name) != want)[:10]

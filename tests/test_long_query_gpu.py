"""Every entry that takes a query of 1 .. FSGPU_MAX_SEQ_LEN = 65535 residues, run at the lengths of tests/long_query_cases.py (8193 .. 65535) and held to the
independent models with exact equality: the gapless scan over 17 .. 128 row tiles (gapless_model), the row-tiled Smith-Waterman in every entry form,
alone and with queries of 128, 64, 3 and 1 tile levels in one call (sw_model), diagonal rescoring with diagonals up to +-65535 (diag_model), the
block aligner from end cells up to row 65534 (ba_model), LDDT and TM on windows of a 65535-residue chain (lddt_model, tm_model), and one query of
65535 residues through Search.prefilter / Search.align.  The conditions that make these inputs reach what they are meant to reach are asserted, on the models alone, in tests/test_long_query_model.py."""
import ctypes as C

import numpy as np
import pytest

import btrace_cases as B
import diag_model as DM
import gapless_model as gm
import helpers
import lddt_cases as LK
import lddt_model as LM
import long_query_cases as LC
import sw_cases as K
import tm_cases as TC
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu

SW_FIELDS = ("score", "qEnd", "dbEnd", "word")
BOTH_TYPES = (32768, 32769, 65535)                 # lengths that run alignment type 0 as well; the others run type 2 only


@pytest.fixture(scope="module")
def ctx():
    """one context for the file: every test loads its own database into it (torch asks for the device first, as bench.py does)"""
    import torch
    torch.cuda.get_device_properties(0)
    c = api.Context(0)
    yield c
    c.close()


def _same_hits(hits, want, what):
    assert len(hits) == len(want), (what, len(hits), len(want))
    assert (hits["id"] == want["id"]).all() and (hits["score"] == want["score"]).all(), what


def _sw_same(got, want, what):
    bad = [k for k in range(len(want)) if any(int(got[k][f]) != int(want[k][f]) for f in SW_FIELDS)]
    assert len(got) == len(want) and not bad, (what, [(k, "device", tuple(int(got[k][f]) for f in SW_FIELDS), "model", tuple(int(want[k][f]) for f in SW_FIELDS))
                                                      for k in bad[:6]])


# ---- 1. the gapless scan -----------------------------------------------------------------------------------------------------------------------------------
def _scan_check(ctx, L, what):
    w = LC.world(L)
    pssm, cap = LC.scan_profile(L)
    want = w.scan_want()
    hits = ctx.gapless_scan(pssm, cap, min_score=30, identity=-1, max_res=1000)
    got = ctx.gapless_scores().astype(np.int32)
    assert (got == want).all(), (what, L, [(int(i), w.kind[i], w.info[i], int(got[i]), int(want[i])) for i in np.flatnonzero(got != want)[:8]])
    _same_hits(hits, gm.select(want, 30, -1, 1000), (what, L))
    return w, pssm, cap, want


@pytest.mark.parametrize("L", LC.LQ)
def test_scan_of_a_long_query(ctx, L):
    """fsgpu_gapless_scan, fsgpu_gapless_launch / _finish and fsgpu_gapless_scan_multi with the long query between two short ones: the score vector
    and the hit list of gapless_model, the planted windows across every border between two row tiles among them"""
    ctx.load_db(LC.world(L).db)
    w, pssm, cap, want = _scan_check(ctx, L, "scan")
    ident = int(np.argmin(want))
    lib = api.lib()
    p = np.ascontiguousarray(pssm, np.int8)
    hits, nout = np.zeros(40, api.HIT_DT), C.c_int(-1)
    assert lib.fsgpu_gapless_launch(ctx.h, p.ctypes.data_as(C.c_void_p), L, cap, 15, ident, 40) == 0, lib.fsgpu_last_error(ctx.h)
    assert lib.fsgpu_gapless_finish(ctx.h, hits.ctypes.data_as(C.c_void_p), C.byref(nout)) == 0, lib.fsgpu_last_error(ctx.h)
    _same_hits(hits[:nout.value], gm.select(want, 15, ident, 40), ("launch / finish", L))
    assert (ctx.gapless_scores().astype(np.int32) == want).all()
    # between two short queries of different classes: one launch each, one scan more for the row-tiled member
    shorts = []
    for n in (100, 300):
        s = api.prefilter_profile(api.Matrix(0, 2.0), LC.query(n)[0], True, 0.15)
        shorts.append((s[0], s[1], gm.scores(s[0], s[1], w.db)))
    batch = [(shorts[0][0], shorts[0][1], -1), (pssm, cap, ident), (shorts[1][0], shorts[1][1], 3)]
    got = ctx.gapless_scan_multi(batch, 30, 50)
    assert ctx.gapless_last_batch() == (3, 3)
    _same_hits(got[1], gm.select(want, 30, ident, 50), ("scan_multi, the long member", L))
    for k, s, idn in ((0, shorts[0], -1), (2, shorts[1], 3)):
        assert (ctx.gapless_scores_multi(k).astype(np.int32) == s[2]).all(), ("scan_multi, a short member's slice", L, k)
        _same_hits(got[k], gm.select(s[2], 30, idn, 50), ("scan_multi, a short member", L, k))


def test_scan_of_17_tiles_behind_one_of_128(ctx):
    """65535 rows, then 8193 on the same context and database: borders and running maxima of 128 tiles lie behind a scan of 17"""
    ctx.load_db(LC.world(8193).db)
    for L in (65535, 8193, 65535):
        w = LC.world(8193)
        pssm, cap = LC.scan_profile(L)
        want = gm.scores(pssm, cap, w.db) if L != 8193 else w.scan_want()
        hits = ctx.gapless_scan(pssm, cap, min_score=30, identity=-1, max_res=1000)
        got = ctx.gapless_scores().astype(np.int32)
        assert (got == want).all(), (L, np.flatnonzero(got != want)[:8])
        _same_hits(hits, gm.select(want, 30, -1, 1000), L)
    assert (LC.world(8193).scan_want() > 100).sum() >= 19


# ---- 2. Smith-Waterman, the profile entries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,atype", [(L, t) for L in LC.LQ for t in ((2, 0) if L in BOTH_TYPES else (2,))])
def test_sw_profile_entries_on_a_long_query(ctx, L, atype):
    """fsgpu_sw_batch, fsgpu_sw_batch_seqs over the same targets as explicit sequences, fsgpu_sw_multi_dir in both directions with and without
    selections: score, qEnd, dbEnd and word of sw_model for windows across multiples of 512 rows, up to row L - 1 and for the int32 re-run"""
    w = LC.world(L)
    ctx.load_db(w.db)
    ids = w.sw_ids()
    want = [w.sw_want(atype, rev, ids) for rev in (False, True)]
    assert (want[0]["word"] == 2).sum() == (len(w.ids("sat")) if atype == 2 else 0) and len(w.ids("sat")) >= 1 and (want[0]["qEnd"] == L - 1).sum() >= 2 and (want[1]["qEnd"] == L - 1).sum() >= 1
    prof = LC.sw_profiles(L, atype)
    fwd, rev = ctx.sw_batch(*prof, ids)
    _sw_same(fwd, want[0], ("sw_batch forward", L, atype)); _sw_same(rev, want[1], ("sw_batch reversed", L, atype))
    seqs = [K.target(w.db, int(i)) for i in ids]
    fwd, rev = ctx.sw_batch_seqs(*prof, [s[1] for s in seqs], [s[0] for s in seqs])
    _sw_same(fwd, want[0], ("sw_batch_seqs forward", L, atype)); _sw_same(rev, want[1], ("sw_batch_seqs reversed", L, atype))
    sel = np.arange(len(ids), dtype=np.int32)[::-1][::2].copy()          # every second pair, from the back
    for d in (0, 1):
        got = ctx.sw_multi_dir([(*prof, L, ids)], d)[0]
        _sw_same(got, want[d], ("sw_multi_dir", L, atype, d))
    for d in (1, 0):                                                      # reversed first: nothing is kept from a forward call over the same pairs
        got = ctx.sw_multi_dir([(*prof, L, ids)], d, selections=[sel])[0]
        _sw_same(got[sel], want[d][sel], ("sw_multi_dir with selections", L, atype, d))
        rest = np.setdiff1d(np.arange(len(ids)), sel)
        assert not got[rest].view(np.int32).any(), "an unselected record was written"


# ---- 3. Smith-Waterman, queries of different depth in one call ------------------------------------------------------------------------------------------------
MIXED = (65535, 32768, 1025, 300)                  # 128, 64 and 3 tile levels, and one query that is not row-tiled


def _mixed_ids(w):
    f, r, p = w.ids("sw_fwd"), w.ids("sw_rev"), w.plain_sample()
    return [np.array(f[::3] + r[::3] + p[::3], np.uint32),
            np.array(f[1::4] + r[1::4] + p[1::3], np.uint32),
            np.array(f[2::4] + p[::2], np.uint32),
            np.array(p + f[:2], np.uint32)]


@pytest.mark.parametrize("go,ge", [(10, 1), (12, 2)])
def test_sw_queries_of_128_64_3_and_1_levels_in_one_call(ctx, go, ge):
    """one fsgpu_sw_multi_dir call serves every level of all row-tiled queries: launches thin out from three queries to one.  The reversed call
    after the forward one takes its records from what the forward call kept -- with the same gap costs only."""
    w = LC.world(65535)
    ctx.load_db(w.db)
    ids = _mixed_ids(w)
    n_long = sum(len(t) for t in ids[:3])
    want = [[w.sw_want(2, rev, t, go, ge, L=L) for L, t in zip(MIXED, ids)] for rev in (False, True)]
    assert any((a != b).any() for a, b in zip(want[1], [w.sw_want(2, True, t, 10 + 12 - go, 1 + 2 - ge, L=L) for L, t in zip(MIXED, ids)])), \
        "gap costs must show in a reversed record"
    queries = [(*LC.sw_profiles(L, 2), L, t) for L, t in zip(MIXED, ids)]

    def step(direction, g, launched, reused, what):
        got = ctx.sw_multi_dir(queries, direction, gap_open=g[0], gap_extend=g[1])
        model = want[direction] if g == (go, ge) else [w.sw_want(2, bool(direction), t, g[0], g[1], L=L) for L, t in zip(MIXED, ids)]
        for i in range(len(MIXED)):
            _sw_same(got[i], model[i], ("profiles", what, "query of", MIXED[i]))
        c = ctx.history_counters()
        assert (c["sw_long_launched"], c["sw_long_reused"]) == (launched, reused), (what, c)

    other = (10 + 12 - go, 1 + 2 - ge)
    step(0, (go, ge), n_long, 0, "forward")
    step(1, (go, ge), 0, n_long, "reversed, nothing changed: the kept records answer")
    step(0, other, n_long, 0, "forward with the other gap costs")
    step(1, (go, ge), n_long, 0, "reversed after a forward call with other gap costs: nothing may be reused")


@pytest.mark.parametrize("go,ge", [(10, 1), (12, 2)])
def test_compact_sw_queries_of_128_64_3_and_1_levels_in_one_call(ctx, go, ge, monkeypatch):
    """the same four queries as codes and bias vectors: fsgpu_sw_multi_dir_c hands the long ones over to the profile path with tables it builds from
    bias vectors of up to 65535 entries; fsgpu_sw_multi_c runs both directions in one submission"""
    for k in ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT"):
        monkeypatch.delenv(k, raising=False)
    w = LC.world(65535)
    ctx.load_db(w.db)
    ids = _mixed_ids(w)
    n_long = sum(len(t) for t in ids[:3])
    want = [[w.sw_want(2, rev, t, go, ge, L=L) for L, t in zip(MIXED, ids)] for rev in (False, True)]
    m3, mA = LC.sw_matrices(2)
    qs = [LC.sw_query(L, 2) for L in MIXED]
    queries = [(q.qa, q.q3, q.cbAf, q.cb3f, q.cbAr, q.cb3r, t) for q, t in zip(qs, ids)]
    for d, counts in ((0, (n_long, 0)), (1, (0, n_long)), (1, (n_long, 0))):
        got = ctx.sw_multi_dir_c(m3, mA, queries, d, gap_open=go, gap_extend=ge)
        for i in range(len(MIXED)):
            _sw_same(got[i], want[d][i], ("sw_multi_dir_c", d, counts, "query of", MIXED[i]))
        c = ctx.history_counters()
        assert (c["sw_long_launched"], c["sw_long_reused"]) == counts, (d, counts, c)
    fwd, rev = ctx.sw_multi_c(m3, mA, queries, gap_open=go, gap_extend=ge)
    for i in range(len(MIXED)):
        _sw_same(fwd[i], want[0][i], ("sw_multi_c forward", "query of", MIXED[i]))
        _sw_same(rev[i], want[1][i], ("sw_multi_c reversed", "query of", MIXED[i]))


# ---- 4. diagonal rescoring ---------------------------------------------------------------------------------------------------------------------------------------
def _diag_world():
    """the query of 65535 residues; a target of 300 residues that repeats it on diagonal +65234; a target of 65535 residues, unrelated but for runs at
    the far end of the diagonals 0, +32768 and -32768"""
    L = 65535
    q3, qa = LC.query(L)
    rng = np.random.default_rng(65)
    short = (qa[65234:65534].copy(), q3[65234:65534].copy())
    ta, t3 = rng.integers(0, 20, L).astype(np.uint8), rng.integers(0, 20, L).astype(np.uint8)
    for t_at, q_at, n in ((64600, 64600, 400), (32400, 32400 + 32768, 300), (65200, 65200 - 32768, 300)):
        ta[t_at:t_at + n], t3[t_at:t_at + n] = qa[q_at:q_at + n], q3[q_at:q_at + n]
    targets = [short, (ta, t3)]
    lens = np.array([300, L], np.int32)
    off = np.zeros(3, np.int64)
    off[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3, da = np.full(off[-1], 20, np.uint8), np.full(off[-1], 20, np.uint8)
    for k, (a, s) in enumerate(targets):
        d3[off[k]:off[k] + lens[k]], da[off[k]:off[k] + lens[k]] = s, a
    return (qa, q3), targets, synth.PaddedDB(d3, da, off, lens)


@pytest.mark.parametrize("aa_factor", [1.4, 0.0])
def test_diagonals_of_a_long_query(ctx, aa_factor):
    """fsgpu_diag_rescore with Lq = 65535 against Lt = 300 and Lt = 65535: diagonals 0, +-1, +-32767, +-32768, +-65234, +-65534, +-65535 and those at
    which the overlap ends; all eight fields of diag_model, status included.  The runs lie at the far end: startPos and endPos pass 32767."""
    query, targets, db = _diag_world()
    ctx.load_db(db)
    m3 = helpers.o_submat("MAT3DI", 2.1)[0].reshape(21, 21).copy()
    mA = helpers.o_submat("BLOSUM62", aa_factor)[0].reshape(21, 21).copy()
    diags = sorted({s * d for d in (0, 1, 299, 300, 32767, 32768, 65234, 65235, 65534, 65535, 65536) for s in (1, -1)})
    pairs = [(0, t, d) for t in (0, 1) for d in diags]
    got = ctx.diag_rescore([query[0]], [query[1]], m3, mA, pairs)
    l3, lA = m3.tolist(), mA.tolist()
    want = [DM.rescore_pair([query], targets, p, l3, lA) for p in pairs]
    by = dict(zip(pairs, want))
    for k, (g, m) in enumerate(zip(got, want)):
        skip = ("revScore",) if m["status"] == DM.UNDEFINED else ()
        bad = [f for f in DM.FIELDS if f not in skip and int(g[f]) != m[f]]
        assert not bad, (pairs[k], bad, dict(zip(DM.FIELDS, g.tolist())), m)
    # what the pairs reach, from the model's own records
    assert by[(0, 1, 0)]["startPos"] > 32767 and by[(0, 1, 0)]["endPos"] >= 64990 and by[(0, 1, 0)]["score"] > 2000
    for d in (32768, -32768):
        assert by[(0, 1, d)]["status"] == DM.OK and by[(0, 1, d)]["diagonalLen"] == 32767 and by[(0, 1, d)]["endPos"] + 32768 > 65000 and by[(0, 1, d)]["score"] > 1500
    assert by[(0, 0, 65234)]["diagonalLen"] == 300 and by[(0, 0, 65234)]["score"] > 1500 and by[(0, 0, 65235)]["diagonalLen"] == 300
    assert by[(0, 0, 65534)]["diagonalLen"] == 1 and by[(0, 0, 65535)]["status"] == DM.NO_OVERLAP and by[(0, 1, 65534)]["diagonalLen"] == 1
    assert by[(0, 1, -65534)]["status"] == DM.OK and by[(0, 1, -65534)]["diagonalLen"] == 1 and by[(0, 1, -65535)]["status"] == DM.NO_OVERLAP
    assert by[(0, 0, -299)]["diagonalLen"] == 1 and by[(0, 0, -300)]["status"] == DM.NO_OVERLAP
    assert {m["status"] for m in want} >= {DM.OK, DM.NO_OVERLAP}


# ---- 5. the block aligner ------------------------------------------------------------------------------------------------------------------------------------
def _bt_world(L):
    """tasks from sw_model's own forward records of planted windows on the query of length L: the window from row 0 (end cell in the first tile), the
    ones across the first multiple of 512, across row 32768 and across the last multiple, the one up to row L - 1, and one more.  Returns
    (device query, tasks without the query index, the model's cases, end cells)"""
    w = LC.world(L)
    q = LC.sw_query(L, 2)
    ids = w.ids("sw_fwd")
    mult = list(range(512, L, 512))
    pick = [i for i in ids if w.info[i]["s"] == 0 or w.info[i]["m"] in (mult[0], 32768, mult[-1]) or (w.info[i]["m"] is None and w.info[i]["end"] == L - 1)]
    pick += [i for i in ids if i not in pick][:6 - len(pick)]
    recs = w.sw_want(2, False, pick)
    bias = q.cbAf.astype(np.int64) + q.cb3f.astype(np.int64)
    tasks, cases, ends = [], [], []
    for i, r in zip(pick, recs):
        qe, de, sc = int(r["qEnd"]), int(r["dbEnd"]), int(r["score"])
        t3, ta = K.target(w.db, i)
        cases.append(B.model_case(f"longq_{L}_{i}", q.qa[:qe + 1], q.q3[:qe + 1], bias[:qe + 1], ta[:de + 1], t3[:de + 1], sc))
        tasks.append((i, qe, de, sc))
        ends.append((qe, de))
    return (q.qa, q.q3, q.cbAf, q.cb3f), tasks, cases, ends


def _bt_check(got, cases, ends, what):
    for r, c, e in zip(got, cases, ends):
        want = c.expected(*e)
        assert {x: r[x] for x in want} == want and r["blockSizes"] == c.attempts, (what, c.name, e, r, want, c.attempts)


def test_block_aligner_from_end_cells_of_long_queries(ctx):
    """fsgpu_block_backtrace on queries of 65535 and 32769 residues: status, start cell, backtrace, identical residues and block sizes of ba_model for
    end cells in the first tile, behind row 32768 and in row L - 1; one alignment per wave, four per wave, one workgroup per compute unit"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tables = B.device_tables()
    n = 0
    for L in (65535, 32769):
        ctx.load_db(LC.world(L).db)
        query, tasks, cases, ends = _bt_world(L)
        assert all(c.cls == "A" and c.score == c.target and len(B.expand(c.cigar)) < 200 for c in cases), [(c.name, c.cls) for c in cases]
        assert min(e[0] for e in ends) < 512 and max(e[0] for e in ends) == L - 1 and any(32768 <= e[0] < 32768 + 200 for e in ends) and len(tasks) >= 5
        one = [(0, *t) for t in tasks]
        got = ctx.block_backtrace(*tables, [query], one, 10, 1)
        _bt_check(got, cases, ends, ("one alignment per wave", L))
        for r, c, e in zip(got, cases, ends):                             # the whole window: the start cell lies a tile before the end cell, or in row 0
            assert r["qStart"] == e[0] + 1 - c.i and (r["qStart"] // 512 < e[0] // 512 or e[0] < 512 or e[0] == L - 1)
        reps = (12 * cus) // len(tasks) + 1
        order = np.random.default_rng(L).permutation(np.repeat(np.arange(len(tasks)), reps))
        assert len(order) > 12 * cus
        many = ctx.block_backtrace(*tables, [query], [one[k] for k in order], 10, 1)
        assert all(many[p] == got[k] for p, k in enumerate(order)), ("four alignments per wave", L)
        ctx.block_backtrace_footprint(1)
        try:
            assert ctx.block_backtrace(*tables, [query], one, 10, 1) == got
        finally:
            ctx.block_backtrace_footprint(0)
        n += len(tasks)
    assert n >= 11


# ---- 6. LDDT and TM --------------------------------------------------------------------------------------------------------------------------------------------
def _geometry_world():
    """a 3.8 A walk of 65535 residues, a second query of 300 residues behind it, and per task a target that is a perturbed window of its query:
    windows from residue 0, across residue 32768 and up to the last residue.  -> (queries, targets, lddt tasks)"""
    rng = np.random.default_rng(655)
    L = 65535
    queries = [TC._walk(rng, L), TC._walk(rng, 300)]
    targets, tasks = [], []
    for q, q_start, n_m, t_start in ((0, 0, 60, 0), (0, 0, 50, 4), (0, 32768 - 30, 60, 2), (0, 32768 - 64, 128, 0), (0, 32767, 40, 3), (0, L - 60, 60, 0),
                                     (0, L - 45, 40, 5), (1, 0, 64, 0), (1, 300 - 50, 50, 7)):
        bt = TC._backtrace(rng, n_m)
        bt = bt[:len(bt) - max(0, q_start + sum(ch in "MI" for ch in bt) - queries[q].shape[1])]       # an I run must not push the window past the chain
        nq, nt = sum(ch in "MI" for ch in bt), sum(ch in "MD" for ch in bt)
        assert q_start + nq <= queries[q].shape[1] and bt[-1] == "M"
        t = TC._walk(rng, t_start + nt + int(rng.integers(0, 4)))
        a2q, a2t = LM.aligned(q_start, t_start, bt)
        t[:, a2t] = queries[q][:, a2q] + rng.normal(scale=1.0, size=(3, len(a2q))).astype(np.float32)
        targets.append(np.ascontiguousarray(t, np.float32))
        tasks.append((q, len(targets) - 1, q_start, t_start, bt))
    return queries, targets, tasks


class _Distances:
    """stands in for the query's distance matrix in lddt_model.columns: the block for the rows and columns asked for, by the same pairwise()"""

    def __init__(self, qc):
        self.q = np.ascontiguousarray(np.asarray(qc, np.float32).T)

    def __getitem__(self, ix):
        rows, cols = ix[0].ravel(), ix[1].ravel()
        assert (rows == cols).all()
        return LM.pairwise(self.q[rows])


def _norms_of(qc, rows):
    """lddt_model.query_norm for the residues `rows` alone: neighbours are counted over the WHOLE chain, row block by row block"""
    q = np.ascontiguousarray(np.asarray(qc, np.float32).T)
    norm = np.full(len(q), np.nan, np.float32)
    rows = np.asarray(sorted(rows), np.int64)
    for a in range(0, len(rows), 32):
        r = rows[a:a + 32]
        close = LM.dist(q[r, None, :], q[None, :, :]) < LM.CUTOFF
        close[np.arange(len(r)), r] = False
        cnt = close.sum(1).astype(np.float32)
        with np.errstate(divide="ignore"):
            norm[r] = np.where(cnt != 0, np.float32(1.0) / np.where(cnt != 0, cnt, np.float32(1)), np.float32(np.inf))
    return norm


def test_lddt_and_tm_on_windows_of_a_65535_residue_chain(ctx):
    """fsgpu_lddt_batch by bit patterns against lddt_model (the norms of a residue count its neighbours over all 65535 residues), fsgpu_tm_batch by bit
    patterns against tm_model, no task differing; a second query of 300 residues lies behind the long one in both calls"""
    queries, targets, tasks = _geometry_world()
    assert sum(1 for t in tasks if t[0] == 0 and t[2] < 32768 <= t[2] + sum(ch in "MI" for ch in t[4]) - 1) >= 2
    assert any(t[0] == 0 and t[2] + sum(ch in "MI" for ch in t[4]) == 65535 for t in tasks) and any(t[0] == 1 for t in tasks)
    want = []
    stand_in = {}
    for qi in (0, 1):
        touched = set()
        for q, _t, qs, ts, bt in tasks:
            if q == qi:
                touched |= set(LM.aligned(qs, ts, bt)[0].tolist())
        stand_in[qi] = (_norms_of(queries[qi], touched), _Distances(queries[qi]))
    norm1, _ = LM.query_norm(queries[1])
    rows1 = ~np.isnan(stand_in[1][0])
    assert LK.same_bits(stand_in[1][0][rows1], norm1[rows1])             # the stand-in is query_norm where that can be computed whole
    for q, t, qs, ts, bt in tasks:
        want.append(LM.columns(queries[q], targets[t], qs, ts, bt, True, stand_in[q]))
    got = ctx.lddt_batch(queries, targets, tasks)
    for k, ((n, cols), w) in enumerate(zip(got, want)):
        assert n == len(w) and LK.same_bits(cols, w), ("lddt task", k, tasks[k][:4], np.flatnonzero(~((cols == w) | (np.isnan(cols) & np.isnan(w))))[:5])
    assert all(np.isfinite(w).all() and len(set(w.tolist())) > len(w) // 2 for w in want)          # every column has neighbours; the values are not one constant
    # TM: every task under its alignment length and under its query's length
    tm_tasks = []
    for q, t, qs, ts, bt in tasks:
        aln, q_len, _t_len = TC.norm_lengths(qs, ts, bt, queries[q].shape[1], targets[t].shape[1])
        tm_tasks += [(q, t, qs, ts, bt, aln), (q, t, qs, ts, bt, q_len)]
    model = TC.model_raw(queries, targets, tm_tasks)
    dev = TC.raw_of_device(ctx.tm_batch(queries, targets, tm_tasks))
    bad = [k for k in range(len(tm_tasks)) if dev[k].tobytes() != model[k].tobytes()]
    assert not bad, [(k, tm_tasks[k][:4], tm_tasks[k][5], TC.as_floats(dev[k]), TC.as_floats(model[k])) for k in bad[:4]]


# ---- 7. through Search -------------------------------------------------------------------------------------------------------------------------------------------
def test_search_with_a_query_of_65535_residues(ctx):
    """Search.prefilter and Search.align(with_backtrace=True): the hit list of gapless_model; per accepted record the score (forward minus reversed),
    end cell and qLen of sw_model, start cell and backtrace of ba_model.  E-value and coverage are not the models' to state.  (The e-value network gives
    this uniformly random query a NEGATIVE lambda: every score comes out at e-value 24.6, above the default threshold of 10, in the compiled reference
    as here, and nothing is accepted.  The threshold is raised to 100 so that there are records to compare.)"""
    L = 65535
    w = LC.world(L)
    ctx.load_db(w.db)
    q3, qa = LC.query(L)
    par = api.default_params()
    par.alignmentType, par.addBacktrace, par.evalThr = 2, 1, 100.0
    s = api.Search(ctx, par)
    try:
        hits = s.prefilter(q3)
        _same_hits(hits, gm.select(w.scan_want(), par.minDiagScoreThr, -1, par.maxResListLen), "Search.prefilter")
        ids = np.array([int(i) for i in hits["id"] if int(i) in set(w.sw_ids().tolist())], np.uint32)
        planted = [i for i in w.ids("sw_fwd", "sat") if i in set(ids.tolist())]
        assert len(planted) >= 12
        res, bts = s.align(qa, q3, ids, with_backtrace=True)
    finally:
        s.close()
    fwd, rev = w.sw_want(2, False, ids), w.sw_want(2, True, ids)
    where = {int(i): k for k, i in enumerate(ids)}
    q = LC.sw_query(L, 2)
    bias = q.cbAf.astype(np.int64) + q.cb3f.astype(np.int64)
    assert set(planted) <= {int(r["dbKey"]) for r in res}, "a planted window was not accepted"
    traced = 0
    for r, bt in zip(res, bts):
        i = int(r["dbKey"])
        f, b = fwd[where[i]], rev[where[i]]
        got = (int(r["score"]), int(r["qEndPos"]), int(r["dbEndPos"]), int(r["qLen"]), int(r["dbLen"]))
        assert got == (int(f["score"]) - int(b["score"]), int(f["qEnd"]), int(f["dbEnd"]), L, int(w.db.lengths[i])), (i, w.kind[i], w.info[i], got, f, b)
        if w.kind[i] != "sw_fwd":
            continue
        t3, ta = K.target(w.db, i)
        qe, de = int(f["qEnd"]), int(f["dbEnd"])
        c = B.model_case(f"search_{i}", q.qa[:qe + 1], q.q3[:qe + 1], bias[:qe + 1], ta[:de + 1], t3[:de + 1], int(f["score"]))
        want = c.expected(qe, de)
        assert c.cls == "A" and want["status"] == 1
        assert (int(r["qStartPos"]), int(r["dbStartPos"]), LM.expand(bt)) == (want["qStart"], want["dbStart"], want["backtrace"]), (i, w.info[i], r, bt, want)
        traced += 1
    assert traced >= 12

"""An answer does not depend on what the context ran before.  Every test keeps ONE context alive through a scripted sequence of calls and compares each
step with the model of that step alone (tests/history_cases.py: gapless_model, sw_model and sw_cases' frozen records, the C k-mer oracle, lddt_model,
tm_cases' frozen fixture answers, ba_model's frozen cases) -- never with a second run of the device.  Where the code keeps something from one call for
the next (reversed records of row-tiled SW queries, scan results behind the score getters, the form of the k-mer count pass, batch sizes, LDDT norms,
SW images) the test also asserts, from fsgpu_history_counters, that the carried state was used where it may be and not where it may not."""
import ctypes as C

import numpy as np
import pytest

import gapless_model as gm
import history_cases as HC
import sw_cases as K
import tm_cases as TC
from foldseek_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def cus():
    """torch asks for the device before the library opens it, whichever test of the file is selected (as bench.py does)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- A1: row-tiled SW across gap costs and databases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["profiles", "compact"])
def test_row_tiled_sw_across_gap_costs_and_databases(entry, monkeypatch):
    """A forward call over a query of 1025 residues (two row tiles) leaves the reversed records of its pairs for the reversed call.  They may be handed out
    only while gap costs, profiles, target ids AND database are those of the forward call."""
    for k in ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT"):
        monkeypatch.delenv(k, raising=False)
    qs, ids = HC.sw_history()
    n_long = len(ids[0])
    assert len(qs[0].q3) == 1025 and len(qs[1].q3) == 64 and n_long == 8
    lens = K.main_db().lengths[ids[0].astype(np.int64)]
    assert lens.min() == 1 and (lens > 64).any()
    # the sequences prove something only if the model's reversed records differ between the two settings of each
    assert (HC.sw_want(0, 10, 1, 1)[0] != HC.sw_want(0, 12, 2, 1)[0]).any(), "gap costs must show in a reversed record of the row-tiled query"
    assert (HC.sw_want(0, 10, 1, 1)[0] != HC.sw_want(1, 10, 1, 1)[0]).any(), "the database must show in a reversed record of the row-tiled query"
    ctx = api.Context(0)
    try:
        def step(db, direction, go, ge, launched, reused, what):
            got = HC.history_run(ctx, entry, direction, go, ge)
            for i, w in enumerate(HC.sw_want(db, go, ge, direction)):
                HC.sw_same(got[i], w, (entry, what, "query", i))
            c = ctx.history_counters()
            assert (c["sw_long_launched"], c["sw_long_reused"]) == (launched, reused), (entry, what, c)

        ctx.load_db(K.main_db())
        step(0, 0, 10, 1, n_long, 0, "forward")
        step(0, 1, 10, 1, 0, n_long, "reversed, nothing changed: the kept records answer")
        step(0, 1, 10, 1, n_long, 0, "reversed again: the records went with the call that used them")
        step(0, 0, 10, 1, n_long, 0, "forward 10/1")
        step(0, 1, 12, 2, n_long, 0, "reversed 12/2 after forward 10/1")
        step(0, 0, 10, 1, n_long, 0, "forward on the first database")
        ctx.load_db(HC.second_main_db())
        step(1, 1, 10, 1, n_long, 0, "reversed after another database was loaded")
        step(1, 0, 12, 2, n_long, 0, "forward 12/2 on the second database")
        step(1, 1, 12, 2, 0, n_long, "reversed 12/2, nothing changed")
    finally:
        ctx.close()


# ---- A2: reloading a database into a used context ---------------------------------------------------------------------------------------------------------
def reload_sequence(sizes):
    """one context, the scan databases of these sizes loaded one after the other; see test_reloading_a_database_into_a_used_context"""
    _, _, _, m8, _ = HC.kmer_matrices()
    order = [9, 0, 1, 2, 3, 4, 5, 6, 7, 8]                          # the row-tiled query first: it runs on its own, behind the batch
    ctx = api.Context(0)
    try:
        for n in sizes:
            w = HC.scan_world(n)
            ctx.load_db(w.db)
            assert ctx.n == n
            with pytest.raises(api.FsgpuError, match="no scan results"):
                ctx.gapless_scores()
            for k in (0, 1, len(order) - 1):
                with pytest.raises(api.FsgpuError, match="no batched scan results"):
                    ctx.gapless_scores_multi(k)
            idents = [-1] * len(order)
            idents[2], idents[5] = int(np.argmin(w.want[1])), n - 1
            w.check_batch(ctx, order, idents, 15, 50, ("batch", n))
            with pytest.raises(api.FsgpuError, match="no batched scan results"):
                ctx.gapless_scores_multi(0)                         # the row-tiled member has no slice
            for i in (3, 9, 0):
                w.check_single(ctx, i, 15, 50, ("single", n))
            w.check_batch(ctx, order[1:4], [-1, -1, -1], 15, 50, ("small batch after single scans", n))
            ctx.kmer_index_build(m8, kmer_thr=78)
            HC.scan_kmer_set(n).check(ctx, ("k-mer", n), 100)
    finally:
        ctx.close()


def test_reloading_a_database_into_a_used_context():
    """600 targets, then 9 000 (three selection chunks, larger than anything the context has sized its buffers for), then 5 (one partial stripe): on each
    a batched scan of mixed classes with a pair and the row-tiled 897, single scans, a k-mer index build and search, all against the model / oracle of
    THAT database.  Right after a load the score getters have nothing to hand out: they refuse and copy nothing."""
    assert HC.SCAN_SIZES == (600, 9000, 5)
    reload_sequence(HC.SCAN_SIZES)


# ---- A3: k-mer history -----------------------------------------------------------------------------------------------------------------------------------
WORKGROUP, WAVE = 1, 2


def test_kmer_count_and_list_passes_in_mixed_forms():
    """The count pass takes its form from the PREVIOUS batch of the context, the list pass from this batch's own count: dense, sparse, dense, sparse on one
    context runs k_kmer_count with k_kmer_lists_w and k_kmer_count_w with k_kmer_lists, which no forced-form test reaches.  The list kernels write into
    slots the count kernels sized: every call must still equal the oracle."""
    w = HC.kmer_world()
    _, _, _, m8, _ = HC.kmer_matrices()
    ctx = api.Context(0)
    try:
        ctx.load_db(w["db"])
        ctx.kmer_index_build(m8, kmer_thr=78)
        forms = []
        for name in ("dense", "sparse", "dense", "sparse"):
            s = w[name]
            s.check(ctx, name, 100)
            per_pos = float(ctx.kmer_counts()[0]) / s.positions
            assert per_pos >= 2048 if name == "dense" else per_pos < 128, (name, per_pos)
            c = ctx.history_counters()
            assert c["kmer_batches"] == 1 and c["kmer_last_batch_queries"] == len(s.queries), c
            forms.append((c["kmer_count_form"], c["kmer_list_form"]))
        assert forms == [(WORKGROUP, WORKGROUP), (WORKGROUP, WAVE), (WAVE, WORKGROUP), (WORKGROUP, WAVE)], forms
    finally:
        ctx.close()


def test_kmer_batches_are_cut_by_history_and_answers_are_not():
    """A context without history cuts a call into device batches of at most 32 queries; once it has seen what a query costs, 70 cheap queries are one
    batch.  Both cuts of the same call equal the oracle."""
    w = HC.kmer_world()
    _, _, _, m8, _ = HC.kmer_matrices()
    ctx = api.Context(0)
    try:
        ctx.load_db(w["db"])
        ctx.kmer_index_build(m8, kmer_thr=78)
        w["many"].check(ctx, "70 queries, no history", 100)
        first = ctx.history_counters()
        assert first["kmer_batches"] > 1 and first["kmer_last_batch_queries"] < 70, first
        w["many"].check(ctx, "70 queries again", 100)
        second = ctx.history_counters()
        assert second["kmer_batches"] == 1 and second["kmer_last_batch_queries"] == 70, second
        w["dense"].check(ctx, "dense after sparse batches", 100)
        w["many"].check(ctx, "70 queries after a dense call", 100)
    finally:
        ctx.close()


KMER_HIT_BUDGET = 2.4e8          # fsgpu_kmer.hip kKmerHitBudget: index hits of one device batch


def test_a_heavy_kmer_call_cuts_the_next_one_small_and_answers_are_not_cut():
    """kmerHitsPerQuery, the index hits per query of the last batch, sizes the next batch: after one query of 1.2e8 hits the next call starts in batches
    of at most two queries, and grows again once it has seen cheap ones.  Then three queries of 1.64e8 hits in ONE call exceed twice the budget: the
    batch is abandoned after its count stage, kmerBatchCap halves it (3 -> 1) and the call runs one query at a time; the cap holds for the next
    call and is only relaxed after four batches in a row went through.  Every call equals the oracle."""
    w = HC.heavy_kmer_world()
    _, _, _, m8, _ = HC.kmer_matrices()
    heavy, heaviest, many = w["heavy"], w["heaviest"], w["many"]
    assert heavy.index_hits > KMER_HIT_BUDGET / 3 and len(many.queries) == 70          # budget / hits < 3: batches of at most two
    assert heaviest.index_hits > 2 * KMER_HIT_BUDGET and len(heaviest.queries) == 3    # the split of a batch that is too large
    assert heaviest.index_hits / 3 * 2 <= 2 * KMER_HIT_BUDGET                          # ... while two of them would pass, so the halving is what is seen
    ctx = api.Context(0)
    try:
        ctx.load_db(w["db"])
        ctx.kmer_index_build(m8, kmer_thr=78)
        heavy.check(ctx, "one heavy query", 100)
        c = ctx.history_counters()
        assert c["kmer_batches"] == 1 and int(ctx.kmer_counts()[1]) == int(heavy.index_hits), (c, ctx.kmer_counts())
        many.check(ctx, "70 queries after the heavy one", 100)
        c = ctx.history_counters()
        assert c["kmer_batches"] > 1 and 1 <= c["kmer_first_batch_queries"] <= 2 < c["kmer_last_batch_queries"], c
        many.check(ctx, "70 queries again", 100)
        c = ctx.history_counters()
        assert c["kmer_batches"] == 1 and c["kmer_first_batch_queries"] == 70, c
        heaviest.check(ctx, "three heavier queries in one call", 100)
        c = ctx.history_counters()
        assert c["kmer_batches"] == 3 and c["kmer_first_batch_queries"] == c["kmer_last_batch_queries"] == 1, c
        many.check(ctx, "70 queries under the cap", 100)
        c = ctx.history_counters()
        assert c["kmer_first_batch_queries"] == 1 and c["kmer_batches"] > 4 and c["kmer_last_batch_queries"] > 1, c
    finally:
        ctx.close()


# ---- A4: LDDT and TM kept state ----------------------------------------------------------------------------------------------------------------------------
def test_lddt_norms_are_kept_only_for_the_query_they_belong_to():
    """The norms of a single query are kept for the next call with the same coordinates.  fsgpu_history_counters counts the launches of k_lddt_norm: it
    is skipped exactly for a repeated single query whose norms are still in the buffer -- not for another query of the same length, not after a
    two-query batch, not after the buffer grew."""
    w = HC.lddt_world()
    A, Bq, Cq, big, T = w["A"], w["B"], w["C"], w["big"], w["targets"]
    bt1, bt2, bt3 = w["bts"]
    assert A.shape == Bq.shape and big.shape[1] > 1024
    lists_A = ([(0, 0, 0, 0, bt1)], [(0, 1, 2, 3, bt2), (0, 0, 5, 1, bt1)], [(0, 0, 0, 0, bt3)])
    ctx = api.Context(0)
    try:
        def step(queries, tasks, runs, what):
            HC.lddt_check(ctx.lddt_batch(queries, T, tasks), HC.lddt_want(queries, T, tasks), what)
            assert ctx.history_counters()["lddt_norm_runs"] == runs, (what, ctx.history_counters())

        step([A], lists_A[0], 1, "A, first list")
        step([A], lists_A[1], 1, "A, second list: norms kept")
        step([A], lists_A[2], 1, "A, third list: norms kept")
        step([Bq], [(0, 2, 0, 0, bt3), (0, 2, 1, 2, bt1)], 2, "B, as long as A")
        step([A, Cq], [(0, 0, 0, 0, bt1), (1, 3, 4, 2, bt2), (1, 3, 0, 0, "M" * 140)], 3, "two queries")
        step([A], lists_A[1], 4, "A after the two-query batch")
        step([A], lists_A[0], 4, "A again: norms kept")
        step([big], [(0, 4, 3, 1, "M" * 300 + "I" + "M" * 50), (0, 4, 900, 900, "M" * 200)], 5, "a query that makes the norm buffer grow")
        step([A], lists_A[2], 6, "A after the buffer grew")
        step([A], lists_A[0], 6, "A again: norms kept")
    finally:
        ctx.close()


def test_tm_answers_survive_larger_calls_and_a_refusal():
    """the fixture list, the LDS-limit edge list (workspaces grow, hits spill to global memory), a refused task, the fixture list again: byte for byte
    the frozen answers both times (the fixture tasks allow no difference)"""
    coords, tasks = TC.fixture_tasks()
    want = TC.frozen_raw("fixture")
    eq, et, etasks = TC.edge()
    ewant = TC.frozen_raw("edge")
    rng = np.random.default_rng(3)
    q, t = TC._walk(rng, 20), TC._walk(rng, 20)
    ctx = api.Context(0)
    try:
        first = TC.raw_of_device(ctx.tm_batch(coords, coords, tasks))
        assert first.tobytes() == want.tobytes(), np.flatnonzero((first != want).any(axis=1))[:10]
        got = TC.raw_of_device(ctx.tm_batch(eq, et, etasks))
        assert got.tobytes() == ewant.tobytes(), np.flatnonzero((got != ewant).any(axis=1))[:10]
        with pytest.raises(api.FsgpuError):
            ctx.tm_batch([q], [t], [(0, 0, 0, 0, "M" * 21, 20)])
        again = TC.raw_of_device(ctx.tm_batch(coords, coords, tasks))
        assert again.tobytes() == want.tobytes(), np.flatnonzero((again != want).any(axis=1))[:10]
    finally:
        ctx.close()


# ---- A5: refusals leave nothing behind ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_nothing_behind(monkeypatch):
    """every entry refuses one call (bad target id, bad selection index, gapOpen <= gapExtend, bins = 3, an oversize query, a second launch before the
    finish) and then answers its smallest valid call like its model: no pending flag, no half-written plan survives a refusal"""
    for k in ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT"):
        monkeypatch.delenv(k, raising=False)
    w = HC.combo()
    db = w["db"]
    L = api.lib()
    qs, ids = HC.sw_history()
    short, short_ids = qs[1], HC.on_combo(ids[1])
    prof = HC.sw_profiles(short)
    m3, mA = K.matrices()
    too_long = api.FSGPU_MAX_SEQ_LEN + 1
    _, pssm, cap = HC.scan_queries()[1]
    scan_want = HC.combo_scan_want()[1]
    _, _, _, m8, _ = HC.kmer_matrices()
    ctx = api.Context(0)
    try:
        ctx.load_db(db)
        n = ctx.n
        refused = lambda **kw: pytest.raises(api.FsgpuError, **kw)  # noqa: E731

        def sw_ok(what):
            for d in (0, 1):
                got = HC.history_run(ctx, "profiles", d, 10, 1, HC.on_combo) if what == "sw_multi_dir" else HC.history_run(ctx, "compact", d, 10, 1, HC.on_combo)
                for i, want in enumerate(HC.sw_want(0, 10, 1, d)):
                    HC.sw_same(got[i], want, (what, "after refusals", d, i))

        # fsgpu_gapless_scan_multi
        with refused(match="bad query"):
            ctx.gapless_scan_multi([(pssm, cap, -1), (np.zeros((21, 0), np.int8), 100, -1)], 15, 40)
        with refused(match="bad query"):
            ctx.gapless_scan_multi([(np.zeros((21, too_long), np.int8), 100, -1)], 15, 40)
        with refused(match="bad argument"):
            ctx.gapless_scan_multi([(pssm, cap, -1)], 15, 0)
        HC.combo_scan_check(ctx, "scan_multi after refusals", order=(1,))
        # fsgpu_gapless_launch / fsgpu_gapless_finish
        p = np.ascontiguousarray(pssm, np.int8)
        hits, nout = np.zeros(40, api.HIT_DT), C.c_int(0)
        pp, hp = p.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)
        assert L.fsgpu_gapless_finish(ctx.h, hp, C.byref(nout)) != 0 and b"no gapless scan in flight" in L.fsgpu_last_error(ctx.h)
        assert L.fsgpu_gapless_launch(ctx.h, pp, p.shape[1], cap, 15, -1, 0) != 0
        assert L.fsgpu_gapless_launch(ctx.h, pp, too_long, cap, 15, -1, 40) != 0
        assert L.fsgpu_gapless_finish(ctx.h, hp, C.byref(nout)) != 0                     # the refused launches left nothing in flight
        assert L.fsgpu_gapless_launch(ctx.h, pp, p.shape[1], cap, 15, -1, 40) == 0
        assert L.fsgpu_gapless_launch(ctx.h, pp, p.shape[1], cap, 15, -1, 40) != 0 and b"not finished" in L.fsgpu_last_error(ctx.h)
        with refused(match="not finished"):
            ctx.gapless_scan_multi([(pssm, cap, -1)], 15, 40)
        assert L.fsgpu_gapless_finish(ctx.h, hp, C.byref(nout)) == 0
        HC.same_hits(hits[:nout.value], gm.select(scan_want, 15, -1, 40), "launch / finish around refused calls")
        assert (ctx.gapless_scores().astype(np.int32) == scan_want).all()
        HC.same_hits(ctx.gapless_scan(pssm, cap, min_score=15, identity=-1, max_res=40), gm.select(scan_want, 15, -1, 40), "scan after launch / finish")
        # fsgpu_sw_batch
        with refused(match="target id out of range"):
            ctx.sw_batch(*prof, np.array([short_ids[0], n], np.uint32))
        with refused(match="gapOpen > gapExtend"):
            ctx.sw_batch(*prof, short_ids, gap_open=1, gap_extend=1)
        f, r = ctx.sw_batch(*prof, short_ids)
        HC.sw_same(f, HC.sw_want(0, 10, 1, 0)[1], "sw_batch after refusals, forward")
        HC.sw_same(r, HC.sw_want(0, 10, 1, 1)[1], "sw_batch after refusals, reversed")
        # fsgpu_sw_multi_dir
        one = [(*prof, 64, short_ids)]
        with refused(match="selection index out of range"):
            ctx.sw_multi_dir(one, 0, selections=[[0, len(short_ids)]])
        with refused(match="target id out of range"):
            ctx.sw_multi_dir([(*prof, 64, np.array([n], np.uint32))], 0)
        with refused(match="gapOpen > gapExtend"):
            ctx.sw_multi_dir(one, 0, gap_open=2, gap_extend=2)
        with refused(match="bad query"):
            ctx.sw_multi_dir([(*prof, too_long, short_ids)], 0)
        sw_ok("sw_multi_dir")
        # fsgpu_sw_multi_dir_c
        cq = (short.qa, short.q3, short.cbAf, short.cb3f, short.cbAr, short.cb3r)
        with refused(match="selection index out of range"):
            ctx.sw_multi_dir_c(m3, mA, [(*cq, short_ids)], 0, selections=[[-1]])
        with refused(match="target id out of range"):
            ctx.sw_multi_dir_c(m3, mA, [(*cq, np.array([n + 7], np.uint32))], 1)
        with refused(match="gapOpen > gapExtend"):
            ctx.sw_multi_dir_c(m3, mA, [(*cq, short_ids)], 0, gap_open=1, gap_extend=3)
        z = np.zeros(too_long, np.uint8)
        with refused(match="bad query"):
            ctx.sw_multi_dir_c(m3, mA, [(z, z, None, None, None, None, short_ids)], 0)
        sw_ok("sw_multi_dir_c")
        # fsgpu_kmer_search
        ks = HC.combo_kmer_set()
        with refused(match="index not built"):
            ctx.kmer_search(ks.prep, max_res=100)
        ctx.kmer_index_build(m8, kmer_thr=78)
        with refused(match="bins must be a power of two"):
            ctx.kmer_search(ks.prep, max_res=100, bins=3)
        with refused():
            ctx.kmer_search(ks.prep, max_res=0)
        ks.check(ctx, "k-mer search after refusals", 100)
        # fsgpu_block_backtrace
        bad = list(w["tasks"])
        bad[3] = (bad[3][0], n, bad[3][2], bad[3][3], bad[3][4])
        with refused(match="task out of range"):
            ctx.block_backtrace(*w["tables"], w["queries"], bad, 10, 1)
        with refused(match="gap costs"):
            ctx.block_backtrace(*w["tables"], w["queries"], w["tasks"], 1, 1)
        HC.btrace_check(HC.btrace_run(ctx), "block_backtrace after refusals")
        # and once more round the entries: nothing of the above lingers
        HC.combo_scan_check(ctx, "scan_multi at the end", order=(1,))
        sw_ok("sw_multi_dir")
    finally:
        ctx.close()


# ---- A6: interleaving on one context -------------------------------------------------------------------------------------------------------------------------
def test_interleaved_entries_keep_their_state_apart(monkeypatch):
    """compact SW forward, a batched scan, block backtraces under both footprints, an explicit-target SW batch, then compact SW reversed over the first
    queries: the reversed call still finds the images the forward call built, and every step equals its model"""
    for k, v in K.ENV_32.items():
        monkeypatch.setenv(k, v)
    w = HC.combo()
    c, _ = HC.compact_call()
    ctx = api.Context(0)
    try:
        ctx.load_db(w["db"])
        plan = HC.compact_run(ctx, 0, "first")
        assert plan["images_built"] > 0 and plan["profile_pairs"] == 0, plan
        HC.combo_scan_check(ctx, "scan between the SW calls")
        default = HC.btrace_run(ctx)
        HC.btrace_check(default, "default footprint")
        ctx.block_backtrace_footprint(1)
        try:
            one = HC.btrace_run(ctx)
        finally:
            ctx.block_backtrace_footprint(0)
        HC.btrace_check(one, "one workgroup per compute unit")
        HC.btrace_check(HC.btrace_run(ctx), "footprint reset")
        q, ids = c.queries[2], c.ids[2]
        targets = [K.target(K.main_db(), int(i)) for i in ids]
        f, r = ctx.sw_batch_seqs(*HC.sw_profiles(q), [t[1] for t in targets], [t[0] for t in targets])
        HC.sw_same(f, HC.compact_want(0)[2], "explicit targets, forward")
        HC.sw_same(r, HC.compact_want(1)[2], "explicit targets, reversed")
        plan = HC.compact_run(ctx, 1, "reversed after the other entries")
        assert plan["images_built"] == 0, plan
        plan = HC.compact_run(ctx, 0, "forward again")
        assert plan["images_built"] == 0, plan
    finally:
        ctx.close()

"""Clones answer as a lone context does.  bench.py, the modules and the adapters run several feeder threads, each on its own fsgpu_clone of one context;
here Python threads do (ctypes releases the GIL inside the library): one process, a handful of contexts, one device.  All workers of a test wait at a
barrier before their first call and then run a fixed, small number of rounds; every result is compared with the model of that call alone
(tests/history_cases.py), never with another run of the device.  Workers are daemon threads joined with a limit of 120 s (a cap, not a measurement:
the work takes seconds): one that has not returned fails the test, which names the entry it was in."""
import os
import threading
import time

import numpy as np
import pytest

import history_cases as HC
import tm_cases as TC
from foldseek_amd import api, synth

pytestmark = pytest.mark.gpu
JOIN_S = 120


@pytest.fixture(scope="module", autouse=True)
def cus():
    """torch asks for the device before the library opens it, whichever test of the file is selected (as bench.py does)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class Worker(threading.Thread):
    """runs body(self) behind the barrier; body sets self.where to the entry it is about to call"""

    def __init__(self, name, barrier, body):
        super().__init__(name=name, daemon=True)
        self.barrier, self.body, self.where, self.error = barrier, body, "the barrier", None

    def run(self):
        try:
            self.barrier.wait(JOIN_S)
            self.body(self)
            self.where = "done"
        except BaseException as e:  # noqa: BLE001 -- handed to the test's thread
            self.error = e


def run_all(bodies, also=None):
    """one worker per (name, body), all released together; `also` runs on the calling thread meanwhile.  Whatever `also` raises is kept until the
    workers have been joined: the caller closes the workers' contexts on its way out, which it may only do once they have stopped using them.
    Raises the calling thread's error, else the first worker's."""
    barrier = threading.Barrier(len(bodies))
    workers = [Worker(name, barrier, body) for name, body in bodies]
    t0 = time.monotonic()
    for w in workers:
        w.start()
    own = None
    if also is not None:
        try:
            also()
        except BaseException as e:  # noqa: BLE001 -- re-raised below, after the join
            own = e
    for w in workers:
        w.join(max(0.0, JOIN_S - (time.monotonic() - t0)))
    stuck = [(w.name, w.where) for w in workers if w.is_alive()]
    assert not stuck, f"workers that did not return within {JOIN_S} s, and the entry each was in: {stuck}"
    if own is not None:
        raise own
    for w in workers:
        if w.error is not None:
            raise AssertionError(f"worker {w.name} failed in {w.where}: {w.error!r}") from w.error


# ---- B1: first use under contention ---------------------------------------------------------------------------------------------------------------------
def test_first_use_of_a_database_by_four_clones_at_once():
    """a database nothing has run on yet: four clones issue their first batched scan together, so the work lists of every register class (built on first
    use under DbStore::itemMutex) are first asked for concurrently, and their scans chain through DbStore::lastScanDone.  Same classes, other
    profiles and caps per clone; three rounds; every slice and hit list against the model; then the same sets on the parent alone."""
    w = HC.scan_world(600)
    sets = HC.clone_scan_sets()
    n = len(sets[0])
    parent = api.Context(0)
    parent.load_db(w.db)
    clones = [parent.clone() for _ in range(4)]
    try:
        def body(k):
            def run(self):
                for r in range(3):
                    self.where = f"gapless_scan_multi, round {r}"
                    order = [(i + r + k) % n for i in range(n)]
                    HC.clone_scan_check(clones[k], sets[k], order, (k, r))
            return run
        run_all([(f"clone {k}", body(k)) for k in range(4)])
        for k in range(4):
            HC.clone_scan_check(parent, sets[k], list(range(n)), ("parent", k))
    finally:
        for c in clones:
            c.close()
        parent.close()


# ---- B2: different entries at once ------------------------------------------------------------------------------------------------------------------------
def test_different_entries_on_four_clones_at_once(monkeypatch):
    """one clone scans, one runs the SW entries forward and reversed (the 1025-residue query included), one searches k-mers, one runs block backtraces,
    LDDT and TM; four rounds; every result against its model"""
    for k in ("FSGPU_SW3_MID", "FSGPU_SW3_SHORT", "FSGPU_KMER_WAVE", "FSGPU_BT_PASS2"):
        monkeypatch.delenv(k, raising=False)
    w = HC.combo()
    _, _, _, m8, _ = HC.kmer_matrices()
    ks = HC.combo_kmer_set()
    HC.combo_scan_want()
    lw = HC.lddt_world()
    ltasks = [(0, 0, 0, 0, lw["bts"][0]), (1, 2, 1, 2, lw["bts"][0]), (0, 1, 2, 3, lw["bts"][1])]
    lqueries = [lw["A"], lw["B"]]
    lwant = HC.lddt_want(lqueries, lw["targets"], ltasks)
    coords, ttasks = TC.fixture_tasks()
    twant = TC.frozen_raw("fixture")
    for db, go, ge, d in ((0, 10, 1, 0), (0, 10, 1, 1)):
        HC.sw_want(db, go, ge, d)
    parent = api.Context(0)
    parent.load_db(w["db"])
    parent.kmer_index_build(m8, kmer_thr=78)
    clones = [parent.clone() for _ in range(4)]
    rounds = 4
    try:
        def scan(self):
            for r in range(rounds):
                self.where = f"gapless_scan_multi, round {r}"
                HC.combo_scan_check(clones[0], ("scan", r))

        def sw(self):
            for r in range(rounds):
                for entry in ("compact", "profiles"):
                    for d in (0, 1):
                        self.where = f"sw_multi_dir{'_c' if entry == 'compact' else ''} direction {d}, round {r}"
                        got = HC.history_run(clones[1], entry, d, 10, 1, HC.on_combo)
                        for i, want in enumerate(HC.sw_want(0, 10, 1, d)):
                            HC.sw_same(got[i], want, (entry, d, r, i))

        def kmer(self):
            for r in range(rounds):
                self.where = f"kmer_search, round {r}"
                ks.check(clones[2], ("k-mer", r), 100)

        def structure(self):
            for r in range(rounds):
                self.where = f"block_backtrace, round {r}"
                HC.btrace_check(HC.btrace_run(clones[3]), ("backtrace", r))
                self.where = f"lddt_batch, round {r}"
                HC.lddt_check(clones[3].lddt_batch(lqueries, lw["targets"], ltasks), lwant, ("lddt", r))
                self.where = f"tm_batch, round {r}"
                got = TC.raw_of_device(clones[3].tm_batch(coords, coords, ttasks))
                assert got.tobytes() == twant.tobytes(), ("tm", r, np.flatnonzero((got != twant).any(axis=1))[:10])

        run_all([("scan", scan), ("sw", sw), ("kmer", kmer), ("backtrace, lddt, tm", structure)])
    finally:
        for c in clones:
            c.close()
        parent.close()


# ---- B3: lifetimes -----------------------------------------------------------------------------------------------------------------------------------------
def test_clones_outlive_a_sibling_and_the_parent():
    """a clone is closed right after its own scan, while its event is the one the next scan of the database waits for; then, with two clones scanning in
    a loop, another clone scans and goes, and the parent goes: the survivors keep answering like the model and close cleanly"""
    w = HC.scan_world(600)
    sets = HC.clone_scan_sets()
    n = len(sets[0])
    parent = api.Context(0)
    parent.load_db(w.db)
    a, b, c = parent.clone(), parent.clone(), parent.clone()
    try:
        # without contention first: c owns the database's last scan event when it goes, a is the next to scan
        HC.clone_scan_check(c, sets[2], [1, 2, 3], "c alone")
        c.close()
        HC.clone_scan_check(a, sets[0], [1, 2, 3], "a after c is gone")

        def loop(ctx, members, k):
            def run(self):
                for r in range(6):
                    self.where = f"gapless_scan_multi, round {r}"
                    HC.clone_scan_check(ctx, members, [(i + r) % n for i in range(n)], (k, r))
            return run

        def meanwhile():
            d = parent.clone()
            HC.clone_scan_check(d, sets[3], [0, 4, 5, 9], "d between the others")
            d.close()
            HC.clone_scan_check(parent, sets[2], [2, 3], "the parent's last scan")
            parent.close()

        run_all([("a", loop(a, sets[0], "a")), ("b", loop(b, sets[1], "b"))], also=meanwhile)
        assert parent.h is None
        HC.clone_scan_check(a, sets[0], list(range(n)), "a after the parent is gone")
        w.check_single(b, 9, 15, 50, "b, row-tiled single scan after the parent is gone")
        assert a.n == b.n == 600
    finally:
        for x in (a, b, c, parent):
            x.close()


def test_a_clone_survives_the_parents_reload_and_close():
    """the parent scans (its event is the one the database's next scan waits for), a clone is made, the parent loads ANOTHER database and is closed:
    the clone's next scan must not wait on the event that went with the parent.  One thread, one fixed sequence; the clone and the parent are each
    held to the model of their own database."""
    w, other = HC.scan_world(600), HC.scan_world(5)
    sets = HC.clone_scan_sets()
    parent = api.Context(0)
    parent.load_db(w.db)
    clone = None
    try:
        HC.clone_scan_check(parent, sets[1], [1, 2, 3], "the parent, first database")
        clone = parent.clone()
        parent.load_db(other.db)
        other.check_batch(parent, [2, 3, 5], [-1, -1, -1], 15, 50, "the parent, second database")
        assert parent.n == 5 and clone.n == 600
        parent.close()
        HC.clone_scan_check(clone, sets[0], [1, 2, 3, 9], "the clone after the parent reloaded and went")
        w.check_single(clone, 3, 15, 50, "the clone, single scan")
    finally:
        if clone is not None:
            clone.close()
        parent.close()


# ---- B4: who has the index ---------------------------------------------------------------------------------------------------------------------------------
def test_a_clone_keeps_the_index_it_was_made_with():
    """fsgpu_clone copies the k-mer index the source holds at that time (include/fsgpu.h): a clone made before the build has none, one made after it
    answers like the parent, and keeps answering by the old index's parameters after the parent has built another -- each held to an oracle built
    with its own parameters"""
    w = HC.kmer_world()
    _, _, _, m8, _ = HC.kmer_matrices()
    old, new = w["dense"], HC.kmer_rebuilt()
    differ = [i for i in range(len(old.queries)) if len(old.want[i][0]) != len(new.want[i][0]) or (old.want[i][0] != new.want[i][0]).any()]
    assert differ, "the two indexes must give different answers for the test to tell them apart"
    parent = api.Context(0)
    parent.load_db(w["db"])
    early = parent.clone()
    parent.kmer_index_build(m8, kmer_thr=78)
    late = parent.clone()
    try:
        with pytest.raises(api.FsgpuError, match="index not built"):
            early.kmer_search(old.prep, max_res=100)
        assert early.kmer_index_entries == 0 and late.kmer_index_entries == parent.kmer_index_entries > 0
        old.check(parent, "parent, first index", 100)
        old.check(late, "clone made after the build", 100)
        w["sparse"].check(late, "clone made after the build, sparse", 100)
        entries = parent.kmer_index_entries
        parent.kmer_index_build(m8, kmer_thr=HC.REBUILD_THR)
        assert parent.kmer_index_entries < entries == late.kmer_index_entries
        new.check(parent, "parent, rebuilt index", 100)
        old.check(late, "the older clone after the parent's rebuild", 100)
        with pytest.raises(api.FsgpuError, match="index not built"):
            early.kmer_search(old.prep, max_res=100)
        newest = parent.clone()
        try:
            new.check(newest, "clone made after the rebuild", 100)
        finally:
            newest.close()
        parent.close()
        old.check(late, "the older clone after the parent is gone", 100)
    finally:
        for x in (early, late, parent):
            x.close()


# ---- B5: two Search objects on clones with backtraces ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def btrace_world():
    """the database, queries and hit lists of tests/test_btrace_gpu.py, and the single-threaded answer that file holds the device aligner to: the
    records of one align_batch with the HOST backtrace (FSGPU_DEVICE_BACKTRACE=0).  Their SW scores and end cells come from the device's SW kernels,
    not from a model (test_sw3_model_gpu.py holds those to sw_model); what is compared here is start positions, identities and CIGARs."""
    q3, qa = synth.make_queries(20, seed=505, lo=40, hi=900)
    q3[0], qa[0] = q3[0][:35], qa[0][:35]
    q3[1], qa[1] = np.concatenate([q3[1], q3[2]])[:1500], np.concatenate([qa[1], qa[2]])[:1500]
    db = synth.make_db_fast(30000, (q3, qa), seed=606, homologs_per_query=40)
    ctx = api.Context(0)
    ctx.load_db(db)
    par = api.default_params()
    par.alignmentType, par.addBacktrace = 2, 1
    pre = api.Search(ctx)
    hits = [pre.prefilter(q)["id"][:300] for q in q3]
    pre.close()
    before = os.environ.get("FSGPU_DEVICE_BACKTRACE")
    os.environ["FSGPU_DEVICE_BACKTRACE"] = "0"
    try:
        s = api.Search(ctx, par)
        res, bts = s.align_batch(qa, q3, hits, with_backtrace=True)
        on_dev, total = s.backtrace_counts()
        s.close()
    finally:
        if before is None:
            os.environ.pop("FSGPU_DEVICE_BACKTRACE", None)
        else:
            os.environ["FSGPU_DEVICE_BACKTRACE"] = before
    assert on_dev == 0 and total >= 400
    yield dict(ctx=ctx, par=par, q3=q3, qa=qa, hits=hits, res=res, bts=bts, total=total)
    ctx.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_two_searches_on_clones_with_backtraces(btrace_world, mode, monkeypatch):
    """align_batch(with_backtrace=True) from two threads at once, each with its own Search on its own clone: under FSGPU_DEVICE_BACKTRACE=1 both use
    the device aligner, under =2 (shared with the host pool from 128 hits on) the thread that finds the device aligner busy answers on the host.
    Records and CIGARs are the single-threaded host answer; the device took hits in at least one thread."""
    bw = btrace_world
    monkeypatch.setenv("FSGPU_DEVICE_BACKTRACE", mode)
    if mode == "2":
        monkeypatch.setenv("FSGPU_BT_SHARE_MIN", "128")
    else:
        monkeypatch.delenv("FSGPU_BT_SHARE_MIN", raising=False)
    clones = [bw["ctx"].clone() for _ in range(2)]
    searches = [api.Search(c, bw["par"]) for c in clones]
    counts = [None, None]
    try:
        def body(k):
            def run(self):
                self.where = "align_batch"
                res, bts = searches[k].align_batch(bw["qa"], bw["q3"], bw["hits"], with_backtrace=True)
                counts[k] = searches[k].backtrace_counts()
                for q in range(len(res)):
                    assert res[q].tobytes() == bw["res"][q].tobytes(), (k, q)
                    assert bts[q] == bw["bts"][q], (k, q)
            return run
        run_all([(f"search {k}", body(k)) for k in range(2)])
        assert all(c[1] == bw["total"] for c in counts), counts
        assert max(c[0] for c in counts) > 0, counts
    finally:
        for s in searches:
            s.close()
        for c in clones:
            c.close()

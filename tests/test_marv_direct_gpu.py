"""`class Marv` (include/marv.h + foldseek_amd/csrc/host/marv_shim.cpp) called directly, through the forwarding C functions of oracle/marv_harness.cpp,
and held to tests/marv_cases.py: the saturation cap the shim recovers from the profile (both built-in matrices, a matrix it does not carry), the
sharding of the targets over 1 / 2 / 3 / 7 contexts (repacking, the unpadded tail, empty shards, id mapping, the merge and its tie order), the handle
bookkeeping, the caller's result buffer, the refusals (each in a child process: they end it) and, without the harness, the asynchronous halves of the
gapless scan on several contexts at once.  Every hit of every list is compared, exactly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gapless_model as gm
import helpers
import marv_cases as MC
import marv_lib as ML
from foldseek_amd import api

pytestmark = pytest.mark.gpu

NAMES = list(MC.cases())
_seen = {}                      # (case, maxSeqs) -> the list the first shard count gave: every other count must give the same bytes


def _marv(monkeypatch, shards, n, max_seqs):
    monkeypatch.setenv("FSGPU_MARV_SHARDS", str(shards))
    return ML.Marv(n, max_seqs)


def _load(m, db, data=None, offsets=None):
    return m.load_db(db.data3di if data is None else data, db.offsets if offsets is None else offsets, db.lengths)


def _check(m, name, what, want_scores=None):
    """one Marv::scan of a case: the list against the model's, the statistics, the records behind the capacity"""
    q = MC.cases()[name]
    want = MC.expected(name, m.max_seqs, want_scores)
    hits, buf, (n, overflows, seconds, gcups) = m.scan(q.seq, q.pssm)
    assert ML.untouched(buf[m.max_seqs:]), (what, name, "records behind results[maxSeqs] were written")
    assert n == len(want) == len(hits), (what, name, n, len(want))
    bad = np.flatnonzero((hits["id"] != want["id"]) | (hits["score"] != want["score"]))
    assert len(bad) == 0, (what, name, len(bad), bad[:5], hits[bad[:5]], want[bad[:5]])
    assert not hits["qEndPos"].any() and not hits["dbEndPos"].any(), (what, name)
    assert overflows == 0 and seconds >= 0 and gcups >= 0, (what, name, overflows, seconds, gcups)
    return hits


# ---- scan against the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", MC.SHARDS)
def test_scan_equals_the_model(shards, monkeypatch):
    """every query, maxSeqs = 1, a cut inside the group at the cap, n and more than n"""
    db = MC.world()["db"]
    for max_seqs in (1, MC.TIE_MAX_SEQS, db.n, db.n + 9):
        m = _marv(monkeypatch, shards, db.n, max_seqs)
        try:
            m.set_db(_load(m, db))
            for name in NAMES:
                hits = _check(m, name, (shards, max_seqs))
                first = _seen.setdefault((name, max_seqs), hits.tobytes())
                assert hits.tobytes() == first, (name, shards, max_seqs, "differs from another shard count")
        finally:
            m.close()


@pytest.mark.parametrize("shards", [1, 3])
def test_a_buffer_that_ends_with_the_last_residue(shards, monkeypatch):
    """no padding behind the last entry: with one shard the caller's buffer goes up as it is, with three the shim repacks and fills with X"""
    db = MC.world()["db"]
    data, off = MC.unpadded(db)
    assert len(data) % 4 != 0 and len(data) < len(db.data3di)
    for max_seqs in (MC.TIE_MAX_SEQS, db.n):
        m = _marv(monkeypatch, shards, db.n, max_seqs)
        try:
            m.set_db(_load(m, db, data, off))
            for name in NAMES:
                _check(m, name, ("unpadded", shards, max_seqs))
        finally:
            m.close()


@pytest.mark.parametrize("entries", [1, 2])
def test_fewer_entries_than_shards(entries, monkeypatch):
    db = MC.small_db(entries)
    for max_seqs in (1, 5):
        m = _marv(monkeypatch, 3, entries, max_seqs)
        try:
            m.set_db(_load(m, db))
            for name in ("3di_L300", "blosum62", "3di_L5"):
                hits = _check(m, name, ("small", entries, max_seqs), MC.scores_on(name, entries))
                assert len(hits) == min(entries, max_seqs)
        finally:
            m.close()


@pytest.mark.parametrize("shards", [1, 3])
def test_an_empty_database(shards, monkeypatch):
    m = _marv(monkeypatch, shards, 0, 10)
    try:
        h = m.load_db(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int32))
        assert h
        m.set_db(h)
        q = MC.cases()["3di_L64"]
        for _ in range(2):
            hits, buf, (n, overflows, seconds, gcups) = m.scan(q.seq, q.pssm)
            assert n == 0 and len(hits) == 0 and ML.untouched(buf) and overflows == 0 and gcups == 0.0       # no residues were scanned
    finally:
        m.close()


# ---- handles ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 3])
def test_handles(shards, monkeypatch):
    A, B = MC.world()["db"], MC.other_db()
    names = ("3di_L300", "blosum62", "3di_L5")
    m = _marv(monkeypatch, shards, A.n, MC.TIE_MAX_SEQS)
    try:
        hA, hB = _load(m, A), _load(m, B)
        assert hA and hB and hA != hB
        on = {"A": lambda what: [_check(m, k, what) for k in names], "B": lambda what: [_check(m, k, what, MC.scores_on(k, "B")) for k in names]}
        for step, (h, which) in enumerate(((hA, "A"), (hA, "A"), (hB, "B"), (hA, "A"), (hB, "B"), (hB, "B"))):
            m.set_db(h)
            on[which]((shards, "setDb", step, which))
        assert m.load_db_other(hA) == hA and m.load_db_other(hB, 12345) == hB           # loadDb(data, size, other) hands `other` back
        on["B"]((shards, "after loadDb(other)"))                                          # and changes nothing
        m.set_db_with_allocation(m.load_db_other(hA), b"an allocation handle of another process")
        on["A"]((shards, "setDbWithAllocation A"))
        m.set_db_with_allocation(hB)
        on["B"]((shards, "setDbWithAllocation B"))
        assert m.db_memory_handle() == (b"", 0)
        # sequenceLength == 0: no result, nothing written, whatever the other arguments are
        q = MC.cases()["3di_L5"]
        for pssm in (None, q.pssm):
            hits, buf, (n, overflows, _, gcups) = m.scan(np.zeros(0, np.uint8), pssm)
            assert n == 0 and ML.untouched(buf) and overflows == 0 and gcups == 0.0
        on["B"]((shards, "after an empty query"))
    finally:
        m.close()


# ---- refusals: Marv ends the process, so each runs in a child; one at a time ---------------------------------------------------------------------
_children = {"stopped": None}


def _blosum_profile_at_20_bits():
    """BLOSUM62 at 20 bits: the X row is -10, beyond what a rounded composition bias can be"""
    sub, _ = helpers.o_submat("BLOSUM62", 20.0)
    m = sub.reshape(21, 21).astype(np.int32)
    assert (m[MC.X] == -10).all() and np.abs(m).max() <= 127
    return m[:, np.arange(8) % 20].astype(np.int8).tobytes().hex()


@pytest.mark.parametrize("name", list(ML.REFUSALS))
def test_refusals_end_the_process_with_a_message(name):
    if _children["stopped"]:
        pytest.fail(f"not started: the child of {_children['stopped']} did not end with a refusal")
    shards, message = ML.REFUSALS[name]
    env = dict(os.environ, FSGPU_MARV_SHARDS=str(shards))
    extra = _blosum_profile_at_20_bits() if name == "blosum_like_other_scale" else None
    code = (f"import sys; sys.path[:0] = [{ML.ROOT!r}, {os.path.join(ML.ROOT, 'tests')!r}]; import marv_lib; "
            f"marv_lib.refusal_child({name!r}, {extra!r})")
    try:
        r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _children["stopped"] = name
        raise
    if r.returncode != 1:                                   # exit(EXIT_FAILURE) is the only end a refusal has
        _children["stopped"] = name
    assert r.returncode == 1, (name, r.returncode, r.stderr[-2000:])
    assert "Marv (fsgpu): " in r.stderr and message in r.stderr, (name, r.stderr[-2000:])


def test_a_good_scan_after_the_refusals(monkeypatch):
    db = MC.world()["db"]
    m = _marv(monkeypatch, 2, db.n, MC.TIE_MAX_SEQS)
    try:
        m.set_db(_load(m, db))
        for name in ("3di_L897", "other_matrix_without_min", "blosum62"):
            _check(m, name, "after the refusals")
    finally:
        m.close()


# ---- the asynchronous halves on several contexts, no harness -------------------------------------------------------------------------------------
def test_launch_on_three_contexts_then_finish_in_reverse_order():
    """three contexts on device 0 hold the three shards of the database (built here, not by the shim); all are launched before any is finished"""
    db = MC.world()["db"]
    n, N, max_res = db.n, 3, 40
    L = api.lib()
    shards = [MC.subset(db, range(k, n, N)) for k in range(N)]
    assert sum(s.n for s in shards) == n
    ctxs = [api.Context(0) for _ in range(N + 1)]
    try:
        for c, s in zip(ctxs, shards + [db]):
            c.load_db(s)
        rounds = [("3di_L300",) * 3] + [tuple("3di_L897" if k == r else "3di_L5" for k in range(N)) for r in range(N)]
        lists = {}
        for names in rounds:
            bufs = [np.zeros(max_res, api.HIT_DT) for _ in range(N)]
            for k in range(N):
                q = MC.cases()[names[k]]
                rc = L.fsgpu_gapless_launch(ctxs[k].h, q.pssm.ctypes.data_as(C.c_void_p), q.L, q.cap, -1, -1, max_res)
                assert rc == 0, (names, k, L.fsgpu_last_error(ctxs[k].h))
            for k in reversed(range(N)):
                nout = C.c_int(-1)
                rc = L.fsgpu_gapless_finish(ctxs[k].h, bufs[k].ctypes.data_as(C.c_void_p), C.byref(nout))
                assert rc == 0, (names, k, L.fsgpu_last_error(ctxs[k].h))
                want = gm.select(MC.scores(names[k])[k::N], -1, -1, max_res)
                got = bufs[k][:nout.value]
                assert nout.value == len(want) == min(max_res, shards[k].n), (names, k, nout.value)
                assert (got["id"] == want["id"]).all() and (got["score"] == want["score"]).all(), (names, k)
                assert (ctxs[k].gapless_scores().astype(np.int32) == MC.scores(names[k])[k::N]).all(), (names, k)
                glob = got.copy()
                glob["id"] = got["id"] * N + k
                lists.setdefault(names[k], {})[k] = glob
        for name, per in lists.items():
            assert sorted(per) == list(range(N)), name
            merged = np.concatenate([per[k] for k in range(N)])
            merged = merged[np.lexsort((merged["id"], -merged["score"].astype(np.int64)))][:max_res]
            q = MC.cases()[name]
            single = ctxs[N].gapless_scan(q.pssm, q.cap, min_score=-1, identity=-1, max_res=max_res)
            want = MC.expected(name, max_res)
            assert len(single) == len(want) and (single["id"] == want["id"]).all() and (single["score"] == want["score"]).all(), name
            assert merged.tobytes() == single.tobytes(), name
    finally:
        for c in ctxs:
            c.close()

"""The database entry -- fsgpu_db_load, fsgpu_db_adopt_device, fsgpu_db_broadcast (foldseek_amd/csrc/fsgpu_db.hip) -- held to its contract
(include/fsgpu.h): every table shape of tests/db_cases.py is loaded once and every reader of the resident database is compared with its independent model
on it; the tables the contract rules out are refused before anything is launched, by either entry, and leave the context without a database.

Per shape: the scan (fsgpu_gapless_scan, fsgpu_gapless_scan_multi: all n scores and the hit list) against tests/gapless_model.py; k_sw, k_sw2 and k_sw3
(fsgpu_sw_batch, fsgpu_sw_multi_dir, fsgpu_sw_multi_dir_c, fsgpu_sw_multi_c: both directions, both alignment types, every target id) against
tests/sw_model.py; fsgpu_diag_rescore on diagonals 0, +-1 (and the far ones of `longest`) against tests/diag_model.py; the k-mer index (masked bytes,
entries) and one search of two queries against the C oracle; fsgpu_block_backtrace on the shapes of D.BACKTRACE_NAMES against tests/ba_model.py.
Where an entry has no answer for a shape it refuses by name and the refusal is what is asserted: a backtrace task on a target without residues, the k-mer
index of a database without residues or with a target of 32768 residues or more (so the index never sees a 16th position bit, in either entry form), and
the entries that need AA data on a table without.  Nothing is skipped.

The refusal tables would make kernels read outside their buffers in a library without the check: they belong to this check and run nowhere else."""
import numpy as np
import pytest

import btrace_cases as B
import db_cases as D
import diag_model as dm
import gapless_model as gm
import history_cases as HC
import sw_cases as K
import sw_model as sm
from foldseek_amd import api

pytestmark = pytest.mark.gpu

MIN_SCORE, MAX_RES = 5, 10
E_ARG, E_NODB, E_UNSUPPORTED = "rc=-1", "rc=-3", "rc=-4"


@pytest.fixture(scope="module", autouse=True)
def torch_first():
    """torch asks for the device before the library opens it, whichever test of the file is selected (as bench.py does): the adopt tests hand torch
    tensors to the library"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- one context per shape ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loaded():
    """name -> context with that shape resident: loaded at first use, all closed when the module is done"""
    ctxs = {}

    def get(name):
        if name not in ctxs:
            ctxs[name] = api.Context(0)
            ctxs[name].load_db(D.shape(name).db)
        return ctxs[name]
    yield get
    for c in ctxs.values():
        c.close()


# ---- the comparisons, for any context that is to hold a shape ------------------------------------------------------------------------------------------
def check_bookkeeping(ctx, sh):
    assert ctx.n == sh.db.n and ctx.residues == int(sh.db.lengths.sum())


def check_scan(ctx, sh, what=""):
    n = sh.db.n
    idents = [-1, n - 1, 0, -1]
    single = []
    for L, ident in zip(D.scan_lengths(sh), idents):
        pssm, cap = D.scan_profile(L)
        want = D.scan_want(sh.name, L)
        assert len(want) == n
        hits = ctx.gapless_scan(pssm, cap, min_score=MIN_SCORE, identity=ident, max_res=MAX_RES)
        got = ctx.gapless_scores().astype(np.int32)
        assert (got == want).all(), (what, sh.name, "scan", L, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
        HC.same_hits(hits, gm.select(want, MIN_SCORE, ident, MAX_RES), (what, sh.name, "hits", L))
        single.append((pssm, cap, ident))
    hits = ctx.gapless_scan_multi(single, MIN_SCORE, MAX_RES)
    for k, (L, (pssm, cap, ident)) in enumerate(zip(D.scan_lengths(sh), single)):
        want = D.scan_want(sh.name, L)
        if L <= 896:
            got = ctx.gapless_scores_multi(k).astype(np.int32)
            assert (got == want).all(), (what, sh.name, "scan_multi", L, np.flatnonzero(got != want)[:8])
        HC.same_hits(hits[k], gm.select(want, MIN_SCORE, ident, MAX_RES), (what, sh.name, "hits_multi", L))


def _profiles(q, with_aa):
    m3, mA = K.matrices()
    p = [sm.profile(m, s, b, rev).astype(np.int16) for m, s, b, rev in ((mA, q.qa, q.cbAf, False), (m3, q.q3, q.cb3f, False), (mA, q.qa, q.cbAr, True), (m3, q.q3, q.cb3r, True))]
    return p if with_aa else [None, p[1], None, p[3]]


def check_sw(ctx, sh, what="", entries=("batch", "dir", "dir_c", "multi_c")):
    m3, mA = K.matrices()
    for with_aa in ((1, 0) if sh.db.dataaa is not None else (0,)):
        qs = [D.query(L) for L in D.sw_lengths(sh)]
        ids = [D.sw_ids(sh, L) for L in D.sw_lengths(sh)]
        want = [[D.sw_want(sh.name, L, rev, with_aa) for L in D.sw_lengths(sh)] for rev in (0, 1)]
        tag = (what, sh.name, "aa" if with_aa else "3di")
        if "batch" in entries:                                       # k_sw: one query per call
            for k, q in enumerate(qs):
                fwd, rev = ctx.sw_batch(*_profiles(q, with_aa), ids[k], gap_open=D.GO, gap_extend=D.GE)
                HC.sw_same(fwd, want[0][k], tag + ("sw_batch fwd", k))
                HC.sw_same(rev, want[1][k], tag + ("sw_batch rev", k))
        if "dir" in entries:                                         # k_sw2: both queries in one call, one direction per call
            for direction in (0, 1):
                got = ctx.sw_multi_dir([(*_profiles(q, with_aa), len(q.q3), t) for q, t in zip(qs, ids)], direction, gap_open=D.GO, gap_extend=D.GE)
                for k in range(len(qs)):
                    HC.sw_same(got[k], want[direction][k], tag + ("sw_multi_dir", direction, k))
        compact = [(q.qa if with_aa else None, q.q3, q.cbAf if with_aa else None, q.cb3f, q.cbAr if with_aa else None, q.cb3r, t) for q, t in zip(qs, ids)]
        if "dir_c" in entries:                                       # k_sw3, one direction per call
            for direction in (0, 1):
                got = ctx.sw_multi_dir_c(m3, mA if with_aa else None, compact, direction, gap_open=D.GO, gap_extend=D.GE)
                for k in range(len(qs)):
                    HC.sw_same(got[k], want[direction][k], tag + ("sw_multi_dir_c", direction, k))
        if "multi_c" in entries:                                     # k_sw3, both directions in one submission
            fwd, rev = ctx.sw_multi_c(m3, mA if with_aa else None, compact, gap_open=D.GO, gap_extend=D.GE)
            for k in range(len(qs)):
                HC.sw_same(fwd[k], want[0][k], tag + ("sw_multi_c fwd", k))
                HC.sw_same(rev[k], want[1][k], tag + ("sw_multi_c rev", k))


def check_diag(ctx, sh, what=""):
    m3, mA = (np.asarray(m, np.int16) for m in K.matrices())
    qs, pairs, want = D.diag_queries(sh), D.diag_pairs(sh), D.diag_want(sh.name)
    got = ctx.diag_rescore([q[0] for q in qs], [q[1] for q in qs], m3, mA, pairs)
    assert len(got) == len(pairs) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        w = dict(zip(dm.FIELDS, (int(x) for x in w)))
        skip = ("revScore",) if w["status"] == dm.UNDEFINED else ()
        bad = [f for f in dm.FIELDS if f not in skip and int(g[f]) != w[f]]
        assert not bad, (what, sh.name, "diag", pairs[k], bad, dict(zip(dm.FIELDS, g.tolist())), w)
    return want


def check_all(ctx, sh, what):
    check_bookkeeping(ctx, sh)
    check_scan(ctx, sh, what)
    if sh.db.dataaa is not None:
        check_sw(ctx, sh, what)
        check_diag(ctx, sh, what)


# ---- every shape through every reader ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.NAMES)
def test_scan(loaded, name):
    sh = D.shape(name)
    check_bookkeeping(loaded(name), sh)
    check_scan(loaded(name), sh)
    if name == "longest":                      # the planted copies saturate the score, the single residue and the short targets do not
        w = D.scan_want(name, 300)
        assert (w[np.asarray(sh.db.lengths) >= 32767] == D.scan_profile(300)[1]).all() and w.min() < D.scan_profile(300)[1]


def test_targets_without_residues_score_zero_whatever_the_context_scanned_before():
    """a stripe of eight targets without residues has no work item; the score buffers are kept from load to load and grow only: after a database whose
    every target scores, the empty targets of the next one must still read 0, in the single-query buffer and in the batch's slices"""
    before = D.shape("order_ascending")
    assert all((D.scan_want(before.name, L)[:11] > 0).all() for L in (17, 300))
    ctx = api.Context(0)
    try:
        ctx.load_db(before.db)
        check_scan(ctx, before, "before")
        for name in ("empty_stripe", "all_empty", "empty_entries"):
            ctx.load_db(D.shape(name).db)
            check_scan(ctx, D.shape(name), ("after order_ascending", name))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", [n for n in D.NAMES if n != "no_aa"])
def test_smith_waterman(loaded, name):
    sh = D.shape(name)
    check_sw(loaded(name), sh)
    if name == "longest":                      # what the shape is for: end cells behind column 32767 and on the final column, in both passes' range
        fwd = D.sw_want(name, 40, 0, 1)
        assert sorted(int(x) for x in fwd["dbEnd"] if x > 30000) == [32767, 32770, 65533]
        assert int(D.sw_want(name, 300, 0, 1)["dbEnd"].max()) == 65534 and int(D.sw_want(name, 300, 0, 0)["dbEnd"].max()) == 65534
    if name in ("empty_entries", "all_empty"):
        empty = np.flatnonzero(np.asarray(sh.db.lengths) == 0)
        assert all(tuple(int(x) for x in D.sw_want(name, 17, 0, 1)[i]) == (0, 0, 0, 1) for i in empty)


@pytest.mark.parametrize("name", [n for n in D.NAMES if n != "no_aa"])
def test_diagonal_rescoring(loaded, name):
    sh = D.shape(name)
    want = check_diag(loaded(name), sh)
    status = want[:, dm.FIELDS.index("status")]
    if name == "longest":
        pairs = D.diag_pairs(sh)
        far = [k for k, p in enumerate(pairs) if p[0] == 2 and abs(p[2]) in (32767, 32768, 65534)]
        assert len(far) == 6 and (status[far] == dm.OK).all() and (want[far, dm.FIELDS.index("diagonalLen")] > 0).all()
        assert want[[k for k, p in enumerate(pairs) if p == (2, D.long_id(sh, 0), 0)][0], dm.FIELDS.index("endPos")] > 32767
    if name == "all_empty":
        assert (status == dm.NO_OVERLAP).all()
    elif name != "longest":
        assert (status == dm.OK).sum() >= min(2, sh.db.n)


def _device_index(ctx, nbytes):
    """(k-mer ids in the reference's numbering, ascending; per k-mer its entries seqId << 16 | position; the masked copy) of the resident index"""
    off, ent, msk = ctx.kmer_index_copy(nbytes)
    off = off.astype(np.int64)
    dev = np.flatnonzero(np.diff(off))                      # device numbering: first 3-mer * 8000 + last 3-mer
    ref = dev // 8000 + 8000 * (dev % 8000)
    order = np.argsort(ref, kind="stable")
    return ref[order], [ent[off[dev[j]]:off[dev[j] + 1]] for j in order], msk


@pytest.mark.parametrize("name", D.NAMES)
def test_kmer_index_and_search(loaded, name):
    sh, ctx = D.shape(name), loaded(name)
    _, _, _, m8, _ = HC.kmer_matrices()
    if int(sh.db.lengths.sum()) == 0 or int(sh.db.lengths.max()) >= 32768:
        with pytest.raises(api.FsgpuError, match=E_UNSUPPORTED) as e:
            ctx.kmer_index_build(m8, kmer_thr=78)
        assert ("no residues" if name == "all_empty" else "32768 residues or more") in str(e.value)
        assert ctx.kmer_index_entry_bytes == 0 and ctx.kmer_index_entries == 0
        with pytest.raises(api.FsgpuError, match=E_NODB):
            ctx.kmer_search([api.kmer_query_prepare(m8, HC.kmer_matrices()[4], D.query(17).q3)])
        return
    targets = [D.kmer_bytes(D.entry(sh.db, i)) for i in range(sh.db.n)]
    o = HC.kmer_oracle(targets)
    try:
        ctx.kmer_index_build(m8, kmer_thr=78)
        assert ctx.kmer_index_entry_bytes == 4
        nbytes = int(sh.db.data3di.size)
        kmers, lists, msk = _device_index(ctx, nbytes)
        for i, t in enumerate(targets):
            got = msk[int(sh.db.offsets[i]):int(sh.db.offsets[i]) + len(t)]
            assert (got == o.masked(i, len(t))).all(), (name, "masked", i)
        ooff, oseq, opos = o.index()
        ooff = ooff.astype(np.int64)
        okm = np.flatnonzero(np.diff(ooff))
        assert ctx.kmer_index_entries == int(ooff[-1]) and len(kmers) == len(okm) and (kmers == okm).all(), (name, len(kmers), len(okm))
        want = (oseq.astype(np.uint64) << np.uint64(16)) | opos.astype(np.uint64)
        got = np.concatenate(lists) if lists else np.zeros(0, np.uint64)
        assert len(got) == len(want) and (got == want).all(), (name, "entries")
        ident = min(sh.db.n - 1, 3)
        s = HC.KmerSet(o, [D.query(300).q3, D.query(17).q3], 78, idents=[-1, ident])
        s.check(ctx, (name, "search"), 100)
        if name.startswith(("bytes_", "order_ties", "counts17")):            # not an empty comparison
            assert len(want) > 0 and sum(len(b) for b, _ in s.want) > 0, name
    finally:
        o.close()


def _backtrace_world(sh):
    """queries and tasks of one fsgpu_block_backtrace call: every pair whose forward Smith-Waterman record (both matrices) scores, ending in that record's
    end cell, with what ba_model answers for the two prefixes"""
    qs = [D.query(L) for L in D.sw_lengths(sh)]
    queries = [(q.qa, q.q3, q.cbAf, q.cb3f) for q in qs]
    tasks, cases = [], []
    for k, (L, q) in enumerate(zip(D.sw_lengths(sh), qs)):
        bias = q.cbAf.astype(np.int64) + q.cb3f.astype(np.int64)
        for r, i in zip(D.sw_want(sh.name, L, 0, 1), D.sw_ids(sh, L)):
            if r["score"] <= 0:
                continue
            t3, ta = D.aligner_target(sh.db, int(i))
            qe, de = int(r["qEnd"]), int(r["dbEnd"])
            cases.append(B.model_case(f"{sh.name}_{L}_{i}", q.qa[:qe + 1], q.q3[:qe + 1], bias[:qe + 1], ta[:de + 1], t3[:de + 1], int(r["score"])))
            tasks.append((k, int(i), qe, de, int(r["score"])))
    return queries, tasks, cases


@pytest.mark.parametrize("name", D.BACKTRACE_NAMES)
def test_block_backtrace(loaded, name):
    sh, ctx = D.shape(name), loaded(name)
    queries, tasks, cases = _backtrace_world(sh)
    got = ctx.block_backtrace(*B.device_tables(), queries, tasks, D.GO, D.GE)
    seen = {"A": 0, "B": 0, "C": 0}
    for r, c, t in zip(got, cases, tasks):
        want = c.expected(t[2], t[3])
        if c.cls != "A":                       # needs a block of more than 128 rows: handed back by the first pass (status 0), the caller's host path answers
            want = dict(status=0, qStart=-1, dbStart=-1, identicalAA=0, backtrace="")
        assert {x: r[x] for x in want} == want, (name, c.name, t, r, want)
        assert c.cls != "A" or r["blockSizes"] == c.attempts, (name, c.name, r["blockSizes"], c.attempts)
        seen[c.cls] += 1
    assert seen["A"] >= 5, seen
    if name == "longest":
        assert seen["B"] + seen["C"] >= 1 and max(t[3] for t, c in zip(tasks, cases) if c.cls == "A") == 65534, seen
    empty = np.flatnonzero(np.asarray(sh.db.lengths) == 0)
    if len(empty):                              # a target without residues has no end cell: the task is refused by name, nothing is launched
        with pytest.raises(api.FsgpuError, match=E_ARG) as e:
            ctx.block_backtrace(*B.device_tables(), queries, tasks[:2] + [(0, int(empty[0]), 0, 0, 1)], D.GO, D.GE)
        assert "task 2" in str(e.value) and "without residues" in str(e.value)


def test_order_of_the_table_does_not_change_an_answer(loaded):
    """the same residues in five tables (by length: ascending, all equal, descending, strictly descending, random with runs of ties) and in three byte
    layouts: the device's own scores, entry by entry of the pool, are equal across them -- over and above each being equal to the model's"""
    for group in (("order_ascending", "order_equal", "order_descending", "order_strict", "order_ties"), ("bytes_odd", "bytes_gaps", "bytes_descending")):
        by_entry = {}
        for name in group:
            sh, ctx = D.shape(name), loaded(name)
            pssm, cap = D.scan_profile(300)
            ctx.gapless_scan(pssm, cap, min_score=MIN_SCORE, max_res=MAX_RES)
            scan = ctx.gapless_scores()
            q = D.query(300)
            fwd, rev = ctx.sw_batch(*_profiles(q, 1), np.arange(sh.db.n, dtype=np.uint32), gap_open=D.GO, gap_extend=D.GE)
            for i, p in enumerate(sh.pool):
                rec = (int(scan[i]), tuple(int(fwd[i][f]) for f in HC.SW_FIELDS), tuple(int(rev[i][f]) for f in HC.SW_FIELDS))
                assert by_entry.setdefault(p, rec) == rec, (name, i, p)
        assert len(by_entry) == len(D.shape(group[0]).pool)


def test_entries_that_need_aa_say_so_on_a_table_without(loaded):
    sh, ctx = D.shape("no_aa"), loaded("no_aa")
    q = D.query(17)
    m3, mA = K.matrices()
    ids = np.arange(sh.db.n, dtype=np.uint32)
    with pytest.raises(api.FsgpuError, match=E_NODB + ".*without AA sequences"):
        ctx.sw_batch(*_profiles(q, 1), ids)
    with pytest.raises(api.FsgpuError, match=E_NODB + ".*without AA sequences"):
        ctx.sw_multi_dir([(*_profiles(q, 1), 17, ids)], 0)
    with pytest.raises(api.FsgpuError, match=E_NODB + ".*without AA sequences"):
        ctx.sw_multi_dir_c(m3, mA, [(q.qa, q.q3, q.cbAf, q.cb3f, q.cbAr, q.cb3r, ids)], 0)
    with pytest.raises(api.FsgpuError, match=E_NODB + ".*needs the AA half"):
        ctx.diag_rescore([q.qa], [q.q3], m3.astype(np.int16), mA.astype(np.int16), [(0, 0, 0)])
    with pytest.raises(api.FsgpuError, match=E_NODB + ".*without AA sequences"):
        ctx.block_backtrace(*B.device_tables(), [(q.qa, q.q3, q.cbAf, q.cb3f)], [(0, 1, 0, 0, 1)])
    check_sw(ctx, sh, "after the refusals")                     # 3Di only: answered
    check_scan(ctx, sh, "after the refusals")


# ---- the load paths ---------------------------------------------------------------------------------------------------------------------------------
def _device_tensors(db):
    """the four buffers of a table as torch tensors on the device (offsets as the int64 image of the uint64 values), complete when this returns"""
    import torch
    dev = torch.device("cuda", 0)
    arrays = [np.ascontiguousarray(db.data3di, np.uint8), None if db.dataaa is None else np.ascontiguousarray(db.dataaa, np.uint8),
              np.ascontiguousarray(db.offsets, np.uint64).view(np.int64), np.ascontiguousarray(db.lengths, np.int32)]
    tensors = [None if a is None else torch.from_numpy(a.copy()).to(dev) for a in arrays]
    torch.cuda.synchronize()
    return tensors


def _adopt(ctx, db):
    """fsgpu_db_adopt_device as bench.py calls it; the moment it returns the caller's buffers are overwritten with 0xff and released"""
    import torch
    t = _device_tensors(db)
    try:
        ctx.adopt_device_db(t[0].data_ptr(), None if t[1] is None else t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), len(db.lengths), int(np.asarray(db.data3di).size))
    finally:
        for x in t:
            if x is not None:
                x.fill_(255 if x.dtype == torch.uint8 else -1)
        torch.cuda.synchronize()
        del t


@pytest.mark.parametrize("name", ["codes", "order_ties", "bytes_gaps"])
def test_adopted_device_buffers_are_not_needed_after_the_call(name):
    sh = D.shape(name)
    ctx = api.Context(0)
    try:
        _adopt(ctx, sh.db)
        check_all(ctx, sh, "adopted")
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["codes", "order_ties", "all_empty"])
def test_broadcast_on_one_device(loaded, name):
    """the peer-copy branch of fsgpu_db_broadcast into a second context on the same device: the destination answers like the source, and the source goes on
    answering when the destination is gone"""
    sh, src = D.shape(name), loaded(name)
    dst = api.Context(0)
    try:
        assert src.broadcast_db_to([dst]) is False
        check_all(dst, sh, "broadcast destination")
    finally:
        dst.close()
    check_all(src, sh, "broadcast source")


def test_clone_keeps_the_table_it_was_made_on():
    old, new = D.shape("codes"), D.shape("order_ties")
    ctx = api.Context(0)
    clone = None
    try:
        ctx.load_db(old.db)
        clone = ctx.clone()
        ctx.load_db(new.db)
        check_all(clone, old, "clone made before the reload")
        check_all(ctx, new, "reloaded source")
        check_all(clone, old, "clone, again")
    finally:
        if clone is not None:
            clone.close()
        ctx.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def _refused_then_good(ctx, r, load):
    """a good database, the refused call, E_NODB from the scan, a good load, one scan comparison"""
    good = D.shape("counts17")
    ctx.load_db(good.db)
    pssm, cap = D.scan_profile(17)
    with pytest.raises(api.FsgpuError, match=E_ARG) as e:
        load(ctx, r.db)
    if r.index is not None:
        assert f"entry {r.index} " in str(e.value), str(e.value)
    assert ctx.n == 0
    with pytest.raises(api.FsgpuError, match=E_NODB):
        ctx.gapless_scan(pssm, cap)
    with pytest.raises(api.FsgpuError, match=E_NODB):
        ctx.gapless_scan_multi([(pssm, cap, -1)])
    ctx.load_db(good.db)
    check_scan(ctx, good, ("after", r.name))


@pytest.fixture(scope="module")
def scratch_ctx():
    ctx = api.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("r", D.refusals(), ids=lambda r: r.name)
def test_load_refuses_a_bad_table(scratch_ctx, r):
    _refused_then_good(scratch_ctx, r, lambda ctx, db: ctx.load_db(db))


@pytest.mark.parametrize("r", D.refusals(), ids=lambda r: r.name)
def test_adopt_refuses_a_bad_table(scratch_ctx, r):
    _refused_then_good(scratch_ctx, r, _adopt)


def test_refusal_messages_say_why(scratch_ctx):
    why = {"offset_past_bytes": "outside the data buffer", "last_residue_past_bytes_by_one": "outside the data buffer", "offset_wraps": "outside the data buffer",
           "end_past_bytes": "end of the table", "negative_length": "length outside", "longer_than_max": "length outside", "no_entries": "bad argument",
           "overlap_by_one": "shares bytes", "overlap_same_start": "shares bytes", "overlap_descending": "shares bytes"}
    for r in D.refusals():
        if r.name in why:
            with pytest.raises(api.FsgpuError, match=why[r.name]):
                scratch_ctx.load_db(r.db)

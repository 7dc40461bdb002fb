"""tests/history_cases.py -- the seeded inputs that tests/test_call_history_gpu.py and tests/test_clones_gpu.py share, with the answers of the
existing models for them (TEST INFRASTRUCTURE: of the project only synth, a plain generator, and the host-side profile builders are used).

Everything here is built once per process (lru_cache) and never changed by a test: the three scan databases of 600, 9 000 and 5 targets with the
batched-scan queries and gapless_model's score vectors, the k-mer worlds with the C oracle, the row-tiled SW calls with sw_model's records, sixteen
frozen block-aligner cases next to sw_cases' main database in one database, the scan sets of four clones, and the LDDT structures."""
import functools

import numpy as np

import btrace_cases as B
import gapless_model as gm
import helpers as H
import kmer_lib as KL
import lddt_cases as LC
import lddt_model as LM
import sw_cases as K
import sw_model as sm
from foldseek_amd import api, synth

SW_FIELDS = ("score", "qEnd", "dbEnd", "word")


def db_from(seqs3, keep_order=False):
    """PaddedDB of 3Di code strings in ascending length, or in the order given (no AA: prefilter only)"""
    seqs3 = list(seqs3) if keep_order else sorted(seqs3, key=len)
    lens = np.array([len(x) for x in seqs3], np.int32)
    offsets = np.zeros(len(lens) + 1, np.int64)
    offsets[1:] = np.cumsum((lens.astype(np.int64) + 3) // 4 * 4)
    d3 = np.full(int(offsets[-1]), 20, np.uint8)
    for k, s in enumerate(seqs3):
        d3[offsets[k]:offsets[k] + lens[k]] = s
    return synth.PaddedDB(d3, None, offsets, lens)


def same_hits(hits, want, what=None):
    assert len(hits) == len(want), (what, len(hits), len(want))
    assert (hits["id"] == want["id"]).all() and (hits["score"] == want["score"]).all(), what


# ---- the scan databases and their queries ---------------------------------------------------------------------------------------------------------
# lengths of the batched-scan queries: class 1 (a pair), class 3 (a pair and an odd one out), class 9 alone, class 16 (the last paired class, a pair),
# class 19 (unpaired kernels), and the row-tiled 897
SCAN_LENGTHS = (9, 16, 40, 45, 37, 130, 250, 256, 300, 897)
SCAN_SIZES = (600, 9000, 5)


@functools.lru_cache(maxsize=None)
def scan_queries():
    """[(3Di codes, pssm int8 [21, L], cap)]"""
    rng = np.random.default_rng(20261019)
    m = api.Matrix(0, 2.0)
    out = []
    for L in SCAN_LENGTHS:
        q = rng.choice(20, size=L).astype(np.uint8)
        pssm, cap = api.prefilter_profile(m, q, True, 0.15)
        out.append((q, pssm, cap))
    return out


class ScanWorld:
    """one database, the model's score vector of every scan query on it, and k-mer queries with the oracle's hit lists"""

    def __init__(self, n):
        rng = np.random.default_rng(1000 + n)
        qs = [q for q, _, _ in scan_queries()]
        seqs = []
        if n >= 100:
            # short background targets keep the model's loop short; one mutated copy of every query, one target of a single residue, one stripe that
            # is far longer than the others (the planner cuts it into column segments)
            for q in qs:
                s = q.copy()
                hit = rng.random(len(s)) < 0.2
                s[hit] = rng.integers(0, 20, int(hit.sum()))
                seqs.append(s)
            seqs += [np.array([7], np.uint8), np.concatenate([qs[-1], rng.choice(20, size=60).astype(np.uint8), qs[-2]])]
            while len(seqs) < n:
                T = int(rng.integers(2, 41))
                s = rng.integers(0, 21, T).astype(np.uint8)
                if len(seqs) % 3 == 0:                                   # a piece of a query: scores spread over the range
                    q = qs[int(rng.integers(2, len(qs)))]
                    a = int(rng.integers(0, len(q) - min(T, len(q)) + 1))
                    s = np.where(rng.random(min(T, len(q))) < 0.15, rng.integers(0, 20, min(T, len(q))), q[a:a + T]).astype(np.uint8)
                if len(seqs) % 50 == 0:
                    s = s + (32 * (rng.random(len(s)) < 0.3)).astype(np.uint8)          # soft-masked residues
                seqs.append(s)
        else:
            seqs = [qs[2].copy(), np.array([3], np.uint8), qs[5][10:75].copy(), rng.integers(0, 20, 12).astype(np.uint8), qs[-1][100:400].copy()][:n]
        self.db = db_from(seqs)
        assert self.db.n == n
        self.packed = gm.pack(self.db)
        self.want = [gm.scores(pssm, cap, self.packed) for _, pssm, cap in scan_queries()]
        self.targets = [self.db.seq(i, "3di", unmask=False) for i in range(n)]

    def check_batch(self, ctx, order, idents, min_score, max_res, what):
        """one gapless_scan_multi call over the queries `order` (indices into scan_queries()): every slice and hit list against the model"""
        qs = scan_queries()
        hits = ctx.gapless_scan_multi([(qs[i][1], qs[i][2], ident) for i, ident in zip(order, idents)], min_score, max_res)
        assert len(hits) == len(order)
        for k, (i, ident) in enumerate(zip(order, idents)):
            if qs[i][1].shape[1] <= 896:
                got = ctx.gapless_scores_multi(k).astype(np.int32)
                assert (got == self.want[i]).all(), (what, "scores", k, i, np.flatnonzero(got != self.want[i])[:10])
            same_hits(hits[k], gm.select(self.want[i], min_score, ident, max_res), (what, "hits", k, i))

    def check_single(self, ctx, i, min_score, max_res, what, identity=-1):
        _, pssm, cap = scan_queries()[i]
        hits = ctx.gapless_scan(pssm, cap, min_score=min_score, identity=identity, max_res=max_res)
        got = ctx.gapless_scores().astype(np.int32)
        assert (got == self.want[i]).all(), (what, "scores", i, np.flatnonzero(got != self.want[i])[:10])
        same_hits(hits, gm.select(self.want[i], min_score, identity, max_res), (what, "hits", i))


@functools.lru_cache(maxsize=None)
def scan_world(n):
    return ScanWorld(n)


# ---- k-mer prefilter: queries, the oracle's answers --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kmer_matrices():
    """(oracle k-mer matrix, background, oracle ungapped matrix, device k-mer Matrix, device ungapped Matrix)"""
    ksub, pb = H.o_submat("MAT3DI", 8.0, -0.2)
    usub, _ = H.o_submat("MAT3DI", 2.0, -0.2)
    m8, m2 = api.Matrix(0, 8.0, -0.2), api.Matrix(0, 2.0, -0.2)
    assert (m8.scores().ravel() == ksub).all() and (m2.scores().ravel() == usub).all()
    return ksub, pb, usub, m8, m2


class KmerSet:
    """queries prepared for one per-position threshold and the oracle's (hit list, statistics) for them.  The oracle is built with the threshold the
    index is built with; the threshold of the QUERIES (the per-position array a device query carries) is set on the oracle before it answers, which
    its query path reads and its index, built before, does not."""

    def __init__(self, oracle, queries, query_thr, idents=None, comp_bias=True, repeat=1):
        """repeat: the queries (and their answers, computed once) that many times over in one call"""
        _, _, _, m8, m2 = kmer_matrices()
        self.thr = query_thr
        idents = [-1] * len(queries) if idents is None else list(idents)
        prep = [api.kmer_query_prepare(m8, m2, q, comp_bias=comp_bias, kmer_thr=query_thr) for q in queries]
        oracle.set(kmerThr=query_thr, compBias=int(comp_bias))
        want = [oracle.query(q, int(i)) for q, i in zip(queries, idents)]
        self.queries, self.idents, self.prep, self.want = list(queries) * repeat, idents * repeat, prep * repeat, want * repeat
        self.positions = sum(len(p[1]) for p in self.prep)
        self.index_hits = sum(st[1] for _, st in self.want)          # the oracle's dbMatches

    def check(self, ctx, what, max_res):
        res, status, stats = ctx.kmer_search(self.prep, identity=self.idents, max_res=max_res, l2_cache_size=2 << 20, want_stats=True)
        for i in range(len(self.queries)):
            b, st = self.want[i]
            assert status[i] == 0 and np.allclose(stats[i], st), (what, i, stats[i], st)
            assert len(res[i]) == len(b) and (res[i] == b).all(), (what, i, len(res[i]), len(b))
        return res


def kmer_oracle(targets, index_thr=78, max_res=100):
    ksub, pb, usub, _, _ = kmer_matrices()
    return KL.OraKpf(KL.load_ora(), ksub, pb, usub, targets, kmerThr=index_thr, maxResListLen=max_res)


@functools.lru_cache(maxsize=None)
def kmer_world():
    """the 400-target database of test_kmer_gpu.py's form tests and three query sets on ONE index (threshold 78): `dense` at the index's own threshold
    (thousands of similar k-mers per position), `sparse` at 130 (a handful), and `many`: 70 sparse queries with identity ids"""
    q3, qa = synth.make_queries(4, seed=77, mean_len=60, lo=40, hi=80)
    db = synth.make_db(400, (q3, qa), seed=78, homologs_per_query=10, mean_len=120, lo=30, hi=300)
    targets = [db.seq(i, "3di", unmask=False) for i in range(db.n)]
    o = kmer_oracle(targets)
    dense = KmerSet(o, list(q3), 78)
    sparse = KmerSet(o, list(q3) + [q3[0][:7], q3[1][3:9]], 130)
    many_q = [db.seq(i)[: 30 + i % 40] for i in range(0, 350, 5)]
    many = KmerSet(o, many_q, 130, idents=[(i * 5 if i % 3 == 0 else -1) for i in range(len(many_q))])
    o.close()
    assert len(many_q) == 70
    return dict(db=db, dense=dense, sparse=sparse, many=many)


@functools.lru_cache(maxsize=None)
def scan_kmer_set(n, query_thr=78, index_thr=78):
    """the short scan queries as k-mer queries on scan database n"""
    w = scan_world(n)
    o = kmer_oracle(w.targets, index_thr)
    qs = [q for q, _, _ in scan_queries()][2:8]
    s = KmerSet(o, qs, query_thr, idents=[-1, 0, -1, -1, min(3, n - 1), -1])
    o.close()
    return s


# ---- row-tiled Smith-Waterman across gap costs and databases ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def second_main_db():
    """sw_cases' main database with the entries of every length rotated by one: same size, same length at every id, other residues"""
    db = K.main_db()
    entries = [(db.data3di[int(db.offsets[i]):int(db.offsets[i]) + int(db.lengths[i])].copy(),
                db.dataaa[int(db.offsets[i]):int(db.offsets[i]) + int(db.lengths[i])].copy(), db.kind[i]) for i in range(db.n)]
    out = list(entries)
    for L in np.unique(db.lengths):
        ids = np.flatnonzero(db.lengths == L)
        for k, i in enumerate(ids):
            out[i] = entries[ids[(k + 1) % len(ids)]]
    db2 = K.pack(out)
    assert db2.n == db.n and (db2.lengths == db.lengths).all()
    return db2


@functools.lru_cache(maxsize=None)
def sw_history():
    """(queries [1025 rows, 64 rows], target ids per query): a 1-column target, one of 65 columns, one of 129 and five more, all at ids whose entry
    differs between the two databases"""
    db, db2 = K.main_db(), second_main_db()
    qs = [K.make_query(1025, 8000 + 1025, "related"), K.make_query(64, 8000 + 64, "related")]
    ids = [K.first_of_length(db, L, kind) for L, kind in ((1, "random"), (65, "derived"), (129, "derived"), (17, "random"), (33, "derived"), (64, "low"), (100, "derived"),
                                                          (130, "derived"))]
    for i in ids:
        assert K.target(db, i)[0].tobytes() != K.target(db2, i)[0].tobytes() or db.lengths[i] == 1, i
    return qs, [np.array(ids, np.uint32), np.array(ids[:5], np.uint32)]


@functools.lru_cache(maxsize=None)
def sw_want(which_db, go, ge, direction):
    """sw_model's records per query of sw_history() against one of the two databases"""
    db = K.main_db() if which_db == 0 else second_main_db()
    m3, mA = K.matrices()
    qs, ids = sw_history()
    return [K.live(m3, mA, q, bool(direction), [K.target(db, int(i)) for i in t], go, ge) for q, t in zip(qs, ids)]


def sw_profiles(q):
    """(pAA fwd, p3Di fwd, pAA rev, p3Di rev) int16 [21, L] of a sw_cases query"""
    m3, mA = K.matrices()
    return [sm.profile(m, s, b, rev).astype(np.int16) for m, s, b, rev in ((mA, q.qa, q.cbAf, False), (m3, q.q3, q.cb3f, False), (mA, q.qa, q.cbAr, True), (m3, q.q3, q.cb3r, True))]


def sw_same(got, want, what):
    bad = [k for k in range(len(want)) if any(int(got[k][f]) != int(want[k][f]) for f in SW_FIELDS)]
    assert len(got) == len(want) and not bad, (what, [(k, "device", tuple(int(got[k][f]) for f in SW_FIELDS), "model", tuple(int(want[k][f]) for f in SW_FIELDS)) for k in bad[:6]])


# ---- one database for Smith-Waterman, the scan and the block aligner ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def combo():
    """sw_cases' main database plus the targets of sixteen frozen block-aligner cases (class A, gap costs 10 / 1, the answers of ba_model as
    btrace_cases holds them), packed the way sw_cases packs: dict(db, main_ids: id in main_db -> id here, queries / tasks / cases / ends of the
    block-aligner call).  Residues and bias values lie behind every end cell, soft-masked residues inside the targets, as in test_btrace_model_gpu.py."""
    rng = np.random.default_rng(20261020)
    main = K.main_db()
    entries = [(main.data3di[int(main.offsets[i]):int(main.offsets[i]) + int(main.lengths[i])].copy(),
                main.dataaa[int(main.offsets[i]):int(main.offsets[i]) + int(main.lengths[i])].copy(), main.kind[i]) for i in range(main.n)]
    cases = [c for c in B.short_cases() if (c.go, c.ge) == (10, 1) and c.cls == "A"][:16]
    assert len(cases) == 16
    queries, ends = [], []
    for c in cases:
        codes = lambda s: np.array([B.CODE[ch] for ch in s[::-1]], np.uint8)  # noqa: E731
        qa, q3, ta, t3 = codes(c.rqa), codes(c.rq3), codes(c.rta), codes(c.rt3)
        bias = np.array(c.rbias[::-1], np.int64)
        nq, nt = int(rng.integers(0, 21)), int(rng.integers(0, 21))
        qa, q3 = np.concatenate([qa, rng.integers(0, 21, nq).astype(np.uint8)]), np.concatenate([q3, rng.integers(0, 21, nq).astype(np.uint8)])
        ta, t3 = np.concatenate([ta, rng.integers(0, 21, nt).astype(np.uint8)]), np.concatenate([t3, rng.integers(0, 21, nt).astype(np.uint8)])
        bias = np.concatenate([bias, rng.integers(-30, 31, nq)])
        lo, hi = np.maximum(-128, bias - 127), np.minimum(127, bias + 128)
        cbA = np.clip(rng.integers(-100, 101, len(bias)), lo, hi)
        cbS = bias - cbA
        assert (cbS >= -128).all() and (cbS <= 127).all()
        queries.append((qa, q3, cbA.astype(np.int8), cbS.astype(np.int8)))
        for s in (ta, t3):
            s[rng.integers(0, len(s), size=1 + len(s) // 25)] += 32
        entries.append((t3, ta, "bt"))
        ends.append((len(c.rqa) - 1, len(c.rta) - 1))
    order = sorted(range(len(entries)), key=lambda k: len(entries[k][0]))          # the order sw_cases.pack gives them
    new_id = np.zeros(len(entries), np.int64)
    new_id[order] = np.arange(len(entries))
    db = K.pack(entries)
    for i in range(main.n):
        assert K.target(db, int(new_id[i]))[0].tobytes() == K.target(main, i)[0].tobytes()
    tasks = [(k, int(new_id[main.n + k]), ends[k][0], ends[k][1], c.target) for k, c in enumerate(cases)]
    return dict(db=db, main_ids=new_id[:main.n], queries=queries, tasks=tasks, cases=cases, ends=ends, tables=B.device_tables())


def btrace_run(ctx):
    w = combo()
    return ctx.block_backtrace(*w["tables"], w["queries"], w["tasks"], 10, 1)


def btrace_check(got, what):
    w = combo()
    assert len(got) == len(w["cases"])
    for r, c, e in zip(got, w["cases"], w["ends"]):
        want = c.expected(*e)
        assert {x: r[x] for x in want} == want, (what, c.name, r, want)
        assert r["blockSizes"] == c.attempts, (what, c.name, r["blockSizes"], c.attempts)


def on_combo(ids):
    """target ids of sw_cases' main database -> the same entries' ids in combo()"""
    return combo()["main_ids"][np.asarray(ids, np.int64)].astype(np.uint32)


# ---- LDDT ------------------------------------------------------------------------------------------------------------------------------------------------
def walk(rng, L, step=3.8):
    v = rng.normal(size=(L, 3))
    v = v / np.linalg.norm(v, axis=1)[:, None] * step
    return np.ascontiguousarray(np.cumsum(v, axis=0).T, np.float32)


@functools.lru_cache(maxsize=None)
def lddt_world():
    """queries A and B of one length, C longer, `big` with more residues than the norm buffer's first allocation holds (4 KiB: 1024 norms); targets are perturbed copies; task lists as
    (query, target, qStart, dbStart, backtrace) with the model's columns"""
    rng = np.random.default_rng(20261021)
    A, Bq, Cq, big = walk(rng, 90), walk(rng, 90), walk(rng, 140), walk(rng, 1100)
    targets = []
    for src in (A, A, Bq, Cq, big):
        t = src + rng.normal(scale=1.2, size=src.shape).astype(np.float32)
        targets.append(np.ascontiguousarray(np.concatenate([t, walk(rng, 6)], axis=1), np.float32))
    bt1 = "M" * 30 + "DD" + "M" * 40
    bt2 = "II" + "M" * 64 + "D" + "M" * 10
    bt3 = "M" * 90
    return dict(A=A, B=Bq, C=Cq, big=big, targets=targets, bts=(bt1, bt2, bt3))


def lddt_want(queries, targets, tasks):
    return [LM.columns(queries[q], targets[t], qs, ts, bt) for q, t, qs, ts, bt in tasks]


def lddt_check(got, want, what):
    assert len(got) == len(want)
    for k, ((n, cols), w) in enumerate(zip(got, want)):
        assert n == len(w), (what, k, n, len(w))
        assert LC.same_bits(cols, w), (what, k)


# ---- the scan on combo() ---------------------------------------------------------------------------------------------------------------------------------
COMBO_SCAN = (1, 3, 5)          # scan_queries() run against combo(): 16, 45 and 130 residues


@functools.lru_cache(maxsize=None)
def combo_scan_want():
    packed = gm.pack(combo()["db"])
    return {i: gm.scores(scan_queries()[i][1], scan_queries()[i][2], packed) for i in COMBO_SCAN}


def combo_scan_check(ctx, what, order=COMBO_SCAN, min_score=15, max_res=40):
    qs, want = scan_queries(), combo_scan_want()
    hits = ctx.gapless_scan_multi([(qs[i][1], qs[i][2], -1) for i in order], min_score, max_res)
    for k, i in enumerate(order):
        got = ctx.gapless_scores_multi(k).astype(np.int32)
        assert (got == want[i]).all(), (what, "scores", i, np.flatnonzero(got != want[i])[:10])
        same_hits(hits[k], gm.select(want[i], min_score, -1, max_res), (what, "hits", i))


# ---- compact Smith-Waterman on combo(): sw_cases' image-reuse queries with their short lists --------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compact_call():
    """(the call as sw_cases states it, on main_db ids; the same call with combo()'s ids for the device)"""
    c = K.section_d()["short"]
    return c, c._replace(ids=[on_combo(x) for x in c.ids])


@functools.lru_cache(maxsize=None)
def compact_want(direction):
    """forward: sw_cases' frozen records; reversed: the same model, live (these lists are frozen for the forward direction only)"""
    c, _ = compact_call()
    if direction == 0:
        return K.call_want(c, 0)
    db = K.main_db()
    return [K.live(c.m3, c.mA, q, True, [K.target(db, int(i)) for i in ids], c.go, c.ge) for q, ids in zip(c.queries, c.ids)]


def compact_run(ctx, direction, what):
    """one direction through sw_multi_dir_c against the model; returns the plan.  The caller has set sw_cases.ENV_32."""
    c, dev = compact_call()
    got = ctx.sw_multi_dir_c(c.m3, c.mA, K.api_queries(dev), direction, gap_open=c.go, gap_extend=c.ge)
    plan = ctx.sw3_last_plan()
    for i, w in enumerate(compact_want(direction)):
        sw_same(got[i], w, (what, "compact", direction, i))
    return plan


def history_run(ctx, entry, direction, go, ge, ids_of=lambda x: x):
    """sw_history() in one direction through fsgpu_sw_multi_dir ("profiles") or fsgpu_sw_multi_dir_c ("compact")"""
    qs, ids = sw_history()
    ids = [np.asarray(ids_of(t), np.uint32) for t in ids]
    m3, mA = K.matrices()
    if entry == "profiles":
        return ctx.sw_multi_dir([(*sw_profiles(q), len(q.q3), t) for q, t in zip(qs, ids)], direction, gap_open=go, gap_extend=ge)
    return ctx.sw_multi_dir_c(m3, mA, [(q.qa, q.q3, q.cbAf, q.cb3f, q.cbAr, q.cb3r, t) for q, t in zip(qs, ids)], direction, gap_open=go, gap_extend=ge)


# ---- k-mer sets on combo() and on a rebuilt index -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def combo_kmer_set():
    """two members of combo() (65 and 257 residues, relatives of sw_cases' master sequence) as k-mer queries on it"""
    db, main = combo()["db"], K.main_db()
    o = kmer_oracle([db.seq(i, "3di", unmask=False) for i in range(db.n)])
    qs = [K.target(main, K.first_of_length(main, L, "derived"))[0] for L in (65, 257)]
    s = KmerSet(o, qs, 78, idents=[-1, int(on_combo([K.first_of_length(main, 257, "derived")])[0])])
    o.close()
    assert sum(len(b) for b, _ in s.want) > 0
    return s


# ---- a k-mer query heavy enough to change how the next call is cut ---------------------------------------------------------------------------------------
HEAVY_TARGETS = 10000


@functools.lru_cache(maxsize=None)
def heavy_kmer_world():
    """An index list holds one entry per (k-mer, target), so the index hits of a query are its positions times the targets that hold its k-mers --
    whatever the targets' lengths.  kmer_world()'s 400 targets, 20 targets of eleven residues of a two-letter repeat (both of its k-mers: double
    hits on every second diagonal, these are the heavy queries' results) and 10 000 of ten residues of the repeat and an X (one k-mer, the one whose
    self score passes threshold 130; no double hit).  `heavy`: one query of 24 000 residues of the repeat, without composition bias (the bias would
    lift the threshold out of reach of a low-complexity query): 12 000 positions x 10 020 targets = 1.2e8 index hits.  `heaviest`: three queries
    of 32 767 residues in one call, 1.64e8 hits each.  `many`: kmer_world()'s 70 sparse queries, answered on this database."""
    w = kmer_world()
    unit = np.array([3, 17], np.uint8)
    targets = [w["db"].seq(i, "3di", unmask=False) for i in range(w["db"].n)]
    targets += [np.resize(unit, 11) for _ in range(20)]
    targets += [np.concatenate([np.resize(unit[::-1], 10), np.array([20], np.uint8)]) for _ in range(HEAVY_TARGETS)]
    db = db_from(targets, keep_order=True)
    o = kmer_oracle(targets)
    heavy = KmerSet(o, [np.resize(unit, 24000)], 130, comp_bias=False)
    heaviest = KmerSet(o, [np.resize(unit, 32767)], 130, comp_bias=False, repeat=3)
    many = KmerSet(o, w["many"].queries, 130, idents=w["many"].idents)
    o.close()
    return dict(db=db, heavy=heavy, heaviest=heaviest, many=many)


REBUILD_THR = 130


@functools.lru_cache(maxsize=None)
def kmer_rebuilt():
    """kmer_world()'s dense queries (threshold 78) against an index built with threshold 130, which leaves out the k-mers whose self score is lower"""
    w = kmer_world()
    o = kmer_oracle([w["db"].seq(i, "3di", unmask=False) for i in range(w["db"].n)], index_thr=REBUILD_THR)
    s = KmerSet(o, w["dense"].queries, 78)
    o.close()
    return s


# ---- the scan sets of four clones: the lengths (register classes) of scan_queries(), other profiles, other caps -------------------------------------------
@functools.lru_cache(maxsize=None)
def clone_scan_sets():
    """[[(pssm, cap, model scores on scan_world(600))]] for four clones: clone 0 the profiles as they are, the others with their letter rows permuted
    and a lower cap"""
    w = scan_world(600)
    rng = np.random.default_rng(4)
    out = []
    for k, cap_k in enumerate((None, 40, 100, 7)):
        perm = np.arange(21) if k == 0 else rng.permutation(21)
        members = []
        for i, (_, pssm, cap) in enumerate(scan_queries()):
            p = np.ascontiguousarray(pssm[perm])
            c = cap if cap_k is None else cap_k
            members.append((p, c, w.want[i] if k == 0 else gm.scores(p, c, w.packed)))
        out.append(members)
    return out


def clone_scan_check(ctx, members, order, what, min_score=15, max_res=50):
    hits = ctx.gapless_scan_multi([(members[i][0], members[i][1], -1) for i in order], min_score, max_res)
    for k, i in enumerate(order):
        p, _, want = members[i]
        if p.shape[1] <= 896:
            got = ctx.gapless_scores_multi(k).astype(np.int32)
            assert (got == want).all(), (what, "scores", i, np.flatnonzero(got != want)[:10])
        same_hits(hits[k], gm.select(want, min_score, -1, max_res), (what, "hits", i))

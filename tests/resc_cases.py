"""tests/resc_cases.py -- what the diagonal-rescoring entry (fshost_search_rescore_diagonal_batch) is run on, and the frozen answers of the independent model
(tests/resc_model.py) for it (tests/golden/resc_v1, generator tests/golden/make_resc_golden.py).  TEST INFRASTRUCTURE: nothing of the project is imported
here.  The GPU test (tests/test_resc_entry_gpu.py) builds the sequences from the seed, reads lists, parameter sets and answers from the frozen files and
never runs the model; the CPU test (tests/test_resc_model.py) re-runs the live model on a sample.

1. THE REFERENCE RUNS: the example structures of tests/golden/scop_v1 with the argument vectors of a MANIFEST.json, through the model (model_db).
2. THE SEEDED WORLD: ten queries (1, 2, 24 .. 320 residues, four of them no multiple of 4, and one of 1025), about 300 targets of 1 .. 420 residues whose
   keys are a non-monotonic function of the id, one list of (target, diagonal) per query (20 .. 110 pairs; only pairs whose reference result is defined):
     identity   the query itself on diagonal 0, on a far diagonal (four cells: its e-value fails) and on diagonal 3
     piece      a mutated stretch of the query between random flanks, at its true diagonal; every third one also one diagonal off (the SAME target twice)
     dup        a byte-identical copy of a piece under another key, same diagonal: compareHits ends at dbKey
     tail       a piece with six X appended, same diagonal: equal e-value and score, dbLen decides
     neg        a piece behind a long left flank: negative diagonal, target not longer than the query
     random     unrelated targets on a random defined diagonal
   and list "mixed": the named query's list with undefined (negative diagonal, target longer than the query) and no-overlap pairs mixed in.
   Parameter sets are derived from the model's own records (derive()): a threshold is a named hit's value, and the next representable number beyond it."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "resc_v1")
SCOP = os.path.join(HERE, "golden", "scop_v1")
SEED = 20261021
Q_LENGTHS = [1, 2, 24, 47, 80, 129, 200, 257, 320, 1025]
N_PIECES = [0, 0, 8, 12, 18, 24, 40, 20, 16, 8]
RANDOM_LENGTHS = [1, 1, 1, 2, 2, 2, 3, 5, 9, 17, 24, 31, 33, 47, 64, 65, 80, 100, 127, 128, 129, 160, 200, 255, 256, 257, 300, 333, 400, 419, 420]
NAMED_QUERY = 5            # the query whose hits name the thresholds
ATYPES = (2, 0)
INT_MAX = 2147483647
E_ALL = 19.0           # an e-value threshold that nearly every pair passes; beyond it pairs of score 0 and 1 tie in every key of compareHits


# ---- 1. the reference's runs on the example structures ----------------------------------------------------------------------------------------------------------
def flags(par):
    return {par[i]: par[i + 1] for i in range(len(par) - 1) if par[i].startswith("-") and not par[i + 1].startswith("--")}


@functools.lru_cache(maxsize=None)
def scop_sequences():
    """-> (keys in index order, {key: (AA codes, 3Di codes)}) of the reference-written example database"""
    import diag_model as D
    aa, ss = D.read_db(os.path.join(SCOP, "db")), D.read_db(os.path.join(SCOP, "db_ss"))
    seqs = {k: (D.encode(aa[k].decode().rstrip("\n")), D.encode(ss[k].decode().rstrip("\n"))) for k in aa}
    return sorted(seqs), seqs


@functools.lru_cache(maxsize=None)
def _scop_world(atype):
    import resc_model as R
    keys, seqs = scop_sequences()
    return R.World([seqs[k] for k in keys], keys=np.array(keys, np.uint32), alignment_type=atype)


def read_pref(path):
    """{query key: [(target key, diagonal as a short)]} of a prefilter-format DB (QueryMatcher::parsePrefilterHit: three columns)"""
    import diag_model as D
    out = {}
    for q, entry in D.read_db(path).items():
        out[q] = [(int(f[0]), (int(f[2]) + 32768) % 65536 - 32768) for f in (l.split() for l in entry.decode().splitlines())]
    return out


def run_params(run):
    """the argument vector of a run -> (alignment type, model parameters, identity possible)"""
    import resc_model as R
    f = flags(run["parameters"])
    f32 = lambda x: float(np.float32(float(x)))  # noqa: E731  float parameters of the reference; -e is a double
    P = R.params(evalThr=float(f["-e"]), covThr=f32(f["-c"]), covMode=int(f["--cov-mode"]), seqIdThr=f32(f["--min-seq-id"]), seqIdMode=int(f["--seq-id-mode"]),
                 alnLenThr=int(f["--min-aln-len"]), maxAccept=int(f["--max-accept"]), maxRejected=int(f["--max-rejected"]), addBacktrace=int(f["-a"]))
    same_db = run["positional"][0] == run["positional"][1]                               # :169: a comparison of the two paths
    return int(f["--alignment-type"]), P, same_db or f["--add-self-matches"] == "1"      # :321


def model_db(run, pref, skip=False):
    """the model's result DB for a run: {query key: entry bytes}, and the Result per query key.  pref: read_pref() of the run's third argument"""
    import resc_model as R
    atype, P, ident = run_params(run)
    W = _scop_world(atype)
    keys, seqs = scop_sequences()
    idx = {k: i for i, k in enumerate(keys)}
    db, res = {}, {}
    for q in sorted(pref):
        r = R.rescore_query(W, seqs[q][0], seqs[q][1], [(idx[t], d) for t, d in pref[q]], P, identity=idx[q] if ident else -1, skip=skip, qname=str(q))
        assert not R.ties(r), ("two records that compareHits cannot order", q)
        db[q], res[q] = R.lines(r, P["addBacktrace"]).encode(), r
    return db, res


# ---- 2. the seeded world ------------------------------------------------------------------------------------------------------------------------------------------
def key_of(i):
    """dbKey of target id i: unique, not monotonic, never equal to a small id"""
    return (i * 7919 + 1013) % 100003


def _rand(rng, n):
    return rng.integers(0, 20, n).astype(np.uint8), rng.integers(0, 20, n).astype(np.uint8)


def _mutate(rng, a, s, p):
    a, s = a.copy(), s.copy()
    m = rng.random(len(a)) < p
    a[m] = rng.integers(0, 20, int(m.sum())); s[m] = rng.integers(0, 20, int(m.sum()))
    return a, s


def defined(Lq, Lt, d):
    """the pairs whose reference result exists: diagonal >= 0 inside the query, or < 0 inside a target that is not longer than the query"""
    return (0 <= d < Lq) or (d < 0 and -d < Lt and Lt <= Lq)


@functools.lru_cache(maxsize=None)
def world():
    """-> dict(queries [(AA, 3Di)], targets [(AA, 3Di)], kinds [str], keys uint32 [n], identity [int], lists {name: (query, target ids, diagonals, kinds)})"""
    rng = np.random.default_rng(SEED)
    queries = [_rand(rng, L) for L in Q_LENGTHS]
    targets, kinds = [], []

    def add(a, s, kind):
        assert 1 <= len(a) == len(s) and (len(a) <= 420 or kind == "identity")
        targets.append((np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8))); kinds.append(kind)
        return len(targets) - 1

    randoms = [add(*_rand(rng, L), "random") for L in RANDOM_LENGTHS]
    lists, identity = {}, []
    for qi, (qa, q3) in enumerate(queries):
        L = len(qa)
        me = add(qa, q3, "identity")
        identity.append(me)
        pairs = [(me, 0, "identity")]
        if L >= 24:
            pairs += [(me, L - 4, "identity far"), (me, 3, "identity near")]
        pieces = []
        for j in range(N_PIECES[qi]):
            n = max(8, int(min(L, 300) * rng.uniform(0.15, 0.9)))
            at = int(rng.integers(0, L - n + 1))
            a, s = _mutate(rng, qa[at:at + n], q3[at:at + n], float(rng.choice([0.05, 0.15, 0.3, 0.45])))
            l = int(rng.integers(0, min(at, 40) + 1)); r = int(min(420 - n - l, rng.integers(0, 41)))
            (la, ls), (ra, rs) = _rand(rng, l), _rand(rng, r)
            t = add(np.concatenate([la, a, ra]), np.concatenate([ls, s, rs]), "piece")
            pieces.append((t, at - l))
            pairs.append((t, at - l, "piece"))
            if j % 3 == 0 and at - l + 1 < L:
                pairs.append((t, at - l + 1, "piece off by one"))
        for j in (1, 4):
            if j < len(pieces):
                t, d = pieces[j]
                pairs.append((add(*targets[t], "dup"), d, "dup"))
        if len(pieces) > 2:
            t, d = pieces[2]
            ta, t3 = targets[t]
            if len(ta) <= 414:
                pairs.append((add(np.concatenate([ta, np.full(6, 20, np.uint8)]), np.concatenate([t3, np.full(6, 20, np.uint8)]), "tail"), d, "tail"))
        for j in range(min(6, N_PIECES[qi] // 3)):                                       # negative diagonals: left flank longer than the offset in the query
            n = max(8, int(L * rng.uniform(0.2, 0.5)))
            at = int(rng.integers(0, max(1, (L - n) // 3)))
            l = at + int(rng.integers(1, max(2, (L - n - at) // 2)))
            if n + l > min(L, 420):
                continue
            a, s = _mutate(rng, qa[at:at + n], q3[at:at + n], 0.1)
            la, ls = _rand(rng, l)
            pairs.append((add(np.concatenate([la, a]), np.concatenate([ls, s]), "neg"), at - l, "neg"))
        want = 20 if L < 24 else 6 + N_PIECES[qi] // 3
        k = 0
        while k < want:
            t = int(rng.choice(randoms))
            Lt = len(targets[t][0])
            d = int(rng.integers(-min(Lt, L) + 1, L)) if L > 1 else 0
            if defined(L, Lt, d) and t not in [x for x, _, _ in pairs]:      # never twice: two low scores of one target tie in every key
                pairs.append((t, d, "random")); k += 1
        order = rng.permutation(len(pairs))
        pairs = [pairs[i] for i in order]
        assert all(defined(L, len(targets[t][0]), d) for t, d, _ in pairs) and 20 <= len(pairs) <= 110, (qi, len(pairs))
        lists[f"q{qi}"] = (qi, np.array([t for t, _, _ in pairs], np.uint32), np.array([d for _, d, _ in pairs], np.int16), [k for _, _, k in pairs])
    # the named query's list with pairs the reference cannot rescore mixed in
    Q = NAMED_QUERY
    L = Q_LENGTHS[Q]
    _, ts, ds, ks = lists[f"q{Q}"]
    longer = [t for t in randoms if len(targets[t][0]) > L]
    short5 = [t for t in randoms if len(targets[t][0]) == 5][0]
    bad = [(longer[0], -1, "undefined"), (longer[1], -100, "undefined"), (longer[-1], -(len(targets[longer[-1]][0]) - 1), "undefined"),
           (longer[2], L, "no overlap"), (short5, -5, "no overlap"), (longer[3], 32767, "no overlap"), (short5, -32768, "no overlap"), (identity[Q], -1, "defined")]
    pairs = list(zip(ts.tolist(), ds.tolist(), ks))
    for i, b in enumerate(bad):
        pairs.insert(3 + 5 * i, b)
    lists["mixed"] = (Q, np.array([t for t, _, _ in pairs], np.uint32), np.array([d for _, d, _ in pairs], np.int16), [k for _, _, k in pairs])
    keys = np.array([key_of(i) for i in range(len(targets))], np.uint32)
    assert len(set(keys.tolist())) == len(keys) and (np.diff(keys.astype(np.int64)) < 0).any() and all(int(keys[i]) != i for i in identity)
    return dict(queries=queries, targets=targets, kinds=kinds, keys=keys, identity=identity, lists=lists)


DEFINED = [f"q{i}" for i in range(len(Q_LENGTHS))]


# ---- the live model on this world (generator, and the sample of the CPU test) -------------------------------------------------------------------------------------
class Live:
    def __init__(self, atype):
        import resc_model as R
        self.R, self.w = R, world()
        self.W = R.World(self.w["targets"], keys=self.w["keys"], alignment_type=atype)
        self.extra = {}
        self._runs = {}

    def list_of(self, name):
        return self.w["lists"][name] if name in self.w["lists"] else self.extra[name]

    def one(self, name, S):
        """the model on list `name` under the set S (dict P / identity / skip)"""
        q, ts, ds = self.list_of(name)[:3]
        k = (name, bytes(ts), bytes(ds), tuple(sorted(S["P"].items())), S["identity"], S["skip"])
        if k not in self._runs:
            qa, q3 = self.w["queries"][q]
            self._runs[k] = self.R.rescore_query(self.W, qa, q3, list(zip(ts.tolist(), ds.tolist())), S["P"], identity=self.w["identity"][q] if S["identity"] else -1,
                                                 skip=S["skip"], qname=name)
        return self._runs[k]


def _next(x, up=True, dt=np.float32):
    return float(np.nextafter(dt(x), dt(np.inf if up else -np.inf)))


def _runs_of_rejected(out):
    """lengths of the runs of counted rejections, each ended by an accepted hit (the last one by the end of the list); skipped pairs count nothing"""
    runs, n = [], 0
    for o in out:
        if o.startswith("accepted"):
            runs.append(n); n = 0
        elif not o.startswith("skipped") and not o.startswith("not reached"):
            n += 1
    return runs + [n]


def derive(live):
    """-> ({set name: dict(P, identity, skip, lists, differs)}, {derived list name: (query, ids, diagonals, kinds)}).  Every threshold is read off a record of
    the live model and kept as the exact number (float32 / double).  `differs`: for a set named *_next / *_below, (the *_eq set, the list, the named
    position, the outcome the named hit must have beyond the threshold) -- check_pairs() holds each such pair of sets to it."""
    R, w = live.R, live.w
    Q, qn = NAMED_QUERY, f"q{NAMED_QUERY}"
    sets = {}

    def S(name, lists=None, identity=True, skip=False, differs=None, **kw):
        sets[name] = dict(P=R.params(**kw), identity=identity, skip=skip, lists=list(lists or DEFINED), differs=differs)
        return sets[name]

    r = live.one(qn, S("default"))
    S("noident", identity=False)
    S("nobt", addBacktrace=0)
    S("e1e-3", evalThr=1e-3)
    S("e_all", evalThr=E_ALL)                                    # nearly everything passes: the same target accepted twice
    _, ts, ds, kinds = w["lists"][qn]
    L = Q_LENGTHS[Q]
    acc = [i for i in range(len(r.records)) if kinds[r.hit_of_record[i]] in ("piece", "neg")]
    assert len(acc) >= 8
    med = lambda f, cand=acc: sorted(cand, key=lambda i: (f(r.records[i]), i))[len(cand) // 2]  # noqa: E731  the median hit by that value
    # canBeCovered, modes 0 .. 5: the length ratio of a listed target, and the next float above it
    f32 = np.float32
    ratio = {0: lambda q, t: min(f32(q) / f32(t), f32(t) / f32(q)), 1: lambda q, t: f32(q) / f32(t), 2: lambda q, t: f32(t) / f32(q),
             3: lambda q, t: f32(t) / f32(q), 4: lambda q, t: f32(q) / f32(t), 5: lambda q, t: min(f32(t), f32(q)) / max(f32(t), f32(q))}
    for mode in range(6):
        cand = sorted({(float(ratio[mode](L, len(w["targets"][int(t)][0]))), k) for k, t in enumerate(ts)})
        cand = [(v, k) for v, k in cand if 0.3 < v < 0.98]
        v, k = cand[len(cand) // 2]
        S(f"cbc{mode}_eq", covMode=mode, covThr=v)
        S(f"cbc{mode}_next", covMode=mode, covThr=_next(v), differs=(f"cbc{mode}_eq", qn, k, "not coverable"))
    # hasCoverage, modes 0 / 1 / 2: the coverage of a named accepted hit; mode 0 once more with each of its two comparisons at equality on its own
    for name, mode, f, cand in (("cov0", 0, lambda x: min(x["qcov"], x["dbcov"]), acc), ("cov1", 1, lambda x: x["dbcov"], acc), ("cov2", 2, lambda x: x["qcov"], acc),
                                ("cov0q", 0, lambda x: x["qcov"], [i for i in acc if r.records[i]["qcov"] < r.records[i]["dbcov"]]),
                                ("cov0t", 0, lambda x: x["dbcov"], [i for i in acc if r.records[i]["dbcov"] < r.records[i]["qcov"]])):
        i = med(f, cand)
        v = float(f(r.records[i]))
        S(f"{name}_eq", covMode=mode, covThr=v)
        S(f"{name}_next", covMode=mode, covThr=_next(v), differs=(f"{name}_eq", qn, r.hit_of_record[i], "coverage"))
    # e-value: a hit's own value as the exact double, and the next double below it
    i = med(lambda x: x["eval"])
    ev = float(r.records[i]["eval"])
    S("ev_eq", evalThr=ev)
    S("ev_below", evalThr=_next(ev, False, np.float64), differs=("ev_eq", qn, r.hit_of_record[i], "e-value"))
    # sequence identity under each mode
    for mode in (0, 1, 2):
        rm = live.one(qn, dict(P=R.params(seqIdMode=mode), identity=True, skip=False))
        assert rm.hit_of_record == r.hit_of_record
        i = sorted(acc, key=lambda i: (rm.records[i]["seqId"], i))[len(acc) // 2]          # the order of the records does not depend on the identity
        v = float(rm.records[i]["seqId"])
        assert 0 < v < 1
        S(f"sid{mode}_eq", seqIdMode=mode, seqIdThr=v)
        S(f"sid{mode}_next", seqIdMode=mode, seqIdThr=_next(v), differs=(f"sid{mode}_eq", qn, r.hit_of_record[i], "seq id"))
    i = med(lambda x: x["alnLength"])
    ln = int(r.records[i]["alnLength"])
    S("len_eq", alnLenThr=ln)
    S("len_next", alnLenThr=ln + 1, differs=("len_eq", qn, r.hit_of_record[i], "aln length"))
    # the identity: accepted although a criterion fails, on all three diagonals; not so without the identity argument
    S("ident_len", alnLenThr=1026)
    S("ident_sid", evalThr=E_ALL, seqIdThr=float(f32(0.9)))
    S("ident_sid_noid", identity=False, evalThr=E_ALL, seqIdThr=float(f32(0.9)))
    # the counters, on a gate that mixes accepted and rejected hits
    mix = dict(evalThr=1e-3)
    out = live.one(qn, dict(P=R.params(**mix), identity=True, skip=False)).outcomes
    nacc, runs = sum(o.startswith("accepted") for o in out), _runs_of_rejected(out)
    longest = max(runs)
    assert nacc >= 4 and longest >= 2, (nacc, runs)
    S("acc1", maxAccept=1, **mix); S("acc2", maxAccept=2, **mix); S("acc_all", maxAccept=nacc, **mix); S("acc_all_but1", maxAccept=nacc - 1, **mix)
    S("rej1", maxRejected=1, **mix); S("rej_longest", maxRejected=longest, **mix); S("rej_longest1", maxRejected=longest + 1, **mix)
    # the reset: a run of m - 1 rejections, an accepted hit, and later a run of at least m
    m = next(a + 1 for k, a in enumerate(runs[:-1]) if a >= 1 and max(runs[:k + 1]) == a and max(runs[k + 1:]) > a)
    reached = live.one(qn, dict(P=R.params(maxRejected=m, **mix), identity=True, skip=False)).outcomes
    S("rej_reset", maxRejected=m, **mix)
    S("acc_rej_reset", maxRejected=m, maxAccept=sum(o.startswith("accepted") for o in reached), **mix)
    S("acc_rej_mix", maxAccept=3, maxRejected=2, **mix)
    S("both_1", maxAccept=1, maxRejected=1)
    # the skip rule: lists made of pairs whose outcome under `mix` is known
    pos_acc = [k for k, o in enumerate(out) if o == "accepted"]
    pos_rej = [k for k, o in enumerate(out) if o == "e-value"]
    _, mts, mds, mks = w["lists"]["mixed"]
    und = [k for k, x in enumerate(mks) if x == "undefined"]
    nov = [k for k, x in enumerate(mks) if x == "no overlap"]
    extra = {}

    def make(name, items):
        """items: ('a' | 'r' | 'u' | 'n', running number) -> a list for the named query"""
        src = {"a": (ts, ds, pos_acc), "r": (ts, ds, pos_rej), "u": (mts, mds, und), "n": (mts, mds, nov), "g": (ts, ds, negs)}
        ids, dg, kd = [], [], []
        for c, j in items:
            a, b, p = src[c]
            ids.append(int(a[p[j]])); dg.append(int(b[p[j]])); kd.append({"a": "accepted", "r": "rejected", "u": "undefined", "n": "no overlap", "g": "negative score"}[c])
        extra[name] = live.extra[name] = (Q, np.array(ids, np.uint32), np.array(dg, np.int16), kd)

    # score differences below zero (the reversed query scores better): their e-value is a double beyond every other one; distinct targets, so no two tie
    wq = live.W.query(*w["queries"][Q])
    diff = lambda k: live.W.pair(wq, ts[k], ds[k])["score"] - live.W.pair(wq, ts[k], ds[k])["revScore"]  # noqa: E731
    negs, seen = [], set()
    for k in range(len(ts)):
        if diff(k) < 0 and int(ts[k]) not in seen:
            negs.append(k); seen.add(int(ts[k]))
    assert len(negs) >= 3
    make("negscore", [("a", 0), ("g", 0), ("g", 1), ("a", 1), ("g", 2)])
    S("negscore", lists=["negscore"], evalThr=1e300)
    # two rejections, a skipped pair, an accepted hit: with maxRejected 3 the run is maxRejected - 1 long if the skipped pair counts nothing (ours) and
    # maxRejected long if it counted as a rejection, which would end the list before the accepted hit
    make("skiprun", [("a", 0), ("r", 0), ("r", 1), ("u", 0), ("a", 1), ("r", 2), ("n", 0), ("r", 3), ("r", 4), ("a", 2)])
    S("skiprun", lists=["skiprun"], skip=True, maxRejected=3, **mix)
    S("skiprun_acc", lists=["skiprun"], skip=True, maxAccept=2, **mix)
    # an undefined pair behind the cut, skip rule off: never looked at
    make("behind", [("a", 0), ("r", 0), ("a", 1), ("u", 1), ("a", 2), ("n", 1)])
    S("behind_acc", lists=["q2", "behind"], maxAccept=2, **mix)
    make("behind_rej", [("a", 0), ("r", 0), ("r", 1), ("n", 0), ("a", 2), ("u", 0)])
    S("behind_rej", lists=["behind_rej", "q3"], maxRejected=2, **mix)
    # ... and reached: refused
    make("nov_first", [("a", 0), ("n", 2), ("u", 0), ("a", 1)])
    S("fail_undefined", lists=["q2", "mixed"])
    S("fail_no_overlap", lists=["nov_first"])
    # the skip rule on the mixed list: default gates, a coverage pre-filter in front of it (an uncoverable undefined pair is a rejection), the counters
    S("mixed_skip", lists=DEFINED + ["mixed"], skip=True)
    S("mixed_skip_cbc", lists=["mixed"], skip=True, covMode=1, covThr=float(f32(0.6)))
    S("mixed_skip_rej", lists=["mixed", "q4"], skip=True, maxRejected=longest, **mix)
    return sets, extra


def answers(live, sets):
    """-> {set: [Result or resc_model.Undefined per list of the set]}"""
    out = {}
    for name, S in sets.items():
        out[name] = []
        for ln in S["lists"]:
            try:
                out[name].append(live.one(ln, S))
            except live.R.Undefined as e:
                out[name].append(e)
    return out


def check_pairs(live, sets):
    """every *_next / *_below set against its *_eq set: the named hit changes to the stated outcome, every other change is a hit that sits at the same value
    (it takes the same new outcome), and at equality the named hit was not rejected by that gate"""
    n = 0
    for name, S in sets.items():
        if not S["differs"]:
            continue
        eq, ln, pos, new = S["differs"]
        a, b = live.one(ln, sets[eq]).outcomes, live.one(ln, S).outcomes
        diff = [k for k in range(len(a)) if a[k] != b[k]]
        assert pos in diff and b[pos] == new and a[pos] != new, (name, pos, a[pos], b[pos])
        # -c feeds canBeCovered and hasCoverage alike: a length ratio and a coverage can be the same float
        ok = {"coverage", "not coverable"} if new in ("coverage", "not coverable") else {new}
        assert all(b[k] in ok for k in diff) and len(diff) <= 8, (name, [(k, a[k], b[k]) for k in diff])
        for other in S["lists"]:
            if other != ln:
                x, y = live.one(other, sets[eq]).outcomes, live.one(other, S).outcomes
                assert all(y[k] in ok for k in range(len(x)) if x[k] != y[k]), (name, other)
        n += 1
    return n


def census(live, sets, ans):
    """what the sets reach, asserted on the model's outcomes, so that a change to the cases cannot hollow the GPU test out.  -> {set: {outcome: count}}"""
    R, w = live.R, live.w
    c = {name: R.count_outcomes([r for r in ans[name] if not isinstance(r, Exception)]) for name in sets}
    total = {}
    for name in c:
        for o, k in c[name].items():
            total[o] = total.get(o, 0) + k
    assert sorted(total) == sorted(R.OUTCOMES), sorted(set(R.OUTCOMES) - set(total))
    outcome = lambda name, ln, kind: [o for o, k in zip(ans[name][sets[name]["lists"].index(ln)].outcomes, live.list_of(ln)[3]) if k == kind]  # noqa: E731
    qn = f"q{NAMED_QUERY}"
    # the identity on its three diagonals: accepted; rejected by the e-value gate and by the coverage gate although it is the identity; accepted as identity
    assert outcome("default", qn, "identity") == ["accepted"] and outcome("default", qn, "identity far") == ["e-value"]
    assert outcome("cov0_eq", qn, "identity far") == ["coverage"]
    assert outcome("ident_len", qn, "identity") == ["accepted as identity"] and outcome("ident_len", qn, "identity far") == ["e-value"]
    # ... on a far or near diagonal, where the identity is all that accepts it: the same pairs without the identity argument fail the identity threshold
    as_id = [(ln, k) for ln, rs in zip(sets["ident_sid"]["lists"], ans["ident_sid"]) for k, o in enumerate(rs.outcomes) if o == "accepted as identity"]
    assert len(as_id) >= 3 and all(live.list_of(ln)[3][k] in ("identity far", "identity near") for ln, k in as_id), as_id
    assert all(ans["ident_sid_noid"][sets["ident_sid_noid"]["lists"].index(ln)].outcomes[k] == "seq id" for ln, k in as_id)
    assert "accepted as identity" not in c["ident_sid_noid"] and outcome("ident_sid_noid", qn, "identity") == ["accepted"]
    assert c["noident"] == c["default"]
    # the same target twice, both accepted; ties decided by dbLen and by dbKey, the key order against the list order at least once
    r = ans["e_all"][DEFINED.index(qn)]
    keys = [int(x) for x in r.records["dbKey"]]
    assert len(keys) > len(set(keys))
    by_key = by_len = 0
    for rs in ans["default"]:
        for i in range(len(rs.records) - 1):
            a, b = rs.records[i], rs.records[i + 1]
            if a["eval"] == b["eval"] and a["score"] == b["score"]:
                by_len += a["dbLen"] != b["dbLen"]
                by_key += a["dbLen"] == b["dbLen"] and rs.hit_of_record[i] > rs.hit_of_record[i + 1]
    assert by_key >= 1 and by_len >= 1, (by_key, by_len)
    for name in sets:                                          # no two records that compareHits cannot order: std::sort would leave their order open
        for rs in ans[name]:
            assert isinstance(rs, Exception) or not R.ties(rs), name
    assert any(r.hit_of_record != sorted(r.hit_of_record) for r in ans["default"])
    # negative diagonals and scores: accepted hits on them; a record whose score difference is negative
    assert sum(o == "accepted" for o in outcome("default", qn, "neg")) >= 2
    assert (ans["negscore"][0].records["score"] < 0).sum() == 3
    # the counters
    out = lambda name, ln=qn: ans[name][sets[name]["lists"].index(ln)].outcomes  # noqa: E731
    assert sum(o == "accepted" for o in out("acc1")) == 1 and sum(o == "accepted" for o in out("acc2")) == 2
    nacc = sum(o == "accepted" for o in out("e1e-3"))
    assert sum(o == "accepted" for o in out("acc_all")) == nacc and sum(o == "accepted" for o in out("acc_all_but1")) == nacc - 1
    assert "not reached: max-accept" in out("acc_all_but1")
    assert out("rej_longest")[-1] == "not reached: max-rejected" and "not reached: max-rejected" not in out("rej_longest1")
    m = sets["rej_reset"]["P"]["maxRejected"]
    runs = _runs_of_rejected(out("rej_reset"))
    assert m - 1 in runs[:-1] and runs[-1] == m and out("rej_reset")[-1] == "not reached: max-rejected"
    assert "not reached: max-accept" in out("acc_rej_reset") or "not reached: max-rejected" in out("acc_rej_reset")
    # the skip rule
    assert out("skiprun", "skiprun") == ["accepted", "e-value", "e-value", "skipped: undefined", "accepted", "e-value", "skipped: no overlap", "e-value", "e-value",
                                         "not reached: max-rejected"]
    assert out("skiprun_acc", "skiprun")[3:6] == ["skipped: undefined", "accepted", "not reached: max-accept"]
    assert out("behind_acc", "behind") == ["accepted", "e-value", "accepted"] + ["not reached: max-accept"] * 3
    assert out("behind_rej", "behind_rej") == ["accepted", "e-value", "e-value"] + ["not reached: max-rejected"] * 3
    e = ans["fail_undefined"][1]
    assert isinstance(e, R.Undefined) and e.kind == "undefined" and isinstance(ans["fail_no_overlap"][0], R.Undefined) and ans["fail_no_overlap"][0].kind == "no overlap"
    assert c["mixed_skip"]["skipped: undefined"] == 3 and c["mixed_skip"]["skipped: no overlap"] == 4
    assert c["mixed_skip_cbc"].get("skipped: undefined", 0) < 3 and c["mixed_skip_cbc"]["not coverable"] >= 1      # canBeCovered comes first
    return c


# ---- the frozen answers -----------------------------------------------------------------------------------------------------------------------------------------
def _hex(p):
    return {k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in p.items()}


def _unhex(p):
    return {k: (float.fromhex(v) if isinstance(v, str) else int(v)) for k, v in p.items()}


def save(atype, sets, extra, ans):
    import resc_model as R
    os.makedirs(GOLD, exist_ok=True)
    pool, recs, arrays, meta = {}, [], {}, {}
    for name, S in sets.items():
        idx, nrec, hit, out, nout, err = [], [], [], [], [], None
        for ln, r in zip(S["lists"], ans[name]):
            if isinstance(r, Exception):
                err = dict(list=ln, key=r.key, diagonal=r.diagonal, kind=r.kind)
                nrec.append(-1); nout.append(0)
                continue
            for rec in r.records:
                k = rec.tobytes()
                if k not in pool:
                    pool[k] = len(recs); recs.append(rec)
                idx.append(pool[k])
            nrec.append(len(r.records)); hit += r.hit_of_record
            out += [R.OUTCOMES.index(o) for o in r.outcomes]; nout.append(len(r.outcomes))
        arrays[f"{name}/idx"], arrays[f"{name}/nrec"], arrays[f"{name}/hit"] = np.array(idx, np.int32), np.array(nrec, np.int32), np.array(hit, np.int32)
        arrays[f"{name}/out"], arrays[f"{name}/nout"] = np.array(out, np.uint8), np.array(nout, np.int32)
        meta[name] = dict(params=_hex(S["P"]), identity=bool(S["identity"]), skip=bool(S["skip"]), lists=S["lists"], error=err)
    arrays["pool"] = np.array(recs, R.REC_DT)
    np.savez_compressed(os.path.join(GOLD, f"answers_t{atype}.npz"), **arrays)
    lists = {n: dict(query=int(q), ids=[int(x) for x in ids], diagonals=[int(x) for x in dg], kinds=kd) for n, (q, ids, dg, kd) in extra.items()}
    json.dump(dict(seed=SEED, outcomes=list(R.OUTCOMES), sets=meta, lists=lists), open(os.path.join(GOLD, f"sets_t{atype}.json"), "w"), indent=0, sort_keys=True)


class Frozen:
    """the frozen answers of one alignment type"""

    def __init__(self, atype):
        j = json.load(open(os.path.join(GOLD, f"sets_t{atype}.json")))
        assert j["seed"] == SEED, "the world changed: run tests/golden/make_resc_golden.py"
        self.outcome_names, self.meta, self.names = j["outcomes"], j["sets"], list(j["sets"])
        self.extra = {n: (v["query"], np.array(v["ids"], np.uint32), np.array(v["diagonals"], np.int16), v["kinds"]) for n, v in j["lists"].items()}
        z = np.load(os.path.join(GOLD, f"answers_t{atype}.npz"))
        self.z = {k: z[k] for k in z.files}

    def list_of(self, name):
        w = world()
        return w["lists"][name] if name in w["lists"] else self.extra[name]

    def params(self, name):
        return _unhex(self.meta[name]["params"])

    def set(self, name):
        m = self.meta[name]
        return dict(P=self.params(name), identity=m["identity"], skip=m["skip"], lists=m["lists"], error=m["error"])

    def records(self, name, k):
        """-> (records REC_DT, backtrace strings, list position of the hit each record belongs to) of the k-th list of the set; None where the model refuses"""
        nrec = self.z[f"{name}/nrec"]
        if nrec[k] < 0:
            return None
        a = int(np.maximum(nrec[:k], 0).sum()); b = a + int(nrec[k])
        rec = self.z["pool"][self.z[f"{name}/idx"][a:b]]
        bt = ["M" * int(x) if self.params(name)["addBacktrace"] else "" for x in rec["alnLength"]]
        return rec, bt, self.z[f"{name}/hit"][a:b]

    def outcomes(self, name, k):
        nout = self.z[f"{name}/nout"]
        a = int(nout[:k].sum())
        return [self.outcome_names[c] for c in self.z[f"{name}/out"][a:a + int(nout[k])]]

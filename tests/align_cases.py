"""tests/align_cases.py -- a seeded world for the alignment entries (fshost_search_align / _align_batch) whose gates are decided AT their edges, and the
frozen answers of the independent model (tests/align_model.py) for it (tests/golden/align_v1, generator tests/golden/make_align_golden.py).
TEST INFRASTRUCTURE: nothing of the project is imported here; the GPU test (tests/test_align_entries_gpu.py) builds the sequences from the seed, reads the
parameter sets and the answers from the frozen files and never runs the model; the CPU test (tests/test_align_model.py) re-runs the live model on a sample.

The world: 8 queries (24 .. 320 residues and one of 1025), about 330 targets of 1 .. 420 residues, one hit list per query (20 .. 110 hits), and a ninth
list that holds the named query's repeat target alone:
  identity   the query itself (the entry's `identity` argument names it)
  piece      a copy of a stretch of the query (20 .. 100 % of it), mutated, between random flanks of 0 .. 60 residues: end-based and start-based
             coverage of query and target spread over 0.1 .. 1.0
  dup        a byte-identical copy of a piece under another key (the keys are a non-monotonic function of the id)
  tail       a piece with six X appended: score, end cell and e-value unchanged, dbLen larger
  repeat     three differently mutated copies of one stretch: --alt-ali finds them one after the other
  near       a lightly mutated full copy, always the LAST hit of the list
  random     unrelated targets of 1 .. 420 residues, shared by all lists
Parameter sets are derived from the model's own records (derive()): a threshold is a named hit's value, and the next representable number beyond it."""
import functools
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "align_v1")
SEED = 20261020
Q_LENGTHS = [24, 48, 80, 129, 200, 257, 320, 1025]
N_PIECES = [14, 20, 30, 40, 70, 30, 24, 8]
RANDOM_LENGTHS = [1, 1, 2, 3, 5, 9, 17, 24, 31, 33, 47, 64, 65, 80, 100, 127, 128, 129, 160, 200, 255, 256, 257, 300, 333, 400, 419, 420]
NAMED_QUERY = 3            # the query whose hits name the thresholds
ATYPES = (2, 0)


def key_of(i):
    """dbKey of target id i: unique, not monotonic"""
    return (i * 7919 + 13) % 100003


def _rand(rng, n):
    return rng.integers(0, 20, n).astype(np.uint8), rng.integers(0, 20, n).astype(np.uint8)


def _mutate(rng, a, s, p):
    a, s = a.copy(), s.copy()
    m = rng.random(len(a)) < p
    a[m] = rng.integers(0, 20, int(m.sum())); s[m] = rng.integers(0, 20, int(m.sum()))
    if len(a) > 30 and rng.random() < 0.4:                     # one indel of 2 .. 9 residues
        n, at = int(rng.integers(2, 10)), int(rng.integers(5, len(a) - 5))
        if rng.random() < 0.5:
            a, s = np.concatenate([a[:at], a[at + n:]]), np.concatenate([s[:at], s[at + n:]])
        else:
            ia, is_ = _rand(rng, n)
            a, s = np.concatenate([a[:at], ia, a[at:]]), np.concatenate([s[:at], is_, s[at:]])
    return a, s


def _flank(rng, a, s, cap=420):
    room = max(0, cap - len(a))
    l = int(min(room, rng.integers(0, 61))); r = int(min(room - l, rng.integers(0, 61)))
    la, ls = _rand(rng, l); ra, rs = _rand(rng, r)
    return np.concatenate([la, a, ra]), np.concatenate([ls, s, rs])


@functools.lru_cache(maxsize=None)
def world():
    """-> dict(queries [(AA, 3Di)], targets [(AA, 3Di)], kinds [str], keys uint32 [n], lists [uint32 arrays], identity [int])"""
    rng = np.random.default_rng(SEED)
    queries = [_rand(rng, L) for L in Q_LENGTHS]
    targets, kinds = [], []

    def add(a, s, kind):
        assert 1 <= len(a) == len(s) <= 1025 and (len(a) <= 420 or kind == "identity")
        targets.append((np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8))); kinds.append(kind)
        return len(targets) - 1

    randoms = [add(*_rand(rng, L), "random") for L in RANDOM_LENGTHS]
    lists, identity = [], []
    for qi, (qa, q3) in enumerate(queries):
        L = len(qa)
        own = [add(qa, q3, "identity")]
        identity.append(own[0])
        longest = L if L <= 420 else 100
        for j in range(N_PIECES[qi]):
            n = max(8, int(longest * rng.uniform(0.2, 1.0)))
            at = int(rng.integers(0, L - n + 1))
            a, s = _mutate(rng, qa[at:at + n], q3[at:at + n], float(rng.choice([0.05, 0.15, 0.3, 0.45])))
            own.append(add(*_flank(rng, a, s), "piece"))
        own.append(add(*targets[own[2]], "dup"))
        own.append(add(*targets[own[5]], "dup"))
        ta, t3 = targets[own[3]]
        own.append(add(np.concatenate([ta, np.full(6, 20, np.uint8)]), np.concatenate([t3, np.full(6, 20, np.uint8)]), "tail"))
        n = min(int(L * 0.6), 110)
        at = int(rng.integers(0, L - n + 1))
        parts_a, parts_s = [], []
        for p in (0.03, 0.12, 0.2):
            a, s = _mutate(rng, qa[at:at + n], q3[at:at + n], p)
            fa, fs = _rand(rng, 7)
            parts_a += [a, fa]; parts_s += [s, fs]
        ra, rs = np.concatenate(parts_a)[:420], np.concatenate(parts_s)[:420]
        own.append(add(ra, rs, "repeat"))
        strangers = [int(x) for x in rng.choice(randoms, size=min(len(randoms), 6 + N_PIECES[qi] // 3), replace=False)]
        order = own + strangers
        rng.shuffle(order)
        if L <= 420:
            a, s = _mutate(rng, qa, q3, 0.05)
        else:
            a, s = _mutate(rng, qa[300:400], q3[300:400], 0.05)
        order.append(add(a, s, "near"))
        lists.append(np.array(order, np.uint32))
    # one more list: the named query again, against its repeat target alone -- with --alt-ali 2 the result capacity n * (1 + alt) is reached
    queries.append(queries[NAMED_QUERY]); identity.append(identity[NAMED_QUERY])
    lists.append(np.array([t for t in lists[NAMED_QUERY] if kinds[int(t)] == "repeat"], np.uint32))
    keys = np.array([key_of(i) for i in range(len(targets))], np.uint32)
    assert len(set(keys.tolist())) == len(keys) and (np.diff(keys.astype(np.int64)) < 0).any()
    return dict(queries=queries, targets=targets, kinds=kinds, keys=keys, lists=lists, identity=identity)


# ---- parameter sets, derived from the model (generator only) --------------------------------------------------------------------------------------------
def _next(x, up=True, dt=np.float32):
    return float(np.nextafter(dt(x), dt(np.inf if up else -np.inf)))


def derive(run, evalue_fwd):
    """run(P) -> [Result per query] (the live model, cached); evalue_fwd(query, hit position) -> the forward e-value of that pair.
    -> {name: params dict}.  Every threshold is read off a record of the model and stored as the exact number (float32 / double)."""
    import align_model as A
    W = world()
    Q = NAMED_QUERY
    sets = {"default": A.params()}
    base = run(sets["default"])
    r = base[Q]
    acc = [i for i in range(len(r.records)) if W["kinds"][int(W["lists"][Q][r.hit_of_record[i]])] == "piece" and r.records[i]["qStartPos"] > 0]
    assert len(acc) >= 8
    by = lambda f: sorted(acc, key=lambda i: (f(r.records[i]), i))[len(acc) // 2]  # noqa: E731  the median hit by that value
    sets["e1e-3"] = A.params(evalThr=1e-3)
    # coverage modes 0, 1, 2: the start-based coverage of a named accepted hit, and the next float above it
    for mode, f in ((0, lambda x: min(x["qcov"], x["dbcov"])), (1, lambda x: x["dbcov"]), (2, lambda x: x["qcov"])):
        thr = float(f(r.records[by(f)]))
        sets[f"cov{mode}_eq"] = A.params(covMode=mode, covThr=thr)
        sets[f"cov{mode}_next"] = A.params(covMode=mode, covThr=_next(thr))
    # mode 0 once more, each of its two comparisons AT equality on its own: a hit whose query coverage is the smaller one, and one whose target coverage is
    for side, mine, other in (("q", "qcov", "dbcov"), ("t", "dbcov", "qcov")):
        cand = [i for i in acc if r.records[i][mine] < r.records[i][other]]
        i = sorted(cand, key=lambda i: (r.records[i][mine], i))[len(cand) // 2]
        thr = float(r.records[i][mine])
        sets[f"cov0{side}_eq"] = A.params(covMode=0, covThr=thr)
        sets[f"cov0{side}_next"] = A.params(covMode=0, covThr=_next(thr))
    # modes 3, 4, 5: the length ratio of a listed target, and the next float above it (ratio 1.0: the identity and any target of the query's length)
    L = Q_LENGTHS[Q]
    lens = sorted({len(W["targets"][int(t)][0]) for t in W["lists"][Q]})
    shorter = [t for t in lens if L // 2 < t < L][len([t for t in lens if L // 2 < t < L]) // 2]
    longer = [t for t in lens if L < t < 2 * L][len([t for t in lens if L < t < 2 * L]) // 2]
    for mode, ratio in ((3, np.float32(shorter) / np.float32(L)), (4, np.float32(L) / np.float32(longer)), (5, np.float32(shorter) / np.float32(L))):
        sets[f"cov{mode}_eq"] = A.params(covMode=mode, covThr=float(ratio))
        sets[f"cov{mode}_next"] = A.params(covMode=mode, covThr=_next(ratio))
    # sequence identity under each mode
    for mode in (0, 1, 2):
        rm = run(A.params(seqIdMode=mode))[Q]
        assert rm.hit_of_record == r.hit_of_record
        thr = float(rm.records[by(lambda x: x["seqId"])]["seqId"])
        assert thr > 0
        sets[f"sid{mode}_eq"] = A.params(seqIdMode=mode, seqIdThr=thr)
        sets[f"sid{mode}_next"] = A.params(seqIdMode=mode, seqIdThr=_next(thr))
    ln = int(r.records[by(lambda x: x["alnLength"])]["alnLength"])
    sets["len_eq"], sets["len_next"] = A.params(alnLenThr=ln), A.params(alnLenThr=ln + 1)
    # e-values: a hit's difference e-value and its forward e-value as exact doubles, and the next double below each
    i = by(lambda x: x["eval"])
    ev = float(r.records[i]["eval"])
    sets["ediff_eq"], sets["ediff_below"] = A.params(evalThr=ev), A.params(evalThr=_next(ev, False, np.float64))
    ef = float(evalue_fwd(Q, r.hit_of_record[i]))
    sets["efwd_eq"], sets["efwd_below"] = A.params(evalThr=ef), A.params(evalThr=_next(ef, False, np.float64))
    # accept / reject limits on top of a coverage gate that mixes accepted and rejected hits
    mix = dict(covMode=0, covThr=sets["cov0_eq"]["covThr"])
    out = run(A.params(**mix))[Q].outcomes
    runs, n = [], 0                                            # lengths of the runs of rejected hits, each ended by an accepted one
    for o in out:
        if o.startswith("accepted"):
            runs.append(n); n = 0
        else:
            n += 1
    runs.append(n)
    m = next(a + 1 for k, a in enumerate(runs[:-1]) if a >= 1 and max(runs[:k + 1]) == a and max(runs[k + 1:]) > a)
    sets["rej_reset"] = A.params(maxRejected=m, **mix)
    nacc = sum(o.startswith("accepted") for o in base[Q].outcomes)
    assert base[Q].outcomes[-1] == "accepted"
    sets["acc_last"], sets["acc_before"] = A.params(maxAccept=nacc), A.params(maxAccept=nacc - 1)
    sets["acc_rej_mix"] = A.params(maxAccept=3, maxRejected=2, **mix)
    sets["both_1"] = A.params(maxAccept=1, maxRejected=1)
    # --alt-ali
    for k in (1, 2, 3):
        sets[f"alt{k}"] = A.params(altAlignment=k)
    a2 = run(sets["alt2"])[Q]
    pos_rep = [k for k, t in enumerate(W["lists"][Q]) if W["kinds"][int(t)] == "repeat"][0]
    reps = [i for i in range(len(a2.records)) if a2.hit_of_record[i] == pos_rep]
    reps.sort(key=lambda i: -int(a2.records[i]["score"]))
    assert len(reps) == 3, "the repeat target yields two further alignments"
    first_alt = a2.records[reps[1]]
    sets["alt_ediff"] = A.params(altAlignment=2, evalThr=_next(float(first_alt["eval"]), False, np.float64))
    sets["alt_len"] = A.params(altAlignment=2, alnLenThr=int(first_alt["alnLength"]) + 1)
    sets["alt_cov"] = A.params(altAlignment=2, covMode=2, covThr=_next(float(first_alt["qcov"])))
    sets["alt_cov_end"] = A.params(altAlignment=1, covMode=0, covThr=sets["cov0_eq"]["covThr"])
    sets["alt_e1e-3"] = A.params(altAlignment=3, evalThr=1e-3)
    # the identity target of the shortest query fails a score gate: it is NOT accepted (isIdentity only overrides checkCriteria)
    r0 = base[0]
    ident = [i for i in range(len(r0.records)) if int(W["lists"][0][r0.hit_of_record[i]]) == W["identity"][0]][0]
    sets["ident_below"] = A.params(evalThr=_next(float(r0.records[ident]["eval"]), False, np.float64))
    return sets


# ---- the frozen answers -----------------------------------------------------------------------------------------------------------------------------------------
def _hex(p):
    return {k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in p.items()}


def _unhex(p):
    return {k: (float.fromhex(v) if isinstance(v, str) else int(v)) for k, v in p.items()}


def save(atype, sets, answers, seed=SEED):
    """answers: {set name: [Result per query]}.  Records and CIGARs go into one pool of distinct (record, CIGAR) pairs; per set: the pool indices of the
    records in order, records per query, the outcome code of every hit, the reversed SW records, the looked-at count per query, the alt_ends."""
    import align_model as A
    os.makedirs(GOLD, exist_ok=True)
    pool, recs, cigs, arrays, meta = {}, [], [], {}, {}
    first = answers["default"]
    arrays["n"] = np.array([len(r.fwd) for r in first], np.int32)
    arrays["fwd"] = np.concatenate([r.fwd for r in first]).view(np.int32).reshape(-1, 4)
    for name, res in answers.items():
        idx = []
        for q, r in enumerate(res):
            assert (r.fwd == first[q].fwd).all()
            for rec, cig in zip(r.records, r.cigars):
                k = (rec.tobytes(), cig)
                if k not in pool:
                    pool[k] = len(recs); recs.append(rec); cigs.append(cig)
                idx.append(pool[k])
        arrays[f"{name}/idx"] = np.array(idx, np.int32)
        arrays[f"{name}/nrec"] = np.array([len(r.records) for r in res], np.int32)
        arrays[f"{name}/hit"] = np.array([k for r in res for k in r.hit_of_record], np.int32)
        arrays[f"{name}/out"] = np.array([A.OUTCOMES.index(o) for r in res for o in r.outcomes], np.uint8)
        arrays[f"{name}/rev"] = np.concatenate([r.rev for r in res]).view(np.int32).reshape(-1, 4)
        arrays[f"{name}/looked"] = np.array([r.reversed for r in res], np.int32)
        meta[name] = dict(params=_hex(sets[name]), alt_ends=[[q, k, n, why] for q, r in enumerate(res) for k, n, why in r.alt_ends])
    arrays["pool"] = np.array(recs, A.REC_DT) if recs else np.zeros(0, A.REC_DT)
    arrays["cigars"] = np.frombuffer("\n".join(cigs).encode(), np.uint8)
    np.savez_compressed(os.path.join(GOLD, f"answers_t{atype}.npz"), **arrays)
    json.dump(dict(seed=seed, outcomes=list(A.OUTCOMES), sets=meta), open(os.path.join(GOLD, f"sets_t{atype}.json"), "w"), indent=0, sort_keys=True)


class Frozen:
    """the frozen answers of one alignment type"""

    def __init__(self, atype):
        self.atype = atype
        j = json.load(open(os.path.join(GOLD, f"sets_t{atype}.json")))
        assert j["seed"] == (SEED if atype != "ca" else CA_SEED), "the world changed: run tests/golden/make_align_golden.py"
        self.outcome_names = j["outcomes"]
        self.meta = j["sets"]
        self.names = list(self.meta)
        z = np.load(os.path.join(GOLD, f"answers_t{atype}.npz"))
        self.z = {k: z[k] for k in z.files}
        self.cigars = bytes(self.z["cigars"]).decode().split("\n")
        self.n = [int(x) for x in self.z["n"]]
        assert atype == "ca" or self.n == [len(x) for x in world()["lists"]]
        self.off = np.concatenate([[0], np.cumsum(self.n)])

    def params(self, name):
        return _unhex(self.meta[name]["params"])

    def alt_ends(self, name):
        return [tuple(x) for x in self.meta[name]["alt_ends"]]

    def fwd(self, q):
        return self.z["fwd"][self.off[q]:self.off[q + 1]]

    def rev(self, name, q):
        return self.z[f"{name}/rev"][self.off[q]:self.off[q + 1]]

    def looked(self, name):
        return self.z[f"{name}/looked"]

    def outcomes(self, name, q):
        return [self.outcome_names[c] for c in self.z[f"{name}/out"][self.off[q]:self.off[q + 1]]]

    def records(self, name, q):
        """-> (records REC_DT, CIGARs, list position of the hit each record belongs to)"""
        nrec = self.z[f"{name}/nrec"]
        a = int(nrec[:q].sum()); b = a + int(nrec[q])
        idx = self.z[f"{name}/idx"][a:b]
        return self.z["pool"][idx], [self.cigars[i] for i in idx], self.z[f"{name}/hit"][a:b]

    def count(self, name):
        c = {}
        for q in range(len(self.n)):
            for o in self.outcomes(name, q):
                c[o] = c.get(o, 0) + 1
        return c


# ---- the live model on this world (generator, and the sample of the CPU test) -------------------------------------------------------------------------------------
class Live:
    def __init__(self, atype):
        import align_model as A
        self.A, self.w = A, world()
        self.W = A.World(self.w["targets"], keys=self.w["keys"], alignment_type=atype)
        self._runs = {}

    def query(self, q, P):
        k = (q, tuple(sorted(P.items())))
        if k not in self._runs:
            qa, q3 = self.w["queries"][q]
            self._runs[k] = self.A.align_query(self.W, qa, q3, self.w["lists"][q], P, identity=self.w["identity"][q])
        return self._runs[k]

    def run(self, P):
        return [self.query(q, P) for q in range(len(self.w["queries"]))]

    def evalue_fwd(self, q, pos):
        qa, q3 = self.w["queries"][q]
        return self.W.evalue(self.W.query(qa, q3), int(self.query(q, self.A.params()).fwd[pos]["score"]))


# ---- the twelve example structures with their C-alpha data (tests/golden/ca_v1): thresholds on LDDT and TM-score, structure bits ----------------------------------
CA_SEED = "ca_v1 shuffled"


@functools.lru_cache(maxsize=None)
def ca_world():
    """every structure against every structure, the frozen prefilter lists in a seeded order; ca[i]: the <db>_ca entry of target i as stored"""
    import diag_model as D
    import lddt_cases as LC
    aa, ss, ca = LC.read_db("db"), LC.read_db("db_ss"), LC.read_db("db_ca")
    keys = sorted(aa)
    idx = {k: i for i, k in enumerate(keys)}
    seqs = [(D.encode(aa[k].decode().rstrip("\n")), D.encode(ss[k].decode().rstrip("\n"))) for k in keys]
    pref = LC.read_db("pref")
    lists = [np.array([idx[int(l.split()[0])] for l in pref[k].decode().splitlines()], np.uint32) for k in keys]
    assert all(len(x) == len(keys) for x in lists)
    # the prefilter's order puts the hits that a threshold drops and the ones an e-value rejects behind all the accepted ones, where a wrong count of
    # the rejected decides nothing: a seeded shuffle of every list mixes them
    rng = np.random.default_rng(SEED + 2)
    lists = [rng.permutation(x).astype(np.uint32) for x in lists]
    return dict(queries=seqs, targets=seqs, keys=np.array(keys, np.uint32), lists=lists, identity=list(range(len(keys))), ca=[ca[k] for k in keys])


@functools.lru_cache(maxsize=None)
def ca_values():
    """{(query key, target key): (qStart, dbStart, cigar, avgLddtScore, the three raw TM rows)} of ca_v1's aln_l0 records: the frozen answers of
    tests/lddt_model.py and tests/tm_model.py (model_fixture_raw.npy)"""
    import lddt_cases
    import lddt_model
    import tm_cases
    recs = lddt_cases.records("aln_l0")
    cols = lddt_cases.model_columns("db", "aln_l0")
    raw = tm_cases.frozen_raw("fixture")
    out = {}
    for r, (q, t, qs, ts, cig) in enumerate(recs):
        assert (q, t) not in out
        out[(q, t)] = (qs, ts, cig, lddt_model.average(cols[r])[0], raw[3 * r:3 * r + 3])
    return out


def ca_callbacks(qkey, tkeys, P):
    """the lddt / tm callbacks of align_model.align_query for a query of ca_v1 (source key qkey) whose hit k is the structure of source key tkeys[k]:
    the frozen value is taken only after the model's own start cells and CIGAR were found equal to the record it belongs to"""
    import align_model as A
    import tm_cases
    import tm_model
    vals = ca_values()

    def entry(k, rec, bt):
        v = vals[(qkey, tkeys[k])]
        assert (int(rec["qStartPos"]), int(rec["dbStartPos"]), A.compress(bt)) == v[:3], "the frozen value belongs to another alignment"
        return v

    def lddt(k, rec, bt):
        return entry(k, rec, bt)[3]

    def tm(k, rec, bt):
        v = entry(k, rec, bt)
        nl = tm_model.normalization(P["tmMode"], min(int(rec["qEndPos"]) - int(rec["qStartPos"]), int(rec["dbEndPos"]) - int(rec["dbStartPos"])),
                                    int(rec["qLen"]), int(rec["dbLen"]))
        n, s1, s2, _ = tm_cases.as_floats(v[4][P["tmMode"]])
        return tm_model.tm_finish(n, s1, s2, nl)
    return lddt, tm


class LiveCa:
    def __init__(self):
        import align_model as A
        self.A, self.w = A, ca_world()
        self.W = A.World(self.w["targets"], keys=self.w["keys"], alignment_type=2)
        self._runs = {}

    def query(self, q, P):
        k = (q, tuple(sorted(P.items())))
        if k not in self._runs:
            qa, q3 = self.w["queries"][q]
            keys = self.w["keys"]
            lddt, tm = ca_callbacks(int(keys[q]), [int(keys[t]) for t in self.w["lists"][q]], P)
            self._runs[k] = self.A.align_query(self.W, qa, q3, self.w["lists"][q], P, identity=q, lddt=lddt, tm=tm)
        return self._runs[k]

    def run(self, P):
        return [self.query(q, P) for q in range(len(self.w["queries"]))]


def ca_sets():
    import align_model as A
    sets = {"default": A.params()}
    for m in (0, 1, 2):
        sets[f"tm07_m{m}"] = A.params(tmThr=float(np.float32(0.7)), tmMode=m)
    sets["lddt07"] = A.params(lddtThr=float(np.float32(0.7)))
    sets["lddt07_tm07_m1"] = A.params(lddtThr=float(np.float32(0.7)), tmThr=float(np.float32(0.7)), tmMode=1)
    sets["sb"] = A.params(structureBits=1)
    sets["sb_lddt07_tm07_m1"] = A.params(structureBits=1, lddtThr=float(np.float32(0.7)), tmThr=float(np.float32(0.7)), tmMode=1)
    # cut-short lists: a hit dropped by a threshold counts neither as accepted nor as rejected
    for name in ("tm07_m0", "tm07_m2", "lddt07", "lddt07_tm07_m1", "sb_lddt07_tm07_m1"):
        sets[name + "_e_rej2"] = dict(sets[name], evalThr=1e-2, maxRejected=2)
        sets[name + "_acc3"] = dict(sets[name], maxAccept=3)
    return sets

"""tests/profile_cases.py -- a seeded world for the profile-query alignment entries (fshost_search_align_profile / _align_batch_profile, and underneath
them profileBacktrace -> startposBacktraceCore -> bandedBacktraceProfile), and the frozen answers of the independent model for it: tests/align_model.py's
accept loop over tests/profile_model.py's ProfileWorld (tests/golden/profile_align_v1, generator tests/golden/make_profile_align_golden.py).
TEST INFRASTRUCTURE: nothing of the project is imported here; the GPU test (tests/test_profile_entries_gpu.py) builds the entries and sequences from the
seed, reads the parameter sets and the answers from the frozen files and never runs the model; the CPU test (tests/test_profile_cases.py) re-runs the live
model on a sample and holds it to the reference binary's frozen runs on this very world.

The world: 7 profile queries of 17 .. 1025 positions (1025: the int16 path), each a pair of entries (AA, 3Di) whose stored scores are 4 x the
substitution-matrix column of a master sequence plus noise, every tenth position at the extremes; about 190 targets of 1 .. 420 residues (the identity
targets are as long as their queries); one hit list per query (12 .. 40 hits), and an eighth list: 600 positions of the constant maximum against the
1025-residue identity target and a 420-residue one.  Target kinds: those of tests/align_cases.py (identity, piece, dup, tail, near, random) and
  edge       a copy of the master stretch that ENDS at row 15, 16, 31, 32, 511, 512, 1023 or 1024: the reverse pass runs on a prefix of qEnd + 1 rows
  xhead      a piece with three X directly before the aligned stretch and no flank on that side: the X row of a profile is zero, so the reverse pass
             reaches the forward score in more than one cell and its tie rule (first column, then smallest row) decides the start cell
  xmid       a piece with a run of four X inside
  longgap    a piece with 25 .. 40 residues deleted, one with as many inserted, and one with both (rectangle near-square, the path far off the diagonal:
             the band |dbLen - qLen| + 1 must double)
  row / col  one master letter between X flanks, and a 1-residue target: the best alignment is a single cell
  slot       two master letters that lie three or four rows apart in the query: where both score, a rectangle of two columns whose path runs down the last
             column, the column banded_sw's `edge` slot (tests/profile_model.py, banded_path) clears in the row above
Parameter sets are derived from the model's own records (derive()): a threshold is a named hit's value, and the next representable number beyond it."""
import functools
import json
import os

import numpy as np

from align_cases import _flank, _mutate, _next, _rand, key_of

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "profile_align_v1")
SEED = 20261022
Q_LENGTHS = [17, 33, 80, 129, 257, 513, 1025]
N_PIECES = [3, 4, 8, 12, 8, 7, 6]
RANDOM_LENGTHS = [1, 2, 5, 17, 33, 64, 129, 257, 420]
BORDERS = (16, 32, 512, 1024)
NAMED_QUERY = 3            # the query whose hits name the thresholds
SAT_QUERY = 7              # the saturating list
SAT_LEN = 600
X = 20
INT_MAX = 2147483647
LETTERS = "ACDEFGHIKLMNPQRSTVWYX"
RECORD = 25
# the parameter sets the reference binary is run with (generator), by name
REFERENCE_SETS = ("default", "cov1_eq", "cov2_eq", "sid1_eq", "len_eq", "gap8_2")

DEFAULTS = dict(evalThr=10.0, covThr=0.0, covMode=0, seqIdThr=0.0, seqIdMode=0, alnLenThr=0, maxAccept=INT_MAX, maxRejected=INT_MAX, altAlignment=0,
                tmThr=0.0, tmMode=0, lddtThr=0.0, structureBits=0, gapOpen=10, gapExtend=1, addBacktrace=1)


def params(**kw):
    """align_model.params()'s keys and three more: the gap costs and -a, which the profile entries read from the handle's parameters"""
    p = dict(DEFAULTS)
    assert all(k in p for k in kw), kw
    p.update(kw)
    return p


def matrices():
    """(3Di at bit factor 2.1, BLOSUM62 at 1.4) as int32 [21, 21], from the frozen reference fixture (a data file)"""
    g = np.load(os.path.join(HERE, "golden", "hotpath_v1.npz"))
    return g["sub_mat3di_2.1"].reshape(21, 21).astype(np.int32), g["sub_blosum62_1.4"].reshape(21, 21).astype(np.int32)


def _entry(rng, mat, master, consensus=None, spoil_first=False):
    """an entry whose stored scores are 4 x the matrix column of the master letter + noise, every tenth position at the extremes, clipped to int8"""
    import profile_model as pm
    L = len(master)
    stored = 4 * mat[:20, master] + rng.integers(-9, 10, (20, L))
    # every tenth position at the extremes: the largest byte on the master's letter, the smallest on the other 19 (extremes thrown per letter AND
    # position would let every target hop from one such row to the next, and every alignment would span the whole query)
    tenth = np.arange(0, L, 10)
    stored[:, tenth] = -128
    stored[master[tenth], tenth] = 127
    if spoil_first:                                        # the master's own letter scores the minimum at position 0: no alignment of the identity
        stored[master[0], 0] = -128                        # target starts there, its coverage stays below 1
    return pm.encode(np.clip(stored, -128, 127).astype(np.int8), master, consensus=consensus)


def _xs(n):
    return np.full(n, X, np.uint8), np.full(n, X, np.uint8)


def _cat(*parts):
    return np.concatenate([p[0] for p in parts]).astype(np.uint8), np.concatenate([p[1] for p in parts]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def world():
    """-> dict(entries [(AA entry, 3Di entry)], masters [(AA, 3Di)], targets [(AA, 3Di)], kinds [str], keys uint32 [n], lists [uint32 arrays], identity [int])"""
    rng = np.random.default_rng(SEED)
    m3, mA = matrices()
    masters = [_rand(rng, L) for L in Q_LENGTHS]
    entries = []
    for qi, (qa, q3) in enumerate(masters):
        cons = rng.integers(0, 21, len(qa)) if qi == 4 else None                       # one query whose consensus letters differ from its query letters
        entries.append((_entry(rng, mA, qa, cons, spoil_first=qi == NAMED_QUERY), _entry(rng, m3, q3, cons, spoil_first=qi == NAMED_QUERY)))
    targets, kinds = [], []

    def add(pair, kind):
        a, s = pair
        assert 1 <= len(a) == len(s) <= 1025 and (len(a) <= 420 or kind == "identity"), (kind, len(a))
        targets.append((np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8))); kinds.append(kind)
        return len(targets) - 1

    randoms = [add(_rand(rng, L), "random") for L in RANDOM_LENGTHS]
    kinds[randoms[0]] = "col"                                                          # the 1-residue target
    lists, identity = [], []
    for qi, (qa, q3) in enumerate(masters):
        L = len(qa)
        own = [add((qa, q3), "identity")]
        identity.append(own[0])
        longest = min(L, 300)

        def stretch(n, at=None, p=None):
            at = int(rng.integers(0, L - n + 1)) if at is None else at
            return at, _mutate(rng, qa[at:at + n], q3[at:at + n], float(rng.choice([0.05, 0.15, 0.3])) if p is None else p)

        for j in range(N_PIECES[qi]):
            n = max(8, int(longest * rng.uniform(0.2, 1.0)))
            own.append(add(_flank(rng, *stretch(n)[1]), "piece"))
        own.append(add(targets[own[2]], "dup"))
        own.append(add(_cat(targets[own[3]], _xs(6)), "tail"))
        # the borders of the SW kernels' shapes: a stretch that ends at row b - 1 (a prefix of b rows) and one that ends at row b
        for b in BORDERS:
            for end in (b - 1, b):
                if end < L and not (end == L - 1):                                     # the identity target already ends at row L - 1
                    n = min(end + 1, 120)
                    a, s = qa[end + 1 - n:end + 1].copy(), q3[end + 1 - n:end + 1].copy()
                    la, ls = _rand(rng, int(rng.integers(0, 30)))
                    own.append(add((np.concatenate([la, a]), np.concatenate([ls, s])), "edge"))
        if L >= 33:
            # xhead: the stretch starts at a row >= 3 that is not at the extremes, its first three residues are the master's
            n = max(20, int(longest * 0.5))
            at = int(rng.integers(3, L - n + 1))
            while at % 10 in (0, 8, 9):
                at -= 1
            _, (a, s) = stretch(n, at, 0.1)
            a[:3], s[:3] = qa[at:at + 3], q3[at:at + 3]
            ra, rs = _rand(rng, int(rng.integers(0, 40)))
            own.append(add(_cat(_xs(3), (a, s), (ra, rs)), "xhead"))
            _, (a, s) = stretch(n, None, 0.1)
            a[len(a) // 2:len(a) // 2 + 4] = X; s[len(s) // 2:len(s) // 2 + 4] = X
            own.append(add(_flank(rng, a, s), "xmid"))
        if L >= 129:
            n = min(L, 240)
            g = int(rng.integers(25, 41)) if n >= 200 else 25
            at = int(rng.integers(0, L - n + 1))
            a, s = qa[at:at + n].copy(), q3[at:at + n].copy()
            cut, put = n // 3, 2 * n // 3
            ia, is_ = _rand(rng, g)
            deleted = (np.concatenate([a[:cut], a[cut + g:]]), np.concatenate([s[:cut], s[cut + g:]]))
            inserted = (np.concatenate([a[:put], ia, a[put:]]), np.concatenate([s[:put], is_, s[put:]]))
            both = (np.concatenate([a[:cut], a[cut + g:put], ia, a[put:]]), np.concatenate([s[:cut], s[cut + g:put], is_, s[put:]]))
            for t in (deleted, inserted, both):
                own.append(add(_flank(rng, *t, cap=420), "longgap"))
        # row: one master letter (a row away from the extremes) between X flanks
        at = 5 if L > 5 else 1
        own.append(add(_cat(_xs(3), (qa[at:at + 1], q3[at:at + 1]), _xs(3)), "row"))
        if L >= 33:
            # slot: two master letters, three and four rows apart, one of them on a row at the extremes
            for rows in ([10, 13], [20, 24]):
                own.append(add((qa[rows], q3[rows]), "slot"))
        strangers = [int(x) for x in rng.choice(randoms, size=4, replace=False)]
        if qi in (0, NAMED_QUERY) and randoms[0] not in strangers:
            strangers[0] = randoms[0]
        order = own + strangers
        rng.shuffle(order)
        if L <= 420:
            a, s = _mutate(rng, qa, q3, 0.05)
        else:
            a, s = _mutate(rng, qa[300:400], q3[300:400], 0.05)
        order.append(add((a, s), "near"))
        assert 12 <= len(order) <= 40, (qi, len(order))
        lists.append(np.array(order, np.uint32))
    # the saturating list: 62 a column against any letter, 37200 against 600 of the 1025 residues
    import profile_model as pm
    sat_a, sat_3 = _rand(rng, SAT_LEN)
    entries.append((pm.encode(np.full((20, SAT_LEN), 127, np.int8), sat_a), pm.encode(np.full((20, SAT_LEN), 127, np.int8), sat_3)))
    masters.append((sat_a, sat_3))
    assert len(targets[identity[6]][0]) == 1025 and len(targets[randoms[-1]][0]) == 420
    lists.append(np.array([identity[6], randoms[-1]], np.uint32))
    identity.append(-1)
    keys = np.array([key_of(i) for i in range(len(targets))], np.uint32)
    assert len(set(keys.tolist())) == len(keys) and (np.diff(keys.astype(np.int64)) < 0).any()
    return dict(entries=entries, masters=masters, targets=targets, kinds=kinds, keys=keys, lists=lists, identity=identity)


# ---- the world as databases (the reference binary and fsgpu-modules read these) -----------------------------------------------------------------------------
def write_db(path, entries, dbtype):
    """entries: {key: bytes without the terminator}"""
    blob, index, off = [], [], 0
    for k in sorted(entries):
        body = entries[k] + b"\0"
        index.append(f"{k}\t{off}\t{len(body)}\n")
        blob.append(body)
        off += len(body)
    open(path, "wb").write(b"".join(blob))
    open(path + ".index", "w").write("".join(index))
    open(path + ".dbtype", "wb").write(int(dbtype).to_bytes(4, "little"))


def read_db(path):
    data = open(path, "rb").read()
    out = {}
    for line in open(path + ".index"):
        k, off, ln = line.split()
        out[int(k)] = data[int(off):int(off) + int(ln) - 1]
    return out


def write_world(directory):
    """qprof / qprof_ss (profile databases, key = query index), tdb / tdb_ss / tdb_h (key = key_of(id)), pref (every list in list order)"""
    w = world()
    text = lambda c: ("".join(LETTERS[int(x)] for x in c) + "\n").encode()  # noqa: E731
    p = lambda n: os.path.join(str(directory), n)  # noqa: E731
    write_db(p("qprof"), {q: e[0] for q, e in enumerate(w["entries"])}, 2)
    write_db(p("qprof_ss"), {q: e[1] for q, e in enumerate(w["entries"])}, 2)
    write_db(p("qprof_h"), {q: f"profile{q}\n".encode() for q in range(len(w["entries"]))}, 12)
    write_db(p("tdb"), {int(w["keys"][i]): text(t[0]) for i, t in enumerate(w["targets"])}, 0)
    write_db(p("tdb_ss"), {int(w["keys"][i]): text(t[1]) for i, t in enumerate(w["targets"])}, 0)
    write_db(p("tdb_h"), {int(w["keys"][i]): f"target{i}\n".encode() for i in range(len(w["targets"]))}, 12)
    write_db(p("pref"), {q: "".join(f"{int(w['keys'][int(t)])}\t{100 - min(k, 99)}\t0\n" for k, t in enumerate(l)).encode() for q, l in enumerate(w["lists"])}, 7)


# ---- the live model on this world (generator, and the sample of the CPU test) ---------------------------------------------------------------------------------
class Live:
    """align_model.align_query over profile_model.ProfileWorld, one world per (coverage rule, gap costs); Smith-Waterman records, start cells and banded
    paths are computed once per distinct input (the model's functions, memoised on their arguments' bytes)"""

    def __init__(self):
        import align_model as A
        import profile_model as pm
        self.A, self.pm, self.w = A, pm, world()
        self._worlds, self._sw, self._runs, self._memo = {}, {}, {}, {}
        self.doublings = {}                                # (rectangle bytes ...) -> band doublings of banded_path
        if not getattr(pm.start_cell, "_memoised", False):
            pm.start_cell, pm.banded_path = self._memoise(pm.start_cell), self._memoise(pm.banded_path)

    @staticmethod
    def _memoise(f):
        cache = {}

        def g(*args, **kw):
            if kw:
                return f(*args, **kw)
            k = tuple(np.asarray(a).tobytes() if isinstance(a, np.ndarray) else a for a in args)
            if k not in cache:
                cache[k] = f(*args)
            return cache[k]
        g._memoised = True
        return g

    def model_world(self, P):
        k = (P["covThr"], P["covMode"], P["gapOpen"], P["gapExtend"])
        if k not in self._worlds:
            W = self.pm.ProfileWorld(self.w["targets"], self.w["keys"], P["covThr"], P["covMode"], P["gapOpen"], P["gapExtend"])
            W._sw = self._sw.setdefault(k[2:], {})
            W.letters = [W.add_query(*e) for e in self.w["entries"]]
            self._worlds[k] = W
        return self._worlds[k]

    def query(self, q, P, identity=None):
        ident = self.w["identity"][q] if identity is None else identity
        k = (q, ident, tuple(sorted(P.items())))
        if k not in self._runs:
            W = self.model_world(P)
            qa, q3 = W.letters[q]
            if q == SAT_QUERY or q == 6:                   # the entries' query letters name the tables: two queries never share them
                assert W.query(qa, q3)["key"] == (bytes(self.w["entries"][q][0]), bytes(self.w["entries"][q][1]))
            self._runs[k] = self.A.align_query(W, qa, q3, self.w["lists"][q], {x: P[x] for x in self.A.DEFAULTS}, identity=ident)
        return self._runs[k]

    def run(self, P, identity=None):
        return [self.query(q, P, identity) for q in range(len(self.w["entries"]))]

    def evalue_fwd(self, q, pos):
        P = params()
        W = self.model_world(P)
        return W.evalue(W.query(*W.letters[q]), int(self.query(q, P).fwd[pos]["score"]))


def derive(live):
    """-> {name: params dict}.  Every threshold is read off a record of the model and stored as the exact number (float32 / double)."""
    W = world()
    Q = NAMED_QUERY
    sets = {"default": params()}
    base = live.run(sets["default"])
    r = base[Q]
    kind = lambda i: W["kinds"][int(W["lists"][Q][r.hit_of_record[i]])]  # noqa: E731
    acc = [i for i in range(len(r.records)) if kind(i) in ("piece", "xmid", "longgap", "edge") and r.cigars[i]]
    assert len(acc) >= 8, len(acc)
    by = lambda f: sorted(acc, key=lambda i: (f(r.records[i]), i))[len(acc) // 2]  # noqa: E731  the median hit by that value
    # e-values: a hit's difference e-value and its forward e-value as exact doubles, and the next double below each
    i = by(lambda x: x["eval"])
    ev = float(r.records[i]["eval"])
    sets["ediff_eq"], sets["ediff_below"] = params(evalThr=ev), params(evalThr=_next(ev, False, np.float64))
    ef = float(live.evalue_fwd(Q, r.hit_of_record[i]))
    sets["efwd_eq"], sets["efwd_below"] = params(evalThr=ef), params(evalThr=_next(ef, False, np.float64))
    # coverage modes 0, 1, 2 at the start-to-end coverage of a named accepted hit: AT it the hit keeps its cigar, one float above it loses cigar and place
    for mode, f in ((0, lambda x: min(x["qcov"], x["dbcov"])), (1, lambda x: x["dbcov"]), (2, lambda x: x["qcov"])):
        thr = float(f(r.records[by(f)]))
        sets[f"cov{mode}_eq"] = params(covMode=mode, covThr=thr)
        sets[f"cov{mode}_next"] = params(covMode=mode, covThr=_next(thr))
    # the same at the coverage of the IDENTITY hit (below 1: position 0 of the named query scores its own letter at the minimum): one float above, the hit
    # has no cigar, fails checkCriteria's coverage test -- and is accepted as the identity: a record with a start cell and an empty cigar
    ident = [i for i in range(len(r.records)) if int(W["lists"][Q][r.hit_of_record[i]]) == W["identity"][Q]][0]
    for mode, f in ((0, lambda x: min(x["qcov"], x["dbcov"])), (1, lambda x: x["dbcov"]), (2, lambda x: x["qcov"])):
        thr = float(f(r.records[ident]))
        assert thr < 1.0
        sets[f"covi{mode}_eq"] = params(covMode=mode, covThr=thr)
        sets[f"covi{mode}_next"] = params(covMode=mode, covThr=_next(thr))
    # sequence identity under each mode: identities are counted against the AA profile's query letters
    for mode in (0, 1, 2):
        rm = live.run(params(seqIdMode=mode))[Q]
        assert rm.hit_of_record == r.hit_of_record
        thr = float(rm.records[by(lambda x: x["seqId"])]["seqId"])
        assert thr > 0
        sets[f"sid{mode}_eq"] = params(seqIdMode=mode, seqIdThr=thr)
        sets[f"sid{mode}_next"] = params(seqIdMode=mode, seqIdThr=_next(thr))
    ln = int(r.records[by(lambda x: x["alnLength"])]["alnLength"])
    sets["len_eq"], sets["len_next"] = params(alnLenThr=ln), params(alnLenThr=ln + 1)
    # accept / reject limits on top of a coverage gate one float above the named hit: the first of the three modes under which, in some list, a hit that
    # lost its cigar is counted before the limit cuts the list short
    for name, limit, cut in (("acc3", dict(maxAccept=3), "not reached: max-accept"), ("rej2", dict(maxRejected=2), "not reached: max-rejected")):
        for mode in (0, 1, 2):
            P = params(covMode=mode, covThr=sets[f"cov{mode}_next"]["covThr"], **limit)
            outs = [x.outcomes for x in live.run(P)]
            if any("start coverage" in o and cut in o and o.index("start coverage") < o.index(cut) for o in outs):
                sets[name] = P
                break
        assert name in sets, name
    sets["no_bt"] = params(addBacktrace=0)
    sets["gap8_2"] = params(gapOpen=8, gapExtend=2)
    # every listed pair through the reverse pass and the banded trace-back, the single cells (row, col) and the unrelated targets included
    sets["e_all"] = params(evalThr=1e300)
    return sets


# ---- the frozen answers -----------------------------------------------------------------------------------------------------------------------------------------
def _hex(p):
    return {k: (float(v).hex() if isinstance(v, float) else int(v)) for k, v in p.items()}


def _unhex(p):
    return {k: (float.fromhex(v) if isinstance(v, str) else int(v)) for k, v in p.items()}


def save(sets, answers, facts):
    """answers: {set name: [Result per query]}.  Records and CIGARs go into one pool of distinct (record, CIGAR) pairs; per set: the pool indices of the
    records in order, records per query, the outcome code of every hit, forward and reversed SW records, the looked-at count per query.
    facts: what the generator measured on the model for the world conditions (band doublings per hit, the xhead ties)"""
    import align_model as A
    os.makedirs(GOLD, exist_ok=True)
    pool, recs, cigs, arrays, meta = {}, [], [], {}, {}
    arrays["n"] = np.array([len(r.fwd) for r in answers["default"]], np.int32)
    for name, res in answers.items():
        idx = []
        for r in res:
            for rec, cig in zip(r.records, r.cigars):
                k = (rec.tobytes(), cig)
                if k not in pool:
                    pool[k] = len(recs); recs.append(rec); cigs.append(cig)
                idx.append(pool[k])
        arrays[f"{name}/idx"] = np.array(idx, np.int32)
        arrays[f"{name}/nrec"] = np.array([len(r.records) for r in res], np.int32)
        arrays[f"{name}/hit"] = np.array([k for r in res for k in r.hit_of_record], np.int32)
        arrays[f"{name}/out"] = np.array([A.OUTCOMES.index(o) for r in res for o in r.outcomes], np.uint8)
        arrays[f"{name}/fwd"] = np.concatenate([r.fwd for r in res]).view(np.int32).reshape(-1, 4)
        arrays[f"{name}/rev"] = np.concatenate([r.rev for r in res]).view(np.int32).reshape(-1, 4)
        arrays[f"{name}/looked"] = np.array([r.reversed for r in res], np.int32)
        meta[name] = dict(params=_hex(sets[name]))
    arrays["pool"] = np.array(recs, A.REC_DT) if recs else np.zeros(0, A.REC_DT)
    arrays["cigars"] = np.frombuffer("\n".join(cigs).encode(), np.uint8)
    np.savez_compressed(os.path.join(GOLD, "answers.npz"), **arrays)
    json.dump(dict(seed=SEED, outcomes=list(A.OUTCOMES), sets=meta, facts=facts), open(os.path.join(GOLD, "sets.json"), "w"), indent=0, sort_keys=True)


class Frozen:
    """the frozen answers"""

    def __init__(self):
        j = json.load(open(os.path.join(GOLD, "sets.json")))
        assert j["seed"] == SEED, "the world changed: run tests/golden/make_profile_align_golden.py"
        self.outcome_names = j["outcomes"]
        self.meta = j["sets"]
        self.facts = j["facts"]
        self.names = list(self.meta)
        z = np.load(os.path.join(GOLD, "answers.npz"))
        self.z = {k: z[k] for k in z.files}
        self.cigars = bytes(self.z["cigars"]).decode().split("\n")
        self.n = [int(x) for x in self.z["n"]]
        assert self.n == [len(x) for x in world()["lists"]]
        self.off = np.concatenate([[0], np.cumsum(self.n)])

    def params(self, name):
        return _unhex(self.meta[name]["params"])

    def fwd(self, name, q=None):
        return self.z[f"{name}/fwd"] if q is None else self.z[f"{name}/fwd"][self.off[q]:self.off[q + 1]]

    def rev(self, name, q=None):
        return self.z[f"{name}/rev"] if q is None else self.z[f"{name}/rev"][self.off[q]:self.off[q + 1]]

    def selection(self, name, q=None):
        """the reverse selection: pairs whose reversed record the reference computes if its loop reaches them"""
        return int((self.rev(name, q)[:, 3] != 0).sum())

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


# ---- the world's conditions: what it must contain to do its job -----------------------------------------------------------------------------------------------------
def tables(q):
    """(AA profile, 3Di profile) int64 [21, L] of query q, (AA query letters)"""
    import profile_model as pm
    ea, e3 = world()["entries"][q]
    ca, _, aF, _ = pm.decode(ea)
    _, _, sF, _ = pm.decode(e3)
    return aF.astype(np.int64), sF.astype(np.int64), ca


def rectangle(q, target, rec):
    """the substitution scores int64 [qLen, dbLen] of a record's rectangle [qStart, qEnd] x [dbStart, dbEnd]"""
    aF, sF, _ = tables(q)
    ta, t3 = world()["targets"][target]
    qs, qe, ds, de = (int(rec[k]) for k in ("qStartPos", "qEndPos", "dbStartPos", "dbEndPos"))
    return sF[:, qs:qe + 1][t3[ds:de + 1].astype(np.int64)].T + aF[:, qs:qe + 1][ta[ds:de + 1].astype(np.int64)].T


def reverse_matrix(q, target, q_end, db_end, go=10, ge=1):
    """H of the reverse pass, every cell, in plain integers: H[i][j] for reversed prefix row i (query row q_end - i) and column j (target column db_end - j)"""
    aF, sF, _ = tables(q)
    ta, t3 = world()["targets"][target]
    s = (sF[:, :q_end + 1][t3[:db_end + 1].astype(np.int64)].T + aF[:, :q_end + 1][ta[:db_end + 1].astype(np.int64)].T)[::-1, ::-1]
    n, m = s.shape
    H = np.zeros((n, m), np.int64)
    up_h, up_f = [0] * m, [0] * m
    for i in range(n):
        row, e, left, diag = [0] * m, 0, 0, 0
        for j in range(m):
            f = max(up_h[j] - go, up_f[j] - ge) if i else 0
            e = max(left - go, e - ge) if j else 0
            h = max(0, (diag if i and j else 0) + int(s[i, j]), e, f)
            diag = up_h[j]
            up_f[j] = f
            row[j] = left = h
        up_h = row
        H[i] = row
    return H


def compress(ops):
    out, k = "", 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out += f"{e - k}{ops[k]}"
        k = e
    return out


def measure_facts(F):
    """what the conditions need from the model's functions, measured on the frozen records of the default set:
    doublings [[query, hit, band widths that were too narrow]], xhead [[query, hit, qStart, dbStart, cells of the reverse matrix that reach the score]]"""
    import profile_model as pm
    w = world()
    doublings, xhead = [], []
    for q in range(len(F.n)):
        recs, cigars, hits = F.records("default", q)
        for rec, cig, k in zip(recs, cigars, hits):
            t = int(w["lists"][q][k])
            score, q_end, db_end, _ = (int(x) for x in F.fwd("default", q)[k])
            if cig:
                m = rectangle(q, t, rec)
                widths = []
                path = pm.banded_path(m, m.shape[0], m.shape[1], score, doublings=widths)
                assert compress(path) == cig, (q, k)
                if widths:
                    doublings.append([q, int(k), widths])
            if w["kinds"][t] == "xhead":
                H = reverse_matrix(q, t, q_end, db_end)
                assert int(H.max()) == score
                cells = np.argwhere(H == score)
                col = cells[:, 1].min()                                                # the first column that reaches the score, then the smallest row
                row = cells[cells[:, 1] == col][:, 0].min()
                assert (q_end - int(row), db_end - int(col)) == (int(rec["qStartPos"]), int(rec["dbStartPos"])), (q, k)
                xhead.append([q, int(k), int(rec["qStartPos"]), int(rec["dbStartPos"]), [[q_end - int(i), db_end - int(j)] for i, j in cells]])
    return dict(doublings=doublings, xhead=xhead)


def conditions(F):
    """asserted by the generator on what it wrote and by tests/test_profile_cases.py on the frozen files"""
    w = world()
    same = lambda a, b: all(F.records(a, q)[0].tobytes() == F.records(b, q)[0].tobytes() and F.records(a, q)[1] == F.records(b, q)[1] for q in range(len(F.n)))  # noqa: E731
    pairs = [(n, n[:-3] + s) for n in F.names if n.endswith("_eq") for s in ("_next", "_below") if n[:-3] + s in F.names]
    assert len(pairs) == 12, pairs
    for a, b in pairs:
        if a == "efwd_eq":                                 # the named hit fails the e-value of the difference either way: what changes is the reverse selection
            assert same(a, b) and F.selection(b) == F.selection(a) - 1 and F.looked(b).sum() == F.looked(a).sum() - 1
        else:
            assert not same(a, b), (a, b, "the step beyond the threshold changes nothing")
    # a hit that loses its cigar fails checkCriteria's own coverage test, which reads the same start-to-end coverage: only the identity hit stays in the
    # result.  The covi sets name the identity hit's coverage; one float above it, its record has a start cell and no cigar
    for mode in (0, 1, 2):
        recs, cigars, hits = F.records(f"covi{mode}_next", NAMED_QUERY)
        bare = [i for i in range(len(recs)) if not cigars[i] and recs[i]["qStartPos"] >= 0 and recs[i]["dbStartPos"] >= 0]
        assert bare and all(int(w["lists"][NAMED_QUERY][hits[i]]) == w["identity"][NAMED_QUERY] for i in bare), mode
        assert F.outcomes(f"covi{mode}_next", NAMED_QUERY)[int(hits[bare[0]])] == "accepted as identity"
        recs, cigars, _ = F.records(f"covi{mode}_eq", NAMED_QUERY)
        assert len(recs) and all(cigars)
        # the ordinary gate one float above a hit's coverage: that hit (and any other of exactly its coverage) is rejected by the start coverage, having lost its cigar
        moved = [k for k, (a, b) in enumerate(zip(F.outcomes(f"cov{mode}_eq", NAMED_QUERY), F.outcomes(f"cov{mode}_next", NAMED_QUERY))) if (a, b) == ("accepted", "start coverage")]
        assert moved, mode
    all_cigars = [c for q in range(len(F.n)) for c in F.records("default", q)[1]]
    assert sum("I" in c and "D" in c for c in all_cigars) >= 10
    assert len(F.facts["doublings"]) >= 3, F.facts["doublings"]
    assert {w["kinds"][int(w["lists"][q][k])] for q, k, _ in F.facts["doublings"]} >= {"longgap"}
    # xhead: the start cell excludes the X columns although the cell one column and one row before it reaches the score as well
    xh = [(q, k) for q in range(len(F.n)) for k, t in enumerate(w["lists"][q]) if w["kinds"][int(t)] == "xhead"]
    assert len(F.facts["xhead"]) >= 4 and {(q, k) for q, k, *_ in F.facts["xhead"]} <= set(xh)
    for q, k, qs, ds, cells in F.facts["xhead"]:
        t3 = w["targets"][int(w["lists"][q][k])][1]
        assert ds == 3 and t3[ds] != X and t3[ds - 1] == X and [qs - 1, ds - 1] in cells and [qs, ds] in cells, (q, k, qs, ds)
    # rectangle heights on both sides of the shape borders, and the reverse pass's prefix lengths AT them
    heights, prefixes = set(), set()
    for q in range(len(F.n)):
        recs, cigars, _ = F.records("default", q)
        heights |= {int(r["qEndPos"]) - int(r["qStartPos"]) + 1 for r in recs}
        prefixes |= {int(r["qEndPos"]) + 1 for r in recs}
    for b in (16, 32, 512):
        assert any(h <= b for h in heights) and any(h > b for h in heights), b
    assert {16, 17, 32, 33, 512, 513, 1024, 1025} <= prefixes, sorted(prefixes)
    # the saturating list: the int32 re-run decides both passes of the pair against the 1025-residue target
    for name in ("default", "e_all"):
        f, r = F.fwd(name, SAT_QUERY), F.rev(name, SAT_QUERY)
        assert f[0, 3] == 2 and r[0, 3] == 2 and f[0, 0] == r[0, 0] == 62 * SAT_LEN == 37200 and f[1, 3] == 1, (f, r)
    recs, cigars, _ = F.records("e_all", SAT_QUERY)
    assert len(recs) == 2 and f"{SAT_LEN}M" in cigars
    # the limits: a hit that lost its cigar is among the counted ones, and the limit cuts lists short
    for name, cut in (("acc3", "not reached: max-accept"), ("rej2", "not reached: max-rejected")):
        outs = [F.outcomes(name, q) for q in range(len(F.n))]
        assert any("start coverage" in o and cut in o and o.index("start coverage") < o.index(cut) for o in outs), name
    # every pair of e_all is backtraced, the single cells included
    for q in range(len(F.n)):
        recs, cigars, hits = F.records("e_all", q)
        assert len(recs) == F.n[q] and all(cigars)
        for r, c, k in zip(recs, cigars, hits):
            if w["kinds"][int(w["lists"][q][k])] in ("row", "col") and q < SAT_QUERY:
                assert c == "1M" and r["qStartPos"] == r["qEndPos"] and r["dbStartPos"] == r["dbEndPos"], (q, k, c)
    assert F.params("gap8_2")["gapOpen"] == 8 and F.params("no_bt")["addBacktrace"] == 0

"""structurealign's accept loop stated a second time, in plain Python / numpy -- written from the reference's text alone (F = foldseek/src, M = lib/mmseqs/src):
F/strucclustutils/structurealign.cpp (alignStructure :37-112, computeAlternativeAlignment :115-138, the per-query loop :343-452, compareHitsByStructureBits
:21-29), M/alignment/Alignment.cpp:548-567 (checkCriteria), M/commons/Util.cpp:542-607 (canBeCovered, hasCoverage, computeSeqId), M/commons/Util.h:396-398
(hasAlignmentLength), M/alignment/Matcher.cpp:158-160 (computeAlnLength), M/alignment/Matcher.h:161-172 (compareHits), M/alignment/Matcher.cpp:282-329
(resultToBuffer), F/commons/StructureSmithWaterman.cpp:358-359, :369-523, :2028-2030 (end-based coverage, alignStartPosBacktraceBlock, computeCov).
It shares no code with foldseek_amd/csrc/host/search.cpp and imports nothing from foldseek_amd.  TEST INFRASTRUCTURE.

Its ingredients are the models the suite already pins: Smith-Waterman records from tests/sw_model.py (forward, reversed query, and the explicit X-masked
target of --alt-ali), start cell / CIGAR / identical count from tests/ba_model.py, mu / lambda / corrected e-value and the composition biases from the
oracle's C restatement (oracle/libfso.so), per-hit LDDT averages and TM-scores from callbacks (tests/lddt_model.py, tests/tm_model.py or their frozen
answers).

Arithmetic types follow the source: coverage and sequence identity are float (np.float32), the e-value is a double, the first e-value reads the forward
score as the unsigned it is stored in (:55, s_align.score1 is uint32_t), the second one reads the int32 difference (:69-70), structure bits are
(int)(score * sqrt(lddt * tm)) with the product taken in double (:409).

Per query the model returns a Result: the ordered records with their CIGARs, the forward and reversed SW record of every listed pair as the loop leaves
them (reversed all zero for a pair the reference would not reverse even if its loop reached it), how many pairs had their reversed score looked at, and for every hit of the list the
outcome that ended it (OUTCOMES); alt_ends lists, per accepted hit of an --alt-ali run, (hit, alternatives found, what ended the search for more)."""
import collections
import ctypes as C
import math
import os

import numpy as np

import ba_model
import helpers
import sw_model

LETTERS = "ACDEFGHIKLMNPQRSTVWYX"
X = 20
INT_MAX = 2147483647
# M/commons/Parameters.h:284-294
COV_BIDIRECTIONAL, COV_TARGET, COV_QUERY, COV_LENGTH_QUERY, COV_LENGTH_TARGET, COV_LENGTH_SHORTER = 0, 1, 2, 3, 4, 5
SEQ_ID_ALN_LEN, SEQ_ID_SHORT, SEQ_ID_LONG = 0, 1, 2
OUTCOMES = ("not coverable", "end coverage", "e-value fwd", "e-value diff", "seq id", "start coverage", "aln length", "accepted", "accepted as identity",
            "tm drop", "lddt drop", "not reached: max-accept", "not reached: max-rejected", "e-value crit")
# "e-value crit": checkCriteria's own res.eval <= evalThr can never fail after alignStructure's identical test (:71) passed; the name exists so that the
# model can say so (it asserts that the count stays 0)

REC_DT = np.dtype([("dbKey", np.uint32), ("score", np.int32), ("qcov", np.float32), ("dbcov", np.float32), ("seqId", np.float32), ("eval", np.float64),
                   ("alnLength", np.uint32), ("qStartPos", np.int32), ("qEndPos", np.int32), ("qLen", np.uint32), ("dbStartPos", np.int32),
                   ("dbEndPos", np.int32), ("dbLen", np.uint32)])
Result = collections.namedtuple("Result", "records cigars fwd rev reversed outcomes hit_of_record alt_ends")
ALT_ENDS = ("end coverage", "e-value fwd", "e-value diff", "criteria", "count reached")

DEFAULTS = dict(evalThr=10.0, covThr=0.0, covMode=0, seqIdThr=0.0, seqIdMode=0, alnLenThr=0, maxAccept=INT_MAX, maxRejected=INT_MAX, altAlignment=0,
                tmThr=0.0, tmMode=0, lddtThr=0.0, structureBits=0)


def params(**kw):
    p = dict(DEFAULTS)
    assert all(k in p for k in kw), kw
    p.update(kw)
    return p


# ---- the small functions, each as its source line states it ------------------------------------------------------------------------------------------------
def f32(x):
    return np.float32(x)


def compute_cov(start, end, length):
    """StructureSmithWaterman.cpp:2028-2030, unsigned operands, float division"""
    return f32(min(length, max(start, end)) - min(start, end) + 1) / f32(length)


def can_be_covered(cov_thr, cov_mode, q_len, t_len):
    """Util.cpp:542-559: float lengths, float threshold; the literal 1.0 is a double, a float ratio converts to it exactly"""
    c, q, t = f32(cov_thr), f32(q_len), f32(t_len)
    if cov_mode == COV_BIDIRECTIONAL:
        return bool(q / t >= c and t / q >= c)
    if cov_mode == COV_QUERY:
        return bool(t / q >= c)
    if cov_mode == COV_TARGET:
        return bool(q / t >= c)
    if cov_mode == 3:
        return bool(t / q >= c and t / q <= 1.0)
    if cov_mode == 4:
        return bool(q / t >= c and q / t <= 1.0)
    if cov_mode == 5:
        return bool(min(t, q) / max(t, q) >= c)
    return True


def has_coverage(cov_thr, cov_mode, q_cov, t_cov):
    """Util.cpp:561-576"""
    c = f32(cov_thr)
    if cov_mode == COV_BIDIRECTIONAL:
        return bool(f32(q_cov) >= c and f32(t_cov) >= c)
    if cov_mode == COV_QUERY:
        return bool(f32(q_cov) >= c)
    if cov_mode == COV_TARGET:
        return bool(f32(t_cov) >= c)
    return True


def compute_seq_id(mode, ids, q_len, t_len, aln_len):
    """Util.cpp:597-607"""
    if mode == SEQ_ID_SHORT:
        return f32(ids) / f32(min(q_len, t_len))
    if mode == SEQ_ID_LONG:
        return f32(ids) / f32(max(q_len, t_len))
    if mode == SEQ_ID_ALN_LEN:
        return f32(ids) / f32(aln_len)
    return f32(0.0)


def compute_aln_length(q_start, q_end, db_start, db_end):
    """Matcher.cpp:158-160"""
    return max(abs(q_end - q_start), abs(db_end - db_start)) + 1


def criteria(rec, P):
    """Alignment.cpp:549-552: the four tests of checkCriteria, in the order (evalOk, seqIdOK, covOK, alnLenOK).  seqIdThr is a double there: the float
    identity converts exactly.  covOK reads res.qcov / res.dbcov, which the block aligner's caller computed from the START cell (:521-522)."""
    return (float(rec["eval"]) <= float(P["evalThr"]), float(rec["seqId"]) >= float(P["seqIdThr"]),
            has_coverage(P["covThr"], P["covMode"], rec["qcov"], rec["dbcov"]), int(rec["alnLength"]) >= int(P["alnLenThr"]))


def compare_hits(a, b):
    """Matcher.h:161-172 as a three-way comparison"""
    for k, sign in (("eval", 1), ("score", -1), ("dbLen", 1), ("dbKey", 1)):
        if a[k] != b[k]:
            return sign if a[k] > b[k] else -sign
    return 0


def compare_structure_bits(a, b):
    """structurealign.cpp:21-29"""
    for k, sign in (("score", -1), ("dbLen", 1), ("dbKey", 1)):
        if a[k] != b[k]:
            return sign if a[k] > b[k] else -sign
    return 0


def compress(ops):
    """Matcher::compressAlignment: run-length text of a backtrace"""
    out, k = "", 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out += f"{e - k}{ops[k]}"
        k = e
    return out


def seq_id_text(seq_id):
    """Util.cpp:251-280 and the tab that Matcher.cpp:289 writes over the last digit of "1.000" """
    s = f32(seq_id)
    if s == f32(1.0):
        return "1.00"
    out = "0."
    if float(s) < 0.10:
        out += "0"
    if float(s) < 0.01:
        out += "0"
    return out + str(int(s * f32(1000)))


def line(rec, cigar=None):
    """Matcher.cpp:282-329 without the newline; cigar None: -a 0"""
    e = "%.3E" % float(rec["eval"])
    f = [str(int(rec["dbKey"])), str(int(rec["score"])), seq_id_text(rec["seqId"]), e, str(int(rec["qStartPos"])), str(int(rec["qEndPos"])),
         str(int(rec["qLen"])), str(int(rec["dbStartPos"])), str(int(rec["dbEndPos"])), str(int(rec["dbLen"]))]
    if cigar is not None:
        f.append(cigar)
    return "\t".join(f)


# ---- a world: matrices, targets, what the e-value needs ------------------------------------------------------------------------------------------------------
def _score_fn(mat):
    tab = {}
    m = np.asarray(mat).reshape(21, 21)
    for a in range(21):
        for b in range(21):
            v = int(np.clip(m[a, b], -128, 127))
            tab[(LETTERS[a], LETTERS[b])] = v
            tab[(LETTERS[b], LETTERS[a])] = v                 # block_set_aamatrix writes both orders (:428-447): the later call wins
    return lambda x, y: tab[(x, y)]


class World:
    """alignment_type 2: 3Di + AA (BLOSUM62 at 1.4 bits), 0: 3Di only (aaFactor 0.0, :264: an all-zero AA matrix and, with it, all-zero biases).
    targets: list of (AA codes, 3Di codes); keys[i] the dbKey of target i; residues: getAminoAcidDBSize of the target DB (:290)."""

    def __init__(self, targets, keys=None, alignment_type=2, comp_bias=True, scale=0.5, go=10, ge=1, residues=None):
        self.targets = [(np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8)) for a, s in targets]
        self.keys = np.arange(len(targets), dtype=np.uint32) if keys is None else np.asarray(keys, np.uint32)
        self.atype, self.comp_bias, self.scale, self.go, self.ge = alignment_type, bool(comp_bias), float(scale), int(go), int(ge)
        self.residues = int(sum(len(a) for a, _ in self.targets)) if residues is None else int(residues)
        self.m3 = helpers.o_submat("MAT3DI", 2.1)[0].reshape(21, 21).astype(np.int8)
        self.mA = helpers.o_submat("BLOSUM62", 1.4 if alignment_type == 2 else 0.0)[0].reshape(21, 21).astype(np.int8)
        self.f3, self.fA = _score_fn(self.m3), _score_fn(self.mA)
        nn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foldseek_amd", "data", "evalue_nn.bin")
        self.nn = np.fromfile(nn, dtype=np.uint8)                # the network's weights: a data file
        self.log_residues = float(np.log(float(self.residues)))
        self._sw, self._bt, self._q = {}, {}, {}

    # -- per query: both directions' biases (ssw_init after Sequence::reverse, :344-347), mu and lambda (:343)
    def query(self, qa, q3):
        key = (bytes(qa), bytes(q3))
        if key not in self._q:
            qa, q3 = np.ascontiguousarray(qa, np.uint8), np.ascontiguousarray(q3, np.uint8)
            _, _, cbAf, cb3f = helpers.o_align_profiles(qa, q3, self.atype, self.comp_bias, self.scale)
            _, _, cbAr, cb3r = helpers.o_align_profiles(qa[::-1].copy(), q3[::-1].copy(), self.atype, self.comp_bias, self.scale)
            a, b = C.c_double(), C.c_double()
            helpers.oracle().fso_predict_mu_lambda(self.nn, q3, len(q3), 21, C.byref(a), C.byref(b))
            self._q[key] = dict(qa=qa, q3=q3, cbAf=cbAf, cb3f=cb3f, cbAr=cbAr, cb3r=cb3r, mu_lambda=(a.value, b.value), key=key)
        return self._q[key]

    def evalue(self, q, score):
        return float(helpers.oracle().fso_evalue_corr(float(score), q["mu_lambda"][0], q["mu_lambda"][1], self.log_residues))

    # -- Smith-Waterman records, cached per (query, direction, target bytes); computed for many targets at once
    def sw(self, q, reverse, seqs):
        keys = [(q["key"], reverse, bytes(a), bytes(s)) for a, s in seqs]
        miss = [k for k in range(len(seqs)) if keys[k] not in self._sw]
        if miss:
            cb3, cbA = (q["cb3r"], q["cbAr"]) if reverse else (q["cb3f"], q["cbAf"])
            recs = sw_model.align(self.m3, self.mA, q["q3"], q["qa"], cb3, cbA, reverse, [seqs[k][1] for k in miss], [seqs[k][0] for k in miss], self.go, self.ge)
            for k, r in zip(miss, recs):
                self._sw[keys[k]] = (int(r["score"]), int(r["qEnd"]), int(r["dbEnd"]), int(r["word"]))
        return [self._sw[k] for k in keys]

    # -- alignStartPosBacktraceBlock (:369-523) through the block aligner's model
    def block(self, q, ta, t3, q_end, db_end, target_score):
        """-> (ok, qStart, dbStart, identical, backtrace in forward order)"""
        key = (q["key"], bytes(ta[:db_end + 1]), bytes(t3[:db_end + 1]), q_end, target_score)
        if key in self._bt:
            return self._bt[key]
        let = lambda x: [LETTERS[int(c)] for c in x]  # noqa: E731
        n = q_end + 1
        # :394-405: the reversed query read from L - (qEnd + 1) on, i.e. the prefix 0..qEnd backwards, with the sum of the two biases
        rqa, rq3 = let(q["qa"][:n][::-1]), let(q["q3"][:n][::-1])
        rbias = [int(a) + int(b) for a, b in zip(q["cbAf"][:n][::-1], q["cb3f"][:n][::-1])]
        rta, rt3 = let(ta[:db_end + 1][::-1]), let(t3[:db_end + 1][::-1])                 # :413-420
        res, ms, model = (-1000000000, -1, -1), 32, None
        while ms <= 4096 and res[0] < target_score:                                      # :458-469
            model = ba_model.BlockModel(rqa, rta, self.fA, -self.go, -self.ge, ms, 4096, x_drop=-(ms * (-self.ge) + (-self.go)), q_bias=rbias,
                                        r_bias=[0] * len(rta), score2=self.f3, q2=rq3, r2=rt3)
            res = model.align()
            ms *= 2
        if res[0] != target_score and not (target_score == 32767 and res[0] >= target_score):      # :474-477
            out = (False, -1, -1, 0, "")
        else:
            ops = btrace_expand(model.trace.cigar(res[1], res[2]))
            qpos = tpos = ids = 0
            for op in ops:                                                                # :495-514
                if op == "M":
                    ids += rqa[qpos] == rta[tpos]; qpos += 1; tpos += 1
                elif op == "I":
                    qpos += 1
                else:
                    tpos += 1
            out = (True, (q_end + 1) - qpos, (db_end + 1) - tpos, ids, ops[::-1])        # :515-519
        self._bt[key] = out
        return out


def btrace_expand(cigar):
    ops, n = "", ""
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            ops += ch * int(n); n = ""
    return ops


# ---- alignStructure (:37-112) -------------------------------------------------------------------------------------------------------------------------------
def align_structure(W, q, ta, t3, key, P, fwd, rev_of):
    """fwd: the forward record (score, qEnd, dbEnd, word); rev_of(): the reversed record, asked for only where the source computes it.
    -> (reason or None, record or None, backtrace, reversed record or None)"""
    L, T = len(q["q3"]), len(t3)
    score1, q_end, db_end, _ = fwd
    q_cov, t_cov = compute_cov(0, q_end, L), compute_cov(0, db_end, T)                   # StructureSmithWaterman.cpp:358-359
    if not has_coverage(P["covThr"], P["covMode"], q_cov, t_cov):                        # :50-53
        return "end coverage", None, "", None
    if W.evalue(q, score1 & 0xFFFFFFFF) > P["evalThr"]:                                 # :55-59
        return "e-value fwd", None, "", None
    rev = rev_of()                                                                       # :65-67
    score = int(np.int32(score1)) - int(np.int32(rev[0]))                                # :69
    ev = W.evalue(q, score)
    if ev > P["evalThr"]:                                                                # :70-74
        return "e-value diff", None, "", rev
    ok, qs, ds, ids, bt = W.block(q, ta, t3, q_end, db_end, score1)                      # :77-89 (never a profile search here)
    # :83 tests the caller's own copy of `align`, which alignStartPosBacktraceBlock (by value) never touches: a failed block alignment is NOT redone by
    # alignStartPosBacktrace, its record keeps the start cells -1, an empty backtrace and the END-based coverage
    if ok:
        q_cov, t_cov = compute_cov(qs, q_end, L), compute_cov(ds, db_end, T)             # StructureSmithWaterman.cpp:521-522
    aln_len = compute_aln_length(qs, q_end, ds, db_end)                                  # :103
    seq_id = f32(0.0)
    if len(bt) > 0:                                                                      # :104-107
        aln_len = len(bt)
        seq_id = compute_seq_id(P["seqIdMode"], ids, L, T, aln_len)
    rec = np.zeros(1, REC_DT)[0]
    rec["dbKey"], rec["score"], rec["qcov"], rec["dbcov"], rec["seqId"], rec["eval"], rec["alnLength"] = key, score, q_cov, t_cov, seq_id, ev, aln_len
    rec["qStartPos"], rec["qEndPos"], rec["qLen"], rec["dbStartPos"], rec["dbEndPos"], rec["dbLen"] = qs, q_end, L, ds, db_end, T
    return None, rec, bt, rev


# ---- the per-query loop (:343-452) ------------------------------------------------------------------------------------------------------------------------------
def align_query(W, qa, q3, hits, P, identity=-1, lddt=None, tm=None):
    """hits: target indices in list order; identity: the target index that is the query itself (isIdentity, :356) or -1.
    lddt(hit index, record, backtrace) -> avgLddtScore (float), tm(...) -> tmscore (double): needed when a threshold or structureBits is set."""
    import functools
    q = W.query(qa, q3)
    hits = [int(h) for h in hits]
    seqs = [W.targets[h] for h in hits]
    fwd = W.sw(q, False, seqs)
    need_tm = P["tmThr"] > 0 or P["structureBits"]
    need_lddt = P["lddtThr"] > 0 or P["structureBits"]
    fwd_out, rev_out = np.zeros(len(hits), sw_model.REC_DT), np.zeros(len(hits), sw_model.REC_DT)
    for k, r in enumerate(fwd):
        fwd_out[k] = r
    # the pairs whose reversed score the loop reads IF it reaches them (:50-67: coverable, end coverage, forward e-value -- none depends on the hits before):
    # their reversed records are computed in one go; `reversed` below counts the ones the loop did reach
    sel = [k for k in range(len(hits)) if can_be_covered(P["covThr"], P["covMode"], len(q3), len(seqs[k][1]))
           and has_coverage(P["covThr"], P["covMode"], compute_cov(0, fwd[k][1], len(q3)), compute_cov(0, fwd[k][2], len(seqs[k][1])))
           and not W.evalue(q, fwd[k][0] & 0xFFFFFFFF) > P["evalThr"]]
    for k, r in zip(sel, W.sw(q, True, [seqs[k] for k in sel])):
        rev_out[k] = r
    outcomes, results, reversed_, alt_ends = [], [], 0, []
    passed = rejected = 0
    for k, h in enumerate(hits):
        if not passed < P["maxAccept"]:                                                  # :350
            outcomes.append("not reached: max-accept"); continue
        if not rejected < P["maxRejected"]:
            outcomes.append("not reached: max-rejected"); continue
        ta, t3 = (x.copy() for x in seqs[k])                                             # tSeq*.mapSequence (:362-363): a fresh copy per hit
        T = len(t3)
        is_identity = h == identity
        if not can_be_covered(P["covThr"], P["covMode"], len(q3), T):                    # :364-367
            rejected += 1; outcomes.append("not coverable"); continue
        reason, rec, bt, rev = align_structure(W, q, ta, t3, W.keys[h], P, fwd[k], lambda: W.sw(q, True, [seqs[k]])[0])
        if rev is not None:
            assert k in sel and tuple(rev_out[k]) == tuple(rev)
            reversed_ += 1
        if reason is not None:                                                           # :369-374
            rejected += 1; outcomes.append(reason); continue
        c = criteria(rec, P)
        if not (is_identity or all(c)):                                                  # :376, :432-434
            rejected += 1
            outcomes.append(("e-value crit", "seq id", "start coverage", "aln length")[c.index(False)])
            continue
        if need_tm or need_lddt:                                                         # :377-411
            tm_score = lddt_avg = None
            if need_tm:
                tm_score = float(tm(k, rec, bt))
                if tm_score < float(f32(P["tmThr"])):                                                # :393-395: neither accepted nor rejected
                    outcomes.append("tm drop"); continue
            if need_lddt:
                lddt_avg = f32(lddt(k, rec, bt))
                if float(lddt_avg) < float(f32(P["lddtThr"])):                           # :403-405 (par.lddtThr is a float)
                    outcomes.append("lddt drop"); continue
                rec["dbcov"] = lddt_avg                                                  # :406
            if P["structureBits"]:                                                       # :408-410: int * double -> int
                rec["score"] = int(float(int(rec["score"])) * math.sqrt(float(lddt_avg) * tm_score))
        results.append((rec, bt, k))                                                     # :414
        outcomes.append("accepted" if all(c) else "accepted as identity")
        alt, prev = P["altAlignment"], rec
        while alt:                                                                       # :415-429
            for pos in range(int(prev["dbStartPos"]), int(prev["dbEndPos"])):            # :124-127: dbEndPos itself stays unmasked; a start of -1 wraps
                ta[pos] = X; t3[pos] = X                                                 # (a failed block alignment) and is not produced here
            assert prev["dbStartPos"] >= 0
            f2 = W.sw(q, False, [(ta, t3)])[0]
            reason, arec, abt, _ = align_structure(W, q, ta, t3, W.keys[h], P, f2, lambda: W.sw(q, True, [(ta, t3)])[0])
            if reason is not None or not all(criteria(arec, P)):                         # :128-137: isIdentity false
                alt_ends.append((k, P["altAlignment"] - alt, reason or "criteria"))
                break
            results.append((arec, abt, k))
            prev = arec
            alt -= 1
            if alt == 0:
                alt_ends.append((k, P["altAlignment"], "count reached"))
        passed += 1                                                                      # :430-431
        rejected = 0
    cmp_ = compare_structure_bits if P["structureBits"] else compare_hits
    if len(results) > 1:                                                                 # :439-445 (a strict weak order whose ties are equal in every
        results.sort(key=functools.cmp_to_key(lambda a, b: cmp_(a[0], b[0])))            # compared field; Python's sort is stable, so list order decides)
    records = np.zeros(len(results), REC_DT)
    for i, (rec, _, _) in enumerate(results):
        records[i] = rec
    return Result(records, [compress(bt) for _, bt, _ in results], fwd_out, rev_out, reversed_, outcomes, [k for _, _, k in results], alt_ends)


def count_outcomes(results):
    c = collections.Counter()
    for r in results:
        c.update(r.outcomes)
    return {k: c[k] for k in OUTCOMES if c[k]}

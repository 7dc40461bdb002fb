"""structurerescorediagonal's per-query body stated a second time, in plain Python / numpy -- written from the reference's text alone
(F/strucclustutils/structurerescorediagonal.cpp: ungappedAlignStructure :52-155, the accept loop :309-386).  It shares no code with
foldseek_amd/csrc/host/search.cpp and imports nothing from foldseek_amd.  TEST INFRASTRUCTURE.

Its ingredients are models the suite already pins: the pair fields (forward score, start, end, reversed score) from tests/diag_model.py, the small
functions (coverage, identity, alignment length, checkCriteria, compareHits, the result line) from tests/align_model.py, mu / lambda / corrected e-value
from the oracle's C restatement (oracle/libfso.so), the matrices (3Di at 2.1 bits, BLOSUM62 at 1.4 bits for alignment type 2 and 0.0 for type 0) through
helpers.o_submat.

Arithmetic types follow the source: coverage and sequence identity are float (np.float32), the e-value is a double of the int32 difference forward -
reversed score (:82, :102, :106), which may be negative.

ONE RULE HERE IS NOT THE REFERENCE'S.  The reference has no notion of a pair it cannot rescore: on a negative diagonal with a target longer than the query
its reversed pass reads past the query (:96-99), on a diagonal outside both sequences neither branch runs and it indexes position -1.  This repository's
entry either refuses such a pair or, with skipUndefinedDiagonals, passes over it.  The model takes that rule as the parameter `skip` and states it the way
the entry's header does: a skipped pair is neither accepted nor rejected -- it touches neither counter -- and it is met only if the loop reaches it AND the
target can be covered (Util::canBeCovered comes first, :329).  With skip off a reached pair of this kind raises Undefined; one behind the cut of
--max-accept / --max-rejected is never looked at."""
import collections
import ctypes as C
import functools
import os

import numpy as np

import diag_model as D
import helpers
from align_model import (REC_DT, INT_MAX, can_be_covered, compare_hits, compute_aln_length, compute_cov, compute_seq_id, criteria, f32,  # noqa: F401
                         has_coverage, line)

OUTCOMES = ("not coverable", "skipped: undefined", "skipped: no overlap", "coverage", "e-value", "seq id", "aln length", "accepted", "accepted as identity",
            "not reached: max-accept", "not reached: max-rejected")
Result = collections.namedtuple("Result", "records backtraces outcomes hit_of_record")
DEFAULTS = dict(evalThr=10.0, covThr=0.0, covMode=0, seqIdThr=0.0, seqIdMode=0, alnLenThr=0, maxAccept=INT_MAX, maxRejected=INT_MAX, addBacktrace=1)


def params(**kw):
    p = dict(DEFAULTS)
    assert all(k in p for k in kw), kw
    p.update(kw)
    return p


class Undefined(Exception):
    """a reached pair whose reference result does not exist, with the skip rule off"""

    def __init__(self, query, key, diagonal, kind):
        super().__init__(f"query {query} target key {key} diagonal {diagonal}: {kind}")
        self.query, self.key, self.diagonal, self.kind = query, int(key), int(diagonal), kind


class World:
    """targets: list of (AA codes, 3Di codes); keys[i]: dbKey of target i; residues: getAminoAcidDBSize of the target DB (:251)"""

    def __init__(self, targets, keys=None, alignment_type=2, residues=None):
        self.targets = [(np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8)) for a, s in targets]
        self.keys = np.arange(len(targets), dtype=np.uint32) if keys is None else np.asarray(keys, np.uint32)
        self.atype = alignment_type
        self.residues = int(sum(len(a) for a, _ in self.targets)) if residues is None else int(residues)
        self.m3 = helpers.o_submat("MAT3DI", 2.1)[0].reshape(21, 21).tolist()                                  # :213
        self.mA = helpers.o_submat("BLOSUM62", 1.4 if alignment_type == 2 else 0.0)[0].reshape(21, 21).tolist()  # :225-226
        nn = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foldseek_amd", "data", "evalue_nn.bin")
        self.nn = np.fromfile(nn, dtype=np.uint8)                # the network's weights: a data file
        self.log_residues = float(np.log(float(self.residues)))
        self._q, self._pair = {}, {}

    def query(self, qa, q3):
        key = (bytes(qa), bytes(q3))
        if key not in self._q:
            qa, q3 = np.ascontiguousarray(qa, np.uint8), np.ascontiguousarray(q3, np.uint8)
            a, b = C.c_double(), C.c_double()
            helpers.oracle().fso_predict_mu_lambda(self.nn, q3, len(q3), 21, C.byref(a), C.byref(b))       # :309
            self._q[key] = dict(qa=qa, q3=q3, mu_lambda=(a.value, b.value), key=key)
        return self._q[key]

    def evalue(self, q, score):
        return float(helpers.oracle().fso_evalue_corr(float(score), q["mu_lambda"][0], q["mu_lambda"][1], self.log_residues))

    def pair(self, q, t, diagonal):
        """the fields of tests/diag_model.py for (query, target index, diagonal): they depend on no parameter"""
        k = (q["key"], int(t), int(diagonal))
        if k not in self._pair:
            ta, t3 = self.targets[int(t)]
            self._pair[k] = D.rescore(q["qa"], q["q3"], ta, t3, int(diagonal), self.m3, self.mA)
        return self._pair[k]


def rescore_query(W, qa, q3, pairs, P, identity=-1, skip=False, qname="?"):
    """pairs: (target index, diagonal as the short the module reads, :333) in list order; identity: the target index that is the query itself when
    isIdentity can be true at all (queryId == targetId && (includeIdentity || sameDB), :321), else -1.  -> Result; hit_of_record[i]: the list position
    record i came from.  backtraces: alnLength times 'M' (:127-130), or '' without -a."""
    q = W.query(qa, q3)
    L = len(q3)
    outcomes, results = [], []
    passed = rejected = 0
    for k, (t, diagonal) in enumerate(pairs):
        t, diagonal = int(t), int(diagonal)
        assert -32768 <= diagonal <= 32767
        if not passed < P["maxAccept"]:                                                  # :316
            outcomes.append("not reached: max-accept"); continue
        if not rejected < P["maxRejected"]:
            outcomes.append("not reached: max-rejected"); continue
        ta = W.targets[t][0]
        T = len(ta)
        is_identity = t == identity                                                      # :321
        if not can_be_covered(P["covThr"], P["covMode"], L, T):                          # :329-332
            rejected += 1; outcomes.append("not coverable"); continue
        r = W.pair(q, t, diagonal)
        if r["status"] != D.OK:                                                          # OURS, see the module text
            kind = "undefined" if r["status"] == D.UNDEFINED else "no overlap"
            if not skip:
                raise Undefined(qname, W.keys[t], diagonal, kind)
            outcomes.append("skipped: " + kind); continue
        dist = abs(diagonal)
        score = int(np.int32(r["score"])) - int(np.int32(r["revScore"]))                 # :82, :102
        ev = W.evalue(q, score)                                                          # :106
        if diagonal >= 0:                                                                # :116-126
            qs, qe, ds, de = r["startPos"] + dist, r["endPos"] + dist, r["startPos"], r["endPos"]
        else:
            qs, qe, ds, de = r["startPos"], r["endPos"], r["startPos"] + dist, r["endPos"] + dist
        aln_len = compute_aln_length(qs, qe, ds, de)                                     # :127
        q_cov, t_cov = compute_cov(qs, qe, L), compute_cov(ds, de, T)                    # :132-133
        if not has_coverage(P["covThr"], P["covMode"], q_cov, t_cov):                    # :135-139: dbKey UINT_MAX, :335-338
            rejected += 1; outcomes.append("coverage"); continue
        if ev > P["evalThr"]:                                                            # :140-143
            rejected += 1; outcomes.append("e-value"); continue
        ids = sum(int(q["qa"][i]) == int(ta[ds + (i - qs)]) for i in range(qs, qe + 1))  # :145-150
        seq_id = compute_seq_id(P["seqIdMode"], ids, L, T, aln_len)                      # :151
        rec = np.zeros(1, REC_DT)[0]
        rec["dbKey"], rec["score"], rec["qcov"], rec["dbcov"], rec["seqId"], rec["eval"], rec["alnLength"] = W.keys[t], score, q_cov, t_cov, seq_id, ev, aln_len
        rec["qStartPos"], rec["qEndPos"], rec["qLen"], rec["dbStartPos"], rec["dbEndPos"], rec["dbLen"] = qs, qe, L, ds, de, T
        c = criteria(rec, P)                                                             # :366
        assert c[0] and c[2]                     # both were decided by the two gates above with the same operands
        if is_identity or all(c):
            results.append((rec, "M" * aln_len if P["addBacktrace"] else "", k))         # :367-369
            outcomes.append("accepted" if all(c) else "accepted as identity")
            passed += 1
            rejected = 0
        else:
            rejected += 1                                                                # :371
            outcomes.append(("e-value", "seq id", "coverage", "aln length")[c.index(False)])
    if len(results) > 1:                                                                 # :377-379
        results.sort(key=functools.cmp_to_key(lambda a, b: compare_hits(a[0], b[0])))
    records = np.zeros(len(results), REC_DT)
    for i, (rec, _, _) in enumerate(results):
        records[i] = rec
    return Result(records, [bt for _, bt, _ in results], outcomes, [k for _, _, k in results])


def lines(result, add_backtrace):
    """the entry of the result DB: Matcher::resultToBuffer per record (:380-384); the backtrace is written run-length compressed"""
    return "".join(line(rec, (f"{len(bt)}M" if add_backtrace else None)) + "\n" for rec, bt in zip(result.records, result.backtraces))


def ties(result):
    """pairs of neighbouring records that compareHits cannot order (std::sort leaves their order open)"""
    return [i for i in range(len(result.records) - 1) if compare_hits(result.records[i], result.records[i + 1]) == 0]


def count_outcomes(results):
    c = collections.Counter()
    for r in results:
        c.update(r.outcomes)
    return {k: c[k] for k in OUTCOMES if c[k]}

"""Profile queries (a query database of type DBTYPE_HMM_PROFILE) stated in numpy, from the reference's sources alone -- Sequence::mapProfile
(M/src/commons/Sequence.cpp:301-340), the profile branch of SmithWaterman::ssw_init (M/src/alignment/StripedSmithWaterman.cpp:1364-1425) and
StructureSmithWaterman::ssw_init (F/src/commons/StructureSmithWaterman.cpp:1586-1660) -- sharing no code with foldseek_amd/csrc.

What the sources do:

* An entry is L records of 25 bytes: 20 signed score bytes, the query letter, the consensus letter, neff, two gap bytes (GAP_POS_SCORING is not
  defined in the reference build: unread).  L = (index length - 1) / 25; here an entry is the records without the terminator.
* Alignment profile: [letter][position] = (short) score / 4 in C, that is, rounded towards zero; row 20 (X) is zero whatever the entry holds.
* Gapless scan: the pssm is that profile, bias = -(smallest of the 20 x L scores) or 0, the cap 255 - bias; no composition bias.
* Structure SW: the 3Di and the AA profile are used as they are (word and int profiles are the table widened), the reversed query is the profile
  reversed position by position; the recurrence is tests/sw_model.py's, which takes ready-made tables (align_profiles).
* Refusals (the project's, where the reference would read past its tables): a length that is no multiple of 25, a letter above 20.
"""
import numpy as np

import gapless_model as gm
import sw_model as sm

RECORD = 25


class Damaged(ValueError):
    """kind: 'length' or 'letter'"""
    def __init__(self, kind, text):
        super().__init__(text)
        self.kind = kind


def decode(entry):
    """(codes uint8 [L], consensus uint8 [L], profile int8 [21, L], reversed profile int8 [21, L]) of the records of one entry"""
    raw = np.frombuffer(bytes(entry), np.uint8)
    if len(raw) % RECORD:
        raise Damaged("length", f"{len(raw)} bytes are not a multiple of {RECORD}")
    rec = raw.reshape(-1, RECORD)
    L = len(rec)
    codes, cons = rec[:, 20].copy(), rec[:, 21].copy()
    if (codes > 20).any() or (cons > 20).any():
        raise Damaged("letter", "a query or consensus letter above 20")
    score = rec[:, :20].view(np.int8).astype(np.int32)               # [L, 20]
    quarter = np.sign(score) * (np.abs(score) // 4)                  # C's division: towards zero
    prof = np.zeros((21, L), np.int8)
    prof[:20] = quarter.T
    return codes, cons, prof, np.ascontiguousarray(prof[:, ::-1])


def encode(prof_scores, codes, consensus=None, neff=0):
    """the records of an entry whose 20 stored scores per position are prof_scores [20, L] (int8, BEFORE the division); bytes 23 and 24 stay 0.
    (A record stores 20 scores: there is no X score in it.  Row 20 of the alignment profile exists only in memory, and is zeroed there.)"""
    s = np.asarray(prof_scores, np.int8).reshape(20, -1)
    L = s.shape[1]
    rec = np.zeros((L, RECORD), np.uint8)
    rec[:, :20] = s.T.view(np.uint8)
    rec[:, 20] = codes
    rec[:, 21] = codes if consensus is None else consensus
    rec[:, 22] = neff
    return rec.tobytes()


def bias(prof):
    """ssw_init's bias of a profile query: |min(0, smallest of the 20 x L scores)|"""
    p = np.asarray(prof, np.int8).reshape(21, -1)[:20]
    return int(-min(0, int(p.min(initial=0))))


def cap(prof):
    return 255 - bias(prof)


def gapless_scores(prof, db):
    """what the scan of a profile query returns per target (ungappedprefilter.cpp:381-384: ssw_init with the alignment profile)"""
    return gm.scores(prof, cap(prof), db)


def sw_records(p3, pA, targets, go=10, ge=1):
    """alignScoreEndPos of one direction: p3 / pA the int8 [21, L] tables of that direction (pA None: 3Di only), targets [(3Di codes, AA codes)]"""
    return sm.align_profiles(np.asarray(p3).astype(np.int32), None if pA is None else np.asarray(pA).astype(np.int32),
                             [t[0] for t in targets], None if pA is None else [t[1] for t in targets], go, ge)


# ---- alignStartPosBacktrace<PROFILE> (F/src/commons/StructureSmithWaterman.cpp:540-739) and the accept loop -----------------------------------------------
# structurealign takes this path instead of the block aligner when both query databases are profiles (structurealign.cpp:91-100):
#   1. the reverse pass: the same recurrence on the reversed profile prefix [0, qEnd] against the reversed target prefix [0, dbEnd]; its score must be
#      the forward score, its end cell (the first column that reaches it, the smallest row) is the start cell (:669-675);
#   2. coverage from start to end; below covThr (or with alignmentMode 1) the record keeps its start cell and gets no cigar (:682-688);
#   3. banded_sw (:1723-1957) over the rectangle, band |dbLen - qLen| + 1 doubled until the score is reached, then its trace-back;
#   4. computerBacktrace (:746-773): identities count target AA letter == the AA profile's query letter.
def start_cell(p3, pA, t3, tA, q_end, db_end, score, go=10, ge=1):
    rp3 = np.ascontiguousarray(np.asarray(p3)[:, :q_end + 1][:, ::-1])
    rpA = np.ascontiguousarray(np.asarray(pA)[:, :q_end + 1][:, ::-1])
    r = sw_records(rp3, rpA, [(np.asarray(t3)[:db_end + 1][::-1], np.asarray(tA)[:db_end + 1][::-1])], go, ge)[0]
    assert int(r["score"]) == int(score), "Score of forward/backward SW differ (the reference exits here)"
    return q_end - int(r["qEnd"]), db_end - int(r["dbEnd"])


def banded_path(match, q_len, db_len, score, go=10, ge=1, doublings=None, edge_slot=True):
    """banded_sw's M / I / D string (start -> end) of a q_len x db_len rectangle; match: int32 [q_len, db_len] substitution scores.  None: trace back error.
    doublings: a list that receives every band width the loop had to double.  edge_slot=False: WITHOUT the slot quirk described below -- not what the
    source does; it exists so that a test can name the rectangles whose path the quirk decides.
    Stated in (row, column) terms.  What the source's band slots amount to: a cell outside the band of the row above reads as H = E = 0, as does the
    cell left of a row's band, F starts every row at 0 -- and one more thing, `h_b[edge] = e_b[edge] = 0` with edge = end + 1 taken as a SLOT (:1783-1784):
    while the band still starts at column 0, that slot is the column `end` of the row above, so once `end` is clamped to the last column the row
    above loses its H and E there.  Every value is an exact integer, F is the running maximum form (gapOpen > gapExtend), directions as :1806-1846."""
    assert go > ge >= 0
    band = abs(db_len - q_len) + 1
    cols = np.arange(db_len, dtype=np.int64)
    while True:
        Hp, Ep = np.zeros(db_len, np.int64), np.zeros(db_len, np.int64)
        rows, best = [], 0
        for i in range(q_len):
            beg, end = max(0, i - band), min(db_len - 1, i + band)
            if edge_slot and 1 <= i <= band + 1 and end == db_len - 1 and db_len - 1 <= i - 1 + band:
                Hp[end] = 0; Ep[end] = 0
            j = cols[beg:end + 1]
            n = len(j)
            if i == 0:
                t1, t2 = np.full(n, -go, np.int64), np.full(n, -ge, np.int64)
            else:
                t1, t2 = Hp[beg:end + 1] - go, Ep[beg:end + 1] - ge
            e = np.maximum(t1, t2)
            de = np.where(t1 > t2, 3, 2).astype(np.int8)
            diag = np.zeros(n, np.int64)
            if i > 0:
                lo = max(beg, 1)
                diag[lo - beg:] = Hp[lo - 1:end]
            diag = diag + match[i, beg:end + 1]
            e1 = np.maximum(e, 0)
            h0 = np.maximum(e1, diag)
            # F: f[j] = max(H[j-1] - go, f[j-1] - ge) with H = f = 0 left of the band
            a = np.concatenate([[0 + (beg - 1) * ge], h0 + j * ge])                     # H[k] + k ge for k = beg - 1 .. end
            run = np.maximum.accumulate(a)[:-1]                                            # max over k <= j - 1
            f = np.maximum(run - go - (j - 1) * ge, -(j - beg + 1) * ge)
            f1 = np.maximum(f, 0)
            H = np.maximum(h0, f1)
            Hl = np.concatenate([[0], H[:-1]]); fl = np.concatenate([[0], f[:-1]])
            df = np.where(Hl - go > fl - ge, 5, 4).astype(np.int8)
            tmp1 = np.maximum(e1, f1)
            dh = np.where(tmp1 <= diag, 1, np.where(e1 > f1, de, df)).astype(np.int8)
            best = max(best, int(H.max()))
            Hp[:] = 0; Ep[:] = 0
            Hp[beg:end + 1] = H; Ep[beg:end + 1] = e
            rows.append((beg, end, (de, df, dh)))
        if best >= score:
            break
        if doublings is not None:
            doublings.append(band)
        band *= 2
    i, j, state, ops = q_len - 1, db_len - 1, 2, []
    while i > 0 or j > 0:
        if i < 0 or j < 0:
            return None
        beg, end, d = rows[i]
        if not beg <= j <= end:
            return None
        code = int(d[state][j - beg])
        if code == 1:
            i -= 1; j -= 1; state = 2; ops.append("M")
        elif code in (2, 3):
            i -= 1; state = 0 if code == 2 else 2; ops.append("I")
        elif code in (4, 5):
            j -= 1; state = 1 if code == 4 else 2; ops.append("D")
        else:
            return None
    ops.append("M")                                                                        # the cell (0, 0) closes the cigar (:1916-1933)
    return "".join(reversed(ops))


class ProfileWorld:
    """what tests/align_model.py's align_query asks of a world, for profile queries: the records from the query's own tables (both of them, whatever
    --alignment-type says), mu / lambda from the 3Di profile's query letters, and alignStartPosBacktrace<PROFILE> where a sequence query has the block aligner.
    targets: [(AA codes, 3Di codes)], keys their dbKeys; cov_thr / cov_mode: the run's, for the no-cigar rule."""

    def __init__(self, targets, keys, cov_thr=0.0, cov_mode=0, go=10, ge=1):
        import ctypes as C
        import os
        import helpers
        self._C, self._helpers = C, helpers
        self.targets = [(np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(s, np.uint8)) for a, s in targets]
        self.keys = np.asarray(keys, np.uint32)
        self.cov_thr, self.cov_mode, self.go, self.ge = cov_thr, cov_mode, go, ge
        self.log_residues = float(np.log(float(sum(len(a) for a, _ in self.targets))))
        self.nn = np.fromfile(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foldseek_amd", "data", "evalue_nn.bin"), dtype=np.uint8)
        self._q, self._sw, self._bt = {}, {}, {}

    def add_query(self, entry_aa, entry_3di):
        """-> (AA query letters, 3Di query letters): what align_query is then called with"""
        ca, _, aF, aR = decode(entry_aa)
        c3, _, sF, sR = decode(entry_3di)
        assert len(ca) == len(c3)
        key = (bytes(entry_aa), bytes(entry_3di))
        a, b = self._C.c_double(), self._C.c_double()
        self._helpers.oracle().fso_predict_mu_lambda(self.nn, np.ascontiguousarray(c3), len(c3), 21, self._C.byref(a), self._C.byref(b))
        self._q[(bytes(ca), bytes(c3))] = dict(qa=ca, q3=c3, aF=aF, aR=aR, sF=sF, sR=sR, mu_lambda=(a.value, b.value), key=key)
        return ca, c3

    def query(self, qa, q3):
        return self._q[(bytes(qa), bytes(q3))]

    def evalue(self, q, score):
        return float(self._helpers.oracle().fso_evalue_corr(float(score), q["mu_lambda"][0], q["mu_lambda"][1], self.log_residues))

    def sw(self, q, reverse, seqs):
        keys = [(q["key"], reverse, bytes(a), bytes(s)) for a, s in seqs]
        miss = [k for k in range(len(seqs)) if keys[k] not in self._sw]
        if miss:
            recs = sw_records(q["sR"] if reverse else q["sF"], q["aR"] if reverse else q["aF"], [(seqs[k][1], seqs[k][0]) for k in miss], self.go, self.ge)
            for k, r in zip(miss, recs):
                self._sw[keys[k]] = (int(r["score"]), int(r["qEnd"]), int(r["dbEnd"]), int(r["word"]))
        return [self._sw[k] for k in keys]

    def block(self, q, ta, t3, q_end, db_end, score):
        """alignStartPosBacktrace<PROFILE> -> (True, qStart, dbStart, identical, backtrace); the backtrace is empty below the coverage threshold"""
        import align_model as am
        key = (q["key"], bytes(ta), bytes(t3), q_end, db_end, score, self.cov_thr, self.cov_mode)
        if key not in self._bt:
            L, T = len(q["q3"]), len(t3)
            qs, ds = start_cell(q["sF"], q["aF"], t3, ta, q_end, db_end, score, self.go, self.ge)
            out = (True, qs, ds, 0, "")
            if am.has_coverage(self.cov_thr, self.cov_mode, am.compute_cov(qs, q_end, L), am.compute_cov(ds, db_end, T)):
                tt3, tta = np.asarray(t3[ds:db_end + 1], np.int64), np.asarray(ta[ds:db_end + 1], np.int64)
                match = (q["sF"].astype(np.int64)[:, qs:q_end + 1][tt3].T + q["aF"].astype(np.int64)[:, qs:q_end + 1][tta].T)
                path = banded_path(match, q_end - qs + 1, db_end - ds + 1, score, self.go, self.ge)
                if path is not None:
                    qp, tp, ids = qs, ds, 0
                    for op in path:
                        if op == "M":
                            ids += int(ta[tp]) == int(q["qa"][qp]); qp += 1; tp += 1
                        elif op == "I":
                            qp += 1
                        else:
                            tp += 1
                    out = (True, qs, ds, ids, path)
            self._bt[key] = out
        return self._bt[key]

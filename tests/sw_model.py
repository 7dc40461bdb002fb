"""The structure Smith-Waterman (score + end position) stated a second time, in numpy -- written from the reference's
StructureSmithWaterman.cpp alone (alignScoreEndPos, sw_sse2_word, sw_sse2_int, ssw_init), sharing no code with oracle/, foldseek_amd/csrc or
tests/helpers.py.  It is what the device kernels (k_sw, k_sw2, k_sw3) are held to; tests/test_sw_model.py holds the model itself to the C oracle,
the compiled reference, the frozen reference records and a textbook Gotoh.

Inputs: the 21 x 21 int8 matrices (`matA` None: 3Di only), the query's codes, its int8 position biases for the direction asked for (None: zeros),
the direction, the gap costs and the target codes (plain, 0..20).  Output per pair: (score, qEnd, dbEnd, word).

What the source does, as stated here:

* Profile (ssw_init / createQueryProfile): table[a][i] = mat[a][q_i] + cb_i.  The reversed query is the query read backwards with a bias vector of
  its own, indexed by the REVERSED position: table[a][i] = mat[a][q_{L-1-i}] + cb_rev_i.  Rows from L up to lanes * segLen score 0.
* Column score: the int16-saturated sum of the two tables' entries for the target's (AA, 3Di) letters.
* Recurrence, per target column, down the query rows.  gap(k) = gapOpen + (k - 1) gapExtend; every subtraction of a gap cost is an unsigned
  saturating one (never below 0); the first pass holds H in int16 (additions saturate at 32767):
      h0[r]    = max(sat(H[r-1][c-1] + s[r]), E[r])
      Fseg[r]  = max over rows r' < r OF THE SAME SEGMENT of h0[r'] - gapOpen - (r - r' - 1) gapExtend
      Ffull[r] = the same over all rows r' < r
      Hmain[r] = max(h0[r], Fseg[r])            what the striped main loop holds when it updates E
      E'[r]    = max(E[r] - gapExtend, Hmain[r] - gapOpen)
      H[r][c]  = max(h0[r], Ffull[r])           what the lazy-F loop leaves, and what the next column's diagonal reads
  The striped kernel cuts the column into `lanes` segments of segLen = ceil(L / lanes) consecutive rows (lanes = 16 for the int16 pass); its
  main loop starts every segment with F = 0 and feeds E from that H, the lazy-F loop then carries F across the segment borders into H but
  "doesn't update E" (its own comment).  That is the quirk: E sees the vertical gap state of its own segment only.
  (While gapOpen > gapExtend no RECORD depends on it: a path that turns from a vertical into a horizontal gap costs exactly what the path through
  the opposite corner costs, horizontal first, and E feeding F is never restricted.  H is therefore textbook Gotoh's in every cell, which
  tests/test_sw_model.py asserts; only E differs.  The kernels keep both F chains all the same, and so does the model.)
  Taking the maxima over h0 instead of over H is the same thing while gapOpen > gapExtend (a gap opened from a cell that F itself set is
  dominated by extending that F): the model asserts gapOpen > gapExtend, and the comparison with the oracle's literal emulation in
  tests/test_sw_model.py is what checks the equivalence; they are running maxima of h0[r'] + r' gapExtend, once per segment, once per column.
* End cell: dbEnd is the first column whose maximum STRICTLY raises the maximum so far, qEnd the smallest row of that column holding it;
  (0, 0, 0) when nothing scores.
* Re-run (alignScoreEndPos): a first pass that returns 32767 is discarded for a second one in int32, without saturation, and with 8 lanes:
  segLen = ceil(L / 8).  word is then 2, else 1.
"""
import numpy as np

NEG = -(1 << 28)


def profile(mat, codes, bias, reverse):
    """[21, L] int32: mat[a][q_i] + cb_i, for the reversed query mat[a][q_{L-1-i}] + cb_i"""
    m = np.asarray(mat).reshape(21, 21).astype(np.int32)
    c = np.asarray(codes).astype(np.int64)
    if reverse:
        c = c[::-1]
    p = m[:, c]
    if bias is not None:
        p = p + np.asarray(bias).astype(np.int32)[None, :]
    return p


def _pad_targets(targets):
    lens = np.array([len(t) for t in targets], np.int64)
    out = np.zeros((len(targets), max(1, int(lens.max()) if len(lens) else 1)), np.int64)
    for k, t in enumerate(targets):
        out[k, :len(t)] = t
    return out, lens


def one_pass(prof3, profA, t3, tA, go, ge, lanes, sat, detail=False):
    """one pass of the striped kernel over P pairs of one query at once.  prof3 / profA: [21, L] int32 (profA None); t3 / tA: lists of P code arrays.
    Returns int32 arrays score, qEnd, dbEnd; with detail also the number of columns whose maximum equals the final one, the number of rows of
    the best column holding it, and the number of columns in which a vertical gap across a segment border raised an H above what E was fed from."""
    assert go > ge >= 0, "the running-maximum form of F needs gapOpen > gapExtend"
    L = prof3.shape[1]
    seg = (L + lanes - 1) // lanes
    Lp = seg * lanes
    P = len(t3)
    T3, lens = _pad_targets(t3)
    TA = _pad_targets(tA)[0] if profA is not None else None
    p3 = np.zeros((21, Lp), np.int32); p3[:, :L] = prof3
    pA = None
    if profA is not None:
        pA = np.zeros((21, Lp), np.int32); pA[:, :L] = profA
    rows = np.arange(Lp, dtype=np.int32)
    rge = rows * ge
    H = np.zeros((P, Lp), np.int32)
    E = np.zeros((P, Lp), np.int32)
    best = np.zeros(P, np.int32); qEnd = np.zeros(P, np.int32); dbEnd = np.zeros(P, np.int32)
    ncol = np.zeros(P, np.int32); nrow = np.zeros(P, np.int32); ncross = np.zeros(P, np.int32)
    shifted = np.empty((P, Lp), np.int32)
    for c in range(int(lens.max()) if P else 0):
        live = c < lens
        s = p3[T3[:, c]]
        if pA is not None:
            s = s + pA[TA[:, c]]
        if sat:
            s = np.clip(s, -32768, 32767)
        shifted[:, 0] = 0; shifted[:, 1:] = H[:, :-1]
        h0 = shifted + s
        if sat:
            np.minimum(h0, 32767, out=h0)
        np.maximum(h0, E, out=h0)
        a = h0 + rge                                                    # h0[r'] + r' ge
        full = np.maximum.accumulate(a, axis=1)
        segm = np.maximum.accumulate(a.reshape(P, lanes, seg), axis=2)
        ffull = np.full((P, Lp), NEG, np.int32); ffull[:, 1:] = full[:, :-1]
        fseg = np.full((P, lanes, seg), NEG, np.int32); fseg[:, :, 1:] = segm[:, :, :-1]
        ffull = np.maximum(ffull - (go - ge) - rge, 0)
        fseg = np.maximum(fseg.reshape(P, Lp) - (go - ge) - rge, 0)
        hmain = np.maximum(h0, fseg)
        E = np.maximum(np.maximum(E - ge, hmain - go), 0)
        H = np.maximum(h0, ffull)
        cm = H.max(axis=1)
        up = live & (cm > best)
        if detail:
            ncol = np.where(up, 1, ncol + (live & (cm == best) & (best > 0)))
            nrow = np.where(up, (H == cm[:, None]).sum(axis=1), nrow)
            ncross += live & (H > hmain).any(axis=1)
        if up.any():
            best = np.where(up, cm, best)
            dbEnd = np.where(up, c, dbEnd)
            qEnd = np.where(up, np.argmax(H == cm[:, None], axis=1), qEnd).astype(np.int32)
    if detail:
        return best, qEnd, dbEnd, ncol, nrow, ncross
    return best, qEnd, dbEnd


REC_DT = np.dtype([("score", np.int32), ("qEnd", np.int32), ("dbEnd", np.int32), ("word", np.int32)])


def align_profiles(prof3, profA, t3, tA, go=10, ge=1, lanes16=16, lanes32=8):
    """alignScoreEndPos over P targets for ready-made [21, L] tables: the int16 pass, the int32 pass for the pairs that returned 32767"""
    out = np.zeros(len(t3), REC_DT)
    if len(t3) == 0:
        return out
    sc, qe, de = one_pass(prof3, profA, t3, tA, go, ge, lanes16, True)
    out["score"], out["qEnd"], out["dbEnd"], out["word"] = sc, qe, de, 1
    again = np.flatnonzero(sc == 32767)
    if len(again):
        sc, qe, de = one_pass(prof3, profA, [t3[k] for k in again], None if profA is None else [tA[k] for k in again], go, ge, lanes32, False)
        out["score"][again], out["qEnd"][again], out["dbEnd"][again], out["word"][again] = sc, qe, de, 2
    return out


def align(mat3, matA, q3, qA, cb3, cbA, reverse, t3, tA, go=10, ge=1):
    """records of one query in one direction against the targets t3 / tA (lists of code arrays).  cb3 / cbA: that direction's bias vectors."""
    p3 = profile(mat3, q3, cb3, reverse)
    pA = None if matA is None else profile(matA, qA, cbA, reverse)
    return align_profiles(p3, pA, t3, None if matA is None else tA, go, ge)

"""Profile queries in the k-mer prefilter, stated in numpy from the reference's sources alone (M = its vendored MMseqs2), sharing no code with
foldseek_amd/csrc:

* Sequence::mapProfile (M/src/commons/Sequence.cpp:301-352): the k-mer generator reads the 20 score bytes of a position as short, undivided, and every
  position's scores are sorted by Util::rankedDescSort20 (M/src/commons/Util.cpp:118-144), a fixed compare-exchange network that swaps only on
  val[x] < val[y]; the letter travels with its score.
* Sequence::nextKmer / nextProfileKmer: a window holds an X when one of the query LETTERS at its six pattern offsets is 20; QueryMatcher::match
  (QueryMatcher.cpp:255-287) skips it.  The composition bias of a profile is zero (:109-117), so every window's threshold is max(kmerThr, 0) (:271).
* Prefiltering::getKmerThreshold (Prefiltering.cpp:1036-1096), profile branch.
* KmerGenerator::generateKmerList / calculateArrayProduct (KmerGenerator.cpp:108-217) with one row per step (setDivideStrategy(ScoreMatrix **), :31-40).
* UngappedAlignment::createProfile (UngappedAlignment.cpp:388-421), profile branch: [pos][21] from the alignment profile, no bias correction;
  getQueryBias() is 0 (UngappedAlignment.h:36), so rescoreHits runs from a cut of 255.
"""
import numpy as np

MAX_KMER_RESULT_SIZE = 262144 * 32          # KmerGenerator.h:45
CAP = MAX_KMER_RESULT_SIZE - 1
SPACED6 = (1, 1, 0, 1, 0, 1, 0, 0, 1, 1)
POW20 = 20 ** np.arange(6, dtype=np.int64)

# Util::rankedDescSort20, comparator by comparator, in its order
SORT20 = ((0, 16), (1, 17), (2, 18), (3, 19), (4, 12), (5, 13), (6, 14), (7, 15),
          (0, 8), (1, 9), (2, 10), (3, 11),
          (8, 16), (9, 17), (10, 18), (11, 19), (0, 4), (1, 5), (2, 6), (3, 7),
          (8, 12), (9, 13), (10, 14), (11, 15), (4, 16), (5, 17), (6, 18), (7, 19), (0, 2), (1, 3),
          (4, 8), (5, 9), (6, 10), (7, 11), (12, 16), (13, 17), (14, 18), (15, 19), (0, 1),
          (4, 6), (5, 7), (8, 10), (9, 11), (12, 14), (13, 15), (16, 18), (17, 19),
          (2, 16), (3, 17), (6, 12), (7, 13), (18, 19),
          (2, 8), (3, 9), (10, 16), (11, 17),
          (2, 4), (3, 5), (6, 8), (7, 9), (10, 12), (11, 13), (14, 16), (15, 17),
          (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (12, 13), (14, 15), (16, 17),
          (1, 16), (3, 18), (5, 12), (7, 14),
          (1, 8), (3, 10), (9, 16), (11, 18),
          (1, 4), (3, 6), (5, 8), (7, 10), (9, 12), (11, 14), (13, 16), (15, 18),
          (1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16), (17, 18))


def raw_scores(entry):
    """int16 [L, 20]: the score bytes of an entry's records as the k-mer generator reads them"""
    rec = np.frombuffer(bytes(entry), np.uint8).reshape(-1, 25)
    return rec[:, :20].view(np.int8).astype(np.int16)


def letters(entry):
    return np.frombuffer(bytes(entry), np.uint8).reshape(-1, 25)[:, 20].copy()


def sort_rows(scores):
    """rankedDescSort20 on every position of scores [L, 20] -> (sorted scores int16 [L, 20], letters uint8 [L, 20])"""
    val = np.array(scores, np.int16).reshape(-1, 20)
    idx = np.tile(np.arange(20, dtype=np.uint8), (len(val), 1))
    for x, y in SORT20:
        swap = val[:, x] < val[:, y]
        val[swap, x], val[swap, y] = val[swap, y], val[swap, x]
        idx[swap, x], idx[swap, y] = idx[swap, y], idx[swap, x]
    return val, idx


def pattern(spaced):
    return [i for i, on in enumerate(SPACED6) if on] if spaced else list(range(6))


def pattern_size(spaced):
    return 10 if spaced else 6


def windows(codes, spaced):
    """[(start, has_x)] of every k-mer start of a query with these letters"""
    pat = pattern(spaced)
    n = len(codes) - pattern_size(spaced) + 1
    return [(i, bool(any(codes[i + o] >= 20 for o in pat))) for i in range(max(0, n))]


def kmer_threshold(sensitivity, kmer_size=6, context_pseudo_counts=False, k_score=None):
    """Prefiltering::getKmerThreshold for a profile query; k_score: --k-score's profile half when set"""
    if k_score is not None:
        return int(k_score)
    base, step = {(True, 5): (97.75, 8.75), (True, 6): (132.75, 8.75), (True, 7): (158.75, 9.75),
                  (False, 5): (108.8, 4.7), (False, 6): (134.35, 6.15), (False, 7): (149.15, 6.85)}[(bool(context_pseudo_counts), kmer_size)]
    # float base; float sensitivity * double step -> double; the difference is stored in a float, then cut to an int
    return int(np.float32(np.float64(np.float32(base)) - np.float64(np.float32(sensitivity)) * step))


def window_threshold(kmer_thr):
    """short kmerMatchScore = std::max(kmerThr - bias, 0) with bias 0"""
    return int(np.int16(max(int(kmer_thr), 0)))


def _short(x):
    return np.asarray(x, np.int64).astype(np.int16)


def generate_literal(rows_s, rows_l, thr):
    """generateKmerList, level by level as calculateArrayProduct does it: rows_s / rows_l [6, 20] in pattern order, thr the window's threshold.
    Returns the k-mers (sum of letter_i * 20^i) in output order.  Cutoffs are shorts, as there."""
    rows_s = np.asarray(rows_s, np.int64); rows_l = np.asarray(rows_l, np.int64)
    high = rows_s[:, 0]
    rest = np.zeros(6, np.int64)
    for i in range(5, 0, -1):
        rest[i - 1] = high[i] + rest[i]
    cutoff1 = int(_short(thr - rest[0]))
    # the input of the first product is row 0 itself; its loop breaks at the first score below cutoff1
    n0 = 0
    while n0 < 20 and rows_s[0, n0] >= cutoff1:
        n0 += 1
    score = rows_s[0, :n0].copy(); index = rows_l[0, :n0].copy()
    for i in range(5):
        nxt_s, nxt_l = rows_s[i + 1], rows_l[i + 1]
        cutoff2 = _short(thr - score - rest[i + 1]).astype(np.int64)
        # scoreArray2[j] >= cutoff2 for a leading run of j: the row is descending
        cnt = np.searchsorted(-nxt_s, -cutoff2, side="right")
        total = int(min(int(cnt.sum()), CAP))                        # counter + 1 < MAX_KMER_RESULT_SIZE in the inner loop, the same test after it
        start = np.cumsum(cnt) - cnt
        parent = np.repeat(np.arange(len(cnt)), cnt)[:total]
        child = np.arange(total) - start[parent] if total else np.zeros(0, np.int64)
        index = index[parent] + nxt_l[child] * POW20[i + 1]
        score = score[parent] + nxt_s[child]
    return index


def count_ge(rows_s, thr):
    """number of rank tuples with sum >= thr, uncapped (a convolution of the six rows' score histograms)"""
    hist = np.ones(1, np.int64); lo = 0
    for r in np.asarray(rows_s, np.int64):
        h = np.bincount(r - r.min(), minlength=1)
        hist = np.convolve(hist, h); lo += int(r.min())
    k = max(0, int(thr) - lo)
    return int(hist[k:].sum())


def generate_lex(rows_s, rows_l, thr, cap=CAP):
    """the claim: all 6-tuples of row ranks whose scores sum to >= thr, in lexicographic order of the ranks, the first `cap` of them -> their k-mers.
    Computed as a filter over the tuples themselves: the 8000 rank triples of rows 0..2 and of rows 3..5 in lexicographic order, every pair tested."""
    rows_s = np.asarray(rows_s, np.int64); rows_l = np.asarray(rows_l, np.int64)
    j = np.arange(8000)
    tri = np.stack([j // 400, (j // 20) % 20, j % 20])                # rank triples in lexicographic order
    A = rows_s[0, tri[0]] + rows_s[1, tri[1]] + rows_s[2, tri[2]]
    B = rows_s[3, tri[0]] + rows_s[4, tri[1]] + rows_s[5, tri[2]]
    ka = rows_l[0, tri[0]] + 20 * rows_l[1, tri[1]] + 400 * rows_l[2, tri[2]]
    kb = rows_l[3, tri[0]] + 20 * rows_l[4, tri[1]] + 400 * rows_l[5, tri[2]]
    sel = np.nonzero(A + B.max() >= thr)[0]                           # (the other rows of the test below are all False)
    out, have = [], 0
    for a0 in range(0, len(sel), 500):
        rows = sel[a0:a0 + 500]
        ok = A[rows, None] + B[None, :] >= thr
        ai, bi = np.nonzero(ok)                                       # row-major: lexicographic
        out.append(ka[rows[ai]] + 8000 * kb[bi]); have += len(ai)
        if have >= cap:
            break
    return (np.concatenate(out) if out else np.zeros(0, np.int64))[:cap]


def position_rows(sorted_s, sorted_l, start, spaced):
    """the six rows of the window at `start` in pattern order"""
    at = [start + o for o in pattern(spaced)]
    return sorted_s[at], sorted_l[at]


def query_lists(entry, kmer_thr, spaced, generate=generate_lex):
    """[(start, k-mers | None for a window with an X)] of one profile entry"""
    s, l = sort_rows(raw_scores(entry))
    thr = window_threshold(kmer_thr)
    out = []
    for start, has_x in windows(letters(entry), spaced):
        out.append((start, None if has_x else generate(*position_rows(s, l, start, spaced), thr)))
    return out


def ungapped_profile(entry):
    """UngappedAlignment::createProfile, profile branch: int8 [L, 21] = (short) score / 4 (towards zero), X column 0"""
    sc = raw_scores(entry).astype(np.int32)
    out = np.zeros((len(sc), 21), np.int8)
    out[:, :20] = np.sign(sc) * (np.abs(sc) // 4)
    return out


QUERY_BIAS = 0          # UngappedAlignment::getQueryBias(): the profile branch adds none, the truncation cut stays at 255


def self_score(entry):
    """rescoreHits' maxSelfScore before the subtraction: the ungapped profile scored against the query letters on diagonal 0"""
    prof, codes = ungapped_profile(entry), letters(entry)
    best = run = 0
    for i, c in enumerate(codes):
        run = max(0, run + int(prof[i, min(int(c), 20)]))
        best = max(best, run)
    return best

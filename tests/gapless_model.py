"""Independent model of the gapless prefilter scan and of its top-K selection, written from the definitions alone (include/fsgpu.h,
fsgpu_gapless_scan): plain numpy / Python ints, no call into foldseek_amd.  tests/test_gapless_model.py holds it to the C oracle, to the compiled
reference where that is built and to a second brute-force form; tests/test_gapless_multi_gpu.py holds k_gapless and k_select to it, and
tests/test_gapless_sweep_gpu.py every instantiation of k_gapless (best_cells states the conditions on that sweep's inputs).

A profile is the int8 [21][L] array fsgpu_gapless_scan takes (pssm[code][row]); a database is PaddedDB-like (data3di, offsets, lengths): codes
0..20, 32 and above = soft-masked, which the scan reads as X (20)."""
import numpy as np

HIT_DT = np.dtype([("id", np.uint32), ("score", np.int32)])
X = 20
_DEAD = 21                    # padding column of a group of targets: its profile row forces the running sum to zero
_NEG = -(1 << 30)            # a sum stays below 128 * 65535 < 2^24: int32 holds _NEG + sum


def clamp(cap):
    """the cap the scan applies: fsgpu_gapless_scan clamps scoreCap into 0..255"""
    return max(0, min(int(cap), 255))


def target_codes(db, i):
    raw = np.asarray(db.data3di[int(db.offsets[i]):int(db.offsets[i]) + int(db.lengths[i])]).astype(np.int64)
    return np.where(raw >= 32, X, raw)


def pack(db, group=64):
    """the targets in groups of similar length, each group one code matrix padded with the dead column: [(ids, codes [len(ids)][Tmax])];
    scores() takes this in place of the database when several profiles meet one database"""
    lens = np.asarray(db.lengths, np.int64)
    order = np.argsort(lens, kind="stable")
    out = []
    for a in range(0, len(order), group):
        ids = order[a:a + group]
        codes = np.full((len(ids), max(1, int(lens[ids].max()))), _DEAD, np.int64)
        for k, t in enumerate(ids):
            codes[k, :lens[t]] = target_codes(db, t)
        out.append((ids, codes))
    return out


def best_runs(pssm, db):
    """per target the maximum, over all diagonals, of the running sum S = max(0, S + pssm[code][row]) -- uncapped"""
    pssm = np.asarray(pssm).astype(np.int32)
    assert pssm.ndim == 2 and pssm.shape[0] == 21 and np.abs(pssm).max(initial=0) <= 128
    L = pssm.shape[1]
    ext = np.vstack([pssm, np.full((1, L), _NEG, np.int32)])
    groups = db if isinstance(db, list) else pack(db)
    best = np.zeros(sum(len(ids) for ids, _ in groups), np.int64)
    for ids, codes in groups:
        m = np.zeros(len(ids), np.int32)
        by_rows = L <= codes.shape[1]                 # walk the shorter side of the matrix, keep the sums of the longer one: the same cells either way
        S = np.zeros(codes.shape if by_rows else (len(ids), L), np.int32)
        for step in range(L if by_rows else codes.shape[1]):
            # by rows: S[t][j] is the sum of the diagonal through (row, column j) of target t; by columns: through (row i, column) for every row i
            cur = ext[:, step][codes] if by_rows else ext[codes[:, step]]
            cur[:, 1:] += S[:, :-1]                   # the diagonal comes from (row - 1, column - 1); the first row / column starts one
            np.maximum(cur, 0, out=cur)
            np.maximum(m, cur.max(axis=1), out=m)
            S = cur
        best[ids] = m
    return best


def scores(pssm, cap, db):
    """what fsgpu_gapless_scores returns: min(max(0, min(cap, 255)), best run) per target, int32"""
    return np.minimum(best_runs(pssm, db), clamp(cap)).astype(np.int32)


def scores_brute(pssm, cap, targets):
    """the same from the whole DP matrix in Python integers; targets: list of code sequences (0..20 or masked)"""
    L = len(pssm[0])
    out = []
    for t in targets:
        t = [X if int(c) >= 32 else int(c) for c in t]
        H = [[0] * (len(t) + 1) for _ in range(L + 1)]
        best = 0
        for i in range(1, L + 1):
            for j in range(1, len(t) + 1):
                H[i][j] = max(0, H[i - 1][j - 1] + int(pssm[t[j - 1]][i - 1]))
                best = max(best, H[i][j])
        out.append(min(clamp(cap), best))
    return np.array(out, np.int32)


def best_cells(pssms, targets):
    """Where the best run of each (profile, target) pair ends, by brute force over the whole matrix: pssms [n][21][L] against n code sequences, pair k =
    (pssms[k], targets[k]).  Per pair (score, cells, start): the uncapped maximum, every (row, column) that holds it, and the cell the run into the
    first of them starts in (back along the diagonal while the cell before it is positive).  The conditions on test inputs are stated with this."""
    pssms = np.asarray(pssms).astype(np.int32)
    n, _, L = pssms.shape
    ext = np.concatenate([pssms, np.full((n, 1, L), _NEG, np.int32)], axis=1)
    T = max(len(t) for t in targets)
    codes = np.full((n, T), _DEAD, np.int64)
    for k, t in enumerate(targets):
        t = np.asarray(t).astype(np.int64)
        codes[k, :len(t)] = np.where(t >= 32, X, t)
    H = np.zeros((n, L, T), np.int32)
    prev = np.zeros((n, L), np.int32)
    pick = np.arange(n)
    for j in range(T):
        cur = ext[pick, codes[:, j], :].copy()
        cur[:, 1:] += prev[:, :-1]
        np.maximum(cur, 0, out=cur)
        H[:, :, j] = prev = cur
    out = []
    for k in range(n):
        score = int(H[k].max())
        cells = [(int(i), int(j)) for i, j in np.argwhere(H[k] == score)] if score > 0 else []
        start = None
        if cells:
            i, j = cells[0]
            while i > 0 and j > 0 and H[k, i - 1, j - 1] > 0:
                i, j = i - 1, j - 1
            start = (i, j)
        out.append((score, cells, start))
    return out


def select(scores, min_score, identity, max_res):
    """the hit list: targets with score > min_score, or the identity id; by (score descending, id ascending); the first min(max_res, n)"""
    s = np.asarray(scores).astype(np.int64)
    ids = np.flatnonzero((s > int(min_score)) | (np.arange(len(s)) == int(identity)))
    ids = ids[np.lexsort((ids, -s[ids]))][:max(0, min(int(max_res), len(s)))]
    out = np.zeros(len(ids), HIT_DT)
    out["id"], out["score"] = ids, s[ids]
    return out

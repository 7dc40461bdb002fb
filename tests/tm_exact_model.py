"""tests/tm_exact_model.py -- an independent model of the reference's TM-score WITH its superposition, approximate and exact (TEST INFRASTRUCTURE, numpy
only).  Built from the pieces of tests/tm_model.py (kabsch_fast, frag_lengths, frag_starts, the parameter formulas); written from
F/src/commons/TMaligner.cpp:50-212 and F/lib/tmalign/TMalign.cpp (TMscore8_search :225-391, TMscore8_search_standard :394-547, score_fun8 :76-143,
parameter_set4final :49-61), not from this repository's kernels.

  * score_fun8()     tm_model's, with the divisor (Lnorm) as an argument: n in the approximate searches, (float) normLen in the exact one.
  * search()         one TMscore8_search[_standard]: fragment lengths outer, starts inner (step 40 / 1), refinement rounds innermost (20 / 10).  t0 / u0
                     are overwritten at every STRICT improvement of score_max, which starts at -1, so what is left is the superposition of the FIRST
                     occurrence of the maximum in that serial order.  A NaN score never wins.
  * approximate()    computeAppoximateTMscore: t / u are written by KabschFast over all pairs, then by standard_TMscore's search, then by
                     detailed_search_standard's: the last search that ever beat -1 wins, else the all-pairs Kabsch.
  * exact()          computeExactTMscore.  Its opening detailed_search_standard has no observable effect (every aligned pair passes `i >= 0 || d <= score_d8`;
                     KabschFast over all pairs then overwrites t, u and rmsd0), so it is not modelled.  What remains: rmsd0 of the all-pairs KabschFast,
                     rmsd = sqrt(rmsd0 / n) in float, TMscore8_search(step 1, n_it 10, Lnorm = (float) normLen, score_d8 of parameter_set4search, d0 /
                     d0_search of parameter_set4final), TM = (double) score_max.

The raw record of a task (what the device entry returns, RAW_COLS uint32 words): pairs, bits of the two scores, of the raw rms, the source code, bits of
t[3] and of u[3][3] row-major.  Without pairs nothing runs: scores -1, rms 0, source none, t = 0, u = identity.
"""
import math

import numpy as np

import tm_model as T

f32 = np.float32
f64 = np.float64

SRC_NONE, SRC_KABSCH, SRC_SEARCH1, SRC_SEARCH2, SRC_EXACT = range(5)
RAW_COLS = 17
NO_ORD = -1


def score_fun8(xtm, ytm, t, u, d, score_d8, d0, div, stats=None):
    """do_rotation + score_fun8 with Lnorm = div -> (selected indices, score float32)"""
    n = xtm.shape[1]
    x, y, z = xtm
    xt = [f32(t[k]) + ((f32(u[k][0]) * x + f32(u[k][1]) * y) + f32(u[k][2]) * z) for k in range(3)]
    dx, dy, dz = xt[0] - ytm[0], xt[1] - ytm[1], xt[2] - ytm[2]
    di = (dx * dx + dy * dy) + dz * dz
    d02 = f32(d0 * d0)
    cut = f32(score_d8 * score_d8)
    term = np.where(di < cut, f32(1.0) / (f32(1.0) + di / d02), f32(0.0)).astype(f32)
    score_sum = np.cumsum(term, dtype=f32)[-1] if n else f32(0)
    d = f32(d)
    d_tmp = f32(d * d)
    inc = 0
    while True:
        sel = np.nonzero(di < d_tmp)[0]
        if len(sel) < 3 and n > 3:
            inc += 1
            dinc = f64(d) + f64(inc) * f64(0.5)
            d_tmp = f32(dinc * dinc)
            if stats is not None:
                stats["relief"] = stats.get("relief", 0) + 1
        else:
            break
    return sel, f32(f32(score_sum) / f32(div))


def search(xtm, ytm, d0_search, score_d8, d0, div, step, rounds, stats=None):
    """-> (score_max float32, ordinal of the start that first reached it or NO_ORD, t, u).  stats["starts"]: per start (ordinal order) the best score
    of the start and the bits of the superposition that first reached it -- what a test needs to see ties"""
    n = xtm.shape[1]
    score_max, best_ord, t0, u0 = f32(-1), NO_ORD, None, None
    d0_search = f32(d0_search)
    ordinal = 0
    per_start = []
    for L in T.frag_lengths(n):
        for i in T.frag_starts(n, L, step):
            own, own_tu = None, None

            def seen(score, t, u):
                nonlocal score_max, best_ord, t0, u0, own, own_tu
                if score > score_max:
                    score_max, best_ord, t0, u0 = score, ordinal, t, u
                if stats is not None and (own is None or score > own):
                    own, own_tu = score, tu_bits(t, u).tobytes()

            rms, t, u = T.kabsch_fast(xtm[:, i:i + L], ytm[:, i:i + L], stats)
            sel, score = score_fun8(xtm, ytm, t, u, f32(d0_search - f32(1)), score_d8, d0, div, stats)
            seen(score, t, u)
            d = f32(d0_search + f32(1))
            for _ in range(rounds):
                prev = sel
                rms, t, u = T.kabsch_fast(xtm[:, sel], ytm[:, sel], stats)
                sel, score = score_fun8(xtm, ytm, t, u, d, score_d8, d0, div, stats)
                seen(score, t, u)
                if len(sel) == len(prev) and np.array_equal(sel, prev):
                    break
            per_start.append((own, own_tu))
            ordinal += 1
    if stats is not None:
        stats["starts"] = per_start
    return score_max, best_ord, t0, u0


def exact_params(norm_len):
    """-> (score_d8 of parameter_set4search, Lnorm, d0, d0_search of parameter_set4final) as float32"""
    score_d8 = T.search_params(norm_len)[1]
    lnorm = f32(norm_len)
    d0 = T.standard_params(norm_len)          # the same formula: 0.5 up to 21, 1.24 (L - 15)^(1/3) - 1.8 beyond, never below 0.5
    d0_search = d0
    if d0_search > 8:
        d0_search = f32(8)
    if d0_search < 4.5:
        d0_search = f32(4.5)
    return score_d8, lnorm, d0, d0_search


IDENT = [[f32(1), f32(0), f32(0)], [f32(0), f32(1), f32(0)], [f32(0), f32(0), f32(1)]]


def approximate(xtm, ytm, norm_len, stats=None):
    """computeAppoximateTMscore -> dict(n, scores [2], rms, source, t, u)"""
    n = xtm.shape[1]
    if n == 0:
        return {"n": 0, "scores": [f32(-1), f32(-1)], "rms": f32(0), "source": SRC_NONE, "t": [f32(0)] * 3, "u": IDENT}
    with np.errstate(all="ignore"):
        _, score_d8, d0, d0_search = T.search_params(norm_len)
        d0s = T.standard_params(norm_len)
        rms, t, u = T.kabsch_fast(xtm, ytm, stats)
        source = SRC_KABSCH
        s1, o1, t1, u1 = search(xtm, ytm, d0s, score_d8, d0s, f32(n), 40, 20, stats)
        if o1 != NO_ORD:
            t, u, source = t1, u1, SRC_SEARCH1
        s2, o2, t2, u2 = search(xtm, ytm, d0_search, score_d8, d0, f32(n), 40, 20, stats)
        if o2 != NO_ORD:
            t, u, source = t2, u2, SRC_SEARCH2
    return {"n": n, "scores": [s1, s2], "rms": rms, "source": source, "t": t, "u": u}


def exact(xtm, ytm, norm_len, stats=None):
    """computeExactTMscore -> dict(n, scores [score_max, -1], rms (raw, of the all-pairs KabschFast), source, t, u, ord)"""
    n = xtm.shape[1]
    if n == 0:
        return {"n": 0, "scores": [f32(-1), f32(-1)], "rms": f32(0), "source": SRC_NONE, "t": [f32(0)] * 3, "u": IDENT, "ord": NO_ORD}
    with np.errstate(all="ignore"):
        score_d8, lnorm, d0, d0_search = exact_params(norm_len)
        rms, t, u = T.kabsch_fast(xtm, ytm, stats)
        source = SRC_KABSCH
        s, o, ts, us = search(xtm, ytm, d0_search, score_d8, d0, lnorm, 1, 10, stats)
        if o != NO_ORD:
            t, u, source = ts, us, SRC_EXACT
    return {"n": n, "scores": [s, f32(-1)], "rms": rms, "source": source, "t": t, "u": u, "ord": o}


def exact_finish(n, score, raw_rms):
    """-> (TM-score as a Python float, rmsd as float32): TM = (double) score_max; rmsd0 = sqrt(rmsd0 / n_ali8) in float"""
    with np.errstate(all="ignore"):
        q = f32(f32(raw_rms) / f32(n))
        rmsd = f32(math.sqrt(float(q))) if q >= 0 else f32(np.sqrt(f64(q)))          # 0 / 0 and its root keep the hardware's NaN
    return float(f32(score)), rmsd


def tu_bits(t, u):
    return np.array([f32(v) for v in t] + [f32(v) for row in u for v in row], f32).view(np.uint32)


def raw_row(res):
    out = np.zeros(RAW_COLS, np.uint32)
    out[0] = res["n"]
    out[1:4] = np.array([res["scores"][0], res["scores"][1], res["rms"]], f32).view(np.uint32)
    out[4] = res["source"]
    out[5:] = tu_bits(res["t"], res["u"])
    return out


def row_fields(row):
    """a raw row -> (n, s0, s1, rms, source, t float32 [3], u float32 [9])"""
    fl = row[1:4].view(f32)
    return int(row[0]), fl[0], fl[1], fl[2], int(row[4]), row[5:8].view(f32), row[8:17].view(f32)


def sstr_f(v):
    """SSTR(float): three decimals"""
    return "%.3f" % float(v)


def tm_of_row(row, norm_len, is_exact):
    n, s0, s1, rms, _, _, _ = row_fields(row)
    return exact_finish(n, s0, rms)[0] if is_exact else T.tm_finish(n, s0, s1, norm_len)


def rmsd_of_row(row, is_exact):
    n, s0, _, rms, _, _, _ = row_fields(row)
    return float(exact_finish(n, s0, rms)[1]) if is_exact else float(rms)


def aln2tmscore_line(db_key, row, norm_len, is_exact):
    """the line aln2tmscore writes for one alignment"""
    _, _, _, _, _, t, u = row_fields(row)
    return " ".join([str(db_key), T.sstr(tm_of_row(row, norm_len, is_exact))] + [sstr_f(v) for v in t] + [sstr_f(v) for v in u])


def convertalis_fields(rows, norm_lens, is_exact):
    """alntmscore, qtmscore, ttmscore, rmsd, u, t of one record from its three raw rows (normalisations 0 / 1 / 2): the rmsd and u / t columns print the
    result of the last computeTMscore call before them, which is the target-length one"""
    out = [T.sstr(tm_of_row(r, nl, is_exact)) for r, nl in zip(rows, norm_lens)]
    _, _, _, _, _, t, u = row_fields(rows[2])
    out.append(T.sstr(rmsd_of_row(rows[2], is_exact)))
    out.append(",".join(sstr_f(v) for v in u))
    out.append(",".join(sstr_f(v) for v in t))
    return out

"""tests/tm_model.py -- an independent float32 / float64 model of the reference's approximate TM-score (TEST INFRASTRUCTURE, numpy only).

Written from F/lib/tmalign/{TMalign.cpp,Kabsch.h,basic_fun.h} and F/src/commons/TMaligner.cpp (computeAppoximateTMscore), not from this repository's
kernels.  The reference compiles that library without floating-point contraction, so every operation below is one plain IEEE operation in source order:

  * pairs()          the backtrace -> aligned (target, query) coordinates in query order ('M' pairs, 'I' advances the query, anything else the target).
  * search_params()  parameter_set4search(normLen, normLen): score_d8, d0 = D0_MIN, d0_search in [4.5, 8]; standard_params(): d0 of standard_TMscore.
  * kabsch_fast()    rmsd_uncentered_avx: the sums are four serial float chains per quantity (elements p = j mod 4 in order, the `permute2f128` halves),
                     combined (l0 + l1) + (l2 + l3) by the hadd trees; ssq takes c1x^2 of both halves and then the five other squares of both halves per
                     chunk of 8; centring in float; the 3x3 eigen step and rmatrix<double> in double; casts to float; R34v4_sse3 for the translation.
                     Any NaN in the rotation -> kabsch_classic(), the double-precision Kabsch() (mode 2), which overwrites rms, t and u:
                     written with this model's own helpers; the reference's operation order, thresholds and float-abs habits are kept.
  * score_fun8()     rotate, squared distance, 1 / (1 + di / d02) masked by di < score_d8^2, LEFT-TO-RIGHT float sum (np.cumsum is sequential, np.sum is
                     not), selection di < d_tmp with the relief loop in double.
  * search()         TMscore8_search_standard: fragment lengths, starts 0, 40, 80 ... with the last start forced, at most 20 refinement rounds.
  * tm_finish()      the scalings of standard_TMscore (double) and detailed_search_standard (float) and their maximum.

Doubles are numpy float64 scalars (IEEE, no exceptions); atan2 / cos / sin / pow come from the C library through `math`, as in the reference.
"""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
SQRT3 = f64(1.732050807568877)


def pairs(qc, tc, q_start, t_start, backtrace):
    """-> (xtm = target [3, n], ytm = query [3, n]) float32"""
    qi, ti, a2q, a2t = q_start, t_start, [], []
    for ch in backtrace:
        if ch == "M":
            a2q.append(qi); a2t.append(ti); qi += 1; ti += 1
        elif ch == "I":
            qi += 1
        else:
            ti += 1
    a2q, a2t = np.array(a2q, np.int64), np.array(a2t, np.int64)
    return np.ascontiguousarray(np.asarray(tc, f32)[:, a2t]), np.ascontiguousarray(np.asarray(qc, f32)[:, a2q])


def _d0_formula(lnorm):
    """(float)(1.24 * pow(Lnorm * 1.0 - 15, 1.0 / 3) - 1.8); a negative base gives NaN as glibc's pow does"""
    base = float(lnorm) - 15.0
    p = math.pow(base, 1.0 / 3) if base >= 0 else float("nan")
    return f32(1.24 * p - 1.8)


def search_params(norm_len):
    """parameter_set4search -> (Lnorm, score_d8, d0, d0_search) as float32"""
    lnorm = f32(norm_len)
    d0 = f32(0.168) if lnorm <= 19 else _d0_formula(lnorm)
    d0 = f32(f64(d0) + f64(0.8))                         # float + double constant: added in double, rounded to float
    d0_search = d0
    if d0_search > 8:
        d0_search = f32(8)
    if d0_search < 4.5:
        d0_search = f32(4.5)
    score_d8 = f32(1.5 * math.pow(float(lnorm), 0.3) + 3.5)
    return lnorm, score_d8, d0, d0_search


def standard_params(norm_len):
    """d0 of standard_TMscore (also its local_d0_search)"""
    lnorm = f32(norm_len)
    d0 = _d0_formula(lnorm) if lnorm > 21 else f32(0.5)
    if d0 < 0.5:
        d0 = f32(0.5)
    return d0


def _chain(a):
    """a float32 [m, 4]: four serial chains down the rows, then (l0 + l1) + (l2 + l3)"""
    if len(a) == 0:
        return f32(0)
    l = np.cumsum(a, axis=0, dtype=f32)[-1]
    return f32(f32(l[0] + l[1]) + f32(l[2] + l[3]))


def _dot4(a, b, c):
    return f32(f32(f32(0) + a) + f32(b + c))


def _sqrt(v):
    return f64(math.sqrt(v)) if v >= 0 else (f64(v) if v != v else f64("nan"))


def _cos(v):
    return f64(math.cos(v)) if math.isfinite(v) else f64("nan")


def _sin(v):
    return f64(math.sin(v)) if math.isfinite(v) else f64("nan")


def key_eigenvector(ev, c):
    """the quaternion (w, x, y, z) of the fit: cofactors along the first row of (K - ev I), K the symmetric 4 x 4 key matrix of the correlation matrix c"""
    kwx, kwy, kwz = c[1][2] - c[2][1], c[2][0] - c[0][2], c[0][1] - c[1][0]
    kxy, kxz, kyz = c[0][1] + c[1][0], c[2][0] + c[0][2], c[1][2] + c[2][1]
    kxx = ((c[0][0] - c[1][1]) - c[2][2]) - ev
    kyy = ((-c[0][0] + c[1][1]) - c[2][2]) - ev
    kzz = ((-c[0][0] - c[1][1]) + c[2][2]) - ev
    m_yy_zz, m_xy_zz, m_xy_yz = kyy * kzz - kyz * kyz, kxy * kzz - kxz * kyz, kxy * kyz - kxz * kyy
    m_wy_yz, m_wy_zz, m_wy_xz = kwy * kyz - kwz * kyy, kwy * kzz - kwz * kyz, kwy * kxz - kwz * kxy
    return ((kxx * m_yy_zz - kxy * m_xy_zz) + kxz * m_xy_yz, (-kwx * m_yy_zz + kxy * m_wy_zz) - kxz * m_wy_yz,
            (kwx * m_xy_zz - kxx * m_wy_zz) + kxz * m_wy_xz, (-kwx * m_xy_yz + kxx * m_wy_yz) - kxy * m_wy_xz)


def quat_rotation(q):
    """rotation matrix of an unnormalised quaternion: every product is scaled by 1 / |q|^2"""
    w, x, y, z = q
    scale = f64(1.0) / (((w * w + x * x) + y * y) + z * z)
    ww, xx, yy, zz = w * w * scale, x * x * scale, y * y * scale, z * z * scale
    xy, wz, zx = x * y * scale, w * z * scale, z * x * scale
    wy, yz, wx = w * y * scale, y * z * scale, w * x * scale
    two = f64(2.0)
    return [[((ww + xx) - yy) - zz, two * (xy + wz), two * (zx - wy)],
            [two * (xy - wz), ((ww - xx) + yy) - zz, two * (yz + wx)],
            [two * (zx + wy), two * (yz - wx), ((ww - xx) - yy) + zz]]


def rmatrix(ev, r):
    """rmatrix<double> of the reference -> u[3][3] float64"""
    return quat_rotation(key_eigenvector(ev, r))


def kabsch_avx(x, y):
    """kabsch_quat_soa_avx(n, x, y): x = c1, y = c2, float32 [3, n], n >= 1 -> (rms float32, t float32[3], u float32[3][3]), possibly NaN"""
    n = x.shape[1]
    up = (n + 7) // 8 * 8
    c1 = np.zeros((3, up), f32); c1[:, :n] = x
    c2 = np.zeros((3, up), f32); c2[:, :n] = y
    c1x, c1y, c1z = c1
    c2x, c2y, c2z = c2
    ch = lambda v: _chain(v.reshape(-1, 4))
    s1x, s1y, s1z, s2x, s2y, s2z = ch(c1x), ch(c1y), ch(c1z), ch(c2x), ch(c2y), ch(c2z)
    sxx, sxy, sxz = ch(c1x * c2x), ch(c1x * c2y), ch(c1x * c2z)
    syx, syy, syz = ch(c1y * c2x), ch(c1y * c2y), ch(c1y * c2z)
    szx, szy, szz = ch(c1z * c2x), ch(c1z * c2y), ch(c1z * c2z)
    t1 = ((c2x * c2x + c2z * c2z) + (c2y * c2y + c1y * c1y)) + c1z * c1z
    ssq = _chain(np.concatenate([(c1x * c1x).reshape(-1, 2, 4), t1.reshape(-1, 2, 4)], axis=1).reshape(-1, 4))
    fnat = f32(n)
    inv = f32(f32(1.0) / fnat)
    c0 = [f32(v * inv) for v in (sxx, s1x, s1y, s1z, ssq, s2x, s2y, s2z)]
    sxx = f32(sxx - c0[1] * s2x)
    sxy = f32(sxy - c0[1] * s2y); sxz = f32(sxz - c0[1] * s2z)
    syx = f32(syx - c0[2] * s2x); syy = f32(syy - c0[2] * s2y)
    syz = f32(syz - c0[7] * s1y); szx = f32(szx - c0[5] * s1z); szy = f32(szy - c0[6] * s1z); szz = f32(szz - c0[7] * s1z)
    r0r0 = _dot4(sxx * sxx, sxy * sxy, sxz * sxz)
    r0r1 = _dot4(sxx * syx, sxy * syy, sxz * syz)
    r1r1 = _dot4(syx * syx, syy * syy, syz * syz)
    r0r2 = _dot4(sxx * szx, sxy * szy, sxz * szz)
    r1r2 = _dot4(syx * szx, syy * szy, syz * szz)
    r2r2 = _dot4(szx * szx, szy * szy, szz * szz)
    detf = _dot4(sxx * f32(syy * szz - szy * syz), sxy * f32(syz * szx - szz * syx), sxz * f32(syx * szy - szx * syy))
    ssqd = f64(f32(f32(f32(f32(f32(f32(f32(c0[4] - c0[1] * c0[1]) - c0[2] * c0[2]) - c0[3] * c0[3]) - c0[5] * c0[5]) - c0[6] * c0[6]) - c0[7] * c0[7]) * fnat))
    det = f64(detf)
    detsq = det * det
    rr = [f64(r0r0), f64(r0r1), f64(r1r1), f64(r0r2), f64(r1r2), f64(r2r2)]
    inv3 = f64(1.0) / f64(3.0)
    spur = ((rr[0] + rr[2]) + rr[5]) * inv3
    cof = (((((rr[2] * rr[5] - rr[4] * rr[4]) + rr[0] * rr[5]) - rr[3] * rr[3]) + rr[0] * rr[2]) - rr[1] * rr[1]) * inv3
    e = [spur, spur, spur]
    h = spur * spur - cof if spur > 0 else f64(-1.0)
    if h > 0:
        g = (spur * cof - detsq) * f64(0.5) - spur * h
        sqrth = _sqrt(h)
        d1 = h * h * h - g * g
        d1 = f64(math.atan2(0.0, -g)) * inv3 if d1 < 0 else f64(math.atan2(_sqrt(d1), -g)) * inv3
        cth = sqrth * _cos(d1)
        sth = sqrth * SQRT3 * _sin(d1)
        e[0] = e[0] + (cth + cth)
        e[1] = e[1] + (-cth + sth)
        e[2] = e[2] + (-cth - sth)
    e = [f64(0) if v < 0 else _sqrt(v) for v in e]
    d = (e[0] + e[1]) - e[2] if det < 0 else (e[0] + e[1]) + e[2]
    rms = ((ssqd - d) - d) * (f64(1.0) / f64(n))
    rms = _sqrt(rms) if rms > 1e-8 else f64(0.0)
    mr = [[f64(sxx), f64(sxy), f64(sxz)], [f64(syx), f64(syy), f64(syz)], [f64(szx), f64(szy), f64(szz)]]
    ud = rmatrix(d, mr)
    c1c, c2c = c0[1:4], c0[5:8]
    t = []
    for k in range(3):
        m = [f32(-ud[0][k]), f32(-ud[1][k]), f32(-ud[2][k])]
        t.append(f32(f32(m[0] * c1c[0] + m[1] * c1c[1]) + f32(m[2] * c1c[2] + c2c[k] * f32(1.0))))
    u = [[f32(ud[j][i]) for j in range(3)] for i in range(3)]
    return f32(rms), t, u


def _abs_as_float(v):
    """the reference calls fabsf() on doubles in places: the value is converted to float first"""
    return f64(abs(f32(v)))


def _unit_or_zero(v):
    """v / |v|, or zeros when |v|^2 is not above 1e-8 (the squared length is summed left to right from 0)"""
    len2 = f64(0.0)
    for x in v:
        len2 = len2 + x * x
    s = f64(1.0) / _sqrt(len2) if len2 > f64(0.00000001) else f64(0.0)
    return [x * s for x in v]


def _cross(x, y):
    return [x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]]


def _eigenvector(g, lam):
    """g = (xx, xy, yy, xz, yz, zz) of the symmetric matrix G: the column of adj(lam I - G) with the largest diagonal entry, normalised"""
    gxx, gxy, gyy, gxz, gyz, gzz = g
    adj = {"xx": (lam - gyy) * (lam - gzz) - gyz * gyz, "xy": (lam - gzz) * gxy + gxz * gyz, "yy": (lam - gxx) * (lam - gzz) - gxz * gxz,
           "xz": (lam - gyy) * gxz + gxy * gyz, "yz": (lam - gxx) * gyz + gxy * gxz, "zz": (lam - gxx) * (lam - gyy) - gxy * gxy}
    adj = {k: (f64(0.0) if _abs_as_float(v) <= f64(0.00000001) else v) for k, v in adj.items()}
    if _abs_as_float(adj["xx"]) >= abs(adj["yy"]):
        col = 2 if _abs_as_float(adj["xx"]) < abs(adj["zz"]) else 0
    else:
        col = 1 if _abs_as_float(adj["yy"]) >= _abs_as_float(adj["zz"]) else 2
    return _unit_or_zero([[adj["xx"], adj["xy"], adj["xz"]], [adj["xy"], adj["yy"], adj["yz"]], [adj["xz"], adj["yz"], adj["zz"]]][col])


def _orthonormal_pair(first, second):
    """-> (second made a unit vector orthogonal to the unit vector first, ok).  The projection is removed; with no more than 0.01 of squared length left,
    second is rebuilt in the plane of the two larger components of first; ok is False when that fails too"""
    along = (first[0] * second[0] + first[1] * second[1]) + first[2] * second[2]
    second = [s - along * f for s, f in zip(second, first)]
    left = f64(0.0)
    for s in second:
        left = left + s * s
    if not left <= f64(0.01):
        scale = f64(1.0) / _sqrt(left)
        return [s * scale for s in second], True
    small, least = 0, f64(1.0)
    for i in range(3):                      # the smallest |component| of first, the last one among equals
        if least < abs(first[i]):
            continue
        least, small = abs(first[i]), i
    k, l = (small + 1) % 3, (small + 2) % 3
    length = _sqrt(first[k] * first[k] + first[l] * first[l])
    if not length > f64(0.01):
        return second, False
    second[small], second[k], second[l] = f64(0.0), -first[l] / length, first[k] / length
    return second, True


def kabsch_classic(x, y):
    """the reference's Kabsch(x, y, n, mode 2) -> (rms float32 -- a SUM of squares there --, t float32[3], u float32[3][3]): eigenvalues of G = C^T C for
    the correlation matrix C by the trigonometric solution of the cubic, the eigenvectors of the largest and the smallest one, a right-handed basis A,
    B = normalised C A, the rotation B A^T"""
    n = x.shape[1]
    ident = [[f32(1), f32(0), f32(0)], [f32(0), f32(1), f32(0)], [f32(0), f32(0), f32(1)]]
    if n < 1:
        return f32(0), [f32(0)] * 3, ident
    zero = f64(0.0)
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    # first moments and the nine cross sums are serial float chains in pair order
    sum_a = [f64(np.cumsum(x[i], dtype=f32)[-1]) for i in range(3)]
    sum_b = [f64(np.cumsum(y[i], dtype=f32)[-1]) for i in range(3)]
    cross = [[f64(np.cumsum(x[i] * y[j], dtype=f32)[-1]) for j in range(3)] for i in range(3)]
    count = f64(n)
    centre_a = [s / count for s in sum_a]
    centre_b = [s / count for s in sum_b]
    xd, yd = x.astype(f64), y.astype(f64)
    terms = np.stack([(xd[i] - centre_a[i]) * (xd[i] - centre_a[i]) + (yd[i] - centre_b[i]) * (yd[i] - centre_b[i]) for i in range(3)], axis=1).reshape(-1)
    spread = f64(np.cumsum(terms, dtype=f64)[-1])          # one term per pair and axis, in double
    corr = [[cross[i][j] - sum_a[i] * sum_b[j] / count for i in range(3)] for j in range(3)]          # corr[j][i]
    det = (corr[0][0] * (corr[1][1] * corr[2][2] - corr[1][2] * corr[2][1]) - corr[0][1] * (corr[1][0] * corr[2][2] - corr[1][2] * corr[2][0])) \
        + corr[0][2] * (corr[1][0] * corr[2][1] - corr[1][1] * corr[2][0])
    col_dot = lambda p, q: (corr[0][p] * corr[0][q] + corr[1][p] * corr[1][q]) + corr[2][p] * corr[2][q]  # noqa: E731
    g = (col_dot(0, 0), col_dot(0, 1), col_dot(1, 1), col_dot(0, 2), col_dot(1, 2), col_dot(2, 2))
    gxx, gxy, gyy, gxz, gyz, gzz = g
    mean = ((gxx + gyy) + gzz) / f64(3.0)
    minors = (((((gyy * gzz - gyz * gyz) + gxx * gzz) - gxz * gxz) + gxx * gyy) - gxy * gxy) / f64(3.0)
    det_sq = det * det
    lam = [mean, mean, mean]
    A = [[f64(v) for v in row] for row in ident]          # A[c]: column c of the eigenvector basis
    rot = [[f64(v) for v in row] for row in ident]
    shift = [zero] * 3
    translate = lambda: [((centre_b[i] - rot[i][0] * centre_a[0]) - rot[i][1] * centre_a[1]) - rot[i][2] * centre_a[2] for i in range(3)]  # noqa: E731
    basis = True
    if mean > 0:
        disc = mean * mean - minors
        half = (mean * minors - det_sq) / f64(2.0) - mean * disc
        if disc > 0:
            root = _sqrt(disc)
            under = disc * disc * disc - half * half
            if under < 0.0:
                under = zero
            angle = f64(math.atan2(_sqrt(under), -half)) / f64(3.0)
            c, s = root * _cos(angle), root * f64(1.73205080756888) * _sin(angle)
            lam = [(mean + c) + c, (mean - c) + s, (mean - c) - s]
            A[0], A[2] = _eigenvector(g, lam[0]), _eigenvector(g, lam[2])
            if (lam[0] - lam[1]) > (lam[1] - lam[2]):          # the better separated eigenvalue's vector is kept
                A[2], basis = _orthonormal_pair(A[0], A[2])
            else:
                A[0], basis = _orthonormal_pair(A[2], A[0])
            if basis:
                A[1] = _cross(A[2], A[0])
        if basis:
            B = [_unit_or_zero([(corr[i][0] * A[c][0] + corr[i][1] * A[c][1]) + corr[i][2] * A[c][2] for i in range(3)]) for c in range(2)]
            B[1], ok = _orthonormal_pair(B[0], B[1])
            if ok:
                B.append(_cross(B[0], B[1]))
                # the reference's rotation is a float matrix: every element is rounded when stored, and the translation reads the rounded values
                rot = [[f64(f32((B[0][i] * A[0][j] + B[1][i] * A[1][j]) + B[2][i] * A[2][j])) for j in range(3)] for i in range(3)]
            shift = translate()
    else:
        shift = translate()
    sv = [_sqrt(zero if v < 0 else v) for v in lam]
    trace = -sv[2] if det < 0.0 else sv[2]
    trace = (trace + sv[1]) + sv[0]
    residual = (spread - trace) - trace
    if residual < 0.0:
        residual = zero
    return f32(residual), [f32(v) for v in shift], [[f32(v) for v in row] for row in rot]


def kabsch_fast(x, y, stats=None):
    """KabschFast"""
    n = x.shape[1]
    if n >= 1:
        rms, t, u = kabsch_avx(x, y)
        if not any(v != v for row in u for v in row):
            return rms, t, u
    # n == 0: 1 / 0 = inf, 0 * inf = NaN in every centred sum, so the rotation is NaN as well
    if stats is not None:
        stats["fallback"] = stats.get("fallback", 0) + 1
    return kabsch_classic(x, y)


def score_fun8(xtm, ytm, t, u, d, score_d8, d0, stats=None):
    """do_rotation + score_fun8 (Lnorm = n) -> (selected indices, score float32)"""
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
    return sel, f32(score_sum / f32(n))


def frag_lengths(n):
    lmin = min(4, n)
    out = []
    i = 0
    while i < 5:
        L = int(n / math.pow(2.0, float(i)))
        if L <= lmin:
            out.append(lmin)
            break
        out.append(L)
        i += 1
    if i == 5:
        out.append(lmin)
    return out


def frag_starts(n, L, step=40):
    imax = n - L
    out, i = [], 0
    while True:
        out.append(i)
        if i < imax:
            i = min(i + step, imax)
        else:
            break
    return out


def search(xtm, ytm, d0_search, score_d8, d0, stats=None):
    """TMscore8_search_standard(simplify_step 40) -> score_max float32"""
    n = xtm.shape[1]
    score_max = f32(-1)
    if n == 0:
        return score_max          # 0 / 0 = NaN never exceeds -1
    d0_search = f32(d0_search)
    for L in frag_lengths(n):
        for i in frag_starts(n, L):
            rms, t, u = kabsch_fast(xtm[:, i:i + L], ytm[:, i:i + L], stats)
            sel, score = score_fun8(xtm, ytm, t, u, f32(d0_search - f32(1)), score_d8, d0, stats)
            if score > score_max:
                score_max = score
            d = f32(d0_search + f32(1))
            for _ in range(20):
                prev = sel
                rms, t, u = kabsch_fast(xtm[:, sel], ytm[:, sel], stats)
                sel, score = score_fun8(xtm, ytm, t, u, d, score_d8, d0, stats)
                if score > score_max:
                    score_max = score
                if len(sel) == len(prev) and np.array_equal(sel, prev):
                    break
    return score_max


def tm_raw(xtm, ytm, norm_len, stats=None):
    """what the device returns: (pairs, score_max of standard_TMscore, score_max of detailed_search_standard, rmsd), floats as float32"""
    n = xtm.shape[1]
    with np.errstate(all="ignore"):
        _, score_d8, d0, d0_search = search_params(norm_len)
        d0s = standard_params(norm_len)
        rmsd = kabsch_fast(xtm, ytm, stats)[0]
        s1 = search(xtm, ytm, d0s, score_d8, d0s, stats)
        s2 = search(xtm, ytm, d0_search, score_d8, d0, stats)
    return n, s1, s2, rmsd


def tm_finish(n, s1, s2, norm_len):
    """-> the TM-score as a Python float (double)"""
    with np.errstate(all="ignore"):
        lnorm = f32(norm_len)
        a = f64(f32(s1)) * f64(n) / (f64(1.0) * f64(lnorm))
        b = f64(f32(f32(f32(s2) * f32(n)) / f32(int(lnorm))))
        # std::max(TM, TMalnScore) = (TM < TMalnScore) ? TMalnScore : TM
        return float(a if b < a else b)


def tmscore(qc, tc, q_start, t_start, backtrace, norm_len, stats=None):
    """TMaligner::computeTMscore(..., computeExactScore = false) -> (tmscore, rmsd) as Python floats"""
    xtm, ytm = pairs(qc, tc, q_start, t_start, backtrace)
    n, s1, s2, rmsd = tm_raw(xtm, ytm, norm_len, stats)
    return tm_finish(n, s1, s2, norm_len), float(rmsd)


def normalization(mode, aln_len, q_len, t_len):
    """TMaligner::normalization"""
    return aln_len if mode == 0 else (q_len if mode == 1 else t_len)


def sstr(v):
    """SSTR(double): %.3E; NaN and infinity as the reference prints them"""
    v = float(v)
    if v != v:
        return "-NAN" if math.copysign(1.0, v) < 0 else "NAN"
    if math.isinf(v):
        return "-INF" if v < 0 else "INF"
    return "%.3E" % v

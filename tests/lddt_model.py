"""tests/lddt_model.py -- an independent float32 model of the reference's LDDT (TEST INFRASTRUCTURE, numpy only).

Written from F/src/commons/LDDT.{h,cpp} and Coordinate16.h, not from this repository's kernels:

  * decode()        Coordinate16::read: raw float32 when the entry holds 3 * L floats, else per axis an int32 start and L - 1 int16
                    differences, value = (start + running sum) / 1000.0f.
  * dist()          three float subtractions, fma(d0, d0, 0), fma(d1, d1, .), fma(d2, d2, .), correctly rounded sqrt -- what the reference BINARY
                    computes (gcc -O3 -mfma contracts `D2 += d * d`).  fused=False gives the C++ text's unfused form, for the fixtures that tell them apart.
  * norm            1 / #{r != c : dist(q_r, q_c) < 15}, +inf without neighbours (LDDTCalculator::initQuery).
  * per column      over ALL other aligned columns with query distance < 15 (the reference's grid visits exactly these, each pair once, and adds the
                    pair's score to both columns; sums of multiples of 0.25 are exact): 0.25 * ((d<0.5)+(d<1)+(d<2)+(d<4)), d = |dist_q - dist_t|;
                    times norm[query residue]; 0 * inf = NaN.
  * average()       LDDTScoreResult: NaN columns skipped and subtracted from scoreLength, float sum in column order, (double)(sum / (float) scoreLength).
  * write_float3()  structureconvertalis.cpp writeFloat3: (unsigned)(val * 1000.0 + 0.5), three decimals.

The fused multiply-add is exact: the product of two float32 is exact in float64, the sum with the addend is rounded to ODD in float64 (TwoSum error term) and
then to float32 -- rounding to odd at 53 bits followed by rounding to nearest at 24 bits equals one rounding to nearest.
"""
import math

import numpy as np

f32 = np.float32
CUTOFF = f32(15.0)


def decode(entry, L):
    """Coordinate16::read -> float32 [3, L]"""
    entry = bytes(entry)
    if len(entry) >= 3 * L * 4:
        return np.frombuffer(entry[:12 * L], "<f4").reshape(3, L).copy()
    out = np.zeros((3, L), f32)
    p = 0
    for axis in range(3):
        start = int(np.frombuffer(entry[p:p + 4], "<i4")[0])
        p += 4
        diffs = np.frombuffer(entry[p:p + 2 * (L - 1)], "<i2").astype(np.int64)
        p += 2 * (L - 1)
        vals = start + np.concatenate([[0], np.cumsum(diffs)])
        # int32 arithmetic in the reference; |coordinates| * 1000 stay far below 2^31 in every fixture
        out[axis] = vals.astype(np.int32).astype(f32) / f32(1000.0)
    return out


def encode16(xyz):
    """the compressed entry form for float32 [3, L] coordinates whose * 1000 values are integers and whose steps fit int16 (fixture writer)"""
    out = b""
    for axis in range(3):
        v = np.rint(np.asarray(xyz[axis], np.float64) * 1000.0).astype(np.int64)
        d = np.diff(v)
        assert np.all(np.abs(d) < 32768)
        out += np.int32(v[0]).tobytes() + d.astype("<i2").tobytes()
    return out


def fma32(a, b, c):
    """correctly rounded float32 fma of float32 arrays"""
    a, b, c = (np.asarray(x, f32).astype(np.float64) for x in (a, b, c))
    p = a * b                                   # exact: 24 + 24 bits
    s = np.asarray(p + c, np.float64)
    bb = s - p
    err = (p - (s - bb)) + (c - bb)             # TwoSum: p + c = s + err exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)    # round to odd: an inexact sum whose last bit is even moves one step towards the lost part
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def dist(A, B, fused=True):
    """A, B: float32 [..., 3] -> float32 [...]"""
    d = (np.asarray(A, f32) - np.asarray(B, f32)).astype(f32)
    if fused:
        acc = fma32(d[..., 0], d[..., 0], np.zeros_like(d[..., 0]))
        acc = fma32(d[..., 1], d[..., 1], acc)
        acc = fma32(d[..., 2], d[..., 2], acc)
    else:
        acc = (d[..., 0] * d[..., 0]).astype(f32)
        acc = (acc + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32)
        acc = (acc + (d[..., 2] * d[..., 2]).astype(f32)).astype(f32)
    return np.sqrt(acc).astype(f32)


def pairwise(P, fused=True, block=256):
    """P float32 [n, 3] -> all-pairs distance matrix float32 [n, n], computed in row blocks (memory)"""
    n = len(P)
    D = np.empty((n, n), f32)
    for r0 in range(0, n, block):
        D[r0:r0 + block] = dist(P[r0:r0 + block, None, :], P[None, :, :], fused)
    return D


def query_norm(qc, fused=True):
    """qc float32 [3, L] -> (norm [L], query distance matrix [L, L])"""
    q = np.ascontiguousarray(np.asarray(qc, f32).T)
    Dq = pairwise(q, fused)
    close = (Dq < CUTOFF) & ~np.eye(len(q), dtype=bool)
    cnt = close.sum(1).astype(f32)
    with np.errstate(divide="ignore"):
        norm = np.where(cnt != 0, f32(1.0) / np.where(cnt != 0, cnt, f32(1)), f32(np.inf)).astype(f32)
    return norm, Dq


def expand(cigar):
    """'3M2I' -> 'MMMII'; a string of M / I / D is returned as it is"""
    if not any(ch.isdigit() for ch in cigar):
        return cigar
    out, n = [], ""
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            out.append(ch * int(n))
            n = ""
    return "".join(out)


def aligned(q_start, t_start, backtrace):
    """LDDTCalculator::constructAlignHashes -> (query index, target index) per aligned column"""
    a2q, a2t, qi, ti = [], [], q_start, t_start
    for ch in backtrace:
        if ch == "M":
            a2q.append(qi); a2t.append(ti); qi += 1; ti += 1
        elif ch == "D":
            ti += 1
        elif ch == "I":
            qi += 1
    return np.array(a2q, np.int64), np.array(a2t, np.int64)


def columns(qc, tc, q_start, t_start, backtrace, fused=True, norm_dq=None):
    """reduce_score[] of LDDTCalculator::calculateLddtScores: float32 per aligned column, NaN where the query residue has no neighbour"""
    norm, Dq = norm_dq if norm_dq is not None else query_norm(qc, fused)
    a2q, a2t = aligned(q_start, t_start, expand(backtrace))
    n = len(a2q)
    if n == 0:
        return np.zeros(0, f32)
    t = np.ascontiguousarray(np.asarray(tc, f32).T)[a2t]
    dq = Dq[np.ix_(a2q, a2q)]
    dt = pairwise(t, fused)
    dl = np.abs((dq - dt).astype(f32))
    quarters = (dl < f32(0.5)).astype(np.int64) + (dl < f32(1.0)) + (dl < f32(2.0)) + (dl < f32(4.0))
    scored = (dq < CUTOFF) & ~np.eye(n, dtype=bool)
    red = (np.where(scored, quarters, 0).sum(1).astype(f32) * f32(0.25)).astype(f32)
    with np.errstate(invalid="ignore"):
        return (red * norm[a2q]).astype(f32)


def average(cols):
    """LDDTScoreResult -> (avgLddtScore as a Python float, scoreLength)"""
    s, n = f32(0.0), len(cols)
    for v in cols:
        if np.isnan(v):
            n -= 1
        else:
            s = f32(s + f32(v))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(f32(s) / f32(n)), n


def write_float3(v):
    v = f32(v)
    sign = ""
    if v < 0:
        sign, v = "-", -v
    iv = int(float(v) * 1000.0 + 0.5)
    return "%s%d.%03d" % (sign, iv // 1000, iv % 1000)


def lddtfull(cols):
    """the lddtfull column: the FIRST scoreLength per-column values (NaN shown as 0), comma separated (structureconvertalis.cpp:1099-1107)"""
    _, n = average(cols)
    vals = [f32(0.0) if np.isnan(v) else v for v in cols]
    return ",".join(write_float3(v) for v in vals[:n])


def lddt_text(avg):
    """SSTR(double) of the reference: %.3E; a NaN with its sign (0 / 0 on x86 is the negative default NaN, and fmt / glibc print the sign)"""
    if avg != avg:
        return "-NAN" if math.copysign(1.0, avg) < 0 else "NAN"
    return "%.3E" % avg

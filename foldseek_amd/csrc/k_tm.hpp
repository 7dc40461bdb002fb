// k_tm.hpp -- approximate TM-score of accepted hits on the device (reference: F/lib/tmalign/{TMalign.cpp,Kabsch.h,basic_fun.h},
// TMaligner::computeAppoximateTMscore; C ABI: fsgpu_tm_batch in fsgpu_tm.hip).
//
// The reference builds its TM library without floating-point contraction, so every value is a chain of plain IEEE operations in source order, and the
// orders are part of the result:
//   * rmsd_uncentered_avx keeps every sum in FOUR serial float chains (selected pair p goes to chain p mod 4, both 128-bit halves of a chunk of 8 feed
//     the same chain, low half first), combined (l0 + l1) + (l2 + l3) by its hadd tree; the sum of squares takes c1x^2 of both halves and then the five
//     other squares of both halves per chunk.  Centring in float, the 3x3 eigen step and the quaternion matrix in double, casts to float last.
//   * score_fun8 sums 1 / (1 + di / d0^2), masked by di < score_d8^2, left to right in float.
//   * A NaN rotation falls back to the classical double-precision Kabsch().
// None of these sums can be split, so the parallelism is across hits x searches x fragment starts: one wave per (hit, search), one lane per fragment start
// (TMscore8_search_standard's `while (1)` body, a start's up to 21 superpositions run serially in its lane).  A hit's pairs sit in LDS; a lane keeps its
// selected subset as a bitmask, word w of lane l at [w * 64 + l] (two masks: the subset being superposed and the one being selected).  Hits with more
// than kTmLdsPairs pairs read the pairs from the global workspace and keep their masks there.
//
//   k_tm_pairs   one workgroup per hit: backtrace -> aligned pairs ('M' pairs, 'I' advances the query, ANYTHING else the target), gathered as
//                pairs[6][n] = target x y z, query x y z (xtm / ytm of the reference)
//   k_tm_search  grid (hits, 3): y = 0 standard_TMscore's search, y = 1 detailed_search_standard's, y = 2 the KabschFast over all pairs (rmsd)
//
// This object is compiled without contraction and with correctly rounded float division and square root (Makefile); double + - * / sqrt are IEEE on
// gfx950; float denormals are kept (HIP's default).  atan2 / cos / sin in double come from the device library: see DESIGN.md for what that allows.
// The functions are __host__ __device__ so that a host build of the same text can be stepped through; libfsgpu.so never calls them on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace fs {

#pragma clang fp contract(off)

constexpr int kTmPairsBlock = 256;        // lanes of a k_tm_pairs workgroup
constexpr int kTmLdsPairs = 1024;         // pairs of a hit held in LDS: 6 x 4 KB of coordinates + 2 x 32 words x 64 lanes of masks = 40 KB
constexpr int kTmLdsWords = kTmLdsPairs / 32;
constexpr int kTmStep = 40;               // simplify_step of both searches
constexpr int kTmRounds = 20;             // n_it

struct TmQuery { uint32_t cOff, L; };     // cOff: float offset of x[L] y[L] z[L] in the query blob
struct TmTask {
    uint32_t query, tLen;
    uint64_t tOff;                        // float offset of x[tLen] y[tLen] z[tLen] in the target blob
    int32_t qStart, dbStart;
    uint64_t btOff;
    uint32_t btLen, nPairs;               // nPairs: 'M' characters of the backtrace (counted by the host: sizes the workspace slices)
    uint64_t pairOff;                     // float offset of pairs[6][nPairs] in the pair workspace
    uint64_t maskOff;                     // word offset of this hit's masks [2 searches][2][words][64] in the mask workspace (hits beyond kTmLdsPairs)
    uint32_t slot;                        // index of the task in the caller's order
    float scoreD8;
    float d0[2], d0Search[2];             // [0] standard_TMscore, [1] detailed_search_standard
    uint32_t pad;
};
struct TmArgs {
    const TmQuery *queries;
    const TmTask *tasks;
    const float *qc, *tc;
    const char *bt;
    float *pairs;
    uint32_t *masks;
    float *out;                           // [3][nt]: score_max of the two searches, rmsd
    int32_t *nPairs;                      // [nt]
    uint32_t nt;
};

// a hit's pairs and one lane's two masks
struct TmView {
    const float *c;                       // c[a * n + i], a = target x y z, query x y z
    uint32_t n, words;
    uint32_t *m[2];
    uint32_t ms;                          // stride between the words of a mask
};

#define TM_HD __host__ __device__ inline

// walks the set bits of a mask in ascending order
struct TmIter {
    const uint32_t *m;
    uint32_t ms, words, w, bits;
    TM_HD TmIter(const uint32_t *mask, uint32_t stride, uint32_t nWords) : m(mask), ms(stride), words(nWords), w(0), bits(nWords ? mask[0] : 0u) {}
    TM_HD int next() {
        while (!bits) {
            if (w + 1 >= words) return -1;
            w++;
            bits = m[(size_t) w * ms];
        }
        const int b = __builtin_ctz(bits);
        bits &= bits - 1;
        return (int) (w * 32 + b);
    }
};

TM_HD bool tmIsNan(float v) { return v != v; }

// The rotation of the quaternion fit (rmatrix<double> of the reference): the unit quaternion is the eigenvector of the symmetric 4 x 4 key matrix K
// of the correlation matrix `c` for the eigenvalue `ev`, read off as cofactors of (K - ev I) along its first row.  Basis (w, x, y, z); only the
// operation order is the reference's.
struct TmQuat { double w, x, y, z; };

TM_HD TmQuat tmKeyEigenvector(double ev, const double c[3][3]) {
    const double kwx = c[1][2] - c[2][1], kwy = c[2][0] - c[0][2], kwz = c[0][1] - c[1][0];
    const double kxy = c[0][1] + c[1][0], kxz = c[2][0] + c[0][2], kyz = c[1][2] + c[2][1];
    const double kxx = ((c[0][0] - c[1][1]) - c[2][2]) - ev;
    const double kyy = ((-c[0][0] + c[1][1]) - c[2][2]) - ev;
    const double kzz = ((-c[0][0] - c[1][1]) + c[2][2]) - ev;
    // 2 x 2 minors of the lower right block and of the first row against it
    const double mYyZz = kyy * kzz - kyz * kyz, mXyZz = kxy * kzz - kxz * kyz, mXyYz = kxy * kyz - kxz * kyy;
    const double mWyYz = kwy * kyz - kwz * kyy, mWyZz = kwy * kzz - kwz * kyz, mWyXz = kwy * kxz - kwz * kxy;
    TmQuat q;
    q.w = (kxx * mYyZz - kxy * mXyZz) + kxz * mXyYz;
    q.x = (-kwx * mYyZz + kxy * mWyZz) - kxz * mWyYz;
    q.y = (kwx * mXyZz - kxx * mWyZz) + kxz * mWyXz;
    q.z = (-kwx * mXyYz + kxx * mWyYz) - kxy * mWyXz;
    return q;
}

TM_HD void tmQuatRotation(const TmQuat &q, double rot[3][3]) {
    const double scale = 1.0 / (((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);          // an unnormalised quaternion: every product is scaled
    const double ww = q.w * q.w * scale, xx = q.x * q.x * scale, yy = q.y * q.y * scale, zz = q.z * q.z * scale;
    const double xy = q.x * q.y * scale, wz = q.w * q.z * scale, zx = q.z * q.x * scale;
    const double wy = q.w * q.y * scale, yz = q.y * q.z * scale, wx = q.w * q.x * scale;
    rot[0][0] = ((ww + xx) - yy) - zz; rot[0][1] = 2.0 * (xy + wz); rot[0][2] = 2.0 * (zx - wy);
    rot[1][0] = 2.0 * (xy - wz); rot[1][1] = ((ww - xx) + yy) - zz; rot[1][2] = 2.0 * (yz + wx);
    rot[2][0] = 2.0 * (zx + wy); rot[2][1] = 2.0 * (yz - wx); rot[2][2] = ((ww - xx) - yy) + zz;
}

TM_HD void tmRmatrix(double ev, const double c[3][3], double rot[3][3]) { tmQuatRotation(tmKeyEigenvector(ev, c), rot); }

TM_HD float tmDot4(float a, float b, float c) { return (0.0f + a) + (b + c); }

// kabsch_quat_soa_avx / rmsd_uncentered_avx over the nSel >= 1 pairs of `mask`; the result may hold NaN
TM_HD void tmKabschAvx(const TmView &v, const uint32_t *mask, uint32_t nSel, float &rmsOut, float t[3], float u[3][3]) {
    // 0-5 s1x s1y s1z s2x s2y s2z, 6-14 sxx sxy sxz syx syy syz szx szy szz, 15 ssq; four chains each
    float a[16][4];
#pragma unroll
    for (int s = 0; s < 16; s++)
#pragma unroll
        for (int j = 0; j < 4; j++) a[s][j] = 0.0f;
    TmIter it(mask, v.ms, v.words);
    const size_t n = v.n;
    for (;;) {
        float b[6][8];
        int got = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int idx = it.next();
            if (idx >= 0) {
                got++;
#pragma unroll
                for (int ax = 0; ax < 6; ax++) b[ax][k] = v.c[ax * n + idx];
            } else {
#pragma unroll
                for (int ax = 0; ax < 6; ax++) b[ax][k] = 0.0f;
            }
        }
        if (!got) break;
        float t1[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float c1x = b[0][k], c1y = b[1][k], c1z = b[2][k], c2x = b[3][k], c2y = b[4][k], c2z = b[5][k];
            const int j = k & 3;          // k = 0..3 is the low half of the chunk, 4..7 the high half: per chain, low before high
            a[0][j] += c1x; a[1][j] += c1y; a[2][j] += c1z; a[3][j] += c2x; a[4][j] += c2y; a[5][j] += c2z;
            a[6][j] += c1x * c2x; a[7][j] += c1x * c2y; a[8][j] += c1x * c2z;
            a[9][j] += c1y * c2x; a[10][j] += c1y * c2y; a[11][j] += c1y * c2z;
            a[12][j] += c1z * c2x; a[13][j] += c1z * c2y; a[14][j] += c1z * c2z;
            a[15][j] += c1x * c1x;
            t1[k] = ((c2x * c2x + c2z * c2z) + (c2y * c2y + c1y * c1y)) + c1z * c1z;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) { a[15][j] += t1[j]; a[15][j] += t1[4 + j]; }
        if (got < 8) break;
    }
    float S[16];
#pragma unroll
    for (int s = 0; s < 16; s++) S[s] = (a[s][0] + a[s][1]) + (a[s][2] + a[s][3]);
    const float fnat = (float) nSel, inv = 1.0f / fnat;
    const float s1x = S[0], s1y = S[1], s1z = S[2], s2x = S[3], s2y = S[4], s2z = S[5];
    const float n1x = s1x * inv, n1y = s1y * inv, n1z = s1z * inv, n2x = s2x * inv, n2y = s2y * inv, n2z = s2z * inv, nssq = S[15] * inv;
    const float sxx = S[6] - n1x * s2x, sxy = S[7] - n1x * s2y, sxz = S[8] - n1x * s2z;
    const float syx = S[9] - n1y * s2x, syy = S[10] - n1y * s2y, syz = S[11] - n2z * s1y;
    const float szx = S[12] - n2x * s1z, szy = S[13] - n2y * s1z, szz = S[14] - n2z * s1z;
    const float r0r0 = tmDot4(sxx * sxx, sxy * sxy, sxz * sxz), r0r1 = tmDot4(sxx * syx, sxy * syy, sxz * syz), r1r1 = tmDot4(syx * syx, syy * syy, syz * syz);
    const float r0r2 = tmDot4(sxx * szx, sxy * szy, sxz * szz), r1r2 = tmDot4(syx * szx, syy * szy, syz * szz), r2r2 = tmDot4(szx * szx, szy * szy, szz * szz);
    const float detf = tmDot4(sxx * (syy * szz - szy * syz), sxy * (syz * szx - szz * syx), sxz * (syx * szy - szx * syy));
    const double ssq = (double) (((((((nssq - n1x * n1x) - n1y * n1y) - n1z * n1z) - n2x * n2x) - n2y * n2y) - n2z * n2z) * fnat);
    const double det = (double) detf, detsq = det * det;
    const double rr0 = r0r0, rr1 = r0r1, rr2 = r1r1, rr3 = r0r2, rr4 = r1r2, rr5 = r2r2;
    const double inv3 = 1.0 / 3.0;
    const double spur = ((rr0 + rr2) + rr5) * inv3;
    const double cof = (((((rr2 * rr5 - rr4 * rr4) + rr0 * rr5) - rr3 * rr3) + rr0 * rr2) - rr1 * rr1) * inv3;
    double e0 = spur, e1 = spur, e2 = spur;
    const double h = (spur > 0) ? spur * spur - cof : -1.0;
    if (h > 0) {
        const double g = (spur * cof - detsq) * 0.5 - spur * h;
        const double sqrth = sqrt(h);
        double d1 = h * h * h - g * g;
        d1 = (d1 < 0) ? atan2(0.0, -g) * inv3 : atan2(sqrt(d1), -g) * inv3;
        const double cth = sqrth * cos(d1);
        const double sth = sqrth * 1.732050807568877 * sin(d1);
        e0 += cth + cth;
        e1 += -cth + sth;
        e2 += -cth - sth;
    }
    e0 = (e0 < 0) ? 0 : sqrt(e0);
    e1 = (e1 < 0) ? 0 : sqrt(e1);
    e2 = (e2 < 0) ? 0 : sqrt(e2);
    const double d = (det < 0) ? (e0 + e1) - e2 : (e0 + e1) + e2;
    double rms = ((ssq - d) - d) * (1.0 / (double) nSel);
    rms = (rms > 1e-8) ? sqrt(rms) : 0.0;
    const double mr[3][3] = {{sxx, sxy, sxz}, {syx, syy, syz}, {szx, szy, szz}};
    double ud[3][3];
    tmRmatrix(d, mr, ud);
    const float c1c[3] = {n1x, n1y, n1z}, c2c[3] = {n2x, n2y, n2z};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float m0 = (float) (-ud[0][k]), m1 = (float) (-ud[1][k]), m2 = (float) (-ud[2][k]);
        t[k] = (m0 * c1c[0] + m1 * c1c[1]) + (m2 * c1c[2] + c2c[k] * 1.0f);
#pragma unroll
        for (int j = 0; j < 3; j++) u[k][j] = (float) ud[j][k];
    }
    rmsOut = (float) rms;
}

// ---- the double-precision superposition behind KabschFast's NaN fallback (the reference's Kabsch(), mode 2) ----
// Eigen decomposition of G = C^T C for the correlation matrix C of the selected pairs: eigenvalues by the trigonometric solution of the cubic,
// the eigenvectors of the largest and the smallest one as columns of adj(lambda I - G), a right-handed basis A from them, B = normalised C A, and the
// rotation B A^T.  Written as small helpers of this project's own; what is kept from the reference is the ORDER of the floating-point operations, its
// thresholds (1e-8 on squared lengths and cofactors, 0.01 on the norm left after the projection) and its habit of taking |x| in float in some places.
struct TmSym3 { double xx, xy, yy, xz, yz, zz; };          // a symmetric 3 x 3 matrix, packed by columns of the upper triangle

TM_HD double tmAbsAsFloat(double v) { return (double) fabsf((float) v); }          // the reference calls fabsf() on doubles here

// v / |v|, or the zero vector when |v|^2 is not above 1e-8
TM_HD void tmUnitOrZero(double v[3]) {
    double len2 = 0.0;
    for (int i = 0; i < 3; i++) len2 = len2 + v[i] * v[i];
    const double s = len2 > 0.00000001 ? 1.0 / sqrt(len2) : 0.0;
    for (int i = 0; i < 3; i++) v[i] = v[i] * s;
}

TM_HD void tmCross(const double x[3], const double y[3], double out[3]) {
    out[0] = x[1] * y[2] - y[1] * x[2];
    out[1] = x[2] * y[0] - y[2] * x[0];
    out[2] = x[0] * y[1] - y[0] * x[1];
}

// the eigenvector of G for lambda: the column of adj(lambda I - G) with the largest diagonal entry, normalised (zero when it vanishes)
TM_HD void tmEigenvector(const TmSym3 &g, double lambda, double out[3]) {
    TmSym3 adj;
    adj.xx = (lambda - g.yy) * (lambda - g.zz) - g.yz * g.yz;
    adj.xy = (lambda - g.zz) * g.xy + g.xz * g.yz;
    adj.yy = (lambda - g.xx) * (lambda - g.zz) - g.xz * g.xz;
    adj.xz = (lambda - g.yy) * g.xz + g.xy * g.yz;
    adj.yz = (lambda - g.xx) * g.yz + g.xy * g.xz;
    adj.zz = (lambda - g.xx) * (lambda - g.yy) - g.xy * g.xy;
    double *e[6] = {&adj.xx, &adj.xy, &adj.yy, &adj.xz, &adj.yz, &adj.zz};
    for (int i = 0; i < 6; i++) if (tmAbsAsFloat(*e[i]) <= 0.00000001) *e[i] = 0.0;
    int col;
    if (tmAbsAsFloat(adj.xx) >= fabs(adj.yy)) col = tmAbsAsFloat(adj.xx) < fabs(adj.zz) ? 2 : 0;
    else col = tmAbsAsFloat(adj.yy) >= tmAbsAsFloat(adj.zz) ? 1 : 2;
    if (col == 0) { out[0] = adj.xx; out[1] = adj.xy; out[2] = adj.xz; }
    else if (col == 1) { out[0] = adj.xy; out[1] = adj.yy; out[2] = adj.yz; }
    else { out[0] = adj.xz; out[1] = adj.yz; out[2] = adj.zz; }
    tmUnitOrZero(out);
}

// Makes `second` a unit vector orthogonal to the unit vector `first`: the projection is removed; if less than 0.01 of squared length is left, `second`
// is rebuilt in the plane of the two larger components of `first`.  False when that fails too (`first` is not a usable axis).
TM_HD bool tmOrthonormalPair(const double first[3], double second[3]) {
    const double along = (first[0] * second[0] + first[1] * second[1]) + first[2] * second[2];
    double left = 0.0;
    for (int i = 0; i < 3; i++) {
        second[i] = second[i] - along * first[i];
        left = left + second[i] * second[i];
    }
    if (!(left <= 0.01)) {          // (a NaN takes this branch)
        const double s = 1.0 / sqrt(left);
        for (int i = 0; i < 3; i++) second[i] = second[i] * s;
        return true;
    }
    // the component of `first` that is smallest in magnitude (the last one among equals); it cannot stay unset: |first[i]| <= 1 for a unit or zero vector
    int small = 0;
    double least = 1.0;
    for (int i = 0; i < 3; i++) {
        if (least < fabs(first[i])) continue;
        least = fabs(first[i]);
        small = i;
    }
    const int k = (small + 1) % 3, l = (small + 2) % 3;
    const double len = sqrt(first[k] * first[k] + first[l] * first[l]);
    if (!(len > 0.01)) return false;
    second[small] = 0.0;
    second[k] = -first[l] / len;
    second[l] = first[k] / len;
    return true;
}

// Kabsch(x, y, n, mode 2) of the reference over the pairs of `mask`: rms (a SUM of squares there, not a root mean), translation and rotation
TM_HD void tmKabschClassic(const TmView &v, const uint32_t *mask, uint32_t nSel, float &rmsOut, float t[3], float u[3][3]) {
    rmsOut = 0.0f;
    for (int i = 0; i < 3; i++) {
        t[i] = 0.0f;
        for (int j = 0; j < 3; j++) u[i][j] = (i == j) ? 1.0f : 0.0f;
    }
    if (nSel < 1) return;
    const size_t n = v.n;
    // first moments and the nine cross sums, serial float chains in pair order
    float sumA[3] = {0, 0, 0}, sumB[3] = {0, 0, 0}, cross[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};          // cross[i][j] = sum a[i] * b[j]
    {
        TmIter it(mask, v.ms, v.words);
        for (int idx = it.next(); idx >= 0; idx = it.next()) {
            float a[3], b[3];
            for (int ax = 0; ax < 3; ax++) { a[ax] = v.c[ax * n + idx]; b[ax] = v.c[(3 + ax) * n + idx]; }
            for (int ax = 0; ax < 3; ax++) { sumA[ax] += a[ax]; sumB[ax] += b[ax]; }
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < 3; i++) cross[i][j] += a[i] * b[j];
        }
    }
    const double count = (double) (int) nSel;
    double sA[3], sB[3], centreA[3], centreB[3];
    for (int i = 0; i < 3; i++) { sA[i] = sumA[i]; sB[i] = sumB[i]; centreA[i] = sA[i] / count; centreB[i] = sB[i] / count; }
    // spread of both sets about their centroids, in double, one term per pair and axis
    double spread = 0;
    {
        TmIter it(mask, v.ms, v.words);
        for (int idx = it.next(); idx >= 0; idx = it.next())
            for (int ax = 0; ax < 3; ax++) {
                const double pa = v.c[ax * n + idx], pb = v.c[(3 + ax) * n + idx];
                spread += (pa - centreA[ax]) * (pa - centreA[ax]) + (pb - centreB[ax]) * (pb - centreB[ax]);
            }
    }
    double corr[3][3];          // corr[j][i]: b axis j against a axis i, centred
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) corr[j][i] = (double) cross[i][j] - sA[i] * sB[j] / count;
    const double det = (corr[0][0] * (corr[1][1] * corr[2][2] - corr[1][2] * corr[2][1]) - corr[0][1] * (corr[1][0] * corr[2][2] - corr[1][2] * corr[2][0])) +
                       corr[0][2] * (corr[1][0] * corr[2][1] - corr[1][1] * corr[2][0]);
    auto colDot = [&](int p, int q) { return (corr[0][p] * corr[0][q] + corr[1][p] * corr[1][q]) + corr[2][p] * corr[2][q]; };
    TmSym3 g;
    g.xx = colDot(0, 0); g.xy = colDot(0, 1); g.yy = colDot(1, 1); g.xz = colDot(0, 2); g.yz = colDot(1, 2); g.zz = colDot(2, 2);
    const double mean = ((g.xx + g.yy) + g.zz) / 3.0;
    const double minors = (((((g.yy * g.zz - g.yz * g.yz) + g.xx * g.zz) - g.xz * g.xz) + g.xx * g.yy) - g.xy * g.xy) / 3.0;
    const double detSq = det * det;
    double lambda[3] = {mean, mean, mean};
    double A[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};          // A[c]: column c of the eigenvector basis
    double rot[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, shift[3] = {0, 0, 0};
    bool basis = true;
    if (mean > 0) {
        const double disc = mean * mean - minors;
        const double half = (mean * minors - detSq) / 2.0 - mean * disc;
        if (disc > 0) {
            const double root = sqrt(disc);
            double under = disc * disc * disc - half * half;
            if (under < 0.0) under = 0.0;
            const double angle = atan2(sqrt(under), -half) / 3.0;
            const double c = root * cos(angle), s = root * 1.73205080756888 * sin(angle);
            lambda[0] = (mean + c) + c;
            lambda[1] = (mean - c) + s;
            lambda[2] = (mean - c) - s;
            tmEigenvector(g, lambda[0], A[0]);
            tmEigenvector(g, lambda[2], A[2]);
            // the better separated eigenvalue's vector is kept, the other one is made orthogonal to it
            const bool keepFirst = (lambda[0] - lambda[1]) > (lambda[1] - lambda[2]);
            basis = keepFirst ? tmOrthonormalPair(A[0], A[2]) : tmOrthonormalPair(A[2], A[0]);
            if (basis) tmCross(A[2], A[0], A[1]);
        }
        if (basis) {
            double B[3][3];
            for (int c = 0; c < 2; c++) {
                for (int i = 0; i < 3; i++) B[c][i] = (corr[i][0] * A[c][0] + corr[i][1] * A[c][1]) + corr[i][2] * A[c][2];
                tmUnitOrZero(B[c]);
            }
            if (tmOrthonormalPair(B[0], B[1])) {
                tmCross(B[0], B[1], B[2]);
                // the reference's rotation is a float matrix: every element is rounded when stored, and the translation reads the rounded values
                for (int i = 0; i < 3; i++)
                    for (int j = 0; j < 3; j++) rot[i][j] = (double) (float) ((B[0][i] * A[0][j] + B[1][i] * A[1][j]) + B[2][i] * A[2][j]);
            }
            for (int i = 0; i < 3; i++) shift[i] = ((centreB[i] - rot[i][0] * centreA[0]) - rot[i][1] * centreA[1]) - rot[i][2] * centreA[2];
        }
    } else {
        for (int i = 0; i < 3; i++) shift[i] = ((centreB[i] - rot[i][0] * centreA[0]) - rot[i][1] * centreA[1]) - rot[i][2] * centreA[2];
    }
    double sv[3];
    for (int i = 0; i < 3; i++) sv[i] = sqrt(lambda[i] < 0 ? 0.0 : lambda[i]);
    double trace = det < 0.0 ? -sv[2] : sv[2];
    trace = (trace + sv[1]) + sv[0];
    double residual = (spread - trace) - trace;
    if (residual < 0.0) residual = 0.0;
    rmsOut = (float) residual;
    for (int i = 0; i < 3; i++) {
        t[i] = (float) shift[i];
        for (int j = 0; j < 3; j++) u[i][j] = (float) rot[i][j];
    }
}

// KabschFast of TMalign.cpp
TM_HD void tmKabschFast(const TmView &v, const uint32_t *mask, uint32_t nSel, float &rms, float t[3], float u[3][3]) {
    if (nSel >= 1) {
        tmKabschAvx(v, mask, nSel, rms, t, u);
        bool bad = false;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) bad |= tmIsNan(u[i][j]);
        if (!bad) return;
    }
    // no pair at all: 1 / 0 = inf and 0 * inf = NaN in every centred sum, so the reference's rotation is NaN there as well
    tmKabschClassic(v, mask, nSel, rms, t, u);
}

// do_rotation + one pass of score_fun8's loops: the selection di < dTmp into `mout`, the number selected, with `sum` the left-to-right score sum, and
// the three smallest di (what the relief loop needs)
TM_HD uint32_t tmScorePass(const TmView &v, const float t[3], const float u[3][3], float dTmp, float cut, float d02, uint32_t *mout, float &sumOut, float low[3]) {
    const size_t n = v.n;
    float sum = 0.0f, l0 = __builtin_inff(), l1 = l0, l2 = l0;
    uint32_t nCut = 0;
    for (uint32_t w = 0; w < v.words; w++) {
        uint32_t bits = 0;
        const uint32_t i0 = w * 32, m = v.n - i0 < 32u ? v.n - i0 : 32u;
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = i0 + k;
            const float x = v.c[i], y = v.c[n + i], z = v.c[2 * n + i];
            const float xt = t[0] + ((u[0][0] * x + u[0][1] * y) + u[0][2] * z);
            const float yt = t[1] + ((u[1][0] * x + u[1][1] * y) + u[1][2] * z);
            const float zt = t[2] + ((u[2][0] * x + u[2][1] * y) + u[2][2] * z);
            const float dx = xt - v.c[3 * n + i], dy = yt - v.c[4 * n + i], dz = zt - v.c[5 * n + i];
            const float di = (dx * dx + dy * dy) + dz * dz;
            sum += (di < cut) ? 1.0f / (1.0f + di / d02) : 0.0f;
            const bool sel = di < dTmp;
            bits |= (sel ? 1u : 0u) << k;
            nCut += sel ? 1u : 0u;
            if (di < l2) {
                if (di < l1) {
                    l2 = l1;
                    if (di < l0) { l1 = l0; l0 = di; } else l1 = di;
                } else l2 = di;
            }
        }
        mout[(size_t) w * v.ms] = bits;
    }
    sumOut = sum;
    low[0] = l0; low[1] = l1; low[2] = l2;
    return nCut;
}

// score_fun8 after do_rotation; `div` is its Lnorm (n in the approximate searches, the normalisation length in the exact one).  The relief loop (`n_cut < 3 && n_ali > 3`: d_tmp = (float) ((d + inc * 0.5)^2), inc = 1, 2, ...) is solved
// for the first inc whose threshold exceeds the third smallest di instead of being walked; the selection of that inc is what the reference ends with.
// Returns false where the reference's loop would never end (fewer than three pairs with a finite distance): the caller leaves the start.
TM_HD bool tmScoreFun8(const TmView &v, const float t[3], const float u[3][3], float d, float scoreD8, float d0, float div, uint32_t *mout, uint32_t &nCut, float &score) {
    const float d02 = d0 * d0, cut = scoreD8 * scoreD8;
    float dTmp = d * d, sum, low[3];
    nCut = tmScorePass(v, t, u, dTmp, cut, d02, mout, sum, low);
    score = sum / div;
    if (nCut < 3 && v.n > 3) {
        if (!(low[2] < __builtin_inff())) return false;
        const double dd = (double) d, third = (double) low[2];
        double inc = floor((sqrt(third) - dd) * 2.0) - 2.0;
        if (!(inc >= 1.0)) inc = 1.0;
        // the threshold does not decrease with inc >= 1 (d >= -0.5 in both searches); the estimate is within a few steps of the answer, so both walks
        // are short, and they are bounded: past the bound (a NaN d, distances beyond 2^53 half-steps) the start is left like a loop that never ends
        int guard = 0;
        while (inc > 1.0 && guard++ < 64) { const double q = dd + (inc - 1.0) * 0.5; if (low[2] < (float) (q * q)) inc -= 1.0; else break; }
        bool found = false;
        for (guard = 0; guard < 64 && !found; guard++) {
            const double q = dd + inc * 0.5;
            dTmp = (float) (q * q);
            if (low[2] < dTmp) found = true; else inc += 1.0;
        }
        if (!found) return false;
        float sum2;
        nCut = tmScorePass(v, t, u, dTmp, cut, d02, mout, sum2, low);
    }
    return true;
}

// a lane's best score with the superposition that first reached it: the reference overwrites t0 / u0 at every STRICT improvement of score_max, so what
// is left is the rotation at the first occurrence of the maximum in its serial order (fragment length, start, refinement round).  ord: the ordinal of
// the fragment start in that order; kTmNoOrd while score_max still has its initial -1.
constexpr uint32_t kTmNoOrd = 0xffffffffu;
struct TmBest {
    float score;
    uint32_t ord;
    float t[3], u[3][3];
};

TM_HD void tmTake(TmBest &b, float score, uint32_t ord, const float t[3], const float u[3][3]) {
    b.score = score; b.ord = ord;
    for (int i = 0; i < 3; i++) {
        b.t[i] = t[i];
        for (int j = 0; j < 3; j++) b.u[i][j] = u[i][j];
    }
}

// one fragment start of TMscore8_search_standard (rounds = 20, div = n) or of TMscore8_search (rounds = 10, div = Lnorm): the body of its `while (1)`.
// Returns the largest score seen (at least `best`); with kTrack, *tb (whose score is `best`) follows every strict improvement.
template <bool kTrack>
TM_HD float tmStartT(const TmView &v, uint32_t start, uint32_t len, float d0Search, float scoreD8, float d0, float div, int rounds, float best, TmBest *tb, uint32_t ord) {
    uint32_t *cur = v.m[0], *nxt = v.m[1];
    for (uint32_t w = 0; w < v.words; w++) {
        const uint32_t lo = w * 32, hi = lo + 32;
        uint32_t bits = 0;
        if (start < hi && start + len > lo) {
            const uint32_t b0 = start > lo ? start - lo : 0u, b1 = (start + len < hi ? start + len : hi) - lo;          // bits [b0, b1)
            bits = (b1 - b0 == 32u ? 0xffffffffu : ((1u << (b1 - b0)) - 1u)) << b0;
        }
        cur[(size_t) w * v.ms] = bits;
    }
    float rms, t[3], u[3][3], score;
    uint32_t nCut;
    tmKabschFast(v, cur, len, rms, t, u);
    if (!tmScoreFun8(v, t, u, d0Search - 1.0f, scoreD8, d0, div, nxt, nCut, score)) return best;
    if (score > best) { best = score; if (kTrack) tmTake(*tb, score, ord, t, u); }
    const float d = d0Search + 1.0f;
    for (int it = 0; it < rounds; it++) {
        uint32_t *s = cur; cur = nxt; nxt = s;
        const uint32_t ka = nCut;
        tmKabschFast(v, cur, ka, rms, t, u);
        if (!tmScoreFun8(v, t, u, d, scoreD8, d0, div, nxt, nCut, score)) return best;
        if (score > best) { best = score; if (kTrack) tmTake(*tb, score, ord, t, u); }
        if (nCut == ka) {
            bool same = true;
            for (uint32_t w = 0; w < v.words; w++) same &= cur[(size_t) w * v.ms] == nxt[(size_t) w * v.ms];
            if (same) break;
        }
    }
    return best;
}

TM_HD float tmStart(const TmView &v, uint32_t start, uint32_t len, float d0Search, float scoreD8, float d0, float best) {
    return tmStartT<false>(v, start, len, d0Search, scoreD8, d0, (float) v.n, kTmRounds, best, nullptr, 0u);
}

// fragment lengths n, n/2, n/4 ... down to min(4, n), at most 6; returns their number.  starts[k]: fragment starts of length k (0, step, 2 step ...,
// last forced)
TM_HD int tmFragments(uint32_t n, uint32_t len[6], uint32_t starts[6], uint32_t step = kTmStep) {
    const uint32_t lmin = n < 4u ? n : 4u;
    int cnt = 0, i;
    for (i = 0; i < 5; i++) {
        cnt++;
        len[i] = n >> i;
        if (len[i] <= lmin) { len[i] = lmin; break; }
    }
    if (i == 5) { cnt++; len[5] = lmin; }
    for (int k = 0; k < cnt; k++) {
        const uint32_t imax = n - len[k];
        starts[k] = imax == 0 ? 1u : (imax + step - 1) / step + 1u;
    }
    return cnt;
}

// the s-th start over all fragment lengths -> (start, length)
TM_HD void tmNthStart(uint32_t n, int cnt, const uint32_t len[6], const uint32_t starts[6], uint32_t s, uint32_t &start, uint32_t &flen, uint32_t step = kTmStep) {
    int k = 0;
    while (k < cnt - 1 && s >= starts[k]) { s -= starts[k]; k++; }
    flen = len[k];
    const uint32_t imax = n - flen, pos = s * step;
    start = pos < imax ? pos : imax;
}

#if defined(__HIPCC__)
// grid (tasks); backtrace -> pairs[6][n] (the prefix-sum walk of k_lddt_pairs; here every character that is neither 'M' nor 'I' advances the target)
__global__ __launch_bounds__(kTmPairsBlock) void k_tm_pairs(TmArgs a) {
    __shared__ uint32_t sWave[kTmPairsBlock / 64];
    const TmTask t = a.tasks[blockIdx.x];
    const TmQuery q = a.queries[t.query];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = t.nPairs;
    float *pairs = a.pairs + t.pairOff;
    const float *qx = a.qc + q.cOff, *qy = qx + q.L, *qz = qy + q.L;
    const float *tx = a.tc + t.tOff, *ty = tx + t.tLen, *tz = ty + t.tLen;
    uint32_t baseM = 0, baseQ = (uint32_t) t.qStart, baseT = (uint32_t) t.dbStart;
    for (uint32_t c0 = 0; c0 < t.btLen; c0 += kTmPairsBlock) {
        const uint32_t i = c0 + tid;
        const bool live = i < t.btLen;
        const char ch = live ? a.bt[t.btOff + i] : '\0';
        const bool isM = live && ch == 'M', isI = live && ch == 'I', isT = live && !isM && !isI;
        const uint32_t v = (isM ? 1u : 0u) | ((isM || isI) ? 1u << 10 : 0u) | ((isM || isT) ? 1u << 20 : 0u);
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if ((int) lane >= d) incl += up; }
        __syncthreads();
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kTmPairsBlock / 64; w++) { const uint32_t s = sWave[w]; if (w < wave) before += s; total += s; }
        const uint32_t excl = before + incl - v;
        if (isM) {
            const uint32_t k = baseM + (excl & 1023u), qi = baseQ + ((excl >> 10) & 1023u), ti = baseT + (excl >> 20);
            if (k < n && qi < q.L && ti < t.tLen) {
                pairs[k] = tx[ti]; pairs[(size_t) n + k] = ty[ti]; pairs[2 * (size_t) n + k] = tz[ti];
                pairs[3 * (size_t) n + k] = qx[qi]; pairs[4 * (size_t) n + k] = qy[qi]; pairs[5 * (size_t) n + k] = qz[qi];
            }
        }
        baseM += total & 1023u; baseQ += (total >> 10) & 1023u; baseT += total >> 20;
    }
    if (tid == 0) a.nPairs[t.slot] = (int32_t) baseM;
}

// grid (tasks, 3), one wave each
__global__ __launch_bounds__(64) void k_tm_search(TmArgs a) {
    __shared__ float sC[6 * kTmLdsPairs];
    __shared__ uint32_t sM[2 * kTmLdsWords * 64];
    const TmTask t = a.tasks[blockIdx.x];
    const uint32_t lane = threadIdx.x, which = blockIdx.y, n = t.nPairs;
    float *out = a.out + (size_t) which * a.nt + t.slot;
    if (n == 0) {                          // score_max keeps its initial -1 (0 / 0 never exceeds it), the rmsd its initial 0; no memory is touched
        if (lane == 0) *out = which < 2 ? -1.0f : 0.0f;
        return;
    }
    const float *pairs = a.pairs + t.pairOff;
    TmView v;
    v.n = n; v.words = (n + 31) / 32; v.ms = 64;
    if (n <= (uint32_t) kTmLdsPairs) {
        for (uint32_t i = lane; i < 6 * n; i += 64) sC[i] = pairs[i];
        __syncthreads();
        v.c = sC;
        v.m[0] = sM + lane; v.m[1] = sM + (size_t) v.words * 64 + lane;
    } else {
        v.c = pairs;
        uint32_t *base = a.masks + t.maskOff + (size_t) which * 2 * v.words * 64;
        v.m[0] = base + lane; v.m[1] = base + (size_t) v.words * 64 + lane;
    }
    if (which == 2) {                      // standard_TMscore's KabschFast over all pairs: RMSD
        if (lane == 0) {
            for (uint32_t w = 0; w < v.words; w++) {
                const uint32_t left = n - w * 32;
                v.m[0][(size_t) w * 64] = left >= 32u ? 0xffffffffu : ((1u << left) - 1u);
            }
            float rms, tt[3], uu[3][3];
            tmKabschFast(v, v.m[0], n, rms, tt, uu);
            *out = rms;
        }
        return;
    }
    uint32_t len[6], starts[6];
    const int cnt = tmFragments(n, len, starts);
    uint32_t total = 0;
    for (int k = 0; k < cnt; k++) total += starts[k];
    float best = -1.0f;
    for (uint32_t s = lane; s < total; s += 64) {
        uint32_t start, flen;
        tmNthStart(n, cnt, len, starts, s, start, flen);
        best = tmStart(v, start, flen, t.d0Search[which], t.scoreD8, t.d0[which], best);
    }
    for (int d = 32; d >= 1; d >>= 1) { const float o = __shfl_xor(best, d, 64); best = o > best ? o : best; }
    if (lane == 0) *out = best;
}
#endif

} // namespace fs

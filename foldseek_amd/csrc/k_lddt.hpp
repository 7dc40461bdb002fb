// k_lddt.hpp -- LDDT of accepted hits on the device (reference: F/src/commons/LDDT.{h,cpp}; C ABI: fsgpu_lddt_batch in fsgpu_lddt.hip).
//
// The reference's grid only prunes: its box edge equals the 15 A cutoff, so it visits every pair of aligned columns whose QUERY distance is below the
// cutoff exactly once.  A pair adds 0.25 * ((d < 0.5) + (d < 1) + (d < 2) + (d < 4)), d = |dist_query - dist_target|, to both of its columns: sums of
// multiples of 0.25, exact in float in any order.  So a column's score is an integer count of quarters over ALL other aligned columns, and the float
// operations that have to be reproduced bit for bit are few: dist() (three subtractions, fma(d0, d0, 0), fma(d1, d1, .), fma(d2, d2, .) -- the reference
// binary is built with contraction on -- and a correctly rounded square root), |a - b|, the reciprocal of the neighbour count and one multiplication.
// This object is compiled without contraction and with correctly rounded division / square root (Makefile); the fmas below are explicit.
//
//   k_lddt_norm   norm[c] = 1 / #{r != c : dist(q_r, q_c) < 15}, +inf for a residue without neighbours (LDDTCalculator::initQuery), once per query
//   k_lddt_pairs  one workgroup per hit: backtrace -> aligned index lists (workgroup prefix sum over M / I / D), aligned coordinates gathered once into
//                 one array per axis, then every lane owns one aligned column and walks ALL columns, streamed through LDS in tiles (all lanes read the
//                 same LDS address: a broadcast, no bank conflict).  No atomics: a pair is computed by both of its columns.
//                 out[column] = quarters * 0.25f * norm[query residue]; 0 * inf = NaN marks a column the reference's average skips.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fs {

#pragma clang fp contract(off)

constexpr int kLddtBlock = 256;          // lanes of a workgroup (4 waves)
constexpr int kLddtTile = 1024;          // aligned columns per LDS tile: 6 axes x 4 KB = 24 KB
constexpr int kLddtAxes = 7;             // per-column workspace arrays: query x y z, target x y z, norm of the query residue

struct LddtQuery { uint32_t cOff, L, nOff, pad; };          // cOff: float offset of x[L] y[L] z[L] in the query blob; nOff: offset into norm[]
struct LddtTask {
    uint32_t query, tLen;
    uint64_t tOff;                       // float offset of x[tLen] y[tLen] z[tLen] in the target blob
    int32_t qStart, dbStart;
    uint64_t btOff;
    uint32_t btLen, nCols;               // nCols: 'M' characters of the backtrace (counted by the host: sizes the workspace slices)
    uint64_t colOff;                     // first column of this task in out[]; its workspace slice starts at colOff * kLddtAxes
    uint32_t slot, pad;                  // index of the task in the caller's order (alnLen[slot])
};
struct LddtArgs {
    const LddtQuery *queries;
    const LddtTask *tasks;
    const float *qc, *tc;
    const char *bt;
    float *norm, *cols, *out;
    int32_t *alnLen;
};

// dist() of LDDT.cpp as the reference binary computes it
__device__ __forceinline__ float lddtDist(float ax, float ay, float az, float bx, float by, float bz) {
    const float d0 = ax - bx, d1 = ay - by, d2 = az - bz;
    float s = __builtin_fmaf(d0, d0, 0.0f);
    s = __builtin_fmaf(d1, d1, s);
    s = __builtin_fmaf(d2, d2, s);
    return __builtin_sqrtf(s);
}

// grid (ceil(maxL / kLddtBlock), queries)
__global__ __launch_bounds__(kLddtBlock) void k_lddt_norm(LddtArgs a) {
    const LddtQuery q = a.queries[blockIdx.y];
    const uint32_t c0 = blockIdx.x * kLddtBlock;
    if (c0 >= q.L) return;
    __shared__ float sx[kLddtBlock], sy[kLddtBlock], sz[kLddtBlock];
    const float *x = a.qc + q.cOff, *y = x + q.L, *z = y + q.L;
    const uint32_t tid = threadIdx.x, c = c0 + tid;
    const bool live = c < q.L;
    const float cx = live ? x[c] : 0.0f, cy = live ? y[c] : 0.0f, cz = live ? z[c] : 0.0f;
    uint32_t count = 0;
    for (uint32_t r0 = 0; r0 < q.L; r0 += kLddtBlock) {
        __syncthreads();
        const uint32_t r = r0 + tid;
        if (r < q.L) { sx[tid] = x[r]; sy[tid] = y[r]; sz[tid] = z[r]; }
        __syncthreads();
        const uint32_t m = min((uint32_t) kLddtBlock, q.L - r0);
        if (live)
            for (uint32_t k = 0; k < m; k++)
                count += (r0 + k != c && lddtDist(sx[k], sy[k], sz[k], cx, cy, cz) < 15.0f) ? 1u : 0u;
    }
    if (live) a.norm[q.nOff + c] = count ? 1.0f / (float) count : __builtin_inff();
}

// quarters one other column adds to the lane's column
__device__ __forceinline__ uint32_t lddtPair(float qx, float qy, float qz, float tx, float ty, float tz, float oqx, float oqy, float oqz, float otx, float oty,
                                             float otz, bool other) {
    const float dq = lddtDist(oqx, oqy, oqz, qx, qy, qz);
    if (!(other && dq < 15.0f)) return 0;
    const float d = __builtin_fabsf(dq - lddtDist(otx, oty, otz, tx, ty, tz));
    return (uint32_t) (d < 0.5f) + (uint32_t) (d < 1.0f) + (uint32_t) (d < 2.0f) + (uint32_t) (d < 4.0f);
}

// grid (tasks), longest first
__global__ __launch_bounds__(kLddtBlock) void k_lddt_pairs(LddtArgs a) {
    __shared__ __attribute__((aligned(16))) float sc[6][kLddtTile];
    __shared__ uint32_t sWave[kLddtBlock / 64];
    const LddtTask t = a.tasks[blockIdx.x];
    const LddtQuery q = a.queries[t.query];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = t.nCols;
    float *cols = a.cols + t.colOff * kLddtAxes;          // [kLddtAxes][n]
    const float *qx = a.qc + q.cOff, *qy = qx + q.L, *qz = qy + q.L;
    const float *tx = a.tc + t.tOff, *ty = tx + t.tLen, *tz = ty + t.tLen;
    const float *norm = a.norm + q.nOff;

    // ---- backtrace -> aligned index lists (LDDTCalculator::constructAlignHashes): exclusive prefix sums of the M / query / target advances, the three
    // counts of a chunk of kLddtBlock characters packed into one word (10 bits each)
    uint32_t baseM = 0, baseQ = (uint32_t) t.qStart, baseT = (uint32_t) t.dbStart;
    for (uint32_t c0 = 0; c0 < t.btLen; c0 += kLddtBlock) {
        const uint32_t i = c0 + tid;
        const char ch = i < t.btLen ? a.bt[t.btOff + i] : '\0';
        const bool isM = ch == 'M';
        const uint32_t v = (isM ? 1u : 0u) | ((isM || ch == 'I') ? 1u << 10 : 0u) | ((isM || ch == 'D') ? 1u << 20 : 0u);
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if ((int) lane >= d) incl += up; }
        __syncthreads();                                  // the previous chunk's readers of sWave are done
        if (lane == 63) sWave[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kLddtBlock / 64; w++) { const uint32_t s = sWave[w]; if (w < wave) before += s; total += s; }
        const uint32_t excl = before + incl - v;
        if (isM) {
            const uint32_t k = baseM + (excl & 1023u), qi = baseQ + ((excl >> 10) & 1023u), ti = baseT + (excl >> 20);
            if (k < n && qi < q.L && ti < t.tLen) {
                cols[k] = qx[qi]; cols[(size_t) n + k] = qy[qi]; cols[2 * (size_t) n + k] = qz[qi];
                cols[3 * (size_t) n + k] = tx[ti]; cols[4 * (size_t) n + k] = ty[ti]; cols[5 * (size_t) n + k] = tz[ti];
                cols[6 * (size_t) n + k] = norm[qi];
            }
        }
        baseM += total & 1023u; baseQ += (total >> 10) & 1023u; baseT += total >> 20;
    }
    if (tid == 0) a.alnLen[t.slot] = (int32_t) baseM;
    __syncthreads();                                      // the gathered columns are visible to the whole workgroup

    // ---- every lane one column, all columns through LDS
    for (uint32_t i0 = 0; i0 < n; i0 += kLddtBlock) {
        const uint32_t i = i0 + tid;
        const bool live = i < n;
        float oq0 = 0, oq1 = 0, oq2 = 0, ot0 = 0, ot1 = 0, ot2 = 0;
        if (live) {
            oq0 = cols[i]; oq1 = cols[(size_t) n + i]; oq2 = cols[2 * (size_t) n + i];
            ot0 = cols[3 * (size_t) n + i]; ot1 = cols[4 * (size_t) n + i]; ot2 = cols[5 * (size_t) n + i];
        }
        uint32_t quarters = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += kLddtTile) {
            const uint32_t m = min((uint32_t) kLddtTile, n - j0);
            __syncthreads();
            for (uint32_t k = tid; k < m; k += kLddtBlock)
                for (int ax = 0; ax < 6; ax++) sc[ax][k] = cols[(size_t) ax * n + j0 + k];
            __syncthreads();
            if (!live) continue;
            uint32_t k = 0;
            for (; k + 4 <= m; k += 4) {
                const float4 x4 = *(const float4 *) &sc[0][k], y4 = *(const float4 *) &sc[1][k], z4 = *(const float4 *) &sc[2][k];
                const float4 u4 = *(const float4 *) &sc[3][k], v4 = *(const float4 *) &sc[4][k], w4 = *(const float4 *) &sc[5][k];
                const uint32_t j = j0 + k;
                quarters += lddtPair(x4.x, y4.x, z4.x, u4.x, v4.x, w4.x, oq0, oq1, oq2, ot0, ot1, ot2, j != i);
                quarters += lddtPair(x4.y, y4.y, z4.y, u4.y, v4.y, w4.y, oq0, oq1, oq2, ot0, ot1, ot2, j + 1 != i);
                quarters += lddtPair(x4.z, y4.z, z4.z, u4.z, v4.z, w4.z, oq0, oq1, oq2, ot0, ot1, ot2, j + 2 != i);
                quarters += lddtPair(x4.w, y4.w, z4.w, u4.w, v4.w, w4.w, oq0, oq1, oq2, ot0, ot1, ot2, j + 3 != i);
            }
            for (; k < m; k++) quarters += lddtPair(sc[0][k], sc[1][k], sc[2][k], sc[3][k], sc[4][k], sc[5][k], oq0, oq1, oq2, ot0, ot1, ot2, j0 + k != i);
        }
        if (live) a.out[t.colOff + i] = (float) quarters * 0.25f * cols[6 * (size_t) n + i];
    }
}

} // namespace fs

// k_kmer_profile.hpp -- gfx950 kernels of stage 1 of the k-mer prefilter for PROFILE queries: the similar k-mers of a query position from the
// six sorted score rows of its window (KmerGenerator::setDivideStrategy(ScoreMatrix **) + generateKmerList, KmerGenerator.cpp:31-40,108-217).
//
// The reference multiplies the list level by level: level i keeps, for every prefix (j0 .. j(i-1)) of row RANKS it has, the ranks ji with
//   row_i[ji] >= thr - (score of the prefix) - possibleRest_i,     possibleRest_i = sum of the maxima of the rows after i.
// A prefix that passes always has a completion (the top entry of every later row gives exactly score + possibleRest >= thr), so no level shrinks
// and the final list is { (j0 .. j5) : sum of row_i[ji] >= thr } in LEXICOGRAPHIC order of the ranks; the per-level cap of MAX_KMER_RESULT_SIZE - 1
// leaves the first 8 388 607 of them (the first N tuples have at most N distinct prefixes at every level).  tests/test_kmer_profile_model.py holds
// the literal product to this claim.  That makes the list a ranked set:
//   C_i[t] = number of (ji .. j5) with row_i[ji] + ... + row_5[j5] >= t           (C_5 from the last row, C_i[t] = sum over j of C_(i+1)[t - row_i[j]])
//   K_p    = min(C_0[thr], cap);   the r-th k-mer: at level i walk j = 0, 1, ... and subtract C_(i+1)[t - row_i[j]] from r until r falls inside.
// A workgroup builds C_1 .. C_5 of its position in LDS (15 KB) and every thread unranks its own k-mers: no order-dependent work, coalesced writes.
// All integer / LDS work; the index probes behind it (bitmap + offset table) are the HBM traffic, exactly as in k_kmer_lists.
#pragma once
#include "k_kmer.hpp"

namespace fs {

// A sum of n score bytes lies in [-128 n, 127 n].  Table of level i (n = 6 - i rows left) holds t in [-128 n, 127 n + 1] at index t + 128 n:
// below that range C is 20^n, the value AT -128 n; above it C is 0, the value AT 127 n + 1.  kpIdx clamps t into the range, so every table
// index is in [0, 255 n + 1] whatever thr is (thr is an int16 >= 0, t = thr - partial sum fits an int with room to spare).
__host__ __device__ constexpr int kpSize(int n) { return 255 * n + 2; }
constexpr int kpOff5 = 0, kpOff4 = kpOff5 + kpSize(1), kpOff3 = kpOff4 + kpSize(2), kpOff2 = kpOff3 + kpSize(3), kpOff1 = kpOff2 + kpSize(4),
              kpTableWords = kpOff1 + kpSize(5);          // 3835 words = 15 340 bytes
__device__ __forceinline__ int kpOff(int level) { return level == 5 ? kpOff5 : level == 4 ? kpOff4 : level == 3 ? kpOff3 : level == 2 ? kpOff2 : kpOff1; }
__device__ __forceinline__ int kpIdx(int t, int n) { return min(max(t, -128 * n), 127 * n + 1) + 128 * n; }

// One staged row entry: score << 8 | letter (score in [-128, 127], letter in [0, 19]); rows[(position) * 20 + rank], sorted by the host the way
// Util::rankedDescSort20 leaves them.
__device__ __forceinline__ int kpScore(int e) { return e >> 8; }
__device__ __forceinline__ uint32_t kpLetter(int e) { return (uint32_t) e & 0xffu; }

struct KmerProfLds {
    int row[6][20];                   // the six rows of the window in pattern order
    uint32_t C[kpTableWords];         // C_5 | C_4 | C_3 | C_2 | C_1
    int thr;
    uint32_t skip;
};

// rows + tables of position p; returns false (for the whole workgroup) when the window holds an X.  Ends with a barrier.
__device__ inline bool kmerProfTables(KmerProfLds &s, const KmerQ &q, const uint8_t *seqs, const int16_t *thrs, const uint16_t *rows /* [batch positions][20] */,
                                      uint64_t rowBase /* first row of the query */, uint32_t p, KmerPattern pat) {
    const uint32_t i = p - q.posBase;
    if (threadIdx.x < 120) {
        const int z = threadIdx.x / 20, j = threadIdx.x - z * 20;
        s.row[z][j] = (int) (int16_t) rows[(rowBase + i + (uint32_t) pat.pos[z]) * 20 + j];
    }
    if (threadIdx.x == 128) {
        const uint8_t *c = seqs + q.seqOff + i;
        bool x = false;
#pragma unroll
        for (int z = 0; z < 6; z++) x |= c[pat.pos[z]] >= 20;
        s.skip = x; s.thr = thrs[p];
    }
    __syncthreads();
    if (s.skip) return false;
    // C_5[t] = #{ j : row_5[j] >= t }
    for (int k = threadIdx.x; k < kpSize(1); k += blockDim.x) {
        const int t = k - 128;
        uint32_t c = 0;
#pragma unroll
        for (int j = 0; j < 20; j++) c += kpScore(s.row[5][j]) >= t;
        s.C[kpOff5 + k] = c;
    }
    __syncthreads();
#pragma unroll
    for (int level = 4; level >= 1; level--) {
        const int n = 6 - level, off = kpOff(level), below = kpOff(level + 1);
        for (int k = threadIdx.x; k < kpSize(n); k += blockDim.x) {
            const int t = k - 128 * n;
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < 20; j++) c += s.C[below + kpIdx(t - kpScore(s.row[level][j]), n - 1)];       // index clamped by kpIdx
            s.C[off + k] = c;                                                                                 // k < kpSize(n): inside the table of this level
        }
        __syncthreads();
    }
    return true;
}

// C_0[thr], capped like calculateArrayProduct (counter + 1 < MAX_KMER_RESULT_SIZE); at most 20^6 = 64e6: no overflow in 32 bits
__device__ inline uint32_t kmerProfCount(const KmerProfLds &s) {
    uint32_t c = 0;
    for (int j = 0; j < 20; j++) c += s.C[kpOff1 + kpIdx(s.thr - kpScore(s.row[0][j]), 5)];
    return min(c, kMaxKmerResult - 1);
}

// the r-th (r < C_0[thr]) rank tuple with sum >= thr in lexicographic order -> its letters as (first 3-mer, last 3-mer)
__device__ inline void kmerProfUnrank(const KmerProfLds &s, uint32_t r, uint32_t &first3, uint32_t &last3) {
    int t = s.thr;
    uint32_t l[6];
#pragma unroll
    for (int level = 0; level < 5; level++) {
        const int n = 5 - level, below = kpOff(level + 1);
        int j = 0, e = s.row[level][0];
        // r < (number of completions of the prefix) = sum over j of the terms below, so the walk ends at some j <= 19; the bound on j keeps the row read
        // inside the row even if that ever failed
        for (;;) {
            const uint32_t c = s.C[below + kpIdx(t - kpScore(e), n)];
            if (r < c || j == 19) break;
            r -= c; j++; e = s.row[level][j];
        }
        t -= kpScore(e); l[level] = kpLetter(e);
    }
    l[5] = kpLetter(s.row[5][min(r, 19u)]);          // the last row is taken from its top: rank = what is left of r (< C_5[t] <= 20)
    first3 = l[0] + 20 * l[1] + 400 * l[2];
    last3 = l[3] + 20 * l[4] + 400 * l[5];
}

// pass 1: K_p per query position
__global__ __launch_bounds__(kKmerBlock) void k_kmer_count_p(const KmerQ *qs, const uint16_t *posQuery, const uint8_t *seqs, const int16_t *thrs, const uint16_t *rows,
                                                             const uint64_t *rowBase, uint32_t nPos, KmerPattern pat, uint32_t *K) {
    const uint32_t p = blockIdx.x;
    if (p >= nPos) return;
    __shared__ KmerProfLds s;
    const uint32_t qi = posQuery[p];
    const bool ok = kmerProfTables(s, qs[qi], seqs, thrs, rows, rowBase[qi], p, pat);
    if (threadIdx.x == 0) K[p] = ok ? kmerProfCount(s) : 0;
}

// pass 2: the lists at Kbase[p] in the reference's order; work items are the slices of k_kmer_lists (same grid slots, same kListSlice).
// INSPECT: instead of probing the index, the slices of position `only` write their k-mers (reference numbering first3 + 8000 * last3) to kmerOut[r].
template <bool INSPECT>
__global__ __launch_bounds__(kKmerBlock) void k_kmer_lists_p(const KmerQ *qs, const uint16_t *posQuery, const uint8_t *seqs, const int16_t *thrs, const uint16_t *rows,
                                                             const uint64_t *rowBase, uint32_t nPos, KmerPattern pat, const uint32_t *Kcount, const uint64_t *Kbase,
                                                             const uint32_t *offsets, const uint32_t *bitmap, uint32_t *listStart, uint32_t *listSize, uint32_t *listPos,
                                                             uint32_t only, uint32_t *kmerOut) {
    __shared__ uint32_t pSh;
    if (threadIdx.x == 0) {
        const uint64_t slot = blockIdx.x;
        uint32_t lo = 0, hi = nPos;                // last position whose first slot is <= this slot
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t) mid + Kbase[mid] / kListSlice <= slot) lo = mid; else hi = mid; }
        pSh = lo;
    }
    __syncthreads();
    const uint32_t p = pSh;
    if (INSPECT && p != only) return;
    const uint32_t Kp = Kcount[p];
    const uint32_t slice = (uint32_t) ((uint64_t) blockIdx.x - ((uint64_t) p + Kbase[p] / kListSlice));
    if ((uint64_t) slice * kListSlice >= Kp) return;            // (covers Kp == 0, and with it every window that holds an X)
    const uint32_t rBeg = slice * kListSlice, rEnd = min(Kp, rBeg + kListSlice);
    __shared__ KmerProfLds s;
    const uint32_t qi = posQuery[p];
    const KmerQ q = qs[qi];
    if (!kmerProfTables(s, q, seqs, thrs, rows, rowBase[qi], p, pat)) return;
    const uint64_t base = Kbase[p];
    const uint32_t qpos = (qi << 16) | (p - q.posBase);
    for (uint32_t r = rBeg + threadIdx.x; r < rEnd; r += kKmerBlock) {
        uint32_t a, b;
        kmerProfUnrank(s, r, a, b);
        if (INSPECT) { kmerOut[r] = a + 8000u * b; continue; }
        const uint32_t kmer = kmerDeviceIndex(a, b);              // a, b < 8000: letters come from the staged rows, which the entry checked to be < 20
        uint32_t st = 0, en = 0;
        if ((bitmap[kmer >> 5] >> (kmer & 31)) & 1u) { st = offsets[kmer]; en = offsets[kmer + 1]; }
        listStart[base + r] = st; listSize[base + r] = en - st; listPos[base + r] = qpos;
    }
}

} // namespace fs

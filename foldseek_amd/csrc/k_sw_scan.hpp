// k_sw_scan.hpp -- device-side selection of a whole-database Smith-Waterman pass (fsgpu_sw_scan_c): of the n records k_sw3 left per query, the ones
// whose score reaches the query's cutoff -- or is the int16 ceiling, which the int32 re-run decides -- are compacted, with their target ids, in slot
// order.  Modelled on k_sel_hist / k_sel_emit (k_select.hpp): a workgroup per chunk of 4096 slots, 16 consecutive slots per thread, blockIdx.y = query;
// count per chunk, an exclusive scan over the chunks of a query, ordered emission.  No atomics: a position is a prefix sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fs {

constexpr int kScanChunk = 4096;     // slots per workgroup
constexpr int kScanThreads = 256;    // 16 consecutive slots per thread -> slot order is preserved
constexpr int kScanPerThread = kScanChunk / kScanThreads;

__device__ __forceinline__ bool scanPasses(int score, int cutoff) { return score >= cutoff || score == 32767; }

// the pass's target ids: the database's order, once per query (tids[y * n + k] = order[k])
__global__ __launch_bounds__(kScanThreads) void k_sw_scan_ids(const uint32_t *order, uint32_t n, uint32_t *tids) {
    uint32_t *dst = tids + (size_t) blockIdx.y * n;
    for (uint32_t k = blockIdx.x * kScanThreads + threadIdx.x; k < n; k += gridDim.x * kScanThreads) dst[k] = order[k];
}

// inclusive scan of one value per thread over the workgroup (Hillis-Steele in LDS); returns this thread's inclusive sum
__device__ __forceinline__ uint32_t scanBlockInclusive(uint32_t *s, uint32_t v) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        uint32_t o = 0;
        if ((int) threadIdx.x >= d) o = s[threadIdx.x - d];
        __syncthreads();
        s[threadIdx.x] += o;
        __syncthreads();
    }
    return s[threadIdx.x];
}

// pass A: survivors per chunk.  rec: n records (score, qEnd, dbEnd, word) per query; chunkCount[y * gridDim.x + x]
__global__ __launch_bounds__(kScanThreads) void k_sw_scan_count(const int4 *rec, uint32_t n, const int32_t *cutoff, uint32_t *chunkCount) {
    __shared__ uint32_t s[kScanThreads];
    rec += (size_t) blockIdx.y * n;
    const int cut = cutoff[blockIdx.y];
    const uint32_t base = blockIdx.x * kScanChunk + threadIdx.x * kScanPerThread;
    uint32_t cnt = 0, c = 0;
    if (base < n) cnt = n - base < (uint32_t) kScanPerThread ? n - base : (uint32_t) kScanPerThread;
    for (uint32_t k = 0; k < cnt; k++) c += scanPasses(rec[base + k].x, cut);
    const uint32_t incl = scanBlockInclusive(s, c);
    if (threadIdx.x == kScanThreads - 1) chunkCount[(size_t) blockIdx.y * gridDim.x + blockIdx.x] = incl;
}

// pass B (one workgroup per query): chunk counts -> exclusive offsets in place, the query's total
__global__ __launch_bounds__(kScanThreads) void k_sw_scan_offsets(uint32_t *chunkCount, uint32_t nChunks, uint32_t *totals) {
    __shared__ uint32_t s[kScanThreads];
    uint32_t *cc = chunkCount + (size_t) blockIdx.x * nChunks;
    const uint32_t per = (nChunks + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = threadIdx.x * per < nChunks ? threadIdx.x * per : nChunks, hi = lo + per < nChunks ? lo + per : nChunks;
    uint32_t sum = 0;
    for (uint32_t c = lo; c < hi; c++) sum += cc[c];
    const uint32_t incl = scanBlockInclusive(s, sum);
    uint32_t at = incl - sum;
    for (uint32_t c = lo; c < hi; c++) { const uint32_t v = cc[c]; cc[c] = at; at += v; }
    if (threadIdx.x == kScanThreads - 1) totals[blockIdx.x] = incl;
}

// pass C: ordered emission.  qBase[y]: first output slot of query y; nothing is written at or beyond outCap
__global__ __launch_bounds__(kScanThreads) void k_sw_scan_emit(const int4 *rec, const uint32_t *tids, uint32_t n, const int32_t *cutoff, const uint32_t *chunkBase,
                                                               const uint64_t *qBase, uint32_t *outIds, int4 *outRec, uint64_t outCap) {
    __shared__ uint32_t s[kScanThreads];
    rec += (size_t) blockIdx.y * n; tids += (size_t) blockIdx.y * n;
    const int cut = cutoff[blockIdx.y];
    const uint32_t base = blockIdx.x * kScanChunk + threadIdx.x * kScanPerThread;
    uint32_t cnt = 0, c = 0;
    if (base < n) cnt = n - base < (uint32_t) kScanPerThread ? n - base : (uint32_t) kScanPerThread;
    for (uint32_t k = 0; k < cnt; k++) c += scanPasses(rec[base + k].x, cut);
    const uint32_t incl = scanBlockInclusive(s, c);
    uint64_t pos = qBase[blockIdx.y] + chunkBase[(size_t) blockIdx.y * gridDim.x + blockIdx.x] + (incl - c);
    for (uint32_t k = 0; k < cnt; k++) {
        const int4 r = rec[base + k];
        if (!scanPasses(r.x, cut)) continue;
        if (pos < outCap) { outIds[pos] = tids[base + k]; outRec[pos] = r; }
        pos++;
    }
}

} // namespace fs

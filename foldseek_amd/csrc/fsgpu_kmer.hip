// fsgpu_kmer.hip -- C ABI of the k-mer prefilter (include/fsgpu.h: fsgpu_kmer_index_build / fsgpu_kmer_search).
// Host side: HIP runtime + rocPRIM's device radix sort / scan (AMD's native primitives; the order-defining work is in
// k_kmer.hpp).  No CPU fallback: everything below fails with FSGPU_E_* when there is no device.
#include <cstring>
#include <hip/hip_runtime.h>
#include <cstddef>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <unistd.h>

#include "fsgpu_ctx.h"
#include "k_kmer.hpp"
#include "k_kmer_profile.hpp"

#include <functional>
void fshostParallelFor(int n, const std::function<void(int)> &fn);      // host/search.cpp: the library's host worker pool

struct KmerIndex {
    fsgpu_kmer_index_params p{};
    KmerPattern pat{};
    std::shared_ptr<DbStore> db;          // keeps offsets / lengths alive
    uint64_t n = 0;
    int tbits = 1;
    uint8_t *masked = nullptr;            // SequenceLookup: masked codes in the padded layout of the DB
    uint32_t *offsets = nullptr;          // 20^6 + 1, in device k-mer order (kmerDeviceIndex)
    uint32_t *bitmap = nullptr;           // 20^6 bits: list non-empty
    uint64_t *entries = nullptr;          // seqId << 16 | first position (posBits == 0) ...
    uint32_t *entries32 = nullptr;        // ... or seqId << posBits | first position when id bits + position bits <= 32 (round 5: the gather of a list moves half the bytes)
    int posBits = 0;
    uint64_t nEntries = 0;
    int16_t *s3 = nullptr;                // extended 3-mer matrix, rows sorted descending
    uint16_t *i3 = nullptr;
    // coarse keys of the hit-stream partition (k_kmer.hpp, stage 2): runs of blocks of 1024 target ids.  levels[0] balances the residues over about
    // 128 keys (what a batch of the metric's size uses); the others hold a fixed number of blocks per key (1, 2, 4 ... 64) for batches with few
    // hits per query and for tests that force a granularity
    struct CoarseLevel { uint32_t nKeys = 0, nBlk = 0, maxIds = 0, blocksPerKey = 0; uint16_t *blkKey = nullptr; uint32_t *keyFirst = nullptr; };   // k_kmer.hpp KmerCoarse
    std::vector<CoarseLevel> levels;
    uint64_t residues = 0;
    ~KmerIndex() {
        (void) hipFree(masked); (void) hipFree(offsets); (void) hipFree(bitmap); (void) hipFree(entries); (void) hipFree(entries32); (void) hipFree(s3); (void) hipFree(i3);
        for (CoarseLevel &l : levels) { (void) hipFree(l.blkKey); (void) hipFree(l.keyFirst); }
    }
};

// Coarse keys of one level (KmerCoarse): consecutive blocks of 1024 target ids are joined into keys.  blocksPerKey > 0: that many blocks per key.
// blocksPerKey == 0: about 128 keys of equal residue count (index hits are proportional to residues; a length-sorted database would otherwise
// give the keys of its long end several times the hits of the others), no key longer than twice the average number of blocks (the duplicate
// stage keeps 16 bits of LDS per target id of a key) nor than kCoarseBlocks (the low 16 bits of an id must be unique inside a key).
// Host-only, tested without a GPU through fsgpu_kmer_plan_coarse.
static void planCoarse(const int32_t *lengths, uint64_t n, uint32_t blocksPerKey, std::vector<uint16_t> &blkKey, std::vector<uint32_t> &keyFirst) {
    const uint64_t nBlk = std::max<uint64_t>(1, (n + 1023) / 1024);
    blkKey.assign(nBlk, 0); keyFirst.clear();
    if (blocksPerKey == 0) {
        std::vector<uint64_t> res(nBlk, 0);
        uint64_t R = 0;
        for (uint64_t i = 0; i < n; i++) { res[i >> 10] += (uint64_t) std::max(lengths[i], 0); R += (uint64_t) std::max(lengths[i], 0); }
        const uint64_t target = std::max<uint64_t>(1, (R + 127) / 128);
        const uint64_t cap = std::min<uint64_t>(kCoarseBlocks, std::max<uint64_t>(1, 2 * ((nBlk + 127) / 128)));
        uint64_t acc = 0, cnt = 0;
        for (uint64_t k = 0; k < nBlk; k++) {
            if (cnt > 0 && (cnt >= cap || acc + res[k] > target)) { acc = 0; cnt = 0; }
            if (cnt == 0) keyFirst.push_back((uint32_t) (k * 1024));
            blkKey[k] = (uint16_t) (keyFirst.size() - 1);
            acc += res[k]; cnt++;
        }
        if (keyFirst.size() <= (size_t) kMaxCoarse) { keyFirst.push_back((uint32_t) n); return; }
        blocksPerKey = (uint32_t) ((nBlk + kMaxCoarse - 1) / kMaxCoarse);        // too many keys (cannot happen below 33.5 M targets): equal id ranges instead
        keyFirst.clear();
    }
    for (uint64_t k = 0; k < nBlk; k++) {
        if (k % blocksPerKey == 0) keyFirst.push_back((uint32_t) (k * 1024));
        blkKey[k] = (uint16_t) (k / blocksPerKey);
    }
    keyFirst.push_back((uint32_t) n);
}

extern "C" int fsgpu_kmer_plan_coarse(const int32_t *lengths, uint64_t n, uint32_t blocksPerKey, uint16_t *blkKey /*[max(1, ceil(n / 1024))]*/, uint32_t *keyFirst /*[cap]*/, uint32_t cap) {
    if ((!lengths && n) || blocksPerKey > (uint32_t) kCoarseBlocks) return FSGPU_E_ARG;
    std::vector<uint16_t> bk; std::vector<uint32_t> kf;
    planCoarse(lengths, n, blocksPerKey, bk, kf);
    if (kf.size() > cap) return FSGPU_E_ARG;
    if (blkKey) std::copy(bk.begin(), bk.end(), blkKey);
    if (keyFirst) std::copy(kf.begin(), kf.end(), keyFirst);
    return (int) kf.size() - 1;
}

// Arrays of this file: a device (KDev) or pinned host (KPin) array that knows its element type and frees itself.  Sizes are element counts
// everywhere (ensureK, kNew, kZero, kCopy); cap stays in bytes.
template <class T, hipError_t (*Free)(void *)> struct KArray {
    T *p = nullptr;
    size_t cap = 0;
    KArray() = default;
    KArray(const KArray &) = delete; KArray &operator=(const KArray &) = delete;          // an owner
    ~KArray() { (void) Free(p); }
};
template <class T> using KDev = KArray<T, hipFree>;
template <class T> using KPin = KArray<T, hipHostFree>;
using KBytes = KDev<unsigned char>;       // several arrays in one allocation, or rocPRIM's temporary storage

// per-context scratch of the search batches (kmerBatch)
struct KmerScratch {
    KDev<KmerQ> qs; KDev<KmerChunks> chunks; KDev<KmerBest> best; KDev<KmerOut> out;
    KDev<uint8_t> seqs, kept, kept0; KDev<int8_t> profiles; KDev<uint16_t> posQuery, recKey, ordA; KDev<int16_t> thrs; KDev<int32_t> score, qSlot;
    KDev<uint32_t> K, listStart, listSize, listPos, rec /* the duplicate stage's notes later */, recA, tileL, cntA, colA, grpSum, segCnt, segStart,
                   candKey, ckeys, ec, rounds, hist, thr, outCount, truncHist, trunc;
    KDev<uint32_t> candCount, nCand;      // [runCand nRuns + 1 | runBase nRuns + 1] (kmerCandidates); 16 words: [0] candidates of the batch, [1] elements handed to the host
    KDev<uint64_t> Kbase, listP, candVal, cvals, scrA, scrB; KDev<unsigned long long> resSize;
    KBytes tiles, tmp;                    // the tile table (carveTiles), rocPRIM's temporary storage
    KPin<KmerQ> hQs; KPin<KmerChunks> hChunks; KPin<KmerOut> hOut; KPin<uint8_t> hSeqs, hTiles; KPin<int8_t> hProfiles; KPin<uint16_t> hPosQuery; KPin<int16_t> hThrs;
    KPin<uint32_t> hEc, hRounds, hThr, hOutCount; KPin<unsigned long long> hResSize;
    KPin<uint64_t> hMisc;                 // 32 words: [0] lists, [1] hits, [2] candidates of the batch
    // profile queries (fsgpu_kmer_search_profile): the sorted score rows of every query position, score << 8 | letter, and where a query's rows start
    KDev<uint16_t> rows; KDev<uint64_t> rowBase; KPin<uint16_t> hRows; KPin<uint64_t> hRowBase;
    int profNq = 0; uint64_t profNPos = 0, profNLists = 0;          // the last device batch when it was a profile batch (fsgpu_kmer_profile_list_copy), else 0
    hipEvent_t ev[14] = {};
    bool evInit = false;
    const uint32_t *candTotal() const { return nCand.p; }
    uint32_t *outTotal() const { return nCand.p + 1; }
};

void fsgpu_kmer_free_scratch(KmerScratch *s) {
    if (s && s->evInit) for (hipEvent_t e : s->ev) (void) hipEventDestroy(e);
    delete s;
}

static inline unsigned gridFor(uint64_t n, unsigned block) { return (unsigned) std::max<uint64_t>(1, (n + block - 1) / block); }

// scratch grows geometrically: batch sizes differ from call to call and a hipFree/hipMalloc pair costs milliseconds
// scratch of a k-mer batch.  Out of device memory is reported as FSGPU_E_NOMEM (with the over-allocation dropped first): the caller of
// kmerBatch halves the batch instead of failing the search
template <class T>
static int ensureK(fsgpu_ctx *ctx, KDev<T> &b, size_t n) {
    const size_t bytes = n * sizeof(T);
    if (b.cap >= bytes && b.p) return FSGPU_OK;
    if (b.p) { HIPCHK(hipStreamSynchronize(ctx->stream)); (void) hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t wants[2] = {bytes + bytes / 2 + (1u << 20), bytes};
    for (size_t want : wants) {
        const hipError_t e = hipMalloc((void **) &b.p, want);
        if (e == hipSuccess) { b.cap = want; return FSGPU_OK; }
        b.p = nullptr;
        (void) hipGetLastError();
        if (e != hipErrorOutOfMemory) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return FSGPU_E_HIP; }
    }
    ctx->err = "k-mer search: out of device memory for the scratch of one batch (" + std::to_string(bytes >> 20) + " MiB requested)";
    return FSGPU_E_NOMEM;
}
template <class T>
static int ensureK(fsgpu_ctx *ctx, KPin<T> &h, size_t n) {            // ensurePinned (fsgpu_ctx.h) by element count
    PinBuf b{h.p, h.cap};
    const int rc = ensurePinned(ctx, b, n * sizeof(T));
    h.p = (T *) b.p; h.cap = b.cap;
    return rc;
}
// several arrays at once: (array, elements) pairs, grown in the order given
static int ensureAllK(fsgpu_ctx *) { return FSGPU_OK; }
template <class A, class... Rest>
static int ensureAllK(fsgpu_ctx *ctx, A &a, size_t n, Rest &&...rest) {
    const int rc = ensureK(ctx, a, n);
    return rc != FSGPU_OK ? rc : ensureAllK(ctx, rest...);
}
// an array of exactly n elements that lives as long as its owner: the temporaries of the index build
template <class T> static hipError_t kNew(KDev<T> &b, size_t n) { b.cap = n * sizeof(T); return hipMalloc((void **) &b.p, b.cap); }
template <class T> static hipError_t kZero(T *p, size_t n, hipStream_t st) { return hipMemsetAsync(p, 0, n * sizeof(T), st); }
template <class T> static hipError_t kCopy(T *dst, const T *src, size_t n, hipMemcpyKind kind, hipStream_t st) { return hipMemcpyAsync(dst, src, n * sizeof(T), kind, st); }

// rocPRIM's pair of calls: the first asks for the size of the temporary storage, the second runs
template <class F>
static int withTemp(fsgpu_ctx *ctx, KBytes &tmp, F call) {
    size_t bytes = 0;
    HIPCHK(call(nullptr, bytes));
    if (int rc = ensureK(ctx, tmp, bytes)) return rc;
    HIPCHK(call(tmp.p, bytes));
    return FSGPU_OK;
}
template <class T>
static int scanExclusive(fsgpu_ctx *ctx, KBytes &tmp, const T *in, T *out, size_t n) {
    return withTemp(ctx, tmp, [&](void *t, size_t &bytes) { return rocprim::exclusive_scan(t, bytes, in, out, (T) 0, n, rocprim::plus<T>(), ctx->stream); });
}
// u32 sizes -> u64 exclusive prefix
struct U32to64 { __host__ __device__ uint64_t operator()(uint32_t v) const { return v; } };
static int scanExclusive32to64(fsgpu_ctx *ctx, KBytes &tmp, const uint32_t *in, uint64_t *out, size_t n) {
    auto it = rocprim::make_transform_iterator(in, U32to64());
    return withTemp(ctx, tmp, [&](void *t, size_t &bytes) { return rocprim::exclusive_scan(t, bytes, it, out, (uint64_t) 0, n, rocprim::plus<uint64_t>(), ctx->stream); });
}
template <class K, class V>
static int sortPairs(fsgpu_ctx *ctx, KBytes &tmp, const K *kin, K *kout, const V *vin, V *vout, size_t n, int bits) {
    return withTemp(ctx, tmp, [&](void *t, size_t &bytes) { return rocprim::radix_sort_pairs(t, bytes, kin, kout, vin, vout, n, 0, bits, ctx->stream); });
}

static int bitsFor(uint64_t n) { int b = 1; while (b < 32 && (1ull << b) < n) b++; return b; }

constexpr double kKmerHitBudget = 2.4e8;          // index hits of one device batch (24 B of scratch each)
// queries of one device batch at most: the candidate keys are (query << tbits | target) in 32 bits
static int kmerMaxBatch(int tbits) { return std::max(1, std::min(1 << std::min(12, 32 - tbits), 1024)); }

// coarse-key levels of the hit-stream partition (index build)
static int buildCoarseLevels(fsgpu_ctx *ctx, KmerIndex &ix, const std::vector<int32_t> &lengths) {
    if ((ix.n + 1023) / 1024 > (uint64_t) kMaxCoarse * kCoarseBlocks) {
        ctx->err = "k-mer prefilter: more than " + std::to_string((uint64_t) kMaxCoarse * kCoarseBlocks * 1024) + " targets are not supported by the device hit-stream partition";
        return FSGPU_E_UNSUPPORTED;
    }
    std::vector<uint16_t> bk; std::vector<uint32_t> kf;
    uint32_t prevKeys = 0;
    for (uint32_t bpk : {0u, 1u, 2u, 4u, 8u, 16u, 32u, 64u}) {
        planCoarse(lengths.data(), ix.n, bpk, bk, kf);
        const uint32_t nk = (uint32_t) kf.size() - 1;
        if (nk > (uint32_t) kMaxCoarse || (bpk > 1 && nk == prevKeys)) continue;           // (a coarser level with the same keys is the same level)
        prevKeys = bpk ? nk : 0;
        ix.levels.emplace_back();                          // owned by the index from here on (freed by its destructor)
        KmerIndex::CoarseLevel &lv = ix.levels.back();
        lv.nKeys = nk; lv.nBlk = (uint32_t) bk.size(); lv.blocksPerKey = bpk;
        for (uint32_t k = 0; k < nk; k++) lv.maxIds = std::max(lv.maxIds, kf[k + 1] - kf[k]);
        HIPCHK(hipMalloc((void **) &lv.blkKey, bk.size() * sizeof(uint16_t)));
        HIPCHK(hipMalloc((void **) &lv.keyFirst, kf.size() * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(lv.blkKey, bk.data(), bk.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(lv.keyFirst, kf.data(), kf.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (ix.levels.empty()) { ctx->err = "k-mer prefilter: no coarse-key level fits the device partition"; return FSGPU_E_UNSUPPORTED; }
    return FSGPU_OK;
}

extern "C" {

uint64_t fsgpu_kmer_index_entries(const fsgpu_ctx *ctx) { return ctx && ctx->kidx ? ctx->kidx->nEntries : 0; }
int fsgpu_kmer_index_entry_bytes(const fsgpu_ctx *ctx) { return ctx && ctx->kidx ? (ctx->kidx->posBits ? 4 : 8) : 0; }
int fsgpu_kmer_index_get_params(const fsgpu_ctx *ctx, fsgpu_kmer_index_params *out) {
    if (!ctx || !out) return FSGPU_E_ARG;
    if (!ctx->kidx) return FSGPU_E_NODB;          // (ctx is const: the text of this refusal is the caller's to write)
    *out = ctx->kidx->p;
    return FSGPU_OK;
}

int fsgpu_kmer_index_build(fsgpu_ctx *ctx, const fsgpu_kmer_index_params *p, const int16_t *kmerSub) {
    if (!ctx || !p || !kmerSub) return FSGPU_E_ARG;
    if (!ctx->db || !ctx->db->raw3di) { ctx->err = "no database loaded"; return FSGPU_E_NODB; }
    if (p->kmerSize != 6) { ctx->err = "k-mer prefilter: only k = 6 is implemented on the device"; return FSGPU_E_UNSUPPORTED; }
    // UngappedAlignment switches to computeLongScore (wrapped 16-bit diagonals) from 32768 residues on (UngappedAlignment.cpp:198,295-312)
    if (ctx->db->maxLen >= 32768) { ctx->err = "k-mer prefilter: targets of 32768 residues or more are not supported on the device"; return FSGPU_E_UNSUPPORTED; }
    if (ctx->db->residues == 0) { ctx->err = "k-mer prefilter: the database holds no residues, there is nothing to index"; return FSGPU_E_UNSUPPORTED; }
    HIPCHK(hipSetDevice(ctx->device));
    std::shared_ptr<KmerIndex> ix = std::make_shared<KmerIndex>();
    ix->p = *p; ix->db = ctx->db; ix->n = ctx->db->n;
    ix->tbits = bitsFor(std::max<uint64_t>(ix->n, 2));
    static const int s6[10] = {1, 1, 0, 1, 0, 1, 0, 0, 1, 1};
    ix->pat.size = p->spaced ? 10 : 6;
    for (int i = 0, k = 0; i < ix->pat.size; i++) if (!p->spaced || s6[i]) ix->pat.pos[k++] = i;
    const DbStore &db = *ctx->db;
    const uint64_t n = db.n, bytes = std::max<uint64_t>(db.bytes, 1);
    const uint64_t tableSize = 64000000ull;
    // the temporaries of the build free themselves on every return
    KDev<int16_t> dSub; KDev<int8_t> dSelf; KDev<uint64_t> dResOff, v0, v1; KDev<uint32_t> k0, k1, flags, scan; KBytes tmp;
    // extended 3-mer matrix
    HIPCHK(kNew(dSub, 441));
    HIPCHK(hipMemcpy(dSub.p, kmerSub, 441 * sizeof(int16_t), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **) &ix->s3, (size_t) kRow3 * kRow3 * sizeof(int16_t)));
    HIPCHK(hipMalloc((void **) &ix->i3, (size_t) kRow3 * kRow3 * sizeof(uint16_t)));
    hipLaunchKernelGGL(k_kmer_rows3, dim3(kRow3), dim3(1024), 0, ctx->stream, dSub.p, ix->s3, ix->i3);
    HIPCHK(hipGetLastError());

    // masked lookup
    HIPCHK(hipMalloc((void **) &ix->masked, bytes + 16));          // + 16: k_kmer_score8 reads whole 8-byte words around a diagonal
    HIPCHK(hipMemsetAsync(ix->masked, 20, bytes, ctx->stream));
    if (n) {
        hipLaunchKernelGGL(k_kmer_mask, dim3(gridFor(n, 128)), dim3(128), 0, ctx->stream, db.raw3di, db.dOffsets, db.dLengths, n,
                           p->maskLowerCase, p->maskNrepeats, ix->masked);
        HIPCHK(hipGetLastError());
    }
    // k-mer extraction in (seqId, pos) order
    std::vector<uint64_t> resOff(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) resOff[i + 1] = resOff[i] + (uint64_t) db.hLengths[i];
    const uint64_t R = resOff[n];
    if (R >= 0xFFFFFFF0ull) { ctx->err = "k-mer index: more than 2^32 residues"; return FSGPU_E_UNSUPPORTED; }
    HIPCHK(hipMalloc((void **) &ix->offsets, (tableSize + 1) * sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(ix->offsets, 0, (tableSize + 1) * sizeof(uint32_t), ctx->stream));
    int rc = FSGPU_OK;
    if (R > 0) {
        int8_t self[21];
        for (int a = 0; a < 21; a++) self[a] = (int8_t) kmerSub[a * 21 + a];
        HIPCHK(kNew(dSelf, 32));
        HIPCHK(hipMemcpy(dSelf.p, self, 21, hipMemcpyHostToDevice));
        HIPCHK(kNew(dResOff, n + 1));
        HIPCHK(hipMemcpy(dResOff.p, resOff.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCHK(kNew(k0, R));
        HIPCHK(kNew(k1, R));
        HIPCHK(kNew(v0, R));
        HIPCHK(kNew(v1, R));
        HIPCHK(kNew(flags, R + 1));
        HIPCHK(kNew(scan, R + 1));
        hipLaunchKernelGGL(k_kmer_extract, dim3((unsigned) std::min<uint64_t>(n, 65535 * 16)), dim3(256), 0, ctx->stream, ix->masked, db.dOffsets, db.dLengths,
                           dResOff.p, n, ix->pat, p->kmerThr, dSelf.p, k0.p, v0.p);
        HIPCHK(hipGetLastError());
        // stable sort by k-mer keeps the (seqId, pos) order inside every k-mer: IndexEntryLocalTmp::comapreByIdAndPos
        if ((rc = sortPairs<uint32_t, uint64_t>(ctx, tmp, k0.p, k1.p, v0.p, v1.p, R, 26)) != FSGPU_OK) return rc;
        HIPCHK(kZero(flags.p + R, 1, ctx->stream));
        hipLaunchKernelGGL(k_kmer_unique_flags, dim3(gridFor(R, 256)), dim3(256), 0, ctx->stream, k1.p, v1.p, R, flags.p, ix->offsets);
        HIPCHK(hipGetLastError());
        if ((rc = scanExclusive<uint32_t>(ctx, tmp, flags.p, scan.p, R + 1)) != FSGPU_OK) return rc;
        uint32_t ne = 0;
        HIPCHK(hipMemcpyAsync(&ne, scan.p + R, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ix->nEntries = ne;
        {   // 4-byte entries while a target id and a position fit 32 bits together (FSGPU_KMER_ENTRY64=1 keeps the 8-byte form: A/B runs, tests)
            const int pbits = bitsFor((uint64_t) std::max(db.maxLen, 1) + 1);
            const char *e64 = getenv("FSGPU_KMER_ENTRY64");
            ix->posBits = (ix->tbits + pbits <= 32 && pbits <= 16 && !(e64 && atoi(e64) != 0)) ? pbits : 0;
        }
        if (ix->posBits) {
            HIPCHK(hipMalloc((void **) &ix->entries32, std::max<uint64_t>(ne, 1) * sizeof(uint32_t)));
            hipLaunchKernelGGL(k_kmer_compact_entries32, dim3(gridFor(R, 256)), dim3(256), 0, ctx->stream, v1.p, flags.p, scan.p, R, ix->posBits, ix->entries32);
        } else {
            HIPCHK(hipMalloc((void **) &ix->entries, std::max<uint64_t>(ne, 1) * sizeof(uint64_t)));
            hipLaunchKernelGGL(k_kmer_compact_entries, dim3(gridFor(R, 256)), dim3(256), 0, ctx->stream, v1.p, flags.p, scan.p, R, ix->entries);
        }
        HIPCHK(hipGetLastError());
    } else {
        HIPCHK(hipMalloc((void **) &ix->entries, sizeof(uint64_t)));
    }
    // counts -> offsets (in place)
    if ((rc = scanExclusive<uint32_t>(ctx, tmp, ix->offsets, ix->offsets, tableSize + 1)) != FSGPU_OK) return rc;
    HIPCHK(hipMalloc((void **) &ix->bitmap, (tableSize / 32) * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_kmer_bitmap, dim3(gridFor(tableSize / 32, 256)), dim3(256), 0, ctx->stream, ix->offsets, (uint32_t) (tableSize / 32), ix->bitmap);
    HIPCHK(hipGetLastError());
    ix->residues = R;
    if ((rc = buildCoarseLevels(ctx, *ix, db.hLengths)) != FSGPU_OK) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->kidx = ix;
    return FSGPU_OK;
}

// Test / inspection accessors: copy parts of the resident index to host memory (any pointer may be NULL).
int fsgpu_kmer_index_copy(fsgpu_ctx *ctx, uint32_t *offsets /*64e6+1*/, uint64_t *entries /*nEntries*/, uint8_t *masked /*db bytes*/) {
    if (!ctx) return FSGPU_E_ARG;
    if (!ctx->kidx) { ctx->err = "k-mer index not built"; return FSGPU_E_NODB; }
    const KmerIndex &ix = *ctx->kidx;
    if (offsets) HIPCHK(hipMemcpy(offsets, ix.offsets, (64000000ull + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (entries && ix.nEntries) {
        if (ix.posBits) {             // the accessor's format stays seqId << 16 | position
            KDev<uint64_t> wide;
            HIPCHK(kNew(wide, ix.nEntries));
            hipLaunchKernelGGL(k_kmer_widen_entries, dim3(gridFor(ix.nEntries, 256)), dim3(256), 0, ctx->stream, ix.entries32, ix.nEntries, ix.posBits, wide.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(ctx->stream));
            HIPCHK(hipMemcpy(entries, wide.p, ix.nEntries * sizeof(uint64_t), hipMemcpyDeviceToHost));
        } else HIPCHK(hipMemcpy(entries, ix.entries, ix.nEntries * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    if (masked && ix.db->bytes) HIPCHK(hipMemcpy(masked, ix.masked, ix.db->bytes, hipMemcpyDeviceToHost));
    return FSGPU_OK;
}
int fsgpu_kmer_batch_hint(const fsgpu_ctx *ctx) {
    if (!ctx || !ctx->kidx || ctx->kmerHitsPerQuery <= 0) return 32;
    int b = (int) std::min<double>(kmerMaxBatch(ctx->kidx->tbits), kKmerHitBudget / ctx->kmerHitsPerQuery);
    if (ctx->kmerBatchCap > 0) b = std::min(b, ctx->kmerBatchCap);
    return std::max(32, b / 32 * 32);
}
void fsgpu_kmer_last_segments(const fsgpu_ctx *ctx, uint32_t *out7) {
    for (int i = 0; i < 7; i++) out7[i] = ctx ? ctx->kmerSegs[i] : 0;
}
void fsgpu_kmer_last_counts(const fsgpu_ctx *ctx, uint64_t *out4) {
    for (int i = 0; i < 4; i++) out4[i] = ctx ? ctx->kmerCounts[i] : 0;
}
int fsgpu_kmer_row_copy(fsgpu_ctx *ctx, int row, int16_t *score /*8000*/, uint16_t *index /*8000*/) {
    if (!ctx || row < 0 || row >= kRow3) return FSGPU_E_ARG;
    if (!ctx->kidx) { ctx->err = "k-mer index not built"; return FSGPU_E_NODB; }
    HIPCHK(hipMemcpy(score, ctx->kidx->s3 + (size_t) row * kRow3, kRow3 * sizeof(int16_t), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(index, ctx->kidx->i3 + (size_t) row * kRow3, kRow3 * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return FSGPU_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------------------
namespace {

using HostOut = KmerOut;              // an element the device hands over, as the host tail reads it

unsigned pickBins(const fsgpu_kmer_search_params &p, uint64_t n) {
    if (p.bins) return (unsigned) p.bins;
    uint64_t l2 = p.l2CacheSize;
    if (l2 == 0) {
        long v = sysconf(_SC_LEVEL2_CACHE_SIZE);      // Util::getL2CacheSize (M/src/commons/Util.cpp:346-361)
        l2 = v > 0 ? (uint64_t) v : 262144;
    }
    for (unsigned x = 2; x <= 1024; x *= 2) if (n / x < l2) return x;
    return 2048;
}

int scalarDiag(const int8_t *profile, int len, const uint8_t *db) {
    int mx = 0, s = 0;
    for (int pos = 0; pos < len; pos++) { s += profile[pos * 21 + db[pos]]; s = s < 0 ? 0 : s; mx = s > mx ? s : mx; }
    return mx;
}

// The tail of QueryMatcher::matchQuery (:146-239) on the elements at or above the cut: array order of the reference
// = (bin = id & (B-1), then the order the overflow rounds left the elements in), radix by score, getResult, final sort.
// findDuplicates output capacity (CacheFriendlyOperations.cpp:217-219), conservative form: true when some chunk's candidates plus the elements the earlier
// rounds left reach foundDiagonalsSize, i.e. when the reference MAY have cut that chunk short (the exact, per-bin test is replayOutputTruncation's)
bool outputTestFires(const fsgpu_kmer_search_params &sp, uint64_t n, const KmerChunks &ck, const uint32_t *ec, const uint32_t *rounds) {
    const uint64_t foundSize = sp.foundDiagonalsSize ? (uint64_t) sp.foundDiagonalsSize : std::max<uint64_t>(n, 1000000);
    const uint32_t C = ck.nChunks - 1;
    const bool lastEmpty = ck.start[ck.nChunks] == ck.start[ck.nChunks - 1];
    if (ck.aborted != 0 || (C >= 1 && lastEmpty)) return false;          // answered empty / with another status
    for (uint32_t c = 0; c <= C; c++)
        if ((uint64_t) ec[c] + (c == 0 ? 0 : rounds[c]) >= foundSize) return true;
    return false;
}

int finishQuery(const fsgpu_kmer_search_params &sp, uint64_t n, const fsgpu_kmer_query &q, const KmerChunks &ck, const uint32_t *ec, const uint32_t *rounds,
                uint64_t resultSize, uint32_t thr, std::vector<HostOut> &el, fsgpu_kmer_hit *out, int32_t *nout, bool truncationReplayed) {
    const uint64_t big = std::max<uint64_t>(n, 1000000);
    const uint64_t foundSize = sp.foundDiagonalsSize ? (uint64_t) sp.foundDiagonalsSize : big;
    const size_t maxHits = (size_t) std::min<uint64_t>((uint64_t) sp.maxResListLen, n);
    const unsigned B = pickBins(sp, n);
    const uint32_t C = ck.nChunks - 1;
    int status = FSGPU_KMER_OK;
    bool empty = false;
    if (ck.aborted == 2) status = FSGPU_KMER_E_CHUNKS;
    if (ck.aborted == 1) empty = true;
    const bool lastEmpty = ck.start[ck.nChunks] == ck.start[ck.nChunks - 1];
    if (C >= 1 && lastEmpty) empty = true;
    // findDuplicates output capacity (CacheFriendlyOperations.cpp:217-219): conservative replay
    for (uint32_t c = 0; c <= C && status == FSGPU_KMER_OK && !empty && !truncationReplayed; c++) {
        if (c == C && lastEmpty) break;
        const uint64_t before = c == 0 ? 0 : rounds[c];
        if ((uint64_t) ec[c] + before >= foundSize) status = FSGPU_KMER_E_OUTPUT;
    }
    size_t cur = 0;
    // getResult: the query's own entry first, with the top raw score of the mode (UCHAR_MAX for KMER_SCORE, USHRT_MAX otherwise; QueryMatcher.cpp:409-421)
    if (q.identity >= 0 && maxHits > 0) { out[0].id = (uint32_t) q.identity; out[0].score = sp.kmerScoreOnly ? 255 : 65535; out[0].diagonal = 0; out[0].pad = 0; cur = 1; }
    if (status < 0) { *nout = 0; return status; }
    if (!empty && resultSize >= foundSize / 2) status = FSGPU_KMER_UNSTABLE;
    if (!empty && !el.empty()) {
        // order of the chunk runs in foundDiagonals after the overflow rounds (k-mer prefilter)
        std::vector<int> rank(C + 1, 0), dir(C + 1, 1);
        {
            std::vector<std::pair<int, int>> order;       // (chunk, direction)
            order.push_back({0, 1});
            for (uint32_t j = 2; j <= C; j++) {
                std::vector<std::pair<int, int>> nx;
                nx.push_back({(int) j - 1, -1});
                for (size_t z = order.size(); z-- > 0;) nx.push_back({order[z].first, -order[z].second});
                order.swap(nx);
            }
            if (C >= 1) order.push_back({(int) C, 1});
            for (size_t z = 0; z < order.size(); z++) { rank[order[z].first] = (int) z; dir[order[z].first] = order[z].second; }
            // --diag-score 0: mergeScoreDuplicates hands every element on in the order it came in -- the earlier rounds' elements, then the new
            // chunk's -- so a bin holds its elements by round of origin, each round's in arrival order of the first candidate
            if (sp.kmerScoreOnly) for (uint32_t c = 0; c <= C; c++) { rank[c] = (int) c; dir[c] = 1; }
        }
        auto chunkOf = [&](uint64_t g) { uint32_t c = 0; while (c + 1 < ck.nChunks && ck.start[c + 1] <= g) c++; return c; };
        // array order of the reference inside one score bucket: (bin, order the overflow rounds left the elements in)
        auto orderKey = [&](const HostOut &e, uint32_t &bin) {
            const uint32_t c = chunkOf(e.g);
            bin = e.id & (B - 1);
            return ((uint64_t) rank[c] << 40) | (dir[c] > 0 ? e.g : ((1ull << 40) - 1 - e.g));
        };
        struct Key { uint32_t count; uint32_t bin; uint64_t ok; const HostOut *e; };
        auto arrayOrder = [](const Key &a, const Key &b) { return a.bin != b.bin ? a.bin < b.bin : a.ok < b.ok; };
        const bool truncated = thr >= 255 && !sp.kmerScoreOnly;      // rescoreHits belongs to the diagonal-score mode only
        if (status == FSGPU_KMER_UNSTABLE) {
            // resultSize >= foundDiagonalsSize/2 (QueryMatcher.cpp:205-215): the reference compacts the elements at or above
            // the cut in array order and orders them with std::sort(sortScore), which is not stable.  The same call on the
            // same sequence reproduces its permutation wherever both sides use libstdc++'s introsort.
            std::vector<Key> ks(el.size());
            for (size_t i = 0; i < el.size(); i++) { uint32_t bin; const uint64_t ok = orderKey(el[i], bin); ks[i] = {el[i].count, bin, ok, &el[i]}; }
            std::sort(ks.begin(), ks.end(), arrayOrder);
            std::sort(ks.begin(), ks.end(), [](const Key &a, const Key &b) { return a.count > b.count; });
            for (size_t i = 0; i < ks.size() && cur < maxHits; i++) {
                if (q.identity >= 0 && (uint32_t) q.identity == ks[i].e->id) continue;
                fsgpu_kmer_hit &h = out[cur++];
                h.id = ks[i].e->id; h.diagonal = (uint16_t) ks[i].e->diag; h.pad = 0;
                h.score = ks[i].e->count >= 255 ? ks[i].e->score : (int32_t) ks[i].e->count;
            }
        } else if (truncated) {
            // rescoreHits (QueryMatcher.cpp:563-589): only the 255-capped hits survive, re-ranked by their real score
            std::vector<Key> ks(el.size());
            for (size_t i = 0; i < el.size(); i++) { uint32_t bin; const uint64_t ok = orderKey(el[i], bin); ks[i] = {el[i].count, bin, ok, &el[i]}; }
            std::sort(ks.begin(), ks.end(), arrayOrder);
            std::vector<uint8_t> clean(q.L);       // Sequence::numSequence of the query: soft-mask flag dropped
            for (int i = 0; i < q.L; i++) { uint8_t c = q.seq[i]; c = c >= 32 ? c - 32 : c; clean[i] = c > 20 ? 20 : c; }
            int maxSelf = scalarDiag(q.profile, q.L, clean.data()) - 255;
            maxSelf = std::max(1, maxSelf);
            maxSelf = std::min(maxSelf, 65535);
            const float fmax = (float) maxSelf;
            for (Key &k : ks) {
                unsigned ns = (unsigned) k.e->score - 255u;
                float sc = (float) std::min(ns, 65535u);
                k.count = (uint8_t) ((sc / fmax) * (float) 255 + 0.5);
            }
            const unsigned rescale = (unsigned) maxSelf;
            std::stable_sort(ks.begin(), ks.end(), [](const Key &a, const Key &b) { return a.count > b.count; });
            for (size_t i = 0; i < ks.size() && cur < maxHits; i++) {
                if (q.identity >= 0 && (uint32_t) q.identity == ks[i].e->id) continue;
                fsgpu_kmer_hit &h = out[cur++];
                h.id = ks[i].e->id; h.diagonal = (uint16_t) ks[i].e->diag; h.pad = 0;
                h.score = (int32_t) (255u + ks[i].count * rescale / 255u);
            }
        } else {
            // everything above the cut is taken (computeScoreThreshold leaves fewer than maxHits of them); the ties at the
            // cut fill the remaining slots in the reference's array order, so only they need the (bin, order) key
            std::vector<Key> ties;
            for (const HostOut &e : el) {
                if (q.identity >= 0 && (uint32_t) q.identity == e.id) continue;
                if (e.count > thr) {
                    if (cur < maxHits) {
                        fsgpu_kmer_hit &h = out[cur++];
                        h.id = e.id; h.diagonal = (uint16_t) e.diag; h.pad = 0;
                        h.score = e.count >= 255 ? e.score : (int32_t) e.count;
                    }
                } else if (e.count == thr) {
                    uint32_t bin; const uint64_t ok = orderKey(e, bin);
                    ties.push_back({e.count, bin, ok, &e});
                }
            }
            const size_t room = maxHits - cur;
            if (ties.size() > room) { std::nth_element(ties.begin(), ties.begin() + room, ties.end(), arrayOrder); ties.resize(room); }
            for (const Key &k : ties) {
                fsgpu_kmer_hit &h = out[cur++];
                h.id = k.e->id; h.diagonal = (uint16_t) k.e->diag; h.pad = 0;
                h.score = k.e->count >= 255 ? k.e->score : (int32_t) k.e->count;
            }
        }
    }
    if (cur > 1) {
        auto cmp = [](const fsgpu_kmer_hit &a, const fsgpu_kmer_hit &b) {
            const int aa = abs(a.score), bb = abs(b.score);
            return aa != bb ? aa > bb : a.id < b.id;
        };
        std::sort(out + (q.identity >= 0 ? 1 : 0), out + cur, cmp);
    }
    *nout = (int32_t) cur;
    return status;
}

// ---- host-only parts of a batch: plain functions of their inputs ------------------------------------------------
// tiles: every databaseHits chunk of every query is cut into tiles of kTileA consecutive hits (the chunk starts came back with the lists)
// The tile table, on the host and on the device (KmerTiles): [tileStart nT+1 | qTile0 nq+1 | vqTile0 nVq+1 | qVq0 nq+1] as u32, then [vqQ nVq] as u16.
// countTiles answers its size in bytes.
size_t countTiles(const KmerChunks *hck, int nq, uint32_t &nVq, uint32_t &nT) {
    nVq = nT = 0;
    for (int q = 0; q < nq; q++) {
        nVq += hck[q].nChunks;
        for (uint32_t c = 0; c < hck[q].nChunks; c++) nT += (uint32_t) ((hck[q].start[c + 1] - hck[q].start[c] + kTileA - 1) / kTileA);
    }
    return ((size_t) nT + 1 + nq + 1 + nVq + 1 + nq + 1) * sizeof(uint32_t) + (size_t) nVq * sizeof(uint16_t);
}
struct TileTable { uint32_t *tileStart, *qTile0, *vqTile0, *qVq0; uint16_t *vqQ; };
TileTable carveTiles(unsigned char *base, uint32_t nT, uint32_t nVq, int nq) {
    TileTable t;
    t.tileStart = (uint32_t *) base; t.qTile0 = t.tileStart + nT + 1; t.vqTile0 = t.qTile0 + nq + 1; t.qVq0 = t.vqTile0 + nVq + 1;
    t.vqQ = (uint16_t *) (t.qVq0 + nq + 1);
    return t;
}
bool fillTiles(const TileTable &t, const KmerChunks *hck, const KmerQ *hq, int nq, uint64_t nHits, uint32_t nT, uint32_t nVq) {
    uint32_t T = 0, v = 0;
    for (int q = 0; q < nq; q++) {
        t.qTile0[q] = T; t.qVq0[q] = v;
        for (uint32_t c = 0; c < hck[q].nChunks; c++, v++) {
            t.vqTile0[v] = T; t.vqQ[v] = (uint16_t) q;
            for (uint64_t o = hck[q].start[c]; o < hck[q].start[c + 1]; o += kTileA) t.tileStart[T++] = (uint32_t) (hq[q].hitBase + o);
        }
    }
    t.qTile0[nq] = T; t.qVq0[nq] = v; t.vqTile0[nVq] = T; t.tileStart[T] = (uint32_t) nHits;
    return T == nT && v == nVq;
}
// granularity of the coarse keys: at most 256 keys of 1, 2, 4 ... blocks of 1024 ids (245 keys of 4096 ids at 1M targets: measured best there -- more
// keys shorten the scatter's runs, fewer widen the duplicate stage's tables and thin out its waves); when the (query, chunk, key) runs would
// average fewer than 1024 hits -- the many-queries-few-hits batches of an all-vs-all search -- the coarsest level of at most 16 blocks per key
const KmerIndex::CoarseLevel *pickCoarseLevel(const std::vector<KmerIndex::CoarseLevel> &levels, uint64_t nHits, uint32_t nVq, int forced) {
    const KmerIndex::CoarseLevel *lv = nullptr;
    for (const KmerIndex::CoarseLevel &l : levels) if (l.blocksPerKey >= 1 && (lv == nullptr || lv->nKeys > 256)) lv = &l;
    if (lv == nullptr) lv = &levels.front();
    if ((double) nHits / ((double) nVq * lv->nKeys) < 1024.0)
        for (const KmerIndex::CoarseLevel &l : levels) if (l.blocksPerKey >= 1 && l.blocksPerKey <= 16 && l.nKeys <= lv->nKeys) lv = &l;
    if (forced >= 0) lv = &levels[std::min<size_t>(levels.size() - 1, (size_t) forced)];   // tests: force a level
    return lv;
}
// the bin at which findDuplicates runs out of its outSize output slots in one (query, chunk), 0xFFFFFFFF when it does not: h holds the two counts
// per bin that k_kmer_trunc_hist collected
uint32_t truncationCut(const uint32_t *h, uint32_t bins, uint64_t outSize) {
    uint64_t dbl = 0;
    for (uint32_t b = 0; b < bins; b++) {
        if (dbl + h[2 * b] >= outSize) return b;
        dbl += h[2 * b + 1];
    }
    return 0xFFFFFFFFu;
}

} // namespace

// ---- one device batch: kmerBatch runs the stage functions below in order, each on the state of the batch (KmerBatch) ----------------------
// environment switches of a batch (A/B runs, tests), read once at its top; -1: not set, the batch decides
struct KmerSwitches {
    int wave = -1;            // FSGPU_KMER_WAVE = 0 / 1: workgroup / wave per query position, in the count and in the list pass
    int waveSmall = -1;       // FSGPU_KMER_WAVE_SMALL = 0 / 1: the large / small LDS form of the wave list pass
    int binLevel = -1;        // FSGPU_KMER_BIN_LEVEL: index of the coarse-key level
    bool score8 = true;       // eight lanes per candidate (k_kmer_score8) unless FSGPU_KMER_SCORE8=0 asks for the one-lane-per-candidate form (A/B runs)
    bool walkFF = true;       // FSGPU_KMER_WALK_FF=0: every round of every target is walked (A/B runs; the truncation replay always uses that form)
};
static KmerSwitches readSwitches() {
    KmerSwitches w;
    if (const char *e = getenv("FSGPU_KMER_WAVE")) w.wave = atoi(e) != 0;
    if (const char *e = getenv("FSGPU_KMER_WAVE_SMALL")) w.waveSmall = *e ? atoi(e) : -1;
    if (const char *e = getenv("FSGPU_KMER_BIN_LEVEL")) w.binLevel = std::max(0, atoi(e));
    if (const char *e = getenv("FSGPU_KMER_SCORE8")) w.score8 = atoi(e) != 0;
    if (const char *e = getenv("FSGPU_KMER_WALK_FF")) w.walkFF = atoi(e) != 0;
    return w;
}

struct KmerBatch {
    fsgpu_ctx *ctx; KmerScratch &S; const KmerIndex &ix; const fsgpu_kmer_search_params &sp; const fsgpu_kmer_query *queries; int nq; hipStream_t st;
    KmerSwitches sw;
    const fsgpu_kmer_profile_query *pq = nullptr;    // profile form: the same nq queries with their raw score rows (queries[] then carries letters, profile, identity)
    uint64_t nPos = 0, nLists = 0, nHits = 0;
    uint32_t nCand = 0, maxChunks = 1;               // maxChunks: the most chunks (databaseHits refills + 1) a query of the batch has
    const KmerChunks *hck = nullptr;                 // the chunk tables on the host (S.hChunks): from kmerSimilar on
    KmerTiles tl{};                                  // tile table, coarse-key level: from kmerPartition on
    const KmerIndex::CoarseLevel *lv = nullptr; KmerCoarse co{};
    std::vector<char> truncReplayed;                 // per query; empty: no truncation replay ran
    std::vector<size_t> outOff; size_t totalOut = 0; // [nq + 1] where a query's elements stand in S.hOut, and how many there are: from kmerHandOver on
    // FSGPU_KMER_TRACE=1: host wall clock of the phases of a batch on stderr (where a feeder thread's time goes between the device stages)
    bool trace = false; std::chrono::steady_clock::time_point tPrev; std::string traceLine;
    void mark(const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        char b[64];
        snprintf(b, sizeof(b), " %s %.3f", what, std::chrono::duration<double, std::milli>(now - tPrev).count());
        traceLine += b; tPrev = now;
    }
};

// The halving rule.  kKmerHalve is what kmerBatch and its stages answer when the caller is to halve the batch and redo it (no FSGPU_* code is positive).
// KCHK passes every failure on and turns FSGPU_E_NOMEM of a batch of several queries into it: nothing of this attempt may still read the staging buffers.
constexpr int kKmerHalve = 1;
#define KCHK(x) do { const int rc_ = (x); if (rc_ == FSGPU_E_NOMEM && B.nq > 1) { (void) hipStreamSynchronize(B.ctx->stream); return kKmerHalve; } if (rc_ != FSGPU_OK) return rc_; } while (0)

// ---- stage the batch: validation, pinned copies of the queries, uploads, cleared counters ------------------------
static int kmerStageQueries(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    const fsgpu_kmer_query *queries = B.queries;
    uint64_t &nPos = B.nPos, seqBytes = 0, profBytes = 0, nRows = 0;
    for (int q = 0; q < nq; q++) {
        const int L = queries[q].L;
        if (L < 0 || L > FSGPU_MAX_SEQ_LEN || (L > 0 && (!queries[q].seq || !queries[q].profile))) { ctx->err = "k-mer search: bad query"; return FSGPU_E_ARG; }
        if (L >= 32768) { ctx->err = "k-mer search: queries of 32768 residues or more are not supported on the device"; return FSGPU_E_UNSUPPORTED; }
        if (B.pq && L > 0 && !B.pq[q].scores) { ctx->err = "k-mer search: profile query without score rows"; return FSGPU_E_ARG; }
        nPos += (uint64_t) std::max(0, L - ix.pat.size + 1);
        seqBytes += (uint64_t) L + 16;
        profBytes += (uint64_t) L * 21 + 16;
        nRows += (uint64_t) L;
    }
    S.profNq = 0; S.profNPos = S.profNLists = 0;
    KCHK(ensureAllK(ctx, S.hQs, nq, S.hPosQuery, nPos + 1, S.hSeqs, seqBytes, S.hThrs, nPos + 1, S.hProfiles, profBytes));
    if (B.pq) {
        // the rows are sorted here, once per query position, the way Sequence::mapProfile leaves them (Util::rankedDescSort20): the kernels read them as they are
        KCHK(ensureAllK(ctx, S.hRows, nRows * 20 + 1, S.hRowBase, nq, S.rows, nRows * 20 + 1, S.rowBase, nq));
        uint64_t ro = 0;
        for (int q = 0; q < nq; q++) { S.hRowBase.p[q] = ro; ro += (uint64_t) queries[q].L; }
        fshostParallelFor(nq, [&](int q) { if (queries[q].L > 0) fsgpu_kmer_profile_sort_rows(B.pq[q].scores, queries[q].L, S.hRows.p + S.hRowBase.p[q] * 20); });
    }
    KmerQ *hq = S.hQs.p;
    uint64_t pb = 0, so = 0, po = 0;
    for (int q = 0; q < nq; q++) {
        const int L = queries[q].L;
        const uint32_t np = (uint32_t) std::max(0, L - ix.pat.size + 1);
        hq[q].posBase = (uint32_t) pb; hq[q].nPos = np; hq[q].seqOff = (uint32_t) so; hq[q].L = (uint32_t) L; hq[q].profOff = (uint32_t) po;
        hq[q].pad = 0; hq[q].hitBase = 0; hq[q].listBase = 0;
        uint8_t *sd = S.hSeqs.p + so;
        for (int i = 0; i < L; i++) { uint8_t c = queries[q].seq[i]; c = c >= 32 ? c - 32 : c; sd[i] = c > 20 ? 20 : c; }
        memset(sd + L, 20, 16);
        if (L) memcpy(S.hProfiles.p + po, queries[q].profile, (size_t) L * 21);
        // a profile query has no composition bias (QueryMatcher.cpp:109-117): every position's threshold is max(kmerThr, 0) (:271)
        const int16_t pthr = B.pq ? (int16_t) std::min(std::max(B.pq[q].kmerThr, 0), 32767) : 0;
        for (uint32_t i = 0; i < np; i++) {
            S.hPosQuery.p[pb + i] = (uint16_t) q;
            S.hThrs.p[pb + i] = B.pq ? pthr : queries[q].kmerThr ? queries[q].kmerThr[i] : (int16_t) ix.p.kmerThr;
        }
        pb += np; so += (uint64_t) L + 16; po += (uint64_t) L * 21 + 16;
    }
    const size_t perChunk = (size_t) nq * kMaxChunks;
    KCHK(ensureAllK(ctx, S.qs, nq, S.posQuery, nPos + 1, S.seqs, seqBytes, S.thrs, nPos + 1, S.profiles, profBytes, S.K, nPos + 1, S.Kbase, nPos + 1, S.chunks, nq));
    KCHK(ensureAllK(ctx, S.ec, perChunk, S.rounds, perChunk, S.resSize, nq, S.hist, (size_t) nq * 256, S.thr, nq, S.outCount, nq, S.nCand, 16));
    KCHK(ensureAllK(ctx, S.hMisc, 32, S.hChunks, nq, S.hEc, perChunk, S.hRounds, perChunk, S.hResSize, nq, S.hThr, nq, S.hOutCount, nq));
    B.mark("stage");
    HIPCHK(hipEventRecord(S.ev[0], st));
    HIPCHK(kCopy(S.qs.p, S.hQs.p, nq, hipMemcpyHostToDevice, st));
    HIPCHK(kCopy(S.posQuery.p, S.hPosQuery.p, nPos + 1, hipMemcpyHostToDevice, st));
    HIPCHK(kCopy(S.seqs.p, S.hSeqs.p, seqBytes, hipMemcpyHostToDevice, st));
    HIPCHK(kCopy(S.thrs.p, S.hThrs.p, nPos + 1, hipMemcpyHostToDevice, st));
    HIPCHK(kCopy(S.profiles.p, S.hProfiles.p, profBytes, hipMemcpyHostToDevice, st));
    if (B.pq) {
        if (nRows) HIPCHK(kCopy(S.rows.p, S.hRows.p, nRows * 20, hipMemcpyHostToDevice, st));
        HIPCHK(kCopy(S.rowBase.p, S.hRowBase.p, nq, hipMemcpyHostToDevice, st));
    }
    HIPCHK(kZero(S.ec.p, perChunk, st));
    HIPCHK(kZero(S.rounds.p, perChunk, st));
    HIPCHK(kZero(S.resSize.p, nq, st));
    HIPCHK(kZero(S.hist.p, (size_t) nq * 256, st));
    HIPCHK(kZero(S.outCount.p, nq, st));
    HIPCHK(kZero(S.nCand.p, 16, st));
    return FSGPU_OK;
}

// ---- stage 1: similar k-mers -> lists ---------------------------------------------------------------------
// one workgroup or one wave per query position (k_kmer.hpp): the wave form when positions have few similar k-mers -- for the count pass
// judged by the previous batch of this context, for the list pass by this batch's own count.  FSGPU_KMER_WAVE = 0 / 1 forces a form.
static int kmerSimilar(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    const uint64_t nPos = B.nPos, maxDbMatches = B.sp.maxDbMatches ? (uint64_t) B.sp.maxDbMatches : std::max<uint64_t>(ix.n, 1000000) * 2;
    ctx->kmerForm[0] = ctx->kmerForm[1] = 0;
    if (nPos && B.pq) {
        // profile form: one workgroup per position builds the count tables of its six rows (k_kmer_profile.hpp)
        ctx->kmerForm[0] = 1;
        hipLaunchKernelGGL(k_kmer_count_p, dim3((unsigned) nPos), dim3(kKmerBlock), 0, st, S.qs.p, S.posQuery.p, S.seqs.p, S.thrs.p, S.rows.p, S.rowBase.p, (uint32_t) nPos,
                           ix.pat, S.K.p);
        HIPCHK(hipGetLastError());
    } else if (nPos) {
        const bool w = B.sw.wave >= 0 ? B.sw.wave != 0 : (ctx->kmerKPerPos > 0 && ctx->kmerKPerPos < 2048);
        ctx->kmerForm[0] = w ? 2 : 1;
        auto count = [&](auto kernel, unsigned grid, unsigned block) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, S.qs.p, S.posQuery.p, S.seqs.p, S.thrs.p, (uint32_t) nPos, ix.pat, ix.s3, S.K.p);
        };
        if (w) count(k_kmer_count_w, (unsigned) ((nPos + 3) / 4), 256);
        else count(k_kmer_count, (unsigned) nPos, kKmerBlock);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(kZero(S.K.p + nPos, 1, st));
    KCHK(scanExclusive32to64(ctx, S.tmp, S.K.p, S.Kbase.p, nPos + 1));
    HIPCHK(kCopy(&S.hMisc.p[0], S.Kbase.p + nPos, 1, hipMemcpyDeviceToHost, st));
    KCHK(syncStream(ctx));
    const uint64_t nLists = B.nLists = S.hMisc.p[0];
    B.mark("count+sync");
    if (nLists >= 0xFFFFFF00ull) {                        // list slots are 32-bit in k_kmer_tile_lists (and 20 bytes of scratch each)
        if (nq > 1) return kKmerHalve;
        ctx->err = "k-mer search: a single query produces more than 2^32 similar k-mers"; return FSGPU_E_UNSUPPORTED;
    }
    HIPCHK(hipEventRecord(S.ev[1], st));
    KCHK(ensureAllK(ctx, S.listStart, nLists + 1, S.listSize, nLists + 1, S.listPos, nLists + 1, S.listP, nLists + 1));
    if (nLists && B.pq) {
        HIPCHK(hipEventRecord(S.ev[10], st));
        ctx->kmerForm[1] = 1;
        hipLaunchKernelGGL(k_kmer_lists_p<false>, dim3((unsigned) (nPos + nLists / kListSlice + 1)), dim3(kKmerBlock), 0, st, S.qs.p, S.posQuery.p, S.seqs.p, S.thrs.p, S.rows.p,
                           S.rowBase.p, (uint32_t) nPos, ix.pat, S.K.p, S.Kbase.p, ix.offsets, ix.bitmap, S.listStart.p, S.listSize.p, S.listPos.p, 0u, (uint32_t *) nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S.ev[11], st));
    } else if (nLists) {
        HIPCHK(hipEventRecord(S.ev[10], st));
        ctx->kmerKPerPos = (double) nLists / (double) std::max<uint64_t>(nPos, 1);
        ctx->kmerForm[1] = (B.sw.wave >= 0 ? B.sw.wave != 0 : ctx->kmerKPerPos < 2048) ? 2 : 1;
        auto lists = [&](auto kernel, unsigned grid, unsigned block) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, S.qs.p, S.posQuery.p, S.seqs.p, S.thrs.p, (uint32_t) nPos, ix.pat, ix.s3, ix.i3, S.K.p, S.Kbase.p,
                               ix.offsets, ix.bitmap, S.listStart.p, S.listSize.p, S.listPos.p);
        };
        // few similar k-mers per position: the small LDS form (more waves per SIMD); FSGPU_KMER_WAVE_SMALL = 0 / 1 forces a form (A/B)
        const bool small = B.sw.waveSmall >= 0 ? B.sw.waveSmall != 0 : ctx->kmerKPerPos < 128;
        const unsigned waveGrid = (unsigned) ((nPos + 3) / 4);
        if (ctx->kmerForm[1] != 2) lists(k_kmer_lists, (unsigned) (nPos + nLists / kListSlice + 1), kKmerBlock);
        else if (small) lists(k_kmer_lists_w<128, 64>, waveGrid, 256);
        else lists(k_kmer_lists_w<kWaveRowCap, kWaveRuns>, waveGrid, 256);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S.ev[11], st));
    }
    HIPCHK(kZero(S.listSize.p + nLists, 1, st));
    KCHK(scanExclusive32to64(ctx, S.tmp, S.listSize.p, S.listP.p, nLists + 1));
    hipLaunchKernelGGL(k_kmer_qbases, dim3(gridFor(nq, 64)), dim3(64), 0, st, S.qs.p, nq, S.Kbase.p, S.listP.p);
    hipLaunchKernelGGL(k_kmer_chunks, dim3(gridFor(nq, 64)), dim3(64), 0, st, S.qs.p, nq, S.Kbase.p, S.listP.p, S.listPos.p, maxDbMatches, S.chunks.p);
    HIPCHK(hipGetLastError());
    HIPCHK(kCopy(&S.hMisc.p[1], S.listP.p + nLists, 1, hipMemcpyDeviceToHost, st));
    // the chunk tables: 2 KB per query, of which a query uses nChunks + 1 entries -- a batch of 1024 all-vs-all queries (one or two chunks each) sent 2.1 MB
    // over PCIe; large batches copy the header + the first nine entries of every query and fetch the rest only when a query has more than eight chunks
    constexpr size_t kChunkHead = offsetof(KmerChunks, start) + 9 * sizeof(uint64_t);
    const bool compactChunks = nq > 64;
    if (compactChunks) HIPCHK(hipMemcpy2DAsync(S.hChunks.p, sizeof(KmerChunks), S.chunks.p, sizeof(KmerChunks), kChunkHead, (size_t) nq, hipMemcpyDeviceToHost, st));
    else HIPCHK(kCopy(S.hChunks.p, S.chunks.p, nq, hipMemcpyDeviceToHost, st));
    HIPCHK(kCopy(S.hQs.p, S.qs.p, nq, hipMemcpyDeviceToHost, st));
    KCHK(syncStream(ctx));
    B.hck = S.hChunks.p;
    if (B.pq) { S.profNq = nq; S.profNPos = nPos; S.profNLists = nLists; }
    for (int q = 0; q < nq; q++) B.maxChunks = std::max<uint32_t>(B.maxChunks, B.hck[q].nChunks);
    if (compactChunks && B.maxChunks > 8) {
        const size_t upTo = offsetof(KmerChunks, start) + ((size_t) std::min<uint32_t>(B.maxChunks, kMaxChunks) + 1) * sizeof(uint64_t);
        HIPCHK(hipMemcpy2DAsync((char *) S.hChunks.p + kChunkHead, sizeof(KmerChunks), (const char *) S.chunks.p + kChunkHead, sizeof(KmerChunks), upTo - kChunkHead, (size_t) nq,
                                hipMemcpyDeviceToHost, st));
        KCHK(syncStream(ctx));
    }
    B.nHits = S.hMisc.p[1];
    B.mark("lists+sync");
    HIPCHK(hipEventRecord(S.ev[2], st));
    if (B.nHits >= 0xFFFFFF00ull) {
        if (nq > 1) return kKmerHalve;
        ctx->err = "k-mer search: a single query produces more than 2^32 index hits"; return FSGPU_E_UNSUPPORTED;
    }
    // the batch was sized from the PREVIOUS batch's hits per query: one that comes out far beyond the budget (long queries after short
    // ones, a first call with many queries) is split here, where its size is known and none of the 24-bytes-per-hit scratch exists yet
    if (nq > 1 && (double) B.nHits > 2.0 * kKmerHitBudget) return kKmerHalve;
    return FSGPU_OK;
}

// ---- stage 2: hit stream -> (query, key) runs in arrival order (k_kmer.hpp) -----------------------------------------------
static int kmerPartition(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    uint32_t nVq = 0, nT = 0;
    const size_t tilesBytes = countTiles(B.hck, nq, nVq, nT);
    KCHK(ensureAllK(ctx, S.hTiles, tilesBytes, S.tiles, tilesBytes));
    if (!fillTiles(carveTiles(S.hTiles.p, nT, nVq, nq), B.hck, S.hQs.p, nq, B.nHits, nT, nVq)) { ctx->err = "k-mer search: inconsistent tile table"; return FSGPU_E_HIP; }
    HIPCHK(kCopy(S.tiles.p, S.hTiles.p, tilesBytes, hipMemcpyHostToDevice, st));
    const TileTable dt = carveTiles(S.tiles.p, nT, nVq, nq);
    const KmerTiles tl{dt.tileStart, dt.qTile0, dt.vqTile0, dt.qVq0, dt.vqQ, nT, nVq};
    const KmerIndex::CoarseLevel *lv = pickCoarseLevel(ix.levels, B.nHits, nVq, B.sw.binLevel);
    const uint32_t nKeys = lv->nKeys;
    const bool blkInLds = (size_t) lv->nBlk * sizeof(uint16_t) <= 16 * 1024;
    const KmerCoarse co{lv->blkKey, lv->keyFirst, lv->nBlk, nKeys, (uint32_t) bitsFor(nKeys), lv->maxIds};
    B.tl = tl; B.lv = lv; B.co = co;
    const size_t nCells = (size_t) nT * nKeys, nSegs = (size_t) nq * nKeys;
    KCHK(ensureAllK(ctx, S.rec, B.nHits, S.recKey, B.nHits, S.recA, B.nHits, S.ordA, B.nHits, S.cntA, std::max<size_t>(nCells, 1), S.colA, std::max<size_t>(nCells, 1)));
    KCHK(ensureAllK(ctx, S.grpSum, nSegs * kColGroups, S.segCnt, nSegs + 1, S.segStart, nSegs + 1));
    HIPCHK(kZero(S.cntA.p, nCells, st));
    HIPCHK(kZero(S.segCnt.p + nSegs, 1, st));
    const uint32_t nEmit = nT * kSubTiles;
    KCHK(ensureK(ctx, S.tileL, (size_t) nEmit * 2));
    hipLaunchKernelGGL(k_kmer_tile_lists, dim3(gridFor((uint64_t) nEmit * 2, 256)), dim3(256), 0, st, S.listP.p, B.nLists, tl.tileStart, nT, S.tileL.p);
    const size_t ldsEmit = blkInLds ? (size_t) lv->nBlk * sizeof(uint16_t) : 0;
    auto emit = [&](auto kernel, auto entries, int posBits) {
        hipLaunchKernelGGL(kernel, dim3(nEmit), dim3(256), ldsEmit, st, B.nLists, S.listP.p, S.listStart.p, S.listPos.p, S.tileL.p, entries, posBits, tl.tileStart, co,
                           blkInLds ? 1 : 0, S.cntA.p, S.rec.p, S.recKey.p);
    };
    if (ix.posBits) emit(k_kmer_emit<uint32_t>, ix.entries32, ix.posBits);
    else emit(k_kmer_emit<uint64_t>, ix.entries, 16);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[3], st));
    // where every (tile, key) run starts: column sums -> segment starts -> column prefixes (in place of the counts)
    const dim3 colGrid((unsigned) nq, (nKeys + 63) / 64);
    hipLaunchKernelGGL(k_kmer_col_sums, colGrid, dim3(64 * kColGroups), 0, st, S.cntA.p, tl.qTile0, nKeys, S.grpSum.p, S.segCnt.p);
    KCHK(scanExclusive<uint32_t>(ctx, S.tmp, S.segCnt.p, S.segStart.p, nSegs + 1));
    hipLaunchKernelGGL(k_kmer_col_offsets, colGrid, dim3(64 * kColGroups), 0, st, S.cntA.p, tl.qTile0, nKeys, S.grpSum.p, S.segStart.p, S.colA.p);
#define FS_SCATTER(KB) hipLaunchKernelGGL(k_kmer_scatter_stable<KB>, dim3(nT), dim3(kScThreads), 0, st, S.rec.p, S.recKey.p, tl.tileStart, S.cntA.p, nKeys, S.recA.p, S.ordA.p)
    switch (co.keyBits) {          // ballots per record = key bits: unrolled per width
        case 1: FS_SCATTER(1); break; case 2: FS_SCATTER(2); break; case 3: FS_SCATTER(3); break; case 4: FS_SCATTER(4); break; case 5: FS_SCATTER(5); break;
        case 6: FS_SCATTER(6); break; case 7: FS_SCATTER(7); break; case 8: FS_SCATTER(8); break; default: FS_SCATTER(9); break;
    }
#undef FS_SCATTER
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[4], st));
    return FSGPU_OK;
}

// ---- stage 3: the double-diagonal rule, run by run in arrival order -> candidates in (query, target, arrival) order ------------------------
static int kmerCandidates(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    const uint32_t nKeys = B.co.nKeys, nVq = B.tl.nVq, nRuns = nVq * nKeys, maxIds = B.lv->maxIds;
    KCHK(ensureK(ctx, S.candCount, ((size_t) nRuns + 1) * 2));
    uint32_t *runBase = S.candCount.p + nRuns + 1;
    KmerDupStream da{};
    da.recA = S.recA.p; da.ordA = S.ordA.p; da.note = S.rec.p; da.offA = S.cntA.p; da.colA = S.colA.p; da.segStart = S.segStart.p; da.tl = B.tl; da.qs = S.qs.p;
    da.keyFirst = B.lv->keyFirst; da.nKeys = nKeys; da.tbits = ix.tbits; da.ecCount = S.ec.p; da.runCand = S.candCount.p; da.runBase = runBase;
    HIPCHK(kZero(S.candCount.p, (size_t) nRuns + 1, st));
    const size_t ldsDup = ((size_t) maxIds / 4 + 1) * sizeof(uint32_t);          // one byte per target id of the widest key
    if (ldsDup > 60 * 1024 && !ctx->kmerDupAttr) {          // the attribute belongs to the device: once per context
        HIPCHK(hipFuncSetAttribute((const void *) k_kmer_dup_stream, hipFuncAttributeMaxDynamicSharedMemorySize, (kCoarseBlocks * 1024 / 4 + 1) * (int) sizeof(uint32_t)));
        ctx->kmerDupAttr = true;
    }
    hipLaunchKernelGGL(k_kmer_dup_stream, dim3(nRuns), dim3(64), ldsDup, st, da);
    HIPCHK(hipGetLastError());
    KCHK(scanExclusive<uint32_t>(ctx, S.tmp, da.runCand, runBase, (size_t) nRuns + 1));
    HIPCHK(kCopy((uint32_t *) &S.hMisc.p[2], runBase + nRuns, 1, hipMemcpyDeviceToHost, st));
    KCHK(syncStream(ctx));
    B.nCand = (uint32_t) S.hMisc.p[2];
    B.mark("emit..dup+sync");
    ctx->kmerSegs[0] = 0; ctx->kmerSegs[1] = nVq * nKeys; ctx->kmerSegs[2] = 0; ctx->kmerSegs[3] = B.tl.nT;
    ctx->kmerSegs[4] = nVq * nKeys; ctx->kmerSegs[5] = nKeys; ctx->kmerSegs[6] = maxIds;
    if (!B.nCand) return FSGPU_OK;
    // (query, target, arrival) order: the gathered candidates stand in (query, key) blocks with ascending stream positions, one STABLE radix sort by
    // (query | target) over the flagged hits finishes it
    const int qtBits = ix.tbits + bitsFor((uint64_t) std::max(nq, 2));
    KCHK(ensureAllK(ctx, S.candKey, B.nCand, S.candVal, B.nCand, S.ckeys, B.nCand, S.cvals, B.nCand));
    da.candKey = S.candKey.p; da.candVal = S.candVal.p;
    hipLaunchKernelGGL(k_kmer_cand_gather, dim3((nRuns + 3) / 4), dim3(256), 0, st, da, nRuns);
    HIPCHK(hipGetLastError());
    KCHK((sortPairs<uint32_t, uint64_t>(ctx, S.tmp, S.candKey.p, S.ckeys.p, S.candVal.p, S.cvals.p, B.nCand, std::min(32, qtBits))));
    HIPCHK(kCopy(S.nCand.p, runBase + nRuns, 1, hipMemcpyDeviceToDevice, st));
    return FSGPU_OK;
}

// ---- stage 4: per-target replay; FF = false walks every round of every target ------------------------------------------
template <bool FF> static void launchWalk(const KmerBatch &B) {
    const KmerScratch &S = B.S;
    hipLaunchKernelGGL(k_kmer_walk<FF>, dim3(gridFor(B.nCand, 128)), dim3(128), 0, B.st, S.ckeys.p, S.cvals.p, S.kept.p, S.score.p, S.candTotal(), B.ix.tbits, S.chunks.p,
                       S.scrA.p, S.scrB.p, S.best.p, S.rounds.p, S.resSize.p);
}

// ---- score the candidates' diagonals and replay the reference's rounds per target, or (--diag-score 0) count the candidates ----------------
static int kmerScore(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    const uint32_t nCand = B.nCand; const int tbits = ix.tbits;
    KCHK(ensureAllK(ctx, S.kept, nCand, S.score, nCand, S.scrA, nCand, S.scrB, nCand, S.best, nCand, S.out, nCand));
    if (B.sp.kmerScoreOnly) {
        // --diag-score 0: the score of a target is the number of its candidates, no diagonal is scored; a query that refilled databaseHits has
        // the reference's merge of the per-refill counts replayed per (query, id >> shift) group (k_kmer_merge_heads)
        bool refilled = false;
        for (int q = 0; q < nq; q++) refilled = refilled || B.hck[q].nChunks > 1;
        if (refilled) {
            const unsigned bins = pickBins(B.sp, ix.n);
            int shift = 0;
            while ((1u << shift) < bins) shift++;
            hipLaunchKernelGGL(k_kmer_merge_heads, dim3(gridFor(nCand, 128)), dim3(128), 0, st, S.ckeys.p, S.cvals.p, S.candTotal(), tbits, shift, S.chunks.p, S.ec.p,
                               S.scrA.p, S.kept.p, S.score.p, S.best.p, S.rounds.p, S.resSize.p);
        } else hipLaunchKernelGGL(k_kmer_count_heads, dim3(gridFor(nCand, 256)), dim3(256), 0, st, S.ckeys.p, S.candTotal(), tbits, S.kept.p, S.score.p, S.best.p, S.resSize.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(S.ev[6], st));
        HIPCHK(hipEventRecord(S.ev[7], st));
        return FSGPU_OK;
    }
    int maxL = 0;
    for (int q = 0; q < nq; q++) maxL = std::max(maxL, B.queries[q].L);
    const int ldsBytes = std::min(maxL * 21, 60 * 1024);
    auto score = [&](auto kernel, unsigned perBlock) {
        hipLaunchKernelGGL(kernel, dim3(gridFor(nCand, perBlock)), dim3(256), (size_t) ldsBytes, st, S.ckeys.p, S.cvals.p, S.candTotal(), tbits, S.qs.p, S.profiles.p, ix.masked,
                           ix.db->dOffsets, ix.db->dLengths, ldsBytes, S.kept.p, S.score.p);
    };
    if (B.sw.score8) score(k_kmer_score8, 32);
    else score(k_kmer_score, 256);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[6], st));
    if (B.sw.walkFF) launchWalk<true>(B);
    else launchWalk<false>(B);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(S.ev[7], st));
    return FSGPU_OK;
}

// ---- stage 5: histogram, cut, hand-over (the normal pass, and once more after a truncation replay) -------------------------------
static int kmerSelect(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    const uint32_t nCand = B.nCand, maxHits = (uint32_t) std::min<uint64_t>((uint64_t) B.sp.maxResListLen, ix.n);
    hipLaunchKernelGGL(k_kmer_hist, dim3(gridFor(nCand, 256)), dim3(256), 0, st, S.ckeys.p, S.best.p, S.candTotal(), ix.tbits, S.hist.p);
    hipLaunchKernelGGL(k_kmer_cut, dim3(gridFor(nq, 64)), dim3(64), 0, st, S.hist.p, nq, maxHits, (uint32_t) B.sp.minDiagScoreThr, S.thr.p);
    hipLaunchKernelGGL(k_kmer_out, dim3(gridFor(nCand, 1024)), dim3(1024), 0, st, S.ckeys.p, S.cvals.p, S.score.p, S.best.p, S.candTotal(), ix.tbits, S.thr.p, nCand,
                       S.outCount.p, S.outTotal(), S.out.p, S.scrA.p, S.scrB.p);
    HIPCHK(hipGetLastError());
    return FSGPU_OK;
}

// ---- the per-query counters of the batch come back -----------------------------------------------------------------
static int kmerCounters(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const hipStream_t st = B.st; const int nq = B.nq;
    // per (query, chunk) counters: the host reads entries [0, nChunks) of a query only -- the columns the batch uses come back, not the 2 x 1 KB per query
    // (a batch of 1024 all-vs-all queries with one or two chunks each sent 2 MB over PCIe for 8 KB)
    const size_t pitch = (size_t) kMaxChunks * sizeof(uint32_t), width = (size_t) std::min<uint32_t>(B.maxChunks, kMaxChunks) * sizeof(uint32_t);
    HIPCHK(hipMemcpy2DAsync(S.hEc.p, pitch, S.ec.p, pitch, width, (size_t) nq, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpy2DAsync(S.hRounds.p, pitch, S.rounds.p, pitch, width, (size_t) nq, hipMemcpyDeviceToHost, st));
    HIPCHK(kCopy(S.hResSize.p, S.resSize.p, nq, hipMemcpyDeviceToHost, st));
    HIPCHK(kCopy(S.hThr.p, S.thr.p, nq, hipMemcpyDeviceToHost, st));
    HIPCHK(kCopy(S.hOutCount.p, S.outCount.p, nq, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(S.ev[8], st));
    KCHK(syncStream(ctx));
    B.mark("score..out+sync");
    return FSGPU_OK;
}

// ---- findDuplicates cut short by its output capacity: replayed per (query, chunk) in the diagonal-score mode -----------------------------
// (--diag-score 0 keeps the status: there the reference's next merge reads the bytes the aborted bin left behind)
static int kmerTruncation(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const KmerIndex &ix = B.ix; const hipStream_t st = B.st; const int nq = B.nq;
    const uint32_t nCand = B.nCand; const size_t perChunk = (size_t) nq * kMaxChunks;
    std::vector<int> flagged;
    for (int q = 0; q < nq; q++)
        if (outputTestFires(B.sp, ix.n, B.hck[q], S.hEc.p + (size_t) q * kMaxChunks, S.hRounds.p + (size_t) q * kMaxChunks)) flagged.push_back(q);
    const uint32_t bins = pickBins(B.sp, ix.n);
    const size_t histWords = flagged.size() * (size_t) kMaxChunks * bins * 2;
    if (flagged.empty() || histWords > (64u << 20)) return FSGPU_OK;              // <= 256 MB of counters; beyond that the queries keep their status
    const uint64_t foundSize = B.sp.foundDiagonalsSize ? (uint64_t) B.sp.foundDiagonalsSize : std::max<uint64_t>(ix.n, 1000000);
    std::vector<int32_t> slot(nq, -1);
    for (size_t k = 0; k < flagged.size(); k++) slot[flagged[k]] = (int32_t) k;
    KCHK(ensureAllK(ctx, S.kept0, nCand, S.qSlot, nq, S.truncHist, histWords, S.trunc, perChunk));
    HIPCHK(kCopy(S.kept0.p, S.kept.p, nCand, hipMemcpyDeviceToDevice, st));
    HIPCHK(kCopy(S.qSlot.p, slot.data(), nq, hipMemcpyHostToDevice, st));
    HIPCHK(kZero(S.truncHist.p, histWords, st));
    hipLaunchKernelGGL(k_kmer_trunc_hist, dim3(gridFor(nCand, 256)), dim3(256), 0, st, S.ckeys.p, S.cvals.p, S.kept.p, S.candTotal(), ix.tbits, bins, S.qSlot.p, S.truncHist.p);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> hh(histWords);
    HIPCHK(kCopy(hh.data(), S.truncHist.p, histWords, hipMemcpyDeviceToHost, st));
    KCHK(syncStream(ctx));
    std::vector<uint32_t> trunc(perChunk, 0xFFFFFFFFu), next(flagged.size(), 0);
    bool any = false;
    for (;;) {
        bool changed = false;
        for (size_t k = 0; k < flagged.size(); k++) {
            const int q = flagged[k];
            const uint32_t C = B.hck[q].nChunks - 1;
            const uint32_t *rounds = S.hRounds.p + (size_t) q * kMaxChunks;
            while (next[k] <= C) {
                const uint32_t c = next[k]++;
                const uint64_t before = c == 0 ? 0 : rounds[c];
                const uint32_t cut = truncationCut(hh.data() + ((k * kMaxChunks + c) * (size_t) bins) * 2, bins, foundSize > before ? foundSize - before : 0);
                if (cut != 0xFFFFFFFFu) { trunc[(size_t) q * kMaxChunks + c] = cut; changed = true; break; }     // the later rounds' element counts are stale now
            }
        }
        if (!changed) break;
        any = true;
        HIPCHK(kCopy(S.trunc.p, trunc.data(), trunc.size(), hipMemcpyHostToDevice, st));
        HIPCHK(kZero(S.rounds.p, perChunk, st));
        HIPCHK(kZero(S.resSize.p, nq, st));
        hipLaunchKernelGGL(k_kmer_apply_trunc, dim3(gridFor(nCand, 256)), dim3(256), 0, st, S.ckeys.p, S.cvals.p, S.kept0.p, S.candTotal(), ix.tbits, bins, S.trunc.p, S.kept.p);
        launchWalk<false>(B);
        HIPCHK(hipGetLastError());
        HIPCHK(kCopy(S.hRounds.p, S.rounds.p, perChunk, hipMemcpyDeviceToHost, st));
        HIPCHK(kCopy(S.hResSize.p, S.resSize.p, nq, hipMemcpyDeviceToHost, st));
        KCHK(syncStream(ctx));
    }
    if (any) {      // histogram, cut and hand-over once more, on the truncated lists
        HIPCHK(kZero(S.hist.p, (size_t) nq * 256, st));
        HIPCHK(kZero(S.outCount.p, nq, st));
        HIPCHK(kZero(S.outTotal(), 1, st));
        KCHK(kmerSelect(B));
        HIPCHK(kCopy(S.hThr.p, S.thr.p, nq, hipMemcpyDeviceToHost, st));
        HIPCHK(kCopy(S.hOutCount.p, S.outCount.p, nq, hipMemcpyDeviceToHost, st));
        KCHK(syncStream(ctx));
    }
    B.truncReplayed.assign(nq, 0);
    for (int q : flagged) B.truncReplayed[q] = 1;
    B.mark("truncation replay");
    return FSGPU_OK;
}

// ---- the selected elements come to the host, in S.hOut by query ---------------------------------------------------------
static int kmerHandOver(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; KmerScratch &S = B.S; const hipStream_t st = B.st; const int nq = B.nq;
    size_t totalOut = 0;
    B.outOff.assign(nq + 1, 0);
    for (int q = 0; q < nq; q++) { B.outOff[q] = totalOut; totalOut += S.hOutCount.p[q]; }
    B.outOff[nq] = B.totalOut = totalOut;
    if (totalOut > B.nCand) { ctx->err = "k-mer search: output count exceeds the candidate count"; return FSGPU_E_HIP; }
    KCHK(ensureK(ctx, S.hOut, std::max<size_t>(1, totalOut) * 2));
    if (totalOut) HIPCHK(kCopy(S.hOut.p + totalOut, S.out.p, totalOut, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(S.ev[9], st));
    KCHK(syncStream(ctx));
    // the device hands the elements over in no particular order: counting sort by query (query index in count >> 8)
    const HostOut *src = S.hOut.p + totalOut; HostOut *dst = S.hOut.p;
    std::vector<size_t> at(B.outOff.begin(), B.outOff.end() - 1);
    for (size_t i = 0; i < totalOut; i++) {
        const uint32_t q = src[i].count >> 8;
        if (q >= (uint32_t) nq || at[q] >= B.outOff[q + 1]) { ctx->err = "k-mer search: inconsistent output element"; return FSGPU_E_HIP; }
        dst[at[q]] = src[i];
        dst[at[q]++].count &= 0xffu;
    }
    return FSGPU_OK;
}

// ---- stage times and counts, summed over the device batches of one fsgpu_kmer_search call (the caller resets them) -----------------------
static void kmerTimes(KmerBatch &B) {
    fsgpu_ctx *ctx = B.ctx; const KmerScratch &S = B.S; float ms = 0;
    static const int a[9] = {0, 0, 1, 2, 3, 4, 5, 6, 7}, b[9] = {9, 1, 2, 3, 4, 5, 6, 7, 8};
    // [0] total, [1] count+scan, [2] lists+chunks, [3] emit, [4] sort, [5] dup flags+scan, [6] compact+score, [7] walk, [8] hist/cut/out
    for (int i = 0; i < 9; i++) if (hipEventElapsedTime(&ms, S.ev[a[i]], S.ev[b[i]]) == hipSuccess) ctx->kmerMs[i] = std::max(0.0, ctx->kmerMs[i]) + (double) ms;
    if (B.nLists && hipEventElapsedTime(&ms, S.ev[10], S.ev[11]) == hipSuccess) ctx->kmerMs[10] = std::max(0.0, ctx->kmerMs[10]) + (double) ms;
    (void) hipGetLastError();   // an elapsed-time query must never leave a sticky error behind
    ctx->kmerCounts[0] += B.nLists; ctx->kmerCounts[1] += B.nHits; ctx->kmerCounts[2] += B.nCand; ctx->kmerCounts[3] += B.totalOut;
    B.mark("copy out+sync");
}

// ---- host tail ---------------------------------------------------------------------------------------------
static void kmerHostTail(KmerBatch &B, fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats) {
    const KmerScratch &S = B.S; const fsgpu_kmer_search_params &sp = B.sp; const fsgpu_kmer_query *queries = B.queries;
    const uint64_t n = B.ix.n; const KmerChunks *hck = B.hck; const KmerQ *hq = S.hQs.p;
    const auto tTail = std::chrono::steady_clock::now();
    // one query per call of the host pool (search.cpp::HostPool; the caller takes part): the tails of a batch are independent -- 40 us each, 1.3 ms per batch
    // of 32 when a single feeder thread walks them
    fshostParallelFor(B.nq, [&](int q) {
        std::vector<HostOut> el(S.hOut.p + B.outOff[q], S.hOut.p + B.outOff[q + 1]);
        status[q] = finishQuery(sp, n, queries[q], hck[q], S.hEc.p + (size_t) q * kMaxChunks, S.hRounds.p + (size_t) q * kMaxChunks, S.hResSize.p[q], S.hThr.p[q], el,
                                out + (size_t) q * sp.maxResListLen, &nout[q], !B.truncReplayed.empty() && B.truncReplayed[q]);
        if (stats) {
            const uint64_t le = q + 1 < B.nq ? hq[q + 1].listBase : B.nLists;
            stats[q * 4 + 0] = queries[q].L > 0 ? (double) (le - hq[q].listBase) / (double) queries[q].L : 0.0;
            stats[q * 4 + 1] = (double) hck[q].total;
            if (hck[q].aborted == 1) {      // match() left its loop at that list (QueryMatcher.cpp:330-332): the statistics stop there too
                stats[q * 4 + 0] = (double) hck[q].abortKmers / (double) queries[q].L;
                stats[q * 4 + 1] = (double) hck[q].start[hck[q].nChunks - 1];
            }
            stats[q * 4 + 2] = hck[q].nChunks > 1 ? 1.0 : 0.0;
            stats[q * 4 + 3] = (double) pickBins(sp, n);
        }
    });
    B.ctx->kmerMs[9] = std::max(0.0, B.ctx->kmerMs[9]) + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tTail).count();
    B.mark("host tail");
}

static int kmerBatch(fsgpu_ctx *ctx, const fsgpu_kmer_search_params &sp, const fsgpu_kmer_query *queries, const fsgpu_kmer_profile_query *pq, int nq,
                     fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats) {
    if (!ctx->kmer) ctx->kmer = new KmerScratch();
    KmerScratch &S = *ctx->kmer;
    if (!S.evInit) { for (hipEvent_t &e : S.ev) HIPCHK(hipEventCreate(&e)); S.evInit = true; }
    static const bool trace = getenv("FSGPU_KMER_TRACE") != nullptr;
    KmerBatch B{ctx, S, *ctx->kidx, sp, queries, nq, ctx->stream, readSwitches()};
    B.trace = trace; B.tPrev = std::chrono::steady_clock::now(); B.pq = pq;
    const hipStream_t st = B.st;
    KCHK(kmerStageQueries(B));
    KCHK(kmerSimilar(B));
    if (B.nHits) {
        KCHK(kmerPartition(B));
        KCHK(kmerCandidates(B));
    } else {                                                 // keep every stage event recorded
        HIPCHK(hipEventRecord(S.ev[3], st));
        HIPCHK(hipEventRecord(S.ev[4], st));
    }
    HIPCHK(hipEventRecord(S.ev[5], st));
    if (B.nCand) {
        KCHK(kmerScore(B));
        KCHK(kmerSelect(B));
    } else {
        for (int e = 6; e <= 7; e++) HIPCHK(hipEventRecord(S.ev[e], st));
        HIPCHK(kZero(S.thr.p, nq, st));
    }
    KCHK(kmerCounters(B));
    if (B.nCand && !sp.kmerScoreOnly) KCHK(kmerTruncation(B));
    KCHK(kmerHandOver(B));
    kmerTimes(B);
    kmerHostTail(B, out, nout, status, stats);
    if (trace) fprintf(stderr, "kmer batch nq=%d hits=%llu cand=%u:%s\n", nq, (unsigned long long) B.nHits, B.nCand, B.traceLine.c_str());
    return FSGPU_OK;
}

// both forms of the search: pq == nullptr for sequence queries; for profile queries queries[] carries letters, ungapped profile and identity
static int kmerSearch(fsgpu_ctx *ctx, const fsgpu_kmer_search_params *p, const fsgpu_kmer_query *queries, const fsgpu_kmer_profile_query *pq, int nq,
                      fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats) {
    if (p->maxResListLen <= 0 || p->minDiagScoreThr < 0 || p->minDiagScoreThr > 255 * (p->kmerScoreOnly ? 1 : 1000)) {
        ctx->err = "k-mer search: maxResListLen >= 1 and minDiagScoreThr >= 0 required"; return FSGPU_E_UNSUPPORTED;
    }
    if (p->bins && (p->bins & (p->bins - 1))) { ctx->err = "k-mer search: bins must be a power of two"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    // queries per device batch: at most kmerMaxBatch; beyond that the batch is sized by its hit stream (24 bytes of scratch per index hit, fewer
    // than 2^32 hits): the hits per query of the previous batch of this context set the size of the next one, a batch that still comes out too
    // large is halved and redone
    const int maxBatch = kmerMaxBatch(ctx->kidx->tbits);
    for (int i = 0; i < 12; i++) ctx->kmerMs[i] = -1;          // < 0: nothing recorded (fsgpu_last_kernel_ms)
    for (int i = 0; i < 4; i++) ctx->kmerCounts[i] = 0;
    ctx->kmerBatches = 0; ctx->kmerLastBatchQueries = 0; ctx->kmerFirstBatchQueries = 0;
    int q0 = 0;
    while (q0 < nq) {
        int batch = std::min(maxBatch, 32);                   // no history on this context: a batch of 32 shows what a query costs here
        if (ctx->kmerHitsPerQuery > 0) batch = (int) std::max(1.0, std::min((double) maxBatch, kKmerHitBudget / ctx->kmerHitsPerQuery));   // queries of more than budget / 8 hits each: fewer than 8 per batch
        batch = std::min(batch, maxBatch);
        if (ctx->kmerBatchCap > 0) batch = std::min(batch, ctx->kmerBatchCap);
        // the rest of the call in device batches of equal size
        const int left = nq - q0, parts = (left + batch - 1) / batch;
        const int m = (left + parts - 1) / parts;
        const uint64_t hitsBefore = ctx->kmerCounts[1];
        int rc = kmerBatch(ctx, *p, queries + q0, pq ? pq + q0 : nullptr, m, out + (size_t) q0 * p->maxResListLen, nout + q0, status + q0, stats ? stats + (size_t) q0 * 4 : nullptr);
        if (rc == kKmerHalve) { ctx->kmerBatchCap = std::max(1, m / 2); ctx->kmerBatchOk = 0; continue; }            // too many hits / out of memory: redo with half the queries
        if (rc != FSGPU_OK) return rc;
        if (ctx->kmerBatches++ == 0) ctx->kmerFirstBatchQueries = (uint32_t) m;
        ctx->kmerLastBatchQueries = (uint32_t) m;
        // one heavy batch does not cap the context for good, but the cap is only relaxed after four batches in a row went through under it: doubling it
        // after every success made every second batch of a run of heavy queries fail, be abandoned after its first stage and be redone
        if (ctx->kmerBatchCap > 0 && ++ctx->kmerBatchOk >= 4) { ctx->kmerBatchCap = 2 * ctx->kmerBatchCap >= maxBatch ? 0 : 2 * ctx->kmerBatchCap; ctx->kmerBatchOk = 0; }
        ctx->kmerHitsPerQuery = (double) (ctx->kmerCounts[1] - hitsBefore) / (double) std::max(1, m);
        q0 += m;
    }
    return FSGPU_OK;
}


extern "C" int fsgpu_kmer_search(fsgpu_ctx *ctx, const fsgpu_kmer_search_params *p, const fsgpu_kmer_query *queries, int nq,
                                 fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats) {
    if (!ctx || !p || (nq > 0 && (!queries || !out || !nout || !status))) return FSGPU_E_ARG;
    if (!ctx->kidx) { ctx->err = "k-mer index not built"; return FSGPU_E_NODB; }
    return kmerSearch(ctx, p, queries, nullptr, nq, out, nout, status, stats);
}

// ---- profile queries -------------------------------------------------------------------------------------------------------------------
// Util::rankedDescSort20 (M/src/commons/Util.cpp:118-144): Batcher's merge-exchange network for 20 inputs, every comparator swapping only when
// the left value is SMALLER than the right one; the letter travels with its score.  Equal scores stay where the network leaves them, and that
// order reaches the results (it is the order of the similar k-mers), so the comparators are applied exactly in this sequence.
static const uint8_t kSort20[][2] = {
    {0, 16}, {1, 17}, {2, 18}, {3, 19}, {4, 12}, {5, 13}, {6, 14}, {7, 15},
    {0, 8}, {1, 9}, {2, 10}, {3, 11},
    {8, 16}, {9, 17}, {10, 18}, {11, 19}, {0, 4}, {1, 5}, {2, 6}, {3, 7},
    {8, 12}, {9, 13}, {10, 14}, {11, 15}, {4, 16}, {5, 17}, {6, 18}, {7, 19}, {0, 2}, {1, 3},
    {4, 8}, {5, 9}, {6, 10}, {7, 11}, {12, 16}, {13, 17}, {14, 18}, {15, 19}, {0, 1},
    {4, 6}, {5, 7}, {8, 10}, {9, 11}, {12, 14}, {13, 15}, {16, 18}, {17, 19},
    {2, 16}, {3, 17}, {6, 12}, {7, 13}, {18, 19},
    {2, 8}, {3, 9}, {10, 16}, {11, 17},
    {2, 4}, {3, 5}, {6, 8}, {7, 9}, {10, 12}, {11, 13}, {14, 16}, {15, 17},
    {2, 3}, {4, 5}, {6, 7}, {8, 9}, {10, 11}, {12, 13}, {14, 15}, {16, 17},
    {1, 16}, {3, 18}, {5, 12}, {7, 14},
    {1, 8}, {3, 10}, {9, 16}, {11, 18},
    {1, 4}, {3, 6}, {5, 8}, {7, 10}, {9, 12}, {11, 14}, {13, 16}, {15, 18},
    {1, 2}, {3, 4}, {5, 6}, {7, 8}, {9, 10}, {11, 12}, {13, 14}, {15, 16}, {17, 18}};

extern "C" int fsgpu_kmer_profile_sort_rows(const int8_t *scores, int L, uint16_t *rows) {
    if (L < 0 || (L > 0 && (!scores || !rows))) return FSGPU_E_ARG;
    for (int i = 0; i < L; i++) {
        int v[20], a[20];
        for (int j = 0; j < 20; j++) { v[j] = scores[(size_t) i * 20 + j]; a[j] = j; }
        for (const uint8_t (&c)[2] : kSort20)
            if (v[c[0]] < v[c[1]]) { std::swap(v[c[0]], v[c[1]]); std::swap(a[c[0]], a[c[1]]); }
        for (int j = 0; j < 20; j++) rows[(size_t) i * 20 + j] = (uint16_t) ((v[j] << 8) | a[j]);
    }
    return FSGPU_OK;
}

extern "C" int fsgpu_kmer_search_profile(fsgpu_ctx *ctx, const fsgpu_kmer_search_params *p, const fsgpu_kmer_profile_query *queries, int nq,
                                         fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats) {
    if (!ctx || !p || (nq > 0 && (!queries || !out || !nout || !status))) return FSGPU_E_ARG;
    if (!ctx->kidx) { ctx->err = "k-mer index not built"; return FSGPU_E_NODB; }
    if (ctx->kidx->p.kmerThr != 0) {
        ctx->err = "k-mer search: a profile query needs an index built with kmerThr = 0 (Prefiltering.cpp:555: localKmerThr is 0 for profile queries, no target k-mer is dropped); "
                   "the resident index was built with kmerThr = " + std::to_string(ctx->kidx->p.kmerThr);
        return FSGPU_E_ARG;
    }
    std::vector<fsgpu_kmer_query> qs((size_t) std::max(nq, 0));
    for (int q = 0; q < nq; q++) { qs[q] = fsgpu_kmer_query{}; qs[q].seq = queries[q].seq; qs[q].profile = queries[q].profile; qs[q].L = queries[q].L; qs[q].identity = queries[q].identity; }
    return kmerSearch(ctx, p, qs.data(), queries, nq, out, nout, status, stats);
}

// the similar k-mers of one position of one query of the last device batch, when that was a profile batch: the list pass itself (same tables, same
// unranking, same slices) writes the k-mers of that position instead of probing the index
extern "C" int fsgpu_kmer_profile_list_copy(fsgpu_ctx *ctx, int query, int pos, uint32_t *kmers, uint32_t cap, uint32_t *count) {
    if (!ctx || !count || (cap > 0 && !kmers)) return FSGPU_E_ARG;
    if (!ctx->kidx) { ctx->err = "k-mer index not built"; return FSGPU_E_NODB; }
    KmerScratch *S = ctx->kmer;
    if (!S || S->profNq == 0) { ctx->err = "k-mer profile list: the last k-mer batch of this context was not a profile batch"; return FSGPU_E_ARG; }
    if (query < 0 || query >= S->profNq || pos < 0 || (uint32_t) pos >= S->hQs.p[query].nPos) {
        ctx->err = "k-mer profile list: query " + std::to_string(query) + " position " + std::to_string(pos) + " is not a k-mer start of the last profile batch";
        return FSGPU_E_ARG;
    }
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = ctx->stream;
    const uint32_t p = S->hQs.p[query].posBase + (uint32_t) pos;
    uint32_t Kp = 0;
    HIPCHK(hipMemcpyAsync(&Kp, S->K.p + p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *count = Kp;
    const uint32_t n = std::min(Kp, cap);
    if (n == 0) return FSGPU_OK;
    if (Kp > kMaxKmerResult - 1) { ctx->err = "k-mer profile list: inconsistent count"; return FSGPU_E_HIP; }
    KDev<uint32_t> dk;
    HIPCHK(kNew(dk, Kp));
    const KmerIndex &ix = *ctx->kidx;
    hipLaunchKernelGGL(k_kmer_lists_p<true>, dim3((unsigned) (S->profNPos + S->profNLists / kListSlice + 1)), dim3(kKmerBlock), 0, st, S->qs.p, S->posQuery.p, S->seqs.p, S->thrs.p,
                       S->rows.p, S->rowBase.p, (uint32_t) S->profNPos, ix.pat, S->K.p, S->Kbase.p, ix.offsets, ix.bitmap, (uint32_t *) nullptr, (uint32_t *) nullptr,
                       (uint32_t *) nullptr, p, dk.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(kmers, dk.p, (size_t) n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return FSGPU_OK;
}

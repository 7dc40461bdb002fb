// fsgpu_sw.hip -- the profile-based Smith-Waterman path (k_sw / k_sw2): LDS images built on the host from word profiles.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_sw.hpp"

// ------------------------------------------------------------------------------------------------------------
// Smith-Waterman batch
// ------------------------------------------------------------------------------------------------------------
static int swPickR(int rows) {
    const int opts[] = {1, 2, 3, 4, 6, 8};   // 5 and 7 were measured: more launch groups + odd LDS chunking cost more than the padding they save
    for (int r : opts) if (64 * r >= rows) return r;
    return 8;
}

// The shape of a query of L rows: one tile of R = 1, 2, 3, 4, 6 or 8 register rows per lane (the smallest with 64 R >= L) up to 64 * kSwMaxR rows,
// beyond that ceil(L / 512) row tiles of R = kSwMaxR.  Pure host function, exported as fsgpu_sw_shape for the CPU tests.
static void swShape(int L, int *nTiles, int *R) {
    *nTiles = L <= 64 * kSwMaxR ? 1 : (L + 64 * kSwMaxR - 1) / (64 * kSwMaxR);
    *R = *nTiles == 1 ? swPickR(L) : kSwMaxR;
}

extern "C" int fsgpu_sw_shape(int L, int *nTiles, int *R) {
    if (L < 1 || L > FSGPU_MAX_SEQ_LEN || !nTiles || !R) return -1;
    swShape(L, nTiles, R);
    return 0;
}

// slot of fsgpu_sw_kernel_counts: kind 0 k_sw Pk16, 1 k_sw I32, 2 k_sw2
static constexpr int swCountSlot(int kind, bool hasAA, int R) {
    return (kind * 2 + (hasAA ? 1 : 0)) * 6 + (R <= 4 ? R - 1 : R == 6 ? 4 : 5);
}

template <int R, bool HAS_AA, typename A>
static int launchSwT(fsgpu_ctx *ctx, const SwArgs &sa, int blocks, int threads, hipStream_t stream) {
    const int lds = (HAS_AA ? 2 : 1) * kAlphabet * swRowDwords(R) * 4;
    static thread_local uint64_t attrDevs = 0;       // devices on which this thread has set the attribute (it is per device)
    const uint64_t devBit = 1ull << (ctx->device & 63);
    if (!(attrDevs & devBit)) {
        HIPCHK(hipFuncSetAttribute((const void *) k_sw<R, HAS_AA, A>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attrDevs |= devBit;
    }
    hipLaunchKernelGGL((k_sw<R, HAS_AA, A>), dim3(blocks), dim3(threads), lds, stream, sa);
    HIPCHK(hipGetLastError());
    ctx->swKernelCount[swCountSlot(A::packed ? 0 : 1, HAS_AA, R)]++;
    return FSGPU_OK;
}

template <typename A>
static int launchSw(fsgpu_ctx *ctx, int R, bool hasAA, const SwArgs &sa, int nPairs) {
    // small batches (one query) -> 4 waves per workgroup so that all CUs get work; big batches -> 8
    const int waves = nPairs <= 4096 ? 4 : 8;
    const int blocks = (nPairs + waves - 1) / waves;
#define FS_SW_CASE(RR)                                                                   \
    case RR: return hasAA ? launchSwT<RR, true, A>(ctx, sa, blocks, waves * 64, ctx->stream) : launchSwT<RR, false, A>(ctx, sa, blocks, waves * 64, ctx->stream);
    switch (R) {
        FS_SW_CASE(1) FS_SW_CASE(2) FS_SW_CASE(3) FS_SW_CASE(4) FS_SW_CASE(6) FS_SW_CASE(8)
        default: ctx->err = "internal: bad SW R"; return FSGPU_E_ARG;
    }
#undef FS_SW_CASE
}

// k_sw2: two targets per wave, one direction (image with the extra "past the end" row)
template <int R, bool HAS_AA>
static int launchSwBlocks2T(fsgpu_ctx *ctx, const SwArgs &sa, int nBlocks, int pairsPerBlock, hipStream_t stream) {
    const int lds = (HAS_AA ? 2 : 1) * kSw2Rows * swRowDwords(R) * 4;
    static thread_local uint64_t attrDevs = 0;       // devices on which this thread has set the attribute (it is per device)
    const uint64_t devBit = 1ull << (ctx->device & 63);
    if (!(attrDevs & devBit)) {
        HIPCHK(hipFuncSetAttribute((const void *) k_sw2<R, HAS_AA>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attrDevs |= devBit;
    }
    hipLaunchKernelGGL((k_sw2<R, HAS_AA>), dim3(nBlocks), dim3(32 * pairsPerBlock), lds, stream, sa);
    HIPCHK(hipGetLastError());
    ctx->swKernelCount[swCountSlot(2, HAS_AA, R)]++;
    return FSGPU_OK;
}
// Pairs of one query that share a workgroup (and one copy of the query's LDS image): two per wave.  8 pairs = 4 waves per image gives
// 4 waves per SIMD (3Di, 33 KB image at R = 6) / 2 per SIMD (3Di + AA).  More waves per image (16 / 32 pairs: 8 waves per SIMD) is SLOWER:
// the kernel is VALU-issue bound already at 4 waves per SIMD and a workgroup lasts as long as its longest pair (32 queries x 1000 targets,
// forward pass, alone on the device: 1.69 / 1.87 / 2.08 ms at 8 / 16 / 32 pairs for 3Di, 2.44 / 2.60 / 2.71 ms for 3Di + AA;
// tools/sw2_probe.py).  FSGPU_SW2_PAIRS = 8 | 16 | 32 overrides it for such measurements.
static int sw2PairsPerBlock() {
    static const int env = [] { const char *e = getenv("FSGPU_SW2_PAIRS"); const int v = e ? atoi(e) : 0; return (v == 8 || v == 16 || v == 32) ? v : 0; }();
    return env ? env : 8;
}
static int launchSwBlocks2(fsgpu_ctx *ctx, int R, bool hasAA, const SwArgs &sa, int nBlocks, int pairsPerBlock, hipStream_t stream) {
#define FS_SW_CASE(RR) case RR: return hasAA ? launchSwBlocks2T<RR, true>(ctx, sa, nBlocks, pairsPerBlock, stream) : launchSwBlocks2T<RR, false>(ctx, sa, nBlocks, pairsPerBlock, stream);
    switch (R) {
        FS_SW_CASE(1) FS_SW_CASE(2) FS_SW_CASE(3) FS_SW_CASE(4) FS_SW_CASE(6) FS_SW_CASE(8)
        default: ctx->err = "internal: bad SW R"; return FSGPU_E_ARG;
    }
#undef FS_SW_CASE
}

// One table of an LDS image (fs_kernels.h): query rows [base, base + 64 R) of a profile, value = packed ? (fwd int16) | (rev int16) << 16 : the int32
// of fwd (rev is not read); rows from L on are 0.
static void swFillTable(uint32_t *dst, int R, int L, int base, bool packed, const int16_t *f, const int16_t *r) {
    const int rowDw = swRowDwords(R);
    for (int a = 0; a < kAlphabet; a++)
        for (int lane = 0; lane < 64; lane++)
            for (int rr = 0; rr < R; rr++) {
                const int row = base + lane * R + rr;
                uint32_t v = 0;
                if (row < L) v = packed ? (uint32_t) (uint16_t) f[(size_t) a * L + row] | ((uint32_t) (uint16_t) r[(size_t) a * L + row] << 16) : (uint32_t) (int32_t) f[(size_t) a * L + row];
                dst[(size_t) a * rowDw + swDwordIndex(R, lane, rr)] = v;
            }
}

// Builds the per-tile LDS images (host) and runs all row tiles of one pass.
//   packed:  value = (fwd int16) | (rev int16) << 16;   int32: value = the selected direction's score
static int runSwPass(fsgpu_ctx *ctx, bool packed, const int16_t *pAA0, const int16_t *p3_0, const int16_t *pAA1, const int16_t *p3_1,
                     int L, const uint32_t *dTids, int nPairs, int maxLt, int go, int ge, int32_t *dRes0, int32_t *dRes1) {
    const bool hasAA = pAA0 != nullptr;
    int nTiles, R;
    swShape(L, &nTiles, &R);
    const int rowDw = swRowDwords(R);
    const size_t tblDw = (size_t) kAlphabet * rowDw;
    const size_t imgDw = tblDw * (hasAA ? 2 : 1);
    int rc;
    if ((rc = ensurePinned(ctx, ctx->hImg, imgDw * nTiles * 4)) != FSGPU_OK) return rc;
    uint32_t *img = (uint32_t *) ctx->hImg.p;
    memset(img, 0, imgDw * nTiles * 4);
    for (int t = 0; t < nTiles; t++) {
        swFillTable(img + imgDw * t, R, L, t * 64 * R, packed, p3_0, p3_1);
        if (hasAA) swFillTable(img + imgDw * t + tblDw, R, L, t * 64 * R, packed, pAA0, pAA1);
    }
    if ((rc = ensure(ctx, ctx->img, imgDw * nTiles * 4)) != FSGPU_OK) return rc;
    HIPCHK(hipMemcpyAsync(ctx->img.p, img, imgDw * nTiles * 4, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t stride = (uint32_t) ((maxLt + 63) / 64 * 64);
    if (nTiles > 1) {
        const size_t bbytes = (size_t) nPairs * stride * 3 * 4;
        if ((rc = ensureAll(ctx, {{ctx->border0, bbytes}, {ctx->border1, bbytes}, {ctx->keys, (size_t) nPairs * 2 * 8}})) != FSGPU_OK) return rc;
    }
    for (int t = 0; t < nTiles; t++) {
        SwArgs sa;
        if (ctx->sw.explicitTargets) {
            sa.aa = (const uint8_t *) ctx->ovAA.p; sa.ss = (const uint8_t *) ctx->ovSS.p; sa.offsets = (const uint64_t *) ctx->ovOff.p; sa.lengths = (const int32_t *) ctx->ovLen.p;
        } else {
            sa.aa = ctx->db->alnAA; sa.ss = ctx->db->aln3di; sa.offsets = ctx->db->dOffsets; sa.lengths = ctx->db->dLengths;
        }
        sa.targetIds = dTids; sa.nPairs = nPairs;
        sa.profSS = (const uint32_t *) ctx->img.p + imgDw * t;
        sa.profAA = hasAA ? sa.profSS + tblDw : nullptr;
        sa.tileBase = t * 64 * R;
        sa.rowsInTile = std::min(64 * R, L - sa.tileBase);
        sa.segLen = packed ? (L + 15) / 16 : (L + 7) / 8;
        sa.go = packed ? ((uint32_t) go | ((uint32_t) go << 16)) : (uint32_t) go;
        sa.ge = packed ? ((uint32_t) ge | ((uint32_t) ge << 16)) : (uint32_t) ge;
        sa.tileIn = t > 0; sa.tileOut = t + 1 < nTiles;
        sa.borderIn = (const uint32_t *) ((t & 1) ? ctx->border1.p : ctx->border0.p);
        sa.borderOut = (uint32_t *) ((t & 1) ? ctx->border0.p : ctx->border1.p);
        sa.borderStride = stride;
        sa.keys = (uint64_t *) ctx->keys.p;
        sa.res0 = dRes0; sa.res1 = dRes1;
        sa.blocks = nullptr;
        rc = packed ? launchSw<Pk16>(ctx, R, hasAA, sa, nPairs) : launchSw<I32>(ctx, R, hasAA, sa, nPairs);
        if (rc != FSGPU_OK) return rc;
    }
    return FSGPU_OK;
}

// ---- multi-query row-tiled SW: the queries of a fsgpu_sw_multi_dir call that are longer than 64 * kSwMaxR rows ----
// One k_sw launch per tile LEVEL serves the tiles of that level of ALL such queries (workgroup = up to 8 pairs of one query,
// SwTileBlock); levels follow each other on a side stream (ctx->swLong) next to the single-tile launches of the same call.
// k_sw carries the forward and the reversed query in the int16 halves, so the forward call already has the reversed-query
// results: they are kept per query (with a hash of what they depend on) and handed out by the following reversed call.
struct SwLongPlan {
    std::vector<uint32_t> slotQ, slotJ;         // launch slot -> query, index into its targetIds
    size_t n = 0;
};

// everything the reversed records of one query depend on, the database apart: that one is covered by freeDb, which drops the records
static uint64_t swLongHash(const fsgpu_sw_query &q, int gapOpen, int gapExtend) {
    uint64_t h = 0xcbf29ce484222325ull ^ (uint64_t) q.L ^ ((uint64_t) q.n << 32);
    const uint32_t gaps[2] = {(uint32_t) gapOpen, (uint32_t) gapExtend};
    h = hashWords(h, gaps, sizeof(gaps));
    h = hashWords(h, q.targetIds, (size_t) q.n * 4);
    h = hashWords(h, q.p3Di_rev, (size_t) q.L * kAlphabet * 2);
    if (q.pAA_rev) h = hashWords(h, q.pAA_rev, (size_t) q.L * kAlphabet * 2);
    return h ? h : 1;
}

// isLong[i]: query i is row-tiled and has selected pairs.  Pairs answered from the forward call's results go straight to out[].
static int swLongEnqueue(fsgpu_ctx *ctx, const fsgpu_sw_query *q, int nq, const std::vector<char> &isLong, const int32_t *const *sel, const int32_t *nsel,
                         const std::vector<size_t> &base, bool hasAA, int gapOpen, int gapExtend, int dir, fsgpu_swres *out, SwLongPlan &plan) {
    plan.n = 0; plan.slotQ.clear(); plan.slotJ.clear();
    if (dir == 0) ctx->swLongRev.assign((size_t) nq, fsgpu_ctx::LongRev());
    const std::vector<int32_t> &len = ctx->db->hLengths;
    std::vector<size_t> qFirst(nq + 1, 0);                 // slots of query i: [qFirst[i], qFirst[i + 1])
    std::vector<uint64_t> lkey;
    for (int i = 0; i < nq; i++) {
        qFirst[i] = plan.n;
        if (!isLong[i]) continue;
        const int ns = sel ? nsel[i] : q[i].n;
        const fsgpu_ctx::LongRev *have = nullptr;
        if (dir == 1 && (size_t) i < ctx->swLongRev.size() && ctx->swLongRev[i].hash != 0 && ctx->swLongRev[i].res.size() == (size_t) q[i].n * 4 &&
            ctx->swLongRev[i].hash == swLongHash(q[i], gapOpen, gapExtend))
            have = &ctx->swLongRev[i];
        lkey.clear();
        for (int k = 0; k < ns; k++) {
            const int j = sel ? sel[i][k] : k;
            if (have && have->res[(size_t) j * 4 + 3] != 0) { memcpy(&out[base[i] + j], &have->res[(size_t) j * 4], 16); ctx->swLongReused++; continue; }
            lkey.push_back(((uint64_t) (0xFFFFFF - len[q[i].targetIds[j]]) << 32) | (uint32_t) j);
        }
        std::sort(lkey.begin(), lkey.end());               // longest target first: the waves of a workgroup are of similar length
        for (uint64_t k : lkey) { plan.slotQ.push_back((uint32_t) i); plan.slotJ.push_back((uint32_t) k); }
        plan.n += lkey.size();
        if (dir == 0) { ctx->swLongRev[i].hash = swLongHash(q[i], gapOpen, gapExtend); ctx->swLongRev[i].res.assign((size_t) q[i].n * 4, 0); }
    }
    qFirst[nq] = plan.n;
    ctx->swLongLaunched = (uint32_t) plan.n;
    if (plan.n == 0) return FSGPU_OK;
    const size_t n = plan.n;
    const int R = kSwMaxR, rowsPerTile = 64 * R, rowDw = swRowDwords(R);       // what swShape gives every query of more than one tile
    const size_t tblDw = (size_t) kAlphabet * rowDw, imgDw = tblDw * (hasAA ? 2 : 1);
    // geometry: tiles per query, image offsets, blocks per level
    int maxTiles = 0;
    std::vector<int> nTiles(nq, 0);
    std::vector<size_t> imgFirst(nq, 0);                   // dword offset of tile 0 of query i inside the image section
    size_t imgTotalDw = 0;
    for (int i = 0; i < nq; i++) {
        if (qFirst[i + 1] == qFirst[i]) continue;
        int tileR;
        swShape(q[i].L, &nTiles[i], &tileR);
        if (tileR != R || nTiles[i] < 2) { ctx->err = "internal: a single-tile query among the row-tiled ones"; return FSGPU_E_ARG; }
        maxTiles = std::max(maxTiles, nTiles[i]);
        imgFirst[i] = imgTotalDw;
        imgTotalDw += imgDw * (size_t) nTiles[i];
    }
    if (imgTotalDw >= (1ull << 32)) { ctx->err = "fsgpu_sw_multi_dir: tile images of one call exceed 16 GiB"; return FSGPU_E_NOMEM; }
    std::vector<size_t> levelFirst(maxTiles + 1, 0);
    for (int t = 0; t < maxTiles; t++) {
        size_t nb = 0;
        for (int i = 0; i < nq; i++) if (nTiles[i] > t) nb += (qFirst[i + 1] - qFirst[i] + 7) / 8;
        levelFirst[t + 1] = levelFirst[t] + nb;
    }
    auto align16 = [](size_t x) { return (x + 15) / 16 * 16; };
    const size_t offTids = 0, offBase = align16(n * 4), offBlocks = align16(offBase + n * 4), offImg = align16(offBlocks + levelFirst[maxTiles] * sizeof(SwTileBlock));
    const size_t bytes = offImg + imgTotalDw * 4;
    int rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hLbuf, bytes}, {ctx->hLres, n * 32}})) != FSGPU_OK) return rc;
    if ((rc = ensureAll(ctx, {{ctx->lbuf, bytes}, {ctx->lres, n * 32}})) != FSGPU_OK) return rc;
    unsigned char *h = (unsigned char *) ctx->hLbuf.p;
    uint32_t *hT = (uint32_t *) (h + offTids), *hB = (uint32_t *) (h + offBase);
    SwTileBlock *hBlk = (SwTileBlock *) (h + offBlocks);
    uint32_t *hImg = (uint32_t *) (h + offImg);
    uint64_t cols = 0;
    for (size_t s2 = 0; s2 < n; s2++) {
        const uint32_t tid = q[plan.slotQ[s2]].targetIds[plan.slotJ[s2]];
        hT[s2] = tid;
        if (cols >= (1ull << 32)) { ctx->err = "fsgpu_sw_multi_dir: tile borders of one call exceed 2^32 columns"; return FSGPU_E_NOMEM; }
        hB[s2] = (uint32_t) cols;
        cols += (uint64_t) ((len[tid] + 63) / 64 * 64);
    }
    for (int t = 0; t < maxTiles; t++) {
        SwTileBlock *b = hBlk + levelFirst[t];
        size_t nb = 0;
        for (int i = 0; i < nq; i++) {
            if (nTiles[i] <= t) continue;
            const int L = q[i].L;
            for (size_t p0 = qFirst[i]; p0 < qFirst[i + 1]; p0 += 8) {
                SwTileBlock &d = b[nb++];
                d.imgOff = (uint32_t) (imgFirst[i] + imgDw * (size_t) t); d.firstPair = (uint32_t) p0; d.nPairs = (uint16_t) std::min<size_t>(8, qFirst[i + 1] - p0);
                d.rowsInTile = (uint16_t) std::min(rowsPerTile, L - t * rowsPerTile); d.segLen = (uint32_t) ((L + 15) / 16);
                d.tileBase = (uint32_t) (t * rowsPerTile); d.flags = (t > 0 ? 1u : 0u) | (t + 1 < nTiles[i] ? 2u : 0u);
            }
        }
        std::stable_sort(b, b + nb, [&](const SwTileBlock &x, const SwTileBlock &y) { return len[hT[x.firstPair]] > len[hT[y.firstPair]]; });
    }
    for (int i = 0; i < nq; i++) {
        if (nTiles[i] == 0) continue;
        const int L = q[i].L;
        for (int t = 0; t < nTiles[i]; t++) {
            uint32_t *dst = hImg + imgFirst[i] + imgDw * (size_t) t;
            swFillTable(dst, R, L, t * rowsPerTile, true, q[i].p3Di_fwd, q[i].p3Di_rev);
            if (hasAA) swFillTable(dst + tblDw, R, L, t * rowsPerTile, true, q[i].pAA_fwd, q[i].pAA_rev);
        }
    }
    if (maxTiles > 1 && (rc = ensureAll(ctx, {{ctx->border0, cols * 12}, {ctx->border1, cols * 12}, {ctx->keys, n * 2 * 8}})) != FSGPU_OK) return rc;
    if (!ctx->swLong) HIPCHK(hipStreamCreateWithFlags(&ctx->swLong, hipStreamNonBlocking));
    HIPCHK(hipMemcpyAsync(ctx->lbuf.p, h, bytes, hipMemcpyHostToDevice, ctx->swLong));
    const unsigned char *d = (const unsigned char *) ctx->lbuf.p;
    for (int t = 0; t < maxTiles; t++) {
        SwArgs sa;
        sa.aa = ctx->db->alnAA; sa.ss = ctx->db->aln3di; sa.offsets = ctx->db->dOffsets; sa.lengths = ctx->db->dLengths;
        sa.targetIds = (const uint32_t *) (d + offTids); sa.nPairs = (int) n;
        sa.profSS = (const uint32_t *) (d + offImg); sa.profAA = nullptr;
        sa.tileBase = 0; sa.rowsInTile = 0; sa.segLen = 1;
        sa.go = (uint32_t) gapOpen | ((uint32_t) gapOpen << 16);
        sa.ge = (uint32_t) gapExtend | ((uint32_t) gapExtend << 16);
        sa.tileIn = 0; sa.tileOut = 0;
        sa.borderIn = (const uint32_t *) ((t & 1) ? ctx->border1.p : ctx->border0.p);
        sa.borderOut = (uint32_t *) ((t & 1) ? ctx->border0.p : ctx->border1.p);
        sa.borderStride = 0;
        sa.keys = (uint64_t *) ctx->keys.p;
        sa.res0 = (int32_t *) ctx->lres.p; sa.res1 = (int32_t *) ctx->lres.p + n * 4;
        sa.blocks = nullptr; sa.dir = 0;
        sa.tblocks = (const SwTileBlock *) (d + offBlocks) + levelFirst[t];
        sa.borderBase = (const uint32_t *) (d + offBase);
        const int nb = (int) (levelFirst[t + 1] - levelFirst[t]);
        rc = hasAA ? launchSwT<kSwMaxR, true, Pk16>(ctx, sa, nb, 512, ctx->swLong) : launchSwT<kSwMaxR, false, Pk16>(ctx, sa, nb, 512, ctx->swLong);
        if (rc != FSGPU_OK) return rc;
    }
    HIPCHK(hipMemcpyAsync(ctx->hLres.p, ctx->lres.p, n * 32, hipMemcpyDeviceToHost, ctx->swLong));
    return FSGPU_OK;
}

static int swLongCollect(fsgpu_ctx *ctx, const SwLongPlan &plan, const std::vector<size_t> &base, int dir, fsgpu_swres *out) {
    if (plan.n == 0) return FSGPU_OK;
    int rc = syncStreamOf(ctx, ctx->swLong);
    if (rc != FSGPU_OK) return rc;
    const int32_t *fwd = (const int32_t *) ctx->hLres.p, *rev = fwd + plan.n * 4;
    for (size_t s2 = 0; s2 < plan.n; s2++) {
        const uint32_t i = plan.slotQ[s2], j = plan.slotJ[s2];
        memcpy(&out[base[i] + j], (dir == 0 ? fwd : rev) + s2 * 4, 16);
        if (dir == 0) memcpy(&ctx->swLongRev[i].res[(size_t) j * 4], rev + s2 * 4, 16);
    }
    return FSGPU_OK;
}

extern "C" {

static int swLaunchImpl(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd, const int16_t *pAA_rev,
                        const int16_t *p3Di_rev, int L, const uint32_t *targetIds, int n, int gapOpen, int gapExtend, bool explicitTargets) {
    if (!ctx) return FSGPU_E_ARG;
    if (!p3Di_fwd || !p3Di_rev || L <= 0 || L > FSGPU_MAX_SEQ_LEN || n < 0 || (n > 0 && !targetIds) || ((pAA_fwd == nullptr) != (pAA_rev == nullptr))) {
        ctx->err = "fsgpu_sw_launch: bad argument"; return FSGPU_E_ARG;
    }
    if (!ctx->db || ctx->db->n == 0) { ctx->err = "no database loaded"; return FSGPU_E_NODB; }
    if (pAA_fwd && !explicitTargets && !ctx->db->hasAA) { ctx->err = "AA profiles given but the database was loaded without AA sequences"; return FSGPU_E_NODB; }
    if (!(gapOpen > gapExtend && gapExtend >= 0 && gapOpen < 32768)) {
        ctx->err = "device SW requires gapOpen > gapExtend >= 0 (the striped reference kernel's lazy-F shortcut is only reproduced for that case)";
        return FSGPU_E_UNSUPPORTED;
    }
    if (ctx->sw.pending) { ctx->err = "previous SW batch not finished"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->sw.explicitTargets = explicitTargets;
    const std::vector<int32_t> &hLen = explicitTargets ? ctx->sw.ovLengths : ctx->db->hLengths;
    const uint64_t nTargets = explicitTargets ? ctx->sw.ovLengths.size() : ctx->db->n;
    ctx->sw.n = n; ctx->sw.L = L; ctx->sw.go = gapOpen; ctx->sw.ge = gapExtend; ctx->sw.hasAA = pAA_fwd != nullptr;
    ctx->sw.pAAf = pAA_fwd; ctx->sw.p3f = p3Di_fwd; ctx->sw.pAAr = pAA_rev; ctx->sw.p3r = p3Di_rev;
    ctx->sw.tids.assign(targetIds, targetIds + n);
    if (n == 0) { ctx->sw.pending = true; return FSGPU_OK; }
    int maxLt = 1;
    for (int i = 0; i < n; i++) {
        if (targetIds[i] >= nTargets) { ctx->err = "target id out of range"; return FSGPU_E_ARG; }
        maxLt = std::max(maxLt, hLen[targetIds[i]]);
    }
    int rc;
    if ((rc = ensureAll(ctx, {{ctx->tids, (size_t) n * 4}, {ctx->res0, (size_t) n * 16}, {ctx->res1, (size_t) n * 16}})) != FSGPU_OK) return rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hRes0, (size_t) n * 16}, {ctx->hRes1, (size_t) n * 16}, {ctx->hTids, (size_t) n * 4}})) != FSGPU_OK) return rc;
    memcpy(ctx->hTids.p, ctx->sw.tids.data(), (size_t) n * 4);
    HIPCHK(hipMemcpyAsync(ctx->tids.p, ctx->hTids.p, (size_t) n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    rc = runSwPass(ctx, true, pAA_fwd, p3Di_fwd, pAA_rev, p3Di_rev, L, (const uint32_t *) ctx->tids.p, n, maxLt, gapOpen, gapExtend,
                   (int32_t *) ctx->res0.p, (int32_t *) ctx->res1.p);
    if (rc != FSGPU_OK) return rc;
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    ctx->evValid[1] = true;
    HIPCHK(hipMemcpyAsync(ctx->hRes0.p, ctx->res0.p, (size_t) n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->hRes1.p, ctx->res1.p, (size_t) n * 16, hipMemcpyDeviceToHost, ctx->stream));
    ctx->sw.pending = true;          // only now: an error above leaves the context free for the next launch
    return FSGPU_OK;
}

int fsgpu_sw_launch(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd, const int16_t *pAA_rev,
                    const int16_t *p3Di_rev, int L, const uint32_t *targetIds, int n, int gapOpen, int gapExtend) {
    return swLaunchImpl(ctx, pAA_fwd, p3Di_fwd, pAA_rev, p3Di_rev, L, targetIds, n, gapOpen, gapExtend, false);
}

// Explicit target sequences (structurealign --alt-ali re-aligns a target whose previous alignment range was overwritten with X,
// F/src/strucclustutils/structurealign.cpp:115-138): the sequences are staged in per-context device buffers and the same
// kernels run on them with ids 0..n-1.
int fsgpu_sw_batch_seqs(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd, const int16_t *pAA_rev, const int16_t *p3Di_rev,
                        int L, const uint8_t *tAA, const uint8_t *t3Di, const uint64_t *offsets, const int32_t *lengths, int n,
                        int gapOpen, int gapExtend, fsgpu_swres *fwd, fsgpu_swres *rev) {
    if (!ctx || !t3Di || !offsets || !lengths || n < 0 || !fwd || !rev || (pAA_fwd && !tAA)) { if (ctx) ctx->err = "fsgpu_sw_batch_seqs: bad argument"; return FSGPU_E_ARG; }
    if (ctx->sw.pending) { ctx->err = "previous SW batch not finished"; return FSGPU_E_ARG; }
    if (n == 0) return FSGPU_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t bytes = offsets[n];
    int rc;
    if ((rc = ensure(ctx, ctx->ovSS, bytes + 16)) != FSGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->ovAA, bytes + 16)) != FSGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->ovOff, (size_t) (n + 1) * 8)) != FSGPU_OK) return rc;
    if ((rc = ensure(ctx, ctx->ovLen, (size_t) n * 4)) != FSGPU_OK) return rc;
    ctx->sw.ovLengths.assign(lengths, lengths + n);
    for (int i = 0; i < n; i++)
        if (lengths[i] <= 0 || lengths[i] > FSGPU_MAX_SEQ_LEN || offsets[i] + (uint64_t) lengths[i] > bytes) { ctx->err = "fsgpu_sw_batch_seqs: bad target layout"; return FSGPU_E_ARG; }
    // pageable sources: synchronous copies (this path serves a handful of pairs per query)
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(ctx->ovSS.p, t3Di, bytes, hipMemcpyHostToDevice));
    if (tAA) HIPCHK(hipMemcpy(ctx->ovAA.p, tAA, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->ovOff.p, offsets, (size_t) (n + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->ovLen.p, lengths, (size_t) n * 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> ids(n);
    for (int i = 0; i < n; i++) ids[i] = (uint32_t) i;
    rc = swLaunchImpl(ctx, pAA_fwd, p3Di_fwd, pAA_rev, p3Di_rev, L, ids.data(), n, gapOpen, gapExtend, true);
    if (rc != FSGPU_OK) { ctx->sw.explicitTargets = false; return rc; }
    rc = fsgpu_sw_finish(ctx, fwd, rev);
    ctx->sw.explicitTargets = false;
    return rc;
}

int fsgpu_sw_finish(fsgpu_ctx *ctx, fsgpu_swres *fwd, fsgpu_swres *rev) {
    if (!ctx || !fwd || !rev) return FSGPU_E_ARG;
    if (!ctx->sw.pending) { ctx->err = "no SW batch in flight"; return FSGPU_E_ARG; }
    ctx->sw.pending = false;
    HIPCHK(hipSetDevice(ctx->device));        // the int32 re-run below launches kernels: the calling thread may have another device current
    const int n = ctx->sw.n;
    if (n == 0) return FSGPU_OK;
    { int rc = syncStream(ctx); if (rc != FSGPU_OK) return rc; }
    memcpy(fwd, ctx->hRes0.p, (size_t) n * 16);
    memcpy(rev, ctx->hRes1.p, (size_t) n * 16);
    // int16 saturation -> int32 re-run with the int32 kernel's segment length (alignScoreEndPos, :313-336)
    for (int dir = 0; dir < 2; dir++) {
        fsgpu_swres *res = dir == 0 ? fwd : rev;
        std::vector<uint32_t> ids;
        std::vector<int> where;
        int maxLt = 1;
        for (int i = 0; i < n; i++)
            if (res[i].score == 32767) {
                ids.push_back(ctx->sw.tids[i]); where.push_back(i);
                maxLt = std::max(maxLt, (ctx->sw.explicitTargets ? ctx->sw.ovLengths : ctx->db->hLengths)[ctx->sw.tids[i]]);
            }
        if (ids.empty()) continue;
        const int m = (int) ids.size();
        memcpy(ctx->hTids.p, ids.data(), (size_t) m * 4);         // pinned staging (sized for n >= m at launch), ordered on the context stream
        HIPCHK(hipMemcpyAsync(ctx->tids.p, ctx->hTids.p, (size_t) m * 4, hipMemcpyHostToDevice, ctx->stream));
        const int16_t *pA = dir == 0 ? ctx->sw.pAAf : ctx->sw.pAAr;
        const int16_t *p3 = dir == 0 ? ctx->sw.p3f : ctx->sw.p3r;
        int rc = runSwPass(ctx, false, pA, p3, nullptr, nullptr, ctx->sw.L, (const uint32_t *) ctx->tids.p, m, maxLt, ctx->sw.go, ctx->sw.ge,
                           (int32_t *) ctx->res0.p, nullptr);
        if (rc != FSGPU_OK) return rc;
        HIPCHK(hipMemcpyAsync(ctx->hRes0.p, ctx->res0.p, (size_t) m * 16, hipMemcpyDeviceToHost, ctx->stream));
        { int rc2 = syncStream(ctx); if (rc2 != FSGPU_OK) return rc2; }
        for (int k = 0; k < m; k++) memcpy(&res[where[k]], (const int32_t *) ctx->hRes0.p + (size_t) k * 4, 16);
    }
    return FSGPU_OK;
}

int fsgpu_sw_batch(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd, const int16_t *pAA_rev, const int16_t *p3Di_rev,
                   int L, const uint32_t *targetIds, int n, int gapOpen, int gapExtend, fsgpu_swres *fwd, fsgpu_swres *rev) {
    int rc = fsgpu_sw_launch(ctx, pAA_fwd, p3Di_fwd, pAA_rev, p3Di_rev, L, targetIds, n, gapOpen, gapExtend);
    if (rc != FSGPU_OK) return rc;
    return fsgpu_sw_finish(ctx, fwd, rev);
}

// Several queries in one go: all single-tile queries (L <= 512) of one register class R share ONE launch -- workgroups
// of 4 waves, each workgroup serving pairs of a single query and loading that query's LDS image -- so the device sees
// tens of thousands of independent waves instead of ~1000 per launch and the long-target tail of one query overlaps
// the bulk of the others.  One call runs ONE direction (dir 0: forward query, 1: reversed query) over the selected
// pairs with k_sw2 (two targets per wave): structurealign looks at the reversed-query score only for pairs that pass
// the forward gates, so the caller runs dir 0 over everything, gates, and runs dir 1 over the survivors.
// Longer queries run as multi-query row-tiled k_sw launches (swLongEnqueue); int16-saturated pairs go through the single-query path.
int fsgpu_sw_multi_dir(fsgpu_ctx *ctx, const fsgpu_sw_query *q, int nq, int gapOpen, int gapExtend, int dir,
                       const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out) {
    if (!ctx || nq < 0 || (nq > 0 && (!q || !out)) || (dir != 0 && dir != 1) || ((sel == nullptr) != (nsel == nullptr))) return FSGPU_E_ARG;
    int rc;
    if ((rc = swCheckCall(ctx, gapOpen, gapExtend)) != FSGPU_OK) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->swLongLaunched = 0; ctx->swLongReused = 0;
    std::vector<size_t> base(nq + 1, 0), sbase(nq + 1, 0);     // offsets into out[] (all pairs) / into the launch (selected pairs)
    bool hasAA = false, anyAA = false, allAA = true;
    for (int i = 0; i < nq; i++) {
        if (!q[i].p3Di_fwd || !q[i].p3Di_rev || q[i].L <= 0 || q[i].L > FSGPU_MAX_SEQ_LEN || q[i].n < 0 || (q[i].n > 0 && !q[i].targetIds) ||
            ((q[i].pAA_fwd == nullptr) != (q[i].pAA_rev == nullptr))) { ctx->err = "fsgpu_sw_multi: bad query"; return FSGPU_E_ARG; }
        anyAA = anyAA || q[i].pAA_fwd != nullptr; allAA = allAA && q[i].pAA_fwd != nullptr;
        base[i + 1] = base[i] + (size_t) q[i].n;
        const int ns = sel ? nsel[i] : q[i].n;
        if ((rc = swCheckPairs(ctx, "fsgpu_sw_multi_dir", q[i].targetIds, q[i].n, sel != nullptr, sel ? sel[i] : nullptr, ns)) != FSGPU_OK) return rc;
        sbase[i + 1] = sbase[i] + (size_t) ns;
    }
    if (anyAA != allAA) { ctx->err = "fsgpu_sw_multi: either all or none of the queries carry AA profiles"; return FSGPU_E_ARG; }
    hasAA = anyAA;
    if (hasAA && !ctx->db->hasAA) { ctx->err = "AA profiles given but the database was loaded without AA sequences"; return FSGPU_E_NODB; }
    const size_t total = sbase[nq];
    auto nSel = [&](int i) { return (int) (sbase[i + 1] - sbase[i]); };
    auto selIdx = [&](int i, int k) { return sel ? sel[i][k] : k; };
    // row-tiled queries: own launches on a side stream, next to the single-tile launches below
    SwLongPlan longPlan;
    {
        std::vector<char> isLong(nq, 0);
        bool any = false;
        for (int i = 0; i < nq; i++) {
            int tiles, R;
            swShape(q[i].L, &tiles, &R);
            if (tiles > 1 && nSel(i) > 0) { isLong[i] = 1; any = true; }
        }
        if (any && (rc = swLongEnqueue(ctx, q, nq, isLong, sel, nsel, base, hasAA, gapOpen, gapExtend, dir, out, longPlan)) != FSGPU_OK) {
            if (ctx->swLong) (void) hipStreamSynchronize(ctx->swLong);
            return rc;
        }
    }
    // whatever goes wrong below: the side stream must be idle before its buffers are reused
    struct LongGuard { fsgpu_ctx *c; bool armed; ~LongGuard() { if (armed && c->swLong) (void) hipStreamSynchronize(c->swLong); } } longGuard{ctx, longPlan.n > 0};
    std::vector<uint32_t> perm;       // launch slot -> index into q[i].targetIds
    std::vector<uint64_t> lkey;
    // ---- launch groups by register class ----
    const int classes[6] = {1, 2, 3, 4, 6, 8};
    std::vector<int> cls(nq, -1);
    for (int i = 0; i < nq; i++) {
        int tiles, R;
        swShape(q[i].L, &tiles, &R);
        if (tiles == 1 && nSel(i) > 0) cls[i] = R;
    }
    size_t imgDwTotal = 0, nBlocks = 0;
    const int ppb = sw2PairsPerBlock();
    for (int i = 0; i < nq; i++) if (cls[i] > 0) { imgDwTotal += (size_t) kSw2Rows * swRowDwords(cls[i]) * (hasAA ? 2 : 1); nBlocks += ((size_t) nSel(i) + ppb - 1) / ppb; }
    if (total) {
        if ((rc = ensureAll(ctx, {{ctx->tids, total * 4}, {ctx->res0, total * 16}})) != FSGPU_OK) return rc;
        if ((rc = ensurePinnedAll(ctx, {{ctx->hRes0, total * 16}, {ctx->hTids, total * 4}})) != FSGPU_OK) return rc;
        // inside every query the pairs are issued longest target first (perm) -- neighbours share a wave, so they should
        // be of similar length --, and the workgroups of a launch are ordered by their longest target (LPT)
        perm.resize(total);
        for (int i = 0; i < nq; i++) {
            const int ns = nSel(i);
            uint32_t *p = perm.data() + sbase[i];
            swSortLongestFirst(ctx->db->hLengths, q[i].targetIds, sel ? sel[i] : nullptr, ns, lkey, p);
            uint32_t *dst = (uint32_t *) ctx->hTids.p + sbase[i];
            for (int k = 0; k < ns; k++) dst[k] = q[i].targetIds[p[k]];
        }
        HIPCHK(hipMemcpyAsync(ctx->tids.p, ctx->hTids.p, total * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    if (dir == 0 || !ctx->evValid[1]) HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));     // a forward + reversed pass pair is timed as one
    if (!ctx->swDirEv[3]) for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ctx->swDirEv[i]));
    ctx->swDirValid[dir] = false;
    if (dir == 0) ctx->swDirValid[1] = false;
    ctx->swDirExtraMs[dir] = 0;
    {
        // work of this pass in the units of the kernel's roofline: DP cells (query rows x target columns of every single-tile pair) and
        // VALU wave-instructions (a wave carries two targets of one query and runs max(LtA, LtB) + lanes - 1 steps; a step is 14 packed
        // instructions per register row + 14 around them -- lane shifts, LDS addresses, column and maximum bookkeeping; counted in the ISA
        // of k_sw2<6, false>: 98 VALU instructions per step outside the new-maximum block -- and 2 per row + 9 more with the AA table: 119)
        double cells = 0, pairs = 0, wsteps = 0;
        const std::vector<int32_t> &len = ctx->db->hLengths;
        for (int i = 0; i < nq; i++) {
            if (cls[i] <= 0) continue;
            const int ns = nSel(i), R = cls[i], lanes = (q[i].L + R - 1) / R;
            const uint32_t *p = perm.data() + sbase[i];
            for (int k = 0; k < ns; k++) {
                const int lt = len[q[i].targetIds[p[k]]];
                cells += (double) q[i].L * lt;
                if ((k & 1) == 0 && lt > 0) wsteps += (double) (lt + lanes - 1) * (14.0 * R + 14.0 + (hasAA ? 2.0 * R + 9.0 : 0.0));   // pairs are longest first: the even one sets the wave's length
            }
            pairs += ns;
        }
        ctx->swDirCells[dir] = cells; ctx->swDirPairs[dir] = pairs; ctx->swDirWaveSteps[dir] = wsteps;
    }
    HIPCHK(hipEventRecord(ctx->swDirEv[2 * dir], ctx->stream));
    
    if (nBlocks) {
        if ((rc = ensurePinned(ctx, ctx->hImg, imgDwTotal * 4 + nBlocks * sizeof(SwBlockDesc) + 64)) != FSGPU_OK) return rc;
        if ((rc = ensure(ctx, ctx->img, imgDwTotal * 4 + nBlocks * sizeof(SwBlockDesc) + 64)) != FSGPU_OK) return rc;
        uint32_t *img = (uint32_t *) ctx->hImg.p;
        SwBlockDesc *hb = (SwBlockDesc *) ((unsigned char *) ctx->hImg.p + ((imgDwTotal * 4 + 15) / 16) * 16);
        const size_t descOff = ((imgDwTotal * 4 + 15) / 16) * 16;
        size_t imgPos = 0, blkPos = 0;
        struct Group { int R; size_t blk0, nblk; };
        std::vector<Group> groups;
        for (int R : classes) {
            Group g{R, blkPos, 0};
            const int rowDw = swRowDwords(R);
            const size_t tblDw = (size_t) kSw2Rows * rowDw;
            for (int i = 0; i < nq; i++) {
                if (cls[i] != R) continue;
                const int L = q[i].L;
                uint32_t *dst0 = img + imgPos;
                for (int tbl = 0; tbl < (hasAA ? 2 : 1); tbl++) {
                    const int16_t *f = tbl == 0 ? q[i].p3Di_fwd : q[i].pAA_fwd;
                    const int16_t *r = tbl == 0 ? q[i].p3Di_rev : q[i].pAA_rev;
                    uint32_t *dst = dst0 + tblDw * tbl;
                    swFillTable(dst, R, L, 0, true, f, r);
                    // row 21: "past the end of this target" -- INT16_MIN in the 3Di table, 0 in the AA table (their sum must not wrap)
                    const uint32_t dead = tbl == 0 ? 0x80008000u : 0u;
                    for (int x = 0; x < rowDw; x++) dst[(size_t) kAlphabet * rowDw + x] = dead;
                }
                const int ns = nSel(i);
                for (int p0 = 0; p0 < ns; p0 += ppb) {
                    SwBlockDesc &d = hb[blkPos++];
                    d.imgOff = (uint32_t) imgPos; d.firstPair = (uint32_t) (sbase[i] + p0); d.nPairs = (uint16_t) std::min(ppb, ns - p0);
                    d.rowsInTile = (uint16_t) L; d.segLen = (uint32_t) ((L + 15) / 16);
                    g.nblk++;
                }
                imgPos += tblDw * (hasAA ? 2 : 1);
            }
            if (g.nblk) {
                // first pair of a workgroup is its longest (pairs are length-sorted inside the query)
                const uint32_t *ht = (const uint32_t *) ctx->hTids.p;
                const std::vector<int32_t> &len = ctx->db->hLengths;
                std::stable_sort(hb + g.blk0, hb + g.blk0 + g.nblk, [&](const SwBlockDesc &x, const SwBlockDesc &y) { return len[ht[x.firstPair]] > len[ht[y.firstPair]]; });
                groups.push_back(g);
            }
        }
        HIPCHK(hipMemcpyAsync(ctx->img.p, ctx->hImg.p, descOff + nBlocks * sizeof(SwBlockDesc), hipMemcpyHostToDevice, ctx->stream));
        // every register-class group gets its own stream: their long-target tails overlap instead of queueing up
        if ((rc = swFork(ctx, ctx->stream, groups.size())) != FSGPU_OK) return rc;
        size_t gi = 0;
        for (const Group &g : groups) {
            hipStream_t gs = gi == 0 ? ctx->stream : ctx->swAux[gi];
            SwArgs sa;
            sa.aa = ctx->db->alnAA; sa.ss = ctx->db->aln3di; sa.offsets = ctx->db->dOffsets; sa.lengths = ctx->db->dLengths;
            sa.targetIds = (const uint32_t *) ctx->tids.p; sa.nPairs = (int) total;
            sa.profSS = (const uint32_t *) ctx->img.p; sa.profAA = nullptr;
            sa.tileBase = 0; sa.rowsInTile = 0; sa.segLen = 1;
            sa.go = (uint32_t) gapOpen | ((uint32_t) gapOpen << 16);
            sa.ge = (uint32_t) gapExtend | ((uint32_t) gapExtend << 16);
            sa.tileIn = 0; sa.tileOut = 0; sa.borderIn = nullptr; sa.borderOut = nullptr; sa.borderStride = 0; sa.keys = nullptr;
            sa.res0 = (int32_t *) ctx->res0.p; sa.res1 = nullptr;
            sa.blocks = (const SwBlockDesc *) ((const unsigned char *) ctx->img.p + descOff) + g.blk0;
            sa.dir = dir;
            rc = launchSwBlocks2(ctx, g.R, hasAA, sa, (int) g.nblk, ppb, gs);
            if (rc != FSGPU_OK) return rc;
            gi++;
        }
        if ((rc = swJoin(ctx, ctx->stream, groups.size())) != FSGPU_OK) return rc;
    }
    HIPCHK(hipEventRecord(ctx->ev[3], ctx->stream));
    HIPCHK(hipEventRecord(ctx->swDirEv[2 * dir + 1], ctx->stream));
    ctx->swDirValid[dir] = true;
    ctx->evValid[1] = true;
    if (total) {
        HIPCHK(hipMemcpyAsync(ctx->hRes0.p, ctx->res0.p, total * 16, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = syncStream(ctx)) != FSGPU_OK) return rc;
        const fsgpu_swres *r0 = (const fsgpu_swres *) ctx->hRes0.p;
        for (int i = 0; i < nq; i++)
            if (cls[i] > 0)
                for (int k = 0; k < nSel(i); k++) out[base[i] + perm[sbase[i] + k]] = r0[sbase[i] + k];
    }
    rc = swLongCollect(ctx, longPlan, base, dir, out);
    longGuard.armed = false;
    if (rc != FSGPU_OK) return rc;
    if (dir == 1) ctx->swLongRev.clear();
    // int16-saturated pairs: the single-query path re-runs them with the int32 kernel (computes both directions, keeps `dir`)
    std::vector<fsgpu_swres> f2, r2;
    for (int i = 0; i < nq; i++) {
        const int ns = nSel(i);
        if (ns == 0) continue;
        std::vector<uint32_t> ids;
        std::vector<int> where;
        for (int k = 0; k < ns; k++) {
            const int j = selIdx(i, k);
            if (out[base[i] + j].score == 32767) { ids.push_back(q[i].targetIds[j]); where.push_back(j); }
        }
        if (ids.empty()) continue;
        f2.resize(ids.size()); r2.resize(ids.size());
        rc = fsgpu_sw_batch(ctx, q[i].pAA_fwd, q[i].p3Di_fwd, q[i].pAA_rev, q[i].p3Di_rev, q[i].L, ids.data(), (int) ids.size(), gapOpen, gapExtend,
                            f2.data(), r2.data());
        if (rc != FSGPU_OK) return rc;
        for (size_t k = 0; k < ids.size(); k++) out[base[i] + where[k]] = dir == 0 ? f2[k] : r2[k];
    }
    return FSGPU_OK;
}

// both directions of every pair: two fsgpu_sw_multi_dir passes (callers that gate between the passes save most of the second)
int fsgpu_sw_multi(fsgpu_ctx *ctx, const fsgpu_sw_query *q, int nq, int gapOpen, int gapExtend, fsgpu_swres *fwd, fsgpu_swres *rev) {
    if (!ctx || nq < 0 || (nq > 0 && (!q || !fwd || !rev))) return FSGPU_E_ARG;
    int rc = fsgpu_sw_multi_dir(ctx, q, nq, gapOpen, gapExtend, 0, nullptr, nullptr, fwd);
    if (rc != FSGPU_OK) return rc;
    return fsgpu_sw_multi_dir(ctx, q, nq, gapOpen, gapExtend, 1, nullptr, nullptr, rev);
}

void fsgpu_sw_kernel_counts(const fsgpu_ctx *ctx, uint64_t out[36]) {
    for (int i = 0; i < 36; i++) out[i] = ctx ? ctx->swKernelCount[i] : 0;
}

} // extern "C"

// fsgpu_sw_scan.hip -- fsgpu_sw_scan_c: the forward structure Smith-Waterman of every query against EVERY target of the database, with the selection
// against a score cutoff on the device (Foldseek's --exhaustive-search: no prefilter, alignStructure's first e-value gate as a cutoff).
//
// The pass is k_sw3 as fsgpu_sw_multi_dir_c launches it, through the same steps (fsgpu_sw3_plan.h) with a "presorted, all targets" plan: the order of the
// targets is sorted once per database, the ids of a pass are written on the device, the records stay in s3res, and k_sw_scan_count / _offsets / _emit
// (k_sw_scan.hpp) compact the survivors, which alone cross the bus.  Queries are taken in sub-batches under a byte budget (FSGPU_SCAN_BYTES, default
// 1 GiB, 20 bytes per target and query).
// Queries of more than 1024 residues are outside k_sw3's classes: they go through fsgpu_sw_multi_dir in chunks of targets and are filtered on the
// host.  That path is correct, not fast: N records per such query are downloaded.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_sw3.hpp"
#include "k_sw_scan.hpp"
#include "fsgpu_sw3.h"
#include "fsgpu_sw3_plan.h"
#include "fs_scan_order.h"

namespace {

constexpr uint64_t kScanDefaultBytes = 1ull << 30;
constexpr int kScanLongChunk = 1 << 16;               // targets per fsgpu_sw_multi_dir call of a long query

struct ScanHit { uint32_t id; fsgpu_swres r; };

// the database's order and its device copy, built by the first scan of any context of this DbStore
int scanOrder(fsgpu_ctx *ctx) {
    DbStore &db = *ctx->db;
    std::lock_guard<std::mutex> g(db.itemMutex);
    if (db.scanOrderBuilt) return FSGPU_OK;
    int maxLen = 0;
    for (int32_t l : db.hLengths) maxLen = std::max(maxLen, (int) l);
    fsScanOrder(db.hLengths.data(), db.n, maxLen, db.hScanOrder);
    HIPCHK(hipMalloc(&db.dScanOrder, std::max<size_t>(db.n, 1) * 4));
    // the host vector is pageable: the copy has left it when the call returns
    hipError_t e = hipMemcpy(db.dScanOrder, db.hScanOrder.data(), db.n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void) hipFree(db.dScanOrder); db.dScanOrder = nullptr; ctx->err = std::string("hipMemcpy: ") + hipGetErrorString(e); return FSGPU_E_HIP; }
    db.scanOrderBuilt = true;
    return FSGPU_OK;
}

float elapsedOr0(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) { (void) hipGetLastError(); return 0; }
    return ms;
}

// the int32 re-run of the survivors whose int16 score is the ceiling (as sw3RerunSaturated), the cutoff on the final scores, ascending ids
int scanFinish(fsgpu_ctx *ctx, const Sw3Plan &p, int i, int cutoff, std::vector<ScanHit> &hits) {
    std::vector<uint32_t> ids;
    std::vector<size_t> where;
    for (size_t k = 0; k < hits.size(); k++) if (hits[k].r.score == 32767) { ids.push_back(hits[k].id); where.push_back(k); }
    if (!ids.empty()) {
        ctx->s3Plan[7] += (uint32_t) ids.size();
        Sw3Prof pr;
        p.profilesOf(i, pr);
        std::vector<fsgpu_swres> f2(ids.size()), r2(ids.size());
        const int rc = fsgpu_sw_batch(ctx, p.hasAA ? pr.aF.data() : nullptr, pr.sF.data(), p.hasAA ? pr.aR.data() : nullptr, pr.sR.data(), p.q[i].L, ids.data(), (int) ids.size(),
                                      p.gapOpen, p.gapExtend, f2.data(), r2.data());
        if (rc != FSGPU_OK) return rc;
        for (size_t k = 0; k < ids.size(); k++) hits[where[k]].r = f2[k];
    }
    hits.erase(std::remove_if(hits.begin(), hits.end(), [&](const ScanHit &h) { return h.r.score < cutoff; }), hits.end());
    std::sort(hits.begin(), hits.end(), [](const ScanHit &a, const ScanHit &b) { return a.id < b.id; });
    return FSGPU_OK;
}

// one long query: the profile path over all targets, kScanLongChunk at a time
int scanLong(fsgpu_ctx *ctx, const Sw3Plan &p, int i, int cutoff, std::vector<ScanHit> &hits, double acc[4]) {
    const uint64_t N = ctx->db->n;
    Sw3Prof pr;
    p.profilesOf(i, pr);
    fsgpu_sw_query cq;
    cq.pAA_fwd = p.hasAA ? pr.aF.data() : nullptr; cq.pAA_rev = p.hasAA ? pr.aR.data() : nullptr;
    cq.p3Di_fwd = pr.sF.data(); cq.p3Di_rev = pr.sR.data();
    cq.L = p.q[i].L;
    std::vector<uint32_t> ids;
    std::vector<fsgpu_swres> res;
    for (uint64_t t0 = 0; t0 < N; t0 += kScanLongChunk) {
        const int n = (int) std::min<uint64_t>(kScanLongChunk, N - t0);
        ids.resize(n); res.resize(n);
        std::iota(ids.begin(), ids.end(), (uint32_t) t0);
        cq.n = n; cq.targetIds = ids.data();
        const int rc = fsgpu_sw_multi_dir(ctx, &cq, 1, p.gapOpen, p.gapExtend, 0, nullptr, nullptr, res.data());
        if (rc != FSGPU_OK) return rc;
        double pp[8];
        fsgpu_sw_last_passes(ctx, pp);
        if (pp[0] >= 0) for (int k = 0; k < 4; k++) acc[k] += pp[k];
        for (int k = 0; k < n; k++) if (res[k].score >= cutoff) hits.push_back({ids[k], res[k]});
    }
    ctx->s3Plan[6] += (uint32_t) N;
    return FSGPU_OK;
}

} // namespace

extern "C" {

int fsgpu_sw_scan_c(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend, const int32_t *cutoff,
                    uint32_t *outIds, fsgpu_swres *outFwd, uint64_t cap, uint64_t *outBase) {
    if (!ctx || !mat3Di || nq < 0 || !outBase || (nq > 0 && (!q || !cutoff)) || (cap > 0 && (!outIds || !outFwd))) return FSGPU_E_ARG;
    const auto tHost0 = std::chrono::steady_clock::now();
    Sw3Plan all;
    all.who = "fsgpu_sw_scan_c";
    all.mat3Di = mat3Di; all.matAA = matAA; all.q = q; all.nq = nq; all.gapOpen = gapOpen; all.gapExtend = gapExtend; all.dir = 0;
    all.hasAA = matAA != nullptr;
    all.slot = 0; all.nDirs = 1; all.dir0 = 0;
    all.S = ctx->swHi ? ctx->swHi : ctx->stream;
    int rc;
    // a database without entries answers empty lists (fsgpu_db_load refuses n == 0, so this is a context whose store is empty by other means)
    if (ctx->db && ctx->db->n == 0) { for (int i = 0; i <= nq; i++) outBase[i] = 0; return FSGPU_OK; }
    if ((rc = sw3Validate(ctx, all)) != FSGPU_OK) return rc;
    for (int i = 0; i < nq; i++) {
        if (q[i].n != 0 || q[i].targetIds) { ctx->err = "fsgpu_sw_scan_c: a query's n / targetIds must be 0 / NULL (the scan runs every target)"; return FSGPU_E_ARG; }
        if (cutoff[i] < 0 || cutoff[i] > 32767) { ctx->err = "fsgpu_sw_scan_c: cutoff outside 0..32767"; return FSGPU_E_ARG; }
    }
    if (ctx->db->n > 0x7fffffffull) { ctx->err = "fsgpu_sw_scan_c: more than 2^31 - 1 targets"; return FSGPU_E_UNSUPPORTED; }
    const uint32_t N = (uint32_t) ctx->db->n;
    const uint64_t budget = [] { const char *e = getenv("FSGPU_SCAN_BYTES"); const long long v = e && *e ? atoll(e) : 0; return v > 0 ? (uint64_t) v : kScanDefaultBytes; }();   // read per call: the tests force one query per sub-batch
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t S = all.S;
    Sw3Drain drain{ctx, S};
    if ((rc = scanOrder(ctx)) != FSGPU_OK) return rc;
    if (!ctx->scanEv[3]) for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ctx->scanEv[i]));
    memset(ctx->s3Plan, 0, sizeof(ctx->s3Plan));
    for (double &m : ctx->scanMs) m = 0;
    memset(ctx->scanStats, 0, sizeof(ctx->scanStats));

    sw3Classify(all);
    std::vector<std::vector<ScanHit>> hits(nq);
    double acc[4] = {0, 0, 0, 0};                      // ms, cells, pairs, wave-instructions of what ran so far (fsgpu_sw_last_passes)
    for (int i : all.classic) if ((rc = scanLong(ctx, all, i, cutoff[i], hits[i], acc)) != FSGPU_OK) return rc;
    std::vector<int> compact;
    for (int i = 0; i < nq; i++) if (all.cR[i] > 0) compact.push_back(i);

    const int perBatch = fsScanQueriesPerBatch(N, budget);
    const uint32_t nChunks = (N + kScanChunk - 1) / kScanChunk;
    double hostPlanMs = 0;
    std::vector<fsgpu_sw_cquery> sq;
    for (size_t b0 = 0; b0 < compact.size(); b0 += (size_t) perBatch) {
        const auto tPlan0 = std::chrono::steady_clock::now();
        const int nb = (int) std::min<size_t>((size_t) perBatch, compact.size() - b0);
        sq.assign(nb, fsgpu_sw_cquery{});
        for (int j = 0; j < nb; j++) sq[j] = q[compact[b0 + j]];
        Sw3Plan p;
        p.who = all.who;
        p.mat3Di = mat3Di; p.matAA = matAA; p.q = sq.data(); p.nq = nb; p.gapOpen = gapOpen; p.gapExtend = gapExtend; p.dir = 0;
        p.hasAA = all.hasAA; p.slot = 0; p.nDirs = 1; p.dir0 = 0; p.S = S;
        p.allOrder = ctx->db->hScanOrder.data(); p.allN = (int) N;
        p.clMs = acc[0]; p.clCells = acc[1]; p.clPairs = acc[2]; p.clSteps = acc[3];
        sw3Classify(p);
        if ((rc = sw3BeginPass(ctx, p)) != FSGPU_OK) return rc;
        sw3SortAndSplit(ctx, p);
        if ((rc = sw3Images(ctx, p)) != FSGPU_OK) return rc;
        sw3Groups(p);
        sw3RecordPlan(ctx, p);
        if ((rc = sw3Descriptors(ctx, p)) != FSGPU_OK) return rc;
        // [cutoffs int32 | survivors per query uint32 | output bases uint64], each part 16-byte aligned
        const size_t part = ((size_t) nb * 4 + 15) / 16 * 16, baseOff = 2 * part, metaBytes = baseOff + (size_t) nb * 8;
        if ((rc = ensurePinned(ctx, ctx->hScanMeta, metaBytes)) != FSGPU_OK) return rc;
        if ((rc = ensureAll(ctx, {{ctx->scanMeta, metaBytes}, {ctx->scanCnt, (size_t) nb * nChunks * 4}})) != FSGPU_OK) return rc;
        unsigned char *hm = (unsigned char *) ctx->hScanMeta.p, *dm = (unsigned char *) ctx->scanMeta.p;
        for (int j = 0; j < nb; j++) ((int32_t *) hm)[j] = cutoff[compact[b0 + j]];
        HIPCHK(hipMemcpyAsync(dm, hm, part, hipMemcpyHostToDevice, S));
        hostPlanMs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tPlan0).count();
        uint32_t *dTids = (uint32_t *) ctx->s3pass.p;               // p.total = nb * N ids, in front of the descriptors
        hipLaunchKernelGGL(k_sw_scan_ids, dim3(std::min<uint32_t>((N + kScanThreads - 1) / kScanThreads, 1024u), nb), dim3(kScanThreads), 0, S,
                           (const uint32_t *) ctx->db->dScanOrder, N, dTids);
        HIPCHK(hipGetLastError());
        if ((rc = sw3Launch(ctx, p)) != FSGPU_OK) return rc;
        // selection, first half: counts and offsets
        const int4 *dRec = (const int4 *) ctx->s3res.p;
        uint32_t *dTotals = (uint32_t *) (dm + part);
        HIPCHK(hipEventRecord(ctx->scanEv[0], S));
        hipLaunchKernelGGL(k_sw_scan_count, dim3(nChunks, nb), dim3(kScanThreads), 0, S, dRec, N, (const int32_t *) dm, (uint32_t *) ctx->scanCnt.p);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_sw_scan_offsets, dim3(nb), dim3(kScanThreads), 0, S, (uint32_t *) ctx->scanCnt.p, nChunks, dTotals);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->scanEv[1], S));
        HIPCHK(hipMemcpyAsync(hm + part, dTotals, (size_t) nb * 4, hipMemcpyDeviceToHost, S));
        if ((rc = syncStreamOf(ctx, S)) != FSGPU_OK) return rc;
        // second half: the output of this sub-batch is sized by its survivors
        const uint32_t *hTotals = (const uint32_t *) (hm + part);
        uint64_t *hBase = (uint64_t *) (hm + baseOff);
        uint64_t nOut = 0;
        for (int j = 0; j < nb; j++) { hBase[j] = nOut; nOut += hTotals[j]; }
        const size_t recOff = ((size_t) nOut * 4 + 15) / 16 * 16, outBytes = recOff + (size_t) nOut * 16;
        if ((rc = ensurePinned(ctx, ctx->hScanOut, std::max<size_t>(outBytes, 16))) != FSGPU_OK) return rc;
        if ((rc = ensure(ctx, ctx->scanOut, std::max<size_t>(outBytes, 16))) != FSGPU_OK) return rc;
        HIPCHK(hipMemcpyAsync(dm + baseOff, hBase, (size_t) nb * 8, hipMemcpyHostToDevice, S));
        HIPCHK(hipEventRecord(ctx->scanEv[2], S));
        hipLaunchKernelGGL(k_sw_scan_emit, dim3(nChunks, nb), dim3(kScanThreads), 0, S, dRec, (const uint32_t *) dTids, N, (const int32_t *) dm,
                           (const uint32_t *) ctx->scanCnt.p, (const uint64_t *) (dm + baseOff), (uint32_t *) ctx->scanOut.p,
                           (int4 *) ((unsigned char *) ctx->scanOut.p + recOff), nOut);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->scanEv[3], S));
        if (nOut > 0) HIPCHK(hipMemcpyAsync(ctx->hScanOut.p, ctx->scanOut.p, outBytes, hipMemcpyDeviceToHost, S));
        if ((rc = syncStreamOf(ctx, S)) != FSGPU_OK) return rc;
        // the accounting carries this sub-batch's figures into the next (sw3Descriptors added its cells to what cl* held)
        acc[0] += elapsedOr0(ctx->swDirEv[0], ctx->swDirEv[1]);
        acc[1] = ctx->swDirCells[0]; acc[2] = ctx->swDirPairs[0]; acc[3] = ctx->swDirWaveSteps[0];
        ctx->scanMs[1] += elapsedOr0(ctx->scanEv[0], ctx->scanEv[1]);
        ctx->scanMs[2] += elapsedOr0(ctx->scanEv[2], ctx->scanEv[3]);
        ctx->scanStats[0] += 1; ctx->scanStats[1] += (double) nOut;
        const uint32_t *hIds = (const uint32_t *) ctx->hScanOut.p;
        const fsgpu_swres *hRec = (const fsgpu_swres *) ((const unsigned char *) ctx->hScanOut.p + recOff);
        for (int j = 0; j < nb; j++) {
            std::vector<ScanHit> &h = hits[compact[b0 + j]];
            h.resize(hTotals[j]);
            for (uint32_t k = 0; k < hTotals[j]; k++) h[k] = {hIds[hBase[j] + k], hRec[hBase[j] + k]};
        }
        // (the re-run goes through fsgpu_sw_batch, which has buffers and a stream of its own: the staging above has been read)
        for (int j = 0; j < nb; j++) if ((rc = scanFinish(ctx, p, j, cutoff[compact[b0 + j]], hits[compact[b0 + j]])) != FSGPU_OK) return rc;
    }
    for (int i : all.classic) std::sort(hits[i].begin(), hits[i].end(), [](const ScanHit &a, const ScanHit &b) { return a.id < b.id; });
    // what fsgpu_sw_last_passes reports: every sub-batch and every long query of the call (the last sub-batch's events carry the rest as extra time)
    if (!compact.empty()) ctx->swDirExtraMs[0] = acc[0] - elapsedOr0(ctx->swDirEv[0], ctx->swDirEv[1]);
    else if (!all.classic.empty()) {
        if (!ctx->swDirEv[3]) for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ctx->swDirEv[i]));
        HIPCHK(hipEventRecord(ctx->swDirEv[0], S)); HIPCHK(hipEventRecord(ctx->swDirEv[1], S));
        if ((rc = syncStreamOf(ctx, S)) != FSGPU_OK) return rc;
        ctx->swDirValid[0] = true; ctx->swDirValid[1] = false;
        ctx->swDirExtraMs[0] = acc[0]; ctx->swDirCells[0] = acc[1]; ctx->swDirPairs[0] = acc[2]; ctx->swDirWaveSteps[0] = acc[3];
    }
    ctx->scanMs[0] = acc[0];
    ctx->scanStats[2] = hostPlanMs;
    drain.ok = true;
    uint64_t at = 0;
    for (int i = 0; i < nq; i++) {
        outBase[i] = at;
        for (const ScanHit &h : hits[i]) { if (at < cap) { outIds[at] = h.id; outFwd[at] = h.r; } at++; }
    }
    outBase[nq] = at;
    ctx->scanStats[3] = (double) at;
    ctx->scanStats[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tHost0).count();
    if (at > cap) { ctx->err = "fsgpu_sw_scan_c: " + std::to_string(at) + " survivors, room for " + std::to_string(cap) + " (outBase holds the counts; call again)"; return FSGPU_E_OUTPUT; }
    return FSGPU_OK;
}

void fsgpu_sw_scan_last(const fsgpu_ctx *ctx, double *out8) {
    if (!out8) return;
    for (int i = 0; i < 8; i++) out8[i] = ctx ? ctx->scanStats[i] : 0;
}

} // extern "C"

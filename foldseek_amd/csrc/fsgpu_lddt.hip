// fsgpu_lddt.hip -- C ABI of the device LDDT (include/fsgpu.h: fsgpu_lddt_batch; kernels: k_lddt.hpp).
// One call = the accepted hits of one alignment batch.  One upload (pinned staging, asynchronous on the context's stream), two kernels, one download, one
// wait.  The workspaces live in the context and only grow.  No host path: an alignment of any length runs on the device.
// Built without floating-point contraction and with correctly rounded division and square root (Makefile): the per-column values are compared bit for bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_lddt.hpp"

namespace {
inline size_t up16(size_t x) { return (x + 15) & ~(size_t) 15; }
}

extern "C" int fsgpu_lddt_batch(fsgpu_ctx *ctx, const fsgpu_lddt_query *queries, int nq, const fsgpu_lddt_task *tasks, int nt, const float *tCoords,
                                uint64_t tCoordsLen, const char *bt, uint64_t btBytes, int32_t *alignLength, float *out, uint64_t outCap) {
    if (!ctx || nq < 0 || nt < 0 || (nt > 0 && (!queries || !tasks || !alignLength || nq == 0))) return FSGPU_E_ARG;
    if (nt == 0) return FSGPU_OK;
    if (nq > 65535) { ctx->err = "fsgpu_lddt_batch: at most 65535 queries per call"; return FSGPU_E_ARG; }
    if ((tCoordsLen > 0 && !tCoords) || (btBytes > 0 && !bt) || (outCap > 0 && !out)) { ctx->err = "fsgpu_lddt_batch: null buffer"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    // ---- plan: query blob, per task the aligned columns (counted here: they size the workspace slices and bound every index the kernel forms)
    size_t qFloats = 0, maxL = 0;
    for (int i = 0; i < nq; i++) {
        if (queries[i].L <= 0 || queries[i].L > FSGPU_MAX_SEQ_LEN || !queries[i].ca) { ctx->err = "fsgpu_lddt_batch: bad query"; return FSGPU_E_ARG; }
        qFloats += 3 * (size_t) queries[i].L;
        maxL = std::max(maxL, (size_t) queries[i].L);
    }
    if (qFloats >= (1ull << 32) || tCoordsLen >= (1ull << 40) || btBytes >= (1ull << 40)) { ctx->err = "fsgpu_lddt_batch: batch too large"; return FSGPU_E_NOMEM; }
    std::vector<uint32_t> &order = ctx->ldOrder, &counts = ctx->ldCounts;
    std::vector<uint64_t> &colOff = ctx->ldColOff;
    order.resize(nt); counts.resize(nt); colOff.resize(nt);
    size_t totalCols = 0;
    for (int t = 0; t < nt; t++) {
        const fsgpu_lddt_task &k = tasks[t];
        if (k.query >= (uint32_t) nq || k.tLen <= 0 || k.tLen > FSGPU_MAX_SEQ_LEN || k.qStart < 0 || k.dbStart < 0 || k.tOff > tCoordsLen ||
            3 * (uint64_t) k.tLen > tCoordsLen - k.tOff || k.btOff > btBytes || k.btLen > btBytes - k.btOff) {
            ctx->err = "fsgpu_lddt_batch: task " + std::to_string(t) + " out of range"; return FSGPU_E_ARG;
        }
        uint64_t nM = 0, nI = 0, nD = 0;
        const char *b = bt + k.btOff;
        for (uint32_t i = 0; i < k.btLen; i++) { nM += b[i] == 'M'; nI += b[i] == 'I'; nD += b[i] == 'D'; }
        if ((uint64_t) k.qStart + nM + nI > (uint64_t) queries[k.query].L || (uint64_t) k.dbStart + nM + nD > (uint64_t) k.tLen) {
            ctx->err = "fsgpu_lddt_batch: the backtrace of task " + std::to_string(t) + " runs past a sequence end"; return FSGPU_E_ARG;
        }
        if (k.outOff > outCap || nM > outCap - k.outOff) { ctx->err = "fsgpu_lddt_batch: out is too small for task " + std::to_string(t); return FSGPU_E_ARG; }
        counts[t] = (uint32_t) nM; order[t] = (uint32_t) t;
        totalCols += nM;
    }
    // longest first: the work of a task is quadratic in its columns, and one workgroup owns it
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return counts[x] > counts[y]; });
    // ---- staging: [query coordinates | target coordinates | backtraces | task descriptors | query descriptors]
    const size_t tcOff = up16(qFloats * 4), btOffB = up16(tcOff + tCoordsLen * 4), taskOff = up16(btOffB + btBytes),
                 qdOff = up16(taskOff + (size_t) nt * sizeof(LddtTask)), inBytes = qdOff + (size_t) nq * sizeof(LddtQuery);
    const size_t outBytes = up16(totalCols * 4) + (size_t) nt * 4;
    int rc;
    const void *normBefore = ctx->ldNorm.p;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hLdIn, inBytes}, {ctx->hLdOut, outBytes}})) != FSGPU_OK) return rc;
    if ((rc = ensureAll(ctx, {{ctx->ldIn, inBytes}, {ctx->ldNorm, std::max<size_t>(qFloats / 3, 1) * 4}, {ctx->ldCols, std::max<size_t>(totalCols, 1) * kLddtAxes * 4},
                              {ctx->ldOut, outBytes}})) != FSGPU_OK) return rc;
    if (!ctx->ldEv[0]) for (int i = 0; i < 3; i++) HIPCHK(hipEventCreate(&ctx->ldEv[i]));
    unsigned char *hb = (unsigned char *) ctx->hLdIn.p;
    LddtQuery *hq = (LddtQuery *) (hb + qdOff);
    {
        size_t off = 0;
        for (int i = 0; i < nq; i++) {
            const size_t L = (size_t) queries[i].L;
            memcpy(hb + off * 4, queries[i].ca, 3 * L * 4);
            hq[i].cOff = (uint32_t) off; hq[i].L = (uint32_t) L; hq[i].nOff = (uint32_t) (off / 3); hq[i].pad = 0;
            off += 3 * L;
        }
    }
    if (tCoordsLen) memcpy(hb + tcOff, tCoords, tCoordsLen * 4);
    if (btBytes) memcpy(hb + btOffB, bt, btBytes);
    LddtTask *ht = (LddtTask *) (hb + taskOff);
    {
        uint64_t col = 0;
        for (int s = 0; s < nt; s++) {
            const uint32_t t = order[s];
            const fsgpu_lddt_task &k = tasks[t];
            LddtTask &d = ht[s];
            d.query = k.query; d.tLen = (uint32_t) k.tLen; d.tOff = k.tOff; d.qStart = k.qStart; d.dbStart = k.dbStart; d.btOff = k.btOff; d.btLen = k.btLen;
            d.nCols = counts[t]; d.colOff = col; d.slot = t; d.pad = 0;
            colOff[t] = col;
            col += counts[t];
        }
    }
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->ldIn.p, hb, inBytes, hipMemcpyHostToDevice, st));
    LddtArgs a;
    const unsigned char *db = (const unsigned char *) ctx->ldIn.p;
    a.queries = (const LddtQuery *) (db + qdOff); a.tasks = (const LddtTask *) (db + taskOff);
    a.qc = (const float *) db; a.tc = (const float *) (db + tcOff); a.bt = (const char *) (db + btOffB);
    a.norm = (float *) ctx->ldNorm.p; a.cols = (float *) ctx->ldCols.p; a.out = (float *) ctx->ldOut.p;
    a.alnLen = (int32_t *) ((char *) ctx->ldOut.p + up16(totalCols * 4));
    // The norms depend on the query alone.  A caller that asks hit by hit (structurealign with --max-accept / --max-rejected) sends the same single query
    // many times: its norms are kept (the coordinates are compared; the buffer only grows, and growing it drops them).
    const bool haveNorm = nq == 1 && ctx->ldNorm.p == normBefore && ctx->ldNormQuery.size() == qFloats &&
                          memcmp(ctx->ldNormQuery.data(), queries[0].ca, qFloats * 4) == 0;
    if (!haveNorm) ctx->ldNormQuery.clear();
    HIPCHK(hipEventRecord(ctx->ldEv[0], st));
    if (!haveNorm) {
        hipLaunchKernelGGL(k_lddt_norm, dim3((unsigned) ((maxL + kLddtBlock - 1) / kLddtBlock), (unsigned) nq), dim3(kLddtBlock), 0, st, a);
        ctx->ldNormRuns++;
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->ldEv[1], st));
    hipLaunchKernelGGL(k_lddt_pairs, dim3((unsigned) nt), dim3(kLddtBlock), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ldEv[2], st));
    HIPCHK(hipMemcpyAsync(ctx->hLdOut.p, ctx->ldOut.p, outBytes, hipMemcpyDeviceToHost, st));
    if ((rc = syncStream(ctx)) != FSGPU_OK) return rc;
    if (nq == 1 && !haveNorm) ctx->ldNormQuery.assign(queries[0].ca, queries[0].ca + qFloats);          // valid from here: the kernels of this call have run
    for (int i = 0; i < 2; i++) {
        float ms = -1;
        if (hipEventElapsedTime(&ms, ctx->ldEv[i], ctx->ldEv[i + 1]) != hipSuccess) { ms = -1; (void) hipGetLastError(); }
        ctx->ldMs[i] = ms;
    }
    const float *ho = (const float *) ctx->hLdOut.p;
    const int32_t *hl = (const int32_t *) ((const char *) ctx->hLdOut.p + up16(totalCols * 4));
    for (int t = 0; t < nt; t++) {
        if (hl[t] != (int32_t) counts[t]) { ctx->err = "fsgpu_lddt_batch: the device counted " + std::to_string(hl[t]) + " aligned columns for task " + std::to_string(t) + ", the host " + std::to_string(counts[t]); return FSGPU_E_HIP; }
        alignLength[t] = hl[t];
        if (counts[t]) memcpy(out + tasks[t].outOff, ho + colOff[t], (size_t) counts[t] * 4);
    }
    return FSGPU_OK;
}

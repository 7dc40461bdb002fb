// fsgpu_tm.hip -- C ABI of the device TM-score (include/fsgpu.h: fsgpu_tm_batch, kernels: k_tm.hpp; fsgpu_tm_superpose_batch, which also returns the
// superposition and has an exact mode, kernels: k_tm_exact.hpp).
// One call = the accepted hits of one alignment batch.  One upload (pinned staging, asynchronous on the context's stream), two kernels, one download, one
// wait.  The workspaces live in the context and only grow.  No host path: an alignment of any length runs on the device.
// Built without floating-point contraction and with correctly rounded division and square root (Makefile): the values are compared bit for bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_tm.hpp"
#include "k_tm_exact.hpp"

namespace {
inline size_t up16(size_t x) { return (x + 15) & ~(size_t) 15; }
}

extern "C" int fsgpu_tm_batch(fsgpu_ctx *ctx, const fsgpu_lddt_query *queries, int nq, const fsgpu_tm_task *tasks, int nt, const float *tCoords,
                              uint64_t tCoordsLen, const char *bt, uint64_t btBytes, int32_t *nPairs, float *scores, float *rmsd) {
    if (!ctx || nq < 0 || nt < 0 || (nt > 0 && (!queries || !tasks || !nPairs || !scores || !rmsd || nq == 0))) return FSGPU_E_ARG;
    if (nt == 0) return FSGPU_OK;
    if (nq > 65535) { ctx->err = "fsgpu_tm_batch: at most 65535 queries per call"; return FSGPU_E_ARG; }
    if ((tCoordsLen > 0 && !tCoords) || (btBytes > 0 && !bt)) { ctx->err = "fsgpu_tm_batch: null buffer"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    // ---- plan: query blob, per task the pairs (counted here: they size the workspace slices and bound every index the kernels form)
    size_t qFloats = 0;
    for (int i = 0; i < nq; i++) {
        if (queries[i].L <= 0 || queries[i].L > FSGPU_MAX_SEQ_LEN || !queries[i].ca) { ctx->err = "fsgpu_tm_batch: bad query"; return FSGPU_E_ARG; }
        qFloats += 3 * (size_t) queries[i].L;
    }
    if (qFloats >= (1ull << 32) || tCoordsLen >= (1ull << 40) || btBytes >= (1ull << 40)) { ctx->err = "fsgpu_tm_batch: batch too large"; return FSGPU_E_NOMEM; }
    std::vector<uint32_t> &counts = ctx->tmCounts;
    counts.resize(nt);
    size_t totalPairs = 0, maskWords = 0;
    for (int t = 0; t < nt; t++) {
        const fsgpu_tm_task &k = tasks[t];
        if (k.query >= (uint32_t) nq || k.tLen <= 0 || k.tLen > FSGPU_MAX_SEQ_LEN || k.qStart < 0 || k.dbStart < 0 || k.tOff > tCoordsLen ||
            3 * (uint64_t) k.tLen > tCoordsLen - k.tOff || k.btOff > btBytes || k.btLen > btBytes - k.btOff) {
            ctx->err = "fsgpu_tm_batch: task " + std::to_string(t) + " out of range"; return FSGPU_E_ARG;
        }
        // the search parameters drive loops in the kernel: only what fshost_tm_params can produce is run
        for (float f : {k.scoreD8, k.d0Std, k.d0, k.d0Search})
            if (!(f > 0.0f) || !(f <= 3.0e38f)) { ctx->err = "fsgpu_tm_batch: task " + std::to_string(t) + " has a search parameter that is not a positive finite number"; return FSGPU_E_ARG; }
        uint64_t nM = 0, nI = 0;
        const char *b = bt + k.btOff;
        for (uint32_t i = 0; i < k.btLen; i++) { nM += b[i] == 'M'; nI += b[i] == 'I'; }
        const uint64_t nT = k.btLen - nM - nI;          // every other character advances the target (TMaligner.cpp:57-69)
        if ((uint64_t) k.qStart + nM + nI > (uint64_t) queries[k.query].L || (uint64_t) k.dbStart + nM + nT > (uint64_t) k.tLen) {
            ctx->err = "fsgpu_tm_batch: the backtrace of task " + std::to_string(t) + " runs past a sequence end"; return FSGPU_E_ARG;
        }
        counts[t] = (uint32_t) nM;
        totalPairs += nM;
        if (nM > (uint64_t) kTmLdsPairs) maskWords += 3 * 2 * ((nM + 31) / 32) * 64;
    }
    // ---- staging: [query coordinates | target coordinates | backtraces | task descriptors | query descriptors]
    const size_t tcOff = up16(qFloats * 4), btOffB = up16(tcOff + tCoordsLen * 4), taskOff = up16(btOffB + btBytes),
                 qdOff = up16(taskOff + (size_t) nt * sizeof(TmTask)), inBytes = qdOff + (size_t) nq * sizeof(TmQuery);
    const size_t cntOff = up16((size_t) nt * 3 * 4), outBytes = cntOff + (size_t) nt * 4;
    int rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hTmIn, inBytes}, {ctx->hTmOut, outBytes}})) != FSGPU_OK) return rc;
    if ((rc = ensureAll(ctx, {{ctx->tmIn, inBytes}, {ctx->tmPairs, std::max<size_t>(totalPairs, 1) * 6 * 4}, {ctx->tmMasks, std::max<size_t>(maskWords, 1) * 4},
                              {ctx->tmOut, outBytes}})) != FSGPU_OK) return rc;
    if (!ctx->tmEv[0]) for (int i = 0; i < 3; i++) HIPCHK(hipEventCreate(&ctx->tmEv[i]));
    unsigned char *hb = (unsigned char *) ctx->hTmIn.p;
    TmQuery *hq = (TmQuery *) (hb + qdOff);
    {
        size_t off = 0;
        for (int i = 0; i < nq; i++) {
            const size_t L = (size_t) queries[i].L;
            memcpy(hb + off * 4, queries[i].ca, 3 * L * 4);
            hq[i].cOff = (uint32_t) off; hq[i].L = (uint32_t) L;
            off += 3 * L;
        }
    }
    if (tCoordsLen) memcpy(hb + tcOff, tCoords, tCoordsLen * 4);
    if (btBytes) memcpy(hb + btOffB, bt, btBytes);
    TmTask *ht = (TmTask *) (hb + taskOff);
    {
        uint64_t pair = 0, mask = 0;
        for (int t = 0; t < nt; t++) {
            const fsgpu_tm_task &k = tasks[t];
            TmTask &d = ht[t];
            d.query = k.query; d.tLen = (uint32_t) k.tLen; d.tOff = k.tOff; d.qStart = k.qStart; d.dbStart = k.dbStart; d.btOff = k.btOff; d.btLen = k.btLen;
            d.nPairs = counts[t]; d.pairOff = pair * 6; d.maskOff = mask; d.slot = (uint32_t) t; d.scoreD8 = k.scoreD8;
            d.d0[0] = k.d0Std; d.d0Search[0] = k.d0Std; d.d0[1] = k.d0; d.d0Search[1] = k.d0Search; d.pad = 0;
            pair += counts[t];
            if (counts[t] > (uint32_t) kTmLdsPairs) mask += 3 * 2 * (uint64_t) ((counts[t] + 31) / 32) * 64;
        }
    }
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->tmIn.p, hb, inBytes, hipMemcpyHostToDevice, st));
    TmArgs a;
    const unsigned char *db = (const unsigned char *) ctx->tmIn.p;
    a.queries = (const TmQuery *) (db + qdOff); a.tasks = (const TmTask *) (db + taskOff);
    a.qc = (const float *) db; a.tc = (const float *) (db + tcOff); a.bt = (const char *) (db + btOffB);
    a.pairs = (float *) ctx->tmPairs.p; a.masks = (uint32_t *) ctx->tmMasks.p; a.out = (float *) ctx->tmOut.p;
    a.nPairs = (int32_t *) ((char *) ctx->tmOut.p + cntOff); a.nt = (uint32_t) nt;
    HIPCHK(hipEventRecord(ctx->tmEv[0], st));
    hipLaunchKernelGGL(k_tm_pairs, dim3((unsigned) nt), dim3(kTmPairsBlock), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->tmEv[1], st));
    hipLaunchKernelGGL(k_tm_search, dim3((unsigned) nt, 3), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->tmEv[2], st));
    HIPCHK(hipMemcpyAsync(ctx->hTmOut.p, ctx->tmOut.p, outBytes, hipMemcpyDeviceToHost, st));
    if ((rc = syncStream(ctx)) != FSGPU_OK) return rc;
    for (int i = 0; i < 2; i++) {
        float ms = -1;
        if (hipEventElapsedTime(&ms, ctx->tmEv[i], ctx->tmEv[i + 1]) != hipSuccess) { ms = -1; (void) hipGetLastError(); }
        ctx->tmMs[i] = ms;
    }
    const float *ho = (const float *) ctx->hTmOut.p;
    const int32_t *hn = (const int32_t *) ((const char *) ctx->hTmOut.p + cntOff);
    for (int t = 0; t < nt; t++) {
        if (hn[t] != (int32_t) counts[t]) { ctx->err = "fsgpu_tm_batch: the device counted " + std::to_string(hn[t]) + " pairs for task " + std::to_string(t) + ", the host " + std::to_string(counts[t]); return FSGPU_E_HIP; }
        nPairs[t] = hn[t];
        scores[t] = ho[t]; scores[(size_t) nt + t] = ho[(size_t) nt + t]; rmsd[t] = ho[2 * (size_t) nt + t];
    }
    return FSGPU_OK;
}

// The same call with the superposition kept, and the exact search.  Three kernels: the pairs, the searches over a host-made list of (task, block of
// starts), the reduction of every task's partials.
extern "C" int fsgpu_tm_superpose_batch(fsgpu_ctx *ctx, const fsgpu_lddt_query *queries, int nq, const fsgpu_tm_task *tasks, int nt, const float *tCoords,
                                        uint64_t tCoordsLen, const char *bt, uint64_t btBytes, int exact, fsgpu_tm_result *out) {
    if (!ctx || nq < 0 || nt < 0 || (exact != 0 && exact != 1) || (nt > 0 && (!queries || !tasks || !out || nq == 0))) return FSGPU_E_ARG;
    if (nt == 0) return FSGPU_OK;
    if (nq > 65535) { ctx->err = "fsgpu_tm_superpose_batch: at most 65535 queries per call"; return FSGPU_E_ARG; }
    if ((tCoordsLen > 0 && !tCoords) || (btBytes > 0 && !bt)) { ctx->err = "fsgpu_tm_superpose_batch: null buffer"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    size_t qFloats = 0;
    for (int i = 0; i < nq; i++) {
        if (queries[i].L <= 0 || queries[i].L > FSGPU_MAX_SEQ_LEN || !queries[i].ca) { ctx->err = "fsgpu_tm_superpose_batch: bad query"; return FSGPU_E_ARG; }
        qFloats += 3 * (size_t) queries[i].L;
    }
    if (qFloats >= (1ull << 32) || tCoordsLen >= (1ull << 40) || btBytes >= (1ull << 40)) { ctx->err = "fsgpu_tm_superpose_batch: batch too large"; return FSGPU_E_NOMEM; }
    std::vector<uint32_t> &counts = ctx->tmCounts;
    counts.resize(nt);
    std::vector<uint32_t> blocks(nt);
    size_t totalPairs = 0, maskWords = 0, totalParts = 0, totalWork = 0;
    for (int t = 0; t < nt; t++) {
        const fsgpu_tm_task &k = tasks[t];
        if (k.query >= (uint32_t) nq || k.tLen <= 0 || k.tLen > FSGPU_MAX_SEQ_LEN || k.qStart < 0 || k.dbStart < 0 || k.tOff > tCoordsLen ||
            3 * (uint64_t) k.tLen > tCoordsLen - k.tOff || k.btOff > btBytes || k.btLen > btBytes - k.btOff) {
            ctx->err = "fsgpu_tm_superpose_batch: task " + std::to_string(t) + " out of range"; return FSGPU_E_ARG;
        }
        // exact: the d0Std field carries Lnorm, the divisor of score_fun8, which is 0 for a one-column alignment (the score is then INF, as the reference's)
        for (float f : {k.scoreD8, exact ? 1.0f : k.d0Std, k.d0, k.d0Search})
            if (!(f > 0.0f) || !(f <= 3.0e38f)) { ctx->err = "fsgpu_tm_superpose_batch: task " + std::to_string(t) + " has a search parameter that is not a positive finite number"; return FSGPU_E_ARG; }
        if (exact && (!(k.d0Std >= 0.0f) || !(k.d0Std <= 3.0e38f))) { ctx->err = "fsgpu_tm_superpose_batch: task " + std::to_string(t) + " has an Lnorm that is not a finite number >= 0"; return FSGPU_E_ARG; }
        uint64_t nM = 0, nI = 0;
        const char *b = bt + k.btOff;
        for (uint32_t i = 0; i < k.btLen; i++) { nM += b[i] == 'M'; nI += b[i] == 'I'; }
        const uint64_t nT = k.btLen - nM - nI;
        if ((uint64_t) k.qStart + nM + nI > (uint64_t) queries[k.query].L || (uint64_t) k.dbStart + nM + nT > (uint64_t) k.tLen) {
            ctx->err = "fsgpu_tm_superpose_batch: the backtrace of task " + std::to_string(t) + " runs past a sequence end"; return FSGPU_E_ARG;
        }
        counts[t] = (uint32_t) nM;
        totalPairs += nM;
        uint32_t nb = 0;
        if (nM > 0) {
            nb = 2;
            if (exact) {
                uint32_t len[6], starts[6], total = 0;
                const int cnt = tmFragments((uint32_t) nM, len, starts, 1u);
                for (int i = 0; i < cnt; i++) total += starts[i];
                nb = (total + kTmSpBlock - 1) / kTmSpBlock;
            }
            totalParts += nb + 1; totalWork += nb + 1;
            if (nM > (uint64_t) kTmLdsPairs) maskWords += (size_t) (nb + 1) * kTmSpWaves * 2 * ((nM + 31) / 32) * 64;
        }
        blocks[t] = nb;
    }
    if (maskWords >= (1ull << 31) || totalWork >= (1ull << 31)) { ctx->err = "fsgpu_tm_superpose_batch: the mask workspace of this call would exceed 8 GB; split the call"; return FSGPU_E_NOMEM; }
    // ---- staging: [query coordinates | target coordinates | backtraces | task descriptors | query descriptors | per-task extras | work list]
    const size_t tcOff = up16(qFloats * 4), btOffB = up16(tcOff + tCoordsLen * 4), taskOff = up16(btOffB + btBytes),
                 qdOff = up16(taskOff + (size_t) nt * sizeof(TmTask)), spOff = up16(qdOff + (size_t) nq * sizeof(TmQuery)),
                 wkOff = up16(spOff + (size_t) nt * sizeof(TmSpTask)), inBytes = wkOff + std::max<size_t>(totalWork, 1) * sizeof(TmSpWork);
    const size_t cntOff = up16((size_t) nt * sizeof(TmSpOut)), outBytes = cntOff + (size_t) nt * 4;
    int rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hTmIn, inBytes}, {ctx->hTmOut, outBytes}})) != FSGPU_OK) return rc;
    if ((rc = ensureAll(ctx, {{ctx->tmIn, inBytes}, {ctx->tmPairs, std::max<size_t>(totalPairs, 1) * 6 * 4}, {ctx->tmMasks, std::max<size_t>(maskWords, 1) * 4},
                              {ctx->tmParts, std::max<size_t>(totalParts, 1) * sizeof(TmPartial)}, {ctx->tmOut, outBytes}})) != FSGPU_OK) return rc;
    if (!ctx->tmSpEv[0]) for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ctx->tmSpEv[i]));
    unsigned char *hb = (unsigned char *) ctx->hTmIn.p;
    TmQuery *hq = (TmQuery *) (hb + qdOff);
    {
        size_t off = 0;
        for (int i = 0; i < nq; i++) {
            const size_t L = (size_t) queries[i].L;
            memcpy(hb + off * 4, queries[i].ca, 3 * L * 4);
            hq[i].cOff = (uint32_t) off; hq[i].L = (uint32_t) L;
            off += 3 * L;
        }
    }
    if (tCoordsLen) memcpy(hb + tcOff, tCoords, tCoordsLen * 4);
    if (btBytes) memcpy(hb + btOffB, bt, btBytes);
    TmTask *ht = (TmTask *) (hb + taskOff);
    TmSpTask *hs = (TmSpTask *) (hb + spOff);
    TmSpWork *hw = (TmSpWork *) (hb + wkOff);
    {
        uint64_t pair = 0, mask = 0, part = 0, work = 0;
        for (int t = 0; t < nt; t++) {
            const fsgpu_tm_task &k = tasks[t];
            TmTask &d = ht[t];
            d.query = k.query; d.tLen = (uint32_t) k.tLen; d.tOff = k.tOff; d.qStart = k.qStart; d.dbStart = k.dbStart; d.btOff = k.btOff; d.btLen = k.btLen;
            d.nPairs = counts[t]; d.pairOff = pair * 6; d.maskOff = 0; d.slot = (uint32_t) t; d.scoreD8 = k.scoreD8; d.pad = 0;
            // exact: both parameter slots hold parameter_set4final's d0 / d0_search (the kernel reads slot 1)
            d.d0[0] = exact ? k.d0 : k.d0Std; d.d0Search[0] = exact ? k.d0Search : k.d0Std; d.d0[1] = k.d0; d.d0Search[1] = k.d0Search;
            TmSpTask &s = hs[t];
            s.partOff = part; s.maskOff = mask; s.nBlocks = blocks[t]; s.lnorm = exact ? k.d0Std : 0.0f; s.pad[0] = s.pad[1] = 0;
            pair += counts[t];
            if (counts[t] > 0) {
                for (uint32_t b = 0; b <= blocks[t]; b++) { hw[work].task = (uint32_t) t; hw[work].block = b; work++; }
                part += blocks[t] + 1;
                if (counts[t] > (uint32_t) kTmLdsPairs) mask += (uint64_t) (blocks[t] + 1) * kTmSpWaves * 2 * ((counts[t] + 31) / 32) * 64;
            }
        }
    }
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->tmIn.p, hb, inBytes, hipMemcpyHostToDevice, st));
    TmSpArgs a;
    const unsigned char *db = (const unsigned char *) ctx->tmIn.p;
    a.base.queries = (const TmQuery *) (db + qdOff); a.base.tasks = (const TmTask *) (db + taskOff);
    a.base.qc = (const float *) db; a.base.tc = (const float *) (db + tcOff); a.base.bt = (const char *) (db + btOffB);
    a.base.pairs = (float *) ctx->tmPairs.p; a.base.masks = (uint32_t *) ctx->tmMasks.p; a.base.out = nullptr;
    a.base.nPairs = (int32_t *) ((char *) ctx->tmOut.p + cntOff); a.base.nt = (uint32_t) nt;
    a.sp = (const TmSpTask *) (db + spOff); a.work = (const TmSpWork *) (db + wkOff);
    a.parts = (TmPartial *) ctx->tmParts.p; a.res = (TmSpOut *) ctx->tmOut.p; a.exact = exact ? 1u : 0u;
    HIPCHK(hipEventRecord(ctx->tmSpEv[0], st));
    hipLaunchKernelGGL(k_tm_pairs, dim3((unsigned) nt), dim3(kTmPairsBlock), 0, st, a.base);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->tmSpEv[1], st));
    if (totalWork) {
        if (exact) hipLaunchKernelGGL(k_tm_sp_search<kTmSpWaves>, dim3((unsigned) totalWork), dim3(64 * kTmSpWaves), 0, st, a);
        else hipLaunchKernelGGL(k_tm_sp_search<kTmSpApproxWaves>, dim3((unsigned) totalWork), dim3(64 * kTmSpApproxWaves), 0, st, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ctx->tmSpEv[2], st));
    hipLaunchKernelGGL(k_tm_sp_finish, dim3((unsigned) nt), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->tmSpEv[3], st));
    HIPCHK(hipMemcpyAsync(ctx->hTmOut.p, ctx->tmOut.p, outBytes, hipMemcpyDeviceToHost, st));
    if ((rc = syncStream(ctx)) != FSGPU_OK) return rc;
    for (int i = 0; i < 3; i++) {
        float ms = -1;
        if (hipEventElapsedTime(&ms, ctx->tmSpEv[i], ctx->tmSpEv[i + 1]) != hipSuccess) { ms = -1; (void) hipGetLastError(); }
        ctx->tmSpMs[i] = ms;
    }
    const TmSpOut *ho = (const TmSpOut *) ctx->hTmOut.p;
    const int32_t *hn = (const int32_t *) ((const char *) ctx->hTmOut.p + cntOff);
    for (int t = 0; t < nt; t++) {
        if (hn[t] != (int32_t) counts[t]) { ctx->err = "fsgpu_tm_superpose_batch: the device counted " + std::to_string(hn[t]) + " pairs for task " + std::to_string(t) + ", the host " + std::to_string(counts[t]); return FSGPU_E_HIP; }
        fsgpu_tm_result &r = out[t];
        r.nPairs = hn[t]; r.source = (int32_t) ho[t].source; r.score[0] = ho[t].score[0]; r.score[1] = ho[t].score[1]; r.rms = ho[t].rms;
        memcpy(r.t, ho[t].t, sizeof(r.t)); memcpy(r.u, ho[t].u, sizeof(r.u));
    }
    return FSGPU_OK;
}

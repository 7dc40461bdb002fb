// fsgpu.hip -- C ABI (include/fsgpu.h): the context's life cycle, accessors and timers.  Host side: HIP runtime only, no torch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <string>

#include "fsgpu_ctx.h"

static thread_local std::string g_createError;

extern "C" {

// devices with at least one live context in this process (fsgpu_live_devices: the host side divides the process's cores by it)
static std::mutex g_liveM;
static int g_liveCtx[64] = {0};
static void liveAdd(int device, int d) { std::lock_guard<std::mutex> g(g_liveM); if (device >= 0 && device < 64) g_liveCtx[device] += d; }
int fsgpu_live_devices(void) {
    std::lock_guard<std::mutex> g(g_liveM);
    int n = 0;
    for (int i = 0; i < 64; i++) if (g_liveCtx[i] > 0) n++;
    return n;
}

int fsgpu_create(int device, fsgpu_ctx **out) {
    if (!out) return FSGPU_E_ARG;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_createError = std::string("no HIP device available: ") + hipGetErrorString(e);
        return FSGPU_E_HIP;
    }
    if (device < 0 || device >= count) { g_createError = "device index out of range"; return FSGPU_E_ARG; }
    fsgpu_ctx *ctx = new fsgpu_ctx();
    ctx->device = device;
    auto fail = [&](const char *what, hipError_t err) {
        g_createError = std::string(what) + ": " + hipGetErrorString(err);
        delete ctx;
        return FSGPU_E_HIP;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail("hipGetDeviceProperties", e);
    ctx->numCU = prop.multiProcessorCount;
    if (const char *e2 = getenv("FSGPU_GAPLESS_BLOCKS_PER_CU")) ctx->gaplessBlocksPerCU = std::max(1, atoi(e2));
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    // the batch SW of a context runs on a stream of the highest priority: its launches are short and a host thread waits for them, while the
    // scans and k-mer batches of the other contexts would otherwise keep them queueing (no priority range or no such stream: the context's stream)
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi < lo) {
        if (hipStreamCreateWithPriority(&ctx->swHi, hipStreamNonBlocking, hi) != hipSuccess) { ctx->swHi = nullptr; (void) hipGetLastError(); }
        ctx->swHiPrio = hi;
    }
    for (int i = 0; i < 4; i++)
        if ((e = hipEventCreate(&ctx->ev[i])) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipMalloc((void **) &ctx->dMeta, sizeof(SelMeta))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc((void **) &ctx->queue, 256)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipHostMalloc((void **) &ctx->hMeta, sizeof(SelMeta))) != hipSuccess) return fail("hipHostMalloc", e);
    liveAdd(device, +1);
    *out = ctx;
    return FSGPU_OK;
}

int fsgpu_clone(const fsgpu_ctx *src, fsgpu_ctx **out) {
    if (!src || !out) return FSGPU_E_ARG;
    int rc = fsgpu_create(src->device, out);
    if (rc != FSGPU_OK) return rc;
    (*out)->db = src->db;
    (*out)->kidx = src->kidx;
    return FSGPU_OK;
}

void fsgpu_destroy(fsgpu_ctx *ctx) {
    if (!ctx) return;
    liveAdd(ctx->device, -1);
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->swLong) (void) hipStreamSynchronize(ctx->swLong);
    if (ctx->swHi) (void) hipStreamSynchronize(ctx->swHi);          // the k_sw3 path runs here and on swAux: nothing may be in flight when its buffers go
    for (int i = 0; i < fsgpu_ctx::kSwAux; i++) if (ctx->swAux[i]) (void) hipStreamSynchronize(ctx->swAux[i]);
    freeDb(ctx);                                                    // leaves the DbStore's chain of scan events before the event goes
    if (ctx->scanDoneEv) (void) hipEventDestroy(ctx->scanDoneEv);
    if (ctx->kmer) fsgpu_kmer_free_scratch(ctx->kmer);
    DevBuf *bufs[] = {&ctx->gBorder0, &ctx->gBorder1, &ctx->scoreAcc, &ctx->pssm, &ctx->scores, &ctx->chunkHist, &ctx->baseGt, &ctx->baseTie, &ctx->outId, &ctx->outScore,
                      &ctx->img, &ctx->tids, &ctx->res0, &ctx->res1, &ctx->border0, &ctx->border1, &ctx->keys, &ctx->lbuf, &ctx->lres,
                      &ctx->ovAA, &ctx->ovSS, &ctx->ovOff, &ctx->ovLen, &ctx->s3img, &ctx->s3pass, &ctx->s3build, &ctx->s3res,
                      &ctx->btSeq, &ctx->btTrace, &ctx->btBlocks, &ctx->btOut, &ctx->btIn, &ctx->pbtIn, &ctx->pbtTasks, &ctx->pbtState, &ctx->pbtDir, &ctx->pbtOut, &ctx->ldIn, &ctx->ldNorm, &ctx->ldCols, &ctx->ldOut,
                      &ctx->tmIn, &ctx->tmPairs, &ctx->tmMasks, &ctx->tmOut, &ctx->tmParts,
                      &ctx->mqPssm, &ctx->mqScores, &ctx->mqQueues, &ctx->mqRec, &ctx->mqHist, &ctx->mqBaseGt, &ctx->mqBaseTie, &ctx->mqMeta,
                      &ctx->mqOutId, &ctx->mqOutScore, &ctx->mqIdent, &ctx->scanCnt, &ctx->scanMeta, &ctx->scanOut};
    for (DevBuf *b : bufs) if (b->p) hipFree(b->p);
    hipFree(ctx->dMeta); hipFree(ctx->queue);
    hipHostFree(ctx->hMeta); hipHostFree(ctx->hOutId.p); hipHostFree(ctx->hOutScore.p);
    hipHostFree(ctx->hRes0.p); hipHostFree(ctx->hRes1.p); hipHostFree(ctx->hLbuf.p); hipHostFree(ctx->hLres.p);
    hipHostFree(ctx->hS3pass.p); hipHostFree(ctx->hS3build.p); hipHostFree(ctx->hS3res.p);
    hipHostFree(ctx->hBtIn.p); hipHostFree(ctx->hBtOut.p); hipHostFree(ctx->hLdIn.p); hipHostFree(ctx->hLdOut.p);
    hipHostFree(ctx->hTmIn.p); hipHostFree(ctx->hTmOut.p);
    hipHostFree(ctx->hPbtIn.p); hipHostFree(ctx->hPbtTasks.p); hipHostFree(ctx->hPbtOut.p);
    for (int i = 0; i < 2; i++) if (ctx->pbtEv[i]) (void) hipEventDestroy(ctx->pbtEv[i]);
    hipHostFree(ctx->hScanMeta.p); hipHostFree(ctx->hScanOut.p);
    for (int i = 0; i < 4; i++) if (ctx->scanEv[i]) (void) hipEventDestroy(ctx->scanEv[i]);
    for (int i = 0; i < 3; i++) if (ctx->tmEv[i]) (void) hipEventDestroy(ctx->tmEv[i]);
    for (int i = 0; i < 4; i++) if (ctx->tmSpEv[i]) (void) hipEventDestroy(ctx->tmSpEv[i]);
    for (int i = 0; i < 3; i++) if (ctx->ldEv[i]) (void) hipEventDestroy(ctx->ldEv[i]);
    if (ctx->swLong) (void) hipStreamDestroy(ctx->swLong);
    if (ctx->swHi) (void) hipStreamDestroy(ctx->swHi);
    hipHostFree(ctx->hPssm.p); hipHostFree(ctx->hImg.p); hipHostFree(ctx->hTids.p);
    hipHostFree(ctx->hMqPssm.p); hipHostFree(ctx->hMqRec.p); hipHostFree(ctx->hMqMeta.p); hipHostFree(ctx->hMqOutId.p); hipHostFree(ctx->hMqOutScore.p); hipHostFree(ctx->hMqIdent.p);
    for (int i = 0; i < 4; i++) if (ctx->ev[i]) hipEventDestroy(ctx->ev[i]);
    for (int i = 0; i < 4; i++) if (ctx->swDirEv[i]) hipEventDestroy(ctx->swDirEv[i]);
    for (int i = 0; i < fsgpu_ctx::kSwAux; i++) if (ctx->swAux[i]) (void) hipStreamDestroy(ctx->swAux[i]);
    for (int i = 0; i <= fsgpu_ctx::kSwAux; i++) if (ctx->swAuxEv[i]) (void) hipEventDestroy(ctx->swAuxEv[i]);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *fsgpu_last_error(const fsgpu_ctx *ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }
int fsgpu_device(const fsgpu_ctx *ctx) { return ctx ? ctx->device : -1; }
int fsgpu_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
void *fsgpu_stream(const fsgpu_ctx *ctx) { return ctx ? (void *) ctx->stream : nullptr; }
uint64_t fsgpu_db_size(const fsgpu_ctx *ctx) { return ctx && ctx->db ? ctx->db->n : 0; }
uint64_t fsgpu_db_residues(const fsgpu_ctx *ctx) { return ctx && ctx->db ? ctx->db->residues : 0; }

/* out[2][4]: per direction (0 forward, 1 reversed query) of the last fsgpu_sw_multi_dir calls: device ms of the pass's k_sw2 launches (HIP events
 * on the context stream, -1 when the pass did not run), DP cells, pairs, VALU wave-instructions of the DP rows (the roofline denominator) */
void fsgpu_sw_last_passes(const fsgpu_ctx *ctx, double *out) {
    for (int d = 0; d < 2; d++) {
        float ms = -1;
        if (!ctx || !ctx->swDirValid[d] || hipEventElapsedTime(&ms, ctx->swDirEv[2 * d], ctx->swDirEv[2 * d + 1]) != hipSuccess) { ms = -1; (void) hipGetLastError(); }
        out[d * 4 + 0] = ms >= 0 ? ms + (float) ctx->swDirExtraMs[d] : ms;
        out[d * 4 + 1] = ctx ? ctx->swDirCells[d] : 0; out[d * 4 + 2] = ctx ? ctx->swDirPairs[d] : 0; out[d * 4 + 3] = ctx ? ctx->swDirWaveSteps[d] : 0;
    }
}

void fsgpu_history_counters(const fsgpu_ctx *ctx, uint64_t *out8) {
    for (int i = 0; i < 8; i++) out8[i] = 0;
    if (!ctx) return;
    out8[0] = ctx->kmerForm[0]; out8[1] = ctx->kmerForm[1]; out8[2] = ctx->kmerBatches; out8[3] = ctx->kmerLastBatchQueries;
    out8[4] = ctx->swLongLaunched; out8[5] = ctx->swLongReused; out8[6] = ctx->ldNormRuns; out8[7] = ctx->kmerFirstBatchQueries;
}

double fsgpu_last_kernel_ms(const fsgpu_ctx *ctx, int which) {
    if (ctx && which >= 2 && which < 14) return ctx->kmerMs[which - 2];
    if (ctx && (which == 14 || which == 15)) return ctx->ldMs[which - 14];
    if (ctx && (which == 16 || which == 17)) return ctx->tmMs[which - 16];
    if (ctx && which >= 18 && which <= 20) return ctx->tmSpMs[which - 18];
    if (ctx && which >= 21 && which <= 23) return ctx->scanMs[which - 21];
    if (!ctx || which < 0 || which > 1 || !ctx->evValid[which]) return -1.0;
    if (which == 0 && ctx->mqScanMs >= 0) return ctx->mqScanMs;      // a multi-query call with row-tiled queries: all of its scans
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev[2 * which], ctx->ev[2 * which + 1]) != hipSuccess) return -1.0;
    return (double) ms;
}

} // extern "C"

// fsgpu_pbtrace.hip -- C ABI of the profile-query start cell + banded trace-back on the device (include/fsgpu.h: fsgpu_profile_backtrace; kernels:
// k_pbtrace.hpp).  One call = the accepted hits of one profile alignment batch.  The reverse pass of every task runs first (one launch; more only when
// prefixes beyond the LDS line need more global line state than the budget holds), its start cells come back to the host, which sizes the direction slices
// from them; the banded pass then runs in as many launches as the byte budget asks for.  A task whose band has to grow beyond its slice comes back with
// the width it needs and joins the next launch, starting at that width (the widths before it are known to fail).  No CPU fallback in here.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_pbtrace.hpp"

namespace {
inline size_t up256(size_t x) { return (x + 255) & ~(size_t) 255; }
// bytes of global line state a line of `cells` cells needs (none up to the LDS line)
inline size_t stateBytes(int cells) { return cells <= kPbtLdsCells ? 0 : up256((size_t) cells * sizeof(int2)); }
inline size_t dirBytes(int qLen, int dbLen, long long band) { return up256((size_t) qLen * (size_t) std::min<long long>(2 * band + 1, dbLen)); }
struct PbtDrain {
    hipStream_t st; bool armed = false;
    ~PbtDrain() { if (armed) { (void) hipStreamSynchronize(st); (void) hipGetLastError(); } }
};
}

extern "C" void fsgpu_profile_backtrace_last(const fsgpu_ctx *ctx, double *out8) {
    if (!out8) return;
    for (int i = 0; i < 8; i++) out8[i] = ctx ? ctx->pbtLast[i] : 0.0;
}

extern "C" int fsgpu_profile_backtrace(fsgpu_ctx *ctx, const fsgpu_pbt_query *queries, int nq, const fsgpu_bt_task *tasks, int nt,
                                       int gapOpen, int gapExtend, fsgpu_bt_res *res, const char **btBase) {
    if (!ctx || nq < 0 || nt < 0 || (nt > 0 && (!queries || !tasks || !res || !btBase))) return FSGPU_E_ARG;
    if (btBase) *btBase = nullptr;
    for (double &v : ctx->pbtLast) v = 0.0;
    if (nt == 0) return FSGPU_OK;
    if (!ctx->db || ctx->db->n == 0) { ctx->err = "no database loaded"; return FSGPU_E_NODB; }
    if (!ctx->db->hasAA) { ctx->err = "fsgpu_profile_backtrace: the database was loaded without AA sequences"; return FSGPU_E_NODB; }
    if (!(gapOpen > gapExtend && gapExtend >= 1)) { ctx->err = "fsgpu_profile_backtrace: gap costs must satisfy gapOpen > gapExtend >= 1"; return FSGPU_E_ARG; }
    if (gapOpen >= 32768) { ctx->err = "fsgpu_profile_backtrace: gapOpen must be below 32768"; return FSGPU_E_UNSUPPORTED; }
    // ---- query blob: [pAA 21 L][p3Di 21 L][lettersAA L] per query ----
    std::vector<PbtQuery> hq(nq);
    size_t qBytes = 0;
    for (int i = 0; i < nq; i++) {
        if (queries[i].L <= 0 || queries[i].L > FSGPU_MAX_SEQ_LEN || !queries[i].pAA || !queries[i].p3Di || !queries[i].lettersAA) { ctx->err = "fsgpu_profile_backtrace: bad query"; return FSGPU_E_ARG; }
        hq[i].off = qBytes; hq[i].L = queries[i].L; hq[i].pad = 0;
        qBytes += up256((size_t) queries[i].L * 43);
    }
    const std::vector<int32_t> &len = ctx->db->hLengths;
    size_t btBytes = 0;
    std::vector<uint64_t> btOff(nt);
    for (int t = 0; t < nt; t++) {
        const fsgpu_bt_task &k = tasks[t];
        if (k.query >= (uint32_t) nq || k.target >= ctx->db->n || k.qEnd < 0 || k.qEnd >= queries[k.query].L || k.dbEnd < 0 || k.dbEnd >= len[k.target]) {
            ctx->err = "fsgpu_profile_backtrace: task out of range (task " + std::to_string(t) + ": ids and an end cell inside the query and the target; a target without residues has none)"; return FSGPU_E_ARG;
        }
        btOff[t] = btBytes;
        btBytes += up256((size_t) k.qEnd + (size_t) k.dbEnd + 2 + 16);
    }
    const size_t budget = [] { const char *e = getenv("FSGPU_PBT_BYTES"); const long long v = e && *e ? atoll(e) : 0; return v > 0 ? (size_t) v : (size_t) 256 << 20; }();   // per call: the tests switch it
    for (int t = 0; t < nt; t++) { res[t].status = 0; res[t].qStart = -1; res[t].dbStart = -1; res[t].identicalAA = 0; res[t].btLen = 0; res[t].blockSizes = 0; res[t].btOff = btOff[t]; }
    HIPCHK(hipSetDevice(ctx->device));
    if (!ctx->pbtEv[0]) for (int i = 0; i < 2; i++) HIPCHK(hipEventCreate(&ctx->pbtEv[i]));
    int rc;
    const size_t qdOff = qBytes, inBytes = qdOff + (size_t) nq * sizeof(PbtQuery), outBytes = btBytes + (size_t) nt * sizeof(PbtRes);
    if ((rc = ensureAll(ctx, {{ctx->pbtIn, inBytes}, {ctx->pbtTasks, (size_t) nt * sizeof(PbtTask)}, {ctx->pbtOut, outBytes}})) != FSGPU_OK) return rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hPbtIn, inBytes}, {ctx->hPbtTasks, (size_t) nt * sizeof(PbtTask)}, {ctx->hPbtOut, outBytes}})) != FSGPU_OK) return rc;
    unsigned char *hb = (unsigned char *) ctx->hPbtIn.p;
    for (int i = 0; i < nq; i++) {
        unsigned char *d = hb + hq[i].off;
        const size_t L = (size_t) queries[i].L;
        memcpy(d, queries[i].pAA, 21 * L); memcpy(d + 21 * L, queries[i].p3Di, 21 * L); memcpy(d + 42 * L, queries[i].lettersAA, L);
    }
    memcpy(hb + qdOff, hq.data(), (size_t) nq * sizeof(PbtQuery));
    hipStream_t st = ctx->stream;
    PbtDrain drain{st};
    drain.armed = true;
    HIPCHK(hipMemcpyAsync(ctx->pbtIn.p, hb, inBytes, hipMemcpyHostToDevice, st));
    PbtArgs a;
    a.queries = (const PbtQuery *) ((const unsigned char *) ctx->pbtIn.p + qdOff); a.qdata = (const int8_t *) ctx->pbtIn.p;
    a.dbAA = ctx->db->alnAA; a.dbSS = ctx->db->aln3di; a.dbOff = ctx->db->dOffsets;
    a.gapOpen = gapOpen; a.gapExtend = gapExtend;
    a.bt = (char *) ctx->pbtOut.p; a.res = (PbtRes *) ((char *) ctx->pbtOut.p + btBytes);
    PbtTask *ht = (PbtTask *) ctx->hPbtTasks.p;
    const PbtRes *hr = (const PbtRes *) ((const char *) ctx->hPbtOut.p + btBytes);
    double ms = 0, launches = 0, bandLaunches = 0;
    size_t scratchMax = 0;
    // one launch over ht[0 .. n): upload the tasks, run, bring the result records back
    auto launch = [&](int n, bool bandPass, size_t stBytes, size_t dBytes) -> int {
        int rc2;
        if ((rc2 = ensureAll(ctx, {{ctx->pbtState, std::max<size_t>(stBytes, 256)}, {ctx->pbtDir, std::max<size_t>(dBytes, 256)}})) != FSGPU_OK) return rc2;
        a.tasks = (const PbtTask *) ctx->pbtTasks.p; a.nTasks = n;
        a.state = (int2 *) ctx->pbtState.p; a.dir = (uint8_t *) ctx->pbtDir.p;
        HIPCHK(hipMemcpyAsync(ctx->pbtTasks.p, ht, (size_t) n * sizeof(PbtTask), hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(ctx->pbtEv[0], st));
        const unsigned grid = (unsigned) ((n + kPbtWaves - 1) / kPbtWaves);
        if (bandPass) hipLaunchKernelGGL(k_pbt_band, dim3(grid), dim3(kPbtWaves * 64), 0, st, a);
        else hipLaunchKernelGGL(k_pbt_reverse, dim3(grid), dim3(kPbtWaves * 64), 0, st, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ctx->pbtEv[1], st));
        HIPCHK(hipMemcpyAsync((char *) ctx->hPbtOut.p + btBytes, a.res, (size_t) nt * sizeof(PbtRes), hipMemcpyDeviceToHost, st));
        if ((rc2 = syncStream(ctx)) != FSGPU_OK) return rc2;
        float m = 0;
        if (hipEventElapsedTime(&m, ctx->pbtEv[0], ctx->pbtEv[1]) == hipSuccess) ms += m; else (void) hipGetLastError();
        launches += 1; bandLaunches += bandPass ? 1 : 0;
        scratchMax = std::max(scratchMax, stBytes + dBytes);
        return FSGPU_OK;
    };
    // ---- the reverse pass: largest prefix rectangle first (the waves of a workgroup finish together) ----
    std::vector<int> order(nt);
    for (int t = 0; t < nt; t++) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
        return ((int64_t) tasks[x].qEnd + 1) * ((int64_t) tasks[x].dbEnd + 1) > ((int64_t) tasks[y].qEnd + 1) * ((int64_t) tasks[y].dbEnd + 1);
    });
    std::vector<int> started;                  // tasks whose reverse pass ran
    {
        int n = 0;
        size_t stBytes = 0;
        std::vector<int> group;
        auto flush = [&]() -> int {
            if (n == 0) return FSGPU_OK;
            const int rc2 = launch(n, false, stBytes, 0);
            if (rc2 != FSGPU_OK) return rc2;
            for (int t : group) {
                res[t].status = hr[t].status; res[t].qStart = hr[t].qStart; res[t].dbStart = hr[t].dbStart;
                if (hr[t].status == 1) started.push_back(t);
            }
            n = 0; stBytes = 0; group.clear();
            return FSGPU_OK;
        };
        for (int t : order) {
            const fsgpu_bt_task &k = tasks[t];
            const size_t sb = stateBytes(k.qEnd + 1);
            if (sb > budget) continue;         // status 0: the line state of this prefix alone exceeds the budget
            if (n > 0 && stBytes + sb > budget && (rc = flush()) != FSGPU_OK) return rc;
            PbtTask &d = ht[n++];
            memset(&d, 0, sizeof(d));
            d.query = k.query; d.target = k.target; d.qEnd = k.qEnd; d.dbEnd = k.dbEnd; d.score = k.score; d.slot = t;
            d.stateOff = stBytes / sizeof(int2); d.btOff = btOff[t];
            stBytes += sb;
            group.push_back(t);
        }
        if ((rc = flush()) != FSGPU_OK) return rc;
    }
    // ---- the banded pass ----
    struct Pending { int t; long long band; };
    std::vector<Pending> pending;
    for (int t : started) {
        const int qLen = tasks[t].qEnd - res[t].qStart + 1, dbLen = tasks[t].dbEnd - res[t].dbStart + 1;
        pending.push_back({t, (long long) std::abs(dbLen - qLen) + 1});
        res[t].status = 0;                     // until the banded pass answers
    }
    while (!pending.empty()) {
        std::vector<Pending> next;
        int n = 0;
        size_t stBytes = 0, dBytes = 0;
        std::vector<int> group;
        auto flush = [&]() -> int {
            if (n == 0) return FSGPU_OK;
            const int rc2 = launch(n, true, stBytes, dBytes);
            if (rc2 != FSGPU_OK) return rc2;
            for (int t : group) {
                const PbtRes &r = hr[t];
                if (r.status == 0) { next.push_back({t, (long long) r.band}); continue; }
                res[t].status = r.status; res[t].blockSizes = r.band;
                if (r.status == 1) { res[t].identicalAA = r.identicalAA; res[t].btLen = r.btLen; res[t].btOff = btOff[t] + (uint64_t) r.btStart; }
            }
            n = 0; stBytes = 0; dBytes = 0; group.clear();
            return FSGPU_OK;
        };
        // widest rectangle first
        std::stable_sort(pending.begin(), pending.end(), [&](const Pending &x, const Pending &y) {
            return (int64_t) (tasks[x.t].qEnd - res[x.t].qStart) * (tasks[x.t].dbEnd - res[x.t].dbStart) > (int64_t) (tasks[y.t].qEnd - res[y.t].qStart) * (tasks[y.t].dbEnd - res[y.t].dbStart);
        });
        for (const Pending &p : pending) {
            const fsgpu_bt_task &k = tasks[p.t];
            const int qLen = k.qEnd - res[p.t].qStart + 1, dbLen = k.dbEnd - res[p.t].dbStart + 1;
            const size_t sb = stateBytes(dbLen);
            if (sb + dirBytes(qLen, dbLen, p.band) > budget) { res[p.t].blockSizes = (int32_t) p.band; continue; }   // status 0: does not fit at the band it needs
            // room for two more doublings where the budget has it
            long long cap = p.band * 4;
            while (cap > p.band && sb + dirBytes(qLen, dbLen, cap) > budget) cap /= 2;
            const size_t db = dirBytes(qLen, dbLen, cap);
            if (n > 0 && stBytes + dBytes + sb + db > budget && (rc = flush()) != FSGPU_OK) return rc;
            PbtTask &d = ht[n++];
            memset(&d, 0, sizeof(d));
            d.query = k.query; d.target = k.target; d.qEnd = k.qEnd; d.dbEnd = k.dbEnd; d.score = k.score; d.slot = p.t;
            d.qStart = res[p.t].qStart; d.dbStart = res[p.t].dbStart;
            d.band = (int32_t) p.band; d.bandCap = 2 * cap + 1 >= dbLen ? INT_MAX / 2 : (int32_t) cap;
            d.stateOff = stBytes / sizeof(int2); d.dirOff = dBytes; d.btOff = btOff[p.t];
            stBytes += sb; dBytes += db;
            group.push_back(p.t);
        }
        if ((rc = flush()) != FSGPU_OK) return rc;
        pending.swap(next);
    }
    HIPCHK(hipMemcpyAsync(ctx->hPbtOut.p, ctx->pbtOut.p, btBytes, hipMemcpyDeviceToHost, st));
    if ((rc = syncStream(ctx)) != FSGPU_OK) return rc;
    drain.armed = false;
    ctx->pbtLast[0] = launches; ctx->pbtLast[5] = ms; ctx->pbtLast[6] = (double) scratchMax; ctx->pbtLast[7] = bandLaunches;
    for (int t = 0; t < nt; t++) ctx->pbtLast[1 + std::min(std::max(res[t].status, 0), 3)] += 1.0;
    *btBase = (const char *) ctx->hPbtOut.p;
    return FSGPU_OK;
}

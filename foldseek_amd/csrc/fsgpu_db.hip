// fsgpu_db.hip -- the device-resident database: re-tiling kernels, load / adopt, replication to other devices (RCCL or peer copies).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <dlfcn.h>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "fs_db_table.h"

// ------------------------------------------------------------------------------------------------------------
// database re-tiling kernels
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_db_scan_layout(const uint8_t *raw, const uint64_t *offsets, const int32_t *lengths,
                                                        uint32_t n, const uint64_t *stripeOff, const uint32_t *stripeLen,
                                                        const uint32_t *stripeTargets, uint4 *out) {
    const uint32_t stripe = blockIdx.x;
    const uint32_t len16 = stripeLen[stripe];
    const int j = threadIdx.x & 7;
    const uint32_t t = stripeTargets[stripe * kStripeTargets + j];
    const bool live = t < n;
    const uint64_t off = live ? offsets[t] : 0;
    const int L = live ? lengths[t] : 0;
    uint4 *dst = out + stripeOff[stripe];
    for (uint32_t c = threadIdx.x >> 3; c < len16; c += 32) {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; b++) {
            int col = (int) c * 16 + b;
            uint32_t code = kDeadCode;
            if (col < L) {
                code = raw[off + col];
                code = code > 20 ? 20 : code;     // soft-masked (>= 32) and anything unknown -> X
            }
            w[b >> 2] |= code << ((b & 3) * 8);
        }
        dst[(size_t) c * 8 + j] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ void k_db_unmask(const uint8_t *raw, uint8_t *out, uint64_t bytes) {
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (; i < bytes; i += stride) {
        uint8_t c = raw[i];
        c = c >= 32 ? c - 32 : c;
        out[i] = c > 20 ? 20 : c;
    }
}

// the table against the buffer before anything reads through it: FSGPU_E_ARG and a message that names the first bad entry
static int checkTable(fsgpu_ctx *ctx, const char *who, const uint64_t *offsets, const int32_t *lengths, uint64_t n, uint64_t bytes) {
    const int64_t bad = fsDbCheckTable(offsets, lengths, n, bytes);
    if (bad < 0) return FSGPU_OK;
    const char *why = "shares bytes with another entry";
    if ((uint64_t) bad == n) why = "(offsets[n], the end of the table) lies beyond the data buffer";
    else if (lengths[bad] < 0 || lengths[bad] > FSGPU_MAX_SEQ_LEN) why = "has a length outside 0 .. FSGPU_MAX_SEQ_LEN";
    else if (offsets[bad] > bytes || (uint64_t) lengths[bad] > bytes - offsets[bad]) why = "lies outside the data buffer";
    ctx->err = std::string(who) + ": entry " + std::to_string(bad) + " " + why;
    return FSGPU_E_ARG;
}

// hLen: the lengths on the host, already checked (checkTable); dOff / dLen: the same table on the device
static int buildDb(fsgpu_ctx *ctx, const uint8_t *dRaw3di, const uint8_t *dRawAA, const uint64_t *dOff, const int32_t *dLen,
                   std::vector<int32_t> &&hLen, uint64_t bytes) {
    const uint64_t n = hLen.size();
    ctx->db = std::make_shared<DbStore>();
    // host copy of the lengths drives the stripe table
    ctx->db->hLengths = std::move(hLen);
    const uint32_t nStripes = (uint32_t) ((n + kStripeTargets - 1) / kStripeTargets);
    std::vector<uint64_t> sOff(nStripes);
    std::vector<uint32_t> sLen(nStripes), sCols(nStripes);
    uint64_t total = 0, residues = 0;
    int maxLen = 0;
    // a stripe = 8 targets of similar length: group along the length-sorted order (identity for a padded DB, which
    // makepaddedseqdb has already sorted; an ASCII DB arrives in arbitrary order)
    std::vector<uint32_t> sTargets((size_t) nStripes * kStripeTargets, 0xffffffffu);
    {
        std::vector<uint32_t> byLen(n);
        std::iota(byLen.begin(), byLen.end(), 0u);
        const std::vector<int32_t> &hl = ctx->db->hLengths;
        if (!std::is_sorted(hl.begin(), hl.end())) std::stable_sort(byLen.begin(), byLen.end(), [&](uint32_t a, uint32_t b) { return hl[a] < hl[b]; });
        std::copy(byLen.begin(), byLen.end(), sTargets.begin());
    }
    for (uint32_t s = 0; s < nStripes; s++) {
        int mx = 0;
        for (uint64_t k = (uint64_t) s * 8; k < std::min<uint64_t>(n, (uint64_t) s * 8 + 8); k++) {
            const int L = ctx->db->hLengths[sTargets[k]];          // 0 .. FSGPU_MAX_SEQ_LEN: checkTable
            mx = std::max(mx, L);
            residues += (uint64_t) L;
        }
        maxLen = std::max(maxLen, mx);
        sCols[s] = (uint32_t) mx;
        sLen[s] = (uint32_t) ((mx + 15) / 16);
        sOff[s] = total;
        total += (uint64_t) sLen[s] * 8;
    }
    ctx->db->hStripeLen = sLen;
    ctx->db->hStripeCols = sCols;

    HIPCHK(hipMalloc((void **) &ctx->db->scan, std::max<uint64_t>(total, 1) * sizeof(uint4)));
    HIPCHK(hipMalloc((void **) &ctx->db->stripeOff, std::max<size_t>(nStripes, 1) * sizeof(uint64_t)));
    HIPCHK(hipMalloc((void **) &ctx->db->stripeLen, std::max<size_t>(nStripes, 1) * sizeof(uint32_t)));
    HIPCHK(hipMalloc((void **) &ctx->db->stripeTargets, std::max<size_t>(sTargets.size(), 1) * sizeof(uint32_t)));
    HIPCHK(hipMalloc((void **) &ctx->db->aln3di, std::max<uint64_t>(bytes, 1)));
    HIPCHK(hipMalloc((void **) &ctx->db->dOffsets, (n + 1) * sizeof(uint64_t)));
    HIPCHK(hipMalloc((void **) &ctx->db->dLengths, std::max<uint64_t>(n, 1) * sizeof(int32_t)));
    if (nStripes) {
        HIPCHK(hipMemcpy(ctx->db->stripeOff, sOff.data(), nStripes * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ctx->db->stripeLen, sLen.data(), nStripes * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(ctx->db->stripeTargets, sTargets.data(), sTargets.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // stream-ordered copies: a device-to-device hipMemcpy runs on the null stream and is NOT synchronous with the host, and the context's
    // stream is non-blocking, so the layout kernels below could otherwise start before their offsets / lengths have arrived (seen as an
    // intermittent memory fault when two processes time-share one device)
    HIPCHK(hipMemcpyAsync(ctx->db->dOffsets, dOff, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->db->dLengths, dLen, n * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    if (nStripes) {
        hipLaunchKernelGGL(k_db_scan_layout, dim3(nStripes), dim3(256), 0, ctx->stream, dRaw3di, ctx->db->dOffsets, ctx->db->dLengths,
                           (uint32_t) n, ctx->db->stripeOff, ctx->db->stripeLen, ctx->db->stripeTargets, ctx->db->scan);
        HIPCHK(hipGetLastError());
    }
    // a database without a single residue (bytes == 0) still owns its buffers: "no buffer" means "no database" / "no AA half" to the entries
    HIPCHK(hipMalloc((void **) &ctx->db->raw3di, std::max<uint64_t>(bytes, 1)));
    if (dRawAA) HIPCHK(hipMalloc((void **) &ctx->db->alnAA, std::max<uint64_t>(bytes, 1)));
    if (bytes) {
        HIPCHK(hipMemcpyAsync(ctx->db->raw3di, dRaw3di, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_db_unmask, dim3(2048), dim3(256), 0, ctx->stream, dRaw3di, ctx->db->aln3di, bytes);
        HIPCHK(hipGetLastError());
        if (dRawAA) {
            hipLaunchKernelGGL(k_db_unmask, dim3(2048), dim3(256), 0, ctx->stream, dRawAA, ctx->db->alnAA, bytes);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->db->scanU4 = total;
    ctx->db->n = n; ctx->db->bytes = bytes; ctx->db->residues = residues; ctx->db->nStripes = nStripes; ctx->db->maxLen = maxLen;
    ctx->db->hasAA = dRawAA != nullptr;
    return FSGPU_OK;
}

// every way out of a failed load or adopt: the context is left without a database, whatever the reason (the message of the failure is kept)
static int dropDb(fsgpu_ctx *ctx, int rc) {
    const std::string why = ctx->err;
    (void) hipStreamSynchronize(ctx->stream);
    freeDb(ctx);
    ctx->err = why;
    return rc;
}
static int dropDbHip(fsgpu_ctx *ctx, const char *what, hipError_t e) {
    ctx->err = std::string(what) + ": " + hipGetErrorString(e);
    return dropDb(ctx, FSGPU_E_HIP);
}
#define DROPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return dropDbHip(ctx, #call, e_); } while (0)

// the context lets go of its database, then takes the new one
static int replaceDb(fsgpu_ctx *ctx, const void *d3, const void *dA, const void *dOff, const void *dLen, std::vector<int32_t> &&hLen, uint64_t bytes) {
    DROPCHK(hipStreamSynchronize(ctx->stream));
    freeDb(ctx);
    int rc = buildDb(ctx, (const uint8_t *) d3, (const uint8_t *) dA, (const uint64_t *) dOff, (const int32_t *) dLen, std::move(hLen), bytes);
    if (rc != FSGPU_OK) { const std::string why = ctx->err; freeDb(ctx); ctx->err = why; }
    return rc;
}

extern "C" {

int64_t fsgpu_db_check_table(const uint64_t *offsets, const int32_t *lengths, uint64_t n, uint64_t bytes) {
    return fsDbCheckTable(offsets, lengths, n, bytes);
}

int fsgpu_db_adopt_device(fsgpu_ctx *ctx, const void *d3, const void *dA, const void *dOff, const void *dLen,
                          uint64_t n, uint64_t bytes) {
    if (!ctx) return FSGPU_E_ARG;
    DROPCHK(hipSetDevice(ctx->device));
    if (!d3 || !dOff || !dLen || n == 0 || n > 0xfffffff0ull) { ctx->err = "fsgpu_db_adopt_device: bad argument"; return dropDb(ctx, FSGPU_E_ARG); }
    // the table comes to the host before anything is freed or launched: every kernel reads data[offsets[t] + col], col < lengths[t], unguarded
    // (through one pinned block: a copy into pageable memory of this size is several times slower and varies from call to call)
    struct Pinned {
        void *p = nullptr;
        ~Pinned() { if (p) (void) hipHostFree(p); }
    } pin;
    DROPCHK(hipHostMalloc(&pin.p, (n + 1) * sizeof(uint64_t) + n * sizeof(int32_t)));
    uint64_t *hOff = (uint64_t *) pin.p;
    int32_t *hl = (int32_t *) (hOff + n + 1);
    DROPCHK(hipMemcpy(hOff, dOff, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    DROPCHK(hipMemcpy(hl, dLen, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int rc = checkTable(ctx, "fsgpu_db_adopt_device", hOff, hl, n, bytes);
    if (rc != FSGPU_OK) return dropDb(ctx, rc);
    std::vector<int32_t> hLen(hl, hl + n);
    return replaceDb(ctx, d3, dA, dOff, dLen, std::move(hLen), bytes);
}

int fsgpu_db_load(fsgpu_ctx *ctx, const uint8_t *data3di, const uint8_t *dataAA, const uint64_t *offsets,
                  const int32_t *lengths, uint64_t n, uint64_t bytes) {
    if (!ctx) return FSGPU_E_ARG;
    DROPCHK(hipSetDevice(ctx->device));
    if (!data3di || !offsets || !lengths || n == 0 || n > 0xfffffff0ull) { ctx->err = "fsgpu_db_load: bad argument"; return dropDb(ctx, FSGPU_E_ARG); }
    int rc = checkTable(ctx, "fsgpu_db_load", offsets, lengths, n, bytes);
    if (rc != FSGPU_OK) return dropDb(ctx, rc);
    // staging copies of the caller's arrays; released on every way out
    struct Staging {
        void *p[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Staging() { for (void *q : p) (void) hipFree(q); }
    } st;
    auto stage = [&](int k, const void *src, uint64_t size) -> hipError_t {
        hipError_t e = hipMalloc(&st.p[k], std::max<uint64_t>(size, 1));
        return e != hipSuccess || size == 0 ? e : hipMemcpy(st.p[k], src, size, hipMemcpyHostToDevice);
    };
    hipError_t e = stage(0, data3di, bytes);
    if (e == hipSuccess && dataAA) e = stage(1, dataAA, bytes);
    if (e == hipSuccess) e = stage(2, offsets, (n + 1) * sizeof(uint64_t));
    if (e == hipSuccess) e = stage(3, lengths, n * sizeof(int32_t));
    if (e != hipSuccess) return dropDbHip(ctx, "fsgpu_db_load: staging the database", e);
    return replaceDb(ctx, st.p[0], st.p[1], st.p[2], st.p[3], std::vector<int32_t>(lengths, lengths + n), bytes);
}

#undef DROPCHK
} // extern "C"

// ------------------------------------------------------------------------------------------------------------
// One node, several GPUs, one process: replicate the resident database of `src` into contexts on other devices
// with ONE broadcast per buffer (RCCL over xGMI, single-process communicator set; librccl is loaded on demand so
// that single-GPU use has no dependency on it) or, when RCCL cannot be loaded, with peer copies.
// ------------------------------------------------------------------------------------------------------------
namespace {
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    bool load() {
        if (getenv("FSGPU_NO_RCCL")) return false;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll)) dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy)) dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart)) dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd)) dlsym(lib, "ncclGroupEnd");
        Broadcast = (decltype(Broadcast)) dlsym(lib, "ncclBroadcast");
        return CommInitAll && CommDestroy && GroupStart && GroupEnd && Broadcast;
    }
};
} // namespace

// librccl on this context's device, alone: a one-rank communicator broadcasts a 1 MiB buffer in place.  What a single-GPU box can show of
// the multi-GPU replication path: the library loads, a communicator comes up on the device, a grouped ncclBroadcast runs on the
// context's stream (FSGPU_REQUIRE_RCCL=1 makes the modules call it even when one GPU is used).
extern "C" int fsgpu_rccl_selfcheck(fsgpu_ctx *ctx) {
    if (!ctx) return FSGPU_E_ARG;
    HIPCHK(hipSetDevice(ctx->device));
    Rccl rccl;
    if (!rccl.load()) { ctx->err = "fsgpu_rccl_selfcheck: librccl could not be loaded (or FSGPU_NO_RCCL is set)"; return FSGPU_E_UNSUPPORTED; }
    const size_t bytes = 1 << 20;
    unsigned char *buf = nullptr;
    HIPCHK(hipMalloc((void **) &buf, bytes));
    std::vector<unsigned char> host(bytes);
    for (size_t i = 0; i < bytes; i++) host[i] = (unsigned char) (i * 131 + 7);
    int rc = FSGPU_OK;
    void *comm = nullptr;
    const int dev = ctx->device;
    if (hipMemcpy(buf, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "fsgpu_rccl_selfcheck: copy failed"; rc = FSGPU_E_HIP; }
    else if (rccl.CommInitAll(&comm, 1, &dev) != 0) { ctx->err = "fsgpu_rccl_selfcheck: ncclCommInitAll failed"; rc = FSGPU_E_HIP; }
    else {
        const bool ok = rccl.GroupStart() == 0 && rccl.Broadcast(buf, buf, bytes, 1 /*ncclUint8*/, 0, comm, ctx->stream) == 0 && rccl.GroupEnd() == 0 &&
                        hipStreamSynchronize(ctx->stream) == hipSuccess;
        std::vector<unsigned char> back(bytes);
        if (!ok || hipMemcpy(back.data(), buf, bytes, hipMemcpyDeviceToHost) != hipSuccess || back != host) { ctx->err = "fsgpu_rccl_selfcheck: the one-rank ncclBroadcast failed"; rc = FSGPU_E_HIP; }
        rccl.CommDestroy(comm);
    }
    (void) hipFree(buf);
    return rc;
}

extern "C" int fsgpu_db_broadcast(fsgpu_ctx *src, fsgpu_ctx **dst, int n, int *usedRccl) {
    fsgpu_ctx *ctx = src;       // HIPCHK reports into the source context
    if (usedRccl) *usedRccl = 0;
    if (!src || (n > 0 && !dst) || n < 0) return FSGPU_E_ARG;
    if (!src->db || src->db->n == 0) { src->err = "fsgpu_db_broadcast: no database loaded"; return FSGPU_E_NODB; }
    if (n == 0) return FSGPU_OK;
    bool distinct = true;
    for (int i = 0; i < n; i++) {
        if (!dst[i] || dst[i] == src) { src->err = "fsgpu_db_broadcast: bad destination context"; return FSGPU_E_ARG; }
        distinct = distinct && dst[i]->device != src->device;      // a second copy on the same device is legal (tests), RCCL is not used for it
    }
    const DbStore &db = *src->db;
    const uint64_t nT = db.n, bytes = db.bytes;
    // the four inputs of buildDb as they live on the source device (the unmasked AA copy is a fixed point of k_db_unmask)
    // (a database without residues has bytes == 0: its two byte buffers are still allocated on the destination, nothing is copied into them)
    struct Buf { const void *srcp; size_t size; bool present; std::vector<void *> dstp; };
    Buf bufs[4] = {{db.raw3di, (size_t) bytes, true, {}}, {db.hasAA ? db.alnAA : nullptr, db.hasAA ? (size_t) bytes : 0, db.hasAA, {}},
                   {db.dOffsets, (size_t) (nT + 1) * sizeof(uint64_t), true, {}}, {db.dLengths, (size_t) nT * sizeof(int32_t), true, {}}};
    auto freeAll = [&]() {
        for (Buf &b : bufs) for (size_t i = 0; i < b.dstp.size(); i++) if (b.dstp[i]) { (void) hipSetDevice(dst[i]->device); (void) hipFree(b.dstp[i]); }
        (void) hipSetDevice(src->device);
    };
    for (Buf &b : bufs) {
        b.dstp.assign(n, nullptr);
        if (!b.present) continue;
        for (int i = 0; i < n; i++) {
            if (hipSetDevice(dst[i]->device) != hipSuccess || hipMalloc(&b.dstp[i], std::max<size_t>(b.size, 1)) != hipSuccess) { freeAll(); src->err = "fsgpu_db_broadcast: out of device memory"; return FSGPU_E_NOMEM; }
        }
    }
    HIPCHK(hipSetDevice(src->device));
    HIPCHK(hipStreamSynchronize(src->stream));
    Rccl rccl;
    bool done = false;
    if (distinct && rccl.load()) {
        std::vector<int> devs(n + 1);
        devs[0] = src->device;
        for (int i = 0; i < n; i++) devs[i + 1] = dst[i]->device;
        std::vector<void *> comms(n + 1, nullptr);
        if (rccl.CommInitAll(comms.data(), n + 1, devs.data()) == 0) {
            bool ok = true;
            for (Buf &b : bufs) {
                if (!b.size) continue;
                ok = ok && rccl.GroupStart() == 0;
                for (int r = 0; r <= n && ok; r++) {
                    fsgpu_ctx *c = r == 0 ? src : dst[r - 1];
                    ok = hipSetDevice(c->device) == hipSuccess &&
                         rccl.Broadcast(b.srcp, r == 0 ? const_cast<void *>(b.srcp) : b.dstp[r - 1], b.size, 1 /*ncclUint8*/, 0, comms[r], c->stream) == 0;
                }
                ok = (rccl.GroupEnd() == 0) && ok;
            }
            for (int r = 0; r <= n; r++) {
                fsgpu_ctx *c = r == 0 ? src : dst[r - 1];
                ok = hipSetDevice(c->device) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess && ok;
            }
            for (void *c : comms) if (c) rccl.CommDestroy(c);
            done = ok;
            if (usedRccl) *usedRccl = ok ? 1 : 0;
        }
    }
    if (!done) {
        for (Buf &b : bufs) {
            if (!b.size) continue;
            for (int i = 0; i < n; i++)
                if (hipMemcpyPeer(b.dstp[i], dst[i]->device, b.srcp, src->device, b.size) != hipSuccess) { freeAll(); src->err = "fsgpu_db_broadcast: peer copy failed"; return FSGPU_E_HIP; }
        }
        // peer copies are device-side work on the null streams: not synchronous with the host, not ordered against the contexts' non-blocking streams
        for (int r = 0; r <= n; r++) {
            fsgpu_ctx *c = r == 0 ? src : dst[r - 1];
            if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { freeAll(); src->err = "fsgpu_db_broadcast: peer copy failed"; return FSGPU_E_HIP; }
        }
    }
    int rc = FSGPU_OK;
    for (int i = 0; i < n && rc == FSGPU_OK; i++) {
        rc = fsgpu_db_adopt_device(dst[i], bufs[0].dstp[i], bufs[1].dstp[i], bufs[2].dstp[i], bufs[3].dstp[i], nT, bytes);
        if (rc != FSGPU_OK) src->err = std::string("fsgpu_db_broadcast: ") + dst[i]->err;
    }
    freeAll();
    return rc;
}

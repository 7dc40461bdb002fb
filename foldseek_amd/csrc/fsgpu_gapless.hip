// fsgpu_gapless.hip -- the gapless prefilter scan: work-item planning, single- and multi-query launches of k_gapless, top-K selection.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_select.hpp"
#include "k_gapless.hpp"

// ------------------------------------------------------------------------------------------------------------
// gapless work list.  ov = warm-up chunks a column segment needs (= register count R of the query, 16 R >= Lq);
// ov = 0: whole stripes only (row-tiled long queries).  A stripe longer than `cap` chunks is cut into K segments of
// equal new length that each start ov chunks early; cap minimises max(cap, (work + warm-up work) / waves), the
// completion time of a longest-first queue over equally fast waves.
// ------------------------------------------------------------------------------------------------------------
// pure planning step (host only, no device calls; exported as fsgpu_gapless_plan_items for the CPU tests)
static void planGaplessItems(const std::vector<uint32_t> &len, int ov, double waves, std::vector<uint64_t> &v, bool &split, uint32_t &capOut) {
    const uint32_t nStripes = (uint32_t) len.size();
    uint64_t total = 0;
    uint32_t maxLen = 0;
    for (uint32_t x : len) { total += x; maxLen = std::max(maxLen, x); }
    uint32_t cap = maxLen;
    if (ov > 0 && maxLen > 2u * ov) {
        // histogram of stripe lengths -> cost of every candidate cap
        std::vector<uint32_t> hist(maxLen + 1, 0);
        for (uint32_t x : len) hist[x]++;
        double best = std::max((double) maxLen, (double) total / waves);
        for (uint32_t c = 2u * ov; c < maxLen; c++) {
            uint64_t extra = 0;
            const uint32_t fresh = c - ov;
            for (uint32_t x = c + 1; x <= maxLen; x++)
                if (hist[x]) extra += (uint64_t) hist[x] * ((x + fresh - 1) / fresh - 1) * ov;
            const double t = std::max((double) c, (double) (total + extra) / waves);
            if (t < best) { best = t; cap = c; }
        }
    }
    capOut = cap;
    v.clear();
    v.reserve(nStripes + 64);
    split = false;
    for (uint32_t s = 0; s < nStripes; s++) {
        const uint32_t L = len[s];
        if (L == 0) continue;
        if (L <= cap || ov == 0) { v.push_back(((uint64_t) s << 32) | L); continue; }
        const uint32_t K = (L + (cap - ov) - 1) / (cap - ov), fresh = (L + K - 1) / K;
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t b = k * fresh, e = std::min(L, (k + 1) * fresh);
            if (b >= e) break;
            const uint32_t b0 = b > (uint32_t) ov ? b - ov : 0;
            v.push_back(((uint64_t) s << 32) | (1ull << 31) | ((uint64_t) b0 << 16) | e);
            split = true;
        }
    }
    std::stable_sort(v.begin(), v.end(), [](uint64_t a, uint64_t b) {
        const uint32_t la = (uint32_t) (a & 0xffff) - (uint32_t) ((a >> 16) & 0x7fff), lb = (uint32_t) (b & 0xffff) - (uint32_t) ((b >> 16) & 0x7fff);
        return la > lb;
    });
}

extern "C" int64_t fsgpu_gapless_plan_items(const uint32_t *stripeLen, uint32_t nStripes, int overlap, double waves, uint64_t *items, uint64_t capacity, uint32_t *cap) {
    if ((!stripeLen && nStripes) || overlap < 0 || waves <= 0) return -1;
    std::vector<uint32_t> len(stripeLen, stripeLen + nStripes);
    std::vector<uint64_t> v;
    bool split = false;
    uint32_t c = 0;
    planGaplessItems(len, overlap, waves, v, split, c);
    if (cap) *cap = c;
    if (items) for (size_t i = 0; i < v.size() && i < capacity; i++) items[i] = v[i];
    return (int64_t) v.size();
}

// Device records of planned items: {stripe, range word, stripe offset in the scan layout (uint4 units) lo, trim << 24 | offset hi}.
// trim = real columns of the stripe's last chunk (1..16: longest target - 16 * (chunks - 1)), carried by the one item whose range ends with
// that chunk -- for a stripe cut into column segments the last segment alone -- and 0 everywhere else.  It rides in the top byte of the
// fourth word, which the offset (56 bits of 16-byte units left) never reaches; k_gapless masks it out where it forms the offset.
// Pure host function, exported as fsgpu_gapless_item_records for the CPU tests.
static bool gaplessRecords(const std::vector<uint64_t> &v, const uint32_t *len, const uint32_t *cols, uint32_t nStripes, uint4 *rec) {
    std::vector<uint64_t> sOff(nStripes);
    uint64_t acc = 0;
    for (uint32_t s = 0; s < nStripes; s++) {
        if (len[s] != (cols[s] + 15) / 16) return false;
        sOff[s] = acc; acc += (uint64_t) len[s] * 8;
    }
    if (acc >> 56) return false;
    for (size_t i = 0; i < v.size(); i++) {
        const uint32_t st = (uint32_t) (v[i] >> 32), endChunk = (uint32_t) (v[i] & 0xffff);
        if (st >= nStripes || endChunk > len[st]) return false;
        const uint32_t trim = endChunk == len[st] ? cols[st] - 16 * (len[st] - 1) : 0;
        rec[i] = make_uint4(st, (uint32_t) v[i], (uint32_t) sOff[st], (uint32_t) (sOff[st] >> 32) | (trim << 24));
    }
    return true;
}

extern "C" int64_t fsgpu_gapless_item_records(const uint64_t *items, uint64_t nItems, const uint32_t *stripeLen, const uint32_t *stripeCols, uint32_t nStripes, uint32_t *records) {
    if ((!items && nItems) || ((!stripeLen || !stripeCols) && nStripes) || (!records && nItems)) return -1;
    std::vector<uint64_t> v(items, items + nItems);
    std::vector<uint4> rec(nItems);
    if (!gaplessRecords(v, stripeLen, stripeCols, nStripes, rec.data())) return -1;
    if (nItems) memcpy(records, rec.data(), nItems * sizeof(uint4));
    return (int64_t) nItems;
}

// *needsClear: the score bytes must be zeroed before the launch -- column segments combine by atomic max into them, and a stripe of eight targets
// without residues has no work item at all, so nothing would store its bytes
static int gaplessItems(fsgpu_ctx *ctx, int ov, const uint4 **items, uint32_t *nItems, bool *needsClear) {
    DbStore &db = *ctx->db;
    std::lock_guard<std::mutex> lock(db.itemMutex);
    DbStore::ItemList &l = db.itemLists[ov];
    if (!l.built) {
        const std::vector<uint32_t> &len = db.hStripeLen;
        const uint32_t nStripes = (uint32_t) len.size();
        std::vector<uint64_t> v;
        bool split = false;
        uint32_t cap = 0;
        planGaplessItems(len, ov, (double) ctx->numCU * 3 * (kGaplessBlock / 64), v, split, cap);
        std::vector<uint4> rec(v.size());
        if (!gaplessRecords(v, len.data(), db.hStripeCols.data(), nStripes, rec.data())) { ctx->err = "internal: gapless work items do not fit the stripe table"; return FSGPU_E_ARG; }
        HIPCHK(hipMalloc((void **) &l.items, std::max<size_t>(rec.size(), 1) * sizeof(uint4)));
        if (!rec.empty()) {
            const hipError_t ce = hipMemcpy(l.items, rec.data(), rec.size() * sizeof(uint4), hipMemcpyHostToDevice);
            if (ce != hipSuccess) { (void) hipFree(l.items); l.items = nullptr; ctx->err = std::string("hipMemcpy(work items): ") + hipGetErrorString(ce); return FSGPU_E_HIP; }
        }
        const bool emptyStripe = std::find(len.begin(), len.end(), 0u) != len.end();
        l.n = (uint32_t) v.size(); l.needsClear = split || emptyStripe; l.built = true;
    }
    *items = l.items; *nItems = l.n; *needsClear = l.needsClear;
    return FSGPU_OK;
}

// ------------------------------------------------------------------------------------------------------------
// gapless scan
// ------------------------------------------------------------------------------------------------------------
// once per thread and device: the dynamic-LDS attribute of an instantiation and the workgroups of it a CU holds
template <int R, bool TILED, bool PAIRED, bool HALVES>
static int prepareGapless(fsgpu_ctx *ctx, int *perCU) {
    const int lds = gaplessLdsBytes(R);
    static thread_local uint64_t attrDevs = 0;       // devices on which this thread has set the attribute (it is per device)
    static thread_local int perCUcached = 0;
    const uint64_t devBit = 1ull << (ctx->device & 63);
    if (!(attrDevs & devBit)) {
        HIPCHK(hipFuncSetAttribute((const void *) k_gapless<R, TILED, PAIRED, HALVES>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCUcached, k_gapless<R, TILED, PAIRED, HALVES>, gaplessBlockThreads(R), lds));
        attrDevs |= devBit;
    }
    *perCU = perCUcached;
    return FSGPU_OK;
}

template <int R, bool TILED, bool PAIRED = false, bool HALVES = false>
static int launchGapless(fsgpu_ctx *ctx, const GaplessArgs &gaIn) {
    GaplessArgs ga = gaIn;
    const int lds = gaplessLdsBytes(R);
    int perCU = 0, rc;
    if ((rc = prepareGapless<R, TILED, PAIRED, HALVES>(ctx, &perCU)) != FSGPU_OK) return rc;
    // A class's two-queries-per-register kernel is made ready with its unpaired one: whoever has run one query of a class alone (a warm-up)
    // does not pay the set-up of the other inside the first batch that pairs the class
    if constexpr (!TILED && !PAIRED && !HALVES && R >= kGaplessHalvesMinR && R <= kGaplessHalvesMaxR) {
        int other = 0;
        if ((rc = prepareGapless<R, false, false, true>(ctx, &other)) != FSGPU_OK) return rc;
    }
    // Workgroups of 4 waves, each with its own LDS image; 3 per CU (12 waves, <= 135 KB LDS): more does not issue faster
    // (profiles/r01_q_gapless_ablation_ubench.txt, tools/bench_ab2.sh) and this leaves wave slots for the latency-bound SW
    // wavefront kernels of other in-flight queries to co-reside.  FSGPU_GAPLESS_BLOCKS_PER_CU overrides.
    constexpr int wavesPerBlock = gaplessBlockThreads(R) / 64;
    perCU = std::max(1, std::min(perCU, ctx->gaplessBlocksPerCU));
    // multi-query launch: 2 workgroups per CU and query (the third resident slot goes to the next query's workgroups, which
    // start while this query's tail drains): 2.75 vs 2.79 ms per query at 1M targets, tools: FSGPU_GAPLESS_BLOCKS_PER_CU sweep
    if (gaIn.queries) {
        static const int multiPerCU = [] { const char *e = getenv("FSGPU_GAPLESS_MULTI_BLOCKS_PER_CU"); return e ? std::max(1, atoi(e)) : 2; }();
        perCU = std::min(perCU, multiPerCU);
    }
    // one wave needs one stripe at a time: do not launch more waves than stripes
    uint32_t blocks = (uint32_t) std::min<uint64_t>((uint64_t) ctx->numCU * perCU, ((uint64_t) ga.nItems + wavesPerBlock - 1) / wavesPerBlock);
    blocks = std::max(blocks, 1u);
    // multi-query launch: ga.blocksPerQuery carries the number of queries on entry; every query gets `blocks` workgroups
    const uint32_t nQueries = ga.queries ? std::max(1u, ga.blocksPerQuery) : 1u;
    ga.blocksPerQuery = blocks;
    hipLaunchKernelGGL((k_gapless<R, TILED, PAIRED, HALVES>), dim3(blocks * nQueries), dim3(gaplessBlockThreads(R)), lds, ctx->stream, ga);
    HIPCHK(hipGetLastError());
    return FSGPU_OK;
}

// one instantiation per register count: a query of L residues runs with R = ceil(L / 16) (16-row granularity)
using GaplessLaunchFn = int (*)(fsgpu_ctx *, const GaplessArgs &);
#define FS_GAPLESS8(M, B, ...) launchGapless<M * (B + 1), __VA_ARGS__>, launchGapless<M * (B + 2), __VA_ARGS__>, launchGapless<M * (B + 3), __VA_ARGS__>, launchGapless<M * (B + 4), __VA_ARGS__>, \
                               launchGapless<M * (B + 5), __VA_ARGS__>, launchGapless<M * (B + 6), __VA_ARGS__>, launchGapless<M * (B + 7), __VA_ARGS__>, launchGapless<M * (B + 8), __VA_ARGS__>
static const GaplessLaunchFn kGaplessUntiled[kGaplessMaxRUntiled + 1] = {nullptr, FS_GAPLESS8(1, 0, false), FS_GAPLESS8(1, 8, false), FS_GAPLESS8(1, 16, false), FS_GAPLESS8(1, 24, false),
                                                                        FS_GAPLESS8(1, 32, false), FS_GAPLESS8(1, 40, false), FS_GAPLESS8(1, 48, false)};
// query row tiles: more than one tile means L > 896, and gaplessShape cuts tiles of equal height: two of 449..512 rows (R = 29..32), three of
// 342..512 (R = 22..32), four or more of at least 385 (R >= 25).  R = 22..32 are all the counts a length can reach (tests walk every L).
constexpr int kGaplessTiledMinR = 22;
static const GaplessLaunchFn kGaplessTiled[kGaplessMaxR - kGaplessTiledMinR + 1] = {launchGapless<22, true>, launchGapless<23, true>, launchGapless<24, true>, FS_GAPLESS8(1, 24, true)};
// two short queries of class R = 1..16 in one kernel of 2 R registers
static const GaplessLaunchFn kGaplessPaired[kGaplessMaxR / 2 + 1] = {nullptr, FS_GAPLESS8(2, 0, false, true), FS_GAPLESS8(2, 8, false, true)};
// two queries of class R = 17..36 in the halves of every register, R registers
static const GaplessLaunchFn kGaplessHalves[kGaplessHalvesMaxR - kGaplessHalvesMinR + 1] = {FS_GAPLESS8(1, 16, false, false, true), FS_GAPLESS8(1, 24, false, false, true),
                                                                                           launchGapless<33, false, false, true>, launchGapless<34, false, false, true>,
                                                                                           launchGapless<35, false, false, true>, launchGapless<36, false, false, true>};
#undef FS_GAPLESS8
static_assert(kGaplessHalvesMinR == 17 && kGaplessHalvesMaxR == 36, "kGaplessHalves lists the classes 17..36");

// The shape of a query of L rows: up to 16 * kGaplessMaxRUntiled rows in one piece, R = ceil(L / 16) registers (16-row granularity); beyond that
// row tiles of at most 512 rows and equal height: L = 1025 runs as 3 x 352 rows (R = 22), not as 512 + 512 + 1 rows at the full R = 32 cost each.
// Pure host function, exported as fsgpu_gapless_shape for the CPU tests.
static void gaplessShape(int L, int *nTiles, int *R) {
    const int rows = (L + 15) / 16;                       // rows per strip per lane
    *nTiles = L <= 16 * kGaplessMaxRUntiled ? 1 : (L + 16 * kGaplessMaxR - 1) / (16 * kGaplessMaxR);
    *R = *nTiles > 1 ? ((L + *nTiles - 1) / *nTiles + 15) / 16 : std::max(1, rows);
}

extern "C" int fsgpu_gapless_shape(int L, int *nTiles, int *R) {
    if (L < 1 || L > FSGPU_MAX_SEQ_LEN || !nTiles || !R) return -1;
    gaplessShape(L, nTiles, R);
    return 0;
}

// hits in the reference's order (hit_t::compareHitsByScoreAndId; scores are non-negative here)
static void emitHits(fsgpu_hit *out, const uint32_t *ids, const int32_t *scores, uint32_t m) {
    for (uint32_t i = 0; i < m; i++) { out[i].id = ids[i]; out[i].score = scores[i]; }
    std::sort(out, out + m, [](const fsgpu_hit &a, const fsgpu_hit &b) { return a.score != b.score ? a.score > b.score : a.id < b.id; });
}

// The device batch of one call: its steps (mq*) in the order fsgpu_gapless_scan_multi runs them.
struct MqBatch {
    const fsgpu_gapless_query *q;
    int minScore, maxRes;
    std::vector<int> batch;                  // the single-tile queries of the call, grouped by register class, long queries first
    int nb;
    uint32_t n, nChunks, K;
    uint64_t scoreStride;
    std::vector<size_t> pOff;                // byte offset of slot k's PSSM in mqPssm
    size_t nRec;                             // GaplessQuery records: one per slot, then one per pair of queries
    struct PairLaunch { int Rq; size_t rec0; int count; bool halves; };      // halves: k_gapless HALVES of class Rq, else PAIRED of the short class Rq
    std::vector<PairLaunch> pairLaunches;
    std::vector<char> isPaired;
    int classOf(int k) const { return std::max(1, (q[batch[k]].L + 15) / 16); }
    int classEnd(int k0) const { int k1 = k0; while (k1 < nb && classOf(k1) == classOf(k0)) k1++; return k1; }
};

// buffers of the batch, and one slot (PSSM, score slice, queue word, record) per query
static int mqSlots(fsgpu_ctx *ctx, MqBatch &b) {
    const int nb = b.nb;
    const uint32_t nChunks = b.nChunks, K = b.K;
    int rc;
    b.pOff.assign(nb + 1, 0);
    for (int k = 0; k < nb; k++) b.pOff[k + 1] = b.pOff[k] + ((size_t) kAlphabet * b.q[b.batch[k]].L + 63) / 64 * 64;
    // one record per query + one per pair; a class of pairHalves may add a record whose B is dead
    const size_t nRecMax = (size_t) nb + (size_t) nb / 2 + 1 + (kGaplessHalvesMaxR - kGaplessHalvesMinR + 1);
    if ((rc = ensureAll(ctx, {{ctx->mqPssm, b.pOff[nb]}, {ctx->mqScores, b.scoreStride * nb}, {ctx->mqQueues, nRecMax * 4}, {ctx->mqRec, nRecMax * sizeof(GaplessQuery)},
                              {ctx->mqHist, (size_t) nb * nChunks * 256 * 4}, {ctx->mqBaseGt, (size_t) nb * nChunks * 4}, {ctx->mqBaseTie, (size_t) nb * nChunks * 4},
                              {ctx->mqMeta, (size_t) nb * sizeof(SelMeta)}, {ctx->mqOutId, (size_t) nb * K * 4}, {ctx->mqOutScore, (size_t) nb * K * 4}, {ctx->mqIdent, (size_t) nb * 8}})) != FSGPU_OK) return rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hMqPssm, b.pOff[nb]}, {ctx->hMqRec, nRecMax * sizeof(GaplessQuery)}, {ctx->hMqMeta, (size_t) nb * sizeof(SelMeta)},
                                    {ctx->hMqOutId, (size_t) nb * K * 4}, {ctx->hMqOutScore, (size_t) nb * K * 4}, {ctx->hMqIdent, (size_t) nb * 8}})) != FSGPU_OK) return rc;
    ctx->mqScoreStride = b.scoreStride;
    GaplessQuery *rec = (GaplessQuery *) ctx->hMqRec.p;
    int64_t *ident = (int64_t *) ctx->hMqIdent.p;
    for (int k = 0; k < nb; k++) {
        const fsgpu_gapless_query &qq = b.q[b.batch[k]];
        memcpy((char *) ctx->hMqPssm.p + b.pOff[k], qq.pssm, (size_t) kAlphabet * qq.L);
        rec[k].pssm = (const int8_t *) ctx->mqPssm.p + b.pOff[k];
        rec[k].scores = (uint8_t *) ctx->mqScores.p + b.scoreStride * k;
        rec[k].queue = (uint32_t *) ctx->mqQueues.p + k;
        rec[k].L = qq.L;
        rec[k].cap = std::max(0, std::min(qq.scoreCap, 255));
        rec[k].pssmB = nullptr; rec[k].scoresB = nullptr; rec[k].LB = 0; rec[k].capB = 0;
        ident[k] = qq.identityId;
        ctx->mqSlot[b.batch[k]] = k;
    }
    b.nRec = (size_t) nb;
    return FSGPU_OK;
}

// ------------------------------------------------------------------------------------------------------------
// Which queries of a call share the registers of k_gapless<R, false, false, HALVES> (classes kGaplessHalvesMinR .. kGaplessHalvesMaxR).
// cls[i] = register class of query i.  Per query: launchClass = the class whose launch carries it, record = its record in that launch and
// half = 0 (query A, low halves) or 1 (query B); record = half = -1: not placed here, the query runs as it did (unpaired kernel, paired
// short classes, row tiles).
//   * a class with one member keeps the unpaired kernel; one with m >= 2 members gets ONE launch over its members two by two, in order;
//   * the odd member out of a class of m >= 3 would run with a dead B, which costs what a whole query costs: it may move up instead, at most
//     kGaplessHalvesPromote registers, as query B beside the odd member out of a class that has one, or beside a single member (whose launch
//     then is one record of this kernel).  Every class keeps its one launch: nobody leaves a class of fewer than three, no launch is added.
//     The guest's profile is zero behind its length like any query's and the larger class's column segments warm up longer than it needs:
//     its scores are those of its own class.  Who moves where is chosen for the fewest dead halves (a small dynamic program over the
//     classes: two odd members out that meet save two, a guest of a single member one).
// Pure host function, exported as fsgpu_gapless_pair_halves for the CPU tests.  Returns the number of records.
// ------------------------------------------------------------------------------------------------------------
static int pairHalves(const int *cls, int n, int *launchClass, int *record, int *half) {
    int members[kGaplessHalvesMaxR + 1] = {0}, placed[kGaplessHalvesMaxR + 1] = {0}, last[kGaplessHalvesMaxR + 1];
    const auto inRange = [](int R) { return R >= kGaplessHalvesMinR && R <= kGaplessHalvesMaxR; };
    for (int i = 0; i < n; i++)
        if (inRange(cls[i])) members[cls[i]]++;
    int records = 0;
    for (int i = 0; i < n; i++) {
        launchClass[i] = cls[i]; record[i] = -1; half[i] = -1;
        if (!inRange(cls[i])) continue;
        last[cls[i]] = i;
        if (members[cls[i]] < 2) continue;
        const int p = placed[cls[i]]++;
        record[i] = p / 2; half[i] = p % 2;
        if (half[i] == 0) records++;
    }
    // Fewest dead halves: dead[R][s] = those from class R on when the odd members out of R - 2 (s & 1) and R - 1 (s & 2) still look for a seat.
    // At R the one from R - 2 is seated or lost; a class that seats nobody and has an odd member out of its own (m >= 3) hands it on.
    static_assert(kGaplessHalvesPromote == 2, "the state below holds the two classes in reach");
    constexpr int N = kGaplessHalvesMaxR + 2;
    int dead[N + 1][4], take[N + 1][4];               // take: 0 nobody, 1 the one from R - 2, 2 the one from R - 1
    for (int s = 0; s < 4; s++) dead[N][s] = (s & 1) + (s >> 1);
    for (int R = N - 1; R >= kGaplessHalvesMinR; R--)
        for (int s = 0; s < 4; s++) {
            const int m = R <= kGaplessHalvesMaxR ? members[R] : 0;
            dead[R][s] = 1 << 30;
            for (int t = 1; t <= 3; t++) {            // seating first: with equal dead halves a shared record is the cheaper one
                const int who = t % 3;
                if (who && (m % 2 == 0 || !(s & who))) continue;
                const int left = s & ~who;
                const int mine = (m >= 3 && m % 2 == 1 && !who) ? 2 : 0;
                const int d = (left & 1) + dead[R + 1][(left >> 1) | mine];
                if (d < dead[R][s]) { dead[R][s] = d; take[R][s] = who; }
            }
        }
    for (int R = kGaplessHalvesMinR, s = 0; R <= kGaplessHalvesMaxR; R++) {
        const int who = take[R][s], m = members[R];
        if (who) {
            const int i = last[R - (who == 1 ? 2 : 1)];                    // that class's odd member out: B of this class's last record
            if (m >= 3) records--;                                           // the two odd members out share a record
            else { record[last[R]] = 0; half[last[R]] = 0; }                // a single member opens its class's only record
            launchClass[i] = R; record[i] = m / 2; half[i] = 1;
        }
        s = ((s & ~who) >> 1) | ((m >= 3 && m % 2 == 1 && !who) ? 2 : 0);
    }
    return records;
}

extern "C" int fsgpu_gapless_pair_halves(const int32_t *classes, int n, int32_t *launchClass, int32_t *record, int32_t *half) {
    if (n < 0 || (n > 0 && (!classes || !launchClass || !record || !half))) return -1;
    for (int i = 0; i < n; i++)
        if (classes[i] < 1) return -1;
    return pairHalves(classes, n, launchClass, record, half);
}

// Short queries (<= 256 residues) of one 16-row class run two to a kernel (k_gapless<2R, false, PAIRED>: the per-column
// instructions that do not scale with the rows are shared); an odd one out runs alone.  Queries of the classes 17 .. 36 share registers
// instead (pairHalves).
static void mqPairShort(fsgpu_ctx *ctx, MqBatch &b) {
    // classes up to 16 registers (256 residues): beyond that the pair would need the 8-wave workgroups of R > 36, which was measured
    // and loses (pairs up to class 20 / 24 / 28 at 1M targets: 2.74 / 2.77 / 2.84 ms per query against 2.76 without)
    constexpr int pairMaxR = kGaplessMaxR / 2;
    GaplessQuery *rec = (GaplessQuery *) ctx->hMqRec.p;
    b.isPaired.assign(b.nb, 0);
    for (int k0 = 0; k0 < b.nb;) {
        const int R = b.classOf(k0), k1 = b.classEnd(k0);
        if (R <= pairMaxR && k1 - k0 >= 2) {
            MqBatch::PairLaunch pl{R, b.nRec, (k1 - k0) / 2, false};
            for (int p2 = 0; p2 < pl.count; p2++) {
                const int ka = k0 + 2 * p2, kb = ka + 1;
                rec[b.nRec] = rec[ka];
                rec[b.nRec].queue = (uint32_t *) ctx->mqQueues.p + b.nRec;
                rec[b.nRec].pssmB = rec[kb].pssm; rec[b.nRec].scoresB = rec[kb].scores; rec[b.nRec].LB = rec[kb].L; rec[b.nRec].capB = rec[kb].cap;
                b.isPaired[ka] = b.isPaired[kb] = 1;
                b.nRec++;
            }
            b.pairLaunches.push_back(pl);
        }
        k0 = k1;
    }
    // classes 17 .. 36: two queries in the halves of every register (pairHalves), one launch per class
    std::vector<int> cls(b.nb), launchClass(b.nb), record(b.nb), half(b.nb);
    for (int k = 0; k < b.nb; k++) cls[k] = b.classOf(k);
    if (pairHalves(cls.data(), b.nb, launchClass.data(), record.data(), half.data()) == 0) return;
    int count[kGaplessHalvesMaxR + 1] = {0};
    for (int k = 0; k < b.nb; k++)
        if (record[k] >= 0) count[launchClass[k]] = std::max(count[launchClass[k]], record[k] + 1);
    size_t rec0[kGaplessHalvesMaxR + 1] = {0};
    for (int R = kGaplessHalvesMaxR; R >= kGaplessHalvesMinR; R--) {           // long classes first, like the unpaired launches
        if (!count[R]) continue;
        rec0[R] = b.nRec;
        b.pairLaunches.push_back(MqBatch::PairLaunch{R, b.nRec, count[R], true});
        b.nRec += (size_t) count[R];
    }
    for (int pass = 0; pass < 2; pass++)                  // every record's A first: it brings the record's own queue word and a B that is absent
        for (int k = 0; k < b.nb; k++) {
            if (record[k] < 0 || half[k] != pass) continue;
            const size_t at = rec0[launchClass[k]] + (size_t) record[k];
            if (pass == 0) {
                rec[at] = rec[k];
                rec[at].queue = (uint32_t *) ctx->mqQueues.p + at;
            } else {
                rec[at].pssmB = rec[k].pssm; rec[at].scoresB = rec[k].scores; rec[at].LB = rec[k].L; rec[at].capB = rec[k].cap;
            }
            b.isPaired[k] = 1;
        }
}

static int mqUpload(fsgpu_ctx *ctx, const MqBatch &b) {
    HIPCHK(hipMemcpyAsync(ctx->mqPssm.p, ctx->hMqPssm.p, b.pOff[b.nb], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->mqRec.p, ctx->hMqRec.p, b.nRec * sizeof(GaplessQuery), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->mqIdent.p, ctx->hMqIdent.p, (size_t) b.nb * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->mqQueues.p, 0, b.nRec * 4, ctx->stream));
    return FSGPU_OK;
}

// one launch over `count` records from rec0 on
static int mqLaunch(fsgpu_ctx *ctx, const MqBatch &b, GaplessLaunchFn launch, const uint4 *items, uint32_t nItems, size_t rec0, int count) {
    GaplessArgs ga;
    ga.scan = ctx->db->scan; ga.stripeOff = ctx->db->stripeOff; ga.stripeLen = ctx->db->stripeLen; ga.stripeTargets = ctx->db->stripeTargets;
    ga.items = items; ga.nItems = nItems;
    ga.queries = (const GaplessQuery *) ctx->mqRec.p + rec0;
    ga.blocksPerQuery = (uint32_t) count;                  // number of queries on entry, see launchGapless
    ga.nTargets = b.n; ga.pssm = nullptr; ga.L = 0; ga.cap = 0; ga.scores = nullptr; ga.queue = nullptr;
    ga.tileBase = 0; ga.firstTile = 1; ga.lastTile = 1; ga.borderIn = nullptr; ga.borderOut = nullptr; ga.scoreAcc = nullptr;
    const int rc = launch(ctx, ga);
    if (rc == FSGPU_OK) ctx->mqLaunches++;
    return rc;
}

// One scan batch at a time per database, ordered ON THE DEVICE: every launch already fills the chip, two batches in
// flight would only stretch each other.  The inputs have gone up first (they may overlap the previous owner's scans), then
// -- under the mutex, which covers enqueueing only -- this stream is made to wait for the event the previous batch's
// owner recorded behind its last scan launch, the scans are enqueued and this batch's event takes its place.  The
// selection passes, copies and the host wait happen outside the mutex; SW / selection kernels of other contexts
// co-run in the slots a scan leaves.
static int mqScan(fsgpu_ctx *ctx, const MqBatch &b) {
    int rc;
    if (!ctx->scanDoneEv) HIPCHK(hipEventCreateWithFlags(&ctx->scanDoneEv, hipEventDisableTiming));
    struct Launch { GaplessLaunchFn fn; const uint4 *items; uint32_t nItems; size_t rec0; int count; };
    std::vector<Launch> launches;
    bool anyClear = false, clear = false;
    for (int k0 = 0; k0 < b.nb;) {
        const int R = b.classOf(k0), k1 = b.classEnd(k0);
        int kFree = k0;                                   // the paired queries of a class are its first ones
        while (kFree < k1 && b.isPaired[kFree]) kFree++;
        Launch l{kGaplessUntiled[R], nullptr, 0, (size_t) kFree, k1 - kFree};
        if ((rc = gaplessItems(ctx, R, &l.items, &l.nItems, &clear)) != FSGPU_OK) return rc;
        anyClear = anyClear || clear;
        if (kFree < k1) launches.push_back(l);
        k0 = k1;
    }
    for (const MqBatch::PairLaunch &pl : b.pairLaunches) {
        Launch l{pl.halves ? kGaplessHalves[pl.Rq - kGaplessHalvesMinR] : kGaplessPaired[pl.Rq], nullptr, 0, pl.rec0, pl.count};
        if ((rc = gaplessItems(ctx, pl.Rq, &l.items, &l.nItems, &clear)) != FSGPU_OK) return rc;     // warm-up of a column segment = the QUERY's rows
        anyClear = anyClear || clear;                     // (the loop above has asked for every class already, paired or not; kept so that this does not depend on it)
        launches.push_back(l);
    }
    // column segments combine by atomic max into zeroed score bytes, stripes without a column store nothing: clear all slices BEFORE the
    // first launch (a memset between launches would wipe what earlier groups stored)
    if (anyClear) HIPCHK(hipMemsetAsync(ctx->mqScores.p, 0, b.scoreStride * b.nb, ctx->stream));
    std::lock_guard<std::mutex> scanLock(ctx->db->scanMutex);
    if (ctx->db->lastScanDone && ctx->db->lastScanDone != ctx->scanDoneEv) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->db->lastScanDone, 0));
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    for (const Launch &l : launches)
        if ((rc = mqLaunch(ctx, b, l.fn, l.items, l.nItems, l.rec0, l.count)) != FSGPU_OK) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(hipEventRecord(ctx->scanDoneEv, ctx->stream));
    ctx->db->lastScanDone = ctx->scanDoneEv;
    return FSGPU_OK;
}

static int mqSelect(fsgpu_ctx *ctx, const MqBatch &b) {
    const uint32_t n = b.n, nChunks = b.nChunks, K = b.K;
    const int nb = b.nb;
    hipLaunchKernelGGL(k_sel_hist, dim3(nChunks, nb), dim3(kSelThreads), 0, ctx->stream, (const uint8_t *) ctx->mqScores.p, n, b.minScore,
                       (int64_t) -1, (uint32_t *) ctx->mqHist.p, (const int64_t *) ctx->mqIdent.p, b.scoreStride);
    hipLaunchKernelGGL(k_sel_threshold, dim3(nb), dim3(256), 0, ctx->stream, (const uint32_t *) ctx->mqHist.p, nChunks, K, (SelMeta *) ctx->mqMeta.p,
                       (uint32_t *) ctx->mqBaseGt.p, (uint32_t *) ctx->mqBaseTie.p);
    hipLaunchKernelGGL(k_sel_emit, dim3(nChunks, nb), dim3(kSelThreads), 0, ctx->stream, (const uint8_t *) ctx->mqScores.p, n, b.minScore,
                       (int64_t) -1, (const SelMeta *) ctx->mqMeta.p, (const uint32_t *) ctx->mqBaseGt.p, (const uint32_t *) ctx->mqBaseTie.p,
                       (uint32_t *) ctx->mqOutId.p, (int32_t *) ctx->mqOutScore.p, (const int64_t *) ctx->mqIdent.p, b.scoreStride, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->hMqMeta.p, ctx->mqMeta.p, (size_t) nb * sizeof(SelMeta), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->hMqOutId.p, ctx->mqOutId.p, (size_t) nb * K * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->hMqOutScore.p, ctx->mqOutScore.p, (size_t) nb * K * 4, hipMemcpyDeviceToHost, ctx->stream));
    return FSGPU_OK;
}

static int mqReadBack(fsgpu_ctx *ctx, const MqBatch &b, fsgpu_hit *out, int *nout) {
    const int rc = syncStream(ctx);
    if (rc != FSGPU_OK) return rc;
    const SelMeta *meta = (const SelMeta *) ctx->hMqMeta.p;
    for (int k = 0; k < b.nb; k++) {
        const int qi = b.batch[k];
        const uint32_t m = std::min<uint32_t>(meta[k].nOut, b.K);
        emitHits(out + (size_t) qi * b.maxRes, (const uint32_t *) ctx->hMqOutId.p + (size_t) k * b.K, (const int32_t *) ctx->hMqOutScore.p + (size_t) k * b.K, m);
        nout[qi] = (int) m;
    }
    return FSGPU_OK;
}

extern "C" {

int fsgpu_gapless_launch(fsgpu_ctx *ctx, const int8_t *pssm, int L, int scoreCap, int minScore, int64_t identityId, int maxRes) {
    if (!ctx) return FSGPU_E_ARG;
    ctx->mqScanMs = -1.0;                                  // fsgpu_last_kernel_ms(ctx, 0) reads this call's own events again
    if (!pssm || L <= 0 || L > FSGPU_MAX_SEQ_LEN || maxRes <= 0) { ctx->err = "fsgpu_gapless_launch: bad argument"; return FSGPU_E_ARG; }
    if (!ctx->db || ctx->db->n == 0) { ctx->err = "no database loaded"; return FSGPU_E_NODB; }
    if (ctx->gaplessPending) { ctx->err = "previous gapless scan not finished"; return FSGPU_E_ARG; }
    int nTiles, R;
    gaplessShape(L, &nTiles, &R);
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t) ctx->db->n;
    const uint32_t nChunks = (n + kSelChunk - 1) / kSelChunk;
    const uint32_t K = (uint32_t) std::min<uint64_t>((uint64_t) maxRes, ctx->db->n);
    int rc;
    if ((rc = ensureAll(ctx, {{ctx->pssm, (size_t) kAlphabet * L}, {ctx->scores, n}, {ctx->chunkHist, (size_t) nChunks * 256 * 4}, {ctx->baseGt, (size_t) nChunks * 4},
                              {ctx->baseTie, (size_t) nChunks * 4}, {ctx->outId, (size_t) K * 4}, {ctx->outScore, (size_t) K * 4}})) != FSGPU_OK) return rc;
    // border rows between query row tiles: 2 bytes per padded target column, ping-pong
    const size_t bbytes = (size_t) ctx->db->scanU4 * 32;
    if (nTiles > 1 && (rc = ensureAll(ctx, {{ctx->gBorder0, bbytes}, {ctx->gBorder1, bbytes}, {ctx->scoreAcc, (size_t) n * 2}})) != FSGPU_OK) return rc;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hOutId, (size_t) K * 4}, {ctx->hOutScore, (size_t) K * 4}, {ctx->hPssm, (size_t) kAlphabet * L}})) != FSGPU_OK) return rc;
    memcpy(ctx->hPssm.p, pssm, (size_t) kAlphabet * L);
    HIPCHK(hipMemcpyAsync(ctx->pssm.p, ctx->hPssm.p, (size_t) kAlphabet * L, hipMemcpyHostToDevice, ctx->stream));
    GaplessArgs ga;
    ga.queries = nullptr; ga.blocksPerQuery = 0;
    ga.scan = ctx->db->scan; ga.stripeOff = ctx->db->stripeOff; ga.stripeLen = ctx->db->stripeLen; ga.stripeTargets = ctx->db->stripeTargets;
    bool needsClear = false;
    if ((rc = gaplessItems(ctx, nTiles > 1 ? 0 : R, &ga.items, &ga.nItems, &needsClear)) != FSGPU_OK) return rc;
    ga.nTargets = n; ga.pssm = (const int8_t *) ctx->pssm.p; ga.L = L;
    ga.cap = std::max(0, std::min(scoreCap, 255));
    ga.scores = (uint8_t *) ctx->scores.p; ga.queue = ctx->queue;
    ga.tileBase = 0; ga.firstTile = 1; ga.lastTile = 1; ga.borderIn = nullptr; ga.borderOut = nullptr; ga.scoreAcc = (int16_t *) ctx->scoreAcc.p;
    if (needsClear) HIPCHK(hipMemsetAsync(ctx->scores.p, 0, n, ctx->stream));     // column segments combine by atomic max; a stripe without columns stores nothing
    HIPCHK(hipEventRecord(ctx->ev[0], ctx->stream));
    if (nTiles == 1) {
        HIPCHK(hipMemsetAsync(ctx->queue, 0, 4, ctx->stream));
        if (R < 1 || R > kGaplessMaxRUntiled) { ctx->err = "internal: bad R"; return FSGPU_E_ARG; }
        rc = kGaplessUntiled[R](ctx, ga);
        if (rc != FSGPU_OK) return rc;
    } else {
        // query row tiles of 16 R <= 512 rows: tile t+1 continues every diagonal of tile t through the border arrays in HBM
        if (R < kGaplessTiledMinR || R > kGaplessMaxR) { ctx->err = "internal: bad tiled R"; return FSGPU_E_ARG; }
        for (int t = 0; t < nTiles; t++) {
            HIPCHK(hipMemsetAsync(ctx->queue, 0, 4, ctx->stream));
            ga.tileBase = t * 16 * R;
            ga.firstTile = t == 0; ga.lastTile = t == nTiles - 1;
            ga.borderIn = (const uint16_t *) ((t & 1) ? ctx->gBorder1.p : ctx->gBorder0.p);
            ga.borderOut = (uint16_t *) ((t & 1) ? ctx->gBorder0.p : ctx->gBorder1.p);
            if ((rc = kGaplessTiled[R - kGaplessTiledMinR](ctx, ga)) != FSGPU_OK) return rc;
        }
    }
    HIPCHK(hipEventRecord(ctx->ev[1], ctx->stream));
    hipLaunchKernelGGL(k_sel_hist, dim3(nChunks), dim3(kSelThreads), 0, ctx->stream, (const uint8_t *) ctx->scores.p, n, minScore,
                       identityId, (uint32_t *) ctx->chunkHist.p, (const int64_t *) nullptr, (uint64_t) 0);
    hipLaunchKernelGGL(k_sel_threshold, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t *) ctx->chunkHist.p, nChunks, K, ctx->dMeta,
                       (uint32_t *) ctx->baseGt.p, (uint32_t *) ctx->baseTie.p);
    hipLaunchKernelGGL(k_sel_emit, dim3(nChunks), dim3(kSelThreads), 0, ctx->stream, (const uint8_t *) ctx->scores.p, n, minScore,
                       identityId, (const SelMeta *) ctx->dMeta, (const uint32_t *) ctx->baseGt.p, (const uint32_t *) ctx->baseTie.p,
                       (uint32_t *) ctx->outId.p, (int32_t *) ctx->outScore.p, (const int64_t *) nullptr, (uint64_t) 0, K);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->hMeta, ctx->dMeta, sizeof(SelMeta), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->hOutId.p, ctx->outId.p, (size_t) K * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->hOutScore.p, ctx->outScore.p, (size_t) K * 4, hipMemcpyDeviceToHost, ctx->stream));
    ctx->pendingMaxRes = (int) K;
    ctx->gaplessPending = true;
    ctx->scoresValid = true;
    ctx->evValid[0] = true;
    return FSGPU_OK;
}

int fsgpu_gapless_finish(fsgpu_ctx *ctx, fsgpu_hit *out, int *nout) {
    if (!ctx || !out || !nout) return FSGPU_E_ARG;
    if (!ctx->gaplessPending) { ctx->err = "no gapless scan in flight"; return FSGPU_E_ARG; }
    ctx->gaplessPending = false;
    HIPCHK(hipSetDevice(ctx->device));
    { int rc = syncStream(ctx); if (rc != FSGPU_OK) return rc; }
    const uint32_t m = std::min<uint32_t>(ctx->hMeta->nOut, (uint32_t) ctx->pendingMaxRes);
    emitHits(out, (const uint32_t *) ctx->hOutId.p, (const int32_t *) ctx->hOutScore.p, m);
    *nout = (int) m;
    return FSGPU_OK;
}

int fsgpu_gapless_scan(fsgpu_ctx *ctx, const int8_t *pssm, int L, int scoreCap, int minScore, int64_t identityId, int maxRes,
                       fsgpu_hit *out, int *nout) {
    int rc = fsgpu_gapless_launch(ctx, pssm, L, scoreCap, minScore, identityId, maxRes);
    if (rc != FSGPU_OK) return rc;
    return fsgpu_gapless_finish(ctx, out, nout);
}

// Several queries, one resident-DB pass each, in as few launches as their lengths allow: queries of one register class
// (R = ceil(L / 16)) share ONE launch of k_gapless (GaplessQuery records; workgroups of query q + 1 move in as those of
// query q drain), the three selection passes run once for the whole batch (blockIdx.y = query).  Results are those of nq
// fsgpu_gapless_scan calls.  Queries longer than 896 residues (row tiles) go through the single-query path.
int fsgpu_gapless_scan_multi(fsgpu_ctx *ctx, const fsgpu_gapless_query *q, int nq, int minScore, int maxRes, fsgpu_hit *out, int *nout) {
    if (!ctx) return FSGPU_E_ARG;
    if (nq < 0 || maxRes <= 0 || (nq > 0 && (!q || !out || !nout))) { ctx->err = "fsgpu_gapless_scan_multi: bad argument"; return FSGPU_E_ARG; }
    if (!ctx->db || ctx->db->n == 0) { ctx->err = "no database loaded"; return FSGPU_E_NODB; }
    if (ctx->gaplessPending) { ctx->err = "previous gapless scan not finished"; return FSGPU_E_ARG; }
    for (int i = 0; i < nq; i++)
        if (!q[i].pssm || q[i].L <= 0 || q[i].L > FSGPU_MAX_SEQ_LEN) { ctx->err = "fsgpu_gapless_scan_multi: bad query"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->mqLaunches = 0; ctx->mqQueries = 0; ctx->mqScanMs = -1.0;
    ctx->mqSlot.assign(nq, -1);
    // ---- device batch: the single-tile queries, grouped by register class ----
    MqBatch b;
    b.q = q; b.minScore = minScore; b.maxRes = maxRes;
    std::vector<int> longQ;
    for (int i = 0; i < nq; i++) {
        int nTiles, R;
        gaplessShape(q[i].L, &nTiles, &R);
        (nTiles == 1 ? b.batch : longQ).push_back(i);
    }
    std::stable_sort(b.batch.begin(), b.batch.end(), [&](int x, int y) { return (q[x].L + 15) / 16 > (q[y].L + 15) / 16; });   // long queries first
    b.nb = (int) b.batch.size();
    b.n = (uint32_t) ctx->db->n;
    b.nChunks = (b.n + kSelChunk - 1) / kSelChunk;
    b.K = (uint32_t) std::min<uint64_t>((uint64_t) maxRes, ctx->db->n);
    b.scoreStride = ((uint64_t) b.n + 255) / 256 * 256;
    if (b.nb > 0) {
        int rc;
        if ((rc = mqSlots(ctx, b)) != FSGPU_OK) return rc;
        mqPairShort(ctx, b);
        if ((rc = mqUpload(ctx, b)) != FSGPU_OK) return rc;
        if ((rc = mqScan(ctx, b)) != FSGPU_OK) return rc;
        ctx->evValid[0] = true;
        ctx->mqQueries = b.nb;
        if ((rc = mqSelect(ctx, b)) != FSGPU_OK) return rc;
        if ((rc = mqReadBack(ctx, b, out, nout)) != FSGPU_OK) return rc;
    }
    // scan time of the whole call (fsgpu_last_kernel_ms(ctx, 0)): the batch's launches plus the row-tiled scans of the long queries, which
    // run one at a time and reuse the same pair of events
    double scanMs = b.nb > 0 ? fsgpu_last_kernel_ms(ctx, 0) : 0.0;
    for (int qi : longQ) {
        const int rc = fsgpu_gapless_scan(ctx, q[qi].pssm, q[qi].L, q[qi].scoreCap, minScore, q[qi].identityId, maxRes, out + (size_t) qi * maxRes, &nout[qi]);
        if (rc != FSGPU_OK) return rc;
        const double ms = fsgpu_last_kernel_ms(ctx, 0);
        if (ms >= 0 && scanMs >= 0) scanMs += ms; else scanMs = -1.0;
        ctx->mqLaunches++; ctx->mqQueries++;
    }
    ctx->mqScanMs = scanMs;
    return FSGPU_OK;
}

int fsgpu_gapless_scores_multi(fsgpu_ctx *ctx, int queryIndex, uint8_t *scores_out) {
    if (!ctx || !scores_out) return FSGPU_E_ARG;
    if (!ctx->db || queryIndex < 0 || queryIndex >= (int) ctx->mqSlot.size() || ctx->mqSlot[queryIndex] < 0) { ctx->err = "no batched scan results for this query"; return FSGPU_E_ARG; }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(scores_out, (const uint8_t *) ctx->mqScores.p + ctx->mqScoreStride * (uint64_t) ctx->mqSlot[queryIndex], ctx->db->n, hipMemcpyDeviceToHost));
    return FSGPU_OK;
}

int fsgpu_gapless_last_batch(const fsgpu_ctx *ctx, int *launches, int *queries) {
    if (!ctx) return FSGPU_E_ARG;
    if (launches) *launches = ctx->mqLaunches;
    if (queries) *queries = ctx->mqQueries;
    return FSGPU_OK;
}

int fsgpu_gapless_scores(fsgpu_ctx *ctx, uint8_t *scores_out) {
    if (!ctx || !scores_out) return FSGPU_E_ARG;
    if (!ctx->db || ctx->db->n == 0 || !ctx->scores.p || !ctx->scoresValid) { ctx->err = "no scan results for the loaded database"; return FSGPU_E_NODB; }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(scores_out, ctx->scores.p, ctx->db->n, hipMemcpyDeviceToHost));
    return FSGPU_OK;
}

} // extern "C"

// fsgpu_sw3_multi.hip -- the compact-query Smith-Waterman path: orchestration of k_sw3 (its kernels and launchers are in fsgpu_sw3.hip).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fsgpu_ctx.h"
#include "k_sw3.hpp"
#include "fsgpu_sw3.h"
#include "fsgpu_sw3_plan.h"

// ---- compact-query form of fsgpu_sw_multi_dir: k_sw3 over device-built images ---------------------------------------------------
// A structurealign profile is matrix column + position bias (StructureSmithWaterman.cpp:1566-1640), so a query is given by its codes and
// biases; the LDS images are built by k_sw3_image.  Queries of up to 32 * 16 rows run with 32 lanes per target pair (four targets per
// wave), up to 64 * 16 rows with 64 lanes; longer ones and the int32 re-run of int16-saturated pairs go through the profile-based
// entry points with profiles materialised here.
// Profile queries (fsgpu_sw_multi_dir_p / _p: a query IS its int8 tables) run through the same plan: Sw3Plan::pq marks them, and only the three steps
// that look at where a score comes from -- sw3Validate, Sw3Plan::profilesOf, sw3Images (k_sw3_image_profile) -- branch on it.
static bool sw3Class(int L, int &R, int &HL) {
    if (L <= 32 * kSw3MaxR) { HL = 32; R = (L + 31) / 32; return true; }
    if (L <= 64 * kSw3MaxR) { HL = 64; R = (L + 63) / 64; return true; }
    return false;
}
static int sw3Waves(int R, int HL, bool hasAA) {
    static const int env = [] { const char *e = getenv("FSGPU_SW3_WAVES"); const int v = e ? atoi(e) : 0; return (v == 2 || v == 4 || v == 8) ? v : 0; }();
    if (env) return env;
    return (160 * 1024) / sw3LdsBytes(R, HL, hasAA, 4) >= 3 ? 4 : 8;
}
static void sw3Materialize(const int8_t *mat, const uint8_t *codes, const int8_t *cb, int L, bool reversed, std::vector<int16_t> &out) {
    out.resize((size_t) kAlphabet * L);
    for (int a = 0; a < kAlphabet; a++)
        for (int i = 0; i < L; i++)
            out[(size_t) a * L + i] = (int16_t) ((int) mat[a * kAlphabet + codes[reversed ? L - 1 - i : i]] + (cb ? (int) cb[i] : 0));
}

constexpr int kShapeHL[3] = {16, 32, 64};       // lanes per target pair of the three shapes

// a profile query's int8 table as the int16 word profile (ssw_init's profile_word_linear: the table itself)
static void sw3Widen(const int8_t *t, int L, std::vector<int16_t> &out) {
    out.resize((size_t) kAlphabet * L);
    for (size_t k = 0; k < out.size(); k++) out[k] = (int16_t) t[k];
}

void Sw3Plan::profilesOf(int i, Sw3Prof &pr) const {
    if (pq) {
        sw3Widen(pq[i].p3Di_fwd, pq[i].L, pr.sF); sw3Widen(pq[i].p3Di_rev, pq[i].L, pr.sR);
        if (hasAA) { sw3Widen(pq[i].pAA_fwd, pq[i].L, pr.aF); sw3Widen(pq[i].pAA_rev, pq[i].L, pr.aR); }
        return;
    }
    sw3Materialize(mat3Di, q[i].q3Di, q[i].cb3Di_fwd, q[i].L, false, pr.sF);
    sw3Materialize(mat3Di, q[i].q3Di, q[i].cb3Di_rev, q[i].L, true, pr.sR);
    if (hasAA) { sw3Materialize(matAA, q[i].qAA, q[i].cbAA_fwd, q[i].L, false, pr.aF); sw3Materialize(matAA, q[i].qAA, q[i].cbAA_rev, q[i].L, true, pr.aR); }
}

int sw3Validate(fsgpu_ctx *ctx, Sw3Plan &p) {
    int rc;
    if ((rc = swCheckCall(ctx, p.gapOpen, p.gapExtend)) != FSGPU_OK) return rc;
    const std::string who = p.who;
    if (p.nq > 65535) { ctx->err = who + ": more than 65535 queries in one call"; return FSGPU_E_ARG; }
    if (p.hasAA && !ctx->db->hasAA) { ctx->err = "AA matrix given but the database was loaded without AA sequences"; return FSGPU_E_NODB; }
    const fsgpu_sw_cquery *q = p.q;
    p.base.assign(p.nq + 1, 0);
    for (int i = 0; i < p.nq; i++) {
        // the score source: four tables or the two 3Di ones, the same for every query of the call (any int8 is a score) / codes below 21
        const bool src = p.pq ? p.pq[i].p3Di_fwd && p.pq[i].p3Di_rev && (p.pq[i].pAA_fwd != nullptr) == p.hasAA && (p.pq[i].pAA_rev != nullptr) == p.hasAA
                              : q[i].q3Di && (!p.hasAA || q[i].qAA);
        if (!src || q[i].L <= 0 || q[i].L > FSGPU_MAX_SEQ_LEN || q[i].n < 0 || (q[i].n > 0 && !q[i].targetIds)) { ctx->err = who + ": bad query"; return FSGPU_E_ARG; }
        if (!p.pq)
            for (int k = 0; k < q[i].L; k++) if (q[i].q3Di[k] >= kAlphabet || (p.hasAA && q[i].qAA[k] >= kAlphabet)) { ctx->err = who + ": residue code out of range"; return FSGPU_E_ARG; }
        p.base[i + 1] = p.base[i] + (size_t) q[i].n;
        if ((rc = swCheckPairs(ctx, p.who, q[i].targetIds, q[i].n, p.sel != nullptr, p.sel ? p.sel[i] : nullptr, p.nSelAll(i))) != FSGPU_OK) return rc;
    }
    return FSGPU_OK;
}

// ---- queries outside k_sw3's classes: the profile-based path, all of them in one sub-call (the same set in both directions) ----
void sw3Classify(Sw3Plan &p) {
    p.cR.assign(p.nq, 0);
    p.classic.clear();
    for (int i = 0; i < p.nq; i++) { int hl; if (!sw3Class(p.q[i].L, p.cR[i], hl)) { p.cR[i] = 0; p.classic.push_back(i); } }
}
int sw3Classic(fsgpu_ctx *ctx, Sw3Plan &p) {
    const fsgpu_sw_cquery *q = p.q;
    sw3Classify(p);
    if (p.classic.empty()) return FSGPU_OK;
    const size_t nc = p.classic.size();
    std::vector<Sw3Prof> prof(nc);
    std::vector<fsgpu_sw_query> cq(nc);
    std::vector<const int32_t *> csel(nc);
    std::vector<int32_t> cnsel(nc);
    size_t ctotal = 0;
    for (size_t c = 0; c < nc; c++) {
        const int i = p.classic[c];
        p.profilesOf(i, prof[c]);
        cq[c].pAA_fwd = p.hasAA ? prof[c].aF.data() : nullptr; cq[c].pAA_rev = p.hasAA ? prof[c].aR.data() : nullptr;
        cq[c].p3Di_fwd = prof[c].sF.data(); cq[c].p3Di_rev = prof[c].sR.data();
        cq[c].L = q[i].L; cq[c].n = q[i].n; cq[c].targetIds = q[i].targetIds;
        csel[c] = p.sel ? p.sel[i] : nullptr; cnsel[c] = p.sel ? p.nsel[i] : 0;
        ctotal += (size_t) q[i].n;
    }
    std::vector<fsgpu_swres> cout(std::max<size_t>(ctotal, 1));
    for (int d = 0; d < p.nDirs; d++) {
        const int cs = p.dir0 + d;
        const int rc = fsgpu_sw_multi_dir(ctx, cq.data(), (int) nc, p.gapOpen, p.gapExtend, cs, p.sel ? csel.data() : nullptr, p.sel ? cnsel.data() : nullptr, cout.data());
        if (rc != FSGPU_OK) return rc;
        // the sub-call's pass belongs to this submission's accounting (fsgpu_sw_last_passes): it is reset and re-recorded for the k_sw3 launches
        double pp[8];
        fsgpu_sw_last_passes(ctx, pp);
        if (pp[cs * 4] >= 0) { p.clMs += pp[cs * 4]; p.clCells += pp[cs * 4 + 1]; p.clPairs += pp[cs * 4 + 2]; p.clSteps += pp[cs * 4 + 3]; }
        fsgpu_swres *dst = d == 0 ? p.out : p.out2;
        size_t cb = 0;
        for (size_t c = 0; c < nc; c++) {
            const int i = p.classic[c];
            for (int k = 0; k < p.nSelAll(i); k++) { const int j = p.selIdx(i, k); dst[p.base[i] + j] = cout[cb + j]; }
            cb += (size_t) q[i].n;
        }
    }
    return FSGPU_OK;
}

// Target ids of the pass, longest first inside a query, and the split of every query's sorted list into the three shapes.
// A query of up to 512 rows has two shapes: 32 lanes per target pair (R32 = ceil(L / 32) rows per lane, four targets per wave: fewest
// instructions per cell) and 64 lanes (R64 = ceil(L / 64), two targets per wave: half the instructions per target COLUMN).  A wave's
// run time is (columns + lanes - 1) steps of ~(14 R + 16) dependent-ish instructions, so the longest targets of a launch set its
// critical path: pairs whose target is longer than the threshold take the 64-lane shape, the others the 32-lane one.
// (32 queries x 1000 random targets, forward pass alone on the device: thresholds 384 / 640 / 896 / none = 1.21 / 1.20 / 1.20 / 1.21 ms for 3Di,
// 1.37 / 1.30 / 1.28 / 1.31 ms for 3Di + AA -- the split matters little once all classes share a launch; FSGPU_SW3_LONG overrides it)
// Round 6: a third shape, 16 lanes per target pair (eight targets per wave, up to 24 rows per lane), for queries of up to 384 rows: least
// fill / drain, bookkeeping and row padding per cell, but twice the run time per target column of the 32-lane shape -- it takes the pairs
// whose target has at most FSGPU_SW3_MID columns (0 switches the shape off).
// Measured (tools/sw2_probe.py N, forward pass alone, fraction of the issue bound without / with the 16-lane shape): N = 32 queries x 1000 targets
// 0.57 / 0.49, 64: 0.67 / 0.59, 128: 0.69 / 0.72, 256: 0.72 / 0.75 (3Di; 3Di + AA the same picture) -- its waves are half as many and twice as
// long, which a launch of one or two rounds of waves pays for in its tail.  All-vs-all's lists of ~8 pairs per query want the opposite: the LDS
// image of a query (34-45 KB with AA) admits three workgroups per CU whatever the shape, so the shape with the MOST waves per pair keeps the SIMDs
// busiest (a batch of 1024 queries solo: 16 lanes 1.42 ms, 32 lanes 1.03 ms, 64 lanes 0.88 ms).  Hence the automatic rule: a call whose lists
// hold at most 16 pairs on average runs with 64 lanes per pair throughout; the 16-lane shape is taken when the call holds at least 100 000 pairs.
// FSGPU_SW3_MID=<columns> forces the 16-lane shape for every query (0: never), FSGPU_SW3_SHORT=<pairs> moves the short-list limit (0: off).
void sw3SortAndSplit(fsgpu_ctx *ctx, Sw3Plan &p) {
    static const int longT = [] { const char *e = getenv("FSGPU_SW3_LONG"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 896; }();
    const int midEnv = [] { const char *e = getenv("FSGPU_SW3_MID"); return e && *e ? atoi(e) : -1; }();      // read per call: the tests switch shapes inside one process
    const int midT = midEnv >= 0 ? midEnv : 512;
    const int shortList = [] { const char *e = getenv("FSGPU_SW3_SHORT"); return e && *e ? atoi(e) : 16; }();
    static const int maxR16 = [] { const char *e = getenv("FSGPU_SW3_MAXR16"); const int v = e ? atoi(e) : 0; return v > 0 && v <= kSw3MaxR16 ? v : kSw3MaxR16; }();
    const std::vector<int32_t> &len = ctx->db->hLengths;
    const fsgpu_sw_cquery *q = p.q;
    if (!p.allOrder) p.perm.resize(p.total);
    p.nLong.assign(p.nq, 0); p.nMid.assign(p.nq, 0);
    // the short-list rule is per CALL (mean pairs per query of the call): a per-query rule left all-vs-all's batches with 64-lane groups for the short
    // lists AND 32-lane groups for the others -- 1.29 ms per batch against 0.88 ms with one shape for the whole call
    size_t nActive = 0;
    for (int i = 0; i < p.nq; i++) if (p.nSel(i) > 0) nActive++;
    const bool callShort = shortList > 0 && nActive > 0 && p.total <= (size_t) shortList * nActive;
    std::vector<uint64_t> lkey;
    // the presorted order: the targets above a threshold are a prefix of it
    auto longerThan = [&](int t) { return (int) (std::partition_point(p.allOrder, p.allOrder + p.allN, [&](uint32_t id) { return len[id] > t; }) - p.allOrder); };
    const int allLong = p.allOrder ? longerThan(longT) : 0, allMid = p.allOrder ? longerThan(midT) - std::min(allLong, longerThan(midT)) : 0;
    for (int i = 0; i < p.nq; i++) {
        const int ns = p.nSel(i);
        if (ns == 0) continue;
        int nl = allLong, nm = allMid;
        if (!p.allOrder) {
            uint32_t *pm = p.perm.data() + p.sbase[i];
            swSortLongestFirst(len, q[i].targetIds, p.sel ? p.sel[i] : nullptr, ns, lkey, pm);
            for (int k = 0; k < ns; k++) { const int lt = len[q[i].targetIds[pm[k]]]; if (lt > longT) nl++; else if (lt > midT) nm++; }
        }
        p.nLong[i] = (q[i].L > 32 * kSw3MaxR || callShort) ? ns : nl;
        const bool shape16 = q[i].L <= 16 * maxR16 && midT > 0 && (midEnv >= 0 || p.total >= 100000);
        p.nMid[i] = p.nLong[i] == ns ? 0 : shape16 ? nm : ns - p.nLong[i];
    }
}

// images: built once per set of queries (the reversed call of a forward call finds them in place)
int sw3Images(fsgpu_ctx *ctx, const Sw3Plan &p) {
    const fsgpu_sw_cquery *q = p.q;
    const int nq = p.nq;
    const bool hasAA = p.hasAA;
    int rc;
    // what an image is made of, all of it: for compact queries the matrices, codes and biases, for profile queries every byte of their tables; the
    // kind is part of the key, so a profile call never finds the images of a compact call of the same lengths in place, nor the other way round
    const bool prof = p.pq != nullptr;
    const std::string who = p.who;
    uint64_t sig = 0xcbf29ce484222325ull ^ (uint64_t) nq ^ ((uint64_t) hasAA << 40) ^ ((uint64_t) prof << 41);
    if (!prof) {
        sig = hashWords(sig, p.mat3Di, kAlphabet * kAlphabet);
        if (hasAA) sig = hashWords(sig, p.matAA, kAlphabet * kAlphabet);
    }
    // bytes a query ships to the builder: [q3Di][qAA][four bias vectors], or its tables in the order k_sw3_image_profile reads them
    auto tablesOf = [&](int i, const int8_t *(&t)[4]) { t[0] = p.pq[i].p3Di_fwd; t[1] = hasAA ? p.pq[i].pAA_fwd : p.pq[i].p3Di_rev; t[2] = p.pq[i].p3Di_rev; t[3] = p.pq[i].pAA_rev; return hasAA ? 4 : 2; };
    auto dataBytesOf = [&](int i) { return ((prof ? (size_t) (hasAA ? 4 : 2) * kAlphabet : (size_t) 6) * q[i].L + 15) / 16 * 16; };
    for (int i = 0; i < nq; i++) {
        if (p.cR[i] == 0) continue;
        const size_t L = (size_t) q[i].L;
        if (prof) {
            const int8_t *t[4];
            const int nt = tablesOf(i, t);
            sig ^= (uint64_t) i * 0x9E3779B97F4A7C15ull ^ L;
            for (int c = 0; c < nt; c++) sig = hashWords(sig, t[c], (size_t) kAlphabet * L);
            continue;
        }
        sig = hashWords(sig ^ (uint64_t) i * 0x9E3779B97F4A7C15ull ^ L, q[i].q3Di, L);
        if (hasAA) sig = hashWords(sig, q[i].qAA, L);
        const int8_t *cbs[4] = {q[i].cb3Di_fwd, q[i].cbAA_fwd, q[i].cb3Di_rev, q[i].cbAA_rev};
        for (int c = 0; c < 4; c++) { if (cbs[c]) sig = hashWords(sig, cbs[c], L); else sig = (sig ^ 0x55) * 0x100000001B3ull; }
    }
    if (!sig) sig = 1;
    bool haveImages = ctx->s3Sig == sig && (int) ctx->s3ImgOff.size() == 3 * nq;
    for (int i = 0; i < nq && haveImages; i++)
        for (int shape = 0; shape < 3; shape++) if (p.nShape(i, shape) > 0 && ctx->s3ImgOff[3 * i + shape] == 0xffffffffu) haveImages = false;
    if (haveImages) return FSGPU_OK;
    ctx->s3Sig = 0;
    ctx->s3ImgOff.assign((size_t) 3 * nq, 0xffffffffu);       // [3 i + shape]: image of query i for 16 / 32 / 64 lanes per target pair
    size_t imgDw = 0, dataBytes = 0;
    int nImg = 0, maxDw = 0;
    for (int i = 0; i < nq; i++) {
        if (p.nSel(i) == 0) continue;
        for (int shape = 0; shape < 3; shape++) {
            if (p.nShape(i, shape) == 0) continue;
            const int HL = kShapeHL[shape], R = (q[i].L + HL - 1) / HL;
            const size_t one = (size_t) 2 * sw3ImageBytes(R, HL, hasAA) / 4;
            if (imgDw + one >= (1ull << 32)) { ctx->err = who + ": images of one call exceed 16 GiB"; return FSGPU_E_NOMEM; }
            ctx->s3ImgOff[3 * i + shape] = (uint32_t) imgDw; imgDw += one; maxDw = std::max(maxDw, (int) one);
            nImg++;
        }
        dataBytes += dataBytesOf(i);
    }
    const size_t descBytes = ((size_t) nImg * sizeof(Sw3ImgQuery) + 15) / 16 * 16, matOff = descBytes, dataOff0 = matOff + 1024;
    if ((rc = ensurePinned(ctx, ctx->hS3build, dataOff0 + dataBytes)) != FSGPU_OK) return rc;
    if ((rc = ensureAll(ctx, {{ctx->s3build, dataOff0 + dataBytes}, {ctx->s3img, imgDw * 4}})) != FSGPU_OK) return rc;
    unsigned char *hb = (unsigned char *) ctx->hS3build.p;
    Sw3ImgQuery *hd = (Sw3ImgQuery *) hb;
    if (!prof) memcpy(hb + matOff, p.mat3Di, kAlphabet * kAlphabet);
    if (!prof && hasAA) memcpy(hb + matOff + 512, p.matAA, kAlphabet * kAlphabet);
    size_t dpos = dataOff0;
    int k = 0;
    for (int i = 0; i < nq; i++) {
        if (p.nSel(i) == 0) continue;
        const size_t L = (size_t) q[i].L;
        for (int shape = 0; shape < 3; shape++) {
            if (ctx->s3ImgOff[3 * i + shape] == 0xffffffffu) continue;
            const int HL = kShapeHL[shape];
            hd[k].imgOff = ctx->s3ImgOff[3 * i + shape]; hd[k].dataOff = (uint32_t) (dpos - dataOff0); hd[k].L = (uint32_t) L;
            hd[k].R = (uint16_t) ((L + HL - 1) / HL); hd[k].HL = (uint16_t) HL;
            k++;
        }
        unsigned char *d = hb + dpos;
        if (prof) {
            const int8_t *t[4];
            const int nt = tablesOf(i, t);
            for (int c = 0; c < nt; c++) memcpy(d + (size_t) c * kAlphabet * L, t[c], (size_t) kAlphabet * L);
        } else {
            memcpy(d, q[i].q3Di, L);
            if (hasAA) memcpy(d + L, q[i].qAA, L); else memset(d + L, 0, L);
            const int8_t *cbs[4] = {q[i].cb3Di_fwd, q[i].cbAA_fwd, q[i].cb3Di_rev, q[i].cbAA_rev};
            for (int c = 0; c < 4; c++) { if (cbs[c]) memcpy(d + (2 + c) * L, cbs[c], L); else memset(d + (2 + c) * L, 0, L); }
        }
        dpos += dataBytesOf(i);
        if (dpos - dataOff0 >= (1ull << 32)) { ctx->err = who + ": query data of one call exceeds 4 GiB"; return FSGPU_E_NOMEM; }
    }
    HIPCHK(hipMemcpyAsync(ctx->s3build.p, hb, dpos, hipMemcpyHostToDevice, p.S));
    const unsigned char *db = (const unsigned char *) ctx->s3build.p;
    rc = prof ? fsgpuLaunchSw3ImageProfile(ctx, (const Sw3ImgQuery *) db, nImg, maxDw, (const int8_t *) (db + dataOff0), (uint32_t *) ctx->s3img.p, hasAA, p.S)
              : fsgpuLaunchSw3Image(ctx, (const Sw3ImgQuery *) db, nImg, maxDw, db + dataOff0, (const int8_t *) (db + matOff), (const int8_t *) (db + matOff + 512),
                                    (uint32_t *) ctx->s3img.p, hasAA, p.S);
    if (rc != FSGPU_OK) return rc;
    ctx->s3Sig = sig;
    ctx->s3Plan[8] += (uint32_t) nImg;
    return FSGPU_OK;
}

void sw3Groups(Sw3Plan &p) {
    const bool hasAA = p.hasAA;
    // launch groups: lanes per target pair x kernel (R = 1..8 / 9..16 / 17..24) x LDS occupancy class of the R range of four (the dynamic LDS of a
    // launch is that of its largest R: a query of 9 rows per lane must not take the 106 KB of one with 16 and lose its second workgroup per CU)
    // (a class whose largest member still fits three workgroups per CU shares its launch with the smaller ones: the register classes of a
    // search batch then run as one or two launches, each with a single long-target tail)
    auto occOf = [&](int HL, int R) { return std::min(3, (160 * 1024) / sw3LdsBytes(std::min(sw3MaxR(HL), (R + 3) / 4 * 4), HL, hasAA, 4)); };
    auto keyOf = [&](int shape, int R) { return shape * 12 + ((R - 1) / 8) * 4 + occOf(kShapeHL[shape], R); };
    for (int i = 0; i < p.nq; i++) {
        if (p.nSel(i) == 0) continue;
        for (int shape = 2; shape >= 0; shape--) {
            if (p.nShape(i, shape) == 0) continue;
            const int R = (p.q[i].L + kShapeHL[shape] - 1) / kShapeHL[shape];
            p.parts.push_back({i, keyOf(shape, R), R, p.firstOfShape(i, shape), p.nShape(i, shape)});
        }
    }
    // (workgroups of one or two waves for lists that fit them -- all-vs-all's ~8 pairs per query -- were measured and lost: 1.30 against 1.08 ms per
    // batch of 1024 solo; the 34 KB image of a workgroup then arrives through 64 lanes, and the extra launch groups queue behind each other)
    for (int key = 35; key >= 0; key--) {           // the 64-lane groups (the long targets) first
        Sw3Plan::Group g{key, kShapeHL[key / 12], ((key % 12) / 4) * 8 + 1, 0, 0, 0, p.nBlocks, 0};
        for (const Sw3Plan::Part &pt : p.parts) if (pt.key == key) g.maxR = std::max(g.maxR, pt.R);
        if (g.maxR == 0) continue;
        g.waves = sw3Waves(g.maxR, g.HL, hasAA);
        g.lds = sw3LdsBytes(g.maxR, g.HL, hasAA, g.waves);
        const size_t ppb = (size_t) g.waves * 2 * (64 / g.HL);
        for (const Sw3Plan::Part &pt : p.parts) if (pt.key == key) g.nblk += ((size_t) pt.n + ppb - 1) / ppb;
        p.nBlocks += g.nblk;
        p.groups.push_back(g);
    }
}

// the view of the plan that fsgpu_sw3_last_plan hands out: counters only, nothing here feeds a launch
void sw3RecordPlan(fsgpu_ctx *ctx, const Sw3Plan &p) {
    uint32_t *o = ctx->s3Plan;
    for (const Sw3Plan::Part &pt : p.parts) {
        const int shape = pt.key / 12;
        o[shape] += (uint32_t) pt.n;
        o[3 + shape] |= 1u << pt.R;
    }
    o[9] += (uint32_t) p.groups.size();           // (+=: the sub-batches of a scan add up; every other call starts from zeroed counters)
    o[10] += (uint32_t) p.nBlocks;
}

// target ids and workgroup descriptors of the pass, with the accounting for fsgpu_sw_last_passes; uploads both
int sw3Descriptors(fsgpu_ctx *ctx, Sw3Plan &p) {
    const fsgpu_sw_cquery *q = p.q;
    const std::vector<int32_t> &len = ctx->db->hLengths;
    const size_t total = p.total;
    int rc;
    p.descOff = (total * 4 + 15) / 16 * 16;
    const size_t passBytes = p.descOff + p.nBlocks * sizeof(SwBlockDesc);
    // presorted: neither the ids nor the records pass through the host, the staging holds the descriptors alone
    const size_t hostOff = p.allOrder ? 0 : p.descOff;
    if ((rc = ensurePinnedAll(ctx, {{ctx->hS3pass, passBytes - p.descOff + hostOff}, {ctx->hS3res, p.allOrder ? 0 : total * 16 * p.nDirs}})) != FSGPU_OK) return rc;
    if ((rc = ensureAll(ctx, {{ctx->s3pass, passBytes}, {ctx->s3res, total * 16 * p.nDirs}})) != FSGPU_OK) return rc;
    uint32_t *hTids = (uint32_t *) ctx->hS3pass.p;
    SwBlockDesc *hBlk = (SwBlockDesc *) ((unsigned char *) ctx->hS3pass.p + hostOff);
    for (int i = 0; i < p.nq && !p.allOrder; i++) {
        const uint32_t *pm = p.perm.data() + p.sbase[i];
        for (int k = 0; k < p.nSel(i); k++) hTids[p.sbase[i] + k] = q[i].targetIds[pm[k]];
    }
    // target id of a pair of the pass (presorted: every query's pairs are the whole order, sbase is a multiple of allN)
    auto tidOfPair = [&](size_t pair) { return p.allOrder ? p.allOrder[pair % (size_t) p.allN] : hTids[pair]; };
    double cells = 0, pairs = 0, winsts = 0;
    for (const Sw3Plan::Group &g : p.groups) {
        const int ppb = g.waves * 2 * (64 / g.HL), ppw = 2 * (64 / g.HL);
        size_t bp = g.blk0;
        for (const Sw3Plan::Part &pt : p.parts) {
            if (pt.key != g.key) continue;
            const int i = pt.q, L = q[i].L, lanes = (L + pt.R - 1) / pt.R;
            for (int p0 = 0; p0 < pt.n; p0 += ppb) {
                SwBlockDesc &d = hBlk[bp++];
                d.imgOff = ctx->s3ImgOff[3 * i + g.key / 12]; d.firstPair = (uint32_t) (p.sbase[i] + pt.first + p0); d.nPairs = (uint16_t) std::min(ppb, pt.n - p0);
                d.rowsInTile = (uint16_t) L; d.segLen = (uint32_t) ((L + 15) / 16);
            }
            // accounting in the units of the kernel's roofline: DP cells and the VALU wave-instructions its waves issue (a wave runs
            // (longest of its targets) + lanes - 1 steps of 14 packed instructions per register row + 16 around them [+ the AA adds])
            const uint32_t *tp = p.allOrder ? p.allOrder + pt.first : hTids + p.sbase[i] + pt.first;
            const double perStep = 14.0 * pt.R + 16.0 + (p.hasAA ? 2.0 * sw3Dw(pt.R) + 4.0 : 0.0);
            for (int k = 0; k < pt.n; k++) {
                const int lt = len[tp[k]];
                cells += (double) L * lt;
                if ((k % ppb) % ppw == 0 && lt > 0) winsts += (double) (lt + lanes - 1) * perStep;
            }
            pairs += pt.n;
        }
        // first pair of a workgroup is its longest: the workgroups with the most work per wave first (steps x instructions per step: a query of 15
        // rows per lane runs twice the instructions per column of one with 7)
        const int hl = g.HL;
        auto work = [&](const SwBlockDesc &x) {
            const long lt = len[tidOfPair(x.firstPair)];
            const long R = ((long) x.rowsInTile + hl - 1) / hl;
            return (lt + hl) * (15 * R + 18);
        };
        std::stable_sort(hBlk + g.blk0, hBlk + g.blk0 + g.nblk, [&](const SwBlockDesc &x, const SwBlockDesc &y) { return work(x) > work(y); });
    }
    ctx->swDirCells[p.slot] = p.clCells + cells * p.nDirs; ctx->swDirPairs[p.slot] = p.clPairs + pairs * p.nDirs; ctx->swDirWaveSteps[p.slot] = p.clSteps + winsts * p.nDirs;
    HIPCHK(hipMemcpyAsync((unsigned char *) ctx->s3pass.p + p.descOff - hostOff, ctx->hS3pass.p, passBytes - p.descOff + hostOff, hipMemcpyHostToDevice, p.S));
    return FSGPU_OK;
}

// Every launch group gets a stream: their long-target tails overlap instead of queueing up
// ... and, in the one-submission form, the two directions of a group: the forward and the reversed-query launch of all-vs-all's batches are one round of
// waves each (0.69 ms apiece for 1024 queries x 8 pairs, the wavefront of the longest target) and ran one behind the other on the group's stream
int sw3Launch(fsgpu_ctx *ctx, const Sw3Plan &p) {
    hipStream_t S = p.S;
    int rc;
    if (p.slot == 0 || !ctx->evValid[1]) HIPCHK(hipEventRecord(ctx->ev[2], S));
    HIPCHK(hipEventRecord(ctx->swDirEv[2 * p.slot], S));
    const size_t nLaunches = p.groups.size() * (size_t) p.nDirs;
    const size_t nStreams = std::min<size_t>(nLaunches, (size_t) fsgpu_ctx::kSwAux);
    if ((rc = swFork(ctx, S, nStreams)) != FSGPU_OK) return rc;
    for (size_t gx = 0; gx < nLaunches; gx++) {
        const Sw3Plan::Group &g = p.groups[gx % p.groups.size()];
        const int d = (int) (gx / p.groups.size());
        const size_t k = gx % nStreams;
        hipStream_t gs = k == 0 ? S : ctx->swAux[k];
        Sw3Args sa;
        sa.aa = ctx->db->alnAA; sa.ss = ctx->db->aln3di; sa.offsets = ctx->db->dOffsets; sa.lengths = ctx->db->dLengths;
        sa.targetIds = (const uint32_t *) ctx->s3pass.p;
        sa.img = (const uint32_t *) ctx->s3img.p;
        sa.blocks = (const SwBlockDesc *) ((const unsigned char *) ctx->s3pass.p + p.descOff) + g.blk0;
        sa.go = (uint32_t) p.gapOpen | ((uint32_t) p.gapOpen << 16);
        sa.ge = (uint32_t) p.gapExtend | ((uint32_t) p.gapExtend << 16);
        sa.dir = p.dir0 + d;
        sa.res0 = (int32_t *) ctx->s3res.p + (size_t) d * p.total * 4;
        rc = p.hasAA ? fsgpuLaunchSw3AA(ctx, g.rlo, g.HL, sa, (int) g.nblk, g.waves, g.lds, gs) : fsgpuLaunchSw3NA(ctx, g.rlo, g.HL, sa, (int) g.nblk, g.waves, g.lds, gs);
        if (rc != FSGPU_OK) return rc;
    }
    if ((rc = swJoin(ctx, S, nStreams)) != FSGPU_OK) return rc;
    HIPCHK(hipEventRecord(ctx->ev[3], S));
    HIPCHK(hipEventRecord(ctx->swDirEv[2 * p.slot + 1], S));
    ctx->swDirValid[p.slot] = true;
    ctx->evValid[1] = true;
    return FSGPU_OK;
}

int sw3BeginPass(fsgpu_ctx *ctx, Sw3Plan &p) {
    p.sbase.assign(p.nq + 1, 0);
    for (int i = 0; i < p.nq; i++) p.sbase[i + 1] = p.sbase[i] + (size_t) p.nSel(i);
    p.total = p.sbase[p.nq];
    if (!ctx->swDirEv[3]) for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&ctx->swDirEv[i]));
    ctx->swDirValid[p.slot] = false;
    if (p.slot == 0) ctx->swDirValid[1] = false;
    ctx->swDirCells[p.slot] = p.clCells; ctx->swDirPairs[p.slot] = p.clPairs; ctx->swDirWaveSteps[p.slot] = p.clSteps;
    ctx->swDirExtraMs[p.slot] = p.clMs;
    return FSGPU_OK;
}

static int sw3Collect(fsgpu_ctx *ctx, const Sw3Plan &p) {
    HIPCHK(hipMemcpyAsync(ctx->hS3res.p, ctx->s3res.p, p.total * 16 * p.nDirs, hipMemcpyDeviceToHost, p.S));
    const int rc = syncStreamOf(ctx, p.S);
    if (rc != FSGPU_OK) return rc;
    for (int d = 0; d < p.nDirs; d++) {
        const fsgpu_swres *r0 = (const fsgpu_swres *) ctx->hS3res.p + (size_t) d * p.total;
        fsgpu_swres *dst = d == 0 ? p.out : p.out2;
        for (int i = 0; i < p.nq; i++)
            for (int k = 0; k < p.nSel(i); k++) dst[p.base[i] + p.perm[p.sbase[i] + k]] = r0[p.sbase[i] + k];
    }
    return FSGPU_OK;
}

// int16-saturated pairs: the single-query path re-runs them with the int32 kernel (computes both directions, keeps `dir`)
static int sw3RerunSaturated(fsgpu_ctx *ctx, const Sw3Plan &p) {
    const fsgpu_sw_cquery *q = p.q;
    fsgpu_swres *out = p.out, *out2 = p.out2;
    std::vector<fsgpu_swres> f2, r2;
    for (int i = 0; i < p.nq; i++) {
        const int ns = p.nSel(i);
        if (ns == 0) continue;
        std::vector<uint32_t> ids;
        std::vector<int> where;
        for (int k = 0; k < ns; k++) {
            const int j = p.selIdx(i, k);
            if (out[p.base[i] + j].score == 32767 || (p.dir == 2 && out2[p.base[i] + j].score == 32767)) { ids.push_back(q[i].targetIds[j]); where.push_back(j); }
        }
        if (ids.empty()) continue;
        ctx->s3Plan[7] += (uint32_t) ids.size();
        Sw3Prof pr;
        p.profilesOf(i, pr);
        f2.resize(ids.size()); r2.resize(ids.size());
        const int rc = fsgpu_sw_batch(ctx, p.hasAA ? pr.aF.data() : nullptr, pr.sF.data(), p.hasAA ? pr.aR.data() : nullptr, pr.sR.data(), q[i].L, ids.data(), (int) ids.size(),
                                      p.gapOpen, p.gapExtend, f2.data(), r2.data());
        if (rc != FSGPU_OK) return rc;
        for (size_t k = 0; k < ids.size(); k++) {
            if (p.dir == 2) {           // only the saturated direction is replaced (the other one's int16 result stands, as in two separate passes)
                if (out[p.base[i] + where[k]].score == 32767) out[p.base[i] + where[k]] = f2[k];
                if (out2[p.base[i] + where[k]].score == 32767) out2[p.base[i] + where[k]] = r2[k];
            } else out[p.base[i] + where[k]] = p.dir == 0 ? f2[k] : r2[k];
        }
    }
    return FSGPU_OK;
}

// one submission of a filled-in plan (who, the score source, q, nq, gap costs, dir, sel / nsel, out / out2, hasAA)
static int sw3Run(fsgpu_ctx *ctx, Sw3Plan &p) {
    const int dir = p.dir;
    p.slot = dir == 1 ? 1 : 0; p.nDirs = dir == 2 ? 2 : 1; p.dir0 = dir == 2 ? 0 : dir;
    p.S = ctx->swHi ? ctx->swHi : ctx->stream;
    int rc;
    if ((rc = sw3Validate(ctx, p)) != FSGPU_OK) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    Sw3Drain drain{ctx, p.S};
    memset(ctx->s3Plan, 0, sizeof(ctx->s3Plan));
    if ((rc = sw3Classic(ctx, p)) != FSGPU_OK) return rc;
    for (int i : p.classic) ctx->s3Plan[6] += (uint32_t) p.nSelAll(i);
    if ((rc = sw3BeginPass(ctx, p)) != FSGPU_OK) return rc;
    if (p.total == 0) {
        if (!p.classic.empty()) {          // every query of the call was row-tiled: an empty k_sw3 interval carries the sub-call's figures
            HIPCHK(hipEventRecord(ctx->swDirEv[2 * p.slot], p.S)); HIPCHK(hipEventRecord(ctx->swDirEv[2 * p.slot + 1], p.S));
            if ((rc = syncStreamOf(ctx, p.S)) != FSGPU_OK) return rc;
            ctx->swDirValid[p.slot] = true;
        }
        drain.ok = true;
        return FSGPU_OK;
    }
    sw3SortAndSplit(ctx, p);
    if ((rc = sw3Images(ctx, p)) != FSGPU_OK) return rc;
    sw3Groups(p);
    sw3RecordPlan(ctx, p);
    if ((rc = sw3Descriptors(ctx, p)) != FSGPU_OK) return rc;
    if ((rc = sw3Launch(ctx, p)) != FSGPU_OK) return rc;
    if ((rc = sw3Collect(ctx, p)) != FSGPU_OK) return rc;
    if ((rc = sw3RerunSaturated(ctx, p)) != FSGPU_OK) return rc;
    drain.ok = true;
    return FSGPU_OK;
}

static int sw3MultiImpl(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend, int dir,
                        const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out, fsgpu_swres *out2) {
    if (!ctx || !mat3Di || nq < 0 || (nq > 0 && (!q || !out)) || dir < 0 || dir > 2 || (dir == 2 && nq > 0 && !out2) || ((sel == nullptr) != (nsel == nullptr))) return FSGPU_E_ARG;
    Sw3Plan p;
    p.mat3Di = mat3Di; p.matAA = matAA; p.q = q; p.nq = nq; p.gapOpen = gapOpen; p.gapExtend = gapExtend; p.dir = dir;
    p.sel = sel; p.nsel = nsel; p.out = out; p.out2 = out2;
    p.hasAA = matAA != nullptr;
    return sw3Run(ctx, p);
}

// profile queries: the plan's q[] carries their L, n and targetIds, the tables stay where the caller has them
static int sw3MultiImplP(fsgpu_ctx *ctx, const char *who, const fsgpu_sw_pquery *pq, int nq, int gapOpen, int gapExtend, int dir,
                         const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out, fsgpu_swres *out2) {
    if (!ctx || nq < 0 || (nq > 0 && (!pq || !out)) || dir < 0 || dir > 2 || (dir == 2 && nq > 0 && !out2) || ((sel == nullptr) != (nsel == nullptr))) return FSGPU_E_ARG;
    std::vector<fsgpu_sw_cquery> shadow((size_t) nq);
    for (int i = 0; i < nq; i++) { shadow[i] = fsgpu_sw_cquery{}; shadow[i].L = pq[i].L; shadow[i].n = pq[i].n; shadow[i].targetIds = pq[i].targetIds; }
    Sw3Plan p;
    p.who = who;
    p.mat3Di = p.matAA = nullptr; p.pq = pq; p.q = shadow.data(); p.nq = nq; p.gapOpen = gapOpen; p.gapExtend = gapExtend; p.dir = dir;
    p.sel = sel; p.nsel = nsel; p.out = out; p.out2 = out2;
    p.hasAA = nq > 0 && pq[0].pAA_fwd != nullptr;
    return sw3Run(ctx, p);
}

extern "C" {

int fsgpu_sw_multi_dir_p(fsgpu_ctx *ctx, const fsgpu_sw_pquery *q, int nq, int gapOpen, int gapExtend, int dir,
                         const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out) {
    if (dir != 0 && dir != 1) return FSGPU_E_ARG;
    return sw3MultiImplP(ctx, "fsgpu_sw_multi_dir_p", q, nq, gapOpen, gapExtend, dir, sel, nsel, out, nullptr);
}

int fsgpu_sw_multi_p(fsgpu_ctx *ctx, const fsgpu_sw_pquery *q, int nq, int gapOpen, int gapExtend, fsgpu_swres *fwd, fsgpu_swres *rev) {
    return sw3MultiImplP(ctx, "fsgpu_sw_multi_p", q, nq, gapOpen, gapExtend, 2, nullptr, nullptr, fwd, rev);
}

int fsgpu_sw_multi_dir_c(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend, int dir,
                         const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out) {
    if (dir != 0 && dir != 1) return FSGPU_E_ARG;
    return sw3MultiImpl(ctx, mat3Di, matAA, q, nq, gapOpen, gapExtend, dir, sel, nsel, out, nullptr);
}

int fsgpu_sw_multi_c(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend,
                     fsgpu_swres *fwd, fsgpu_swres *rev) {
    return sw3MultiImpl(ctx, mat3Di, matAA, q, nq, gapOpen, gapExtend, 2, nullptr, nullptr, fwd, rev);
}

void fsgpu_sw3_last_plan(const fsgpu_ctx *ctx, uint32_t *out) {
    if (!out) return;
    for (int i = 0; i < 12; i++) out[i] = ctx ? ctx->s3Plan[i] : 0u;
}

} // extern "C"

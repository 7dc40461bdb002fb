// k_tm_exact.hpp -- TM-score WITH its superposition, approximate and exact (reference: TMaligner::computeAppoximateTMscore / computeExactTMscore,
// F/src/commons/TMaligner.cpp:50-202; TMscore8_search, F/lib/tmalign/TMalign.cpp:225-391; C ABI: fsgpu_tm_superpose_batch in fsgpu_tm.hip).
//
// The building blocks are k_tm.hpp's (same object, same compiler flags: no contraction, correctly rounded division and square root).  What is new:
//   * a lane keeps, next to its best score, the t / u of its first strict improvement and the ordinal of the fragment start that produced it (TmBest);
//   * the exact search (simplify_step 1: every start of every fragment length, about 5.6 n of them; n_it 10; score_fun8 divides by Lnorm) spans many
//     workgroups per hit, so the grid is a host-made list of (task, block of kTmSpBlock starts);
//   * every block writes ONE partial (score, ordinal, t, u); k_tm_sp_finish reduces a task's partials with the reference's rule -- the larger score
//     wins, equal scores go to the smaller ordinal (the reference's strict `>` keeps the first), a NaN never wins -- and applies the fallback chain.
// No atomics; every partial has one writer and the reduction reads them in a fixed order, so nothing depends on the launch order.
//
//   approximate  blocks 0 / 1 of a task: standard_TMscore's / detailed_search_standard's search over ALL starts (step 40, 20 rounds, divisor n), one
//                wave each, as k_tm_search runs them
//   exact        block b: starts [b * kTmSpBlock, (b + 1) * kTmSpBlock) of TMscore8_search (step 1, 10 rounds, divisor Lnorm)
//   both         block nBlocks: KabschFast over all pairs (rmsd; the superposition of last resort)
// t / u of the result: approximate = second search's if it ever beat -1, else the first one's, else the all-pairs Kabsch; exact = the search's, else
// the all-pairs Kabsch.  (The opening detailed_search_standard of computeExactTMscore has no observable effect: every aligned pair passes
// `i >= 0 || d <= score_d8`, and the KabschFast after it overwrites t, u and rmsd0.)
//
// An exact-mode workgroup is kTmSpWaves waves that share the hit's pair coordinates in LDS (24 KB); each wave has its own mask slice (16 KB).  Two waves = 56 KB
// declared; the compiler moves the lanes' small indexed arrays from scratch into LDS on top of that (about 74 KB in all, `make resource-usage`).  Two
// such workgroups fit the 160 KB of a CU, and the registers allow no more either: like k_tm_search this kernel runs one wave per SIMD.  Hits beyond
// kTmLdsPairs read the pairs from the global workspace and keep their masks there, one slice per (block, wave).
#pragma once
#include "k_tm.hpp"

namespace fs {

#pragma clang fp contract(off)

constexpr int kTmSpWaves = 2;                      // waves of an exact-mode workgroup
constexpr int kTmSpBlock = 64 * kTmSpWaves;        // fragment starts of one exact-mode workgroup
constexpr int kTmSpApproxWaves = 1;                // approximate mode: a search has n / 40 + 6 starts or so, one wave covers a hit of 2 300 pairs at once
constexpr int kTmExactRounds = 10;                 // n_it of TMscore8_search

enum : uint32_t { kTmSrcNone = 0, kTmSrcKabsch = 1, kTmSrcSearch1 = 2, kTmSrcSearch2 = 3, kTmSrcExact = 4 };

struct TmSpTask {
    uint64_t partOff;                     // first of this task's nBlocks + 1 partials
    uint64_t maskOff;                     // word offset of its masks [nBlocks + 1][kTmSpWaves][2][words][64] (hits beyond kTmLdsPairs)
    uint32_t nBlocks;                     // search blocks (0 for a task without pairs: it gets no work item at all)
    float lnorm;                          // exact: the divisor of score_fun8
    uint32_t pad[2];
};
struct TmPartial {                        // 64 bytes
    float score;                          // the all-pairs block: the raw rms of KabschFast
    uint32_t ord;
    float t[3], u[9];
    uint32_t pad[2];
};
struct TmSpOut {                          // 64 bytes; fsgpu_tm_result without its pair count
    float score[2];
    float rms;
    uint32_t source;
    float t[3], u[9];
};
struct TmSpWork { uint32_t task, block; };
struct TmSpArgs {
    TmArgs base;                          // queries, tasks, coordinates, backtraces, pairs, masks (base.out is not used)
    const TmSpTask *sp;
    const TmSpWork *work;
    TmPartial *parts;
    TmSpOut *res;
    uint32_t exact;
};

// the reference's rule between two candidates (neither score is ever NaN: a lane's best only moves through `>`)
TM_HD bool tmBeats(float s, uint32_t o, float bs, uint32_t bo) { return s > bs || (s == bs && o < bo); }

#if defined(__HIPCC__)
__device__ inline void tmWritePartial(TmPartial *p, float score, uint32_t ord, const float t[3], const float u[3][3]) {
    p->score = score; p->ord = ord;
    for (int i = 0; i < 3; i++) {
        p->t[i] = t[i];
        for (int j = 0; j < 3; j++) p->u[3 * i + j] = u[i][j];
    }
    p->pad[0] = 0; p->pad[1] = 0;
}

// grid (work items), kWaves waves each: kTmSpWaves in exact mode (a block of kTmSpBlock starts), kTmSpApproxWaves in approximate mode (a whole search)
template <int kWaves>
__global__ __launch_bounds__(64 * kWaves) void k_tm_sp_search(TmSpArgs a) {
    constexpr uint32_t kLanes = 64 * kWaves;
    __shared__ float sC[6 * kTmLdsPairs];
    __shared__ uint32_t sM[kWaves * 2 * kTmLdsWords * 64];
    __shared__ float sRedS[kWaves];
    __shared__ uint32_t sRedO[kWaves];
    const TmSpWork wk = a.work[blockIdx.x];
    const TmTask t = a.base.tasks[wk.task];
    const TmSpTask sp = a.sp[wk.task];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, blk = wk.block, n = t.nPairs;
    TmPartial *part = a.parts + sp.partOff + blk;
    const float *pairs = a.base.pairs + t.pairOff;
    TmView v;
    v.n = n; v.words = (n + 31) / 32; v.ms = 64;
    if (n <= (uint32_t) kTmLdsPairs) {
        for (uint32_t i = tid; i < 6 * n; i += kLanes) sC[i] = pairs[i];
        __syncthreads();
        v.c = sC;
        uint32_t *base = sM + (size_t) wave * 2 * kTmLdsWords * 64;
        v.m[0] = base + lane; v.m[1] = base + (size_t) v.words * 64 + lane;
    } else {
        v.c = pairs;
        uint32_t *base = a.base.masks + sp.maskOff + ((size_t) blk * kTmSpWaves + wave) * 2 * v.words * 64;
        v.m[0] = base + lane; v.m[1] = base + (size_t) v.words * 64 + lane;
    }
    if (blk == sp.nBlocks) {               // KabschFast over all pairs (the whole workgroup takes this branch)
        if (tid == 0) {
            for (uint32_t w = 0; w < v.words; w++) {
                const uint32_t left = n - w * 32;
                v.m[0][(size_t) w * 64] = left >= 32u ? 0xffffffffu : ((1u << left) - 1u);
            }
            float rms, tt[3], uu[3][3];
            tmKabschFast(v, v.m[0], n, rms, tt, uu);
            tmWritePartial(part, rms, kTmNoOrd, tt, uu);
        }
        return;
    }
    const bool exact = a.exact != 0;
    const uint32_t step = exact ? 1u : (uint32_t) kTmStep;
    uint32_t len[6], starts[6];
    const int cnt = tmFragments(n, len, starts, step);
    uint32_t total = 0;
    for (int k = 0; k < cnt; k++) total += starts[k];
    const int which = exact ? 1 : (int) blk;
    const float div = exact ? sp.lnorm : (float) n;
    const int rounds = exact ? kTmExactRounds : kTmRounds;
    uint32_t s = tid, end = total;
    if (exact) {
        s = blk * kLanes + tid;
        const uint32_t lim = (blk + 1) * kLanes;
        end = lim < total ? lim : total;
    }
    TmBest tb;
    tb.score = -1.0f; tb.ord = kTmNoOrd;
    for (int i = 0; i < 3; i++) { tb.t[i] = 0.0f; for (int j = 0; j < 3; j++) tb.u[i][j] = 0.0f; }
    for (; s < end; s += kLanes) {
        uint32_t start, flen;
        tmNthStart(n, cnt, len, starts, s, start, flen, step);
        tmStartT<true>(v, start, flen, t.d0Search[which], t.scoreD8, t.d0[which], div, rounds, tb.score, &tb, s);
    }
    float bs = tb.score;
    uint32_t bo = tb.ord;
    for (int d = 32; d >= 1; d >>= 1) {
        const float os = __shfl_xor(bs, d, 64);
        const uint32_t oo = __shfl_xor(bo, d, 64);
        if (tmBeats(os, oo, bs, bo)) { bs = os; bo = oo; }
    }
    if (lane == 0) { sRedS[wave] = bs; sRedO[wave] = bo; }
    __syncthreads();
    bs = sRedS[0]; bo = sRedO[0];
    for (int w = 1; w < kWaves; w++)
        if (tmBeats(sRedS[w], sRedO[w], bs, bo)) { bs = sRedS[w]; bo = sRedO[w]; }
    // ordinals are unique among the starts, so exactly one lane holds the winner; without one (score_max never left -1) lane 0 says so
    if (bo == kTmNoOrd) { if (tid == 0) tmWritePartial(part, -1.0f, kTmNoOrd, tb.t, tb.u); }
    else if (tb.ord == bo) tmWritePartial(part, tb.score, tb.ord, tb.t, tb.u);
}

// grid (tasks), one wave each: the reduction of a task's partials and the fallback chain
__global__ __launch_bounds__(64) void k_tm_sp_finish(TmSpArgs a) {
    const TmTask t = a.base.tasks[blockIdx.x];
    const TmSpTask sp = a.sp[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    TmSpOut *res = a.res + t.slot;
    if (t.nPairs == 0) {                   // nothing ran: score_max keeps its -1, the rmsd its 0, the superposition is the identity
        if (lane == 0) {
            res->score[0] = -1.0f; res->score[1] = -1.0f; res->rms = 0.0f; res->source = kTmSrcNone;
            for (int i = 0; i < 3; i++) res->t[i] = 0.0f;
            for (int i = 0; i < 9; i++) res->u[i] = (i % 4 == 0) ? 1.0f : 0.0f;
        }
        return;
    }
    const TmPartial *parts = a.parts + sp.partOff;
    const TmPartial *kab = parts + sp.nBlocks;
    const TmPartial *pick = kab;
    uint32_t source = kTmSrcKabsch;
    float s0 = -1.0f, s1 = -1.0f;
    if (a.exact) {
        float bs = -1.0f;
        uint32_t bo = kTmNoOrd, bi = 0;
        for (uint32_t b = lane; b < sp.nBlocks; b += 64) {
            const float ps = parts[b].score;
            const uint32_t po = parts[b].ord;
            if (po != kTmNoOrd && tmBeats(ps, po, bs, bo)) { bs = ps; bo = po; bi = b; }
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const float os = __shfl_xor(bs, d, 64);
            const uint32_t oo = __shfl_xor(bo, d, 64), oi = __shfl_xor(bi, d, 64);
            if (tmBeats(os, oo, bs, bo)) { bs = os; bo = oo; bi = oi; }
        }
        s0 = bs;
        if (bo != kTmNoOrd) { pick = parts + bi; source = kTmSrcExact; }
    } else {
        s0 = parts[0].score; s1 = parts[1].score;
        if (parts[1].ord != kTmNoOrd) { pick = parts + 1; source = kTmSrcSearch2; }
        else if (parts[0].ord != kTmNoOrd) { pick = parts; source = kTmSrcSearch1; }
    }
    if (lane == 0) {
        res->score[0] = s0; res->score[1] = s1; res->rms = kab->score; res->source = source;
        for (int i = 0; i < 3; i++) res->t[i] = pick->t[i];
        for (int i = 0; i < 9; i++) res->u[i] = pick->u[i];
    }
}
#endif

} // namespace fs

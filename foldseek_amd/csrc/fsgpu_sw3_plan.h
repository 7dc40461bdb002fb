// fsgpu_sw3_plan.h -- private: the plan of one k_sw3 submission and the steps that work on it (fsgpu_sw3_multi.hip).  Two callers run them:
// fsgpu_sw_multi_dir_c / fsgpu_sw_multi_c over the target lists of their queries, and fsgpu_sw_scan_c (fsgpu_sw_scan.hip) over ALL targets of the
// database in an order that is sorted once per database.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "fsgpu_ctx.h"

struct Sw3Prof { std::vector<int16_t> aF, sF, aR, sR; };

// One submission: the call's arguments and what the steps below (sw3*, in the order sw3MultiImpl runs them) work out about it.
struct Sw3Plan {
    const char *who = "fsgpu_sw_multi_dir_c";         // the entry, for its messages
    const int8_t *mat3Di, *matAA;
    const fsgpu_sw_cquery *q;
    // profile queries (fsgpu_sw_multi_dir_p / _p): the int8 tables of query i are pq[i]'s; q[i] then carries L, n and targetIds alone (no codes, no
    // biases) and mat3Di / matAA are not read.  What differs is where a score comes from: sw3Validate, profilesOf and sw3Images branch on it.
    const fsgpu_sw_pquery *pq = nullptr;
    int nq, gapOpen, gapExtend, dir;                  // dir 0 / 1: one direction into out; dir 2: both directions in ONE submission (forward into out, reversed into out2)
    const int32_t *const *sel = nullptr;
    const int32_t *nsel = nullptr;
    fsgpu_swres *out = nullptr, *out2 = nullptr;
    bool hasAA;
    int slot, nDirs, dir0;                            // accounting slot of fsgpu_sw_last_passes; directions of the submission and the first of them
    hipStream_t S;                                    // everything of the k_sw3 path: uploads, image build, launches, download
    // "presorted, all targets" (the scan): every query of the plan runs against the allN targets allOrder[0 .. allN), which are longest first already.
    // q[i].n / targetIds are not read, no permutation is kept, and the target ids of the pass are not staged on the host: the caller writes them on the
    // device (allN ids per query, query-major, at the front of s3pass) between sw3Descriptors and sw3Launch, and reads the records from s3res itself.
    const uint32_t *allOrder = nullptr;
    int allN = 0;
    std::vector<size_t> base, sbase;                  // offsets into out[] (all pairs of a query) / into the pass (the selected pairs of the k_sw3 queries)
    size_t total = 0;                                 // pairs of the pass
    std::vector<int> cR;                              // > 0: the query runs through k_sw3
    std::vector<int> classic;                         // the others
    double clMs = 0, clCells = 0, clPairs = 0, clSteps = 0;          // what their sub-call ran (the scan: what its earlier sub-batches ran)
    // pairs [0, nLong) of a query's sorted list (perm) run with 64 lanes, [nLong, nLong + nMid) with 32, the rest with 16
    std::vector<uint32_t> perm;
    std::vector<int> nLong, nMid;
    struct Part { int q, key, R, first, n; };         // pairs [first, first + n) of query q's sorted list run with R rows per lane in launch group `key`
    std::vector<Part> parts;
    struct Group { int key, HL, rlo, maxR, waves, lds; size_t blk0, nblk; };
    std::vector<Group> groups;
    size_t nBlocks = 0, descOff = 0;                  // workgroup descriptors of the pass and their byte offset in s3pass (behind the target ids)

    int nSelAll(int i) const { return allOrder ? allN : sel ? (int) nsel[i] : q[i].n; }
    int selIdx(int i, int k) const { return sel ? sel[i][k] : k; }
    int nSel(int i) const { return cR[i] > 0 ? nSelAll(i) : 0; }
    int nShape(int i, int shape) const { return shape == 2 ? nLong[i] : shape == 1 ? nMid[i] : nSel(i) - nLong[i] - nMid[i]; }
    int firstOfShape(int i, int shape) const { return shape == 2 ? 0 : shape == 1 ? nLong[i] : nLong[i] + nMid[i]; }
    void profilesOf(int i, Sw3Prof &pr) const;
};

int sw3Validate(fsgpu_ctx *ctx, Sw3Plan &p);
void sw3Classify(Sw3Plan &p);                         // cR, classic
int sw3Classic(fsgpu_ctx *ctx, Sw3Plan &p);
int sw3BeginPass(fsgpu_ctx *ctx, Sw3Plan &p);         // sbase, total; the accounting of the pass starts from what cl* hold
void sw3SortAndSplit(fsgpu_ctx *ctx, Sw3Plan &p);
int sw3Images(fsgpu_ctx *ctx, const Sw3Plan &p);
void sw3Groups(Sw3Plan &p);
void sw3RecordPlan(fsgpu_ctx *ctx, const Sw3Plan &p);
int sw3Descriptors(fsgpu_ctx *ctx, Sw3Plan &p);
int sw3Launch(fsgpu_ctx *ctx, const Sw3Plan &p);

// an error return after work was enqueued must not leave copies out of the pinned staging buffers or kernels in flight: the next call (or
// fsgpu_destroy) would refill / free memory that is still being read
struct Sw3Drain {
    fsgpu_ctx *c; hipStream_t s; bool ok = false;
    ~Sw3Drain() { if (ok) return; (void) hipStreamSynchronize(s); for (int i = 0; i < fsgpu_ctx::kSwAux; i++) if (c->swAux[i]) (void) hipStreamSynchronize(c->swAux[i]); (void) hipGetLastError(); }
};

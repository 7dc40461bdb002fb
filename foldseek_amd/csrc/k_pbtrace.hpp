// k_pbtrace.hpp -- start cell and banded trace-back of profile-query hits (include/fsgpu.h: fsgpu_profile_backtrace; host side: fsgpu_pbtrace.hip).
// StructureSmithWaterman::alignStartPosBacktrace<PROFILE> (F/src/commons/StructureSmithWaterman.cpp:540-739) per task (query, target, qEnd, dbEnd, score):
//   k_pbt_reverse   the affine SW recurrence over the reversed profile prefix [0, qEnd] x the reversed target prefix [0, dbEnd], in int32, column by
//                   column, stopped at the first column whose maximum reaches `score` (:1280); the smallest row holding it is the start row
//   k_pbt_band      banded_sw (:1723-1957) over [qStart, qEnd] x [dbStart, dbEnd], band doubled until the best score reaches `score`, the directions of a
//                   cell packed into one byte of the context's scratch, then the trace-back from the end cell and the identity count (:746-773)
// One wave per task, four tasks per workgroup.  Both kernels spread ONE LINE of the matrix over the lanes and walk the other dimension: the reverse pass
// a column (lanes own query rows, 64 at a time), the banded pass a band line (lanes own target columns).  The gap state that runs ALONG the line -- F in the
// source's terms -- is a running maximum, exact while gapOpen > gapExtend >= 1 (a gap opened from a cell that F itself set is dominated by extending that
// F): an inclusive scan of max(v[k] - (l - k) * gapExtend) over the lanes, carried from one 64-lane chunk to the next.  The state of the previous line
// (H and E per cell of the line, 8 bytes) lives in LDS up to kPbtLdsCells cells and in the call's global scratch beyond.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kPbtWaves = 4;               // tasks (waves) of a workgroup
constexpr int kPbtLdsCells = 1024;         // line cells per wave held in LDS: 4 x 1024 x 8 B = 32 KB per workgroup
constexpr int kPbtNeg = -(1 << 29);

struct PbtQuery { uint64_t off; int32_t L, pad; };          // off: bytes into the query blob: [pAA 21 * L][p3Di 21 * L][lettersAA L]
struct PbtTask {
    uint32_t query, target;
    int32_t qEnd, dbEnd, score;
    int32_t qStart, dbStart;               // k_pbt_band: the start cell
    int32_t band, bandCap;                 // k_pbt_band: first band width to try, widest one the direction slice holds
    int32_t slot;                          // result slot of the call
    uint64_t stateOff;                     // int2 cells into the global line state (used when the line is longer than kPbtLdsCells)
    uint64_t dirOff;                       // bytes into the direction scratch
    uint64_t btOff;                        // bytes into the backtrace buffer: a slice of qEnd + dbEnd + 2 + 16 characters
};
struct PbtRes { int32_t status, qStart, dbStart, identicalAA, btLen, band, btStart, pad; };
struct PbtArgs {
    const PbtTask *tasks; int nTasks;
    const PbtQuery *queries; const int8_t *qdata;
    const uint8_t *dbAA, *dbSS; const uint64_t *dbOff;
    int gapOpen, gapExtend;
    int2 *state; uint8_t *dir; char *bt; PbtRes *res;
};

// out[l] = max over k <= l of v[k] - (l - k) * ge
__device__ __forceinline__ int pbtDecayScan(int v, int ge, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64) - d * ge;
        if (lane >= d) v = max(v, t);
    }
    return v;
}
__device__ __forceinline__ int pbtWaveMax(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int pbtWaveMin(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

// ---- the reverse pass.  Row i of the reversed prefix reads profile position qEnd - i of the forward tables, column j target position dbEnd - j.
// res[slot]: status 1 + start cell when the first column that reaches `score` holds exactly `score`, status 2 otherwise.
__global__ __launch_bounds__(kPbtWaves * 64) void k_pbt_reverse(PbtArgs a) {
    __shared__ int2 lds[kPbtWaves][kPbtLdsCells];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * kPbtWaves + wave;
    if (t >= a.nTasks) return;
    const PbtTask tk = a.tasks[t];
    const PbtQuery q = a.queries[tk.query];
    const int L = q.L, rows = tk.qEnd + 1, cols = tk.dbEnd + 1, go = a.gapOpen, ge = a.gapExtend;
    const int8_t *pAA = a.qdata + q.off, *p3 = pAA + (size_t) 21 * L;
    const uint8_t *tA = a.dbAA + a.dbOff[tk.target], *t3 = a.dbSS + a.dbOff[tk.target];
    int2 *st = rows <= kPbtLdsCells ? lds[wave] : a.state + tk.stateOff;
    int status = 2, startRow = 0, startCol = 0;
    int nextA = tA[tk.dbEnd], next3 = t3[tk.dbEnd];                  // the letters of a column are fetched one column ahead
    for (int j = 0; j < cols; j++) {
        const int8_t *lineA = pAA + (size_t) nextA * L + tk.qEnd, *line3 = p3 + (size_t) next3 * L + tk.qEnd;
        if (j + 1 < cols) { nextA = tA[tk.dbEnd - j - 1]; next3 = t3[tk.dbEnd - j - 1]; }
        int carryH = 0;                    // H of the row above this chunk in the previous column: the diagonal of lane 0
        int carryV = kPbtNeg;              // the scan's value at the last row of the chunk above
        int lmax = -1, lrow = 0;
        for (int base = 0; base < rows; base += 64) {
            const int i = base + lane;
            const bool in = i < rows;
            int2 old = make_int2(0, 0);    // (H, E) of this row in the previous column; E is the floored one: >= 0
            if (in && j > 0) old = st[i];
            int up = __shfl_up(old.x, 1, 64);
            if (lane == 0) up = carryH;
            carryH = __shfl(old.x, 63, 64);
            const int s = in ? (int) lineA[-i] + (int) line3[-i] : 0;
            const int h0 = in ? max(up + s, old.y) : kPbtNeg;
            int v = pbtDecayScan(h0, ge, lane);
            v = max(v, carryV - (lane + 1) * ge);
            int ex = __shfl_up(v, 1, 64);
            if (lane == 0) ex = carryV;
            carryV = __shfl(v, 63, 64);
            const int H = max(h0, max(ex - go, 0));
            const int E = max(max(old.y - ge, H - go), 0);
            if (in) {
                st[i] = make_int2(H, E);
                if (H > lmax) { lmax = H; lrow = i; }
            }
        }
        const int m = pbtWaveMax(lmax);
        if (m >= tk.score) {
            startRow = pbtWaveMin(lmax == m ? lrow : 0x7fffffff);
            startCol = j;
            status = m == tk.score ? 1 : 2;
            break;
        }
    }
    if (lane == 0) {
        PbtRes r;
        r.status = status; r.qStart = status == 1 ? tk.qEnd - startRow : -1; r.dbStart = status == 1 ? tk.dbEnd - startCol : -1;
        r.identicalAA = 0; r.btLen = 0; r.band = 0; r.btStart = 0; r.pad = 0;
        a.res[tk.slot] = r;
    }
}

// ---- the banded pass.  Line i covers the columns [max(0, i - band), min(dbLen - 1, i + band)]; a cell outside the band of the line above, and the cell
// left of a line's band, read as H = E = 0; F starts every line at 0; the `edge` slot of the source (h_b[edge] = e_b[edge] = 0, :1783-1784) clears H and E
// of the line above at the last column while the band still starts at column 0 and `end` is clamped.  Direction byte of a cell: bit 0 E came from H
// (code 3, else 2), bit 1 F came from H (code 5, else 4), bits 2-3 where H came from (0 the diagonal: code 1, 1 E, 2 F).
// res[slot]: status 1 + identities + backtrace; 3 no path; 0 with band = the width it would need next: the direction slice is too small for it.
__global__ __launch_bounds__(kPbtWaves * 64) void k_pbt_band(PbtArgs a) {
    __shared__ int2 lds[kPbtWaves][kPbtLdsCells];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * kPbtWaves + wave;
    if (t >= a.nTasks) return;
    const PbtTask tk = a.tasks[t];
    const PbtQuery q = a.queries[tk.query];
    const int L = q.L, go = a.gapOpen, ge = a.gapExtend;
    const int qLen = tk.qEnd - tk.qStart + 1, dbLen = tk.dbEnd - tk.dbStart + 1;
    const int8_t *pAA = a.qdata + q.off + tk.qStart, *p3 = pAA + (size_t) 21 * L;
    const uint8_t *letters = (const uint8_t *) a.qdata + q.off + (size_t) 42 * L + tk.qStart;
    const uint8_t *tA = a.dbAA + a.dbOff[tk.target] + tk.dbStart, *t3 = a.dbSS + a.dbOff[tk.target] + tk.dbStart;
    int2 *st = dbLen <= kPbtLdsCells ? lds[wave] : a.state + tk.stateOff;
    uint8_t *dir = a.dir + tk.dirOff;
    const int maxDim = max(qLen, dbLen);
    int band = tk.band, status = -1, W = 0;
    while (status < 0) {
        W = (int) min((long long) 2 * band + 1, (long long) dbLen);
        int lbest = 0;
        for (int i = 0; i < qLen; i++) {
            const int beg = max(0, i - band), end = (int) min((long long) dbLen - 1, (long long) i + band);
            const int pend = (int) min((long long) dbLen - 1, (long long) i - 1 + band);
            const bool edge = i >= 1 && i <= band + 1 && end == dbLen - 1 && (long long) dbLen - 1 <= (long long) i - 1 + band;
            // The line above was written by other lanes of THIS wave (a column changes lanes as the band moves).  The fence orders them only because one
            // wave owns the task: its accesses go through one CU's LDS and L1 in program order, in LDS and in the global line state alike (lines
            // beyond kPbtLdsCells).  A task spread over several waves or workgroups would need barriers and device-scope visibility instead.
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            int carryD = (i > 0 && beg > 0) ? st[beg - 1].x : 0;       // H of the line above at column beg - 1 (inside its band: beg - 1 is its first column)
            int carryV = 0;                // H left of the band is 0
            int carryH = 0, carryF = 0;    // H and F of the cell left of this chunk
            uint8_t *dline = dir + (size_t) i * W;
            for (int base = beg; base <= end; base += 64) {
                const int j = base + lane;
                const bool in = j <= end;
                int2 old = make_int2(0, 0);
                if (in && i > 0 && j <= pend) old = st[j];
                int diag = __shfl_up(old.x, 1, 64);
                if (lane == 0) diag = carryD;
                carryD = __shfl(old.x, 63, 64);
                const bool cleared = edge && j == end;
                const int hp = cleared ? 0 : old.x, ep = cleared ? 0 : old.y;
                const int t1 = i == 0 ? -go : hp - go, t2 = i == 0 ? -ge : ep - ge;
                const int e = max(t1, t2), de = t1 > t2 ? 1 : 0;
                if (in) diag += (int) pAA[(size_t) tA[j] * L + i] + (int) p3[(size_t) t3[j] * L + i];
                const int e1 = max(e, 0);
                const int h0 = max(e1, diag);
                int v = pbtDecayScan(in ? h0 : kPbtNeg, ge, lane);
                v = max(v, carryV - (lane + 1) * ge);
                int ex = __shfl_up(v, 1, 64);
                if (lane == 0) ex = carryV;
                carryV = __shfl(v, 63, 64);
                // F: opened from a cell of this line (or from the 0 left of the band), or the line's initial F = 0 extended
                const int f = max(ex - go, -(int) min((long long) (j - beg + 1) * ge, (long long) (1 << 29)));
                const int f1 = max(f, 0);
                const int H = max(h0, f1);
                int hl = __shfl_up(H, 1, 64), fl = __shfl_up(f, 1, 64);
                if (lane == 0) { hl = carryH; fl = carryF; }
                carryH = __shfl(H, 63, 64); carryF = __shfl(f, 63, 64);
                const int df = hl - go > fl - ge ? 1 : 0;
                const int sel = max(e1, f1) <= diag ? 0 : (e1 > f1 ? 1 : 2);
                if (in) {
                    st[j] = make_int2(H, e);
                    dline[j - beg] = (uint8_t) (de | (df << 1) | (sel << 2));
                    lbest = max(lbest, H);
                }
            }
        }
        const int best = pbtWaveMax(lbest);
        if (best >= tk.score) status = 1;
        else if (band >= maxDim) status = 3;                          // a band of max(qLen, dbLen) is the rectangle: the score cannot be reached
        else if (2 * (long long) band > (long long) tk.bandCap) { status = 0; band *= 2; }
        else band *= 2;
    }
    // the directions were written by all lanes of this wave and lane 0 reads them: the same single-wave ordering as above (the slices are 256-byte
    // aligned, so no other task's wave shares a cache line with them)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (lane != 0) return;
    PbtRes r;
    r.status = status; r.qStart = tk.qStart; r.dbStart = tk.dbStart; r.identicalAA = 0; r.btLen = 0; r.band = band; r.btStart = 0; r.pad = 0;
    if (status == 1) {
        char *out = a.bt + tk.btOff;
        const int top = qLen + dbLen + 8;
        int pos = top, i = qLen - 1, j = dbLen - 1, state = 2, ids = 0;
        bool ok = true;
        while (i > 0 || j > 0) {
            if (i < 0 || j < 0) { ok = false; break; }
            const int beg = max(0, i - band), end = (int) min((long long) dbLen - 1, (long long) i + band);
            if (j < beg || j > end) { ok = false; break; }
            const int b = dir[(size_t) i * W + (j - beg)];
            const int sel = state == 2 ? (b >> 2) & 3 : state + 1;   // 0 diagonal, 1 the E code, 2 the F code
            if (sel == 0) { ids += tA[j] == letters[i]; i--; j--; state = 2; out[--pos] = 'M'; }
            else if (sel == 1) { i--; state = (b & 1) ? 2 : 0; out[--pos] = 'I'; }
            else if (sel == 2) { j--; state = (b & 2) ? 2 : 1; out[--pos] = 'D'; }
            else { ok = false; break; }
        }
        if (ok) {
            ids += tA[0] == letters[0];
            out[--pos] = 'M';                                         // the cell (0, 0) closes the path (:1916-1933)
            r.identicalAA = ids; r.btLen = top - pos; r.btStart = pos;
        } else r.status = 3;
    }
    a.res[tk.slot] = r;
}

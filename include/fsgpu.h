/*
 * fsgpu.h -- C ABI of the MI355X-native Foldseek hot path (prefilter + structure alignment).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types, never throws, never exits.
 * Every entry point returns 0 on success or a negative FSGPU_E_* code; fsgpu_last_error() gives the text.
 * One context per GPU and per host thread (the reference's single-caller Marv contract,
 * M/src/prefiltering/ungappedprefilter.cpp:124-158,207).
 *
 * Reference interfaces these replace (M/ = lib/mmseqs of the reference tree, F/ = its root):
 *   fsgpu_create / fsgpu_destroy      Marv::Marv / ~Marv                      M/lib/libmarv/src/marv.h:6-27
 *   fsgpu_db_load                     Marv::loadDb + Marv::setDb              M/lib/libmarv/src/marv.h:37-43,
 *                                                                             call site ungappedprefilter.cpp:150-155
 *   fsgpu_db_adopt_device             (none: the reference has no collective; lets the caller hand over a
 *                                      buffer that an RCCL broadcast already placed in HBM)
 *   fsgpu_gapless_scan                Marv::scan                              M/lib/libmarv/src/marv.h:45-51,
 *                                     + the filter/sort tail of runFilterOnCpu ungappedprefilter.cpp:450-470
 *                                     (score semantics = SmithWaterman::ungapped_alignment,
 *                                      M/src/alignment/StripedSmithWaterman.cpp:1817-1876, i.e. capped at 255-bias)
 *   fsgpu_sw_batch                    StructureSmithWaterman::alignScoreEndPos x2 (forward query, reversed query)
 *                                     F/src/commons/StructureSmithWaterman.cpp:263-362, call sites
 *                                     F/src/strucclustutils/structurealign.cpp:46-47,65-67
 *   fsgpu_kmer_index_build            Prefiltering::getIndexTable -> IndexBuilder::fillDatabase + the extended 3-mer matrix
 *                                     M/src/prefiltering/Prefiltering.cpp:544-583,220-225, IndexBuilder.cpp:56-271
 *   fsgpu_kmer_search                 the per-query body of Prefiltering::runSplit = QueryMatcher::matchQuery
 *                                     M/src/prefiltering/Prefiltering.cpp:847-917, QueryMatcher.cpp:103-376
 *   fsgpu_sw_multi / _multi_dir       the same for a batch of queries, one device launch per register class and direction
 *                                     (forward over all pairs, reversed over the pairs alignStructure still needs:
 *                                     F/src/strucclustutils/structurealign.cpp:50-65)
 *   fsgpu_tm_superpose_batch          TMaligner::computeTMscore (both modes) with t / u                  F/src/commons/TMaligner.cpp:50-212
 *   fsgpu_tm_batch                    TMaligner::computeAppoximateTMscore                               F/src/commons/TMaligner.cpp:50-104, F/lib/tmalign
 *   fsgpu_lddt_batch                  LDDTCalculator::initQuery / computeLDDTScore                      F/src/commons/LDDT.cpp:87-215, call sites
 *                                     F/src/strucclustutils/structurealign.cpp:331-341,398-408, structureconvertalis.cpp:770-773
 *   fsgpu_db_broadcast                replication of the resident DB over the GPUs of a node (RCCL), SURVEY 8e
 *   fshost_*                          host-side pieces of the same path that stay on the CPU, exported so the
 *                                     reference-side adapter and the tests can reach them.
 */
#ifndef FSGPU_H
#define FSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSGPU_ALPHABET 21          /* 20 states + X, order ACDEFGHIKLMNPQRSTVWYX (M/src/commons/DBReader.cpp:353-361) */
#define FSGPU_MAX_SEQ_LEN 65535    /* Parameters::maxSeqLen default, M/src/commons/Parameters.cpp:2496 */

enum {
    FSGPU_OK = 0,
    FSGPU_E_ARG = -1,        /* bad argument */
    FSGPU_E_HIP = -2,        /* a HIP runtime call failed (text in fsgpu_last_error) */
    FSGPU_E_NODB = -3,       /* no database loaded / AA part missing */
    FSGPU_E_UNSUPPORTED = -4,/* parameter combination not implemented on the device path */
    FSGPU_E_NOMEM = -5,
    FSGPU_E_OUTPUT = -6      /* the caller's output buffer is too small; the needed sizes were reported, call again */
};

typedef struct fsgpu_ctx fsgpu_ctx;

/* == Marv::Result without the unused end positions (M/lib/libmarv/src/marv.h:16-28): id = target index in the
 * loaded DB (the caller maps it to a key with DBReader::getDbKey), score = gapless diagonal score. */
typedef struct {
    uint32_t id;
    int32_t score;
} fsgpu_hit;

/* == the fields of StructureSmithWaterman::s_align that alignScoreEndPos fills (StructureSmithWaterman.h:84-109):
 * score1, qEndPos1, dbEndPos1 and `word` (1: int16 pass final, 2: int32 re-run because score1 hit INT16_MAX). */
typedef struct {
    int32_t score;
    int32_t qEnd;
    int32_t dbEnd;
    int32_t word;
} fsgpu_swres;

/* ---- context ---------------------------------------------------------------------------------------------- */
int fsgpu_create(int device, fsgpu_ctx **out);
void fsgpu_destroy(fsgpu_ctx *ctx);
const char *fsgpu_last_error(const fsgpu_ctx *ctx); /* ctx may be NULL: returns the last creation error */
/* A second context on the same GPU with its own HIP stream and scratch buffers that SHARES the resident database of
 * `src` (reference counted): lets several host threads keep the device busy, the way the reference runs one aligner
 * object per OpenMP thread over one shared DBReader (F/src/strucclustutils/structurealign.cpp:284-321).
 * What a clone shares, and when: the database AND the k-mer index the source holds AT THE TIME OF THE CALL, both reference counted.  Neither side
 * sees what the other does afterwards: a clone made before fsgpu_kmer_index_build has no index (fsgpu_kmer_search refuses with FSGPU_E_NODB), a
 * clone made after it keeps searching that index, by that index's parameters, when the source builds another one or loads another database; the
 * source may be destroyed while its clones go on.  Everything else is per context, and nothing of it decides an ANSWER: state a context keeps
 * from call to call (kept LDDT norms, SW images and reversed records, batch sizes of the k-mer search, grow-only workspaces) is either keyed by all
 * it depends on or dropped when the database goes (fsgpu_db_load, fsgpu_db_adopt_device).  One context serves one host thread at a time. */
int fsgpu_clone(const fsgpu_ctx *src, fsgpu_ctx **out);
/* One node, several GPUs, one process: replicates the resident database of `src` into the n contexts dst[] created on
 * OTHER devices, one broadcast per buffer over RCCL (xGMI; librccl is loaded on demand) or peer copies when RCCL is
 * not available (FSGPU_NO_RCCL=1 forces that).  *usedRccl (may be NULL) reports which.  Queries then shard over the
 * devices with no further communication (the reference's multi-GPU path shards TARGETS per device and
 * merges top-N lists, M/lib/libmarv/src/cudasw4.cuh:1477-1553 -- not needed when the DB fits every GPU's 288 GB). */
int fsgpu_db_broadcast(fsgpu_ctx *src, fsgpu_ctx **dst, int n, int *usedRccl);
/* librccl alone on this context's device: a one-rank communicator broadcasts 1 MiB in place on the context's stream.  FSGPU_OK when the
 * library loaded and the call sequence of fsgpu_db_broadcast's RCCL branch ran; what a one-GPU box can verify of the replication path. */
int fsgpu_rccl_selfcheck(fsgpu_ctx *ctx);
int fsgpu_device(const fsgpu_ctx *ctx);
int fsgpu_device_count(void);      /* visible HIP devices, 0 when there is none */
/* HIP stream all kernels of this context are launched on (a hipStream_t), for callers that time with events */
void *fsgpu_stream(const fsgpu_ctx *ctx);

/* ---- target database -------------------------------------------------------------------------------------- */
/* data3di/dataAA: the *padded GPU database* byte buffers exactly as makepaddedseqdb writes them
 * (M/src/util/makepaddedseqdb.cpp:59-109): numeric codes 0..20, +32 when soft-masked, entries padded with 20.
 * offsets[n+1] in bytes (offsets[n] = end), lengths[n] = residues per entry (index length - 2).
 * dataAA may be NULL (prefilter only).  Pointers are borrowed for the duration of the call; the DB is copied to HBM
 * and re-tiled there (coalesced 8-target stripes for the scan, plain unmasked copies for the aligner).
 * The table contract.  Every kernel reads data[offsets[t] + col] for col < lengths[t] and nothing else guards it, so the table is checked
 * (fsgpu_db_check_table) before anything is allocated or launched: 0 <= lengths[t] <= FSGPU_MAX_SEQ_LEN, offsets[t] + lengths[t] <= bytes
 * (tested without forming the sum), offsets[n] <= bytes, and no two entries share a byte (the k-mer index build writes a masked copy of every
 * entry in place: two entries over one byte would be two writers).  Nothing else is asked of the layout: entries may lie in any memory
 * order (descending included), at offsets that are no multiple of 4, with no padding at all or with gaps of any size between them -- bytes
 * outside every entry are never read -- and in any order of length (the scan groups the targets by length itself).  An entry may be empty
 * (lengths[t] == 0, any offset up to bytes), and so may the whole buffer (bytes == 0); what the entries answer for such a target is said
 * below.  A bad table is FSGPU_E_ARG with a message that names the first bad entry.  A call that fails -- a refused table, a bad argument
 * (n == 0 is one), a HIP call that fails at any point of the load -- leaves the context WITHOUT a database (every entry then answers
 * FSGPU_E_NODB) and holds no device memory of the attempt; the next good load works.
 * A target without residues: the scan scores it 0; the Smith-Waterman entries answer (0, 0, 0, word 1); fsgpu_diag_rescore answers
 * FSGPU_DIAG_NO_OVERLAP on every diagonal; fsgpu_block_backtrace refuses a task on it (no end cell exists: FSGPU_E_ARG); the k-mer index
 * holds nothing of it.  A database of nothing but such targets loads, scans and aligns like any other; fsgpu_kmer_index_build refuses it
 * by name (FSGPU_E_UNSUPPORTED: nothing to index).
 * Bytes outside 0..20 and 32..52: the scan copy reads every byte above 20 as X; the aligner copies take 32 off a byte of 32 or more and
 * read what is then above 20 as X; the k-mer index's copy does the same and then, with maskLowerCase, reads every byte that was 32 or more as X. */
int fsgpu_db_load(fsgpu_ctx *ctx, const uint8_t *data3di, const uint8_t *dataAA,
                  const uint64_t *offsets, const int32_t *lengths, uint64_t n, uint64_t bytes);
/* Same, but the four buffers already live in this device's HBM (e.g. filled by an RCCL broadcast over xGMI).
 * The caller's writes to them must be COMPLETE before the call (synchronise the stream or device that filled them: the call reads them on
 * the context's own stream and copies the table to the host, ordered against nobody else's work).  The context does not take ownership of
 * them and does not need them after the call returns: they may be overwritten or freed at once.  Same table contract, same refusals. */
int fsgpu_db_adopt_device(fsgpu_ctx *ctx, const void *d_data3di, const void *d_dataAA,
                          const void *d_offsets, const void *d_lengths, uint64_t n, uint64_t bytes);
/* Host-only (no device call): the table contract above for host arrays.  -1 for a good table, else the index of the first bad entry: the
 * lowest t whose length is outside 0 .. FSGPU_MAX_SEQ_LEN, which lies outside the buffer (offsets[t] > bytes || lengths[t] > bytes -
 * offsets[t]), or which begins inside the bytes of another entry (of two entries that begin at one address, the later one; entries
 * without residues hold no byte); n when only offsets[n] > bytes.  A NULL offsets, or a NULL lengths with n > 0, is no table at all: the
 * answer is 0, as for a bad first entry (n == 0 with offsets[0] <= bytes is a good table; the load entries refuse n == 0 themselves). */
int64_t fsgpu_db_check_table(const uint64_t *offsets, const int32_t *lengths, uint64_t n, uint64_t bytes);
uint64_t fsgpu_db_size(const fsgpu_ctx *ctx);      /* entries */
uint64_t fsgpu_db_residues(const fsgpu_ctx *ctx);  /* sum of lengths */

/* ---- prefilter: exhaustive gapless diagonal scan ----------------------------------------------------------- */
/* pssm: int8 [21][L] row-major, pssm[a*L+i] = subMat[a][q_i] + round(compBias_i) -- what runFilterOnGpu hands to
 *       Marv::scan (ungappedprefilter.cpp:195-203).
 * scoreCap: 255 - bias of the CPU path (StripedSmithWaterman.cpp:1397-1406), 0..255; scores are
 *       min(cap, best diagonal run), which is exactly what the uint8 striped kernel returns.
 * Keeps targets with score > minScore (plus identityId if >= 0), orders them by (score desc, id asc)
 * (hit_t::compareHitsByScoreAndId, QueryMatcher.h:38-48) and returns the first maxRes in out[0..*nout). */
int fsgpu_gapless_scan(fsgpu_ctx *ctx, const int8_t *pssm, int L, int scoreCap, int minScore,
                       int64_t identityId, int maxRes, fsgpu_hit *out, int *nout);
/* The same for nq queries with as few device launches as their lengths allow (queries of equal ceil(L / 16) share one
 * launch; the workgroups of one query move in as those of the previous one drain, so the device stays full across
 * queries and a launch's duration is a per-launch figure worth quoting).  out[q * maxRes ...] / nout[q] per query. */
typedef struct {
    const int8_t *pssm;     /* int8 [21][L], as for fsgpu_gapless_scan */
    int32_t L;
    int32_t scoreCap;
    int64_t identityId;     /* target id that is always kept, or -1 */
} fsgpu_gapless_query;
int fsgpu_gapless_scan_multi(fsgpu_ctx *ctx, const fsgpu_gapless_query *q, int nq, int minScore, int maxRes, fsgpu_hit *out, int *nout);
/* scans / queries of the last fsgpu_gapless_scan_multi: one per launch of the device batch plus one per row-tiled query (> 896 residues, run on
 * its own); fsgpu_last_kernel_ms(ctx, 0) then is the device time of all of them together */
int fsgpu_gapless_last_batch(const fsgpu_ctx *ctx, int *launches, int *queries);
/* raw scores of query `queryIndex` of the last fsgpu_gapless_scan_multi call (queries of <= 896 residues); for tests.  Loading a database forgets
 * the call: until the next one the getter refuses (FSGPU_E_ARG) and copies nothing. */
int fsgpu_gapless_scores_multi(fsgpu_ctx *ctx, int queryIndex, uint8_t *scores_out);
/* Raw per-target scores of the last scan (n bytes, already capped); for tests and statistics.  Refuses (FSGPU_E_NODB) and copies nothing when no
 * single-query scan has run on the database that is loaded now. */
int fsgpu_gapless_scores(fsgpu_ctx *ctx, uint8_t *scores_out);
/* Asynchronous halves of fsgpu_gapless_scan for callers that pipeline several queries / time the device part:
 * _launch enqueues profile upload + kernels on the context stream, _finish waits and post-processes. */
/* Host-only planning step of the scan (no device call): the work list for stripes of stripeLen[] 16-column chunks when a
 * column segment needs `overlap` warm-up chunks (= ceil(Lq / 16)) and `waves` waves pull from the queue.  items[i] =
 * stripe << 32 | split << 31 | firstChunk << 16 | endChunk, longest first; *cap = the cut length chosen (minimises
 * max(cut, (work + warm-up work) / waves)).  Returns the number of items (may exceed capacity; nothing beyond it is
 * written).  Exported so that the policy can be tested without a GPU. */
int64_t fsgpu_gapless_plan_items(const uint32_t *stripeLen, uint32_t nStripes, int overlap, double waves, uint64_t *items,
                                 uint64_t capacity, uint32_t *cap);
/* Host-only: the 16-byte device records the scan makes of planned items.  stripeCols[s] = real columns of stripe s (its longest
 * target), stripeLen[s] = ceil(stripeCols[s] / 16).  records[4 i ..] = {stripe, the item's low word, stripe offset in 16-byte units
 * low, trim << 24 | offset high}: trim = stripeCols - 16 * (stripeLen - 1) (1..16) for the item that ends with its stripe's last
 * chunk, 0 for every other.  Returns nItems, or -1 for arguments that do not fit each other. */
int64_t fsgpu_gapless_item_records(const uint64_t *items, uint64_t nItems, const uint32_t *stripeLen, const uint32_t *stripeCols,
                                   uint32_t nStripes, uint32_t *records);
/* Host-only: which queries of one fsgpu_gapless_scan_multi call share registers in the classes 17 .. 36 (two queries in the halves of
 * every register, 16 lanes a target).  classes[i] = ceil(L_i / 16) >= 1.  Per query: launchClass[i] = the class whose launch carries it,
 * record[i] = its record in that launch, half[i] = 0 (query A) or 1 (query B); record = half = -1 and launchClass = its own class: the
 * query is not placed here (a class with one member and no guest, the classes up to 16 and beyond 36).  A class with two or more members gets one launch
 * over its members two by two; the odd member out of a class of three or more may move up, two registers at most, as query B beside the odd
 * member out of another such class or beside a single member (that class's launch then is one record of this kind), chosen so that the
 * fewest records run without a B.  Every class present keeps exactly one launch.  Returns the number of records, or -1 for a bad argument. */
int fsgpu_gapless_pair_halves(const int32_t *classes, int n, int32_t *launchClass, int32_t *record, int32_t *half);
/* Host-only: the shape the scan gives a query of L residues.  *nTiles = 1 and *R = ceil(L / 16) = 1..56 registers for L <= 896 (one piece); beyond
 * that *nTiles = ceil(L / 512) row tiles of equal height, 16 * *R rows each, *R = ceil(ceil(L / *nTiles) / 16) = 22..32.  The register class *R
 * (with the pairing of fsgpu_gapless_scan_multi) names the kernel that runs.  Returns 0, or -1 for L outside 1 .. FSGPU_MAX_SEQ_LEN or a null pointer. */
int fsgpu_gapless_shape(int L, int *nTiles, int *R);
int fsgpu_gapless_launch(fsgpu_ctx *ctx, const int8_t *pssm, int L, int scoreCap, int minScore,
                         int64_t identityId, int maxRes);
int fsgpu_gapless_finish(fsgpu_ctx *ctx, fsgpu_hit *out, int *nout);

/* ---- alignment: dual-profile striped-semantics affine Smith-Waterman, score + end position ----------------- */
/* Profiles are the linear int16 word profiles of StructureSmithWaterman::ssw_init (StructureSmithWaterman.cpp:
 * 1566-1640): pAA[a*L+i] = matAA[a][qAA_i] + cbAA_i, p3Di[a*L+i] = mat3Di[a][q3Di_i] + cbSS_i, a in 0..20,
 * once for the forward query (_fwd) and once built from the reversed query (_rev, structurealign.cpp:345-347).
 * pAA_* may be NULL when the AA matrix is all zero (--alignment-type 0).
 * For every targetIds[k] the call returns alignScoreEndPos(...) of the forward profile in fwd[k] and of the
 * reversed-query profile in rev[k], bit-identical to the AVX2 striped kernels including the int16->int32 re-run.
 * The tables may hold any int16: the column score is the SATURATING int16 sum of the AA and the 3Di entry, as the reference's
 * simdi16_adds makes it (StructureSmithWaterman.cpp:1178), and the plain sum in the int32 re-run (:1410); what the caller has to
 * keep is the int32 pass below 2^31 (min(L, target length) * 65534 at most: any pair of up to 32768 rows or columns).
 * Requires gapOpen > gapExtend >= 0 (Foldseek: 10/1); otherwise FSGPU_E_UNSUPPORTED. */
/* Host-only: the shape the profile path (k_sw / k_sw2) gives a query of L residues.  *nTiles = 1 and *R = the smallest of 1, 2, 3, 4, 6, 8 register
 * rows per lane with 64 * *R >= L for L <= 512; beyond that *nTiles = ceil(L / 512) row tiles of *R = 8.  Returns 0, or -1 for L outside
 * 1 .. FSGPU_MAX_SEQ_LEN or a null pointer. */
int fsgpu_sw_shape(int L, int *nTiles, int *R);
int fsgpu_sw_batch(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd,
                   const int16_t *pAA_rev, const int16_t *p3Di_rev, int L,
                   const uint32_t *targetIds, int n, int gapOpen, int gapExtend,
                   fsgpu_swres *fwd, fsgpu_swres *rev);
/* The same for n EXPLICIT target sequences instead of database entries: tAA / t3Di hold unmasked codes 0..20, entry k at
 * offsets[k] with lengths[k] residues (offsets[n] = total bytes).  structurealign --alt-ali re-aligns a target whose
 * previous alignment range was overwritten with X (F/src/strucclustutils/structurealign.cpp:115-138, 415-429); that
 * sequence exists nowhere in the database.  tAA may be NULL when pAA_* are. */
int fsgpu_sw_batch_seqs(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd, const int16_t *pAA_rev,
                        const int16_t *p3Di_rev, int L, const uint8_t *tAA, const uint8_t *t3Di, const uint64_t *offsets,
                        const int32_t *lengths, int n, int gapOpen, int gapExtend, fsgpu_swres *fwd, fsgpu_swres *rev);
/* Several queries per call (what a host thread of structurealign would do one after the other, structurealign.cpp:322-452):
 * same semantics per query as fsgpu_sw_batch; results are concatenated in query order (sum of n entries).  All queries of
 * at most 512 residues that share a register class run in ONE launch, which fills the device where a single query's
 * ~1000 pairs cannot; longer queries run row-tiled, one launch per tile level for all of them.  Either all or none of the queries carry AA profiles. */
typedef struct {
    const int16_t *pAA_fwd, *p3Di_fwd, *pAA_rev, *p3Di_rev;
    int32_t L;
    int32_t n;
    const uint32_t *targetIds;
} fsgpu_sw_query;
int fsgpu_sw_multi(fsgpu_ctx *ctx, const fsgpu_sw_query *queries, int nq, int gapOpen, int gapExtend,
                   fsgpu_swres *fwd, fsgpu_swres *rev);
/* ONE direction of the same (dir 0: forward-query profiles, 1: reversed-query profiles) for a selection of the pairs:
 * sel[i][0..nsel[i]) are indices into q[i].targetIds (sel = nsel = NULL: every pair).  out has the layout of fwd[] above
 * (all pairs of all queries, concatenated); only the selected entries are written.  structurealign looks at the
 * reversed-query score only for pairs whose forward score passes the coverage and e-value gates
 * (F/src/strucclustutils/structurealign.cpp:55-65): run dir 0 over everything, gate on the host, run dir 1 over the
 * survivors.  Device side: two targets of one query share a wave (int16 halves), half the waves of fsgpu_sw_batch. */
int fsgpu_sw_multi_dir(fsgpu_ctx *ctx, const fsgpu_sw_query *q, int nq, int gapOpen, int gapExtend, int dir,
                       const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out);
/* The same with COMPACT queries.  A structurealign profile is nothing but a matrix column plus a position bias
 * (pAA[a*L+i] = matAA[a][qAA_i] + cbAA_i, StructureSmithWaterman.cpp:1566-1640), so a query is its codes (0..20) and its bias arrays --
 * for the forward query and for the reversed query (cb*_rev[i] belongs to position i of the REVERSED sequence; NULL = all zero) --
 * and the 21 x 21 int8 matrices are passed once: mat[a * 21 + b], matAA = NULL for --alignment-type 0 (then qAA / cbAA_* are not read).
 * The device builds its profile images itself: 6 L bytes per query cross the bus instead of 4 x 21 x L int16 words.  Results, selection
 * and the int16 -> int32 re-run are those of fsgpu_sw_multi_dir; a reversed call (dir 1) over the queries of the preceding forward call
 * finds the images in place.  Device side: queries of up to 512 residues run four targets per wave (32 lanes per target pair), up to
 * 1024 residues two per wave, longer ones row-tiled through the profile-based path. */
typedef struct {
    const uint8_t *qAA, *q3Di;
    const int8_t *cbAA_fwd, *cb3Di_fwd, *cbAA_rev, *cb3Di_rev;
    int32_t L;
    int32_t n;
    const uint32_t *targetIds;
} fsgpu_sw_cquery;
int fsgpu_sw_multi_dir_c(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend,
                         int dir, const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out);
/* Both directions of every pair in ONE submission (one upload, one wait): for batches whose device time is small against a round trip --
 * all-vs-all steps with a handful of hits per query -- computing the reversed-query score of every pair is cheaper than gating on the
 * host between two passes.  fwd / rev as in fsgpu_sw_multi. */
int fsgpu_sw_multi_c(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend,
                     fsgpu_swres *fwd, fsgpu_swres *rev);
/* The same for PROFILE queries (a query database of type DBTYPE_HMM_PROFILE: every round of `search --num-iterations` after the first).
 * The alignment profile of such a query is its own table -- Sequence::mapProfile's profile_score / 4, [letter][position], X row 0
 * (fshost_profile_decode) -- and StructureSmithWaterman::ssw_init takes it as it is (StructureSmithWaterman.cpp:1586-1660: no matrix, no
 * composition bias, word and int profiles are the table widened).  p*[a * L + i], a in 0..20, int8; the _rev tables are the profile reversed
 * position by position.  pAA_* NULL for --alignment-type 0: either all queries of a call carry them or none.  Results, selection, the
 * int16 -> int32 re-run, fsgpu_sw3_last_plan and the gap-cost rule are those of fsgpu_sw_multi_dir_c / fsgpu_sw_multi_c: queries of up
 * to 1024 positions run through the same k_sw3 launches over images built from the tables (k_sw3_image_profile), longer ones are widened
 * to int16 on the host and take fsgpu_sw_multi_dir.  The images a context keeps are keyed by every byte of the tables. */
typedef struct {
    const int8_t *pAA_fwd, *p3Di_fwd, *pAA_rev, *p3Di_rev;
    int32_t L;
    int32_t n;
    const uint32_t *targetIds;
} fsgpu_sw_pquery;
int fsgpu_sw_multi_dir_p(fsgpu_ctx *ctx, const fsgpu_sw_pquery *q, int nq, int gapOpen, int gapExtend, int dir,
                         const int32_t *const *sel, const int32_t *nsel, fsgpu_swres *out);
int fsgpu_sw_multi_p(fsgpu_ctx *ctx, const fsgpu_sw_pquery *q, int nq, int gapOpen, int gapExtend, fsgpu_swres *fwd, fsgpu_swres *rev);
/* Exhaustive search (Foldseek's --exhaustive-search 1 / search --prefilter-mode 2: no prefilter, every target goes to structurealign,
 * F/src/workflow/StructureSearch.cpp:114-127): the forward pass of every query against EVERY target of the database, selected on the device against
 * a score cutoff per query (fshost_evalue_score_cutoff: alignStructure's first e-value gate, structurealign.cpp:55-59).
 * q[] as for fsgpu_sw_multi_dir_c with n = 0 and targetIds = NULL.  For every query i the answer is outIds[outBase[i] .. outBase[i + 1]) in ascending
 * target id with the forward records in outFwd at the same places: exactly what fsgpu_sw_multi_dir_c(dir 0) returns for targetIds = 0 .. N-1,
 * restricted to the pairs with score >= cutoff[i] (the int32 re-run included: its score decides).  An empty target scores 0.
 * cap: room in outIds / outFwd, in records.  When the survivors of the call exceed it the call returns FSGPU_E_OUTPUT: outBase[0 .. nq] holds the
 * offsets that were needed (outBase[nq] = the total), nothing is written at or beyond cap, and the caller may call again with larger buffers.
 * A cutoff outside 0..32767 is FSGPU_E_ARG.  Queries are run in sub-batches of 20 bytes x N per query under a budget of 1 GiB
 * (FSGPU_SCAN_BYTES=<bytes>, read per call); the order of the targets is sorted once per database.  Queries of more than 1024 residues take the
 * profile path in chunks of targets and are filtered on the host: correct, not fast.  fsgpu_sw3_last_plan and fsgpu_sw_last_passes (forward slot)
 * report the whole call. */
int fsgpu_sw_scan_c(fsgpu_ctx *ctx, const int8_t *mat3Di, const int8_t *matAA, const fsgpu_sw_cquery *q, int nq, int gapOpen, int gapExtend,
                    const int32_t *cutoff, uint32_t *outIds, fsgpu_swres *outFwd, uint64_t cap, uint64_t *outBase);
/* out[8] of the last fsgpu_sw_scan_c: [0] sub-batches, [1] records the device selection handed to the host (survivors and int16-saturated pairs),
 * [2] host ms spent planning the sub-batches, [3] survivors, [4] host ms of the whole call, [5..7] 0. */
void fsgpu_sw_scan_last(const fsgpu_ctx *ctx, double *out8);
/* Asynchronous halves of fsgpu_sw_batch.  The four profile arrays and targetIds are BORROWED until fsgpu_sw_finish returns
 * (the int32 re-run of saturated pairs reads the profiles again); after a failed _launch nothing is pending. */
int fsgpu_sw_launch(fsgpu_ctx *ctx, const int16_t *pAA_fwd, const int16_t *p3Di_fwd,
                    const int16_t *pAA_rev, const int16_t *p3Di_rev, int L,
                    const uint32_t *targetIds, int n, int gapOpen, int gapExtend);
int fsgpu_sw_finish(fsgpu_ctx *ctx, fsgpu_swres *fwd, fsgpu_swres *rev);

/* ---- single-diagonal rescoring: Foldseek's structurerescorediagonal (F/src/strucclustutils/structurerescorediagonal.cpp:23-102) ----
 * For every (query, target, diagonal) triple -- what linclust's kmermatcher hands on, prefilter-format lines
 * "targetKey score diagonal" -- the best ungapped run of sub3Di[q][t] + subAA[q][t] along that one diagonal for the forward
 * and for the reversed query.  Targets are entries of the resident database (AA half required), queries are given
 * explicitly: codes 0..20, query k at qOffsets[k] with qLengths[k] residues (qOffsets[nq] = bytes).  mat3Di / matAA: the
 * bit-scaled int16 matrices [21*21] (SubstitutionMatrix(3di.out, 2.1, 0) and (blosum62.out, 1.4 or 0.0, 0)). */
typedef struct {
    uint32_t query;         /* index into the query batch */
    uint32_t target;        /* index in the loaded DB */
    int32_t diagonal;       /* i - j as the prefilter prints it (int16 range) */
} fsgpu_diag_pair;
enum {
    FSGPU_DIAG_OK = 0,
    FSGPU_DIAG_NO_OVERLAP = 1,   /* |diagonal| beyond the sequence, or a target without residues: the reference keeps LocalAlignment's defaults (-1, -1, 0) */
    FSGPU_DIAG_UNDEFINED = 2,    /* negative diagonal with a target longer than the query: the reference's reverse pass reads
                                    past the query (structurerescorediagonal.cpp:96-99); forward fields are valid, revScore is not */
    FSGPU_DIAG_BAD_ID = 3
};
typedef struct {
    int32_t score;          /* forward run */
    int32_t startPos, endPos;   /* along the diagonal, like DistanceCalculator::LocalAlignment */
    int32_t revScore;       /* reversed-query run (module score = score - revScore) */
    int32_t diagonalLen;
    int32_t identicalAA;    /* equal amino acids inside [startPos, endPos] */
    int32_t status;         /* FSGPU_DIAG_* */
    int32_t reserved;
} fsgpu_diag_res;
int fsgpu_diag_rescore(fsgpu_ctx *ctx, const uint8_t *qAA, const uint8_t *q3Di, const uint64_t *qOffsets, const int32_t *qLengths,
                       int nq, const int16_t *mat3Di, const int16_t *matAA, const fsgpu_diag_pair *pairs, int64_t n, fsgpu_diag_res *out);

/* ---- start position + backtrace of accepted hits on the device (rounds 5-6) ------------------------------------------------
 * StructureSmithWaterman::alignStartPosBacktraceBlock (F/src/commons/StructureSmithWaterman.cpp:369-537) over the block-aligner crate's align_3di
 * (M/lib/block-aligner/src/scan_block.rs:120-630, 1302-1443, 1844-2007) for a batch of hits: the reversed prefixes query[0..qEnd], target[0..dbEnd] are
 * aligned from their ends with starting block sizes 32, 64, 128 until the SW score is reproduced.  tblAA / tbl3Di: the crate's AAMatrix of the two
 * substitution matrices ([27][32] int8, letter-indexed, as block_set_aamatrix fills them: host/block_aligner.cpp, block_aamatrix_scores); letterAA /
 * letter3Di [21]: residue code -> letter - 'A'.  cbAA / cbSS: the query's forward composition bias (int8 per residue, StructureSmithWaterman.cpp:1566-1640).
 * status 1: qStart / dbStart / identicalAA and btLen characters ('M', 'I', 'D', query start to end) at *btBase + btOff (valid until the next call on this
 * context); status 2: the aligner's score differs from the SW score -- the reference leaves such a hit without start position and backtrace
 * (structurealign.cpp:83); status 0: not computed here -- the alignment needs a block of more than 128 rows and the second pass (blocks of up to 512 rows;
 * the crate grows to 4096) did not run for it (it runs when at least 64 such hits per usable host core have come back from the first pass, or with
 * FSGPU_BT_PASS2=1) or could not finish it either: the caller runs its host path (fshost_block_backtrace) -- same answer either way.
 * Needs a database loaded WITH AA sequences. */
typedef struct { const uint8_t *qAA, *q3Di; const int8_t *cbAA, *cbSS; int32_t L; int32_t reserved; } fsgpu_bt_query;
typedef struct { uint32_t query, target; int32_t qEnd, dbEnd, score; } fsgpu_bt_task;
typedef struct { int32_t status, qStart, dbStart, identicalAA, btLen, blockSizes; uint64_t btOff; } fsgpu_bt_res;
int fsgpu_block_backtrace(fsgpu_ctx *ctx, const int8_t *tblAA, const int8_t *tbl3Di, const uint8_t *letterAA, const uint8_t *letter3Di,
                          const fsgpu_bt_query *queries, int nq, const fsgpu_bt_task *tasks, int nt, int gapOpen, int gapExtend,
                          fsgpu_bt_res *res, const char **btBase);
/* Workgroups of the block aligner per compute unit for the following fsgpu_block_backtrace calls of this context (0: the default, 4 -- every CU's LDS
 * and three waves per SIMD for the 10-20 ms of a call).  1 leaves two thirds of a CU's LDS and most issue slots to the kernels of other contexts: what a
 * caller that shares a batch between its host threads and the device asks for (fshost_search_align_batch with FSGPU_DEVICE_BACKTRACE=2). */
int fsgpu_block_backtrace_footprint(fsgpu_ctx *ctx, int workgroupsPerCU);
/* ---- start cell + banded trace-back of accepted hits of PROFILE queries ------------------------------------------------------------
 * StructureSmithWaterman::alignStartPosBacktrace<PROFILE> (F/src/commons/StructureSmithWaterman.cpp:540-739; banded_sw :1723-1957, computerBacktrace
 * :746-773) for a batch of hits, which structurealign takes instead of the block aligner when the query database holds profiles.  Per task: the
 * affine SW recurrence over the reversed profile prefix [0, qEnd] x the reversed target prefix [0, dbEnd] in int32, stopped at the first column whose
 * maximum reaches `score` (its smallest row: the start cell); then the banded pass over [qStart, qEnd] x [dbStart, dbEnd], band |dbLen - qLen| + 1
 * doubled until the best score reaches `score`, its trace-back from the end cell, and the identities against lettersAA.  pAA / p3Di: the FORWARD alignment
 * profiles [21 * L] (X row included), read in place by both passes; target letters come from the resident database.  Tasks and results are those of
 * fsgpu_block_backtrace; blockSizes carries the band width the banded pass ended with.
 * status 1: qStart / dbStart / identicalAA and btLen characters at *btBase + btOff (valid until the next call on this context);
 * status 2: the reverse pass did not reproduce `score` (the reference exits there): no start cell;
 * status 3: start cell set, no path: the trace-back met a cell outside the band or an impossible direction, or the whole rectangle does not reach `score`;
 * status 0: not computed here, the caller runs its host path -- the task does not fit the scratch budget at the band it needs (blockSizes: that band).
 * Scratch: one direction byte per band cell, qLen x min(2 band + 1, dbLen) per task (slices are sized for two doublings ahead where the budget has room;
 * a band that outgrows its slice re-runs in a later launch of the same call), plus 8 bytes per line cell for lines beyond 1024 cells.  The budget of one
 * launch is FSGPU_PBT_BYTES (read per call; default 268435456 = 256 MiB: a module batch of 64 queries x 50 hits of 300 x 300 cells at 4 x its
 * first band stays below it, and eight feeder contexts of a device together stay below 2 GiB); a call whose tasks exceed it runs in several launches.
 * Refused with nothing launched and res untouched, FSGPU_E_ARG: a query index, target id or end cell out of range, gapOpen <= gapExtend or
 * gapExtend < 1; FSGPU_E_NODB: no database, or one loaded without AA sequences; FSGPU_E_UNSUPPORTED: gapOpen >= 32768 (the limit of the SW entries whose
 * records the tasks come from; the kernels' "no value" of -2^29 and their gap-cost products are sized for it).  nt == 0 is FSGPU_OK. */
typedef struct { const int8_t *pAA, *p3Di; const uint8_t *lettersAA; int32_t L; int32_t reserved; } fsgpu_pbt_query;
int fsgpu_profile_backtrace(fsgpu_ctx *ctx, const fsgpu_pbt_query *queries, int nq, const fsgpu_bt_task *tasks, int nt,
                            int gapOpen, int gapExtend, fsgpu_bt_res *res, const char **btBase);
/* The last fsgpu_profile_backtrace call of the context: [0] kernel launches, [1..4] tasks that came back with status 0, 1, 2, 3, [5] device milliseconds of
 * the launches (events), [6] scratch bytes of its largest launch, [7] launches of the banded pass among [0]. */
void fsgpu_profile_backtrace_last(const fsgpu_ctx *ctx, double *out8);
/* Number of devices that hold at least one live context of this process (a module run with --gpus 8 : 8).  The host side divides the cores the process may
 * use by it when it decides who computes the backtraces (FSGPU_CORES_PER_GPU overrides the quotient: one rank of a multi-process job sets it to its share). */
int fsgpu_live_devices(void);

/* ---- LDDT of accepted hits: LDDTCalculator::initQuery + computeLDDTScore (F/src/commons/LDDT.{h,cpp}) for a batch of hits ----------------------------
 * Per aligned column ('M' of the backtrace, from (qStart, dbStart)) the reference's per-residue score reduce_score[column], bit for bit: the count of
 * preserved-distance quarters over all other aligned columns whose query distance is below 15 A, times 1 / (neighbours of the query residue among ALL
 * query residues); NaN (0 * inf) for a query residue without neighbours.  The ordered float sum of the non-NaN columns, scoreLength and the division
 * (LDDTScoreResult, LDDT.h:102-119) are the caller's: fshost_lddt_average.
 * ca of a query: x[L] y[L] z[L], what Coordinate16::read hands out (fshost_ca_decode).  tCoords: the same layout per target, task k's at tOff (floats) with
 * tLen residues; several tasks may share one.  bt: 'M' / 'I' / 'D' characters (anything else is skipped, as in the reference), task k's at btOff, btLen of them.
 * alignLength[k] receives the number of aligned columns, out[outOff .. outOff + alignLength[k]) the per-column values (outOff + alignLength <= outCap is checked).
 * Alignments of any length up to FSGPU_MAX_SEQ_LEN run on the device; there is no host path. */
typedef struct { const float *ca; int32_t L; int32_t reserved; } fsgpu_lddt_query;
typedef struct {
    uint32_t query;         /* index into queries */
    int32_t tLen;           /* residues of the target */
    uint64_t tOff;          /* float offset of its coordinates in tCoords */
    int32_t qStart, dbStart;
    uint64_t btOff;
    uint32_t btLen;
    uint32_t reserved;
    uint64_t outOff;        /* float offset of its per-column values in out */
} fsgpu_lddt_task;
int fsgpu_lddt_batch(fsgpu_ctx *ctx, const fsgpu_lddt_query *queries, int nq, const fsgpu_lddt_task *tasks, int nt, const float *tCoords, uint64_t tCoordsLen,
                     const char *bt, uint64_t btBytes, int32_t *alignLength, float *out, uint64_t outCap);

/* ---- TM-score of accepted hits: TMaligner::computeTMscore with computeExactScore == false (F/src/commons/TMaligner.cpp:50-104, F/lib/tmalign) ------------
 * Per task the device pairs the residues along the backtrace ('M' pairs, 'I' advances the query, every other character the target), runs the two
 * fragment searches of computeAppoximateTMscore (standard_TMscore's and detailed_search_standard's TMscore8_search_standard, simplify_step 40) and the
 * KabschFast over all pairs, and returns raw values: nPairs[k], scores[k] / scores[nt + k] = the float score_max of the two searches (-1 without pairs),
 * rmsd[k].  All of it bit for bit what the reference computes, except where the double-precision atan2 / cos / sin of the device library differ from
 * the host's in the last place AND the difference survives the cast to float.  The scalars that need pow() and the final scalings are the
 * host's, with the C library the reference uses: fshost_tm_params fills the five floats of a task from its normalisation length, fshost_tm_finish
 * turns the raw values into the TM-score.  fsgpu_tm_batch does not return the rotation and translation; fsgpu_tm_superpose_batch (below) does.
 * Queries, tCoords, bt and the task geometry as for fsgpu_lddt_batch.  Alignments of any length up to FSGPU_MAX_SEQ_LEN run on the device; there is no
 * host path. */
typedef struct {
    uint32_t query;         /* index into queries */
    int32_t tLen;           /* residues of the target */
    uint64_t tOff;          /* float offset of its coordinates in tCoords */
    int32_t qStart, dbStart;
    uint64_t btOff;
    uint32_t btLen;
    float scoreD8;          /* parameter_set4search: score_d8 */
    float d0Std;            /* standard_TMscore: its d0, which is also its local_d0_search */
    float d0;               /* parameter_set4search: d0 (= D0_MIN) */
    float d0Search;         /* parameter_set4search: d0_search */
    uint32_t reserved;
} fsgpu_tm_task;
int fsgpu_tm_batch(fsgpu_ctx *ctx, const fsgpu_lddt_query *queries, int nq, const fsgpu_tm_task *tasks, int nt, const float *tCoords, uint64_t tCoordsLen,
                   const char *bt, uint64_t btBytes, int32_t *nPairs, float *scores, float *rmsd);

/* ---- TM-score with its superposition, approximate or exact (TMaligner::computeTMscore, F/src/commons/TMaligner.cpp:50-212) ------------------------------
 * Same arguments and checks as fsgpu_tm_batch.  One record per task; t / u are the translation and rotation the reference's TMscoreResult carries
 * (x' = t + u x moves the TARGET's residues onto the query's), i.e. the superposition at the FIRST occurrence of the winning search's maximum in the
 * reference's serial order (fragment length, fragment start, refinement round), whichever workgroup found it.
 *   exact == 0  computeAppoximateTMscore: score[0] / score[1] = score_max of standard_TMscore's / detailed_search_standard's search, rms = the raw
 *               rmsd, all three bit for bit what fsgpu_tm_batch returns; fshost_tm_finish as before.  t / u: the second search's, or the first one's
 *               if the second never beat its initial -1, or the all-pairs KabschFast's if neither did.
 *   exact == 1  computeExactTMscore: TMscore8_search over all pairs with simplify_step 1 (every fragment start), n_it 10, score_fun8 dividing by
 *               Lnorm.  The task's four floats are fshost_tm_exact_params' in order: scoreD8, Lnorm IN THE d0Std FIELD (>= 0; 0 gives INF / NaN scores as
 *               the reference's), d0, d0Search (parameter_set4final).  score[0] = score_max (the TM-score is (double) score[0]), score[1] = -1,
 *               rms = the raw rms of the all-pairs KabschFast (fshost_tm_exact_finish: sqrt(rms / nPairs)).  t / u: the search's, else the all-pairs
 *               KabschFast's.  The search spans ceil(starts / 128) workgroups per task; their partials are reduced on the device: larger score, then
 *               smaller start ordinal, NaN never -- no atomics, nothing depends on the launch order.
 * A task without 'M' columns: scores -1, rms 0, source FSGPU_TM_SRC_NONE, t = 0, u = identity (nothing runs for it).
 * The double atan2 / cos / sin caveat of fsgpu_tm_batch applies to every field. */
#define FSGPU_TM_SRC_NONE 0      /* no pairs */
#define FSGPU_TM_SRC_KABSCH 1    /* KabschFast over all pairs */
#define FSGPU_TM_SRC_SEARCH1 2   /* standard_TMscore's search */
#define FSGPU_TM_SRC_SEARCH2 3   /* detailed_search_standard's search */
#define FSGPU_TM_SRC_EXACT 4     /* TMscore8_search of the exact mode */
typedef struct {
    int32_t nPairs;
    int32_t source;         /* FSGPU_TM_SRC_*: where t / u came from */
    float score[2];
    float rms;
    float t[3];
    float u[9];             /* u[3 * i + j] = u[i][j] */
} fsgpu_tm_result;
int fsgpu_tm_superpose_batch(fsgpu_ctx *ctx, const fsgpu_lddt_query *queries, int nq, const fsgpu_tm_task *tasks, int nt, const float *tCoords,
                             uint64_t tCoordsLen, const char *bt, uint64_t btBytes, int exact, fsgpu_tm_result *out);

/* ---- prefilter: k-mer matching with double-diagonal hits + ungapped diagonal scoring ------------------------- */
/* Index parameters == the subset of Prefiltering's members that shape IndexTable / SequenceLookup.  Sequence-
 * sequence searches with k = 6 only (what setupSplit picks below 3.35e9 residues, IndexTable.h:456-458). */
typedef struct {
    int32_t kmerSize;       /* 6 */
    int32_t spaced;         /* 1: pattern 1101010011 (M/src/commons/Sequence.h:25), 0: contiguous */
    int32_t kmerThr;        /* Prefiltering::getKmerThreshold (Prefiltering.cpp:1036-1096); 78 at -s 9.5 */
    int32_t maskLowerCase;  /* --mask-lower-case (Foldseek: 1) */
    int32_t maskNrepeats;   /* --mask-n-repeat   (Foldseek: 6); tantan masking (--mask 1) is not available */
} fsgpu_kmer_index_params;
/* Builds, in HBM and from the resident 3Di database (fsgpu_db_load / fsgpu_db_adopt_device), the masked sequence
 * lookup, the k-mer index (offset table over 20^6 k-mers + one (seqId, first position) entry per distinct k-mer of
 * every target, lists ordered by seqId) and the sorted 8000 x 8000 extended 3-mer matrix of kmerSubMat21x21
 * (the 8-bit "k-mer" matrix of the prefilter: SubstitutionMatrix(3di.out, 8.0, -0.2), int16 row-major 21x21).
 * Limits (FSGPU_E_UNSUPPORTED beyond them): k = 6; fewer than 2^32 residues in the database (the reference switches to k = 7 from 3.35e9 residues
 * on, IndexTable.h:456-458, before that limit is reached); at most 33.5 M targets (512 coarse bins of the hit-stream partition, each inside one block of
 * 65536 target ids; 16.4 M until round 5); no target of 32768 residues or more (so a position never needs a 16th bit: 15 at most in either entry form);
 * at least one residue in the database.  Index entries are 4 bytes (seqId << posBits | position) while the id
 * bits and the position bits of the database fit 32 together, 8 bytes otherwise. */
int fsgpu_kmer_index_build(fsgpu_ctx *ctx, const fsgpu_kmer_index_params *p, const int16_t *kmerSubMat21x21);
uint64_t fsgpu_kmer_index_entries(const fsgpu_ctx *ctx);
/* Bytes of one index entry of the resident index: 4 or 8 (see above; FSGPU_KMER_ENTRY64=1 at build time keeps the 8-byte form); 0 before an index is built. */
int fsgpu_kmer_index_entry_bytes(const fsgpu_ctx *ctx);
/* The parameters the resident index was built with (a clone answers with those of the index it shares).  FSGPU_E_NODB while the context has
 * no index, FSGPU_E_ARG for a null pointer; *out is written only on FSGPU_OK.  What prepares queries for fsgpu_kmer_search reads `spaced` here. */
int fsgpu_kmer_index_get_params(const fsgpu_ctx *ctx, fsgpu_kmer_index_params *out);
/* Inspection (tests): copy the offset table (64e6+1 uint32), the entries (seqId << 16 | position) and/or the masked
 * sequence lookup (padded DB layout) to host memory; any pointer may be NULL.  The table is kept in the DEVICE k-mer
 * order: index = first3mer * 8000 + last3mer (the reference numbers k-mers first3mer + 8000 * last3mer).  Row `row` of the extended 3-mer matrix. */
int fsgpu_kmer_index_copy(fsgpu_ctx *ctx, uint32_t *offsets, uint64_t *entries, uint8_t *masked);
int fsgpu_kmer_row_copy(fsgpu_ctx *ctx, int row, int16_t *score, uint16_t *index);

typedef struct {
    int32_t maxResListLen;      /* --max-seqs */
    int32_t minDiagScoreThr;    /* --min-ungapped-score, >= 0 (0: a query with fewer than maxResListLen scored targets also gets the score-0 elements the reference hands on) */
    int32_t bins;               /* BINSIZE of CacheFriendlyOperations; 0 = derive from l2CacheSize like initDiagonalMatcher */
    int32_t kmerScoreOnly;      /* 1 = --diag-score 0 (QueryMatcher with diagonalScoring == false, QueryMatcher.cpp:215-232): no ungapped diagonal scores,
                                 * the score of a target is its number of double-diagonal k-mer matches (findDuplicates with computeTotalScore,
                                 * CacheFriendlyOperations.cpp:217-241; capped at 255), the diagonal that of its first one; the first step of
                                 * easy-cluster's cascaded prefilter runs like this (-s 1 --diag-score 0 --min-ungapped-score 0) */
    int64_t maxDbMatches;       /* 0 = 2*max(1e6,N) (QueryMatcher.cpp:45) */
    int64_t foundDiagonalsSize; /* 0 = max(1e6,N)   (QueryMatcher.cpp:44) */
    uint64_t l2CacheSize;       /* Util::getL2CacheSize() of the host whose tie order is to be reproduced; 0 = this host */
} fsgpu_kmer_search_params;
/* One query: numeric codes seq[L]; kmerThr[i] for every k-mer start i in [0, L - patternSize] =
 * max(kmerThr - round(sum of the composition bias over the k-mer), 0) (QueryMatcher.cpp:262-270);
 * profile[L][21] = ungappedSubMat[q_i][a] + round(bias_i / 4) (UngappedAlignment::createProfile).
 * fshost_kmer_query_prepare fills both.  identity = target id that is the query itself, or -1. */
typedef struct {
    const uint8_t *seq;
    const int16_t *kmerThr;
    const int8_t *profile;
    int32_t L;
    int32_t reserved;
    int64_t identity;
} fsgpu_kmer_query;
/* == hit_t (QueryMatcher.h:31-48) with the target's DB index instead of its key */
typedef struct {
    uint32_t id;
    int32_t score;
    uint16_t diagonal;
    uint16_t pad;
} fsgpu_kmer_hit;
enum {
    FSGPU_KMER_OK = 0,
    FSGPU_KMER_UNSTABLE = 1,     /* >= foundDiagonalsSize/2 targets carried a diagonal: the reference orders equal scores with an
                                    unstable std::sort there (QueryMatcher.cpp:205-215); replayed with the same call on the same
                                    sequence, identical wherever both builds use libstdc++'s introsort (informational) */
    FSGPU_KMER_E_OUTPUT = -1,    /* the reference would have cut findDuplicates short (output array full): replayed in the diagonal-score mode since round 4,
                                    still a status with kmerScoreOnly (and beyond 256 MB of per-bin counters for the flagged queries of a batch) */
    FSGPU_KMER_E_CHUNKS = -2,    /* more than 255 databaseHits refills */
    FSGPU_KMER_E_REFILL_COUNTS = -3  /* no longer returned (kept for the ABI): kmerScoreOnly queries that refill databaseHits have the reference's merge of the
                                        per-refill counts (mergeScoreDuplicates, CacheFriendlyOperations.cpp:150-180) replayed on the device since round 4 */
};
/* Runs nq queries (batched on the device), writes per query q up to maxResListLen hits to out[q*maxResListLen ..],
 * their number to nout[q] and a FSGPU_KMER_* code to status[q]; hits are bit-identical to QueryMatcher::matchQuery
 * (order included) whenever status[q] == 0.  stats (may be NULL): per query kmersPerPos, dbMatches, overflowed, bins.
 * kmerThr[] of every query must be prepared with the pattern of the RESIDENT index (fsgpu_kmer_index_get_params: 10 residues with spaced = 1,
 * 6 with spaced = 0): the call reads max(0, L - patternSize + 1) thresholds per query and cannot tell an array prepared for the other pattern --
 * a shorter one is read past its end, a longer one gives thresholds summed over the wrong residues.  fshost_search_kmer_batch checks its `spaced`
 * argument against the index and refuses a mismatch. */
int fsgpu_kmer_search(fsgpu_ctx *ctx, const fsgpu_kmer_search_params *p, const fsgpu_kmer_query *queries, int nq,
                      fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats);

/* ---- profile queries in the k-mer prefilter (`prefilter <profileDB_ss> ...` with --prefilter-mode 0: every round of an iterative search after the
 * first).  One query: the query letters seq[L] (Sequence::numSequence of the 3Di profile; a window with a letter >= 20 at one of its six pattern
 * offsets is skipped, QueryMatcher.cpp:264), the RAW score bytes scores[L][20] of the entry (Sequence::mapProfile reads them as short without the
 * division by four; fshost_profile_decode_raw), the ungapped profile[L][21] = score / 4 with a zero X column (UngappedAlignment::createProfile,
 * profile branch: no bias correction), kmerThr (fshost_kmer_threshold_profile or --k-score's profile half; every position's threshold is
 * max(kmerThr, 0): a profile has no composition bias, QueryMatcher.cpp:109-117,271) and identity as in fsgpu_kmer_query.
 * The similar k-mers of a position are KmerGenerator::generateKmerList over the six rows of its window, each sorted by Util::rankedDescSort20 (the
 * call sorts them while it stages the batch): all 6-tuples of row ranks whose scores sum to >= the threshold, in lexicographic order of the ranks,
 * the first 8 388 607 of them (MAX_KMER_RESULT_SIZE - 1).  The reference computes its cutoffs in 16 bits; they wrap for a kmerThr above 31 999,
 * which this call does not reproduce: there it gives what the rule gives without the wrap (no k-mer, as for every kmerThr above 762). */
typedef struct {
    const uint8_t *seq;
    const int8_t *scores;
    const int8_t *profile;
    int32_t L;
    int32_t kmerThr;
    int64_t identity;
} fsgpu_kmer_profile_query;
/* fsgpu_kmer_search for profile queries: same parameters, outputs, status codes, statistics, batching and halving rule; everything behind the
 * similar-k-mer lists is the same code.  fsgpu_kmer_last_counts / _batch_hint / _last_segments / fsgpu_last_kernel_ms read it like a sequence call.
 * The resident index must have been built with kmerThr = 0 (Prefiltering.cpp:555-557: localKmerThr is 0 with a profile query, no target k-mer is
 * dropped for its self-score); any other index is refused with FSGPU_E_ARG before anything is staged. */
int fsgpu_kmer_search_profile(fsgpu_ctx *ctx, const fsgpu_kmer_search_params *p, const fsgpu_kmer_profile_query *queries, int nq,
                              fsgpu_kmer_hit *out, int32_t *nout, int32_t *status, double *stats);
/* Test / inspection: the similar k-mers of k-mer start `pos` of query `query` of the LAST DEVICE BATCH of this context, which must have been a profile
 * batch (a call of more queries than one batch takes leaves its last batch; a sequence call in between leaves none: FSGPU_E_ARG).  *count receives K_p
 * (capped); kmers[0 .. min(cap, K_p)) the k-mers in emission order, in the reference's numbering sum of letter_i * 20^i (i in pattern order).  The list
 * pass itself writes them, with the index probes switched off. */
int fsgpu_kmer_profile_list_copy(fsgpu_ctx *ctx, int query, int pos, uint32_t *kmers, uint32_t cap, uint32_t *count);
/* Host only: the rows of L positions as the device reads them, rows[i * 20 + rank] = score << 8 | letter, sorted by the comparator sequence of
 * Util::rankedDescSort20 (equal scores stay where that network leaves them: neither stable nor by letter, and visible in the results). */
int fsgpu_kmer_profile_sort_rows(const int8_t *scores, int L, uint16_t *rows);

/* Work counters of the last fsgpu_kmer_search batch: [0] similar k-mers probed in the index table, [1] index hits,
 * [2] double-diagonal candidates, [3] elements handed to the host tail. */
void fsgpu_kmer_last_counts(const fsgpu_ctx *ctx, uint64_t *out4);
/* Queries worth handing to the next fsgpu_kmer_search call of this context (a multiple of 32, 32..1024): as many as one device batch takes at
 * the index hits per query the previous call saw.  A low-sensitivity prefilter (clustering: ~10^4 hits per query) needs hundreds of queries
 * per batch to fill the device, the sensitive search default (~10^7 hits per query at 1M targets) fills it with 32. */
int fsgpu_kmer_batch_hint(const fsgpu_ctx *ctx);
/* Accounting of the last batch's hit-stream partition (round 6: one order-preserving scatter into (query, key) runs, a key = a run of blocks
 * of 1024 target ids): [1] = [4] (query, databaseHits chunk, key) runs walked by the duplicate stage, [3] tiles of the scatter, [5] coarse keys
 * of the level the batch used, [6] target ids of its widest key (one byte of LDS each in k_kmer_dup_stream); [0] = [2] = 0. */
void fsgpu_kmer_last_segments(const fsgpu_ctx *ctx, uint32_t *out7);
/* The coarse keys of that partition (host-only planning, also used by the index build): consecutive blocks of 1024 target ids joined into keys.
 * blocksPerKey = 1..64: that many blocks per key; 0: about 128 keys of equal residue count, none longer than twice the average number of blocks
 * nor than 64.  key(t) = blkKey[t >> 10]; keyFirst[key] .. keyFirst[key + 1] are its target ids (at most 65536: the low 16 bits of an id are unique
 * inside a key).  Fills blkKey[max(1, ceil(n / 1024))] / keyFirst[keys + 1] (either may be NULL) and returns the number of keys (<= 512 up to
 * 33.5 M targets), or FSGPU_E_ARG when cap is too small. */
int fsgpu_kmer_plan_coarse(const int32_t *lengths, uint64_t n, uint32_t blocksPerKey, uint16_t *blkKey, uint32_t *keyFirst, uint32_t cap);

/* ---- instrumentation -------------------------------------------------------------------------------------- */
/* Device time (ms, HIP events on the context stream) of the dominant kernel of the last _finish()ed call:
 * which = 0 gapless scan kernel, 1 SW kernel, 2 whole device part of the last fsgpu_kmer_search batch,
 * 3..10 its stages (similar-k-mer count, index probes, hit gather, partition into (query, bin) segments, double-diagonal
 * detection per segment, scoring, replay, selection), 11 host tail, 12 the index-probe kernel (k_kmer_lists) alone,
 * 14 / 15 the two kernels of the last fsgpu_lddt_batch (k_lddt_norm, k_lddt_pairs),
 * 16 / 17 the two kernels of the last fsgpu_tm_batch (k_tm_pairs, k_tm_search),
 * 18 / 19 / 20 the three kernels of the last fsgpu_tm_superpose_batch (k_tm_pairs, k_tm_sp_search, k_tm_sp_finish),
 * 21 / 22 / 23 of the last fsgpu_sw_scan_c, summed over its sub-batches: the Smith-Waterman launches, k_sw_scan_count + k_sw_scan_offsets, k_sw_scan_emit.
 * Returns < 0 if nothing was recorded. */
double fsgpu_last_kernel_ms(const fsgpu_ctx *ctx, int which);
/* Read-only record of the choices a context makes from what it ran before (for tests; nothing reads it back): out8[0] / [1] the form the count pass
 * / the list pass of the last k-mer device batch ran in (0 not run, 1 one workgroup per query position, 2 one wave per position); [2] device batches
 * of the last fsgpu_kmer_search call, [3] queries of its last batch; [4] / [5] pairs of row-tiled queries (> 1024 residues) the last
 * fsgpu_sw_multi_dir call ran on the device / answered from the records its forward call had kept; [6] k_lddt_norm launches of this context since
 * it was created; [7] queries of the FIRST device batch of the last fsgpu_kmer_search call. */
void fsgpu_history_counters(const fsgpu_ctx *ctx, uint64_t *out8);
/* out[2][4], per direction (0 forward, 1 reversed query) of the last fsgpu_sw_multi_dir calls of this context: device ms of that pass's
 * k_sw2 launches (HIP events on the context stream; -1 when the pass did not run), DP cells (query rows x target columns over the
 * single-tile pairs), pairs, and the VALU wave-instructions its waves issue (DP rows + per-step overhead; the issue-rate roofline's unit). */
void fsgpu_sw_last_passes(const fsgpu_ctx *ctx, double *out);
/* out[12]: what the last fsgpu_sw_multi_dir_c / fsgpu_sw_multi_c (or _dir_p / _p) call of this context planned and ran (counters kept on the host; a call that
 * fails its argument checks leaves them as they were; one that fails later, out of memory for instance, leaves them zeroed or partly filled).  A pair counts once, also when fsgpu_sw_multi_c runs it in both directions.
 * [0] [1] [2] pairs run by k_sw3 with 16 / 32 / 64 lanes per target pair; [3] [4] [5] for the same three shapes the rows-per-lane classes that
 * were launched, bit R set for R rows per lane (R = 1..24 with 16 lanes, 1..16 with 32 and 64); [6] pairs of the queries of more than 1024 rows,
 * which took the profile path; [7] pairs handed to the int32 re-run because a direction of theirs returned 32767; [8] LDS images built in this call
 * (0: those of an earlier call over the same queries were reused, or no pair ran through k_sw3); [9] launch groups per direction; [10] workgroups per direction;
 * [11] 0. */
void fsgpu_sw3_last_plan(const fsgpu_ctx *ctx, uint32_t *out);
/* out[36]: launches of every instantiation of the profile path's kernels by this context since it was created (a clone starts at zero; counters
 * only, nothing reads them for a launch).  Index (kind * 2 + hasAA) * 6 + c: kind 0 k_sw with the two int16 halves, 1 k_sw in int32 (the re-run of
 * saturated pairs), 2 k_sw2; hasAA 1 with an AA table; c the index of R in {1, 2, 3, 4, 6, 8}. */
void fsgpu_sw_kernel_counts(const fsgpu_ctx *ctx, uint64_t out[36]);

#ifdef __cplusplus
}
#endif
#endif /* FSGPU_H */

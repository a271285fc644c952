/*
 * kbest_c.h -- C ABI of the MI355X-native k-best assignment engine.
 *
 * This is the drop-in boundary for the reference's k-best / association-weight
 * hot path.  Every entry point names the reference interface it replaces
 * (paths relative to the reference repository root):
 *
 *   kbest_batch_f64 / kbest_batch_f64_dev
 *        batched form of  kBest2D        (shortestPathCPP.hpp:204-212, cpp:571-644)
 *        and of           kBest2DCutoff  (shortestPathCPP.hpp:256-265, cpp:646-733)
 *        (opts.use_cutoff selects which); with k == 1 it is also the batched
 *        form of          assign2D       (shortestPathCPP.hpp:144-149) as used by
 *        asgnBB (assignment.cpp:750, k=1, maximize).
 *   kbest_weights_batch_f64
 *        batched form of  assignmentProb (assignment.h:11, assignment.cpp:547-683)
 *   kbest_condition_costs_f64
 *        batched form of  conditionCosts (assignment.h:26, assignment.cpp:439-525)
 *   kbest_assoc_probs_batch_f64
 *        batched form of  getAssignmentProbs from the cost matrix on (assignment.cpp:57-74)
 *   kbest_quadric_costs_f64 / kbest_quadric_assoc_probs_batch_f64
 *        batched form of  computeQuadricCostMatrix (assignment.cpp:705-722) and of the whole
 *        getAssignmentProbs chain behind it
 *   kbest_bb_costs_f64 / kbest_bb_match_batch_f64
 *        batched form of  asgnBB (assignment.cpp:724-797; k = 1, maximize)
 *   kbest_permanent_probs_batch_f64 / kbest_permanent_probs_batch_f64_dev
 *        batched form of  permanentProb (assignment.h:13, assignment.cpp:145-290), exact for every permOpt
 *   kbest_sample_assoc_batch_f64 / kbest_sample_assoc_batch_f64_dev
 *        joint associations drawn from the exact posterior those probabilities are the marginals of (not in the reference)
 *   kbest_belief_probs_batch_f64 / kbest_belief_probs_batch_f64_dev
 *        the association probabilities by loopy belief propagation, for frames of any size (not in the reference)
 *   kbest_clustered_probs_batch_f64 / kbest_clustered_probs_batch_f64_dev
 *   kbest_hybrid_probs_batch_f64 / kbest_clustered_partial_batch_f64_dev
 *   kbest_hybrid_exact_probs_batch_f64 / kbest_bigcluster_probs_f64_dev
 *   kbest_hybrid_frontier_probs_batch_f64 / kbest_frontier_probs_f64_dev
 *   kbest_hybrid_frontier_probs_batch_f64_dev / kbest_reserve_hybrid_dev
 *        the exact association probabilities by gated clusters, for frames of up to 128 measurements (not in the reference)
 *   kbest_quadric_map_probs_batch_f64 / kbest_quadric_map_probs_batch_f64_dev / kbest_reserve_quadric_map_dev
 *        getAssignmentProbs (assignment.cpp:38-74, usePerm) from quadrics against a map of any size: the exact probabilities
 *   kbest_clustered_sample_assoc_batch_f64 / kbest_clustered_sample_assoc_batch_f64_dev
 *   kbest_hybrid_frontier_sample_assoc_batch_f64 / kbest_hybrid_frontier_sample_assoc_batch_f64_dev
 *        joint associations drawn from the exact posterior of such frames, one walk per cluster (not in the reference)
 *   kbest_quadric_map_sample_assoc_batch_f64 / kbest_quadric_map_sample_assoc_batch_f64_dev / kbest_reserve_quadric_map_sample_dev
 *        the same draws from quadrics against a map of any size, in the rows of the raw block (not in the reference)
 *   kbest_assoc_factors_f64_dev / kbest_quadric_map_factors_batch_f64_dev / kbest_assoc_factors_batch_f64
 *        the consumer loop (system.cpp:279-346): thresholded, ordered factor and new-landmark lists from the probabilities
 *
 * Conventions kept from the reference: cost matrices are column-major
 * C[row + col*numRow] with numRow >= numCol (shortestPathCPP.hpp:185-190);
 * row4col is indexed by column, col4row by row; col4row values >= numCol mean
 * "row sits on a zero-padded column" (SURVEY 8(a) quirk 6); the number of
 * solutions found is returned per problem, 0 = infeasible (cpp:588-593).
 * The solver never throws; negative return values are engine errors.
 *
 * Order of exact ties.  Hypotheses with EXACTLY equal gain have no defined relative order in the reference (it is an
 * artefact of std::priority_queue's binary heap, shortestPathCPP.cpp:30-42, 574; which of them fill the last slots of a
 * call is an artefact too).  For continuous costs ties have probability zero and every output is the reference's, bit for bit.
 * For integer-like costs (conditionCosts produces exact zeros) there are two answers to choose from:
 *   (1) THE REFERENCE'S OWN -- what its heap pops, slot for slot.  The SYNCHRONOUS k-best entries (kbest_batch_f64,
 *       kbest_resolve_ties_dev behind the asynchronous entry, kbest_batch_f64_multi in batch mode) give it BY DEFAULT: the batch runs
 *       on the fast kernels, every enumeration launch enumerates ONE solution more than asked for (its gain only; measured free) and
 *       is followed by a small launch that reports, per problem, KBEST_TIE_* flags (kbest_opts.tie_flags): every problem with two
 *       exactly equal gains among its k + 1 best -- inside the table or across slot k -- is then enumerated AGAIN by the
 *       reference-order kernel (kbest_exact.hip: the reference's algorithm as it stands) and its tables are replaced
 *       (KBEST_TIE_REFERENCE).  A tie-free problem has ONE sequence of k best, which the fast kernels return bit for bit, so the call
 *       as a whole answers as the reference does, at the fast kernels' speed wherever nothing ties.  KBEST_FLAG_REFERENCE_ORDER runs
 *       EVERY problem on that kernel (slow, exact; also names col4row's padded columns as the reference does on every problem).
 *   (2) THE ENGINE'S RULE, the same in every kernel and for every batch a problem may travel in: solutions ordered by
 *       (gain, row4col), row4col compared lexicographically in the reference's column order; when the k-th and the (k+1)-th best
 *       gains are equal -- the k best are then not a unique set -- the lexicographically first assignments of that gain level are
 *       kept.  The multiset of gains and the validity of every assignment are the reference's; the order inside a run of equal gains
 *       and the members of a level that straddles slot k are the rule's.  This is what the finishing launch leaves in the tables, so
 *       what the ASYNCHRONOUS entries return (with the flags), what the association entries weigh by default (the exhaustive kernel
 *       and the bounded walk see a whole gain level and keep its lexicographically first members themselves, whatever its size), and
 *       what the synchronous entries return with KBEST_FLAG_CANONICAL_TIES: a tie at slot k (KBEST_TIE_BOUNDARY) is then completed by
 *       enumerating the problem again with k + 64, then k + 256, k + 1 024, k + KBEST_TIE_CAP solutions until the level ends inside
 *       the table (KBEST_TIE_RESOLVED; a level with more than KBEST_TIE_CAP members beyond k -- on the association entries, whose
 *       weights are summed on the device: of more than 4 096 members in all -- stays KBEST_TIE_UNRESOLVED: the emitted set is then one
 *       of several equally good ones and may depend on the kernel; a re-run that fails leaves the first pass' tables and that flag).
 *       On tie-heavy batches (1) is also the cheaper one: one more run of k solutions instead of thousands of members of a level.
 * KBEST_FLAG_NO_TIE_RESOLVE: the synchronous entries only report the flags; KBEST_FLAG_NO_TIE_CHECK switches all of it off (the
 * kernels' own orders, round 4).  Association entries: kbest_set_reference_order(ctx, 2) weighs the reference's own k best on frames
 * with a tie at slot k (1: on every frame).
 * Index outputs are int32 (the reference ABI uses ptrdiff_t; the C++ shims in
 * include/kbest_shims.hpp widen on the host).
 *
 * All compute runs in hand-written HIP kernels for gfx950
 * (probabilisticsemslam_amd/csrc/kbest_engine.hip).  There is no CPU fallback:
 * without a GPU every compute entry point returns KBEST_ERR_NO_DEVICE.
 */
#ifndef KBEST_C_H
#define KBEST_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kbest_ctx kbest_ctx; /* opaque: device, stream, workspace pools */

enum {
    KBEST_OK = 0,
    KBEST_ERR_NO_DEVICE = -1,   /* no HIP device / HIP runtime error at create    */
    KBEST_ERR_BAD_ARG = -2,     /* null pointer, k < 1, numRow < numCol, ...      */
    KBEST_ERR_UNSUPPORTED = -3, /* numRow > KBEST_MAX_DIM_EXACT                                                     */
    KBEST_ERR_HIP = -4,         /* a HIP call failed; see kbest_last_error()      */
    KBEST_ERR_NOMEM = -5,
    KBEST_ERR_NOT_RESERVED = -6, /* kbest_batch_f64_dev: workspace too small, call kbest_reserve first   */
    KBEST_ERR_INTERNAL = -7     /* a problem came back with nf < 0 although its shape was accepted       */
};

#define KBEST_MAX_DIM 64       /* rows per problem handled by the LDS-resident kernel (the fast path)      */
#define KBEST_MAX_DIM_WIDE 1024 /* rows per problem of the general-size kernel (beyond KBEST_MAX_DIM, or a k beyond the LDS    */
                               /* candidate pool: HBM work space)                                                         */
#define KBEST_MAX_DIM_EXACT 16384 /* rows per problem handled at all: beyond KBEST_MAX_DIM_WIDE the reference-order kernel runs */
                               /* (kbest_exact.hip: the reference's algorithm as it stands, one wave per problem -- slow, total; */
                               /* its work space holds one record of 25 numRow bytes per pushed hypothesis: KBEST_ERR_NOMEM    */
                               /* where 1 + (k - 1) numCol of them do not fit 16 GiB)                                         */

/* flags */
#define KBEST_FLAG_NO_PRUNE 1u     /* disable early termination (for counting P)   */
#define KBEST_FLAG_COUNT_PUSHED 2u /* fill `pushed` with the reference's push count */
#define KBEST_FLAG_RECT_ROOT 4u    /* internal (kbest_assign_batch_f64): numCol augmentations on the rectangular problem */
#define KBEST_FLAG_NO_SHIFT 8u     /* internal (kbest_assign_batch_f64): the cost matrix is already non-negative         */
#define KBEST_FLAG_NO_T0 32u       /* do not use the a-priori threshold from combinations of the root's children (A/B tests) */
#define KBEST_FLAG_EXACT_ROOT 16u  /* root LAP by the reference's own sequence of augmentations (no column reduction first)  */
#define KBEST_FLAG_NO_REORDER 128u /* 64-row kernel: enumerate in the reference's column order (A/B tests; same results)          */
#define KBEST_FLAG_NO_OPT 256u     /* 64-row kernel: no optimistic bounds / re-split tickets (A/B tests; same results)           */
#define KBEST_FLAG_NO_TIE_CHECK 512u /* do not enumerate the (k+1)-th solution / order exact ties canonically (see "Order of exact ties") */
#define KBEST_FLAG_REFERENCE_ORDER 2048u /* kbest_batch_f64[_dev]: the REFERENCE's own order of operations (kbest_exact.hip) -- the   */
                                        /* zero-padded N x N formulation, one priority queue of fully solved hypotheses with libstdc++'s */
                                        /* sift rules: hypotheses with exactly equal gains come out in the order the reference's heap  */
                                        /* pops them (shortestPathCPP.cpp:30-42, 574) and col4row names the padded column of every      */
                                        /* left-over row as the reference does.  Slow (up to 8 waves per problem, nothing pruned): for */
                                        /* callers with integer-like costs who need the reference's answer slot for slot.  No tie flags. */
#define KBEST_FLAG_REFERENCE_TIES 4096u /* (accepted; the DEFAULT of the synchronous k-best entries since round 6: every problem whose    */
                                       /* k + 1 best gains hold an exact tie is enumerated again by the reference-order kernel and its  */
                                       /* tables replaced, KBEST_TIE_REFERENCE: "Order of exact ties" (1))                              */
#define KBEST_FLAG_CANONICAL_TIES 8192u /* synchronous k-best entries, kbest_resolve_ties_dev, the multi-device batch entry: the        */
                                       /* engine's own rule on exact ties instead of the reference's answer: "Order of exact ties" (2)  */
#define KBEST_FLAG_NO_TIE_RESOLVE 1024u /* synchronous entries: report a tie at slot k (KBEST_TIE_BOUNDARY), do not complete its gain level */
#define KBEST_FLAG_TABLES_I8 64u   /* kbest_batch_f64 / kbest_batch_f64_dev: row4col / col4row are tables of int8_t (same shapes, */
                                   /* same values, -1 = unassigned / unused) instead of int32_t: every index of a problem of up   */
                                   /* to 127 rows fits a byte, and a quarter of the bytes cross PCIe.  numRow > 127:              */
                                   /* KBEST_ERR_UNSUPPORTED.  Not with the multi-GPU entries: the caller's tables are int32 there  */
                                   /* (what travels BETWEEN the devices is in bytes by itself wherever the indices fit them).      */

/* per-problem tie flags (kbest_opts.tie_flags, kbest_set_assoc_tie_flags_dev, kbest_last_tie_flags; see "Order of exact ties" above) */
#define KBEST_TIE_INSIDE 1            /* some of the emitted gains are exactly equal (they are in the canonical order)        */
#define KBEST_TIE_BOUNDARY 2          /* the k-th and the (k+1)-th best gains are exactly equal: the k best are not unique    */
#define KBEST_TIE_RESOLVED 4          /* ... and the entry completed that gain level: the lexicographically first were kept   */
#define KBEST_TIE_REFERENCE 8         /* KBEST_FLAG_REFERENCE_TIES: the problem was enumerated again by the reference-order kernel: its tables are the reference's own */
#define KBEST_TIE_UNCHECKED (1 << 28) /* ASYNCHRONOUS entries only: k sits at the limit of the kernel the problem ran on (e.g.     */
                                      /* k = 1 024 on the fused association kernel): the (k+1)-th solution was not enumerated, so */
                                      /* a tie at slot k would not have been seen (runs of equal gains INSIDE the tables are       */
                                      /* ordered as ever).  The synchronous entries take a kernel that fits k + 1 instead.         */
#define KBEST_TIE_UNORDERED (1 << 29) /* a run of more than 4 096 equal gains was left in the kernel's own order (asynchronous   */
                                      /* and association entries; kbest_batch_f64 orders such a run on the host)                */
#define KBEST_TIE_UNRESOLVED (1 << 30) /* BOUNDARY without RESOLVED: the emitted set is one of several equally good ones       */
#define KBEST_TIE_CAP 4096            /* members of the gain level at slot k beyond k that a synchronous entry enumerates at     */
                                      /* most (it tries 64, 256, 1 024, 4 096)                                                  */

/* ALWAYS initialise a kbest_opts with kbest_default_opts() and then set what you need: the struct has grown at its end
 * (tie_flags, round 5) and may grow again; a struct filled member by member by code compiled against an older header -- or one
 * that was never initialised -- hands the engine an indeterminate tie_flags pointer, which the finishing launch WRITES through. */
typedef struct kbest_opts {
    int32_t  maximize;     /* reference `maximize` argument                       */
    int32_t  use_cutoff;   /* 0: kBest2D semantics; 1: kBest2DCutoff semantics    */
    double   cutoff;       /* reference `cutoff` argument (assignment.cpp:9: 42)  */
    uint32_t flags;        /* KBEST_FLAG_*                                        */
    int32_t  root_col_offset; /* subtree sharding (multi-GPU latency mode):       */
    int32_t  root_col_stride; /* only root children on columns c with             */
                              /* c % stride == offset are expanded; 0/1 = all.    */
                              /* c is the REFERENCE's column and the partition is the reference's (split, cpp:455-532: the    */
                              /* child on column c keeps the root's rows on columns 0 .. c-1): a sharded run enumerates in    */
                              /* the reference's column order whatever kernel or launch shape runs it, so shards computed by  */
                              /* differently configured ranks still partition the problem.                                     */
    int32_t *tie_flags;       /* [B] KBEST_TIE_* per problem, or NULL: a host pointer for the host-buffer entries, a device     */
                              /* pointer for the _dev entries                                                                  */
} kbest_opts;

void kbest_default_opts(kbest_opts *o);

int kbest_create(kbest_ctx **ctx, int device);
int kbest_destroy(kbest_ctx *ctx);
const char *kbest_strerror(int code);
const char *kbest_last_error(const kbest_ctx *ctx);
int kbest_device_count(void);

/*
 * Batched k-best, buffers already resident in device memory (HBM).
 *   B         number of problems
 *   maxRow/maxCol  upper bounds of the shapes in the batch; also the leading
 *             dimensions of the outputs
 *   d_nRow/d_nCol  per-problem shapes, or NULL for uniform maxRow x maxCol
 *   d_cost    packed column-major cost blocks; problem b starts at
 *             d_costOff[b] doubles (or b*maxRow*maxCol when d_costOff is NULL)
 *   d_row4col [B][k][maxCol] int32   col -> row   (row4colBest, hpp:228-229)
 *   d_col4row [B][k][maxRow] int32   row -> col   (col4rowBest, hpp:226-227); NULL = not wanted
 *   d_gain    [B][k] double                       (gainBest,    hpp:230-231)
 *   d_nf      [B] int32   number found, 0 = infeasible (return value of kBest2D)
 *   d_pushed  [B] int64 or NULL; with KBEST_FLAG_COUNT_PUSHED the number of
 *             feasible children the reference would push (SURVEY 8(d) "P")
 *   opts->tie_flags  [B] int32 in device memory or NULL: KBEST_TIE_* per problem (this entry reports a tie at slot k,
 *             it cannot complete it: no synchronisation inside)
 *   stream    hipStream_t (NULL = the context's own stream).  Asynchronous:
 *             returns after enqueueing; no host synchronisation and no allocation
 *             inside -- the workspace must have been sized by kbest_reserve(B, maxRow, k)
 *             beforehand (else KBEST_ERR_NOT_RESERVED), which keeps the entry legal
 *             inside a graph capture.
 * ONE hypothesis workspace per context: launches of one context execute one after the
 * other.  A launch on a different stream than the previous one is ordered behind it
 * with an event (so results stay correct), but there is no overlap to be had -- use one
 * context per stream (or per host thread) for concurrent launches.
 */
int kbest_batch_f64_dev(kbest_ctx *ctx, const kbest_opts *opts, int B, int maxRow, int maxCol,
                        const int32_t *d_nRow, const int32_t *d_nCol, const double *d_cost,
                        const int64_t *d_costOff, int k, int32_t *d_row4col, int32_t *d_col4row,
                        double *d_gain, int32_t *d_nf, int64_t *d_pushed, void *stream);
/*
 * The second call for callers of kbest_batch_f64_dev whose costs can tie exactly (integer-like costs): SYNCHRONOUS.  Same
 * arguments as the launch it follows (same opts, shapes, cost blocks, tables -- all still on the device), d_tie_flags = the
 * opts->tie_flags the launch wrote.  Waits for `stream` and does what the synchronous entries do with flagged problems ("Order of exact
 * ties"): by default every problem flagged with a tie (inside its table, across slot k, or unchecked) is enumerated again by the
 * reference-order kernel and its slots of d_row4col / d_col4row / d_gain are replaced (KBEST_TIE_REFERENCE: the reference's own answer);
 * with KBEST_FLAG_CANONICAL_TIES every problem flagged KBEST_TIE_BOUNDARY has its gain level at slot k completed under the engine's rule
 * (the problem again with k + 64 / 256 / 1 024 / KBEST_TIE_CAP solutions; the first k of the canonically ordered table written over the
 * problem's slots; KBEST_TIE_RESOLVED, or KBEST_TIE_UNRESOLVED where the level is larger than the cap).  d_nf: the launch's nf
 * (may be NULL); a re-run problem's entry takes the re-run's count -- with a cutoff, gains that are equal in exact arithmetic but
 * round apart can make the reference keep another number of solutions than the first pass.  A batch without flagged problems costs
 * one small copy.
 */
int kbest_resolve_ties_dev(kbest_ctx *ctx, const kbest_opts *opts, int B, int maxRow, int maxCol, const int32_t *d_nRow,
                           const int32_t *d_nCol, const double *d_cost, const int64_t *d_costOff, int k, int32_t *d_row4col,
                           int32_t *d_col4row, double *d_gain, int32_t *d_tie_flags, int32_t *d_nf, void *stream);

/*
 * Same with host buffers (copies in, runs, copies out, synchronises; col4row may be NULL = not wanted).  Uniform square batches
 * of up to KBEST_MAX_DIM rows go through narrow staging: the kernels write row4col as bytes into pinned memory of the context, in
 * pieces, and host threads of the context widen a piece into the caller's int32 row4col and its inverse col4row while the GPU
 * works on the next one (the same tables bit for bit; 1 024 x 64x64, k = 200, 107 MB of int32 tables: 2.5 - 2.8 ms per call, the
 * kernel alone 1.8; round 3's paths -- copying 4.3, kernels writing the int32 tables into registered memory 3.1 -- remain for
 * everything else and behind KBEST_NO_NARROW).  A caller that runs batch after batch with the same buffers can register them
 * once (kbest_register_host_buffer): result tables that lie in registered memory are written there by the kernels themselves,
 * spread over the whole run; cost blocks in registered memory are read in place (each block once, into its LDS tile).  With
 * KBEST_FLAG_TABLES_I8 the caller takes the byte tables as they are (2.2 ms).
 */
int kbest_batch_f64(kbest_ctx *ctx, const kbest_opts *opts, int B, int maxRow, int maxCol,
                    const int32_t *nRow, const int32_t *nCol, const double *cost,
                    const int64_t *costOff, int k, int32_t *row4col, int32_t *col4row, double *gain,
                    int32_t *nf, int64_t *pushed);

/*
 * Batched assign2D (shortestPathCPP.hpp:144-149, cpp:735-762) and shortestPathCPP (hpp:178-182, cpp:119-238): the
 * single best assignment of each numRow x numCol problem by numCol shortest-augmenting-path steps on the
 * RECTANGULAR matrix (no zero-padded columns), with the dual variables.
 *   shift      1: assign2D -- the matrix is made non-negative first (makeCostMatrixSafe) and the gain is un-shifted;
 *              0: shortestPathCPP -- the matrix is used as it is (it must be non-negative; maximize must be 0)
 *   gainCols   numCol4Gain of shortestPathCPP (the gain sums the first gainCols columns, cpp:232); 0 = numCol
 *   row4col    [B][maxCol]  col -> row          col4row [B][maxRow]  row -> col, -1 = unassigned (cpp:134)
 *   u          [B][maxCol] MurtyHyp::u (per column), v [B][maxRow] MurtyHyp::v (per row); either may be NULL
 *   feasible   [B] 1, or 0 = infeasible (then gain = -1, cpp:197-203, and the index outputs are -1)
 * numRow <= KBEST_MAX_DIM.  Host buffers.
 */
int kbest_assign_batch_f64(kbest_ctx *ctx, int B, int maxRow, int maxCol, const int32_t *nRow, const int32_t *nCol,
                           const double *cost, const int64_t *costOff, int maximize, int shift, int gainCols,
                           int32_t *row4col, int32_t *col4row, double *gain, double *u, double *v,
                           int32_t *feasible);

/* toProbs (assignment.h:19, assignment.cpp:527-542): x[i] <- exp(min(x) - x[i]) where min(x) + 42 > x[i], else 0;
 * in place on a host buffer of n doubles. */
int kbest_to_probs_f64(kbest_ctx *ctx, double *x, int64_t n);

/* Size the context's workspace for launches of up to B problems of up to maxRow rows and k solutions.
 * Required before kbest_batch_f64_dev; the host-pointer entries call it implicitly.  When it has to
 * grow the workspace it waits for the device to go idle (hipDeviceSynchronize) and reallocates.
 * The workspace is: the hypothesis states ([B][k + 64 + up to 1 024] records of 18 maxRow + 24 bytes), the slot tables, the
 * gains behind the tables (exact ties) and -- for batches of more than one generation of resident workgroups, which the 64-row
 * kernel enumerates as a relay of several workgroups per matrix -- one LDS image per matrix (25 KB at 32 rows, 70 KB at 64;
 * at most ~400 MB: larger batches are not relayed).  A kbest_batch_f64_dev call whose batch was not reserved for fails with
 * KBEST_ERR_NOT_RESERVED; one whose relay images alone are missing (reserved with a smaller B) runs as a plain launch.
 * A graph that captured a relay launch holds the addresses of the relay work space: reserve for the largest batch BEFORE
 * capturing -- a later kbest_reserve that would have to grow that work space returns KBEST_ERR_BAD_ARG.
 * WORK SPACES UNDER A CAPTURED LAUNCH -- the same rule for every work space of the context and every asynchronous (_dev) entry:
 * a launch recorded by a stream capture bakes the addresses of the context's work spaces it uses into the graph, so the context
 * marks each of them as held, until kbest_destroy.  Reserve (kbest_reserve*, with the bounds of the LARGEST call) before capturing.
 * Afterwards any reservation, and any host-buffer entry (which stages, reserves and runs the _dev entry), of that context that
 * would have to grow -- that is, free and reallocate -- a held work space returns KBEST_ERR_BAD_ARG and kbest_last_error says
 * which work space a captured launch holds; nothing is freed, the graph stays valid.  Calls that fit what is reserved, and work
 * spaces no captured launch has used, are not affected.  Use another context for larger calls.  A piece of a relay
 * waits for its predecessor at most a few seconds (a healthy launch never gets there); a matrix whose hand-over did not come is
 * reported with nf = -3 (KBEST_ERR_INTERNAL from the host entries), and the context re-zeroes its progress words before the
 * next relay launch after any failed entry. */
int kbest_reserve(kbest_ctx *ctx, int B, int maxRow, int k);
/* The same for launches that run on the reference-order kernel (KBEST_FLAG_REFERENCE_ORDER, or maxRow > KBEST_MAX_DIM_WIDE): its work
 * space -- per resident problem a padded cost copy (8 maxRow^2 bytes) and a pool of 2 + (k - 1) maxCol hypotheses of 25 maxRow bytes.
 * kbest_batch_f64_dev needs it up front for such launches; the host entries grow it on demand. */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_exact(kbest_ctx *ctx, int B, int maxRow, int maxCol, int k);

/* Diagnostic builds only (make -C probabilisticsemslam_amd/csrc PROFILE=1): device buffer of B*16 uint64
 * that receives per-matrix cycle stamps of the kernel phases.  The regular build never touches it. */
int kbest_set_profile_buffer(kbest_ctx *ctx, void *d_buf);

/*
 * Batched assignmentProb (assignment.cpp:547-683): k-best with cutoff 42, then
 * sum of exp(best - cost) over the solutions scattered into probs.
 *   nL[b], nM[b]   landmarks / measurements of problem b; its cost block is
 *                  (nL+nM) x nM column-major
 *   probs          packed, problem b at probOff[b] doubles: [nM][nL+1] row-major
 *                  (the reference's vector<vector<double>>)
 *   nf[b]          the solutions the k-best found (at most k); nM == 1, where the reference
 *                  enumerates nothing (:554-570): the entries it weighs, x < 42
 * Host buffers.
 */
int kbest_weights_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM,
                            const double *cost, const int64_t *costOff, int k, double *probs,
                            const int64_t *probOff, int32_t *nf);

/*
 * The accumulation of bruteForceProb (assignment.h:43, assignment.cpp:880-945): plain kBest2D with the caller's k
 * (the reference derives it from a Minc-type bound, :858-868 -- the shim in kbest_shims.hpp does the same) and the
 * weights summed WITHOUT the best+42 mask.  Same layout as kbest_weights_batch_f64.
 */
int kbest_bruteforce_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM,
                                     const double *cost, const int64_t *costOff, int k, double *probs,
                                     const int64_t *probOff, int32_t *nf);

/*
 * Batched conditionCosts (assignment.h:26, assignment.cpp:439-525).  Problem b: nRow[b] x nCol[b] column-major
 * at cost + costOff[b].  out receives the conditioned goodRows[b] x nCol[b] block at the same offset; rowIdx
 * [B][maxRow] the original row of each kept row (rowIdxOut of the reference; unused tail = -1).  Host buffers.
 */
int kbest_condition_costs_f64(kbest_ctx *ctx, int B, const int32_t *nRow, const int32_t *nCol,
                              const double *cost, const int64_t *costOff, double *out, int32_t *goodRows,
                              int32_t *rowIdx, int maxRow);

/*
 * Cost block in, association probabilities out: conditionCosts -> assignmentProb(k) -> scatter back to the
 * original landmark numbering, i.e. getAssignmentProbs (assignment.cpp:57-74) from the cost matrix on, all on
 * the device.  Same argument layout as kbest_weights_batch_f64; cost blocks are the UNconditioned
 * (nL+nM) x nM matrices of computeQuadricCostMatrix (assignment.cpp:705-722); probs is [nM][nL+1] per problem.
 * One launch for frame-sized blocks.  Frames of up to 16 measurements and 64 rows (all frames of the call) are not
 * enumerated at all: conditioned costs are >= 0, so a walk over the columns that drops every partial assignment whose
 * partial sum exceeds a bound visits exactly the assignments below the bound; the bound is raised until k assignments
 * lie below it and the k cheapest of those are the answer (kbest_bnb.hip) -- gains bit for bit calcGain's sums, same
 * solutions, same probabilities as the enumeration; KBEST_NO_BNB=1 at kbest_create switches it off.  Larger frames take
 * the fused association kernel (kbest_small.hip), and -- when every frame of the
 * call has so few assignments in all, (nL+nM)!/nL! <= 2^23 (and <= 2^15 choices for the first nM-2 columns) with
 * 2 <= nM <= 8 and nL+nM <= 64: the reference's real
 * frames of 3-5 measurements (README.md:11) -- the exhaustive kernel (kbest_tiny.hip), which looks at every assignment
 * instead of enumerating the k best: same gains bit for bit (calcGain's sum), same solutions, same probabilities -- exact
 * ties included ("Order of exact ties" above: the flags of these entries are read with kbest_last_tie_flags).  KBEST_NO_TINY=1 at kbest_create
 * switches it off.  kbest_weights_batch_f64 on blocks that are conditioned already (all entries >= 0, an exact zero
 * somewhere: what conditionCosts returns and assignment.cpp:58-62 passes on) takes the same kernel; any other block
 * is answered by the enumeration kernels.
 */
int kbest_assoc_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM,
                                const double *cost, const int64_t *costOff, int k, double *probs,
                                const int64_t *probOff, int32_t *nf);

/*
 * The same on device buffers, asynchronous on `stream` (NULL = the context's stream): ONE launch -- of the bounded walk
 * (kbest_bnb.hip) when maxRawRow <= 64 and maxCol <= 16 (followed by a launch of the enumeration kernel that looks only at
 * what the walk handed back: frames with masses of equal gains), else of the fused association kernel (kbest_small.hip):
 * conditionCosts while the cost tile is loaded, the k best within the cutoff 42, the exp-weights, the scatter back --
 * for callers whose cost blocks are produced on the GPU.
 *   d_nRow[b] = d_nL[b] + d_nM[b] rows of the cost block of frame b; condition = 0: the blocks are already
 *   conditioned (assignmentProb only).  Limits of the fused kernel: nM <= 32, k <= 1024, at most 32 rows kept by
 *   conditionCosts (a frame beyond that comes back with d_nf[b] = -2 and zero probabilities: re-run it through the
 *   host-pointer entry, which falls back to the general pipeline by itself).  Needs kbest_reserve_assoc first.
 */
int kbest_assoc_probs_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                    const int32_t *d_nM, const int32_t *d_nRow, const double *d_cost,
                                    const int64_t *d_costOff, int k, int condition, double *d_probs,
                                    const int64_t *d_probOff, int32_t *d_nf, void *stream);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_assoc(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, int k);

/*
 * Batched permanentProb (assignment.h:13, assignment.cpp:145-290) for every permOpt: the EXACT association probabilities, as
 * ratios of matrix permanents (kbest_perm.hip: sums over column subsets, every term non-negative; the reference's permOpt 0,
 * Huber's sampling estimate, is answered exactly as well).  Layout of kbest_weights_batch_f64: frame b is an (nL+nM) x nM
 * column-major block at costOff[b], probs [nM][nL+1] at probOff[b]; rows r >= nL are folded into slot nL.
 * condition = 1: raw blocks, conditionCosts -> permanentProb -> scatter back (getAssignmentProbs with usePerm,
 * assignment.cpp:57-74; landmarks conditionCosts drops get exactly 0.0).  perm (may be NULL): perm[b] = the permanent of the
 * frame's toProbs matrix (after conditioning when asked for), i.e. the normaliser.  A frame whose permanent is 0 (a column
 * without a finite entry, fewer usable rows than columns) comes back with all probabilities 0 and perm[b] = 0, not NaN.
 * Limits: 1 <= nM <= KBEST_PERM_MAX_COLS (a product of one entry per column is at least exp(-42 * 16), still a normal double;
 * beyond, the sums would lose small terms silently: KBEST_ERR_UNSUPPORTED), nL + nM <= KBEST_MAX_DIM_WIDE.  A frame's result
 * does not depend on the batch it travels in, bit for bit.  Host buffers; stages, reserves and runs kbest_permanent_probs_batch_f64_dev.
 */
#define KBEST_PERM_MAX_COLS 16
int kbest_permanent_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                    const int64_t *costOff, int condition, double *probs, const int64_t *probOff,
                                    double *perm);
/* The same on device buffers, asynchronous on `stream` (NULL: the context's): one launch, no allocation.  maxRawRow / maxCol:
 * upper bounds of nL + nM / nM over the batch (a frame beyond them gets perm = 0 and its probs are left alone).  Needs
 * kbest_reserve_permanent first (KBEST_ERR_NOT_RESERVED): frames whose subset layers do not fit LDS keep them in a work space
 * in HBM, (maxRawRow + 2) * 2^maxCol * 8 bytes per frame IN FLIGHT (64 rows x 16 columns: 34 MB).  The launch has as many
 * workgroups as the chip holds at a time and as frames fit the reserved work space (at most KBEST_PERM_WORK_CAP bytes, at least one frame) and each of them
 * takes frame after frame: a large batch is processed in chunks of that many frames without a workgroup ever waiting for another. */
#define KBEST_PERM_WORK_CAP ((size_t)1 << 30)
int kbest_permanent_probs_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                        const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff,
                                        int condition, double *d_probs, const int64_t *d_probOff, double *d_perm,
                                        void *stream);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_permanent(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);
/* Diagnostic, for tests: another cap of the permanent work space (bytes; 0: KBEST_PERM_WORK_CAP again).  A lower cap means
 * fewer frames in flight -- smaller chunks -- and the same results bit for bit. */
int kbest_set_permanent_work_cap(kbest_ctx *ctx, size_t bytes);
/* Diagnostic, for tests: workgroups -- frames in flight -- of the context's last permanent launch (-1: null context). */
int kbest_last_permanent_grid(kbest_ctx *ctx);

/*
 * Joint associations DRAWN from the exact posterior (kbest_sample.hip; not in the reference, whose permOpt 0 only estimates the
 * permanent by sampling): nSample independent draws per frame, each a whole consistent hypothesis -- no two measurements on one
 * landmark -- with probability (product of its toProbs entries) / perm exactly.  Frames, layout and conditioning of
 * kbest_permanent_probs_batch_f64; the forward sums over column subsets are that entry's, and perm[b] (may be NULL) carries the
 * bits of its perm[b].  Outputs per frame b:
 *   assign   int32 [nSample][nM] at asgOff[b] (in int32s): assign[s][c] is the RAW row of the caller's block that measurement c
 *            takes in draw s, in the caller's numbering before any conditioning; a miss is the measurement's own row >= nL (with
 *            the block-diagonal miss rows of this project: nL + c), it is not folded into nL.
 *   logProb  double [nSample] at lpOff[b] (in doubles): log(product of the chosen toProbs entries) - log(perm[b]).
 * A frame whose permanent is 0 comes back with every assign -1, every logProb NaN and perm[b] = 0.
 * The uniforms -- this definition is the contract; a caller can reproduce every draw from it: row i of the frame's ACTIVE rows
 * (the rows that are not all zero after conditioning and toProbs, in order, i counted from 0) uses, for draw s of the launch,
 *   Philox4x32-10 with key (seed low word, seed high word) and counter (sampleBase + s, i >> 1, frameKey[b] low word,
 *   frameKey[b] high word); output words 0, 1 serve even i and words 2, 3 serve odd i;
 *   u = (((hi << 32) | lo) >> 11) * 2^-53, lo the first and hi the second word of the pair.
 * The walk runs over the active rows from the last to the first with S = all measurements: tot = F[i+1][S], T = u * tot,
 * acc = F[i][S]; T < acc: row i takes nothing; else for the measurements c of S in ascending order with a non-zero entry:
 * acc = acc + a[i][c] * F[i][S without c], and the first c with T < acc is taken (none, by rounding: the last c whose term was
 * > 0).  F[i][S]: the sum over the ways rows 0 .. i-1 fill exactly S.  frameKey (may be NULL: frame b has key b) makes a frame's
 * draws independent of the batch it travels in, bit for bit; counting the active rows makes them the same on a raw block with
 * condition = 1 and on its conditioned block with condition = 0.  sampleBase continues a sequence: draws sampleBase .. sampleBase +
 * nSample - 1 are what one larger call returns at those places.
 * Limits: those of the permanent entry, 1 <= nSample, sampleBase + nSample <= 2^32.  Host buffers; stages, reserves and runs the
 * device entry below.
 */
int kbest_sample_assoc_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                 const int64_t *costOff, int condition, int nSample, uint64_t seed, uint32_t sampleBase,
                                 const uint64_t *frameKey, int32_t *assign, const int64_t *asgOff, double *logProb,
                                 const int64_t *lpOff, double *perm);
/* The same on device buffers, asynchronous on `stream` (NULL: the context's): one launch, no allocation.  maxRawRow / maxCol as
 * for the permanent entry (a frame beyond them gets perm = 0, its assign and logProb are left alone).  Needs kbest_reserve_sample
 * first (KBEST_ERR_NOT_RESERVED) where the subset layers do not fit LDS: the work space, its size and its cap are the permanent
 * entry's, and kbest_reserve_sample reserves exactly what kbest_reserve_permanent does. */
int kbest_sample_assoc_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                     const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff, int condition,
                                     int nSample, uint64_t seed, uint32_t sampleBase, const uint64_t *d_frameKey,
                                     int32_t *d_assign, const int64_t *d_asgOff, double *d_logProb, const int64_t *d_lpOff,
                                     double *d_perm, void *stream);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_sample(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);

/*
 * Association probabilities by loopy belief propagation on the assignment model (kbest_lbp.hip; not in the reference): the
 * marginals of the Bethe approximation of the permanent, for the frames the exact entry above does not take -- deterministic,
 * every term non-negative, O(rows x columns) per sweep.  Layout and conditioning of kbest_permanent_probs_batch_f64: frame b is an
 * (nL+nM) x nM column-major block at costOff[b], probs [nM][nL+1] at probOff[b], rows r >= nL are folded into slot nL;
 * condition = 1: raw blocks, conditionCosts -> the iteration -> scatter back (landmarks conditionCosts drops get exactly 0.0).
 * On a = the frame's toProbs matrix (all-zero rows left out), from nu = 1, Jacobi sweeps
 *     x = a nu,  s[r][c] = sum_{r' != r} x[r'][c],  mu = a / s where a > 0 (s = 0: +inf), else 0,
 *     nu'[r][c] = 1 / (1 + sum_{c' != c} mu[r][c']),  resid = max over a > 0 of |nu' - nu|
 * until resid <= tol or maxIter sweeps (tol <= 0: exactly maxIter sweeps); then w = a nu and
 * probs[c][min(r, nL)] += w[r][c] / sum_r w[r][c].  iters (may be NULL): iters[b] = sweeps run, or -2 for an infeasible frame --
 * a column whose w sums to 0 (no finite entry, two columns forced onto one row): all its probabilities 0, not NaN.  resid (may be
 * NULL): resid[b] = the last sweep's resid.  An approximation: on 200 KITTI-like 30x10 frames the largest deviation from the exact
 * probabilities has median 0.012 and maximum 0.20 (the numpy restatement, tests/test_lbp_cpu.py), about what 1 000 best assignments give; frames
 * of a single measurement and frames whose rows have one finite entry each are exact.
 * Limits: 1 <= nM <= KBEST_LBP_MAX_COLS, nL + nM <= KBEST_MAX_DIM_WIDE (KBEST_ERR_UNSUPPORTED beyond).  A frame's result does not
 * depend on the batch it travels in, bit for bit.  Host buffers; stages, reserves and runs kbest_belief_probs_batch_f64_dev.
 */
#define KBEST_LBP_MAX_COLS 128
int kbest_belief_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                 const int64_t *costOff, int condition, double tol, int maxIter, double *probs,
                                 const int64_t *probOff, int32_t *iters, double *resid);
/* The same on device buffers, asynchronous on `stream` (NULL: the context's): one launch, no allocation.  maxRawRow / maxCol:
 * upper bounds of nL + nM / nM over the batch (a frame beyond them gets iters = -1 and its probs are left alone); the launch has
 * one wave per 64 rows of maxRawRow in a workgroup, so bounds close to the frames keep frame-sized work frame-sized.  Needs
 * kbest_reserve_belief first (KBEST_ERR_NOT_RESERVED): frames whose a and nu do not fit LDS keep them in a work space in HBM,
 * 32 * maxRawRow * maxCol bytes per frame IN FLIGHT, at most KBEST_LBP_WORK_CAP bytes in all (at least one frame); the workgroups
 * take frame after frame, none ever waits for another. */
#define KBEST_LBP_WORK_CAP ((size_t)1 << 30)
int kbest_belief_probs_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                     const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff, int condition,
                                     double tol, int maxIter, double *d_probs, const int64_t *d_probOff, int32_t *d_iters,
                                     double *d_resid, void *stream);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_belief(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);
/* Diagnostic, for tests: the LDS bytes the belief-propagation launches of this context may plan with (0: the device's limit
 * again).  A low value sends small frames through the work space in HBM -- the same results bit for bit. */
int kbest_set_belief_lds_limit(kbest_ctx *ctx, size_t bytes);

/*
 * The EXACT association probabilities by gated clusters (kbest_cluster.hip; not in the reference), for frames of up to
 * KBEST_CLUSTER_MAX_COLS measurements and KBEST_MAX_DIM_WIDE rows.  Layout and conditioning of kbest_permanent_probs_batch_f64:
 * frame b is an (nL+nM) x nM column-major block at costOff[b], probs [nM][nL+1] at probOff[b], rows r >= nL are folded into slot nL;
 * condition = 1: raw blocks, conditionCosts -> the sums -> scatter back (landmarks conditionCosts drops get exactly 0.0).
 * On a = the frame's toProbs matrix (the minimum of the WHOLE block): columns c and c' are adjacent when some row has a non-zero
 * entry in both; a cluster is a connected component of columns with every row that has a non-zero entry in one of them (a column
 * without a non-zero entry is a cluster by itself).  The permanent factorises over the clusters and so do the marginals: per
 * cluster k the sums of kbest_permanent_probs_batch_f64 on the sub-matrix give Z_k and probs[c][min(r, nL)] += w[r][c] / Z_k.
 *   logPerm (may be NULL): logPerm[b] = sum_k log Z_k in cluster order (the product itself leaves the doubles);
 *   info (may be NULL): info[b] > 0: the number of clusters, every probability is exact;  0: infeasible (some Z_k = 0): zeros and
 *       logPerm = -inf;  -1: the frame lies beyond the launch's bounds and is untouched (the device entry);  -2: a cluster of more
 *       than KBEST_CLUSTER_MAX_SIZE measurements;  -3: a cluster whose layers, (R_k + 2) * 2^m_k * 8 bytes, exceed the slot cap.
 *       -2 and -3 refuse the FRAME, not the call: its probabilities are zeros and logPerm is NaN;
 *   maxCluster (may be NULL): maxCluster[b] = measurements of the frame's largest cluster, always written;
 *   label (may be NULL; int32 [B][labelStride], labelStride >= the largest nM): label[b][c] = the lowest column of the cluster of
 *       column c, -1 for c >= nM.  Clusters are ordered by label.
 * A frame's result does not depend on the batch it travels in, on the launch's bounds or on the caps, bit for bit.  Host buffers;
 * stages, reserves and runs kbest_clustered_probs_batch_f64_dev.  nM > 128 or nL + nM > 1 024: KBEST_ERR_UNSUPPORTED.
 */
#define KBEST_CLUSTER_MAX_COLS 128                   /* per frame */
#define KBEST_CLUSTER_MAX_SIZE 16                    /* per cluster: KBEST_PERM_MAX_COLS, for its reason */
#define KBEST_CLUSTER_SLOT_CAP ((size_t)64 << 20)    /* layers of one cluster: 16 columns x 126 rows */
#define KBEST_CLUSTER_WORK_CAP ((size_t)1 << 30)
int kbest_clustered_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                    const int64_t *costOff, int condition, double *probs, const int64_t *probOff, double *logPerm,
                                    int32_t *info, int32_t *maxCluster, int32_t *label, int labelStride);
/* The same on device buffers, asynchronous on `stream` (NULL: the context's): one launch, no allocation.  maxRawRow / maxCol: upper
 * bounds of nL + nM / nM over the batch (a frame beyond them gets info = -1 and is left alone).  Needs kbest_reserve_clustered
 * first (KBEST_ERR_NOT_RESERVED): per frame IN FLIGHT a slot of min(slot cap, (maxRawRow + 2) * 2^min(maxCol, 16) * 8) bytes of
 * layers plus maxRawRow * 128 bytes, at most KBEST_CLUSTER_WORK_CAP bytes in all (at least one frame); the workgroups take frame
 * after frame, none ever waits for another. */
int kbest_clustered_probs_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                        const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff, int condition,
                                        double *d_probs, const int64_t *d_probOff, double *d_logPerm, int32_t *d_info,
                                        int32_t *d_maxCluster, int32_t *d_label, int labelStride, void *stream);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_clustered(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);
/* For tests: the layers of one cluster / the whole work space at the most (0: the default again).  The results do not depend on
 * either, bit for bit -- except that a lower slot cap refuses (-3) the frames whose clusters need more. */
int kbest_set_clustered_slot_cap(kbest_ctx *ctx, size_t bytes);
int kbest_set_clustered_work_cap(kbest_ctx *ctx, size_t bytes);
/* Diagnostic, for tests: workgroups -- frames in flight -- of the context's last clustered launch (-1: null context). */
int kbest_last_clustered_grid(kbest_ctx *ctx);

/*
 * Joint associations DRAWN from the exact posterior by gated clusters (kbest_cluster_sample.hip; not in the reference): what
 * kbest_sample_assoc_batch_f64 does, for the frames kbest_clustered_probs_batch_f64 takes -- up to KBEST_CLUSTER_MAX_COLS
 * measurements and KBEST_MAX_DIM_WIDE rows, clusters of at most KBEST_CLUSTER_MAX_SIZE measurements.  The posterior of a gated frame
 * is the product of its clusters' posteriors: one backward walk per cluster on the cluster's own forward sums F_k, the joints
 * concatenated, is an exact, independent draw of the whole frame, with probability (product of its toProbs entries) / (product of
 * the Z_k).  Frames, layout, conditioning, clusters, their order (by label) and the refusals of kbest_clustered_probs_batch_f64;
 * seed, sampleBase, frameKey, assign, asgOff, logProb and lpOff of kbest_sample_assoc_batch_f64.  Outputs per frame b:
 *   assign   int32 [nSample][nM] at asgOff[b] (in int32s): assign[s][c] is the RAW row of the caller's block that measurement c
 *            takes in draw s, in the caller's numbering before any conditioning; a miss is the measurement's own row >= nL, it is
 *            not folded into nL.
 *   logProb  double [nSample] at lpOff[b] (in doubles): sum_k (log(product of the entries chosen in cluster k) - log Z_k), one
 *            term per cluster, added left to right in cluster order starting from 0.0 (no product over the whole frame is formed:
 *            that of 128 gated entries leaves the doubles).
 *   logPerm, info, maxCluster (each may be NULL): those of kbest_clustered_probs_batch_f64, logPerm and maxCluster with its bits.
 * info = -2 (a cluster of more than KBEST_CLUSTER_MAX_SIZE measurements) and info = -3 (layers beyond the slot cap) refuse the FRAME,
 * not the call: every assign -1, every logProb NaN, logPerm NaN.  An infeasible frame (some Z_k = 0): every assign -1, every logProb
 * NaN, logPerm = -inf, info = 0.
 * The uniforms -- this definition is the contract; a caller can reproduce every draw from it: for a row of a cluster, u(s, i) takes
 * i as that row's index among the frame's ACTIVE rows (the rows that are not all zero after conditioning and toProbs, in order, i
 * counted from 0 over the WHOLE frame, not inside the cluster); for draw s of the launch,
 *   Philox4x32-10 with key (seed low word, seed high word) and counter (sampleBase + s, i >> 1, frameKey[b] low word,
 *   frameKey[b] high word); output words 0, 1 serve even i and words 2, 3 serve odd i;
 *   u = (((hi << 32) | lo) >> 11) * 2^-53, lo the first and hi the second word of the pair.
 * The walk of a cluster runs over the cluster's rows from the last to the first (ascending row order inside a cluster) with S = all
 * measurements of the cluster: tot = F_k[i+1][S] (Z_k at the cluster's last row), T = u * tot, acc = F_k[i][S]; T < acc: the row
 * takes nothing; else for the measurements c of S in ascending order with a non-zero entry: acc = acc + a[i][c] * F_k[i][S without
 * c], and the first c with T < acc is taken (none, by rounding: the last c whose term was > 0).  The whole-frame sums factorise,
 * F[i+1][S] = product over the clusters of F_k[.][S_k], so the ratio that decides row i in the whole-frame walk is the ratio inside
 * its cluster: on a frame that kbest_sample_assoc_batch_f64 takes, the decisions are the same function of the same uniforms.
 * (They are made on sums that differ in their last bits; a draw differs only where a uniform falls within those bits of a boundary.)
 * A frame's outputs are a function of (seed, frame key, draw index, frame) alone: the same bits alone, anywhere in a batch, under any
 * slot cap or work cap that still takes the frame, and for condition = 1 on the raw block against condition = 0 on its conditioned
 * block.  sampleBase continues a sequence, as in kbest_sample_assoc_batch_f64.
 * Limits: those of the clustered entry, 1 <= nSample, sampleBase + nSample <= 2^32.  Host buffers; stages, reserves and runs the
 * device entry below.
 */
int kbest_clustered_sample_assoc_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                           const int64_t *costOff, int condition, int nSample, uint64_t seed, uint32_t sampleBase,
                                           const uint64_t *frameKey, int32_t *assign, const int64_t *asgOff, double *logProb,
                                           const int64_t *lpOff, double *logPerm, int32_t *info, int32_t *maxCluster);
/* The same on device buffers, asynchronous on `stream` (NULL: the context's): one launch, no allocation.  maxRawRow / maxCol as
 * for the clustered entry (a frame beyond them gets info = -1 and nothing else of it is touched).  Needs
 * kbest_reserve_clustered_sample first (KBEST_ERR_NOT_RESERVED): the work space, its size, kbest_set_clustered_slot_cap and
 * kbest_set_clustered_work_cap are the clustered entry's, and kbest_reserve_clustered_sample reserves exactly what
 * kbest_reserve_clustered does. */
int kbest_clustered_sample_assoc_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                               const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff, int condition,
                                               int nSample, uint64_t seed, uint32_t sampleBase, const uint64_t *d_frameKey,
                                               int32_t *d_assign, const int64_t *d_asgOff, double *d_logProb, const int64_t *d_lpOff,
                                               double *d_logPerm, int32_t *d_info, int32_t *d_maxCluster, void *stream);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_clustered_sample(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);

/*
 * Hybrid association probabilities (not in the reference): every gated frame of up to KBEST_CLUSTER_MAX_COLS measurements is
 * answered -- exactly on every cluster the clustered kernel can take, by assignmentProb (kBest2DCutoff(k, 42) -> weights) on the
 * clusters it cannot.  The marginals factorise over the clusters, and so does a k-best approximation: all k assignments are spent
 * on the cluster that needs them.
 *
 * kbest_clustered_partial_batch_f64_dev: kbest_clustered_probs_batch_f64_dev in its PARTIAL mode (a second instantiation of the
 * kernel; the plain entries do not run it).  maxExact (1 .. 16, 0 = 16): the largest cluster answered exactly.  A cluster of more
 * columns, or one whose layers exceed the slot (the plain entry's -3), is OPEN: it does not refuse the frame.  The columns of every
 * other cluster are bit-identical to kbest_clustered_probs_batch_f64, whatever maxExact is and whatever else is open; the
 * columns of open clusters stay 0.0.  Per frame b (device buffers of the caller, all required):
 *   d_nOpen[b]: its open clusters, in label order j = 0 .. nOpen - 1;
 *   d_openDesc (int32 [B][descStride][4], descStride >= maxCol): { root label, m_k, nL_k, R_k } of open cluster j: its columns
 *       are those with d_label[b][c] == root (ascending), nL_k of its R_k rows are landmarks (raw row < nL);
 *   d_openRows (int32 [B][rowStride], rowStride >= maxRawRow): those landmark rows in the caller's numbering, ascending, cluster
 *       after cluster (cluster j starts at the sum of nL_k' over j' < j);
 *   d_sub (doubles, sized and addressed like d_cost): from d_costOff[b] on, cluster after cluster, the (nL_k + m_k) x m_k
 *       column-major sub-block of open cluster j: the cluster's R_k rows in ascending raw order (its landmark rows first, then
 *       its rows >= nL -- in the reference's layout the miss rows of its columns, in column order), then rows that are all +inf up
 *       to nL_k + m_k; columns ascending.  An entry is the value toProbs is applied to -- the raw cost, x - colMin[c] with
 *       condition = 1: the bits kbest_condition_costs_f64 gives -- and +inf wherever the frame's gate (block minimum + 42) makes a
 *       zero.  The sum of (nL_k + m_k) m_k over a frame never exceeds (nL + nM) nM.  Nothing else of d_sub is written.
 *   d_info[b]: the number of clusters, open ones included;  0: an ANSWERED cluster has Z_k = 0: zeros, logPerm -inf, nOpen 0 (what
 *       was written to d_sub / d_openDesc / d_openRows before that was known stays);  -1: beyond the launch's bounds;  -2: an open
 *       cluster holds more rows >= nL than columns (not the reference's block-diagonal layout): zeros, logPerm NaN, nOpen 0;
 *   d_logPerm[b]: the sum over the answered clusters only;  d_maxCluster, d_label: as the plain entry.
 * Asynchronous, never allocates or synchronises; needs kbest_reserve_clustered (the same work space and the same launch plan).
 *
 * kbest_hybrid_probs_batch_f64 (host buffers, synchronous): the partial kernel on the whole batch; the descriptors and ONLY the
 * open clusters' sub-blocks come back; the open clusters of ALL frames go through kbest_weights_batch_f64's path as one batch (with
 * the context's tie settings); their [m_k][nL_k + 1] probabilities are scattered into the frames on the host.
 *   method[b]:  0: every cluster exact, the bits of kbest_clustered_probs_batch_f64;  1: some clusters enumerated and every
 *       enumeration ended before k (nf < k): everything within the cutoff 42 was weighed;  2: some enumeration was cut at k;
 *       -2: infeasible, zeros (an answered cluster with Z = 0 or an open one without an assignment);  -1: refused (d_info < 0);
 *   nOpen, maxCluster (may be NULL): as above.  k < 1 or maxExact outside 0 .. 16: KBEST_ERR_BAD_ARG.
 */
int kbest_clustered_partial_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                          const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff, int condition,
                                          int maxExact, double *d_probs, const int64_t *d_probOff, double *d_logPerm,
                                          int32_t *d_info, int32_t *d_maxCluster, int32_t *d_label, int labelStride,
                                          int32_t *d_nOpen, int32_t *d_openDesc, int descStride, int32_t *d_openRows, int rowStride,
                                          double *d_sub, void *stream);
int kbest_hybrid_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                 const int64_t *costOff, int condition, int k, int maxExact, double *probs, const int64_t *probOff,
                                 int32_t *method, int32_t *nOpen, int32_t *maxCluster);
/*
 * Exact association probabilities of clusters of 17 .. 20 measurements (kbest_bigcluster.hip; not in the reference): a third tier
 * of the exact subset sums -- ONE cluster over the whole chip, its layers in HBM -- fed by what the partial mode above hands out.
 *
 * The 16 of KBEST_CLUSTER_MAX_SIZE has a numeric reason (entries of a lie in (e^-42, 1]: a product of 17 may leave the normal
 * doubles) and a structural one (one workgroup does a whole cluster).  This tier lifts both.  Per cluster it works on
 * a'[r][c] = exp(colMin_c - x[r][c]), colMin_c the smallest finite entry of column c INSIDE the sub-block: a column factor is the
 * only rescaling that commutes with the recurrence, it leaves the marginals alone, and log Z_k = log Z'_k - sum_c colMin_c in the
 * units a = exp(-x).  What remains: every a' lies in (0, 1] and every column holds a 1, so Z'_k leaves the normal doubles only when
 * EVERY complete assignment of the cluster costs about 700 more than the sum of its column minima.
 * RANGE (this tier, the frontier tier and the frontier sampler below): a cluster is answered while Z'_k >= 2^-970 = e^-672.3 --
 * every term within 2^-52 of Z'_k is then a normal double.  Below that, Z'_k = 0 included, the tier counts the complete assignments
 * of the pattern a' > 0 (the same recurrence with every non-zero entry 1: a sum of ones cannot underflow).  None, and no finite
 * entry whose a' underflowed to 0: info 0, INFEASIBLE -- info 0, method -2, logPerm -inf and assign -1 always mean that the cluster
 * has no complete assignment.  Else the cluster is DECLINED: info KBEST_INFO_OUT_OF_RANGE (-5), its outputs untouched, as with the
 * refusals -3 and -4.  In the host frame entries a declined cluster goes on to the next tier (frontier -> big-cluster -> k-best
 * path; with k = 0 it refuses its frame: method -1, logPerm NaN); in the one-stream device entries it refuses its frame.
 *
 * kbest_bigcluster_probs_f64_dev: n clusters.  m[k] (1 .. KBEST_BIGCLUSTER_MAX_SIZE), nLk[k], subOff[k], probOff[k] are HOST arrays
 * (the launches are planned from them); the data is on the device: cluster k is the (nLk + m) x m column-major block at
 * d_sub + subOff[k] in the format of d_sub above (+inf: zero; rows that are all +inf are left out), d_probs + probOff[k] takes its
 * [m][nLk + 1] probabilities (sub-block row i < nLk -> slot i, rows >= nLk -> slot nLk), d_logZ[k] (may be NULL) its log Z_k in
 * the units a = exp(-x) -- add m * (the frame's block minimum) for the frame's units a = exp(min - x) --, d_info[k] (may be NULL):
 * 1 answered;  0: no complete assignment (zeros, log Z_k = -inf);  KBEST_INFO_OUT_OF_RANGE (-5): declined, Z'_k < 2^-970 (RANGE
 * above);  -3: its layers, (nLk + m + 3) * 2^m * 8 bytes (R_k counted as the sub-block's rows), exceed the work cap.  After -5 and
 * -3 its outputs are untouched.
 * One launch per row forward and backward: launches of one stream order the layers, no kernel waits for another workgroup.  The
 * workgroups of every launch follow from m alone and no floating-point atomics are used: a cluster gives the same bits alone, in
 * any batch and under any cap.  Clusters share launches as far as the work space holds their layers (at most KBEST_BIGCLUSTER_WORK_CAP
 * bytes in flight), else they run one after another.  Asynchronous on `stream` (NULL: the context's), allocates nothing: needs
 * kbest_reserve_bigcluster(ctx, maxM, maxRows) first -- layers of min(cap, (maxRows + 3) * 2^maxM * 8) bytes, maxRows the largest
 * nLk + m -- else KBEST_ERR_NOT_RESERVED.  m outside 1 .. 20: KBEST_ERR_BAD_ARG.
 *
 * kbest_hybrid_exact_probs_batch_f64 (host buffers, synchronous): kbest_hybrid_probs_batch_f64 with this tier between the two.  The
 * partial kernel runs as there; every open cluster of at most maxBig (0 .. 20) measurements whose layers fit the work cap is
 * answered by the tier from the sub-block that already lies on the device; the remaining open clusters, those the tier declines
 * (-5) among them, go through the k-best path unchanged when k >= 1; with k = 0 a frame that has one is refused (method -1, zeros,
 * logPerm NaN).
 *   method[b]:  0: every cluster exact (either tier);  1 / 2 / -2 / -1: as kbest_hybrid_probs_batch_f64; a big cluster without a
 *       complete assignment (info 0): -2;
 *   nOpen[b] (may be NULL): the clusters the partial kernel left open;  nBig[b] (may be NULL): those of them this tier answered;
 *   logPerm[b] (may be NULL): the sum of log Z_k over all exactly answered clusters in the frame's units (method 0: the definition
 *       of kbest_clustered_probs_batch_f64);  -inf for method -2, NaN for method -1.
 * With maxBig = 0 and k >= 1 every common output carries the bits of kbest_hybrid_probs_batch_f64.  maxBig outside 0 .. 20, maxExact
 * outside 0 .. 16 or k < 0: KBEST_ERR_BAD_ARG.
 */
#define KBEST_BIGCLUSTER_MAX_SIZE 20
#define KBEST_INFO_OUT_OF_RANGE (-5)  /* d_info of the column-scaled tiers: declined, Z' < 2^-970 although an assignment exists */
#define KBEST_BIGCLUSTER_WORK_CAP ((size_t)1 << 30)  /* the layers of the clusters in flight */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_bigcluster(kbest_ctx *ctx, int maxM, int maxRows);
/* For tests: the layers in flight at the most (0: the default again).  The results do not depend on it, bit for bit -- except that
 * a cluster whose own layers exceed it is not answered (-3). */
int kbest_set_bigcluster_work_cap(kbest_ctx *ctx, size_t bytes);
int kbest_bigcluster_probs_f64_dev(kbest_ctx *ctx, int n, const int32_t *m, const int32_t *nLk, const int64_t *subOff,
                                   const int64_t *probOff, const double *d_sub, double *d_probs, double *d_logZ, int32_t *d_info,
                                   void *stream);
int kbest_hybrid_exact_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                       const int64_t *costOff, int condition, int k, int maxExact, int maxBig, double *probs,
                                       const int64_t *probOff, double *logPerm, int32_t *method, int32_t *nOpen, int32_t *nBig,
                                       int32_t *maxCluster);
/*
 * Exact association probabilities of sparse clusters of up to 64 measurements (kbest_frontier.hip; not in the reference): a fourth
 * tier of the exact subset sums whose limit is a cluster's structure, not its column count.
 *
 * The clusters the gate opens are chains of overlapping neighbourhoods.  With the rows taken in a good order a column is a state
 * bit only between its first and its last non-zero row: before, it is unused; after, it must be used.  The order is greedy and a
 * pure function of the pattern: of the unprocessed rows the one that leaves the fewest columns open, then the one that opens the
 * fewest, then the lowest (DESIGN.md section 14 has the two counts).  W is the largest number of columns open during a step; the
 * sweep keeps sum_i 2^|open after i rows| doubles of forward layers and two buffers of 2^W.  Scaling as the big-cluster tier's:
 * a'[r][c] = exp(colMin_c - x[r][c]), log Z_k = log Z'_k - sum_c colMin_c.
 *
 * kbest_frontier_probs_f64_dev: n clusters, arguments as kbest_bigcluster_probs_f64_dev with m[k] in 1 .. KBEST_FRONTIER_MAX_COLS
 * and nLk[k] in 0 .. 1024, plus d_width[k] (may be NULL): the cluster's W, written for every cluster.  d_info[k]: 1 answered;
 * 0: no complete assignment (zeros, log Z_k = -inf) -- fewer counting rows than columns, or two columns whose only row is the same
 * row;  KBEST_INFO_OUT_OF_RANGE (-5): declined, Z'_k < 2^-970 although the pattern has a complete assignment (RANGE at the
 * big-cluster tier; the count is one more forward sweep with every non-zero entry 1, run only for such a cluster);
 * -4: W > KBEST_FRONTIER_MAX_WIDTH;  -3: its layers exceed the slot (KBEST_FRONTIER_SLOT bytes).  A refused cluster's probabilities
 * and log Z_k are untouched, and all three refusals follow from the cluster alone -- never from the device, the batch or the cap.
 * One workgroup takes a cluster at a time and the grid strides over the clusters: ONE launch per KB_FRONTIER_PACK = 128 clusters (the
 * descriptors travel as a kernel argument), no workgroup waits for another, no floating-point atomics: a cluster gives the same bits
 * alone, anywhere in a batch and under any work cap.  Asynchronous on `stream` (NULL: the context's), allocates nothing: needs
 * kbest_reserve_frontier(ctx, n, maxM, maxRows) first -- a slot and a plan of maxRows (the largest nLk + m) steps for each of the
 * clusters in flight, at most KBEST_FRONTIER_WORK_CAP bytes of slots -- else KBEST_ERR_NOT_RESERVED.  m outside 1 .. 64:
 * KBEST_ERR_BAD_ARG.
 *
 * kbest_hybrid_frontier_probs_batch_f64 (host buffers, synchronous): kbest_hybrid_exact_probs_batch_f64 with this tier first among
 * the open clusters.  The partial kernel runs as there; every open cluster of at most 64 measurements goes through the tier from
 * the sub-block that already lies on the device; what it refuses (-3, -4, -5, or W > maxWidth, 0 .. 16) goes to the big-cluster tier
 * when it has at most maxBig measurements, the rest to the k-best path when k >= 1; with k = 0 a frame that has one is refused.
 *   method[b], nOpen[b], nBig[b], maxCluster[b], logPerm[b]: as kbest_hybrid_exact_probs_batch_f64 (method 0: every cluster exact by
 *       any tier; logPerm sums log Z_k over all exactly answered clusters);  nFrontier[b] (may be NULL): the clusters this tier answered.
 * With maxWidth = 0 every common output carries the bits of kbest_hybrid_exact_probs_batch_f64.  maxWidth outside 0 .. 16 or an
 * argument kbest_hybrid_exact_probs_batch_f64 refuses: KBEST_ERR_BAD_ARG.
 */
#define KBEST_FRONTIER_MAX_COLS 64
#define KBEST_FRONTIER_MAX_WIDTH 16
#define KBEST_FRONTIER_SLOT ((size_t)4 << 20)       /* the layers of one cluster */
#define KBEST_FRONTIER_WORK_CAP ((size_t)1 << 30)   /* the slots of the clusters in flight */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_frontier(kbest_ctx *ctx, int n, int maxM, int maxRows);
/* For tests: the slots in flight at the most / the layers of one cluster at the most (0: the default again).  The results do not
 * depend on the first, bit for bit; a cluster whose layers exceed the second is not answered (-3). */
int kbest_set_frontier_work_cap(kbest_ctx *ctx, size_t bytes);
int kbest_set_frontier_slot(kbest_ctx *ctx, size_t bytes);
int kbest_frontier_probs_f64_dev(kbest_ctx *ctx, int n, const int32_t *m, const int32_t *nLk, const int64_t *subOff,
                                 const int64_t *probOff, const double *d_sub, double *d_probs, double *d_logZ, int32_t *d_info,
                                 int32_t *d_width, void *stream);
int kbest_hybrid_frontier_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                          const int64_t *costOff, int condition, int k, int maxExact, int maxBig, int maxWidth,
                                          double *probs, const int64_t *probOff, double *logPerm, int32_t *method, int32_t *nOpen,
                                          int32_t *nBig, int32_t *maxCluster, int32_t *nFrontier);
/*
 * Draws from the exact posterior of sparse clusters (kbest_frontier_sample.hip; not in the reference): whole joint associations of a
 * cluster the frontier tier answers, drawn by a backward walk over the forward layers that tier keeps.  Nothing new is summed: the
 * plan, the scaling a'[r][c] = exp(colMin_c - x[r][c]) and the forward sweep are kbest_frontier.hip's, and d_logZ[k], d_info[k]
 * (1 / 0 / -3 / -4 / -5) and d_width[k] carry the bits of kbest_frontier_probs_f64_dev on the same cluster.  No backward sweep.
 *
 * The walk of one draw: S = empty after the last row; from the last step of the plan to the first, with row r of step i:
 * T = S | closing_i, tot = F_{i+1}[S], Tt = u tot; where T holds no new column, acc = F_i[T] and Tt < acc leaves the row
 * unassigned; else the columns c of T in the row, ascending, whose T \ c holds no new column: acc += a'[r][c] F_i[T \ c], the
 * first c with Tt < acc is taken (if rounding leaves none: the last c whose term was > 0).  Rows that are all +inf are no steps.
 * The uniform u is Philox4x32-10 with the key (seed low word, seed high word) and the counter
 *     (sampleBase + s, 0x80000000 | (q >> 1), frameKey low word, frameKey high word);
 * output words 0, 1 serve an even q, words 2, 3 an odd q, and u is built from the pair as in kbest_sample_assoc_batch_f64.
 * q = d_rowKey[rowKeyOff[k] + r] is the caller's integer for row r of the sub-block (0 <= q).  Bit 31 of the second counter word
 * keeps these uniforms disjoint from those of kbest_clustered_sample_assoc_batch_f64, whose second word is at most 511: no uniform
 * is ever shared between a small cluster and a frontier cluster of one frame.
 *
 * kbest_frontier_sample_f64_dev: n clusters; m, nLk, subOff and d_sub as kbest_frontier_probs_f64_dev; frameKeyOfCluster[k] (host,
 * may be NULL: 0) the frame key of the cluster's frame.  Out, on the device: d_assignLocal + asgOff[k]: int32 [nSample][m_k], the
 * row of the sub-block every column takes; d_logTerm + ltOff[k]: double [nSample], sum_c (colMin_c - x[r_c][c]) - log Z'_k over the
 * cluster's columns in ascending order -- every log from the cost itself, no log of a product.  d_info[k] = 0 (no complete
 * assignment): -1 and NaN; a refused cluster (-3, -4, or -5: declined, Z'_k < 2^-970): neither is touched.  One workgroup takes a
 * cluster at a time, the grid strides over the clusters, ONE launch per 64 clusters, no workgroup waits for another, no floating-point atomics: a cluster's outputs are a
 * function of (cluster, row keys, seed, frame key, draw index) alone -- the same bits alone, anywhere in a batch and under any
 * work cap.  Asynchronous on `stream` (NULL: the context's), allocates nothing: kbest_reserve_frontier_sample reserves exactly
 * what kbest_reserve_frontier does, and without it the entry returns KBEST_ERR_NOT_RESERVED; kbest_set_frontier_work_cap and
 * kbest_set_frontier_slot apply as they do to the marginal tier.  The argument checks of kbest_frontier_probs_f64_dev, plus
 * 1 <= nSample and sampleBase + nSample <= 2^32: KBEST_ERR_BAD_ARG.
 *
 * kbest_hybrid_frontier_sample_assoc_batch_f64 (host buffers, synchronous): nSample whole hypotheses for every frame that
 * kbest_hybrid_frontier_probs_batch_f64(k = 0, maxBig = 0) answers.  Frames, cost, costOff, condition, maxExact (0: 16) and
 * maxWidth (0 .. 16) as there; nSample, seed, sampleBase, frameKey, assign, asgOff, logProb and lpOff as
 * kbest_clustered_sample_assoc_batch_f64.  Every cluster of at most maxExact measurements is drawn by the walk of
 * kbest_clustered_sample_assoc_batch_f64 with its contract unchanged (a second instantiation of its kernel that leaves the open
 * clusters alone): the uniforms are indexed by the frame's ACTIVE rows and the rows of a cluster are walked from last to first; on
 * a frame without an open cluster assign, logProb and logPerm carry the bits of kbest_clustered_sample_assoc_batch_f64.  Every
 * open cluster goes through kbest_frontier_sample_f64_dev with q = the RAW row of the caller's block: a landmark row's entry in the
 * partial kernel's row list, nL + c for the miss row of column c (in general: the row's own index in the block); its draws are
 * mapped back to raw rows.  logProb[s] is built in two passes: the small clusters' terms in label order from 0.0, then the open
 * clusters' terms in label order.  method[b], nOpen[b], nFrontier[b], maxCluster[b] (the last three may be NULL) and logPerm[b]
 * (may be NULL): those of kbest_hybrid_frontier_probs_batch_f64(k = 0, maxBig = 0) on the same frames, bit for bit.  A frame with
 * a cluster nobody takes (more than 64 measurements, -3, -4, -5, or W > maxWidth): method -1, every assign -1, every logProb NaN; an
 * infeasible frame: method -2, -1s and NaNs; the call itself succeeds in both cases.
 * NOTE: the draws with condition = 1 on a raw block and with condition = 0 on its conditioned block are NOT equal for the open
 * clusters, because q is a raw row and conditionCosts renumbers the rows it keeps.  Both are exact draws from the same posterior.
 * The small clusters keep that equality (their uniforms are indexed by the active rows, which conditioning does not renumber).
 */
int kbest_hybrid_frontier_sample_assoc_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                                 const int64_t *costOff, int condition, int maxExact, int maxWidth, int nSample,
                                                 uint64_t seed, uint32_t sampleBase, const uint64_t *frameKey, int32_t *assign,
                                                 const int64_t *asgOff, double *logProb, const int64_t *lpOff, double *logPerm,
                                                 int32_t *method, int32_t *nOpen, int32_t *nFrontier, int32_t *maxCluster);
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_frontier_sample(kbest_ctx *ctx, int n, int maxM, int maxRows);
int kbest_frontier_sample_f64_dev(kbest_ctx *ctx, int n, const int32_t *m, const int32_t *nLk, const int64_t *subOff,
                                  const double *d_sub, const int32_t *d_rowKey, const int64_t *rowKeyOff,
                                  const uint64_t *frameKeyOfCluster, int nSample, uint64_t seed, uint32_t sampleBase,
                                  int32_t *d_assignLocal, const int64_t *asgOff, double *d_logTerm, const int64_t *ltOff,
                                  double *d_logZ, int32_t *d_info, int32_t *d_width, void *stream);
/*
 * Draws for every gated frame (kbest_table_sample.hip; not in the reference): whole joint associations of a cluster no exact tier
 * takes, drawn from a table of its k best assignments under the weights assignmentProb gives them (assignment.cpp:616-648).
 *
 * The distribution.  For one problem: gain[0 .. nf-1] in ascending table order and row4col[j][0 .. m-1], in the layout
 * kbest_batch_f64_dev writes: [n][k][maxCol] int32, [n][k] double, [n] int32 (an nf beyond k counts as k).
 *   w_j = exp(gain_0 - gain_j) where gain_0 + cutoff > gain_j, strictly; otherwise slot j is skipped and has weight 0.
 *   P_j = P_{j-1} + w_j, added left to right from 0.0 in table order; total = P_{nf-1}.
 *   Draw s takes the FIRST j with T < P_j, where T = u total.  If rounding leaves none, it takes the last j whose weight was > 0.
 *   logTerm[s] = (gain_0 - gain_j) - log(total): no log of a product.  assignLocal[s][c] = row4col[j][c].  pick[s] = j.
 * The uniform.  Philox4x32-10.  The key is the seed's two words.  The counter is
 *     (sampleBase + s, 0x40000000 | clusterKey, frameKey low word, frameKey high word).
 * u = (((word1 << 32) | word0) >> 11) * 2^-53, from words 0 and 1.  clusterKey < 2^30, else KBEST_ERR_BAD_ARG.
 * Bit 30 set and bit 31 clear keeps these uniforms disjoint from those of kbest_clustered_sample_assoc_batch_f64, whose second
 * word is at most 511, and from those of kbest_frontier_sample_f64_dev, whose second word has bit 31 set: no uniform is ever
 * shared between a small cluster, a frontier cluster and an enumerated cluster of one frame.
 *
 * kbest_table_sample_f64_dev: n problems; k (1 .. KBEST_TABLE_SAMPLE_MAX_K: the running sums of a problem lie in LDS) and maxCol
 * the strides of the tables; m[i] (host) the columns of problem i; d_row4col, d_gain, d_nf on the device; cutoff the reference's
 * (42 in assignmentProb); clusterKey[i] and frameKeyOfCluster[i] (host, each may be NULL: 0).  Out, on the device:
 * d_assignLocal + asgOff[i]: int32 [nSample][m_i]; d_logTerm + ltOff[i]: double [nSample]; d_pick (may be NULL): int32 [n][nSample];
 * d_info[i] (may be NULL): 1 drawn; 0: nf <= 0 (or no slot has a weight > 0) -- assignLocal -1, logTerm NaN, pick -1; -1: m_i
 * outside 1 .. maxCol -- nothing is touched.  One workgroup of 256 per problem, the grid strides over the problems of a launch,
 * ONE launch per 64 problems; shapes, offsets and keys travel as kernel arguments: the entry copies nothing, allocates nothing and
 * needs no reservation.  No workgroup waits for another, no floating-point atomics, no sum over threads: a problem's outputs are a
 * function of (table, cutoff, seed, keys, draw index) alone.  Asynchronous on `stream` (NULL: the context's).  k outside
 * 1 .. 4096, maxCol < 1, nSample < 1, sampleBase + nSample > 2^32, a negative offset: KBEST_ERR_BAD_ARG.
 *
 * kbest_hybrid_sample_assoc_batch_f64 (host buffers, synchronous): the drawing twin of
 * kbest_hybrid_frontier_probs_batch_f64(k, maxBig = 0) -- kbest_hybrid_frontier_sample_assoc_batch_f64 with int k after condition
 * and nEnum after nFrontier, and one body with it.  k = 0: that entry, step for step and bit for bit.  k >= 1 (up to
 * KBEST_TABLE_SAMPLE_MAX_K): every open cluster the frontier sampler does not take (more than 64 measurements, info < 0,
 * W > maxWidth, or maxWidth = 0) is enumerated instead of refusing its frame: kBest2DCutoff(k, 42) on the (nL_k + m_k) x m_k
 * sub-block the partial kernel handed out (use_cutoff = 1, cutoff = 42, KBEST_FLAG_CANONICAL_TIES), all such clusters of a call
 * as ONE batch, then ONE call of kbest_table_sample_f64_dev with clusterKey = the cluster's label (its first column) and the
 * frame's key.  So the distribution drawn from is the one whose marginals kbest_hybrid_frontier_probs_batch_f64(k, maxBig = 0)
 * returns for that cluster.  Local rows map to raw rows through the list the frontier clusters use (the partial kernel's row
 * list, then the rows >= nL the gate finds, ascending), and ONE loop over the frame's open clusters in label order joins the
 * draws, whichever tier answered: assign[s][col_j] = the key of the local row (-1 beyond the rows that count),
 * logProb[s] = logProb[s] + term[s], after the small clusters' sum.
 *   method[b]: 0 everything exact; 1 every enumeration complete within the cutoff (nf < k); 2 some enumeration cut at k; -2 some
 *       cluster without a feasible assignment (nf <= 0 included): -1s, NaNs, logPerm -inf; -1 refused by the partial kernel: NaN.
 *   nEnum[b] (may be NULL): the enumerated clusters of the frame; 0 where method < 0.
 *   logPerm[b]: the sum over the exactly answered clusters only; the enumerated ones add nothing.
 *   logProb of a frame with method 1 or 2 is the log-probability under the product of the exact posteriors of its exactly
 *   answered clusters and the TRUNCATED posteriors (the k best within the cutoff, renormalised) of its enumerated ones.
 */
#define KBEST_TABLE_SAMPLE_MAX_K 4096
int kbest_table_sample_f64_dev(kbest_ctx *ctx, int n, int k, int maxCol, const int32_t *m, const int32_t *d_row4col,
                               const double *d_gain, const int32_t *d_nf, double cutoff, const uint32_t *clusterKey,
                               const uint64_t *frameKeyOfCluster, int nSample, uint64_t seed, uint32_t sampleBase,
                               int32_t *d_assignLocal, const int64_t *asgOff, double *d_logTerm, const int64_t *ltOff,
                               int32_t *d_pick /* or NULL */, int32_t *d_info, void *stream);
int kbest_hybrid_sample_assoc_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *cost,
                                        const int64_t *costOff, int condition, int k, int maxExact, int maxWidth, int nSample,
                                        uint64_t seed, uint32_t sampleBase, const uint64_t *frameKey, int32_t *assign,
                                        const int64_t *asgOff, double *logProb, const int64_t *lpOff, double *logPerm, int32_t *method,
                                        int32_t *nOpen, int32_t *nFrontier, int32_t *nEnum, int32_t *maxCluster);
/*
 * Asynchronous exact hybrid probabilities (kbest_hybrid.hip; not in the reference): the whole exact path of
 * kbest_hybrid_frontier_probs_batch_f64(k = 0, maxBig = 0) on buffers that already lie on the device, on ONE stream -- the partial
 * clustered kernel, a gather of the open clusters of all frames into one list (frame order, then label order: a prefix sum, no
 * atomics), the frontier sweep over that list in one launch, and the scatter of every cluster's [m_k][nL_k + 1] block into its
 * frame.  No host read, no synchronise, no allocation; stream order between the four launches is the only synchronisation.  Every
 * output carries the bits of that host entry.  The big-cluster tier and the k-best leg stay host-only: a frame that holds a cluster
 * the frontier tier does not take is refused here, as there, and may be sent to the host entry.
 *
 * kbest_hybrid_frontier_probs_batch_f64_dev: frames, d_cost, d_costOff, d_probs, d_probOff, condition and d_sub (the caller's work
 * buffer, sized and addressed like d_cost: the host does not know the extent of the cost buffer) as in
 * kbest_clustered_partial_batch_f64_dev.  maxExact 0 .. 16 (0 = 16), maxWidth 1 .. 16: maxWidth = 0 would turn the tier off, which
 * with k = 0 answers nothing new -- KBEST_ERR_BAD_ARG, as everything outside those ranges.
 *   d_method[b] (required):  0: every cluster exact;  -2: an answered or frontier cluster without a complete assignment (Z = 0 /
 *       info 0): the frame is zeros, logPerm -inf;  -1: the partial kernel's d_info < 0, or an open cluster nobody took (more than
 *       64 measurements, frontier info -3, -4 or -5 (declined, out of range), or W > maxWidth): a frame with open clusters is zeros,
 *       nFrontier 0, logPerm NaN;
 *   d_logPerm[b], d_nOpen[b], d_nFrontier[b], d_maxCluster[b] (each may be NULL): as kbest_hybrid_frontier_probs_batch_f64.
 * d_probs: the entry writes EVERY element of the slice of every frame within the launch bounds (the partial kernel zeroes the slice
 * before anything else), and nothing outside the slices.  A frame beyond the bounds (nM < 1, nM > maxCol, nL < 0 or
 * nL + nM > maxRawRow: method -1) is not touched at all -- neither its slice nor d_maxCluster[b]; a caller that wants zeros there,
 * as the host entry's zeroed buffer gives, zeroes d_probs before the call.
 * The context holds everything else: kbest_reserve_hybrid_dev(ctx, B, maxRawRow, maxCol) sizes, from those three alone, the
 * clustered work space (kbest_reserve_clustered), the frontier slots and plans (clusters of up to min(maxCol, 64) measurements and
 * maxRawRow rows, as many in flight as KBEST_FRONTIER_WORK_CAP and the chip allow), labels, descriptors and row lists, the list of
 * up to B * maxCol clusters, their log Z_k | info | width, and maxCol * maxRawRow packed probabilities per frame.  Without it, or
 * with a call beyond what was reserved: KBEST_ERR_NOT_RESERVED.  B = 0: KBEST_OK, nothing launched.  Asynchronous on `stream` (NULL:
 * the context's); takes the context's lock like the other _dev entries; two calls on one stream need no synchronise between them.
 */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_hybrid_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol);
int kbest_hybrid_frontier_probs_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                              const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff, int condition,
                                              int maxExact, int maxWidth, double *d_sub, double *d_probs, const int64_t *d_probOff,
                                              double *d_logPerm, int32_t *d_method, int32_t *d_nOpen, int32_t *d_nFrontier,
                                              int32_t *d_maxCluster, void *stream);
/*
 * Asynchronous exact hybrid draws (kbest_hybrid_sample.hip; not in the reference): kbest_hybrid_frontier_sample_assoc_batch_f64 on
 * buffers that already lie on the device, on ONE stream -- the partial clustered kernel, the clustered sampler's second
 * instantiation, the gather of the open clusters of all frames into one list (frame order, then label order: a prefix sum, no
 * atomics), a kernel that finds every listed cluster's row keys (the RAW rows of the caller's block: the landmark rows of the
 * partial kernel's row list, then the rows >= nL that have a non-zero entry in a column of the cluster, by the gate of the partial
 * kernel restated with comparisons and differences), the sampler of kbest_frontier_sample_f64_dev over that list in ONE launch, and
 * a join that maps the local rows back and adds the terms.  No host read, no synchronise, no allocation, no floating-point atomics,
 * no workgroup waits for another; stream order between the launches is the only synchronisation.  Every output carries the bits of
 * the host entry on the same frames, arguments, seed, keys and sampleBase: assign, logProb and logPerm (NaN as NaN, -inf as -inf),
 * method, nOpen, nFrontier, maxCluster.  A frame's outputs are a function of (frame, seed, frame key, draw index) alone.
 *
 * kbest_hybrid_frontier_sample_assoc_batch_f64_dev: frames, d_cost, d_costOff, condition, maxExact (0 .. 16, 0 = 16) and d_sub (the
 * caller's work buffer, sized and addressed like d_cost) as in kbest_hybrid_frontier_probs_batch_f64_dev; maxWidth 0 .. 16, where 0
 * refuses every frame with an open cluster, as on the host; nSample >= 1, seed, sampleBase (sampleBase + nSample <= 2^32),
 * d_frameKey (may be NULL: frame b has key b), d_assign, d_asgOff, d_logProb and d_lpOff as in
 * kbest_clustered_sample_assoc_batch_f64_dev.  Anything outside those ranges: KBEST_ERR_BAD_ARG.  d_method is required; d_logPerm,
 * d_nOpen, d_nFrontier and d_maxCluster may be NULL.
 *   method -1 or -2 on a frame within the launch bounds: every assign -1, every logProb NaN, as on the host.
 *   A frame beyond the bounds (nM < 1, nM > maxCol, nL < 0 or nL + nM > maxRawRow): method -1, nOpen and nFrontier 0, logPerm NaN;
 *   its assign, logProb and maxCluster are not touched.
 *   An open cluster whose rows the key kernel cannot tell (the host entry's KBEST_ERR_INTERNAL) is not sent: method -1.
 * The context holds everything else: kbest_reserve_hybrid_sample_dev(ctx, B, maxRawRow, maxCol, nSample) sizes, from those four
 * alone, what kbest_reserve_hybrid_dev and kbest_reserve_clustered_sample size, and per frame its offset into the packed scratch,
 * two sums and the sampler's info, maxRawRow row keys and nSample * maxCol local rows, and per cluster of the list its key item and
 * nSample terms.  A reservation never shrinks: it is sized for the largest of each of the four numbers so far.  Without it, or
 * with a call beyond it in any of the four numbers: KBEST_ERR_NOT_RESERVED.  B = 0: KBEST_OK, nothing
 * launched.  Asynchronous on `stream` (NULL: the context's); two calls on one stream need no synchronise between them.
 */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_hybrid_sample_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, int nSample);
int kbest_hybrid_frontier_sample_assoc_batch_f64_dev(kbest_ctx *ctx, int B, int maxRawRow, int maxCol, const int32_t *d_nL,
                                                     const int32_t *d_nM, const double *d_cost, const int64_t *d_costOff,
                                                     int condition, int maxExact, int maxWidth, int nSample, uint64_t seed,
                                                     uint32_t sampleBase, const uint64_t *d_frameKey, double *d_sub,
                                                     int32_t *d_assign, const int64_t *d_asgOff, double *d_logProb,
                                                     const int64_t *d_lpOff, double *d_logPerm, int32_t *d_method, int32_t *d_nOpen,
                                                     int32_t *d_nFrontier, int32_t *d_maxCluster, void *stream);
/*
 * Exact getAssignmentProbs from quadrics against a map of any size, on ONE stream (kbest_quadric_map.hip; the usePerm branch of
 * getAssignmentProbs, assignment.cpp:38-74, from (mean, covariance) pairs).  The cost builder conditions while it builds: the raw
 * (nL + nM) x nM block is never written.  conditionCosts (:450-494) keeps a landmark row only if some column has
 * cost <= colMin[c] + 42, and colMin[c] <= gate, so of thousands of landmarks a few dozen remain.  Three passes recompute the
 * costs (bits of kbest_quadric_costs_f64) rather than store them: per-tile column minima, the kept rows (ballots and counts, a
 * prefix sum over the tile counts), the compact block.  No floating-point atomics, no workgroup waits for another, no host read,
 * synchronise or allocation; stream order between the launches is the only synchronisation.  A frame's outputs are a function of
 * the frame alone: not of the batch, the tile size, or the bounds of the launch.
 *
 * One map for the call: d_mapMean [nMap][3], d_mapCov [nMap][9] (row-major 3 x 3).  Frame b sees landmarks d_landOff[b] ..
 * d_landOff[b] + d_nL[b] - 1 of it -- the caller keeps these windows inside the map, the entry cannot know nMap -- and has
 * d_nM[b] measurements from d_measOff[b] in d_measMean / d_measCov.  Offsets are int64, counts int32.
 *   d_nKeep[b]:   the landmark rows conditionCosts keeps -- the TRUE count, also where it exceeds maxKeep.
 *   d_rowIdx:     [B][maxKeep] int32, frame-local landmark numbers, ascending: conditionCosts' rowIdx restricted to landmarks.
 *   d_ccost:      (may be NULL: the context's) frame b's (nKeep + nM) x nM column-major compact block at
 *                 b * (maxKeep + maxCol) * maxCol: the kept landmark rows in order, then ALL nM dummy rows, whether conditionCosts
 *                 keeps them or not; each entry x <= colMin[c] + 42 ? x - colMin[c] : +inf, colMin over all nL + nM raw rows.
 *   d_cprobs:     frame b's [nM][nKeep + 1] probabilities at b * maxCol * (maxKeep + 1).
 *   d_probs:      (may be NULL) the dense [nM][nL + 1] slice at d_probOff[b]: EVERY element written, probs[m][rowIdx[l]] =
 *                 cprobs[m][l], probs[m][nL] = cprobs[m][nKeep], every other element exactly 0.0.
 *   d_logPerm, d_method (required), d_nOpen, d_nFrontier, d_maxCluster: what kbest_hybrid_frontier_probs_batch_f64_dev writes, which
 *                 the entry calls on the compact blocks with condition = 0, maxRawRow = maxKeep + maxCol, on the same stream -- the
 *                 bits of condition = 1 on the raw block, where that can be formed (the clustered kernel leaves all-zero rows out
 *                 after the gate, x - colMin is the subtraction it does itself, the block minimum is 0 either way).
 * Per-frame outcomes.  nKeep > maxKeep: method -1, d_nKeep[b] the true count (reserve again and call again), nothing of the frame
 * written beyond its slices, its dense slice zeros.  nM < 1, nM > maxCol, nL < 0, nL > maxMap or a negative offset: method -1,
 * and as for every frame that entry refuses nOpen and nFrontier 0, logPerm NaN; nKeep, rowIdx, maxCluster and every slice of the
 * frame are not touched.  nL = 0 is no special case: every measurement gets 1.0 in slot 0.
 * Limits: 1 <= maxCol <= 128, maxKeep >= 1, maxKeep + maxCol <= 1 024, 1 <= maxMap <= KBEST_QUADRIC_MAP_MAX, maxExact 0 .. 16
 * (0 = 16), maxWidth 1 .. 16, gate not NaN -- else KBEST_ERR_BAD_ARG.  KBEST_QUADRIC_MAP_MAX is 2^22 landmarks a frame: row numbers
 * are int32, every index into the map and the buffers is 64-bit, and the workgroup number b * ceil(maxMap / 256) + tile of a pass is
 * an int32, which with 2^22 leaves room for 2^17 frames a call (more: KBEST_ERR_BAD_ARG).
 * kbest_reserve_quadric_map_dev(ctx, B, maxMap, maxKeep, maxCol) sizes the tile minima, ballots, counts and offsets, the compact
 * blocks, the d_sub work buffer of the hybrid entry, and calls kbest_reserve_hybrid_dev(B, maxKeep + maxCol, maxCol).  A
 * reservation never shrinks: it holds the largest of each of the four numbers so far.  Without it, or with a call beyond it in any
 * of the four: KBEST_ERR_NOT_RESERVED, nothing launched.  B = 0: KBEST_OK, nothing launched.  Asynchronous on `stream` (NULL: the
 * context's); two calls on one stream need no synchronise between them.
 */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
#define KBEST_QUADRIC_MAP_MAX (1 << 22)
#define KBEST_QUADRIC_MAP_TILE 256 /* landmark rows per workgroup of the passes over the map (for tests of the tile edges) */
int kbest_reserve_quadric_map_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol);
int kbest_quadric_map_probs_batch_f64_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol, const double *d_mapMean,
                                          const double *d_mapCov, const int64_t *d_landOff, const int32_t *d_nL,
                                          const double *d_measMean, const double *d_measCov, const int64_t *d_measOff,
                                          const int32_t *d_nM, double gate, int maxExact, int maxWidth, int32_t *d_nKeep,
                                          int32_t *d_rowIdx, double *d_ccost, double *d_cprobs, double *d_probs,
                                          const int64_t *d_probOff, double *d_logPerm, int32_t *d_method, int32_t *d_nOpen,
                                          int32_t *d_nFrontier, int32_t *d_maxCluster, void *stream);
/*
 * The same from host buffers, synchronous, with the tiers the one-stream path lacks.  The map (mapMean [nMap][3], mapCov [nMap][9])
 * is staged once; frame b sees landmarks landOff[b] .. + nL[b] of it (inside the map, else KBEST_ERR_BAD_ARG) and has nM[b]
 * measurements, packed frame after frame in measMean / measCov.  The gate passes run first, nKeep is read back and the rest is
 * sized from it.  A frame the one-stream path refuses (an open cluster the frontier tier does not take) goes on, when maxBig > 0
 * or k >= 1, as its compact block -- one device-to-host copy -- through kbest_hybrid_frontier_probs_batch_f64(k, maxBig,
 * condition = 0), so k >= 1 answers every gated frame and method 1 / 2 says so.  probs: the dense [nM][nL + 1] slices at
 * probOff[b], zeros where nothing is assigned; logPerm, nOpen, nBig, nFrontier, maxCluster (each may be NULL), method and nKeep
 * (required) as that entry's.  More than 1 024 - nM kept landmarks: method -1 for that frame (zeros, logPerm NaN, nKeep the true
 * count), the call succeeds.  k >= 0, maxExact 0 .. 16, maxBig 0 .. 20, maxWidth 1 .. 16; nM > 128 or nL > KBEST_QUADRIC_MAP_MAX:
 * KBEST_ERR_UNSUPPORTED.
 */
int kbest_quadric_map_probs_batch_f64(kbest_ctx *ctx, int B, int nMap, const double *mapMean, const double *mapCov, const int64_t *landOff,
                                      const int32_t *nL, const int32_t *nM, const double *measMean, const double *measCov, double gate,
                                      int k, int maxExact, int maxBig, int maxWidth, double *probs, const int64_t *probOff,
                                      double *logPerm, int32_t *method, int32_t *nKeep, int32_t *nOpen, int32_t *nBig,
                                      int32_t *nFrontier, int32_t *maxCluster);
/* Diagnostic: registers, scratch bytes and static LDS bytes of the passes that compute costs (which = 0: minima, 1: kept rows,
 * 2: compact block), for tools/bench_quadric_map.py. */
int kbest_quadric_map_kernel_usage(int which, int32_t *vgprs, int32_t *scratchBytes, int32_t *ldsBytes);
/*
 * Joint associations from quadrics against a map of any size, on ONE stream (kbest_quadric_map_sample.hip; not in the reference):
 * the drawing twin of kbest_quadric_map_probs_batch_f64_dev.  Four steps on the stream: the gate passes and the fill of
 * kbest_quadric_map.hip (nKeep, rowIdx, the compact conditioned blocks -- the raw block is never written),
 * kbest_hybrid_frontier_sample_assoc_batch_f64_dev on the compact blocks (condition = 0, maxRawRow = maxKeep + maxCol, nL = the
 * kept rows, the context's d_sub, the caller's d_assign, d_logProb and offsets), and one kernel that rewrites d_assign in place
 * from compact rows to the rows of the notional raw (nL + nM) x nM block, which is what every other sampling entry returns (a miss
 * is not folded into nL): v < 0 stays -1; v < nKeep becomes rowIdx[b][v]; otherwise v becomes nL + (v - nKeep), the miss row of
 * measurement v - nKeep.  No host read, no synchronise, no allocation, no atomics, no workgroup waits for another; stream order
 * between the launches is the only synchronisation.
 *
 * kbest_quadric_map_sample_assoc_batch_f64_dev: the map, frames, gate, d_nKeep, d_rowIdx and d_ccost (may be NULL: the context's) as
 * in kbest_quadric_map_probs_batch_f64_dev; maxExact, maxWidth, nSample, seed, sampleBase, d_frameKey (may be NULL: frame b has key
 * b), d_assign, d_asgOff, d_logProb, d_lpOff, d_logPerm, d_method (required), d_nOpen, d_nFrontier and d_maxCluster (each may be
 * NULL) as in kbest_hybrid_frontier_sample_assoc_batch_f64_dev.
 *   nKeep, rowIdx, ccost, logPerm, method, nOpen, nFrontier, maxCluster: the bits of kbest_quadric_map_probs_batch_f64_dev on the
 *       same frames.
 *   assign, logProb: those of kbest_hybrid_frontier_sample_assoc_batch_f64_dev on the compact block with condition = 0, assign
 *       mapped as above.  A frame's draws are a function of (frame, seed, frame key, draw index) alone.  On a frame without an
 *       open cluster they are, bit for bit, the draws of the older path -- kbest_quadric_costs_f64, then that entry with
 *       condition = 1 on the raw block: the uniforms are indexed by active rows, and conditioning does not renumber those.
 *   NOTE: on a frame with a frontier cluster they are exact draws from the same posterior but NOT the same draws as on the raw
 *       block: the frontier sampler's key is the row number of the block it is given (the NOTE at
 *       kbest_hybrid_frontier_sample_assoc_batch_f64), and that is a compact row here.
 * Per-frame outcomes.  nKeep > maxKeep: method -1, d_nKeep[b] the true count (reserve again and call again), every assign -1,
 * every logProb NaN, rowIdx and the compact block not written.  nM < 1, nM > maxCol, nL < 0, nL > maxMap or a negative offset:
 * method -1, nOpen and nFrontier 0, logPerm NaN; nKeep, rowIdx, maxCluster, assign and logProb of the frame are not touched.
 * nL = 0 is no special case: assign[s][c] = c, the miss row of measurement c.
 * Limits: those of kbest_quadric_map_probs_batch_f64_dev, but maxWidth 0 .. 16, where 0 refuses every frame with an open cluster, as
 * the sampler defines it; nSample >= 1; sampleBase + nSample <= 2^32 -- else KBEST_ERR_BAD_ARG.
 * kbest_reserve_quadric_map_sample_dev(ctx, B, maxMap, maxKeep, maxCol, nSample) calls kbest_reserve_quadric_map_dev(B, maxMap,
 * maxKeep, maxCol) and kbest_reserve_hybrid_sample_dev(B, min(maxKeep + maxCol, 1 024), maxCol, nSample), the latter with the
 * largest of each number so far.  A reservation never shrinks.  Without it, or with a call beyond it in any of the five numbers:
 * KBEST_ERR_NOT_RESERVED, nothing launched.  B = 0: KBEST_OK, nothing launched.  Asynchronous on `stream` (NULL: the context's);
 * two calls on one stream need no synchronise between them.
 */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_quadric_map_sample_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol, int nSample);
int kbest_quadric_map_sample_assoc_batch_f64_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol, const double *d_mapMean,
                                                 const double *d_mapCov, const int64_t *d_landOff, const int32_t *d_nL,
                                                 const double *d_measMean, const double *d_measCov, const int64_t *d_measOff,
                                                 const int32_t *d_nM, double gate, int maxExact, int maxWidth, int nSample, uint64_t seed,
                                                 uint32_t sampleBase, const uint64_t *d_frameKey, int32_t *d_nKeep, int32_t *d_rowIdx,
                                                 double *d_ccost, int32_t *d_assign, const int64_t *d_asgOff, double *d_logProb,
                                                 const int64_t *d_lpOff, double *d_logPerm, int32_t *d_method, int32_t *d_nOpen,
                                                 int32_t *d_nFrontier, int32_t *d_maxCluster, void *stream);
/*
 * The same from host buffers, synchronous, shaped like kbest_quadric_map_probs_batch_f64 and sharing its staging, gate and round
 * plumbing: the map staged once, the gate passes, nKeep read back, the rest sized from it, rounds where maxKeep + maxCol would
 * exceed 1 024.  assign at asgOff[b]: int32 [nSample][nM], raw rows as above; logProb at lpOff[b]: double [nSample]; frameKey (may
 * be NULL: frame b has key b).  k = 0: the bits of the one-stream entry.  k >= 1 (up to KBEST_TABLE_SAMPLE_MAX_K): a frame that
 * entry refuses because of an open cluster goes on, as its compact block -- one device-to-host copy --, through
 * kbest_hybrid_sample_assoc_batch_f64(condition = 0, k) with the frame's own key and the same sampleBase, and its rows are mapped on
 * the host; so k >= 1 draws every gated frame, and method 1 / 2 and nEnum say which frames were enumerated.  logPerm, nOpen,
 * nFrontier, nEnum, maxCluster (each may be NULL), method and nKeep (required) as that entry's.  More than 1 024 - nM kept
 * landmarks: method -1 for that frame (every assign -1, every logProb NaN, logPerm NaN, nKeep the true count), the call succeeds.
 * nM > 128 or nL > KBEST_QUADRIC_MAP_MAX: KBEST_ERR_UNSUPPORTED.
 */
int kbest_quadric_map_sample_assoc_batch_f64(kbest_ctx *ctx, int B, int nMap, const double *mapMean, const double *mapCov,
                                             const int64_t *landOff, const int32_t *nL, const int32_t *nM, const double *measMean,
                                             const double *measCov, double gate, int k, int maxExact, int maxWidth, int nSample,
                                             uint64_t seed, uint32_t sampleBase, const uint64_t *frameKey, int32_t *assign,
                                             const int64_t *asgOff, double *logProb, const int64_t *lpOff, double *logPerm,
                                             int32_t *method, int32_t *nKeep, int32_t *nOpen, int32_t *nFrontier, int32_t *nEnum,
                                             int32_t *maxCluster);
/* Diagnostic: registers, scratch bytes and static LDS bytes of the kernel that maps compact rows to raw rows, for
 * tools/bench_quadric_map_sample.py. */
int kbest_quadric_map_sample_kernel_usage(int32_t *vgprs, int32_t *scratchBytes, int32_t *ldsBytes);
/*
 * Factor lists from association probabilities, on the stream (kbest_factors.hip): what the reference's consumer loop makes of a
 * frame's probabilities (system.cpp:279-346; the window keeps per landmark whether a frame still constrains it,
 * slidingWindow.cpp:351-460), as a stream compaction on the device instead of a copy of the dense slice and a scan on the host.
 *
 *   for m, for q < nL:  if (probs[m][q] < NEW_FACTOR_PROB_THRESH) continue;   two factors, noise BOX_SD / probs[m][q]
 *   for m:              if (probs[m][nL] > NEW_LANDMARK_THRESH)               a new landmark, noise BOX_SD / probs[m][nL]
 *   (constsUtils.h:57-59 for the noise, :75-78 for the defaults BOX_SD 3, NEW_LANDMARK_THRESH 0.33, NEW_FACTOR_PROB_THRESH 0.05)
 *
 * kbest_assoc_factors_f64_dev takes the output of ANY probability entry.  Frame b has probabilities row-major
 * [d_nM[b]][d_nSlot[b] + 1] at d_probOff[b] in d_probs.  Slot nSlot is the miss / new-landmark column; slot l < nSlot is the
 * landmark d_rowIdx[b * rowStride + l] (compact form: d_cprobs, d_rowIdx and d_nKeep of the quadric-map entries) or, with
 * d_rowIdx NULL, the landmark l (dense form, nSlot = nL).  The map index of a landmark is d_landOff[b] + landmark (d_landOff NULL: 0).
 *   Factor list:  every (b, m, l) with !(p < factorThresh), in the order b ascending, then m ascending, then l ascending.  rowIdx is
 *                 ascending, so this is the reference's q order, and the compact and the dense form of a frame give the same list.
 *                 A struct of arrays: d_fFrame, d_fMeas, d_fLand (int32, the frame-local landmark), d_fMap (int64, may be NULL),
 *                 d_fProb (the bits of p), d_fSigma = boxSd / p (one IEEE division: the bits of C's BOX_SD / prob; +inf for p = 0).
 *   New-landmark list:  every (b, m) with P_b[m][nSlot] > newThresh, strictly, in the order b, then m: d_nFrame, d_nMeas, d_nProb,
 *                 d_nSigma.  The two comparisons are the reference's: p equal to factorThresh is kept, p equal to newThresh is not new.
 *   Counts:       d_nFactor[b], d_nNew[b] (int32) the TRUE counts; d_factorOff[b], d_newOff[b] (int64) the exclusive prefix sums of
 *                 the true counts; d_total[2] (int64) the true totals.
 *   Capacity:     an entry whose position is >= maxFactor (>= maxNew) is not written, and nothing else changes: the caller sees
 *                 total > capacity and calls again.  Capacity 0 with NULL arrays is a legal counting call.
 *   Support:      d_support[nSupport] (int32, may be NULL) is zeroed on the stream, then 1 is added per factor at its map index;
 *                 indices outside [0, nSupport) are not counted.  The value does not depend on the capacities.
 *   Frames that emit nothing (counts 0):  d_method given and d_method[b] < 0; nM < 1, nM > maxCol, nSlot < 0, nSlot > maxSlot, a
 *                 negative offset.  A refused frame's slice was never written, and a NaN would pass !(p < t).
 * The position of every entry is computed (a count pass, an integer prefix pass, an emit pass that recomputes the predicates), so a
 * frame's entries are the same alone and in any batch; only fFrame and the offsets differ.  No floating-point atomics (the support
 * is an integer sum, which does not depend on the order), no workgroup waits for another, no host read, synchronise or allocation;
 * every index into a buffer is 64-bit.
 * Limits: B >= 0, 1 <= maxCol <= 128, 0 <= maxSlot <= KBEST_QUADRIC_MAP_MAX, B * maxCol < 2^31, thresholds and boxSd not NaN,
 * capacities and nSupport >= 0, rowStride >= maxSlot where d_rowIdx is given -- else KBEST_ERR_BAD_ARG.
 * kbest_reserve_assoc_factors_dev(ctx, B, maxCol) reserves the per-(frame, measurement) counts and scan partials (all integer); it
 * never shrinks.  A call beyond it: KBEST_ERR_NOT_RESERVED, nothing launched.  B = 0: KBEST_OK, the totals 0 and the support
 * zeroed.  Asynchronous on `stream` (NULL: the context's); two calls on one stream need no synchronise between them.
 */
/* (a work space a captured launch holds does not grow: "WORK SPACES UNDER A CAPTURED LAUNCH" at kbest_reserve) */
int kbest_reserve_assoc_factors_dev(kbest_ctx *ctx, int B, int maxCol);
int kbest_assoc_factors_f64_dev(kbest_ctx *ctx, int B, int maxSlot, int maxCol, const double *d_probs, const int64_t *d_probOff,
                                const int32_t *d_nSlot, const int32_t *d_nM, const int32_t *d_rowIdx, int64_t rowStride,
                                const int64_t *d_landOff, const int32_t *d_method, double factorThresh, double newThresh, double boxSd,
                                int64_t maxFactor, int32_t *d_fFrame, int32_t *d_fMeas, int32_t *d_fLand, int64_t *d_fMap,
                                double *d_fProb, double *d_fSigma, int64_t maxNew, int32_t *d_nFrame, int32_t *d_nMeas, double *d_nProb,
                                double *d_nSigma, int32_t *d_nFactor, int64_t *d_factorOff, int32_t *d_nNew, int64_t *d_newOff,
                                int64_t *d_total, int32_t *d_support, int64_t nSupport, void *stream);
/*
 * The same fused behind kbest_quadric_map_probs_batch_f64_dev, on one stream: the arguments of that entry (its body is unchanged,
 * d_probs may be NULL, every output has its bits), then the factor arguments.  The factor passes run in compact form on d_cprobs,
 * d_rowIdx and d_nKeep with d_method, maxSlot = maxKeep, and d_landOff gives the map index.  A frame with nKeep > maxKeep or
 * method -1 emits nothing.  kbest_reserve_quadric_map_factors_dev calls kbest_reserve_quadric_map_dev and
 * kbest_reserve_assoc_factors_dev; without either, KBEST_ERR_NOT_RESERVED and nothing is launched.
 */
int kbest_reserve_quadric_map_factors_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol);
int kbest_quadric_map_factors_batch_f64_dev(kbest_ctx *ctx, int B, int maxMap, int maxKeep, int maxCol, const double *d_mapMean,
                                            const double *d_mapCov, const int64_t *d_landOff, const int32_t *d_nL,
                                            const double *d_measMean, const double *d_measCov, const int64_t *d_measOff,
                                            const int32_t *d_nM, double gate, int maxExact, int maxWidth, int32_t *d_nKeep,
                                            int32_t *d_rowIdx, double *d_ccost, double *d_cprobs, double *d_probs,
                                            const int64_t *d_probOff, double *d_logPerm, int32_t *d_method, int32_t *d_nOpen,
                                            int32_t *d_nFrontier, int32_t *d_maxCluster, double factorThresh, double newThresh,
                                            double boxSd, int64_t maxFactor, int32_t *d_fFrame, int32_t *d_fMeas, int32_t *d_fLand,
                                            int64_t *d_fMap, double *d_fProb, double *d_fSigma, int64_t maxNew, int32_t *d_nFrame,
                                            int32_t *d_nMeas, double *d_nProb, double *d_nSigma, int32_t *d_nFactor,
                                            int64_t *d_factorOff, int32_t *d_nNew, int64_t *d_newOff, int64_t *d_total,
                                            int32_t *d_support, int64_t nSupport, void *stream);
/*
 * The same from host buffers, synchronous: the dense [nM][nL + 1] slices at probOff[b] that every host probability entry returns
 * (landOff and method may be NULL) are staged, the device entry runs in dense form, and the lists -- their first
 * min(total, capacity) entries -- the counts, offsets and support are copied back.  total[2] holds the true totals.  A frame with
 * nM < 1, nL < 0, a negative offset or method < 0 emits nothing; nM > 128 or nL > KBEST_QUADRIC_MAP_MAX: KBEST_ERR_UNSUPPORTED.
 */
int kbest_assoc_factors_batch_f64(kbest_ctx *ctx, int B, const double *probs, const int64_t *probOff, const int32_t *nL,
                                  const int32_t *nM, const int64_t *landOff, const int32_t *method, double factorThresh,
                                  double newThresh, double boxSd, int64_t maxFactor, int32_t *fFrame, int32_t *fMeas, int32_t *fLand,
                                  int64_t *fMap, double *fProb, double *fSigma, int64_t maxNew, int32_t *nFrame, int32_t *nMeas,
                                  double *nProb, double *nSigma, int32_t *nFactor, int64_t *factorOff, int32_t *nNew, int64_t *newOff,
                                  int64_t *total, int32_t *support, int64_t nSupport);
/* Diagnostic: registers, scratch bytes and static LDS bytes of the factor passes (which = 0: count, 1: scan inside a frame, 2: scan
 * over the frames, 3: emit), for tools/bench_factors.py. */
int kbest_factors_kernel_usage(int which, int32_t *vgprs, int32_t *scratchBytes, int32_t *ldsBytes);
/* on = 1: the HOST-buffer association entries of this context (kbest_weights / assoc_probs / bruteforce / quadric_assoc) enumerate
 * their k best in the REFERENCE's own order of operations (the reference-order kernel, as KBEST_FLAG_REFERENCE_ORDER does for
 * kbest_batch_f64): where exactly equal gains straddle slot k the assignments that are weighed are the ones the reference's
 * kBest2DCutoff returns (assignment.cpp:594), so the probabilities are the reference's there too (integer-like costs).  Slower: no
 * fused kernels.  The reference-named shims switch it on with KBEST_SHIM_REFERENCE_ORDER=1.
 * on = 2: the same answer at the fused kernels' speed wherever nothing ties (as KBEST_FLAG_REFERENCE_TIES does for kbest_batch_f64):
 * the batch runs on the fused kernels, and only the frames whose k-th and (k+1)-th gains are exactly equal -- the only frames whose
 * weights depend on the order of ties: inside a run of equal gains every order sums the same terms -- are enumerated again by the
 * reference-order kernel and weighed from its table (KBEST_TIE_REFERENCE in kbest_last_tie_flags).  KBEST_SHIM_REFERENCE_ORDER=2.
 * on = 0: the engine's own rule (the default). */
int kbest_set_reference_order(kbest_ctx *ctx, int on);
/* Where kbest_assoc_probs_batch_f64_dev writes its frames' KBEST_TIE_* flags ([B] int32 in device memory; NULL, the default:
 * nowhere).  Stays set until changed. */
int kbest_set_assoc_tie_flags_dev(kbest_ctx *ctx, int32_t *d_flags);
/* KBEST_TIE_* flags of the problems of the context's last SYNCHRONOUS call (kbest_batch_f64 and every host-buffer association
 * entry, which have no other way to return them: the shims of kbest_shims.hpp included).  Copies min(n, cap) flags, returns n. */
int kbest_last_tie_flags(kbest_ctx *ctx, int32_t *flags, int cap);
/* Diagnostic: launches of the 64-row kernel this context has made as a relay (several workgroups per matrix in turn; the
 * comment of kbest_reserve, NOTES.md 10.6) since it was created -- for tests that must know the path they exercise was taken. */
long long kbest_relay_launches(kbest_ctx *ctx);  /* (-1: null context) */
/* Diagnostic: the kernel(s) the context's last k-best launch (kbest_batch_f64[_dev] and whatever goes through them) was routed
 * to -- KBEST_ROUTE_* bits -- for tests that must know the path they exercise was taken.  -1: null context. */
#define KBEST_ROUTE_LANE 1    /* the lane-per-child kernel: <= 32 rows, dense batches                   */
#define KBEST_ROUTE_SMALL 2   /* the small-problem kernel: <= 32 rows, rectangular / chip-underfilling  */
#define KBEST_ROUTE_FAST 4    /* the 64-row kernel                                                      */
#define KBEST_ROUTE_WIDE 8    /* the general-size kernel: any size, any k                               */
#define KBEST_ROUTE_RELAY 16  /* ... as a relay of several workgroups per matrix                        */
#define KBEST_ROUTE_EXACT 64  /* the reference-order kernel (KBEST_FLAG_REFERENCE_ORDER; > 1 024 rows)   */
#define KBEST_ROUTE_SPLIT 128 /* the 64-row kernel with several workgroups per matrix and the merge      */
#define KBEST_ROUTE_EXTRA 32  /* the launch enumerated the solution behind the k-th (exact ties checked) */
int kbest_last_route(kbest_ctx *ctx);

/*
 * Batched computeQuadricCostMatrix (assignment.h:28-29, assignment.cpp:705-722).  Frame b has nL[b] landmarks and
 * nM[b] measurements, each a (mean[3], cov[3][3] row-major) pair, packed frame after frame; gate is
 * NONASSIGN_QUADRIC.  cost receives the (nL+nM) x nM column-major blocks packed back to back.  Host buffers.
 */
int kbest_quadric_costs_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM, const double *landMean,
                            const double *landCov, const double *measMean, const double *measCov, double gate,
                            double *cost);

/*
 * getAssignmentProbs from the (mean, covariance) pairs on (assignment.cpp:42-74 after getMeans/getCovs): cost
 * construction, conditionCosts, assignmentProb(k), scatter back -- one stream-ordered device pipeline, the cost
 * matrix never visits the host.  probs: [nM][nL+1] per frame at probOff[b].
 */
int kbest_quadric_assoc_probs_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nM,
                                        const double *landMean, const double *landCov, const double *measMean,
                                        const double *measCov, double gate, int k, double *probs,
                                        const int64_t *probOff, int32_t *nf);

/*
 * Batched computeBBCostMatrix (assignment.cpp:777-797), the cost-only counterpart of kbest_quadric_costs_f64: boxes and
 * gate as kbest_bb_match_batch_f64 takes them; cost receives the (nR+nL) x nL column-major profit blocks -- min of the two
 * asymmetric IoUs (boundBox.h:62-75), -inf fill, the gate on each left box's own dummy row -- packed back to back.  Runs no
 * solver.  Host buffers.
 */
int kbest_bb_costs_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nR, const double *boxL, const double *boxR,
                       double gate, double *cost);

/*
 * Batched asgnBB (assignment.h:21, assignment.cpp:724-797): stereo bounding-box matching.  Boxes are
 * (xmin, ymin, xmax, ymax, xOffset) -- boundBox.h:13-25 -- nL[b] left and nR[b] right boxes per frame, packed;
 * gate is NONASSIGN_BOUNDBOX.  assign[sum nL]: for every left box the index of its right box, or -1.
 * Synchronous, so on exact ties it answers as the reference does ("Order of exact ties" (1)): a frame whose optimum is
 * attained by more than one matching (duplicate detections, containment, an IoU equal to the gate) is solved again by the
 * reference-order kernel; frames without a tie stay on the fast kernels.
 */
int kbest_bb_match_batch_f64(kbest_ctx *ctx, int B, const int32_t *nL, const int32_t *nR, const double *boxL,
                             const double *boxR, double gate, int32_t *assign);

/*
 * Pin [ptr, ptr + bytes) of caller-owned host memory and map it into the device's address space (hipHostRegister), for the
 * host-buffer entries above.  The range must stay allocated until kbest_unregister_host_buffer (or kbest_destroy).  Any number
 * of ranges; a buffer argument is taken as registered when it lies completely inside one of them.  Honoured by
 * kbest_batch_f64 (cost, row4col, col4row, gain, nf) and by the association entries (cost, probs).
 */
int kbest_register_host_buffer(kbest_ctx *ctx, void *ptr, size_t bytes);
int kbest_unregister_host_buffer(kbest_ctx *ctx, void *ptr);

/*
 * The "global k-best heap" of the subtree-sharded enumeration (reference partition: split,
 * shortestPathCPP.cpp:455-532): shard s of nShard enumerated the root's children on columns c % nShard == s
 * (kbest_opts.root_col_offset / root_col_stride) and holds its own k best -- slot 0 is the root on every shard.  This
 * k-way merge on the device gives the global table: the root, then the k - 1 best of the union of the shards' slots 1..
 * in increasing cost (decreasing profit when `maximize`); exact ties are ordered by the assignment (lexicographic
 * row4col), so the result does not depend on the number of shards.  d_gain / d_row4col / d_nf point at shard 0's
 * [B][k] fp64 / [B][k][maxCol] i32 / [B] i32 tables, shard s's tables start s * shardStrideBytes behind them (the
 * packed per-rank slices of the all-gather, or plain [nShard][B][...] arrays).  Asynchronous on `stream`
 * (NULL = the context's stream); device pointers.
 */
int kbest_merge_topk_f64_dev(kbest_ctx *ctx, int B, int nShard, int k, int maxCol, int maximize, const void *d_gain,
                             const void *d_row4col, const void *d_nf, int64_t shardStrideBytes, double *d_outGain,
                             int32_t *d_outRow4col, int32_t *d_outNf, void *stream);
/* The same with the shards' row4col tables as int8 ([B][k][maxCol] bytes: what KBEST_FLAG_TABLES_I8 launches write and what the
 * exchange of problems of up to 127 rows moves); the merged table is int32. */
int kbest_merge_topk_i8_f64_dev(kbest_ctx *ctx, int B, int nShard, int k, int maxCol, int maximize, const void *d_gain,
                                const void *d_row4col8, const void *d_nf, int64_t shardStrideBytes, double *d_outGain,
                                int32_t *d_outRow4col, int32_t *d_outNf, void *stream);
/*
 * The global k-best heap from the shards' COSTS alone (the north star's "allgather of per-rank top-k costs into a global k-best
 * heap"): d_gain [nShard][B][k] fp64 and d_nf [nShard][B] i32 are what an all-gather of every rank's (gain, nf) leaves on every
 * rank -- 8 k + 4 bytes per matrix and shard --; d_ownRow4col8 [B][k][maxCol] int8 are the rows of THIS rank's shard `ownShard`
 * (a KBEST_FLAG_TABLES_I8 launch with root_col_offset / stride).  Writes the merged gains d_outGain [B][k] and counts d_outNf [B]
 * in full (identical on every rank), and into d_outRow4col8 [B][k][maxCol] -- which the caller has ZEROED -- the rows of this
 * rank's own winners at their merged positions: ONE sum all-reduce of that byte table over the ranks (k maxCol bytes per matrix,
 * whatever the number of ranks; every entry is non-zero on at most one rank) completes it everywhere; slots beyond d_outNf stay 0.
 * *d_tied (one int32, zeroed by the caller) is set when two candidates of some matrix have EXACTLY the same gain within the k best
 * or at slot k: their order is the assignments' ("Order of exact ties" above), which this merge does not see -- the caller then
 * exchanges the whole lists and merges with kbest_merge_topk_i8_f64_dev.  numRow <= 127.  Asynchronous on `stream`.
 */
int kbest_merge_gains_f64_dev(kbest_ctx *ctx, int B, int nShard, int k, int maxCol, int maximize, const double *d_gain,
                              const int32_t *d_nf, int ownShard, const int8_t *d_ownRow4col8, double *d_outGain,
                              int8_t *d_outRow4col8, int32_t *d_outNf, int32_t *d_tied, void *stream);

/*
 * Multi-device entries (BASELINE.json config 4): one engine context + one stream per GPU and an
 * RCCL communicator over them (ncclCommInitAll; xGMI inside a node).  kbest_batch_f64_multi shards the batch in
 * contiguous blocks (device g solves matrices [g*ceil(B/G), ...)), each device solving its block with the kernels of
 * the single-device entries straight into its packed slice (gain | row4col | nf) of a global table; ONE in-place
 * ncclAllGather of those slices then leaves EVERY device with the same global k-best table (there is no
 * other collective: the matrices are independent).  Between the devices row4col travels as int8 wherever every index fits a
 * byte (numRow <= 127: 8 + numCol instead of 8 + 4 numCol bytes per solution); the caller's tables are int32 as ever.  Every device is fed and read back by a host thread of its own: the
 * host outputs of a block come from the device that solved it (col4row is not part of the exchange).  device_ids may
 * name one GPU several times ("logical devices", e.g. {0, 0, 0, 0}): the slices then travel by device-to-device copies
 * instead of RCCL -- the same host path, testable on one GPU.  Same argument meaning as kbest_batch_f64
 * (uniform packing b*maxRow*maxCol; nRow/nCol optional).  Exact ties: every device's tables come back in the one order of
 * equal gains ("Order of exact ties" above); a gain level that straddles slot k is NOT completed by these entries (their tables
 * stay on the devices for the exchange) and no flags are returned: a caller with integer-like costs that needs the canonical
 * members of such a level runs kbest_batch_f64 on the problems kbest_batch_f64_dev / kbest_batch_f64 flag.
 * RCCL is bound at run time (dlopen): without it
 * kbest_create_multi returns KBEST_ERR_NO_DEVICE and every single-device entry still works.
 */
typedef struct kbest_multi kbest_multi;
int kbest_create_multi(kbest_multi **m, const int *device_ids, int nDev);
int kbest_destroy_multi(kbest_multi *m);
int kbest_multi_size(const kbest_multi *m);
const char *kbest_multi_last_error(const kbest_multi *m);
int kbest_batch_f64_multi(kbest_multi *m, const kbest_opts *opts, int B, int maxRow, int maxCol, const int32_t *nRow,
                          const int32_t *nCol, const double *cost, int k, int32_t *row4col, int32_t *col4row, double *gain,
                          int32_t *nf);
/*
 * The same with the sharding mode explicit.  KBEST_MULTI_BATCH: as above.  KBEST_MULTI_SUBTREE (few large matrices; the
 * north star's "per-rank top-k into a global k-best heap"): every device receives ALL B matrices; shard s of nShard
 * (0 = one per device; more than devices: dealt round robin, a device runs its shards one after the other) expands only
 * the root's children on columns c % nShard == s (reference partition: split, shortestPathCPP.cpp:455-532) and enumerates
 * its own k best.  The exchange is gains first (numRow <= 127): ONE all-gather of every shard's top-k COSTS (gain[k] + nf), the merge
 * into the global k-best heap on every device (kbest_merge_gains_f64_dev), and ONE sum all-reduce of the byte table that holds every
 * winner's row at its merged position -- 8 k S + k numCol bytes per matrix instead of (8 + 4 numCol) k S.  A call in which two
 * candidates have exactly the same gain (integer-like costs: their order is the assignments'), and problems of more than 127 rows,
 * all-gather the whole per-shard lists and merge those (kbest_merge_topk[_i8]_f64_dev).  Results are those of the batch mode for
 * tie-free costs (exact ties: ordered by the assignment); col4row, which is not part of the exchange, is returned as the inverse of
 * row4col with -1 for rows without a real column.  opts->root_col_offset / stride must be unset.
 */
#define KBEST_MULTI_BATCH 0
#define KBEST_MULTI_SUBTREE 1
int kbest_batch_f64_multi_ex(kbest_multi *m, const kbest_opts *opts, int mode, int nShard, int B, int maxRow, int maxCol,
                             const int32_t *nRow, const int32_t *nCol, const double *cost, int k, int32_t *row4col,
                             int32_t *col4row, double *gain, int32_t *nf);
/* 1 when every device holds the same global table after the last kbest_batch_f64_multi[_ex] call, 0 when not (test aid). */
int kbest_multi_tables_agree(kbest_multi *m);
/* Bytes that ARRIVE at one device in the exchanges of the last kbest_batch_f64_multi[_ex] call: an all-gather of b bytes per device
 * brings (G - 1) b, the ring all-reduce of the n-byte table of subtree mode 2 n (G - 1) / G; *path (optional): 0 batch mode,
 * 1 subtree mode gains first, 2 subtree mode whole lists. */
long long kbest_multi_exchange_bytes(const kbest_multi *m, int *path);
/* KBEST_TIE_* flags of the problems of the last kbest_batch_f64_multi call (batch mode): copies min(n, cap) flags, returns n. */
int kbest_multi_last_tie_flags(kbest_multi *m, int32_t *flags, int cap);
/*
 * Host timeline of the last kbest_batch_f64_multi[_ex] call: out[g * KBEST_MULTI_STAMPS + i], seconds since the call was
 * entered, for device g: [0] its worker thread started, [1] its first upload was issued, [2] its first kernel was issued,
 * [3] it was fed (batch mode: its own results are back in the caller's tables as well), [4] the exchange was issued, [5] done.
 * Every device is fed and read back by a thread of its own, so no device waits for another one's copies; this is the
 * evidence.  Returns the number of devices written (at most capDevices).
 */
#define KBEST_MULTI_STAMPS 6
int kbest_multi_timeline(const kbest_multi *m, double *out, int capDevices);

#ifdef __cplusplus
}
#endif
#endif /* KBEST_C_H */

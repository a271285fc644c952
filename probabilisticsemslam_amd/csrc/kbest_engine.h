// kbest_engine.h -- internal interface between the C ABI (kbest_capi.cpp) and
// the device code (kbest_engine.hip).  Not installed; include/kbest_c.h is the
// public boundary.
#ifndef KBEST_ENGINE_H
#define KBEST_ENGINE_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kbest_c.h"

namespace kb {

typedef unsigned long long u64;
typedef unsigned int u32;

// Kernel arguments of one batched launch (all pointers are device pointers).
struct Params {
    const double *cost;       // packed column-major cost blocks
    const long long *costOff; // per-problem offset in doubles, or nullptr (uniform)
    const int *nRow;          // per-problem shapes, or nullptr (uniform maxRow x maxCol)
    const int *nCol;
    int maxRow, maxCol;       // capacity of this launch: larger problems get nf = -1
    int ldRow, ldCol;         // leading dimensions of the outputs / of the default cost packing (>= maxRow, maxCol)
    int k;
    int maximize, useCutoff;
    unsigned flags;
    double cutoff;
    int rootColOffset, rootColStride;
    int *row4col;             // [B][k][maxCol]
    int *col4row;             // [B][k][maxRow]
    double *gain;             // [B][k]
    int *nf;                  // [B]
    long long *pushed;        // [B] or nullptr
    unsigned char *states;    // workspace: [B][statesPerProblem] saved hypotheses, stateStride bytes each
    long long stateStride;
    int statesPerProblem;     // all state slots of one matrix: [0, lazyStates) + the eager region behind it
    int lazyStates;           // >= k: slots for the root and for candidates that are re-solved when selected
    int spec;                 // candidates re-solved / split per round (1 = the reference's order exactly)
    unsigned long long *prof; // [B][16] cycle stamps; only read by diagnostic builds (make PROFILE=1)
    unsigned short *slotSid;  // workspace: [B][slot_table_stride(k)] state slot of each output slot
    double *dualU;            // [B][ldCol] duals of the root solution per column (MurtyHyp::u), or nullptr
    double *dualV;            // [B][ldRow] ... per row (MurtyHyp::v), or nullptr
    int gainCols;             // numCol4Gain of shortestPathCPP (cpp:232); 0 = numCol
    int split, splitB;        // split > 1 (64-row kernel): `split` workgroups per matrix, splitB matrices; tables / work space per workgroup
    unsigned long long *sharedT;  // [splitB] smallest threshold any share of a matrix has published (ordered key; ~0 = none)
    // optimistic bounds (64-row kernel; kbest_engine.hip "optimistic bounds and tickets"): a node is split against the optRho-quantile
    // of the pool's candidates instead of its last one; optRho grows linearly from optRho0 to optRho1 while the first optPhi * k
    // solutions go out.  optRho0 >= 1: off.
    float optRho0, optRho1, optSlope;  // optSlope = (optRho1 - optRho0) / (optPhi * k), by the host: no loop-invariant float arithmetic in the kernel
    double optKappa;          // a ticket's re-split goes at least optKappa * (key - optimum) beyond its key
    int optMinPool;           // candidates the pool must hold before a quantile of it is used
    // exact ties (kbest_ties.h): the tables hold kTab slots per problem -- k, or k - 1: the k-th solution is then enumerated for its
    // gain only, which goes to tieGain[problem] (NaN: there is none)
    int kTab;
    double *tieGain;
    // relay (kbest_engine.hip): relayP > 1: every matrix is enumerated by relayP workgroups one after the other (grid = relayB x
    // relayP); relayBuf: [relayB] LDS images of relayStride bytes; three words per matrix, all zero between launches (the last of a
    // matrix' workgroups to leave clears them): relayClaim -- pieces claimed (a workgroup's piece is what it claims), relayFlag --
    // pieces done (15: the matrix is finished), relayGone -- workgroups that have left
    int relayP, relayB;
    int relayFirst, relayStep;  // piece j hands over once k * (relayFirst + j * relayStep) / 1024 solutions are out (the last piece runs to the end;
                                // the launch ends with a generation of LAST pieces: they should be short; scalar integer arithmetic only)
    unsigned char *relayBuf;
    long long relayStride;
    unsigned *relayFlag;
    unsigned *relayClaim, *relayGone;
    // 64-row kernel: the result tables are in HOST memory (registered or pinned staging, written over the link): the slots that
    // have become final are then written at the start of a round's children phase, so that the stores drain under the children;
    // tables in device memory (0) are written behind a wave's children, in the slack in front of the barrier after them
    int tablesHost;
};

struct CondParams {
    const double *cost;       // raw (nL+nM) x nM blocks
    const long long *costOff;
    const int *nRow, *nCol;
    double *out;              // conditioned blocks, same offsets (goodRows x nCol, column-major)
    int *goodRows;            // [B]
    int *condL;               // [B] goodRows - nCol (assignment.cpp:60), or nullptr
    int *rowIdx;              // [B][maxRow] original row of each kept row
    int maxRow;
};

struct WeightParams {
    const int *nL, *nM;
    const double *cost;
    const long long *costOff;
    const double *gain;       // [B][k]
    const int *row4col;       // [B][k][maxCol]
    int *nf;                  // [B] (nM == 1: set to the entries weighed)
    double *probs;
    const long long *probOff;
    int k, maxCol;
    const int *rowIdx;        // [B][maxRow] or nullptr: scatter back through conditionCosts' row map
    const int *nLout;         // [B] landmarks in the output numbering (with rowIdx)
    int maxRow;
    int gate;                 // 1: assignmentProb (skip solutions beyond best + 42, :622-626); 0: bruteForceProb (:918-923)
    int solveRows;            // rows of the largest solved problem (bounds nL + 1: sizes the LDS accumulator)
    int chunk, ldsAcc;        // set by launch_weights: solutions per LDS chunk; 1: the [nM][nL+1] table accumulates in LDS
    long long accBytes;
    int kUse;                 // > 0: only the first kUse solutions of a problem are weighed (its table holds k >= kUse slots)
};

// Dynamic LDS of weights_kernel (launch_weights sets chunk, ldsAcc and accBytes from it): weights and row maps of one chunk of
// solutions, and -- when it fits 96 KiB with them -- the [maxCol][solveRows] accumulator table
struct WeightsLds { int chunk, ldsAcc; long long accBytes; size_t total; };
inline WeightsLds weights_lds_plan(int maxCol, int solveRows)
{
    WeightsLds w;
    int chunk = 8192 / (maxCol > 0 ? maxCol : 1);
    chunk = chunk > 256 ? 256 : (chunk < 8 ? 8 : chunk);
    const size_t base = (size_t)chunk * 8 + (size_t)chunk * maxCol * 4;
    const size_t accWant = (size_t)maxCol * (size_t)(solveRows > 0 ? solveRows : 1) * 8;
    w.chunk = chunk;
    w.ldsAcc = (base + accWant <= 96 * 1024) ? 1 : 0;
    w.accBytes = w.ldsAcc ? (long long)accWant : 0;
    w.total = ((base + (w.ldsAcc ? accWant : 0)) + 15) & ~(size_t)15;
    return w;
}

// Bytes of one saved hypothesis: u[D] v[D] (fp64), row4col[D] col4row[D] (u8),
// forbidden-row mask, gain, activeCol.
__host__ __device__ inline long long state_stride(int maxRow)
{
    // u, v (fp64), row4col, col4row (u8), forbidden mask, gain, activeCol, columns whose child has been completed (u64: the
    // 64-row kernel's re-split tickets); rounded to whole 128-byte lines: neighbouring states never share a cache line
    return ((((long long)18 * maxRow + 7) & ~7LL) + 32 + 127) & ~127LL;
}

// u16 entries of one matrix's slot -> state table, rounded to whole 128-byte lines
__host__ __device__ inline long long slot_table_stride(int k) { return (((long long)k * 2 + 127) & ~127LL) / 2; }

// LDS carve-up of one workgroup (= one cost matrix).
constexpr int OPT_TICKETS = 64;   // re-split tickets a problem can hold (one wave sorts them)
constexpr int OPT_BYTES = 16 * 8 * 3 + 16 + 8 + OPT_TICKETS * 10 + 8;  // struct Opt (kbest_engine.hip)
struct Lds {
    int offC, offNodes, nodeStride, offFreshG, offFreshM, offPoolG, offPoolM, offPoolS, offSurv, offFreshS, offRootMap, offPerm, offCtrl, offOpt, offGainW, total;
};

__host__ __device__ inline Lds lds_layout(int maxRow, int k, int spec, int nWaves)
{
    Lds L;
    const int ldc = maxRow | 1;
    int o = 0;
    L.offC = o;          o += maxRow * ldc * 8;      // shifted, zero-padded cost tile
    L.nodeStride = (18 * maxRow + 24 + 7) & ~7;      // u, v (fp64), scalars, row4col, col4row (u8)
    L.offNodes = o;      o += spec * L.nodeStride;   // solved hypotheses waiting to be split
    L.offFreshG = o;     o += (spec * 64 > 16 ? spec * 64 : 16) * 8;  // surviving children of this round: gain
                                                     //   (also: the first-step minima during the filter phase)
    L.offPoolG = o;      o += k * 8;                 // sorted candidate pool: gain
    L.offFreshM = o;     o += spec * 64 * 4;         //   (parent state, column); during the filter: last-arc minima
    L.offPoolM = o;      o += k * 4;                 //   (parent state, column, flags)
    L.offPoolS = o;      o += k * 2;                 //   own state slot
    L.offSurv = o;       o += spec * 64 * 2;         // children that passed the filter: (last-arc bound / 7 bits, node, column)
    L.offFreshS = o;     o += spec * 64 * 2;         //   own state slot of the surviving children
    L.offRootMap = o;    o += maxRow;                // the optimum's col4row (u8): atoms of the a-priori threshold
    o = (o + 3) & ~3;
    L.offPerm = o;       o += 128;                   // column order of the enumeration: original column of a position, and back
    o = (o + 7) & ~7;
    L.offCtrl = o;       o += 240;                   // struct Ctrl
    o = (o + 7) & ~7;
    L.offOpt = o;        o += OPT_BYTES;             // struct Opt: optimistic bounds, per-node accumulators, re-split tickets
    o = (o + 15) & ~15;
    L.offGainW = o;      o += nWaves * 512;          // one line of gain terms per wave (calcGain)
    L.total = (o + 15) & ~15;
    return L;
}

// Sizes around a launch of the 64-row kernel, for the kernel's host build (tests/cpp/engine_host.cpp).  They restate, line for line,
// what the entry computes (kbest_capi.cpp: states_need, p.statesPerProblem, SplitLayout, relay_plan's image, relay_reserve's words).
// The entry keeps its own text for now: its compiled code is to stay the parent's while the GPU fault of NOTES sections 34, 35 and
// 37 is unexplained; it should call these once that is settled.
// State slots of one matrix: the lazy region (k + extraStates: the root and the candidates that are re-solved when selected) and
// the eager region behind it (children kept in full when they are found).
inline int engine_states_per_problem(int k, int extraStates, int eagerStates) { return k + extraStates + eagerStates; }
// Bytes of the work space of a (B, maxRow, k) launch -- saved hypotheses, then the slot -> state table, then 256 spare bytes -- and
// where the table starts in it.
inline size_t engine_states_need(int B, int maxRow, int k, int extraStates, int eagerStates, size_t *slotOff)
{
    const size_t nStates = (size_t)B * (size_t)engine_states_per_problem(k, extraStates, eagerStates) * (size_t)state_stride(maxRow);
    if (slotOff) *slotOff = (nStates + 127) & ~(size_t)127;
    return nStates + (size_t)B * (size_t)slot_table_stride(k) * 2 + 256;
}
// per-share result tables [S][B][...] + one shared threshold per matrix of a split launch
struct SplitLayout {
    size_t offGain, offR4C, offNf, offT, bytes;
    SplitLayout(int B, int S, int k, int maxCol)
    {
        auto up = [](size_t x) { return (x + 127) & ~(size_t)127; };
        offGain = 0;
        offR4C = up((size_t)S * B * k * 8);
        offNf = offR4C + up((size_t)S * B * k * maxCol * 4);
        offT = offNf + up((size_t)S * B * 4);
        bytes = offT + up((size_t)B * 8);
    }
};
// relay launches: bytes of one matrix' LDS image in HBM, and of the three arrays of words (pieces done, pieces claimed, workgroups
// gone: quarters of one buffer)
inline size_t relay_image_bytes(int ldsBytes) { return ((size_t)ldsBytes + 16 + 127) & ~(size_t)127; }
inline size_t relay_words_bytes(int B) { return (size_t)B * 16; }

// computeQuadricCostMatrix inputs: per frame nL landmark and nM measurement (mean[3], cov[3][3]) pairs
struct QuadricParams {
    const int *nL, *nM;
    const long long *landOff, *measOff;  // first landmark / measurement of each frame
    const double *landMean, *landCov, *measMean, *measCov;
    double gate;                         // NONASSIGN_QUADRIC
    double *cost;                        // (nL+nM) x nM column-major per frame
    const long long *costOff;
};

// computeBBCostMatrix / asgnBB inputs: boxes are (xmin, ymin, xmax, ymax, xOffset)
struct BoxParams {
    const int *nL, *nR;
    const long long *offL, *offR;
    const double *boxL, *boxR;
    double gate;                         // NONASSIGN_BOUNDBOX
    double *cost;                        // (nR+nL) x nL column-major per frame
    const long long *costOff;
    int *assign;                         // [sum nL] matched right box or -1
};

// ---- general-size kernel (kbest_wide.hip): numRow up to 64 * 16, any k; hypotheses and pool in HBM work space ----
constexpr int WIDE_NW = 8;         // waves per problem (16 in the one-workgroup-per-CU shapes, 4 beyond 512 rows: WideParams::nw)
constexpr int WIDE_MAX_DIM = 1024; // rows per problem (16 rows per lane at most)
constexpr int WIDE_MAX_SPEC = 64;  // hypotheses split per round at most
constexpr int WIDE_CTRL_BYTES = 1920;
constexpr int WIDE_SAMPLES = 1024; // LDS index of the sorted pool: every 64th gain (k up to 65 535; beyond: binary search in HBM)

struct WideParams {
    const double *cost;
    const long long *costOff;
    const int *nRow, *nCol;
    int B;                    // problems in the batch (the grid strides over them)
    int maxRow, maxCol;       // capacity of this launch (work space, LDS, rows per lane)
    int ldRow, ldCol;         // leading dimensions of the outputs / of the default cost packing
    int minRows;              // problems with fewer rows are left to the LDS kernel (mixed batches); 0 = take all
    int tile;                 // 1: the square cost copy lives in LDS (it fits), Cw is not used
    int spec;                 // hypotheses split per round (1 = the reference's order of operations exactly), <= WIDE_MAX_SPEC
    int nw;                   // waves per problem: 8 or 16 (4 beyond 512 rows: the waves' working sets are 20 bytes per row each)
    int k;
    int maximize, useCutoff;
    unsigned flags;
    double cutoff;
    int rootColOffset, rootColStride;
    int *row4col;             // [B][k][ldCol]
    int *col4row;             // [B][k][ldRow] or nullptr
    double *gain;             // [B][k]
    int *nf;                  // [B]
    long long *pushed;        // [B] or nullptr
    // work space, one slot per workgroup of the grid
    double *Cw;               // shifted, zero-padded square copy of the cost matrix
    long long cwStride;       // doubles per slot
    unsigned char *states;    // [statesPerProblem] saved hypotheses, stateStride bytes each
    long long stateStride;
    int statesPerProblem;     // k + maxCol + 2: pool + children of one sweep + the hypothesis being split
    double *poolG;            // two buffers of poolStride gains (sorted candidate pool, ping-pong)
    int *poolS;               //   ... and their state slots
    long long poolStride;
    int *freeList;            // stack of free state slots
    long long freeStride;
    unsigned long long *prof; // diagnostic builds (KB_PROFILE): [B][16] cycle sums over the waves
    int kTab;                 // exact ties (kbest_ties.h), as in Params
    double *tieGain;
    unsigned *queue;          // [0] problems taken beyond the first gridDim.x, [1] workgroups that have left (zero between launches); null: fixed stride
};

// bytes of one saved hypothesis of the general-size kernel: u[D] v[D] (fp64), row4col[D] col4row[D] (i32),
// forbidden rows (u32 per lane), gain, activeCol; whole 128-byte lines
__host__ __device__ inline long long wide_state_stride(int maxRow) { return (24LL * maxRow + 256 + 16 + 127) & ~127LL; }

// state slots at the end of a problem's work space that hold the atoms of the a-priori threshold: per column cost + rows
// moved (rows per lane words), then the root's gain
__host__ __device__ inline int wide_atom_slots(int maxRow, int maxCol)
{
    const int R = maxRow <= 64 ? 1 : (maxRow <= 128 ? 2 : (maxRow <= 256 ? 4 : (maxRow <= 512 ? 8 : 16)));
    const long long bytes = 8LL * ((long long)maxCol * (1 + R) + 1);
    return (int)((bytes + wide_state_stride(maxRow) - 1) / wide_state_stride(maxRow));
}

struct WideLds { int offWave, waveStride, offNode, nodeStride, offChildG, offChildS, offChildC, offSample, offRed, offCtrl, offPerm, offTile, total; };

// tile: keep the shifted square cost copy in LDS instead of the HBM work space (when maxRow^2 * 8 bytes fit)
// hypotheses split per round by the general-size kernel.  Measured (kernel ms at 1 / 2 / 4 / 8 per round).  Eight waves
// per problem, two or three problems per CU: 1024 x 100x20 4.1 / 3.2 / 2.7 / 2.5, 512 x 128x128 18.5 / 18.2 / 18.6 / 20.2,
// 512 x 96x96 12.0 / 11.5 / 11.7 / 12.3.  Sixteen waves, one problem per CU: 256 x 64x64 3.7 / 3.0 / 2.6 / 2.5,
// 256 x 128x128 10.5 / 9.3 / 8.8 / 9.1, 256 x 256x256 44.6 / 42.4 / 43.1 / 43.1.  With few columns a round is a handful of
// children and the rounds' latency dominates (speculation pays); with many columns one split already fills eight waves
// and speculative splits are wasted work; sixteen waves want twice the children per round.
// With k in the thousands (bruteForceProb, assignment.cpp:868) nearly every hypothesis near the pool's head is output
// sooner or later, so speculation is almost never wasted and the number of rounds is what costs (each a chain of dependent
// HBM round trips: 64 x 30x10, k = 20 000: 45 ms at 8 per round, 2 500 rounds): as many as the LDS copies allow.
__host__ __device__ inline int wide_spec(int maxCol, int nw = 8, int k = 200)
{
    // (re-scanned with the a-priori threshold in place, which makes the early rounds' speculative splits cheap: 16 waves,
    //  256 x 128x128 at 2 / 4 / 8 per round 7.5 / 6.8 / 6.7 ms, 256 x 256x256 29.4 / 28.0 / 27.9, 256 x 64x64 3.0 / 2.5 / 2.3;
    //  8 waves, 512 x 128x128 at 2 / 3 / 4 / 8: 13.2 / 13.0 / 13.0 / 19.6 -- the last one loses the second workgroup per CU)
    const int s = (nw == 16 ? 1024 : 384) / (maxCol > 0 ? maxCol : 1), lo = nw == 16 ? 2 : 1;
    if (k >= 1024) return WIDE_MAX_SPEC;  // (clamped to wide_spec_cap by the caller)
    return s >= 8 ? 8 : (s >= lo ? s : lo);
}
// capacity (LDS arrays, state slots): what KBEST_WIDE_SPEC may ask for
__host__ __device__ inline int wide_node_stride(int maxRow) { return (24 * maxRow + 256 + 16 + 15) & ~15; }  // LDS copy of a saved hypothesis
__host__ __device__ inline int wide_spec_cap(int maxCol, int maxRow)
{
    int s = 1024 / (maxCol > 0 ? maxCol : 1);
    const int fit = ((maxRow <= 64 ? 64 : 32) * 1024) / wide_node_stride(maxRow);  // the split hypotheses' LDS copies: 32 KiB at most (64 for small problems)
    s = s < fit ? s : fit;
    return s >= WIDE_MAX_SPEC ? WIDE_MAX_SPEC : (s >= 1 ? s : 1);
}

// (sized for the `spec` hypotheses actually split per round -- LDS decides how many problems a CU holds)
__host__ __device__ inline WideLds wide_lds_layout(int maxRow, int maxCol, bool tile, int nw, int spec)
{
    WideLds L;
    const int nc = spec * maxCol;                  // children of one round at most
    int o = 0;
    L.waveStride = (20 * maxRow + 15) & ~15;       // per wave: u (fp64), col4row, row4col, pred (i32)
    L.offWave = o;       o += nw * L.waveStride;
    L.nodeStride = wide_node_stride(maxRow);       // copy of a saved hypothesis (wide_state_stride's content)
    L.offNode = o;       o += spec * L.nodeStride;  // the hypotheses being split in this round
    int ncP = 1;
    while (ncP <= nc) ncP <<= 1;                   // (the gains: padded to a power of two for the merge's searches)
    L.offChildG = o;     o += ncP * 8;              // surviving children of the round: gain, state slot, (parent, column)
    L.offChildS = o;     o += nc * 4;
    L.offChildC = o;     o += nc * 4;
    o = (o + 7) & ~7;
    L.offSample = o;     o += WIDE_SAMPLES * 8;
    L.offRed = o;        o += nw * 8;
    L.offCtrl = o;       o += WIDE_CTRL_BYTES;      // struct WideCtrl
    L.offPerm = o;       o += 4 * maxRow;           // column order of the enumeration: original column of a position, and back (u16)
    o = (o + 15) & ~15;
    L.offTile = o;       if (tile) o += maxRow * maxRow * 8;
    L.total = (o + 15) & ~15;
    return L;
}

// ---- small-problem kernel (kbest_small.hip): numRow <= 32.  Half-wave workers (two children per wavefront), the
//      zero-padded columns of the reference kept implicit, two barriers per round, optional fused
//      conditionCosts prologue and assignmentProb epilogue (cost block in -> probabilities out, one launch) ----
constexpr int SMALL_MAX_DIM = 32;
constexpr int SMALL_MAX_K = 1024;
constexpr int TINY_MAX_COL = 8;        // kbest_tiny.hip: measurements per frame,
constexpr int TINY_MAX_ROW = 64;       //   rows of the raw block (landmarks + measurements),
constexpr int TINY_MAX_COUNT = 1 << 23; //   assignments of the frame in all: (nL + nM)! / nL!,
constexpr int TINY_MAX_PREFIX = 1 << 15; //  ... and prefixes of nM - 2 columns (each is decoded once by some thread),
constexpr int TINY_CAP = 1024;         //   candidates kept for the final sort
// feasible prefixes kept in LDS for the passes (1 024-thread workgroups: a lone frame on its CU; 256: batches, four per CU)
__host__ __device__ constexpr int tiny_prefix_cap(int nThreads) { return nThreads >= 1024 ? 2048 : 512; }
constexpr int BNB_MAX_COL = 16;        // kbest_bnb.hip: measurements per frame (rows of an assignment packed one byte each in 16 bytes),
constexpr int BNB_MAX_ROW = 64;        //   rows of the raw block,
// entries of each of the two frontier lists (1 024-thread workgroups: a lone frame on its CU; 256: batches)
#ifndef KB_BNB_FCAP_SMALL
#define KB_BNB_FCAP_SMALL 512
#endif
__host__ __device__ constexpr int bnb_frontier_cap(int nThreads) { return nThreads >= 1024 ? 1536 : KB_BNB_FCAP_SMALL; }
// candidates kept for the final sort (they lie in one frontier list: 28 bytes each), and the largest k that leaves them room
__host__ __device__ constexpr int bnb_cand_cap(int nThreads) { return bnb_frontier_cap(nThreads) * 32 / 28 - 4; }
__host__ __device__ constexpr int bnb_max_k(int nThreads) { return bnb_cand_cap(nThreads) - 64 < bnb_frontier_cap(nThreads) ? bnb_cand_cap(nThreads) - 64 : bnb_frontier_cap(nThreads); }
constexpr int SMALL_MAX_RAW_ROWS = 2048;  // rows of the unconditioned block (assoc mode)

struct SmallParams {
    const double *cost;       // packed column-major blocks
    const long long *costOff; // per-problem offset in doubles, or nullptr (uniform ldRow x ldCol packing)
    const int *nRow;          // rows per problem, or nullptr (uniform maxRow).  assoc mode: nL + nM of the RAW block
    const int *nCol;          // columns per problem, or nullptr (uniform maxCol)
    int maxRow, maxCol;       // solver capacity of this launch (<= 32): LDS tile, state layout
    int ldRow, ldCol;         // leading dimensions of row4col / col4row outputs and of the default cost packing
    int k;
    int maximize, useCutoff;
    double cutoff;
    int *row4col;             // [B][k][ldCol] or nullptr
    int *col4row;             // [B][k][ldRow] or nullptr
    double *gain;             // [B][k] or nullptr
    int *nf;                  // [B]; -1 shape error, -2 "does not fit this kernel" (the host re-runs it on the general path)
    unsigned char *states;    // workspace [B][statesPerProblem] x stateStride
    long long stateStride;
    int statesPerProblem;
    // association weights (assignment.cpp:547-683) fused behind the enumeration
    int weights;              // 1: write probabilities instead of / besides the assignments
    int condition;            // 1: conditionCosts first (assignment.cpp:439-525) and scatter back through its row map (:68-74)
    int gate;                 // 1: assignmentProb (solutions beyond best + 42 are skipped, :622-626); 0: bruteForceProb (:918-923)
    const int *nL;            // [B] landmarks (weights mode; nRow = nL + nM)
    double *probs;            // packed [nM][nL+1] per problem
    const long long *probOff;
    unsigned long long *prof; // diagnostic builds only
    int imm, immRow, immCol, immL;  // imm = 1 (B = 1): the shape of the one problem travels in the kernel arguments
    int tabI8;                // 1: row4col / col4row are int8 tables (KBEST_FLAG_TABLES_I8)
    int *done;                // host-mapped completion counter (zero-copy calls) or nullptr
    int bnbRow;               // kbest_bnb.hip: rows of the largest raw block of the launch (<= 64; sizes its tile)
    int onlyUnfit;            // kbest_small.hip: 1 = answer only the problems whose nf is -2 (handed back by the launch before)
    int kTab;                 // exact ties (kbest_ties.h), as in Params (the weights are those of the first kTab solutions)
    double *tieGain;
    int *tieFlags;            // fused association launches (no tables for the finishing kernel to look at): [B] KBEST_TIE_* or nullptr
    int tieBase;              // ... what a frame's flags start from (KBEST_TIE_UNCHECKED when k sits at the kernel's limit: no solution behind the k-th)
};

__host__ __device__ inline long long small_state_stride(int maxRow, int maxCol)
{
    // u[maxCol] v[maxRow] (fp64), row4col[maxCol] col4row[maxRow] (u8), forbidden-row mask (u32), activeCol, gain; whole 128-byte lines
    return ((((long long)9 * (maxRow + maxCol) + 7) & ~7LL) + 16 + 127) & ~127LL;
}

__host__ __device__ inline int small_states_per_problem(int k, int nWaves, int maxCol) { return 2 * k + 2 * nWaves * maxCol + 4; }

struct SmallLds {
    int offC, offNodes, nodeStride, offPoolG, offPoolM, offPoolS, offFreshG, offFreshM, offFreshS, offFree, offEmitG, offEmitS, offSurv,
        offProb, offRowIdx, offColMin, offKeep, offCtrl, total;
};

__host__ __device__ inline SmallLds small_lds_layout(int maxRow, int maxCol, int k, int nWaves, bool weights)
{
    SmallLds L;
    const int W = 2 * nWaves, S = small_states_per_problem(k, nWaves, maxCol);
    int o = 0;
    L.offC = o;        o += (maxCol + 1) * 33 * 8;       // cost tile: the real columns + ONE zero column (the padded ones), column stride 33
    L.nodeStride = 2 * 256 + 64 + 32 + 256 + 272;        // per worker: u[32] v[32] (fp64), col4row[32] row4col[32] (u8), scalars, gain-term line, private u[33]
    o = (o + 15) & ~15;
    L.offNodes = o;    o += W * L.nodeStride;
    L.offPoolG = o;    o += 2 * k * 8;                   // sorted candidate pool, two buffers: gain
    L.offEmitG = o;    o += k * 8;                       // gains of the emitted solutions (un-shifted)
    o = (o + 15) & ~15;
    L.offFreshG = o;   o += W * maxCol * 8;              // children completed in this round (16-byte aligned: read as double2)
    L.offProb = o;     o += weights ? maxCol * 33 * 8 : 0;  // probability accumulators [nM][condL + 1]
    L.offColMin = o;   o += weights ? maxCol * 8 : 0;
    L.offKeep = o;     o += weights ? (SMALL_MAX_RAW_ROWS / 64) * 8 : 0;  // kept-row bits of conditionCosts
    L.offPoolM = o;    o += 2 * k * 4;                   //   (parent state, column, flags)
    L.offFreshM = o;   o += W * maxCol * 4;
    L.offPoolS = o;    o += 2 * k * 2;                   //   own state slot
    L.offFreshS = o;   o += W * maxCol * 2;
    L.offEmitS = o;    o += k * 2;
    L.offSurv = o;     o += W * 32 * 2;                  // children that passed the filter: (node, column)
    L.offFree = o;     o += S * 2;                       // stack of free state slots
    L.offRowIdx = o;   o += weights ? 32 * 2 : 0;        // original row of each kept row
    o = (o + 15) & ~15;
    L.offCtrl = o;     o += 96;
    L.total = (o + 15) & ~15;
    return L;
}

// ---- lane-per-child kernel (kbest_lane.hip): numRow <= 32, dense batches.  One LANE per child of Murty's partition: the
//      rows of a child's Dijkstra are an unrolled loop over registers (spc[DR], pred[DR] per lane), 64 children advance one
//      step per pass; uses kb::Params (lazyStates, slotSid as in the 64-row kernel; every completed child is kept in full,
//      state slots come from an LDS free list) ----
constexpr int LANE_MAX_DIM = 32;
constexpr int LANE_MAX_SPEC = 16;

__host__ __device__ inline int lane_rows(int maxRow) { return maxRow <= 16 ? 16 : 32; }  // rows unrolled per lane (template DR)
// saved hypothesis of the lane kernel: the 64-row kernel's layout with DR rows -- u[DR] v[DR] (fp64), row4col[DR] col4row[DR]
// (u8), forbidden mask (u64), gain, activeCol; whole 128-byte lines
__host__ __device__ inline long long lane_state_stride(int maxRow) { return state_stride(lane_rows(maxRow)); }
// emitted + pool (<= k together) + the children completed in one round (<= spec * maxCol) + the root
__host__ __device__ inline int lane_states_per_problem(int k, int spec, int maxCol) { return k + spec * maxCol + 2; }
// bytes of the lane kernel's work space (saved hypotheses, then the slot -> state table, then 256 spare bytes) and where the table
// starts: the entry (kbest_capi.cpp) and the kernel's host build (tests/cpp/lane_host.cpp) size from this one definition
inline size_t lane_states_need(int B, int maxRow, int maxCol, int k, int spec, size_t *slotOff)
{
    const size_t nStates = (size_t)B * (size_t)lane_states_per_problem(k, spec, maxCol) * (size_t)lane_state_stride(maxRow);
    if (slotOff) *slotOff = (nStates + 127) & ~(size_t)127;
    return ((nStates + 127) & ~(size_t)127) + (size_t)B * (size_t)slot_table_stride(k) * 2 + 256;
}

struct LaneLds {
    int offC, offNodes, nodeStride, offPoolG, offFreshG, offPoolM, offFreshM, offPoolS, offFreshS, offItems, offComp, offFree, offScr,
        scrStride, offCtrl, offGainW, total;
};
// node block (a hypothesis being split), DR = lane_rows: u[DR] v[DR] (fp64) | row4col[DR] col4row[DR] (u8) | cand[DR] (u32:
// rows of the columns >= c) | gain, bound (fp64) | forbidden mask, activeCol, state slot (i32)
__host__ __device__ inline int lane_node_bytes(int DR) { return 22 * DR + 32; }

__host__ __device__ inline LaneLds lane_lds_layout(int maxRow, int maxCol, int k, int spec, int nWaves, int lanesPerChild)
{
    LaneLds L;
    const int DR = lane_rows(maxRow), ldc = maxRow | 1, nc = spec * maxCol;
    int o = 0;
    L.offC = o;        o += maxRow * ldc * 8;            // shifted, zero-padded cost tile (column stride odd: lanes on different columns hit different banks)
    o = (o + 15) & ~15;
    // lanes of one wave read v[r] of DIFFERENT nodes in one instruction: a stride of 8 (mod 128) bytes puts them on different banks
    L.nodeStride = ((lane_node_bytes(DR) + 119) & ~127) + 8;
    if (L.nodeStride < lane_node_bytes(DR)) L.nodeStride += 128;
    L.offNodes = o;    o += spec * L.nodeStride;
    o = (o + 15) & ~15;
    L.offPoolG = o;    o += k * 8;                       // sorted candidate pool: gain
    o = (o + 15) & ~15;
    L.offFreshG = o;   o += (nc > 16 ? nc : 16) * 8;     // children completed in this round (16-byte aligned: read as double2; phase 0's scratch)
    L.offPoolM = o;    o += k * 4;                       //   (parent state, column, flags)
    L.offFreshM = o;   o += nc * 4;
    L.offPoolS = o;    o += k * 2;                       //   own state slot
    L.offFreshS = o;   o += nc * 2;
    L.offItems = o;    o += nc * 2;                      // children of this round: (node, column)
    L.offComp = o;     o += nc * 2;                      // state slots of the children that reached their sink this round
    L.offFree = o;     o += lane_states_per_problem(k, spec, maxCol) * 2;  // stack of free state slots
    o = (o + 3) & ~3;
    L.scrStride = 4 * DR + 4;                            // per finishing child: row4col, col4row (u8 each), (pred, pred's row) pairs
    L.offScr = o;      o += nWaves * (64 / lanesPerChild) * L.scrStride;  // completed children are finished 64 / lanesPerChild at a time per wave
    o = (o + 15) & ~15;
    L.offCtrl = o;     o += 160;
    L.offGainW = o;    o += 512;                         // wave 0: the root's scratch line
    L.total = (o + 15) & ~15;
    return L;
}

// k-way merge of per-shard k-best lists into the global k best (kbest_merge.hip).  The lists of shard s start
// s * shardStride BYTES behind those of shard 0 (the packed per-rank slices of the all-gather, or plain [S][B][...] arrays).
struct MergeParams {
    const unsigned char *gain;     // shard 0: [B][k] fp64
    const unsigned char *row4col;  // shard 0: [B][k][ldCol] i32
    const unsigned char *nf;       // shard 0: [B] i32
    long long shardStride;         // bytes between consecutive shards' gain tables (and, unless the next two are set, of all three)
    long long strideR4C, strideNf; // 0 = shardStride (packed slices); else the tables' own strides (plain [S][B][...] arrays)
    int nShard, k, maxCol, ldCol, maximize;
    double *outGain;               // [B][k]
    int *outRow4col;               // [B][k][ldCol]
    int *outNf;                    // [B]
    int *outCol4row;               // [B][k][ldRow] or nullptr: the inverse of the merged row4col, -1 for rows without a column
    int ldRow;
    int inI8;                      // the shards' row4col tables are int8 (the merged table is int32 either way)
    int spd;                       // > 1: every block (shardStride apart) holds this many shards, tables of B problems back to back
};
// The merge from the shards' gains alone (kbest_merge.hip, merge_gains_kernel): all shards' gains and counts, the device's own
// shards' rows; out: merged gains and counts (whole), the own winners' rows at their merged positions in a byte table (zero
// elsewhere: a sum all-reduce completes it), and one word that is set when two candidates of a matrix have exactly the same gain.
struct MergeGainsParams {
    const unsigned char *gain;     // block 0: [spd][B][k] fp64; block j (a device's share of the all-gather) blockStride bytes behind
    const unsigned char *nf;       // block 0: [spd][B] i32
    long long blockStride;
    int spd;                       // shards per block (<= 1: one)
    const signed char *ownRow8;    // [ownHi - ownLo][B][k][maxCol]: the rows of shards ownLo .. ownHi-1
    int ownLo, ownHi;
    int nShard, B, k, maxCol, maximize;
    double *outGain;               // [B][k]
    signed char *outRow8;          // [B][k][maxCol], zeroed by the caller
    int *outNf;                    // [B]
    int *tied;                     // one word, zeroed by the caller
};
// kbest_batch_f64 with the tables staged in (and left in) caller-owned device buffers: the multi-device entry's per-device step
// (kbest_capi.cpp).  stamps (optional): host times (seconds, steady clock) at which the first upload / the first kernel was issued.
// row4col8 (optional): device memory for the block's row4col as bytes -- the narrow staging of uniform square batches then
// runs with it (bytes cross PCIe, col4row is rebuilt on the host and not kept).  keepI8 = 0: the table that is KEPT is the int32
// `row4col` (the narrow-staged path widens the bytes into it on the device); keepI8 = 1: the kept table is the byte table
// `row4col8` (a device's slice of the multi-device exchange, which travels in bytes) and `row4col` is int32 staging for the paths
// whose kernels write int32 (they narrow it into row4col8 on the device).
struct KeepTables { int32_t *row4col, *col4row; double *gain; int32_t *nf; double *stamps; signed char *row4col8; int keepI8; };
hipError_t launch_widen_i8(const signed char *src, int *dst, long long n, hipStream_t stream);
hipError_t launch_copy_words(const void *src, void *dst, long long bytes, hipStream_t stream);  // bytes: a multiple of 4
double now_s();
// kbest_exact.hip: kBest2D / kBest2DCutoff in the reference's own order of operations (padded N x N formulation, one heap of fully
// solved hypotheses with libstdc++'s sift rules), any size: KBEST_FLAG_REFERENCE_ORDER, and every problem beyond KBEST_MAX_DIM_WIDE rows
struct ExactParams {
    const double *cost;
    const long long *costOff;
    const int *nRow, *nCol;
    int B, maxRow, maxCol, ldRow, ldCol, k, maximize, useCutoff;
    unsigned flags;            // KBEST_FLAG_TABLES_I8
    double cutoff;
    int *row4col, *col4row;    // [B][k][ldCol] / [B][k][ldRow] (col4row may be null; padded columns named as the reference names them)
    double *gain;
    int *nf;                   // -4: the work space's pool of hypotheses ran out
    long long *pushed;         // or null
    unsigned char *work;       // gridDim.x slots of exact_slot_bytes(maxRow, hypPerSlot)
    int hypPerSlot;
    int childWaves;            // (set by launch_kbest_exact: waves of a workgroup that solve children, 65 .. 1 024 rows)
};
long long exact_slot_bytes(int maxRow, int hypPerSlot);
hipError_t launch_kbest_exact(const ExactParams &p, int grid, hipStream_t stream);
hipError_t launch_merge_topk(const MergeParams &p, int B, hipStream_t stream);
hipError_t launch_merge_gains(const MergeGainsParams &p, hipStream_t stream);
hipError_t launch_zero_words(unsigned *w, long long n, hipStream_t stream);
hipError_t launch_narrow_i32(const int *src, signed char *dst, long long n, hipStream_t stream);
hipError_t launch_add_i8(signed char *dst, const signed char *src, long long n, hipStream_t stream);
hipError_t launch_fill_unused(const int *nf, const int *nRow, const int *nCol, int B, int k, int ldCol, int ldRow, int *row4col,
                              int *col4row, double *gain, bool tablesI8, hipStream_t stream);
// The kernel behind every enumeration launch (kbest_merge.hip, kbest_ties.h): runs of equal gains into the canonical order,
// KBEST_TIE_* flags from tieGain (the gain of the solution behind the tables; nullptr: none was enumerated) into tieFlags (or
// nullptr), and -- fill -- the unused slots / the padding of a ragged batch as launch_fill_unused defines them.
hipError_t launch_finish_tables(const int *nf, const int *nRow, const int *nCol, int B, int k, int ldCol, int ldRow, int *row4col,
                                int *col4row, double *gain, bool tablesI8, const double *tieGain, int *tieFlags, bool fill, hipStream_t stream,
                                int baseFlags = 0, bool order = true);  // baseFlags: or-ed into every problem's flags (KBEST_TIE_UNCHECKED);
                                                                        // order = false: runs of equal gains are reported, not ordered (tables in host memory)
hipError_t launch_kbest_lane(const Params &p, int B, int nWaves, int lanesPerChild, hipStream_t stream);
hipError_t launch_kbest_small(const SmallParams &p, int B, int nWaves, hipStream_t stream);
// kbest_tiny.hip: the fused association path by exhaustive enumeration, for frames whose assignments are few (condition + gate +
// cutoff mode of SmallParams only); nf = -2: the frame is for the enumeration kernels after all
hipError_t launch_kbest_tiny(const SmallParams &p, int B, bool many, hipStream_t stream);
// kbest_bnb.hip: the fused association path by a bounded depth-first walk over the columns (every assignment whose partial sums
// stay below a bound that is raised until k assignments lie below it); same modes and -2 convention as kbest_tiny.hip
hipError_t launch_kbest_bnb(const SmallParams &p, int B, bool many, hipStream_t stream);
int bnb_lds_bytes(int k, int nThreads = 1024, int maxRow = 64, int maxCol = 16);
int tiny_lds_bytes(int k, int nThreads = 1024);
hipError_t launch_kbest(const Params &p, int B, int nWaves, hipStream_t stream);
hipError_t launch_kbest_wide(const WideParams &p, int grid, hipStream_t stream);
hipError_t launch_quadric_costs(const QuadricParams &p, int B, hipStream_t stream);
hipError_t launch_bb_costs(const BoxParams &p, int B, hipStream_t stream);
hipError_t launch_bb_assign(const BoxParams &p, const int *row4col, const int *nf, int k, int maxCol, int B,
                            hipStream_t stream);
hipError_t launch_weights(const WeightParams &p, int B, hipStream_t stream);
hipError_t launch_condition(const CondParams &p, int B, hipStream_t stream);
hipError_t launch_to_probs(double *x, long long n, hipStream_t stream);

// kbest_perm.hip: permanentProb, the exact association probabilities by sums over column subsets
struct PermParams {
    const double *cost;        // packed column-major (nL + nM) x nM blocks
    const long long *costOff;  // [B]
    const long long *probOff;  // [B]
    const int *nL, *nM;        // [B]
    double *probs;             // [nM][nL + 1] per frame
    double *perm;              // [B] or nullptr: the permanent of the frame's toProbs matrix
    double *work;              // work space: slotStride doubles per workgroup of the launch (modes 1, 2)
    long long slotStride;
    int B, maxRawRow, maxCol, condition;
};
struct PermPlan {
    int mode;               // 0: every layer in LDS; 1: the forward layers in the work space; 2: everything there
    int threads, lds;       // workgroup size, dynamic LDS bytes
    long long slotDoubles;  // work space per workgroup
};
PermPlan perm_plan(int maxRawRow, int maxCol, int ldsLimit, int ldsPerCU);
hipError_t launch_kbest_perm(const PermParams &p, const PermPlan &pl, int grid, hipStream_t stream);

// kbest_sample.hip: joint associations drawn from the exact posterior, on the forward layers of the permanent kernel (its plan)
struct SampleParams {
    const double *cost;        // packed column-major (nL + nM) x nM blocks
    const long long *costOff;  // [B]
    const int *nL, *nM;        // [B]
    const u64 *frameKey;       // [B] or nullptr (frame b: b): words 2 and 3 of the generator's counter
    int *assign;               // [nSample][nM] per frame at asgOff[b]: the raw row every column takes
    const long long *asgOff;   // [B]
    double *logProb;           // [nSample] per frame at lpOff[b]
    const long long *lpOff;    // [B]
    double *perm;              // [B] or nullptr: the permanent of the frame's toProbs matrix
    double *work;              // work space: slotStride doubles per workgroup of the launch (modes 1, 2)
    long long slotStride;
    u64 seed;                  // the generator's key
    u32 sampleBase;            // sample s of the launch is draw sampleBase + s of the frame
    int nSample;
    int B, maxRawRow, maxCol, condition;
};
hipError_t launch_kbest_sample(const SampleParams &p, const PermPlan &pl, int grid, hipStream_t stream);

// kbest_lbp.hip: beliefProb, the association probabilities by loopy belief propagation on the assignment model (any frame size)
struct LbpParams {
    const double *cost;        // packed column-major (nL + nM) x nM blocks
    const long long *costOff;  // [B]
    const long long *probOff;  // [B]
    const int *nL, *nM;        // [B]
    double *probs;             // [nM][nL + 1] per frame
    int *iters;                // [B] or nullptr: sweeps run; -1: frame beyond the launch's bounds; -2: infeasible frame
    double *resid;             // [B] or nullptr: max |nu' - nu| of the last sweep
    double *work;              // work space: slotStride doubles per workgroup of the launch (mode 1)
    long long slotStride;
    double tol;
    int maxIter, B, maxRawRow, maxCol, condition;
};
struct LbpPlan {
    int mode;               // 0: a, nu and the two sweep buffers in LDS; 1: in the work space
    int threads, lds;       // workgroup size (one wave per 64 rows of the launch's bound), dynamic LDS bytes
    long long slotDoubles;  // work space per workgroup
};
LbpPlan lbp_plan(int maxRawRow, int maxCol, int ldsLimit);
hipError_t launch_kbest_lbp(const LbpParams &p, const LbpPlan &pl, int grid, hipStream_t stream);

// kbest_cluster.hip: clusterProb, the exact association probabilities by gated clusters (frames of up to 128 measurements whose
// clusters have at most 16)
struct ClusterParams {
    const double *cost;        // packed column-major (nL + nM) x nM blocks
    const long long *costOff;  // [B]
    const long long *probOff;  // [B]
    const int *nL, *nM;        // [B]
    double *probs;             // [nM][nL + 1] per frame
    double *logPerm;           // [B] or nullptr: sum over the clusters of log Z_k; -inf: infeasible; NaN: refused
    int *info;                 // [B] or nullptr: clusters; 0: infeasible; -1: beyond the launch's bounds; -2 / -3: refused
    int *maxCluster;           // [B] or nullptr: columns of the frame's largest cluster
    int *label;                // [B][labelStride] or nullptr: the lowest column of every column's cluster, -1 beyond nM
    double *work;              // work space: slotStride doubles per workgroup of the launch
    long long slotStride;      // maxRawRow * 16 doubles for a cluster's a, then slotBytes of layers
    long long slotBytes;       // layers (R_k + 2) 2^m_k 8 bytes beyond it: the frame is refused (-3)
    int labelStride, arenaBytes, B, maxRawRow, maxCol, condition;
};
// the partial mode's own arguments (launch_kbest_cluster_partial; kbest_c.h, "Hybrid association probabilities")
struct ClusterOpenParams {
    int maxExact;              // 1 .. 16: a cluster of more columns is open
    int descStride, rowStride; // >= the largest nM; >= the largest nL
    int *nOpen;                // [B]: open clusters of the frame
    int *openDesc;             // [B][descStride][4]: root label, m_k, nL_k, R_k of every open cluster, in label order
    int *openRows;             // [B][rowStride]: their landmark rows (caller numbering, ascending), one cluster after another
    double *sub;               // shaped like cost: their (nL_k + m_k) x m_k sub-blocks, one after another from costOff[b]
};
struct ClusterPlan {
    int threads, lds, arena;  // workgroup size, dynamic LDS bytes (-1: the device's LDS is too small), its part for layers
    long long slotBytes, slotDoubles;
};
ClusterPlan cluster_plan(int maxRawRow, int maxCol, int ldsLimit, size_t slotCap);
hipError_t launch_kbest_cluster(const ClusterParams &p, const ClusterPlan &pl, int grid, hipStream_t stream);
hipError_t launch_kbest_cluster_partial(const ClusterParams &p, const ClusterOpenParams &q, const ClusterPlan &pl, int grid,
                                        hipStream_t stream);

// kbest_cluster_sample.hip: joint associations drawn from the exact posterior of a gated frame, one walk per cluster (the plan, the
// work space and the refusals of kbest_cluster.hip, the generator and the walk of kbest_sample.hip)
struct ClusterSampleParams {
    const double *cost;        // packed column-major (nL + nM) x nM blocks
    const long long *costOff;  // [B]
    const int *nL, *nM;        // [B]
    const u64 *frameKey;       // [B] or nullptr (frame b: b): words 2 and 3 of the generator's counter
    int *assign;               // [nSample][nM] per frame at asgOff[b]: the raw row every column takes
    const long long *asgOff;   // [B]
    double *logProb;           // [nSample] per frame at lpOff[b]
    const long long *lpOff;    // [B]
    double *logPerm;           // [B] or nullptr, info, maxCluster: as ClusterParams
    int *info;
    int *maxCluster;
    double *work;              // work space: slotStride doubles per workgroup of the launch
    long long slotStride;      // maxRawRow * 16 doubles for a cluster's a, then slotBytes of layers
    long long slotBytes;       // layers (R_k + 2) 2^m_k 8 bytes beyond it: the frame is refused (-3)
    u64 seed;                  // the generator's key
    u32 sampleBase;            // sample s of the launch is draw sampleBase + s of the frame
    int nSample;
    int arenaBytes, B, maxRawRow, maxCol, condition;
};
hipError_t launch_kbest_cluster_sample(const ClusterSampleParams &p, const ClusterPlan &pl, int grid, hipStream_t stream);
// ... its second instantiation (kbest_cluster_sample_partial.hip): clusters of more than maxExact columns, or beyond the slot, are
// left open -- their columns -1, no term of theirs in logProb or logPerm
hipError_t launch_kbest_cluster_sample_partial(const ClusterSampleParams &p, int maxExact, const ClusterPlan &pl, int grid,
                                               hipStream_t stream);

// The column-scaled exact tiers (kbest_bigcluster.hip, kbest_frontier.hip, kbest_frontier_sample.hip) answer a cluster only while
// Z' >= 2^-970: there every term within 2^-52 of Z' is still a normal double.  Below it (Z' = 0 included) a cluster that has a
// complete assignment is declined with KB_INFO_OUT_OF_RANGE, its outputs untouched; info 0 is left to the clusters that have none.
constexpr double KB_RANGE_MIN_Z = 0x1.0p-970;
constexpr int KB_INFO_OUT_OF_RANGE = -5;       // KBEST_INFO_OUT_OF_RANGE

// kbest_bigcluster.hip: one open cluster of up to 20 measurements over the whole chip, its layers in HBM (kbest_c.h, "Exact
// association probabilities of clusters of 17 .. 20 measurements").  The clusters of a pack share every launch (grid.y).
constexpr int KB_BIGCLUSTER_PACK = 32;
struct BigClusterDesc {
    long long subOff, probOff;     // the cluster's sub-block / its [m][nL + 1] probabilities, in doubles from the caller's buffers
    long long layerOff, smallOff;  // its layers (rows + 3) 2^m / its small arrays (bigcluster_small), in doubles from the work spaces
    int m, nL, rows, idx;          // columns, landmark rows, rows of the sub-block (nL + m), its place in logZ / info
};
struct BigClusterPack {
    BigClusterDesc c[KB_BIGCLUSTER_PACK];
    int n;
};
// workgroups of the backward sweep, one partial sum each: from m alone (1 024 subsets a workgroup)
__host__ __device__ inline int bigcluster_workgroups(int m) { return m <= 10 ? 1 : 1 << (m - 10); }
struct BigClusterSmall { long long a, colMin, sumCol, miss, part, ints, total; };  // offsets in doubles
__host__ __device__ inline BigClusterSmall bigcluster_small(int m, int rows)
{
    BigClusterSmall s;
    long long o = 0;
    s.a = o;      o += (long long)rows * m;                              // a'[R][m]
    s.colMin = o; o += m;
    s.sumCol = o; o += 1;
    s.miss = o;   o += (long long)m * m;                                 // w of the rows >= nL: [row - nL][column]
    s.part = o;   o += (long long)rows * bigcluster_workgroups(m) * m;   // [row][workgroup][column]
    s.ints = o;   o += (2ll * rows + 1 + 1) / 2;                         // int R, rowIdx[rows], mask[rows]
    s.total = o;
    return s;
}
hipError_t launch_bigcluster_pack(const BigClusterPack &p, const double *sub, double *probs, double *logZ, int *info, double *layers,
                                  double *small, hipStream_t stream);
hipError_t launch_bigcluster_flag(int *info, int idx, int value, hipStream_t stream);

// kbest_frontier.hip: an open cluster of up to 64 measurements by a frontier sweep, one workgroup per cluster (kbest_c.h, "Exact
// association probabilities of sparse clusters").  The descriptors travel as a kernel argument: nothing is staged or allocated.
constexpr int KB_FRONTIER_PACK = 128;          // clusters of one launch
constexpr int KB_FRONTIER_MAX_COLS = 64;       // KBEST_FRONTIER_MAX_COLS
constexpr int KB_FRONTIER_MAX_WIDTH = 16;      // KBEST_FRONTIER_MAX_WIDTH
constexpr int KB_FRONTIER_MAX_ROWS = 1024 + 64;  // nL_k + m_k
constexpr int KB_FRONTIER_THREADS = 256;
constexpr int KB_FRONTIER_STEP_DOUBLES = 10;   // one step of the plan (FrontierStep, 80 bytes)
struct FrontierDesc {
    long long subOff, probOff;  // the cluster's sub-block / its [m][nL + 1] probabilities, in doubles from the caller's buffers
    int m, nL;                  // columns, landmark rows
};
struct FrontierPack {
    FrontierDesc c[KB_FRONTIER_PACK];
    int n, base;                // clusters; the place of the first one in logZ / info / width
};
struct FrontierWork {
    double *layers;             // slotDoubles per workgroup: the forward layers, then two buffers of 2^W for the backward sweep
    double *plan;               // planDoubles per workgroup: KB_FRONTIER_STEP_DOUBLES per row of the largest cluster
    long long slotDoubles, planDoubles;
};
hipError_t launch_frontier_pack(const FrontierPack &p, const double *sub, double *probs, double *logZ, int *info, int *width,
                                const FrontierWork &w, int grid, hipStream_t stream);

// kbest_frontier_sample.hip: joint associations drawn from the exact posterior of such a cluster -- the plan and the forward sweep
// of kbest_frontier.hip, then one backward walk per draw (kbest_c.h, "Draws from the exact posterior of sparse clusters").  The
// work space is the frontier tier's (FrontierWork); the descriptors travel as a kernel argument.
constexpr int KB_FRONTIER_SAMPLE_PACK = 64;    // clusters of one launch
struct FrontierSampleDesc {
    long long subOff;           // the cluster's sub-block, in doubles from sub
    long long rowKeyOff;        // the keys q of its nL + m rows, in int32s from rowKeys
    long long asgOff, ltOff;    // its [nSample][m] rows / its [nSample] terms, from the caller's buffers
    u64 frameKey;               // words 2 and 3 of the generator's counter
    int m, nL;                  // columns, landmark rows
};
struct FrontierSamplePack {
    FrontierSampleDesc c[KB_FRONTIER_SAMPLE_PACK];
    int n, base;                // clusters; the place of the first one in logZ / info / width
};
hipError_t launch_frontier_sample_pack(const FrontierSamplePack &p, const double *sub, const int *rowKeys, int nSample, u64 seed,
                                       u32 sampleBase, int *assignLocal, double *logTerm, double *logZ, int *info, int *width,
                                       const FrontierWork &w, int grid, hipStream_t stream);

// kbest_hybrid.hip: the exact hybrid path on the device (kbest_c.h, "Asynchronous exact hybrid probabilities").  One open cluster
// of the flat list hybrid_gather_kernel makes of the partial kernel's descriptors, in frame order, then label order.
struct HybridItem {
    long long subOff, probOff;  // its sub-block in sub / its [m][nL + 1] probabilities in the packed buffer, in doubles
    long long rowAt;            // its landmark rows in openRows
    int b, root, m, nL;         // frame, root label, columns, landmark rows
    int idx, sent;              // its place in the list (and in logZ / info / width); 0: more than 64 columns, the sweep skips it
};
struct HybridParams {
    const int *nL, *nM;                        // [B]
    const long long *costOff, *probOff;        // [B]
    const double *cost;
    double *probs, *logPerm;                   // logPerm: the partial kernel's sums in, the frames' out (or nullptr)
    int *method, *nOpenOut, *nFrontier;        // [B]; nOpenOut, nFrontier may be nullptr
    const int *info, *nOpen, *label, *openDesc, *openRows;  // the partial kernel's outputs: [B], [B], [B][maxCol], [B][maxCol][4], [B][maxRawRow]
    HybridItem *list;                          // [B * maxCol]
    int *count, *first;                        // clusters in the list; [B]: the first cluster of every frame
    const double *packed, *logZ;               // the sweep's outputs per cluster of the list
    const int *finfo, *width;
    long long packStride;                      // doubles of the packed buffer per frame
    int B, maxRawRow, maxCol, condition, maxWidth;
};
// the sweep of kbest_frontier.hip on the gathered list: `grid` workgroups, each with a slot and a plan of w
hipError_t launch_frontier_list(const HybridItem *list, const int *count, const double *sub, double *probs, double *logZ, int *info,
                                int *width, const FrontierWork &w, int grid, hipStream_t stream);
hipError_t launch_hybrid_gather(const HybridParams &p, hipStream_t stream);
hipError_t launch_hybrid_scatter(const HybridParams &p, hipStream_t stream);

// kbest_hybrid_sample.hip: the exact hybrid DRAWS on the device (kbest_c.h, "Asynchronous exact hybrid draws").  What the sampler of
// kbest_frontier_sample.hip needs of a cluster of that list besides its HybridItem, at the same place k.
struct HybridKeyItem {
    long long rowKeyOff;        // the keys q of its nL + m rows, in int32s from rowKey
    long long asgOff, ltOff;    // its [nSample][m] local rows in local / its [nSample] terms in term
    u64 frameKey;               // words 2 and 3 of the generator's counter
    int R, sent;                // rows that count; 0: not sent (HybridItem::sent == 0, or its rows could not be told)
};
struct HybridSampleParams {
    const int *nL, *nM;                        // [B]
    const long long *costOff, *asgOff, *lpOff; // [B]: the caller's
    const double *cost;
    const u64 *frameKey;                       // [B] or nullptr (frame b: b)
    int *assign;                               // the clustered sampler's draws in, the frames' out
    double *logProb, *logPerm;                 // logPerm: out, or nullptr
    int *method, *nOpenOut, *nFrontier;        // [B]; nOpenOut, nFrontier may be nullptr
    const int *info, *nOpen, *label, *openDesc, *openRows;  // the partial kernel's outputs, as HybridParams
    const double *partLogPerm, *drawLogPerm;   // [B]: the partial kernel's sums / the clustered sampler's
    long long *probOff;                        // [B]: where the partial kernel's (dropped) probabilities go in the packed scratch
    const HybridItem *list;                    // hybrid_gather_kernel's
    const int *count, *first;
    HybridKeyItem *keys;                       // [B * maxCol], beside list
    int *rowKey;                               // [B][maxRawRow]
    int *local;                                // [B][nSample * maxCol]
    double *term;                              // [B * maxCol][nSample]
    const double *logZ;                        // the list sampler's outputs per cluster of the list
    const int *finfo, *width;
    long long packStride;
    int B, maxRawRow, maxCol, condition, maxWidth, nSample;
};
hipError_t launch_hybrid_sample_prepare(const HybridSampleParams &p, hipStream_t stream);
hipError_t launch_hybrid_sample_keys(const HybridSampleParams &p, hipStream_t stream);
hipError_t launch_hybrid_sample_join(const HybridSampleParams &p, hipStream_t stream);
// the sampler of kbest_frontier_sample.hip on that list: `grid` workgroups, each with a slot and a plan of w
hipError_t launch_frontier_sample_list(const HybridItem *list, const HybridKeyItem *keys, const int *count, const double *sub,
                                       const int *rowKeys, int nSample, u64 seed, u32 sampleBase, int *assignLocal, double *logTerm,
                                       double *logZ, int *info, int *width, const FrontierWork &w, int grid, hipStream_t stream);

}  // namespace kb

// kbest_capi.cpp: completes the gain levels that straddle slot k in the caller's HOST tables (see there)
#ifdef __cplusplus
#include <vector>
void kb_complete_tie_levels(kbest_ctx *ctx, const kbest_opts *opts, int B, int maxRow, int maxCol, const int32_t *nRow, const int32_t *nCol,
                            const double *cost, const int64_t *costOff, int k, void *row4col, void *col4row, double *gain, int32_t *nf,
                            int32_t *fl, std::vector<int> *changed);
#endif
int kbest_batch_f64_keep(kbest_ctx *ctx, const kbest_opts *opts, int B, int maxRow, int maxCol, const int32_t *nRow,
                         const int32_t *nCol, const double *cost, const int64_t *costOff, int k, int32_t *row4col,
                         int32_t *col4row, double *gain, int32_t *nf, int64_t *pushed, const kb::KeepTables *keep);
#endif

// kbest_shims.hpp -- C++ drop-in declarations with the reference's own names
// and signatures, implemented on the MI355X engine (kbest_c.h) with B = 1.
//
// A caller written against the reference's shortestPathCPP.hpp / assignment.h
// keeps compiling against this header and links libkbest_amd.so instead of
// shortestPathCPP.o / the solver part of assignment.o:
//
//   kBest2D        shortestPathCPP.hpp:204-212   (callers: assignment.cpp:880)
//   kBest2DCutoff  shortestPathCPP.hpp:256-265   (callers: assignment.cpp:594)
//   assign2D       shortestPathCPP.hpp:144-149   (no caller in the reference)
//   shortestPathCPP shortestPathCPP.hpp:178-182  (callers: cpp:587, 668, 749)
//   toProbs        assignment.h:19               (callers: assignment.cpp:164)
//   assignmentProb assignment.h:11               (callers: assignment.cpp:66, comparison.cpp:194-222)
//   conditionCosts assignment.h:26               (callers: assignment.cpp:58, comparison.cpp:161)
//   permanentProb  assignment.h:13               (callers: assignment.cpp:64, comparison.cpp:225, 233)
//
// MurtyHyp / ScratchSpace keep the reference's public member names, types and
// declaration order (shortestPathCPP.hpp:22-65, 73-142) so that objects built
// by such a caller have the layout these functions expect.  The engine keeps
// its own device workspace, so ScratchSpace is only honoured as an interface:
// its flags are set the way kBest2DCutoff sets them (cpp:650-651), its buffers
// are not used.
//
// col4rowBest on zero-padded columns: for numRow > numCol the reference pads to a square, and WHICH padded column a
// left-over row lands on is an artefact of tie resolution among identical zero columns.  The
// engine's root starts from a column reduction and places left-over rows on the padded columns in ascending row order:
// values >= numCol in col4rowBest can differ from the reference's; values < numCol, row4colBest, gainBest and the return
// value are identical (the reference's own callers read only row4colBest, assignment.cpp:629).  KBEST_EXACT_ROOT=1 (or
// KBEST_FLAG_EXACT_ROOT) makes the root run the reference's own sequence of augmentations instead.
//
// Exact ties: hypotheses with exactly equal gains come back in the engine's one order -- (gain, row4col lexicographic), and
// the lexicographically first assignments of a gain level that straddles slot k (kbest_c.h, "Order of exact ties") -- not in
// the order of the reference's heap, which is an artefact (cpp:30-42, 574).  The flags of the last call are read with
// kbest_last_tie_flags on the shims' context (kbest_shims_context()).
//
// Error behaviour follows the reference: no exceptions from the solver, the
// return value is the number of solutions found and 0 means infeasible.  An
// engine failure (no GPU, unsupported size) cannot be expressed in that
// convention, so it throws std::runtime_error -- the product never silently
// falls back to a CPU path.
#ifndef KBEST_SHIMS_HPP
#define KBEST_SHIMS_HPP

#include <cstddef>
#include <cstdint>
#include <vector>

class MurtyHyp {
private:
    char *buffer;

public:
    ptrdiff_t *col4row;
    ptrdiff_t *row4col;
    double gain;
    double *u;
    double *v;
    size_t activeCol;
    bool *forbiddenActiveRows;
    bool solved;

    MurtyHyp() : buffer(nullptr) {}
    MurtyHyp(const size_t numRow, const size_t numCol);
    ~MurtyHyp() { delete[] buffer; }
    MurtyHyp(const MurtyHyp &) = delete;
    MurtyHyp &operator=(const MurtyHyp &) = delete;
};

class ScratchSpace {
public:
    char *buffer;
    double *C;
    size_t *ScannedColIdx;
    bool *ScannedRows;
    size_t *pred;
    double *shortestPathCost;
    ptrdiff_t *Row2ScanParent;
    ptrdiff_t *Row2Scan;
    bool *forbiddenActiveRows;
    bool toCut;
    double cutoffGain;
    bool maximize;

    ScratchSpace() : buffer(nullptr), toCut(false) {}
    ScratchSpace(const size_t numRow, const size_t numCol) : buffer(nullptr) { init(numRow, numCol); }
    void init(const size_t numRow, const size_t numCol);
    ~ScratchSpace() { delete[] buffer; }
    inline bool cutHyp(double gain) const { return toCut ? (maximize ? gain < cutoffGain : gain > cutoffGain) : false; }
};

size_t kBest2D(const size_t k, const size_t numRow, const size_t numCol, const bool maximize, const double *C,
               ScratchSpace &workMem, ptrdiff_t *col4rowBest, ptrdiff_t *row4colBest, double *gainBest);

size_t kBest2DCutoff(const size_t k, const size_t numRow, const size_t numCol, const bool maximize, const double *C,
                     ScratchSpace &workMem, ptrdiff_t *col4rowBest, ptrdiff_t *row4colBest, double *gainBest,
                     double cutoff);

int assign2D(const size_t numRow, const size_t numCol, const bool maximize, const double *C, ScratchSpace &workMem,
             MurtyHyp *problemSol);

// shortestPathCPP.hpp:178-182 (cpp:119-238): the root LAP on workMem.C (numRow x numCol, already non-negative);
// fills problemSol (col4row, row4col, u, v, gain over the first numCol4Gain columns, forbiddenActiveRows);
// returns 1 with gain = -1 when infeasible, else 0
int shortestPathCPP(MurtyHyp *problemSol, ScratchSpace &workMem, const size_t numRow, const size_t numCol,
                    const size_t numCol4Gain);

std::vector<std::vector<double>> assignmentProb(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t k);

// assignment.h:43 (assignment.cpp:835-963): every assignment up to a Minc-type bound (at most 20000), no 42-gate
std::vector<std::vector<double>> bruteForceProb(const std::vector<double> &costMatrix, size_t nL, size_t nM);

// assignment.h:19 (assignment.cpp:527-542): exp(min - c) with the 42 gate, in place
void toProbs(std::vector<double> &costMatrix);

// assignment.h:26 (assignment.cpp:439-525)
std::vector<double> conditionCosts(const std::vector<double> &costs, size_t nRows, size_t nCols,
                                   std::vector<ptrdiff_t> &rowIdxOut);

// assignment.h:13 (assignment.cpp:145-290): the exact association probabilities as ratios of permanents, [nM][nL+1].  By value, as
// the reference declares it.  permOpt 0 (Huber's sampling estimate), 1 (exact) and 2 (long double) all return the exact marginals
// (kbest_permanent_probs_batch_f64: sums over column subsets, nM <= 16); any other value throws std::runtime_error
// (assignment.cpp:344, 406).
std::vector<std::vector<double>> permanentProb(std::vector<double> costMatrix, size_t nL, size_t nM, int permOpt);

// Not in the reference: nSample joint associations drawn from the exact posterior permanentProb gives the marginals of
// (kbest_sample_assoc_batch_f64, nM <= 16; frame key 0, draws 0 .. nSample-1 of `seed`): [nSample][nM], entry [s][c] the row of
// costMatrix that measurement c takes in draw s (a row >= nL: unassigned).  A frame without any consistent association (permanent
// 0) throws std::runtime_error.
std::vector<std::vector<int>> sampleAssoc(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t nSample, uint64_t seed);

// Not in the reference: the association probabilities by loopy belief propagation (kbest_belief_probs_batch_f64, tol 1e-12, at most
// 10 000 sweeps), [nM][nL+1] like assignmentProb, for frames of up to 128 measurements and 1 024 rows -- the frames permanentProb
// does not take.  An approximation of known quality (include/kbest_c.h); an infeasible frame comes back as all zeros.
std::vector<std::vector<double>> beliefProb(const std::vector<double> &costMatrix, size_t nL, size_t nM);

// Not in the reference: the EXACT association probabilities by gated clusters (kbest_clustered_probs_batch_f64), [nM][nL+1] like
// assignmentProb, for frames of up to 128 measurements and 1 024 rows whose clusters have at most 16 measurements.  Throws
// std::runtime_error naming the largest cluster when the frame is refused; an infeasible frame comes back as all zeros.
std::vector<std::vector<double>> clusterProb(const std::vector<double> &costMatrix, size_t nL, size_t nM);

// Not in the reference: sampleAssoc for the frames clusterProb takes (kbest_clustered_sample_assoc_batch_f64: up to 128
// measurements and 1 024 rows, clusters of at most 16 measurements; frame key 0, draws 0 .. nSample-1 of `seed`): [nSample][nM],
// entry [s][c] the row of costMatrix that measurement c takes in draw s (a row >= nL: unassigned).  On a frame sampleAssoc takes the
// draws are sampleAssoc's.  Throws std::runtime_error naming the largest cluster when the frame is refused, and when the frame has no
// consistent association.
std::vector<std::vector<int>> clusterSampleAssoc(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t nSample,
                                                 uint64_t seed);

// Not in the reference: clusterSampleAssoc for the frames hybridFrontierProb(k = 0) takes
// (kbest_hybrid_frontier_sample_assoc_batch_f64 with maxExact = 16, maxWidth = 16; frame key 0, draws 0 .. nSample-1 of `seed`):
// clusters of up to 64 measurements whose rows, in the greedy order, keep at most 16 columns open are drawn too.  [nSample][nM] as
// clusterSampleAssoc, and on a frame clusterSampleAssoc takes its draws.  Throws std::runtime_error naming the largest cluster when
// the frame is refused, and when the frame has no consistent association.
std::vector<std::vector<int>> hybridFrontierSampleAssoc(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t nSample,
                                                        uint64_t seed);

// Not in the reference: hybridFrontierSampleAssoc for EVERY gated frame (kbest_hybrid_sample_assoc_batch_f64, frame key 0): a cluster
// no exact tier takes is drawn from its k best assignments within the cutoff 42 under assignmentProb's weights (k >= 1; k = 0 refuses
// such a frame, as hybridFrontierSampleAssoc does).  [nSample][nM] as clusterSampleAssoc.  Throws std::runtime_error when the frame is
// refused, and when the frame has no consistent association.
std::vector<std::vector<int>> hybridSampleAssoc(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t nSample, size_t k,
                                                uint64_t seed = 0);

// Not in the reference: the hybrid association probabilities (kbest_hybrid_probs_batch_f64), [nM][nL+1] like assignmentProb, for
// frames of up to 128 measurements and 1 024 rows: exact on every cluster of at most 16 measurements, assignmentProb(k) on the
// larger ones alone.  Throws std::runtime_error only when the frame is refused (method -1: not the reference's layout of miss
// rows); an infeasible frame comes back as all zeros.
std::vector<std::vector<double>> hybridProb(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t k);

// Not in the reference: hybridProb with the exact tier for clusters of 17 .. 20 measurements in between
// (kbest_hybrid_exact_probs_batch_f64): exact on every cluster of at most 20 measurements, assignmentProb(k) on the larger ones alone;
// k = 0: a frame with a larger cluster is refused.  Throws std::runtime_error only when the frame is refused (method -1); an
// infeasible frame comes back as all zeros.
std::vector<std::vector<double>> hybridExactProb(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t k);

// Not in the reference: hybridExactProb with the frontier tier first (kbest_hybrid_frontier_probs_batch_f64): exact on every cluster
// of at most 64 measurements whose rows, in the greedy order, keep at most 16 columns open, and on every other of at most 20;
// assignmentProb(k) on what is left; k = 0: a frame with such a cluster is refused.  Throws std::runtime_error only when the frame
// is refused (method -1); an infeasible frame comes back as all zeros.
std::vector<std::vector<double>> hybridFrontierProb(const std::vector<double> &costMatrix, size_t nL, size_t nM, size_t k);

// Not in the reference: the engine context behind the functions above (created on first use, GPU 0), for the entries of
// kbest_c.h that take one -- e.g. kbest_last_tie_flags after a call.
struct kbest_ctx;
kbest_ctx *kbest_shims_context();

#endif

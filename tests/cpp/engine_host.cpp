// kbest_engine.hip -- the 64-row k-best kernel, condition_kernel, weights_kernel -- and the launches behind it (kbest_merge.hip with
// kbest_ties.h: merge_topk_kernel, finish_tables_kernel, fill_unused_kernel) compiled for the HOST, line for line: a workgroup is
// waves * 64 std::threads, __syncthreads a std::barrier, every wave operation an exchange through the wave's barrier with the lane
// semantics of gfx950 (hip_on_host.h).  The places of the kernel that are written in assembly run their C++ restatements (the step
// loop of dijkstra, kbest_lap.h; the lane masks of the first-step filter).  The launches are issued as batch_dev_impl
// (kbest_capi.cpp) issues them for the 64-row route -- launch_kbest, launch_merge_topk behind an internal split,
// launch_finish_tables in tie mode, launch_fill_unused -- on exact-size heap blocks: the state work space with its slot table
// (engine_states_need), every output table, gain, nf, tieGain, the tie flags, pushed, dualU / dualV, the split buffer (SplitLayout),
// the relay images (relay_image_bytes) and each workgroup's LDS -- all PREFILLED with what the fill selector says: a device
// clears none of them, so an index that is read before it is written shows either under AddressSanitizer or as an answer that
// changes with the fill.
// TWO things are exempt from the fill, because the host entry really initialises them: sharedT (the thresholds of a split launch)
// is 0xFF as the entry's memset leaves it, and the three relay words per matrix are zero (relay_reserve zeroes them once; the last
// workgroup of a matrix to leave puts them back).
// Built with -fsanitize=address,undefined (tests/test_engine_cpu.py); nothing is loaded into python.
// usage: engine_host IN OUT
//   IN:  int h[32]: mode, then per mode.  double d[8].
//   mode 0 (k-best): h = mode, B, maxRow, maxCol, hasShapes, k, tie, spec, waves, maximize, useCutoff, flags, rootColOffset,
//        rootColStride, fill, seed, extraStates, eagerStates, split, relayP, relayFirst, relayStep, optMinPool, gainCols, wantDuals,
//        tablesHost, wantPushed; d = cutoff, optRho0, optRho1, optSlope, optKappa.  hasShapes: int nRow[B], nCol[B]; double
//        cost[B][maxRow * maxCol] (problem b: nRow x nCol column-major from b * maxRow * maxCol).  k: slots of the tables; tie = 1:
//        the kernel enumerates k + 1 (kbest_ties.h) and the finishing kernel runs.  fill: 1 = 0x00, 2 = 0xFF, 3 = seeded bytes.
//   OUT: int statesPerProblem, lazyStates, atomSlots, maxSid (both for maxRow rows), ldsBytes, kernelK, launchStatus, relayImage;
//        per problem int nf, tieFlags; long long pushed; double tieGain, gain[k]; int row4col[k][maxCol], col4row[k][maxRow];
//        per workgroup (B * split) int nf, slotSid[k]; wantDuals: double dualU[B][maxCol], dualV[B][maxRow]; relayP > 1: unsigned
//        flag[B], claim[B], gone[B]
//   mode 1 (condition_kernel): h = mode, B, maxRow, fill, seed; int nRow[B], nCol[B]; long long costOff[B]; double cost[total]
//   OUT: int goodRows[B], condL[B], rowIdx[B][maxRow]; double out[total]
//   mode 2 (weights_kernel): h = mode, B, k, maxCol, maxRow, gate, solveRows, kUse, hasRowIdx, fill, seed, totalCost, totalProbs;
//        int nL[B], nM[B], nf[B]; long long costOff[B], probOff[B]; double cost[totalCost], gain[B][k]; int row4col[B][k][maxCol];
//        hasRowIdx: int rowIdx[B][maxRow], nLout[B]
//   OUT: int chunk, ldsAcc, nf[B]; double probs[totalProbs]
#include <algorithm>

#include "hip_on_host.h"
#include "kbest_engine.hip"
#include "kbest_merge.hip"

#ifndef ENGINE_HOST_MUTANT
#define ENGINE_HOST_MUTANT 0  // tests/test_engine_cpu.py builds the mutants from patched copies of the kernel's text; this only names the build
#endif

template <class T>
static T *block(size_t n, int fill, unsigned long long seed)
{
    T *p = reinterpret_cast<T *>(new unsigned char[n * sizeof(T)]);
    emu_fill_bytes(reinterpret_cast<unsigned char *>(p), n * sizeof(T), fill, seed);
    return p;
}
template <class T>
static void drop(T *p) { delete[] reinterpret_cast<unsigned char *>(p); }
template <class T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static int run_kbest(const int *h, const double *d, FILE *f, const char *outName)
{
    const int B = h[1], maxRow = h[2], maxCol = h[3], hasShapes = h[4], kT = h[5], tie = h[6], spec = h[7], waves = h[8];
    const unsigned flags = (unsigned)h[11];
    const int fill = h[14];
    const unsigned long long seed = (unsigned)h[15];
    const int extraStates = h[16], eager = h[17], S = h[18] > 1 ? h[18] : 1, relayP = h[19];
    const bool wantDuals = h[24] != 0, wantPushed = h[26] != 0;
    const bool i8 = (flags & KBEST_FLAG_TABLES_I8) != 0;
    std::vector<int> nRow(B), nCol(B);
    if (hasShapes && (!get(f, nRow.data(), B) || !get(f, nCol.data(), B))) return 2;
    const size_t nCost = (size_t)B * maxRow * maxCol;
    double *cost = block<double>(nCost, 0, 0);
    if (!get(f, cost, nCost)) return 2;
    const int k = tie ? kT + 1 : kT;  // kernel-side
    const int PB = B * S;              // workgroups = problems of the launch as the kernel sees them
    // exact-size heap blocks, prefilled
    size_t slotOff = 0;
    const size_t wsBytes = kb::engine_states_need(PB, maxRow, k, extraStates, eager, &slotOff);
    const size_t esz = i8 ? 1 : 4;
    const size_t r4cBytes = (size_t)B * kT * maxCol * esz, c4rBytes = (size_t)B * kT * maxRow * esz;
    unsigned char *ws = block<unsigned char>(wsBytes, fill, seed + 101);
    unsigned char *r4c = block<unsigned char>(r4cBytes, fill, seed + 102), *c4r = block<unsigned char>(c4rBytes, fill, seed + 103);
    double *gain = block<double>((size_t)B * kT, fill, seed + 104), *tieGain = block<double>(B, fill, seed + 105);
    int *nf = block<int>(B, fill, seed + 106), *tieFlags = block<int>(B, fill, seed + 107);
    long long *pushed = block<long long>(B, fill, seed + 108);
    double *dualU = block<double>((size_t)B * maxCol, fill, seed + 109), *dualV = block<double>((size_t)B * maxRow, fill, seed + 110);
    const kb::SplitLayout sl(B, S, k, maxCol);
    unsigned char *sb = block<unsigned char>(S > 1 ? sl.bytes : 0, fill, seed + 111);
    if (S > 1) memset(sb + sl.offT, 0xFF, (size_t)B * 8);  // no threshold yet: the entry's memset
    const kb::Lds L = kb::lds_layout(maxRow, k, spec, waves);
    const size_t relayImg = kb::relay_image_bytes(L.total), relayWords = kb::relay_words_bytes(B);
    unsigned char *relayBuf = block<unsigned char>(relayP > 1 ? (size_t)B * relayImg : 0, fill, seed + 112);
    unsigned *relayFlag = block<unsigned>(relayP > 1 ? relayWords / 4 : 0, 1, 0);  // zero: relay_reserve
    emuLdsFill = fill;
    emuLdsSeed = seed + 1000;
    // the launch of batch_dev_impl (kbest_capi.cpp), one piece: base = 0, LB = B
    kb::Params p;
    memset(&p, 0, sizeof(p));
    p.cost = cost;
    p.nRow = hasShapes ? nRow.data() : nullptr;
    p.nCol = hasShapes ? nCol.data() : nullptr;
    p.maxRow = maxRow;
    p.maxCol = maxCol;
    p.ldRow = maxRow;
    p.ldCol = maxCol;
    p.k = k;
    p.maximize = h[9];
    p.useCutoff = h[10];
    p.flags = flags;
    p.cutoff = d[0];
    p.rootColOffset = h[12];
    p.rootColStride = h[13];
    p.row4col = S > 1 ? reinterpret_cast<int *>(sb + sl.offR4C) : reinterpret_cast<int *>(r4c);
    p.col4row = S > 1 ? nullptr : reinterpret_cast<int *>(c4r);
    p.gain = S > 1 ? reinterpret_cast<double *>(sb + sl.offGain) : gain;
    p.nf = S > 1 ? reinterpret_cast<int *>(sb + sl.offNf) : nf;
    p.pushed = wantPushed ? pushed : nullptr;
    p.stateStride = kb::state_stride(maxRow);
    p.statesPerProblem = kb::engine_states_per_problem(k, extraStates, eager);
    p.states = ws;
    p.lazyStates = k + extraStates;
    p.spec = spec;
    p.slotSid = reinterpret_cast<unsigned short *>(ws + slotOff);
    p.dualU = wantDuals ? dualU : nullptr;
    p.dualV = wantDuals ? dualV : nullptr;
    p.gainCols = h[23];
    p.kTab = kT;
    p.tieGain = tie ? tieGain : nullptr;
    p.split = S;
    p.splitB = B;
    p.sharedT = S > 1 ? reinterpret_cast<unsigned long long *>(sb + sl.offT) : nullptr;
    p.tablesHost = h[25];
    p.optRho0 = (float)d[1];
    p.optRho1 = (float)d[2];
    p.optSlope = (float)d[3];
    p.optKappa = d[4];
    p.optMinPool = h[22];
    if (relayP > 1) {
        p.relayP = relayP;
        p.relayB = B;
        p.relayFirst = h[20];
        p.relayStep = h[21];
        p.relayBuf = relayBuf;
        p.relayStride = (long long)relayImg;
        p.relayFlag = relayFlag;
        p.relayClaim = p.relayFlag + relayWords / 16;  // (quarters of the buffer)
        p.relayGone = p.relayFlag + relayWords / 8;
    }
    int status = kb::launch_kbest(p, PB, waves, nullptr);
    if (status == hipSuccess && S > 1) {  // the global k best of every matrix from its shares' lists
        kb::MergeParams mp;
        memset(&mp, 0, sizeof(mp));
        mp.gain = sb + sl.offGain;
        mp.row4col = sb + sl.offR4C;
        mp.nf = sb + sl.offNf;
        mp.shardStride = (long long)B * k * 8;
        mp.strideR4C = (long long)B * k * maxCol * 4;
        mp.strideNf = (long long)B * 4;
        mp.nShard = S;
        mp.k = k;
        mp.maxCol = maxCol;
        mp.ldCol = maxCol;
        mp.maximize = h[9];
        mp.outGain = gain;
        mp.outRow4col = reinterpret_cast<int *>(r4c);
        mp.outNf = nf;
        mp.outCol4row = reinterpret_cast<int *>(c4r);
        mp.ldRow = maxRow;
        status = kb::launch_merge_topk(mp, B, nullptr);
    }
    if (status == hipSuccess && tie)
        status = kb::launch_finish_tables(nf, p.nRow, p.nCol, B, kT, maxCol, maxRow, reinterpret_cast<int *>(r4c), reinterpret_cast<int *>(c4r), gain, i8,
                                          tieGain, tieFlags, false, nullptr, 0, !h[25]);
    if (status == hipSuccess)
        status = kb::launch_fill_unused(nf, p.nRow, p.nCol, B, kT, maxCol, maxRow, reinterpret_cast<int *>(r4c), reinterpret_cast<int *>(c4r), gain, i8,
                                        nullptr);
    fclose(f);
    f = fopen(outName, "wb");
    if (!f) return 2;
    const int atomSlots = (kb::t0_area_bytes(maxRow) + (int)p.stateStride - 1) / (int)p.stateStride;
    const int maxSid = p.statesPerProblem - atomSlots > p.lazyStates ? p.statesPerProblem - atomSlots : p.statesPerProblem;
    const int head[8] = {p.statesPerProblem, p.lazyStates, atomSlots, maxSid, L.total, k, status, (int)relayImg};
    fwrite(head, 4, 8, f);
    const long long sst = kb::slot_table_stride(k);
    for (int b = 0; b < B; b++) {
        const int two[2] = {nf[b], tie ? tieFlags[b] : 0};
        fwrite(two, 4, 2, f);
        const long long pu = wantPushed ? pushed[b] : 0;
        fwrite(&pu, 8, 1, f);
        fwrite(&tieGain[b], 8, 1, f);
        fwrite(gain + (size_t)b * kT, 8, kT, f);
        for (size_t i = 0; i < (size_t)kT * maxCol; i++) {
            const size_t at = (size_t)b * kT * maxCol + i;
            const int v = i8 ? (int)reinterpret_cast<signed char *>(r4c)[at] : reinterpret_cast<int *>(r4c)[at];
            fwrite(&v, 4, 1, f);
        }
        for (size_t i = 0; i < (size_t)kT * maxRow; i++) {
            const size_t at = (size_t)b * kT * maxRow + i;
            const int v = i8 ? (int)reinterpret_cast<signed char *>(c4r)[at] : reinterpret_cast<int *>(c4r)[at];
            fwrite(&v, 4, 1, f);
        }
    }
    for (int w = 0; w < PB; w++) {
        fwrite(&p.nf[w], 4, 1, f);
        for (int s = 0; s < kT; s++) {
            const int v = p.slotSid[w * sst + s];
            fwrite(&v, 4, 1, f);
        }
    }
    if (wantDuals) {
        fwrite(dualU, 8, (size_t)B * maxCol, f);
        fwrite(dualV, 8, (size_t)B * maxRow, f);
    }
    if (relayP > 1) {
        fwrite(p.relayFlag, 4, B, f);
        fwrite(p.relayClaim, 4, B, f);
        fwrite(p.relayGone, 4, B, f);
    }
    fclose(f);
    drop(ws); drop(r4c); drop(c4r); drop(gain); drop(tieGain); drop(nf); drop(tieFlags); drop(pushed); drop(dualU); drop(dualV); drop(sb);
    drop(relayBuf); drop(relayFlag); drop(cost);
    return 0;
}

static int run_condition(const int *h, FILE *f, const char *outName)
{
    const int B = h[1], maxRow = h[2], fill = h[3];
    const unsigned long long seed = (unsigned)h[4];
    std::vector<int> nRow(B), nCol(B);
    std::vector<long long> off(B);
    if (!get(f, nRow.data(), B) || !get(f, nCol.data(), B) || !get(f, off.data(), B)) return 2;
    size_t total = 0;
    for (int b = 0; b < B; b++) total = std::max(total, (size_t)off[b] + (size_t)nRow[b] * nCol[b]);
    double *cost = block<double>(total, 0, 0), *out = block<double>(total, fill, seed + 201);
    if (!get(f, cost, total)) return 2;
    int *good = block<int>(B, fill, seed + 202), *condL = block<int>(B, fill, seed + 203), *ridx = block<int>((size_t)B * maxRow, fill, seed + 204);
    kb::CondParams p;
    memset(&p, 0, sizeof(p));
    p.cost = cost;
    p.costOff = off.data();
    p.nRow = nRow.data();
    p.nCol = nCol.data();
    p.out = out;
    p.goodRows = good;
    p.condL = condL;
    p.rowIdx = ridx;
    p.maxRow = maxRow;
    if (kb::launch_condition(p, B, nullptr) != hipSuccess) return 3;
    fclose(f);
    f = fopen(outName, "wb");
    if (!f) return 2;
    fwrite(good, 4, B, f);
    fwrite(condL, 4, B, f);
    fwrite(ridx, 4, (size_t)B * maxRow, f);
    fwrite(out, 8, total, f);
    fclose(f);
    drop(cost); drop(out); drop(good); drop(condL); drop(ridx);
    return 0;
}

static int run_weights(const int *h, FILE *f, const char *outName)
{
    const int B = h[1], k = h[2], maxCol = h[3], maxRow = h[4], hasRowIdx = h[8], fill = h[9];
    const unsigned long long seed = (unsigned)h[10];
    const size_t totalCost = (size_t)h[11], totalProbs = (size_t)h[12];
    std::vector<int> nL(B), nM(B), nLout(B);
    std::vector<long long> costOff(B), probOff(B);
    int *nf = block<int>(B, 0, 0);
    if (!get(f, nL.data(), B) || !get(f, nM.data(), B) || !get(f, nf, B) || !get(f, costOff.data(), B) || !get(f, probOff.data(), B)) return 2;
    double *cost = block<double>(totalCost, 0, 0), *gain = block<double>((size_t)B * k, 0, 0);
    int *r4c = block<int>((size_t)B * k * maxCol, 0, 0), *ridx = block<int>(hasRowIdx ? (size_t)B * maxRow : 0, 0, 0);
    if (!get(f, cost, totalCost) || !get(f, gain, (size_t)B * k) || !get(f, r4c, (size_t)B * k * maxCol)) return 2;
    if (hasRowIdx && (!get(f, ridx, (size_t)B * maxRow) || !get(f, nLout.data(), B))) return 2;
    double *probs = block<double>(totalProbs, fill, seed + 301);
    emuLdsFill = fill;
    emuLdsSeed = seed + 2000;
    kb::WeightParams p;
    memset(&p, 0, sizeof(p));
    p.nL = nL.data();
    p.nM = nM.data();
    p.cost = cost;
    p.costOff = costOff.data();
    p.gain = gain;
    p.row4col = r4c;
    p.nf = nf;
    p.probs = probs;
    p.probOff = probOff.data();
    p.k = k;
    p.maxCol = maxCol;
    p.rowIdx = hasRowIdx ? ridx : nullptr;
    p.nLout = hasRowIdx ? nLout.data() : nullptr;
    p.maxRow = maxRow;
    p.gate = h[5];
    p.solveRows = h[6];
    p.kUse = h[7];
    if (kb::launch_weights(p, B, nullptr) != hipSuccess) return 3;
    const kb::WeightsLds wl = kb::weights_lds_plan(maxCol, p.solveRows);  // (what launch_weights set in its copy of the arguments)
    const int two[2] = {wl.chunk, wl.ldsAcc};
    fclose(f);
    f = fopen(outName, "wb");
    if (!f) return 2;
    fwrite(two, 4, 2, f);
    fwrite(nf, 4, B, f);
    fwrite(probs, 8, totalProbs, f);
    fclose(f);
    drop(nf); drop(cost); drop(gain); drop(r4c); drop(ridx); drop(probs);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h[32];
    double d[8];
    if (fread(h, 4, 32, f) != 32 || fread(d, 8, 8, f) != 8) return 2;
    int rc = 2;
    if (h[0] == 0) rc = run_kbest(h, d, f, argv[2]);
    else if (h[0] == 1) rc = run_condition(h, f, argv[2]);
    else if (h[0] == 2) rc = run_weights(h, f, argv[2]);
    return rc;
}

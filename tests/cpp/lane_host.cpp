// kbest_lane.hip and the launch behind it (finish_tables_kernel, kbest_merge.hip with kbest_ties.h) compiled for the HOST, line for
// line: a workgroup is waves * 64 std::threads, __syncthreads a std::barrier, every wave operation an exchange through the wave's
// barrier with the lane semantics of gfx950 (hip_on_host.h).  The three places of the kernel that are written in assembly run their
// C++ restatements (lane_row; the step loop of dijkstra, kbest_lap.h).  The pair is launched as kbest_capi.cpp issues it, on
// exact-size heap blocks -- the work space (saved hypotheses, slot table, the spare bytes: lane_states_need), every output table, each
// workgroup's LDS -- all PREFILLED with what the fill selector says: a device clears none of them, so an index that is read before
// it is written shows either under AddressSanitizer or as an answer that changes with the fill.
// Built with -fsanitize=address,undefined (tests/test_lane_cpu.py) or -fsanitize=thread; nothing is loaded into python.
// usage: lane_host IN OUT
//   IN:  int B, maxRow, maxCol, hasShapes, k, tie, spec, waves, maximize, useCutoff, flags, rootColOffset, rootColStride, fill, seed,
//        0; double cutoff; hasShapes: int nRow[B], nCol[B]; double cost[B][maxRow * maxCol] (problem b: nRow x nCol column-major
//        from b * maxRow * maxCol).  k: slots of the tables; tie = 1: the kernel enumerates k + 1 (kbest_ties.h) and the finishing
//        kernel runs.  fill: 1 = 0x00, 2 = 0xFF, 3 = bytes of a generator seeded with `seed`.
//   OUT: int statesPerProblem, offFreshG, offFree, ldsBytes, kernelK, launchStatus; per problem int nf, tieFlags; double tieGain,
//        gain[k]; int row4col[k][maxCol], col4row[k][maxRow], slotSid[k]
#include "hip_on_host.h"
#include "kbest_lane.hip"
#include "kbest_merge.hip"

#ifndef LANE_HOST_MUTANT
#define LANE_HOST_MUTANT 0  // tests/test_lane_cpu.py builds the mutants from patched copies of the kernel's text; this only names the build
#endif

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int h[16];
    double cutoff;
    if (fread(h, 4, 16, f) != 16 || fread(&cutoff, 8, 1, f) != 1) return 2;
    const int B = h[0], maxRow = h[1], maxCol = h[2], hasShapes = h[3], kT = h[4], tie = h[5], spec = h[6], waves = h[7];
    const int fill = h[13];
    const unsigned long long seed = (unsigned)h[14];
    const unsigned flags = (unsigned)h[10];
    const bool i8 = (flags & KBEST_FLAG_TABLES_I8) != 0;
    std::vector<int> nRow(B), nCol(B);
    if (hasShapes && (fread(nRow.data(), 4, B, f) != (size_t)B || fread(nCol.data(), 4, B, f) != (size_t)B)) return 2;
    const size_t nCost = (size_t)B * maxRow * maxCol;
    double *cost = new double[nCost];
    if (fread(cost, 8, nCost, f) != nCost) return 2;
    fclose(f);
    const int k = tie ? kT + 1 : kT;  // kernel-side
    // exact-size heap blocks, prefilled
    size_t slotOff = 0;
    const size_t wsBytes = kb::lane_states_need(B, maxRow, maxCol, k, spec, &slotOff);
    const size_t esz = i8 ? 1 : 4;
    const size_t r4cBytes = (size_t)B * kT * maxCol * esz, c4rBytes = (size_t)B * kT * maxRow * esz;
    unsigned char *ws = new unsigned char[wsBytes];
    unsigned char *r4c = new unsigned char[r4cBytes], *c4r = new unsigned char[c4rBytes];
    double *gain = new double[(size_t)B * kT], *tieGain = new double[B];
    int *nf = new int[B], *tieFlags = new int[B];
    emu_fill_bytes(ws, wsBytes, fill, seed + 101);
    emu_fill_bytes(r4c, r4cBytes, fill, seed + 102);
    emu_fill_bytes(c4r, c4rBytes, fill, seed + 103);
    emu_fill_bytes(reinterpret_cast<unsigned char *>(gain), (size_t)B * kT * 8, fill, seed + 104);
    emu_fill_bytes(reinterpret_cast<unsigned char *>(tieGain), (size_t)B * 8, fill, seed + 105);
    emu_fill_bytes(reinterpret_cast<unsigned char *>(nf), (size_t)B * 4, fill, seed + 106);
    emu_fill_bytes(reinterpret_cast<unsigned char *>(tieFlags), (size_t)B * 4, fill, seed + 107);
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
    p.maximize = h[8];
    p.useCutoff = h[9];
    p.flags = flags;
    p.cutoff = cutoff;
    p.rootColOffset = h[11];
    p.rootColStride = h[12];
    p.row4col = reinterpret_cast<int *>(r4c);
    p.col4row = reinterpret_cast<int *>(c4r);
    p.gain = gain;
    p.nf = nf;
    p.stateStride = kb::lane_state_stride(maxRow);
    p.statesPerProblem = kb::lane_states_per_problem(k, spec, maxCol);
    p.states = ws;
    p.lazyStates = p.statesPerProblem;
    p.spec = spec;
    p.slotSid = reinterpret_cast<unsigned short *>(ws + slotOff);
    p.kTab = kT;
    p.tieGain = tie ? tieGain : nullptr;
    int status = kb::launch_kbest_lane(p, B, waves, 4, nullptr);
    if (status == hipSuccess && tie)
        status = kb::launch_finish_tables(nf, p.nRow, p.nCol, B, kT, maxCol, maxRow, p.row4col, p.col4row, gain, i8, tieGain, tieFlags, false, nullptr, 0, true);
    const kb::LaneLds L = kb::lane_lds_layout(maxRow, maxCol, k, spec, waves, 4);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int head[6] = {p.statesPerProblem, L.offFreshG, L.offFree, L.total, k, status};
    fwrite(head, 4, 6, f);
    const long long sst = kb::slot_table_stride(k);
    for (int b = 0; b < B; b++) {
        const int two[2] = {nf[b], tie ? tieFlags[b] : 0};
        fwrite(two, 4, 2, f);
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
        for (int s = 0; s < kT; s++) {
            const int v = p.slotSid[b * sst + s];
            fwrite(&v, 4, 1, f);
        }
    }
    fclose(f);
    delete[] ws; delete[] r4c; delete[] c4r; delete[] gain; delete[] tieGain; delete[] nf; delete[] tieFlags; delete[] cost;
    return 0;
}

// kbest_sample.hip compiled for the HOST, line for line: a workgroup is perm_threads(maxCol) std::threads, __syncthreads a
// std::barrier, the wave operations (ballot, the wave minimum) go through per-wave barriers.  Built with
// -fsanitize=address,undefined and run on exact-size heap buffers -- the LDS plan, the work space, every output -- it checks what a
// GPU run cannot show without risk: that no step reads or writes beyond them.  tests/test_sample_cpu.py builds and runs it and
// compares the draws with tests/sample_check.py.
// usage: sample_host IN OUT
//   IN: int n, mode, nSample, condition, grid; u32 sampleBase; u64 seed; per frame int nL, nM; u64 key; the (nL + nM) * nM doubles
//   OUT: per frame double perm; int assign[nSample][nM]; double logProb[nSample]   (prefilled: -7 / -7.0)
#include "hip_on_host.h"
#include "kbest_sample.hip"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[5];
    u32 sampleBase;
    u64 seed;
    if (fread(hdr, 4, 5, f) != 5 || fread(&sampleBase, 4, 1, f) != 1 || fread(&seed, 8, 1, f) != 1) return 2;
    const int n = hdr[0], mode = hdr[1], nSample = hdr[2], condition = hdr[3], grid = hdr[4];
    std::vector<int> nL(n), nM(n);
    std::vector<u64> key(n);
    std::vector<long long> costOff(n), asgOff(n), lpOff(n);
    std::vector<double> cost;
    size_t asgN = 0;
    int maxRawRow = 1, maxCol = 1;
    for (int b = 0; b < n; b++) {
        if (fread(&nL[b], 4, 1, f) != 1 || fread(&nM[b], 4, 1, f) != 1 || fread(&key[b], 8, 1, f) != 1) return 2;
        const size_t sz = (size_t)(nL[b] + nM[b]) * nM[b];
        costOff[b] = (long long)cost.size();
        cost.resize(cost.size() + sz);
        if (fread(cost.data() + costOff[b], 8, sz, f) != sz) return 2;
        asgOff[b] = (long long)asgN;
        lpOff[b] = (long long)b * nSample;
        asgN += (size_t)nSample * nM[b];
        if (nL[b] + nM[b] > maxRawRow) maxRawRow = nL[b] + nM[b];
        if (nM[b] > maxCol) maxCol = nM[b];
    }
    fclose(f);
    // exact-size heap buffers: AddressSanitizer sees any access beyond the plan, a slot or an output
    kb::PermPlan pl;
    pl.mode = mode;
    pl.threads = kb::perm_threads(maxCol);
    pl.lds = kb::perm_lds(mode, maxRawRow, maxCol).total;
    pl.slotDoubles = mode == 0 ? 0 : (long long)maxRawRow * maxCol + ((long long)(maxRawRow + 2) << maxCol);  // perm_plan's
    std::vector<int> assign(asgN, -7);
    std::vector<double> logProb((size_t)n * nSample, -7.0), perm(n, -7.0);
    double *work = new double[(size_t)pl.slotDoubles * grid];
    kb::SampleParams sp;
    sp.cost = cost.data(); sp.costOff = costOff.data(); sp.nL = nL.data(); sp.nM = nM.data(); sp.frameKey = key.data();
    sp.assign = assign.data(); sp.asgOff = asgOff.data(); sp.logProb = logProb.data(); sp.lpOff = lpOff.data(); sp.perm = perm.data();
    sp.work = work; sp.slotStride = pl.slotDoubles; sp.seed = seed; sp.sampleBase = sampleBase; sp.nSample = nSample;
    sp.B = n; sp.maxRawRow = maxRawRow; sp.maxCol = maxCol; sp.condition = condition;
    kb::launch_kbest_sample(sp, pl, grid, nullptr);
    f = fopen(argv[2], "wb");
    for (int b = 0; b < n; b++) {
        fwrite(&perm[b], 8, 1, f);
        fwrite(assign.data() + asgOff[b], 4, (size_t)nSample * nM[b], f);
        fwrite(logProb.data() + lpOff[b], 8, (size_t)nSample, f);
    }
    fclose(f);
    delete[] work;
    return 0;
}

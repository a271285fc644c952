// kbest_frontier.hip compiled for the HOST, line for line: a workgroup is 256 std::threads, __syncthreads a std::barrier, the wave
// operations (ballot, the DPP butterfly, the wave minimum) go through per-wave barriers with the lane semantics of gfx950.  Built
// with -fsanitize=address,undefined and run on exact-size heap buffers, it checks what a GPU run cannot show without risk: that
// no step reads or writes beyond its slot, its plan or its outputs.  tests/test_frontier_cpu.py builds and runs it.
// usage: frontier_host IN OUT [slotDoubles [grid]]
//   IN: int n; per cluster int m, nL and the (nL + m) * m doubles of its sub-block.
//   OUT: per cluster int info, width; double logZ; the m * (nL + 1) doubles of its probabilities (-5: untouched)
#include "hip_on_host.h"
#include "kbest_frontier.hip"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int n;
    if (fread(&n, 4, 1, f) != 1) return 2;
    const long long slotDoubles = argc > 3 ? atoll(argv[3]) : (4 << 20) / 8;
    const int grid = argc > 4 ? atoi(argv[4]) : 2;
    kb::FrontierPack pk;
    std::vector<double> sub, probs;
    int maxRows = 1;
    pk.n = n; pk.base = 0;
    for (int k = 0; k < n; k++) {
        int m, nL;
        if (fread(&m, 4, 1, f) != 1 || fread(&nL, 4, 1, f) != 1) return 2;
        const size_t sz = (size_t)(nL + m) * m;
        pk.c[k].subOff = (long long)sub.size(); pk.c[k].probOff = (long long)probs.size(); pk.c[k].m = m; pk.c[k].nL = nL;
        sub.resize(sub.size() + sz);
        if (fread(sub.data() + pk.c[k].subOff, 8, sz, f) != sz) return 2;
        probs.resize(probs.size() + (size_t)m * (nL + 1), -5.0);
        if (nL + m > maxRows) maxRows = nL + m;
    }
    fclose(f);
    // exact-size heap buffers: AddressSanitizer sees any access beyond a slot or a plan
    std::vector<double> logZ(n, -5.0);
    std::vector<int> info(n, -77), width(n, -77);
    kb::FrontierWork w;
    w.slotDoubles = slotDoubles; w.planDoubles = (long long)maxRows * kb::KB_FRONTIER_STEP_DOUBLES;
    double *layers = new double[(size_t)w.slotDoubles * grid], *plan = new double[(size_t)w.planDoubles * grid];
    w.layers = layers; w.plan = plan;
    kb::launch_frontier_pack(pk, sub.data(), probs.data(), logZ.data(), info.data(), width.data(), w, grid, nullptr);
    f = fopen(argv[2], "wb");
    for (int k = 0; k < n; k++) {
        fwrite(&info[k], 4, 1, f); fwrite(&width[k], 4, 1, f); fwrite(&logZ[k], 8, 1, f);
        fwrite(probs.data() + pk.c[k].probOff, 8, (size_t)pk.c[k].m * (pk.c[k].nL + 1), f);
    }
    fclose(f);
    delete[] layers; delete[] plan;
    return 0;
}

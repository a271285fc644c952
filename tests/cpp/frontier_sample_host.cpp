// kbest_frontier_sample.hip compiled for the HOST, line for line, as tests/cpp/frontier_host.cpp compiles kbest_frontier.hip: a
// workgroup is 256 std::threads, __syncthreads a std::barrier, the wave operations go through per-wave barriers with the lane
// semantics of gfx950.  Built with -fsanitize=address,undefined and run on exact-size heap buffers, it checks what a GPU run cannot
// show without risk: that neither the sweep nor the walk reads or writes beyond the slot, the plan, the row keys or the outputs.
// tests/test_frontier_sample_cpu.py builds and runs it.
// usage: frontier_sample_host IN OUT [slotDoubles [grid]]
//   IN: int n, nSample; u64 seed; u32 sampleBase, pad; per cluster int m, nL; u64 frameKey; the (nL + m) * m doubles of its
//       sub-block; the nL + m int32 keys of its rows.
//   OUT: per cluster int info, width; double logZ; nSample * m int32 (assignLocal, -5: untouched); nSample doubles (logTerm, -5.0)
#include "hip_on_host.h"
#include "kbest_frontier_sample.hip"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int n, nSample;
    u64 seed;
    u32 base[2];
    if (fread(&n, 4, 1, f) != 1 || fread(&nSample, 4, 1, f) != 1 || fread(&seed, 8, 1, f) != 1 || fread(base, 4, 2, f) != 2) return 2;
    const long long slotDoubles = argc > 3 ? atoll(argv[3]) : (4 << 20) / 8;
    const int grid = argc > 4 ? atoi(argv[4]) : 2;
    if (n > kb::KB_FRONTIER_SAMPLE_PACK) return 2;
    kb::FrontierSamplePack pk;
    std::vector<double> sub;
    std::vector<int> keys;
    long long asgN = 0;
    int maxRows = 1;
    pk.n = n; pk.base = 0;
    for (int k = 0; k < n; k++) {
        int m, nL;
        u64 fk;
        if (fread(&m, 4, 1, f) != 1 || fread(&nL, 4, 1, f) != 1 || fread(&fk, 8, 1, f) != 1) return 2;
        const size_t sz = (size_t)(nL + m) * m;
        pk.c[k].subOff = (long long)sub.size(); pk.c[k].rowKeyOff = (long long)keys.size(); pk.c[k].asgOff = asgN;
        pk.c[k].ltOff = (long long)k * nSample; pk.c[k].frameKey = fk; pk.c[k].m = m; pk.c[k].nL = nL;
        sub.resize(sub.size() + sz);
        if (fread(sub.data() + pk.c[k].subOff, 8, sz, f) != sz) return 2;
        keys.resize(keys.size() + nL + m);
        if (fread(keys.data() + pk.c[k].rowKeyOff, 4, nL + m, f) != (size_t)(nL + m)) return 2;
        asgN += (long long)nSample * m;
        if (nL + m > maxRows) maxRows = nL + m;
    }
    fclose(f);
    // exact-size heap buffers: AddressSanitizer sees any access beyond a slot, a plan, the keys or a cluster's draws
    std::vector<double> logZ(n, -5.0), lt((size_t)n * nSample, -5.0);
    std::vector<int> info(n, -77), width(n, -77), asg((size_t)asgN, -5);
    kb::FrontierWork w;
    w.slotDoubles = slotDoubles; w.planDoubles = (long long)maxRows * kb::KB_FRONTIER_STEP_DOUBLES;
    double *layers = new double[(size_t)w.slotDoubles * grid], *plan = new double[(size_t)w.planDoubles * grid];
    w.layers = layers; w.plan = plan;
    kb::launch_frontier_sample_pack(pk, sub.data(), keys.data(), nSample, seed, base[0], asg.data(), lt.data(), logZ.data(), info.data(),
                                    width.data(), w, grid, nullptr);
    f = fopen(argv[2], "wb");
    for (int k = 0; k < n; k++) {
        fwrite(&info[k], 4, 1, f); fwrite(&width[k], 4, 1, f); fwrite(&logZ[k], 8, 1, f);
        fwrite(asg.data() + pk.c[k].asgOff, 4, (size_t)nSample * pk.c[k].m, f);
        fwrite(lt.data() + pk.c[k].ltOff, 8, nSample, f);
    }
    fclose(f);
    delete[] layers; delete[] plan;
    return 0;
}

// A caller of hybridFrontierSampleAssoc written like the reference's call sites of permanentProb, compiled against
// include/kbest_shims.hpp and linked to libkbest_amd.so.
// usage: shim_frontier_sample FILE NSAMPLE SEED   -- FILE: "nL nM" and then the (nL+nM)*nM column-major costs as C99 hex floats ("inf" allowed)
// prints one line "s <draw> <nM rows>" per draw; then what a frame without any consistent association does.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <vector>

#include "kbest_shims.hpp"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long nL = 0, nM = 0;
    if (fscanf(f, "%lu %lu", &nL, &nM) != 2) return 2;
    std::vector<double> cost((nL + nM) * nM);
    char tok[64];
    for (double &x : cost) {
        if (fscanf(f, "%63s", tok) != 1) return 2;
        x = strtod(tok, nullptr);
    }
    fclose(f);
    const size_t nSample = strtoul(argv[2], nullptr, 10);
    const std::vector<std::vector<int>> draws = hybridFrontierSampleAssoc(cost, nL, nM, nSample, strtoull(argv[3], nullptr, 10));
    if (draws.size() != nSample) return 3;
    for (size_t s = 0; s < nSample; s++) {
        if (draws[s].size() != nM) return 3;
        printf("s %zu", s);
        for (int r : draws[s]) printf(" %d", r);
        printf("\n");
    }
    for (size_t r = 0; r < nL + nM; r++) cost[r] = std::numeric_limits<double>::infinity();  // column 0 without a finite entry
    try {
        hybridFrontierSampleAssoc(cost, nL, nM, 1, 0);
        printf("empty column: no throw\n");
    } catch (const std::runtime_error &e) {
        printf("empty column: runtime_error %s\n", e.what());
    }
    return 0;
}

// A caller of hybridSampleAssoc written like the reference's call sites of assignmentProb, compiled against
// include/kbest_shims.hpp and linked to libkbest_amd.so.
// usage: shim_table_sample FILE NSAMPLE K SEED   -- FILE: "nL nM" and then the (nL+nM)*nM column-major costs as C99 hex floats ("inf" allowed)
// prints one line "s <draw> <nM rows>" per draw; then what k = 0 does on the same frame, and what a frame without any consistent
// association does.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <vector>

#include "kbest_shims.hpp"

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
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
    const size_t nSample = strtoul(argv[2], nullptr, 10), k = strtoul(argv[3], nullptr, 10);
    const std::vector<std::vector<int>> draws = hybridSampleAssoc(cost, nL, nM, nSample, k, strtoull(argv[4], nullptr, 10));
    if (draws.size() != nSample) return 3;
    for (size_t s = 0; s < nSample; s++) {
        if (draws[s].size() != nM) return 3;
        printf("s %zu", s);
        for (int r : draws[s]) printf(" %d", r);
        printf("\n");
    }
    try {
        hybridSampleAssoc(cost, nL, nM, 1, 0);
        printf("k = 0: no throw\n");
    } catch (const std::runtime_error &e) {
        printf("k = 0: runtime_error %s\n", e.what());
    }
    // column 0 without a finite entry (and its miss row nL without one: no other cluster keeps a row >= nL too many)
    for (size_t r = 0; r < nL + nM; r++) cost[r] = std::numeric_limits<double>::infinity();
    for (size_t c = 0; c < nM; c++) cost[c * (nL + nM) + nL] = std::numeric_limits<double>::infinity();
    try {
        hybridSampleAssoc(cost, nL, nM, 1, k);
        printf("empty column: no throw\n");
    } catch (const std::runtime_error &e) {
        printf("empty column: runtime_error %s\n", e.what());
    }
    return 0;
}

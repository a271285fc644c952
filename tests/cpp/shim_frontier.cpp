// A caller of hybridFrontierProb written like the reference's call sites of assignmentProb / permanentProb, compiled against
// include/kbest_shims.hpp and linked to libkbest_amd.so.
// usage: shim_frontier K FILE...   -- FILE: "nL nM" and then the (nL+nM)*nM column-major costs as C99 hex floats ("inf" allowed)
// per file: one line "p <column> <nL+1 hex floats>" per column, or one line "hybridFrontierProb: runtime_error <what>".
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "kbest_shims.hpp"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const unsigned long k = strtoul(argv[1], nullptr, 10);
    for (int i = 2; i < argc; i++) {
        FILE *f = fopen(argv[i], "r");
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
        try {
            const std::vector<std::vector<double>> probs = hybridFrontierProb(cost, nL, nM, k);
            if (probs.size() != nM) return 3;
            for (size_t c = 0; c < nM; c++) {
                if (probs[c].size() != nL + 1) return 3;
                printf("p %zu", c);
                for (double v : probs[c]) printf(" %a", v);
                printf("\n");
            }
        } catch (const std::runtime_error &e) {
            printf("hybridFrontierProb: runtime_error %s\n", e.what());
        }
    }
    return 0;
}

// The plain C++ of kbest_table_sample.hip (kbest_table_sample.h: the uniform, the weight of a slot, the running sums, the pick, the
// log term) on the HOST, built with -fsanitize=address,undefined and run on heap blocks of exactly the size a problem needs: P of nf
// doubles, the table of k * maxCol words, every output.  It checks what a GPU run cannot show without risk: that no step of the
// selection or of the index arithmetic around it reads or writes beyond them.  tests/test_table_sample_cpu.py builds and runs it
// and compares the draws with tests/table_sample_check.py.  It also calls the pick with T = total and beyond: the fall-through.
// usage: table_sample_host IN OUT
//   IN: int nProb, nSample; u64 seed; u32 sampleBase, pad; per problem int k, maxCol, m, nf; u32 clusterKey, pad; u64 frameKey;
//       double cutoff; int row4col[k][maxCol]; double gain[k]
//   OUT: per problem int info, last; double total; int assign[nSample][m]; int pick[nSample]; double logTerm[nSample];
//        int pickAtTotal, pickBeyond, pickAtZero, pad
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#define __host__
#define __device__
#include "kbest_table_sample.h"

typedef unsigned long long u64;
typedef unsigned u32;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g) return 2;
    int hdr[2];
    u64 seed;
    u32 base[2];
    if (fread(hdr, 4, 2, f) != 2 || fread(&seed, 8, 1, f) != 1 || fread(base, 4, 2, f) != 2) return 2;
    const int nProb = hdr[0], nSample = hdr[1];
    const u32 sampleBase = base[0], k0 = (u32)seed, k1 = (u32)(seed >> 32);
    for (int q = 0; q < nProb; q++) {
        int sh[4];
        u32 ck[2];
        u64 frameKey;
        double cutoff;
        if (fread(sh, 4, 4, f) != 4 || fread(ck, 4, 2, f) != 2 || fread(&frameKey, 8, 1, f) != 1 || fread(&cutoff, 8, 1, f) != 1) return 2;
        const int k = sh[0], maxCol = sh[1], m = sh[2];
        int n = sh[3];
        if (k < 1 || k > kb::TS_MAX_K || m < 1 || m > maxCol || ck[0] >= kb::TS_MAX_KEY) return 3;
        int *tab = new int[(size_t)k * maxCol];
        double *gain = new double[k];
        if (fread(tab, 4, (size_t)k * maxCol, f) != (size_t)k * maxCol || fread(gain, 8, k, f) != (size_t)k) return 2;
        if (n > k) n = k;
        // exact-size blocks: AddressSanitizer sees any access beyond them
        int *assign = new int[(size_t)nSample * m], *pick = new int[nSample];
        double *logTerm = new double[nSample];
        double *P = new double[n > 0 ? n : 0];
        const double g0 = n > 0 ? gain[0] : 0.0;
        for (int j = 0; j < n; j++) P[j] = kb::ts_weight(g0, gain[j], cutoff);
        const int last = kb::ts_accumulate(P, n);
        int info = 1, edge[4] = {-1, -1, -1, 0};
        double total = 0.0;
        if (last < 0) {
            info = 0;
            for (size_t e = 0; e < (size_t)nSample * m; e++) assign[e] = -1;
            for (int s = 0; s < nSample; s++) { pick[s] = -1; logTerm[s] = std::numeric_limits<double>::quiet_NaN(); }
        } else {
            total = P[n - 1];
            const double logTotal = log(total);
            for (int s = 0; s < nSample; s++) {
                const double T = kb::ts_uniform(sampleBase + (u32)s, ck[0], (u32)frameKey, (u32)(frameKey >> 32), k0, k1) * total;
                const int j = kb::ts_pick(P, n, last, T);
                pick[s] = j;
                logTerm[s] = kb::ts_log_term(g0, gain[j], logTotal);
                for (int c = 0; c < m; c++) assign[(size_t)s * m + c] = tab[(size_t)j * maxCol + c];
            }
            edge[0] = kb::ts_pick(P, n, last, total);          // rounding left no slot: the last one with a weight > 0
            edge[1] = kb::ts_pick(P, n, last, total * 2.0);
            edge[2] = kb::ts_pick(P, n, last, 0.0);
        }
        fwrite(&info, 4, 1, g);
        fwrite(&last, 4, 1, g);
        fwrite(&total, 8, 1, g);
        fwrite(assign, 4, (size_t)nSample * m, g);
        fwrite(pick, 4, nSample, g);
        fwrite(logTerm, 8, nSample, g);
        fwrite(edge, 4, 4, g);
        delete[] tab; delete[] gain; delete[] assign; delete[] pick; delete[] logTerm; delete[] P;
    }
    fclose(f);
    fclose(g);
    return 0;
}

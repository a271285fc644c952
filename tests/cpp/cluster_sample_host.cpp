// The plain C++ of kbest_cluster_sample.hip (kbest_cluster_sample.h: the generator, the tier, the placement of a cluster's layers,
// one entry of a forward layer, the walk) on the HOST, built with -fsanitize=address,undefined and run on heap blocks of exactly
// the planned size: a small cluster's 4 KiB part (history and entries, to the byte), the arena, the slot of the work space, every
// output.  It checks what a GPU run cannot show without risk: that no step of the walk or of the index arithmetic around it reads
// or writes beyond them.  tests/test_cluster_sample_cpu.py builds and runs it and compares the draws with
// tests/cluster_sample_check.py.  NOT run here: the kernel's prologue and the wave-shuffle sweep of the small tier (the layers of a
// small cluster are built by cs_layer_entry instead: the same additions in the same order).
// usage: cluster_sample_host IN OUT
//   IN: int nClus, nSample, M, arenaBytes; u32 sampleBase; u64 seed, key; per cluster int m, R; int col[m]; u16 gidx[R]; u16 raw[R];
//       double a[R][m]
//   OUT: double Z[nClus]; int tier[nClus] (0 small, 1 layers in the arena, 2 layers in the slot); int assign[nSample][M]
//        (prefilled -7); double logProb[nSample]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __host__
#define __device__
#include "kbest_cluster_sample.h"

typedef unsigned long long u64;
typedef unsigned u32;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hdr[4];
    u32 sampleBase;
    u64 seed, key;
    if (fread(hdr, 4, 4, f) != 4 || fread(&sampleBase, 4, 1, f) != 1 || fread(&seed, 8, 1, f) != 1 || fread(&key, 8, 1, f) != 1) return 2;
    const int nClus = hdr[0], nSample = hdr[1], M = hdr[2], arenaBytes = hdr[3];
    const u32 k0 = (u32)seed, k1 = (u32)(seed >> 32), f0 = (u32)key, f1 = (u32)(key >> 32);
    // exact-size outputs: AddressSanitizer sees any access beyond them
    int *assign = new int[(size_t)nSample * M];
    double *logProb = new double[nSample];
    for (size_t i = 0; i < (size_t)nSample * M; i++) assign[i] = -7;
    for (int s = 0; s < nSample; s++) logProb[s] = 0.0;
    std::vector<double> Zs(nClus);
    std::vector<int> tier(nClus);
    for (int k = 0; k < nClus; k++) {
        int mr[2];
        if (fread(mr, 4, 2, f) != 2) return 2;
        const int m = mr[0], R = mr[1], nsub = 1 << m;
        int *col = new int[m];
        unsigned short *gidx = new unsigned short[R], *raw = new unsigned short[R], *rows = new unsigned short[R], *mask = new unsigned short[R];
        double *ain = new double[(size_t)R * m];
        if (fread(col, 4, m, f) != (size_t)m || fread(gidx, 2, R, f) != (size_t)R || fread(raw, 2, R, f) != (size_t)R ||
            fread(ain, 8, (size_t)R * m, f) != (size_t)R * m)
            return 2;
        for (int i = 0; i < R; i++) rows[i] = (unsigned short)i;  // (the kept index of the cluster's row i: raw[] stands for rawRow)
        double *arena = nullptr, *slot = nullptr, *a, *hist;
        if (kb::cs_small(m, R)) {  // the wave's part of the arena: history, then entries -- exactly as many bytes as they take
            const size_t bytes = ((size_t)R * nsub + (size_t)R * m) * 8;
            if (bytes > (size_t)kb::CS_WAVE_BYTES) return 4;
            arena = new double[bytes / 8];
            hist = arena;
            a = hist + R * nsub;
            tier[k] = 0;
        } else {  // the workgroup tier: the arena of the launch, the slot of a launch whose maxRawRow is R
            const kb::CsPlace where = kb::cs_place(m, R, arenaBytes);
            const long long aPart = (long long)R * 16;
            arena = new double[arenaBytes / 8];
            slot = new double[(size_t)aPart + ((size_t)R << m)];  // (at most the (R + 2) 2^m doubles a slot holds for this cluster)
            a = where.aInArena ? arena : slot;
            hist = where.histInArena ? arena + where.histArenaOff : slot + aPart;
            tier[k] = where.histInArena ? 1 : 2;
        }
        memcpy(a, ain, (size_t)R * m * 8);
        for (int i = 0; i < R; i++) {
            unsigned mk = 0;
            for (int j = 0; j < m; j++) mk |= (a[i * m + j] > 0.0) ? (1u << j) : 0u;
            mask[i] = (unsigned short)mk;
        }
        for (int S = 0; S < nsub; S++) hist[S] = (S == 0) ? 1.0 : 0.0;
        for (int i = 0; i + 1 < R; i++)
            for (int S = 0; S < nsub; S++)
                hist[(long long)(i + 1) * nsub + S] = kb::cs_layer_entry(hist + (long long)i * nsub, a + i * m, mask[i], (unsigned)S, i + 1);
        const unsigned full = (unsigned)nsub - 1u;
        const double Z = R >= m ? kb::cs_layer_entry(hist + (long long)(R - 1) * nsub, a + (R - 1) * m, mask[R - 1], full, R) : 0.0;
        Zs[k] = Z;
        if (Z > 0.0)
            for (int s = 0; s < nSample; s++) {
                const double prod = kb::cs_walk(hist, a, R, m, Z, rows, gidx, raw, col, sampleBase + (u32)s, f0, f1, k0, k1,
                                                assign + (size_t)s * M);
                logProb[s] = logProb[s] + (log(prod) - log(Z));
            }
        delete[] col; delete[] gidx; delete[] raw; delete[] rows; delete[] mask; delete[] ain; delete[] arena; delete[] slot;
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(Zs.data(), 8, nClus, f);
    fwrite(tier.data(), 4, nClus, f);
    fwrite(assign, 4, (size_t)nSample * M, f);
    fwrite(logProb, 8, nSample, f);
    fclose(f);
    delete[] assign;
    delete[] logProb;
    return 0;
}

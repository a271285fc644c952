// kbest_cluster_sample.h -- the parts of kbest_cluster_sample.hip that are plain C++: the generator, the tier and the placement of a
// cluster's layers, one entry of a forward layer, and the backward walk of one draw over one cluster.  __host__ __device__, no HIP
// type: tests/cpp/cluster_sample_host.cpp includes this file alone and runs it under sanitizers on exact-size heap blocks.
#ifndef KBEST_CLUSTER_SAMPLE_H
#define KBEST_CLUSTER_SAMPLE_H

namespace kb {

constexpr int CS_WAVE_BYTES = 4096;  // LDS of one wave of the small tier (CL_WAVE_BYTES of kbest_cluster.hip)

struct CsPhilox { unsigned w[4]; };

// Philox4x32-10 (Salmon et al., SC11), as kbest_sample.hip has it
__host__ __device__ inline CsPhilox cs_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
    for (int round = 0; round < 10; round++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return CsPhilox{{c0, c1, c2, c3}};
}

// the tier of a cluster of m columns and R rows: cl_small of kbest_cluster.hip
__host__ __device__ inline bool cs_small(int m, int R) { return m <= 6 && (R * (1 << m) + R * m) * 8 <= CS_WAVE_BYTES; }

// Where the workgroup tier keeps a cluster's entries a[R][m] and its layers hist[R][2^m]: in the LDS arena where they fit (a first,
// the layers behind it), else in the workgroup's slot of the work space (a at its start, the layers aPart doubles further).
struct CsPlace {
    bool aInArena, histInArena;
    long long histArenaOff;  // doubles from the arena's start (histInArena)
};
__host__ __device__ inline CsPlace cs_place(int m, int R, long long arenaBytes)
{
    const long long aBytes = (long long)R * m * 8, allBytes = aBytes + ((long long)R << m) * 8;
    CsPlace pl;
    pl.aInArena = aBytes <= arenaBytes;
    pl.histInArena = allBytes <= arenaBytes;
    pl.histArenaOff = (long long)R * m;
    return pl;
}

// F[i+1][S] from F[i] (Fi), row i's entries ar[m] and the mask mk of its non-zero ones; rowsDone = i + 1.  The expression and the
// order of the additions are kbest_perm.hip's.
__host__ __device__ inline double cs_layer_entry(const double *Fi, const double *ar, unsigned mk, unsigned S, int rowsDone)
{
    double v = 0.0;
    if (__builtin_popcount(S) <= rowsDone) {  // (more columns than rows so far: 0)
        v = Fi[S];
        unsigned cols = S & mk;
        while (cols) {
            const int c = __builtin_ctz(cols);
            cols &= cols - 1u;
            v = v + ar[c] * Fi[S ^ (1u << c)];
        }
    }
    return v;
}

// The walk of kbest_sample.hip for ONE draw on ONE cluster: hist[R][2^m] its layers F_k[0 .. R-1], a[R][m] its entries, Z = Z_k > 0.
// rows[i]: the kept index of the cluster's row i, rawRow[rows[i]] the row of the caller's block; ridx[i]: the index of that row among
// the frame's ACTIVE rows -- the i of u(s, i); col[j]: the frame's column of the cluster's column j.  Writes out[col[j]] for every j
// and returns the product of the chosen entries.
__host__ __device__ inline double cs_walk(const double *hist, const double *a, int R, int m, double Z, const unsigned short *rows,
                                          const unsigned short *ridx, const unsigned short *rawRow, const int *col, unsigned draw,
                                          unsigned f0, unsigned f1, unsigned k0, unsigned k1, int *out)
{
    const int nsub = 1 << m;
    unsigned S = (unsigned)nsub - 1u;
    double prod = 1.0;
    CsPhilox rnd = {};
    int blk = -1;
    for (int i = R - 1; i >= 0 && S != 0u; i--) {
        const int gi = ridx[i];
        if ((gi >> 1) != blk) {
            blk = gi >> 1;
            rnd = cs_philox4x32_10(draw, (unsigned)blk, f0, f1, k0, k1);
        }
        const unsigned lo = (gi & 1) ? rnd.w[2] : rnd.w[0], hi = (gi & 1) ? rnd.w[3] : rnd.w[1];
        const double u = (double)((((unsigned long long)hi << 32) | lo) >> 11) * 0x1.0p-53;
        const double *Fi = hist + (long long)i * nsub;
        const double tot = (i == R - 1) ? Z : Fi[nsub + S];  // F[i+1][S]
        const double T = u * tot;
        double acc = Fi[S];
        if (T < acc) continue;  // row i stays unassigned
        const double *ar = a + i * m;
        unsigned cols = S;
        int take = -1;
        double at = 1.0;
        while (cols) {
            const int c = __builtin_ctz(cols);
            cols &= cols - 1u;
            const double ac = ar[c];
            if (!(ac > 0.0)) continue;  // (not in the row's mask: no term)
            const double term = ac * Fi[S ^ (1u << c)];
            acc = acc + term;
            if (term > 0.0) { take = c; at = ac; }
            if (T < acc) break;
        }
        if (take >= 0) {
            out[col[take]] = rawRow[rows[i]];
            S ^= 1u << take;
            prod = prod * at;
        }
    }
    return prod;
}

}  // namespace kb
#endif

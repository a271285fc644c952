// kbest_quadric.h -- what the two quadric cost builders share (kbest_costs.hip: the raw block; kbest_quadric_map.hip: the
// conditioned compact block of a frame against a large map): the 3x3 solve and the cost of one (landmark, measurement) pair, so
// that both produce the same bits.  Device code only.
#ifndef KBEST_QUADRIC_H
#define KBEST_QUADRIC_H

namespace kb {

// x = S^-1 d for a symmetric 3x3 S by LDL^T with diagonal pivoting (largest remaining |diagonal| first): the
// published algorithm of Eigen::LDLT, which computeQuadricCostMatrix calls (assignment.cpp:717).  Same operation
// order as the checker's restatement, so the two agree bit for bit; against Eigen itself (absent, unpinned) the
// contract is 1e-12 relative.
__device__ inline void ldlt3_solve(const double *S, const double *d, double *x)
{
    double A[3][3], b[3], L[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, D[3];
    int perm[3] = {0, 1, 2};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        b[i] = d[i];
#pragma unroll
        for (int j = 0; j < 3; j++) A[i][j] = S[i * 3 + j];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int piv = k;
#pragma unroll
        for (int i = k + 1; i < 3; i++) if (fabs(A[i][i]) > fabs(A[piv][piv])) piv = i;
        if (piv != k) {
#pragma unroll
            for (int j = 0; j < 3; j++) { const double t = A[k][j]; A[k][j] = A[piv][j]; A[piv][j] = t; }
#pragma unroll
            for (int i = 0; i < 3; i++) { const double t = A[i][k]; A[i][k] = A[i][piv]; A[i][piv] = t; }
#pragma unroll
            for (int j = 0; j < 3; j++) if (j < k) { const double t = L[k][j]; L[k][j] = L[piv][j]; L[piv][j] = t; }
            const int t = perm[k]; perm[k] = perm[piv]; perm[piv] = t;
        }
        D[k] = A[k][k];
#pragma unroll
        for (int i = k + 1; i < 3; i++) L[i][k] = A[i][k] / D[k];
#pragma unroll
        for (int i = k + 1; i < 3; i++)
#pragma unroll
            for (int j = k + 1; j < 3; j++) A[i][j] = A[i][j] - L[i][k] * D[k] * L[j][k];
    }
    double y[3], z[3];
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = b[perm[i]];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) if (j < i) y[i] = y[i] - L[i][j] * y[j];
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = y[i] / D[i];
#pragma unroll
    for (int i = 2; i >= 0; i--)
#pragma unroll
        for (int j = 0; j < 3; j++) if (j > i) y[i] = y[i] - L[j][i] * y[j];
#pragma unroll
    for (int i = 0; i < 3; i++) z[perm[i]] = y[i];
#pragma unroll
    for (int i = 0; i < 3; i++) x[i] = z[i];
}

}  // namespace kb
#endif

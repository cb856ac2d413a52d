// ldlt.h -- the 6 x 6 symmetric solve shared by kernels_mlpnp.hip (S13: the Gauss-Newton step of computePose) and
// kernels_poseopt.hip (S14: the Levenberg step of PoseOptimization).  Contraction is off in every including unit.
// Also compiled as plain host C++ by tests/cpp/poseopt.cpp (the S14 host loop), which includes this text instead of copying it.
#pragma once
#include <cmath>

#include "host_device.h"

namespace orbfe {

// A x = b for symmetric 6 x 6 A (destroyed) by L D L^T with diagonal pivoting (S13).  *positive (optional) = every pivot d > 0:
// what Eigen's LDLT::isPositive() tells LinearSolverDense (S14).
// The pivot row is a run-time value; every array index below is a compile-time one all the same (the swaps and the two permuted
// accesses are written as selects over the candidates), so that on the device the 80 doubles stay in registers instead of scratch
// memory.  The arithmetic and its order are those of the indexed form: at step k the largest |diagonal| of the trailing block (first
// of equals, found with '>') is swapped to k.
ORBFE_HD inline void ldlt_solve6(double (&A)[6][6], const double (&b)[6], double (&x)[6], bool* positive = nullptr)
{
    double L[6][6], d[6];
    int perm[6];
    ORBFE_UNROLL
    for (int i = 0; i < 6; i++) {
        perm[i] = i;
        ORBFE_UNROLL
        for (int j = 0; j < 6; j++) L[i][j] = 0.0;
    }
    ORBFE_UNROLL
    for (int k = 0; k < 6; k++) {
        int best = k;
        double bestAbs = fabs(A[k][k]);
        ORBFE_UNROLL
        for (int i = k + 1; i < 6; i++) {
            const double v = fabs(A[i][i]);
            if (v > bestAbs) { best = i; bestAbs = v; }
        }
        ORBFE_UNROLL
        for (int i = k + 1; i < 6; i++) {   // rows k and best of A and of L, the two entries of perm
            const bool sw = best == i;
            ORBFE_UNROLL
            for (int j = 0; j < 6; j++) {
                const double ak = A[k][j], ai = A[i][j], lk = L[k][j], li = L[i][j];
                A[k][j] = sw ? ai : ak;
                A[i][j] = sw ? ak : ai;
                L[k][j] = sw ? li : lk;
                L[i][j] = sw ? lk : li;
            }
            const int pk = perm[k], pi = perm[i];
            perm[k] = sw ? pi : pk;
            perm[i] = sw ? pk : pi;
        }
        ORBFE_UNROLL
        for (int i = k + 1; i < 6; i++) {   // columns k and best of A
            const bool sw = best == i;
            ORBFE_UNROLL
            for (int r = 0; r < 6; r++) {
                const double ak = A[r][k], ai = A[r][i];
                A[r][k] = sw ? ai : ak;
                A[r][i] = sw ? ak : ai;
            }
        }
        const double dk = A[k][k];
        d[k] = dk;
        double col[6];
        ORBFE_UNROLL
        for (int i = 0; i < 6; i++) col[i] = A[i][k];
        ORBFE_UNROLL
        for (int i = k + 1; i < 6; i++) {
            const double li = dk == 0.0 ? 0.0 : col[i] / dk;
            L[i][k] = li;
            ORBFE_UNROLL
            for (int j = k + 1; j <= i; j++) {
                const double val = A[i][j] - li * col[j];
                A[i][j] = val;
                A[j][i] = val;
            }
        }
    }
    double z[6], w[6], xs[6];
    ORBFE_UNROLL
    for (int i = 0; i < 6; i++) {
        double acc = b[0];   // b[perm[i]]
        ORBFE_UNROLL
        for (int j = 1; j < 6; j++) acc = perm[i] == j ? b[j] : acc;
        ORBFE_UNROLL
        for (int j = 0; j < i; j++) acc = acc - L[i][j] * z[j];
        z[i] = acc;
    }
    ORBFE_UNROLL
    for (int i = 0; i < 6; i++) w[i] = d[i] == 0.0 ? 0.0 : z[i] / d[i];
    ORBFE_UNROLL
    for (int i = 5; i >= 0; i--) {
        double acc = w[i];
        ORBFE_UNROLL
        for (int j = i + 1; j < 6; j++) acc = acc - L[j][i] * xs[j];
        xs[i] = acc;
    }
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++) {   // x[perm[i]] = xs[i]
        double v = xs[0];
        ORBFE_UNROLL
        for (int i = 1; i < 6; i++) v = perm[i] == j ? xs[i] : v;
        x[j] = v;
    }
    if (positive) {
        bool pos = true;
        ORBFE_UNROLL
        for (int i = 0; i < 6; i++) pos = pos && d[i] > 0.0;
        *positive = pos;
    }
}

// The indexed form of exactly the arithmetic and pivot rule above, for any N (S19: the 15 x 15 Gauss-Newton step of
// PoseInertialOptimizationLastKeyFrame).  One thread, run-time indices: the host loops and the restatements read this; a kernel
// maps the same operations onto a wave (kernels_poseimu.hip) or, for N = 6, uses ldlt_solve6.
template <int N>
ORBFE_HD inline void ldlt_solve_n(double (&A)[N][N], const double (&b)[N], double (&x)[N], bool* positive = nullptr)
{
    double L[N][N], d[N];
    int perm[N];
    for (int i = 0; i < N; i++) {
        perm[i] = i;
        for (int j = 0; j < N; j++) L[i][j] = 0.0;
    }
    for (int k = 0; k < N; k++) {
        int best = k;
        double bestAbs = fabs(A[k][k]);
        for (int i = k + 1; i < N; i++) {
            const double v = fabs(A[i][i]);
            if (v > bestAbs) { best = i; bestAbs = v; }
        }
        if (best != k) {
            for (int j = 0; j < N; j++) {
                const double a = A[k][j], l = L[k][j];
                A[k][j] = A[best][j];
                A[best][j] = a;
                L[k][j] = L[best][j];
                L[best][j] = l;
            }
            const int p = perm[k];
            perm[k] = perm[best];
            perm[best] = p;
            for (int r = 0; r < N; r++) {
                const double a = A[r][k];
                A[r][k] = A[r][best];
                A[r][best] = a;
            }
        }
        const double dk = A[k][k];
        d[k] = dk;
        double col[N];
        for (int i = 0; i < N; i++) col[i] = A[i][k];
        for (int i = k + 1; i < N; i++) {
            const double li = dk == 0.0 ? 0.0 : col[i] / dk;
            L[i][k] = li;
            for (int j = k + 1; j <= i; j++) {
                const double val = A[i][j] - li * col[j];
                A[i][j] = val;
                A[j][i] = val;
            }
        }
    }
    double z[N], w[N], xs[N];
    for (int i = 0; i < N; i++) {
        double acc = b[perm[i]];
        for (int j = 0; j < i; j++) acc = acc - L[i][j] * z[j];
        z[i] = acc;
    }
    for (int i = 0; i < N; i++) w[i] = d[i] == 0.0 ? 0.0 : z[i] / d[i];
    for (int i = N - 1; i >= 0; i--) {
        double acc = w[i];
        for (int j = i + 1; j < N; j++) acc = acc - L[j][i] * xs[j];
        xs[i] = acc;
    }
    for (int i = 0; i < N; i++) x[perm[i]] = xs[i];
    if (positive) {
        bool pos = true;
        for (int i = 0; i < N; i++) pos = pos && d[i] > 0.0;
        *positive = pos;
    }
}

}  // namespace orbfe

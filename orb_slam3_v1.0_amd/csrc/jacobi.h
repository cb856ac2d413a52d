// jacobi.h -- the pinned Jacobi sequences of SPEC DECISIONS S10 / S12 / S13 and the 3 x 3 binary32 helpers of S12, shared by
// kernels_match_tri.hip, kernels_twoview.hip and kernels_mlpnp.hip (device), the host step of orbfe_two_view_reconstruct and, as
// plain host C++, tests/cpp/mlpnp.cpp and tests/cpp/two_view.cpp.  No HIP outside the __HIPCC__ block at the end.
// Every translation unit that includes this is built with -ffp-contract=off: c * a - s * b is two products and one add.
#pragma once
#include <cmath>

#include "host_device.h"

namespace orbfe {

// smallest-eigenvalue eigenvector of the symmetric 4x4 matrix M (destroyed)
ORBFE_HD inline void sym4_min_eigenvector(double (&M)[4][4], double (&vOut)[4])
{
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 8; sweep++) {
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                const double apq = M[p][q];
                if (apq == 0.0) continue;
                const double theta = (M[q][q] - M[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double sn = t * c;
                for (int k = 0; k < 4; k++) {  // columns p, q of M
                    const double mkp = M[k][p], mkq = M[k][q];
                    M[k][p] = c * mkp - sn * mkq;
                    M[k][q] = sn * mkp + c * mkq;
                }
                for (int k = 0; k < 4; k++) {  // rows p, q of M
                    const double mpk = M[p][k], mqk = M[q][k];
                    M[p][k] = c * mpk - sn * mqk;
                    M[q][k] = sn * mpk + c * mqk;
                }
                for (int k = 0; k < 4; k++) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - sn * vkq;
                    V[k][q] = sn * vkp + c * vkq;
                }
            }
    }
    // column of the smallest diagonal entry, lowest index on ties (selects instead of a run-time column index: the arrays
    // stay in registers)
    double best = M[0][0];
    for (int k = 0; k < 4; k++) vOut[k] = V[k][0];
    for (int i = 1; i < 4; i++) {
        const bool less = M[i][i] < best;
        best = less ? M[i][i] : best;
        for (int k = 0; k < 4; k++) vOut[k] = less ? V[k][i] : vOut[k];
    }
}

constexpr int kTwoViewSweeps = 10;  // S12: fixed, no data-dependent exit

// the rotation angle of every Jacobi sequence here (S10): c, s from M[p][p], M[q][q], M[p][q] != 0
ORBFE_HD inline void jacobi_angle(double app, double aqq, double apq, double& c, double& sn)
{
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    sn = t * c;
}

// S12, n = 3: kTwoViewSweeps cyclic sweeps in the pair order (0,1) (0,2) (1,2); M becomes (nearly) diagonal, V its eigenvectors
template <int P, int Q>
ORBFE_HD inline void jacobi3_rotate(double (&M)[3][3], double (&V)[3][3])
{
    const double apq = M[P][Q];
    if (apq == 0.0) return;
    double c, sn;
    jacobi_angle(M[P][P], M[Q][Q], apq, c, sn);
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) {
        const double mkp = M[k][P], mkq = M[k][Q];
        M[k][P] = c * mkp - sn * mkq;
        M[k][Q] = sn * mkp + c * mkq;
    }
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) {
        const double mpk = M[P][k], mqk = M[Q][k];
        M[P][k] = c * mpk - sn * mqk;
        M[Q][k] = sn * mpk + c * mqk;
    }
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - sn * vkq;
        V[k][Q] = sn * vkp + c * vkq;
    }
}

ORBFE_HD inline void jacobi3(double (&M)[3][3], double (&V)[3][3])
{
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kTwoViewSweeps; sweep++) {
        jacobi3_rotate<0, 1>(M, V);
        jacobi3_rotate<0, 2>(M, V);
        jacobi3_rotate<1, 2>(M, V);
    }
}

// C = A B, row-major 3 x 3 binary32, k ascending
ORBFE_HD inline void mul3(const float (&A)[9], const float (&B)[9], float (&C)[9])
{
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

ORBFE_HD inline void transpose3(const float (&A)[9], float (&T)[9])
{
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}

// adjugate / determinant (S12: Matrix3f::inverse())
ORBFE_HD inline void inv3(const float (&a)[9], float (&o)[9])
{
    const float c00 = a[4] * a[8] - a[5] * a[7];
    const float c01 = a[2] * a[7] - a[1] * a[8];
    const float c02 = a[1] * a[5] - a[2] * a[4];
    const float c10 = a[5] * a[6] - a[3] * a[8];
    const float c11 = a[0] * a[8] - a[2] * a[6];
    const float c12 = a[2] * a[3] - a[0] * a[5];
    const float c20 = a[3] * a[7] - a[4] * a[6];
    const float c21 = a[1] * a[6] - a[0] * a[7];
    const float c22 = a[0] * a[4] - a[1] * a[3];
    const float det = (a[0] * c00 + a[1] * c10) + a[2] * c20;
    const float inv = 1.0f / det;
    o[0] = c00 * inv; o[1] = c01 * inv; o[2] = c02 * inv;
    o[3] = c10 * inv; o[4] = c11 * inv; o[5] = c12 * inv;
    o[6] = c20 * inv; o[7] = c21 * inv; o[8] = c22 * inv;
}

ORBFE_HD inline float det3(const float (&a)[9])
{
    const float c00 = a[4] * a[8] - a[5] * a[7];
    const float c10 = a[5] * a[6] - a[3] * a[8];
    const float c20 = a[3] * a[7] - a[4] * a[6];
    return (a[0] * c00 + a[1] * c10) + a[2] * c20;
}

// rank-2 step of ComputeF21 (src/TwoViewReconstruction.cc:300-305): Fpre - (Fpre v) v^T with v the eigenvector of the
// smallest eigenvalue of Fpre^T Fpre (lowest index on ties), binary64, rounded to float per entry
ORBFE_HD inline void rank2_f(const float (&F)[9], float (&Fn)[9])
{
    double G[3][3], V[3][3];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
            ORBFE_UNROLL
            for (int k = 0; k < 3; k++) acc = acc + (double)F[3 * k + i] * (double)F[3 * k + j];
            G[i][j] = acc;
        }
    jacobi3(G, V);
    double best = G[0][0];
    double v[3] = {V[0][0], V[1][0], V[2][0]};
    ORBFE_UNROLL
    for (int i = 1; i < 3; i++) {
        const bool less = G[i][i] < best;
        best = less ? G[i][i] : best;
        ORBFE_UNROLL
        for (int k = 0; k < 3; k++) v[k] = less ? V[k][i] : v[k];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        const double w = ((double)F[3 * i] * v[0] + (double)F[3 * i + 1] * v[1]) + (double)F[3 * i + 2] * v[2];
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) Fn[3 * i + j] = (float)((double)F[3 * i + j] - w * v[j]);
    }
}

// ---- SPEC DECISION S13: the 12 x 12 sequence, and S12's 9 x 9 sequence, run by a team of threads ----
constexpr int kMlpnpSweeps = 12;  // S13: fixed, no data-dependent exit

// the pairs of round r.  n = 12 (11 rounds of 6): {r, 11} and {(r + k) mod 11, (r - k) mod 11}, k = 1 .. 5 (the circle method);
// n = 9 (9 rounds of 4, S12): the pairs {i, j}, i < j, i + j == r (mod 9), in ascending i
ORBFE_HD inline void jacobi_round_pair(int n, int r, int slot, int& p, int& q)
{
    if (n == 12) {
        if (slot == 0) { p = r; q = 11; return; }
        const int a = (r + slot) % 11, b = (r - slot + 11) % 11;
        p = a < b ? a : b;
        q = a < b ? b : a;
        return;
    }
    int cnt = 0;
    p = 0; q = 0;
    for (int i = 0; i < 9; i++) {
        const int j = (r - i + 9) % 9;
        if (i < j) {
            if (cnt == slot) { p = i; q = j; }
            cnt++;
        }
    }
}

// what a team shares while it diagonalises one matrix (LDS on the device)
struct JacobiTeamWork {
    double M[12][12], V[12][12];
    double c[6], s[6];
    int skip[6];
    int P[11][6], Q[11][6];
};

#if defined(__HIPCC__)
// n = 12: kMlpnpSweeps sweeps of 11 rounds of 6 pairs; n = 9: kTwoViewSweeps sweeps of 9 rounds of 4 pairs.  Per round the angles
// from M as it stands at the start of the round, then the column phase of all pairs, then the row phase of all pairs and V's
// column phase.  M (symmetric, n x n in W.M) becomes (nearly) diagonal, W.V its eigenvectors.  Called by every thread of the block.
__device__ inline void jacobi_rounds_block(JacobiTeamWork& W, int n)
{
    const int tid = threadIdx.x, nth = blockDim.x;
    const int np = n == 12 ? 6 : 4, nr = n == 12 ? 11 : 9, sweeps = n == 12 ? kMlpnpSweeps : kTwoViewSweeps;
    for (int e = tid; e < nr * np; e += nth) jacobi_round_pair(n, e / np, e % np, W.P[e / np][e % np], W.Q[e / np][e % np]);
    for (int e = tid; e < n * n; e += nth) W.V[e / n][e % n] = e / n == e % n ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < sweeps; sweep++)
        for (int r = 0; r < nr; r++) {
            for (int e = tid; e < np; e += nth) {
                const int p = W.P[r][e], q = W.Q[r][e];
                const double apq = W.M[p][q];
                const int skip = apq == 0.0;
                double c = 1.0, sn = 0.0;
                if (!skip) jacobi_angle(W.M[p][p], W.M[q][q], apq, c, sn);
                W.c[e] = c; W.s[e] = sn; W.skip[e] = skip;
            }
            __syncthreads();
            for (int e = tid; e < np * n; e += nth) {  // columns p, q of M
                const int pr = e / n, k = e % n;
                if (W.skip[pr]) continue;
                const int p = W.P[r][pr], q = W.Q[r][pr];
                const double c = W.c[pr], sn = W.s[pr];
                const double a = W.M[k][p], b = W.M[k][q];
                W.M[k][p] = c * a - sn * b;
                W.M[k][q] = sn * a + c * b;
            }
            __syncthreads();
            for (int e = tid; e < np * n; e += nth) {  // rows p, q of M; columns p, q of V
                const int pr = e / n, k = e % n;
                if (W.skip[pr]) continue;
                const int p = W.P[r][pr], q = W.Q[r][pr];
                const double c = W.c[pr], sn = W.s[pr];
                const double a = W.M[p][k], b = W.M[q][k];
                W.M[p][k] = c * a - sn * b;
                W.M[q][k] = sn * a + c * b;
                const double va = W.V[k][p], vb = W.V[k][q];
                W.V[k][p] = c * va - sn * vb;
                W.V[k][q] = sn * va + c * vb;
            }
            __syncthreads();
        }
}
#endif  // __HIPCC__

}  // namespace orbfe

// mat3d.h -- the 3 x 3 binary64 helpers (row-major) shared by kernels_mlpnp.hip (S13) and kernels_poseopt.hip (S14), and the per-thread
// leaf functions of S13's computePose: the 3 x 3 decompositions by the n = 3 sequence of jacobi.h, Rodrigues both ways on the
// sequences of spec_math.h, the two Jacobian rows of one point.  Contraction is off in every including unit.
// No HIP here: tests/cpp/mlpnp.cpp and tests/cpp/poseopt.cpp include this text as host C++ instead of copying it.
#pragma once
#include <cmath>
#include <cstring>

#include "host_device.h"
#include "jacobi.h"
#include "spec_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

constexpr double kEps = 0x1p-52;
constexpr double kRankTol = 0x1.8p-51;     // 3 eps: Eigen's FullPivHouseholderQR threshold for a 3 x 3

// ---- 3 x 3 binary64 helpers, row-major ----
ORBFE_HD inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
ORBFE_HD inline double norm3(const double* a) { return sqrt(dot3(a, a)); }
ORBFE_HD inline void matvec3(const double* R, const double* x, double* o)
{
    for (int i = 0; i < 3; i++) o[i] = (R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2];
}
ORBFE_HD inline void mul3d(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
ORBFE_HD inline void transpose3d(const double* A, double* T)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}
ORBFE_HD inline double det3d(const double* a)
{
    const double c00 = a[4] * a[8] - a[5] * a[7];
    const double c10 = a[5] * a[6] - a[3] * a[8];
    const double c20 = a[3] * a[7] - a[4] * a[6];
    return (a[0] * c00 + a[1] * c10) + a[2] * c20;
}
// the inverse of a symmetric 3 x 3 given as its six distinct entries (00 01 02 11 12 22), returned the same way (S17): the six
// distinct cofactors in the order of S12's adjugate (jacobi.h inv3), the determinant by the first row, one reciprocal
ORBFE_HD inline void inv3_sym(const double (&a)[6], double (&o)[6])
{
    const double c00 = a[3] * a[5] - a[4] * a[4];
    const double c01 = a[2] * a[4] - a[1] * a[5];
    const double c02 = a[1] * a[4] - a[2] * a[3];
    const double c11 = a[0] * a[5] - a[2] * a[2];
    const double c12 = a[2] * a[1] - a[0] * a[4];
    const double c22 = a[0] * a[3] - a[1] * a[1];
    const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
    const double inv = 1.0 / det;
    o[0] = c00 * inv; o[1] = c01 * inv; o[2] = c02 * inv;
    o[3] = c11 * inv; o[4] = c12 * inv; o[5] = c22 * inv;
}
ORBFE_HD inline void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// eigen-decomposition of the symmetric G (row-major, destroyed) by the n = 3 sequence; order[] = the columns stably sorted by
// ascending (descending) eigenvalue
ORBFE_HD inline void eig3_sorted(const double* G, bool descending, double (&lam)[3], double (&E)[3][3], int (&order)[3])
{
    double M[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = G[3 * i + j];
    jacobi3(M, E);
    for (int i = 0; i < 3; i++) { lam[i] = M[i][i]; order[i] = i; }
    for (int a = 1; a < 3; a++)  // stable insertion sort
        for (int b = a; b > 0; b--) {
            const double x = lam[order[b]], y = lam[order[b - 1]];
            const bool before = descending ? x > y : x < y;
            if (!before) break;
            const int t = order[b]; order[b] = order[b - 1]; order[b - 1] = t;
        }
}

// U V^T of A's singular value decomposition, negated when its determinant is negative (:545-549, :604-608)
ORBFE_HD inline void polar3(const double* A, double* R)
{
    double G[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc = acc + A[3 * k + i] * A[3 * k + j];
            G[3 * i + j] = acc;
        }
    double lam[3], E[3][3];
    int order[3];
    eig3_sorted(G, true, lam, E, order);
    double v[3][3], av[3][3], u[3][3];
    for (int i = 0; i < 3; i++) {
        for (int k = 0; k < 3; k++) v[i][k] = E[k][order[i]];
        matvec3(A, v[i], av[i]);
    }
    for (int i = 0; i < 2; i++) {
        const double nrm = norm3(av[i]);
        for (int k = 0; k < 3; k++) u[i][k] = av[i][k] / nrm;
    }
    cross3(u[0], u[1], u[2]);
    if (dot3(av[2], u[2]) < 0.0)
        for (int k = 0; k < 3; k++) u[2][k] = -u[2][k];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (u[0][i] * v[0][j] + u[1][i] * v[1][j]) + u[2][i] * v[2][j];
    if (det3d(R) < 0.0)
        for (int k = 0; k < 9; k++) R[k] = -R[k];
}

ORBFE_HD inline void skew3(const double* w, double* K)
{
    K[0] = 0.0; K[1] = -w[2]; K[2] = w[1];
    K[3] = w[2]; K[4] = 0.0; K[5] = -w[0];
    K[6] = -w[1]; K[7] = w[0]; K[8] = 0.0;
}

// rodrigues2rot (:659-674) and, when D is given, dR / dw_k from the closed form (the limit [e_k]x for |w| <= eps)
ORBFE_HD inline void rodrigues2rot(const double* w, double* R, double (*D)[9])
{
    double K[9], K2[9];
    skew3(w, K);
    mul3d(K, K, K2);
    const double n = norm3(w);
    const bool big = n > kEps;
    double sn, cs;
    spec_sincos64(n, sn, cs);
    const double a = sn / n;
    const double nn = n * n;
    const double b = (1.0 - cs) / nn;
    for (int k = 0; k < 9; k++) {
        const double I = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        R[k] = big ? (I + a * K[k]) + b * K2[k] : I;
    }
    if (!D) return;
    const double da = (n * cs - sn) / nn;
    const double db = (n * sn - 2.0 * (1.0 - cs)) / (nn * n);
    for (int k = 0; k < 3; k++) {
        const double ek[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double G[9], GK[9], KG[9];
        skew3(ek, G);
        for (int e = 0; e < 9; e++) G[e] = G[e] == 0.0 ? 0.0 : G[e];  // (-0.0 of skew3 -> +0.0: the restatement's table holds +0.0)
        mul3d(G, K, GK);
        mul3d(K, G, KG);
        const double wk = w[k] / n;
        const double ca = da * wk, cb = db * wk;
        for (int e = 0; e < 9; e++) {
            const double S = GK[e] + KG[e];
            const double Dk = ((ca * K[e] + a * G[e]) + cb * K2[e]) + b * S;
            D[k][e] = big ? Dk : G[e];
        }
    }
}

// rot2rodrigues (:676-691)
ORBFE_HD inline void rot2rodrigues(const double* R, double* om)
{
    const double trace = ((R[0] + R[4]) + R[8]) - 1.0;
    const double wn = spec_acos64(trace / 2.0);
    om[0] = 0.0; om[1] = 0.0; om[2] = 0.0;
    if (wn > kEps) {
        double sn, cs;
        spec_sincos64(wn, sn, cs);
        const double sc = wn / (2.0 * sn);
        om[0] = (R[7] - R[5]) * sc;
        om[1] = (R[2] - R[6]) * sc;
        om[2] = (R[3] - R[1]) * sc;
    }
}

// the two rows of mlpnp_residuals_and_jacs (:759-805) of one point: J0 / J1 (6 each) and the residuals
ORBFE_HD inline void point_rows(const double* R, const double (*D)[9], const double* T, const double* X, const double* nr,
                                const double* ns, double* J0, double& r0, double* J1, double& r1)
{
    double q[3], v[3], DX[3][3];
    matvec3(R, X, q);
    for (int i = 0; i < 3; i++) q[i] = q[i] + T[i];
    const double nq = norm3(q);
    for (int i = 0; i < 3; i++) v[i] = q[i] / nq;
    for (int k = 0; k < 3; k++) matvec3(D[k], X, DX[k]);
    for (int h = 0; h < 2; h++) {
        const double* nv = h ? ns : nr;
        double* J = h ? J1 : J0;
        const double d = dot3(nv, v);
        double g[3];
        for (int i = 0; i < 3; i++) g[i] = (nv[i] - d * v[i]) / nq;
        for (int k = 0; k < 3; k++) J[k] = dot3(g, DX[k]);
        for (int i = 0; i < 3; i++) J[3 + i] = g[i];
        (h ? r1 : r0) = d;
    }
}

// bit image of a non-negative, non-NaN double: ordered like the value
ORBFE_HD inline unsigned long long nonneg_bits(double v)
{
    unsigned long long u;
    memcpy(&u, &v, sizeof u);
    return u;
}

}  // namespace orbfe

// initial_ba_math.h -- what one thread computes for one point of the initial map's bundle adjustment (SPEC DECISION S17): the
// linearisation of its two edges (the 27 doubles of Hpp, bp and Hxp, and the 28 terms of Hxx, bx and the cost), the Schur terms at a
// damping lambda, the back-substitution and the terms of a trial.  The residual, the robust kernel, the pose Jacobian and the pose
// update are S14's (poseopt_math.h), word for word.  Contraction is off in every including unit.
// No HIP here: kernels_initial_ba.hip and tests/cpp/initial_ba.cpp (as host C++) read this one text.
#pragma once
#include <cmath>

#include "host_device.h"
#include "mat3d.h"
#include "poseopt_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

constexpr int kBaNS = 21 + 6;   // the Schur terms of one point: 21 of s (upper triangle, row by row), 6 of r
constexpr int kBaNT = 2;    // the terms of a trial: the cost, the point part of the gain's denominator

// the two observations of one point: edge 0 from the fixed pose 1, edge 1 from the free pose 2
struct BaObs {
    double ox1, oy1, w1, ox2, oy2, w2;
};

// the linearisation of one point: Hpp (00 01 02 11 12 22), bp, Hxp (6 x 3, row-major)
struct BaPoint {
    double Hpp[6], bp[3], Hxp[18];
};
constexpr int kBaNL = 6 + 3 + 18;   // doubles in a BaPoint (equal to kBaNS = 21 + 6 by coincidence: another count)
static_assert(sizeof(BaPoint) == kBaNL * sizeof(double), "BaPoint is kBaNL doubles");

// where entry (j, k) of a symmetric 3 x 3 sits among its six stored entries
ORBFE_HD constexpr int sym_ix(int j, int k) { return j == 0 ? k : (k == 0 ? j : j + k + 1); }

// the two rows of -projectJac(Xc) R (OptimizableTypes.cpp:150-152); the structural zeros of projectJac are not multiplied
ORBFE_HD inline void ba_point_rows(const PoseCam& G, const double (&R)[9], double x, double y, double z, double (&P0)[3], double (&P1)[3])
{
    const double zz = z * z;
    const double a = G.fx / z;
    const double b = -G.fx * x / zz;
    const double c = G.fy / z;
    const double d = -G.fy * y / zz;
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) {
        P0[k] = ((-a) * R[k]) + ((-b) * R[6 + k]);
        P1[k] = ((-c) * R[3 + k]) + ((-d) * R[6 + k]);
    }
}

// the build of one point at (pose 1, pose 2, X): its linearisation L and the 28 terms v (21 of Hxx, 6 of bx, the cost); edge 0's
// terms first, then edge 1's added to them
ORBFE_HD inline void ba_build(const PoseCam& G, const BaObs& O, const double (&Ra)[9], const double (&ta)[3], const double (&R)[9],
                              const double (&t)[3], const double (&X)[3], bool huber, BaPoint& L, double (&v)[kNV])
{
    double x, y, z, e0, e1, chi2, rho0a, rho0b, rho1, P0[3], P1[3];
    EdgeD E{X[0], X[1], X[2], O.ox1, O.oy1, O.w1};
    edge_residual(G, E, Ra, ta, x, y, z, e0, e1, chi2);
    robust(chi2, G.delta, huber, rho0a, rho1);
    ba_point_rows(G, Ra, x, y, z, P0, P1);
    {
        const double ww = rho1 * E.w;
        const double we0 = ww * e0, we1 = ww * e1;
        int at = 0;
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++)
            ORBFE_UNROLL
            for (int k = j; k < 3; k++) L.Hpp[at++] = ((P0[j] * ww) * P0[k]) + ((P1[j] * ww) * P1[k]);
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) L.bp[j] = -((P0[j] * we0) + (P1[j] * we1));
    }
    E.ox = O.ox2;
    E.oy = O.oy2;
    E.w = O.w2;
    edge_residual(G, E, R, t, x, y, z, e0, e1, chi2);
    robust(chi2, G.delta, huber, rho0b, rho1);
    ba_point_rows(G, R, x, y, z, P0, P1);
    // J = -projectJac(Xc) SE3deriv as in S14 (OptimizableTypes.cpp:154-159)
    const double zz = z * z;
    const double a = G.fx / z;
    const double b = -G.fx * x / zz;
    const double c = G.fy / z;
    const double d = -G.fy * y / zz;
    const double J0[6] = {-(b * y), -(a * z - b * x), a * y, -a, 0.0, -b};
    const double J1[6] = {-(d * y - c * z), d * x, -(c * x), 0.0, -c, -d};
    const double ww = rho1 * E.w;
    const double we0 = ww * e0, we1 = ww * e1;
    int at = 0;
    ORBFE_UNROLL
    for (int j = 0; j < 3; j++)
        ORBFE_UNROLL
        for (int k = j; k < 3; k++) {
            L.Hpp[at] = L.Hpp[at] + (((P0[j] * ww) * P0[k]) + ((P1[j] * ww) * P1[k]));
            at++;
        }
    ORBFE_UNROLL
    for (int j = 0; j < 3; j++) L.bp[j] = L.bp[j] + (-((P0[j] * we0) + (P1[j] * we1)));
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++)
        ORBFE_UNROLL
        for (int k = 0; k < 3; k++) L.Hxp[3 * j + k] = ((J0[j] * ww) * P0[k]) + ((J1[j] * ww) * P1[k]);
    at = 0;
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++)
        ORBFE_UNROLL
        for (int k = j; k < 6; k++) v[at++] = (J0[j] * ww) * J0[k] + (J1[j] * ww) * J1[k];
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++) v[21 + j] = -(J0[j] * we0 + J1[j] * we1);
    v[27] = rho0a + rho0b;
}

// the largest diagonal entry of Hpp above m, found with '>' (a NaN is never kept)
ORBFE_HD inline double ba_diag_max(const BaPoint& L, double m)
{
    if (L.Hpp[0] > m) m = L.Hpp[0];
    if (L.Hpp[3] > m) m = L.Hpp[3];
    if (L.Hpp[5] > m) m = L.Hpp[5];
    return m;
}

// (Hpp + lambda I)^-1 as six entries
ORBFE_HD inline void ba_dinv(const BaPoint& L, double lam, double (&Dinv)[6])
{
    const double D[6] = {L.Hpp[0] + lam, L.Hpp[1], L.Hpp[2], L.Hpp[3] + lam, L.Hpp[4], L.Hpp[5] + lam};
    inv3_sym(D, Dinv);
}

// the Schur terms of one point at lambda: s_jk (j <= k) and r_j of B = Hxp Dinv
ORBFE_HD inline void ba_schur(const BaPoint& L, double lam, double (&v)[kBaNS])
{
    double Dinv[6], B[18];
    ba_dinv(L, lam, Dinv);
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++)
        ORBFE_UNROLL
        for (int k = 0; k < 3; k++)
            B[3 * j + k] = (L.Hxp[3 * j] * Dinv[sym_ix(0, k)] + L.Hxp[3 * j + 1] * Dinv[sym_ix(1, k)]) + L.Hxp[3 * j + 2] * Dinv[sym_ix(2, k)];
    int at = 0;
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++)
        ORBFE_UNROLL
        for (int k = j; k < 6; k++) v[at++] = (B[3 * j] * L.Hxp[3 * k] + B[3 * j + 1] * L.Hxp[3 * k + 1]) + B[3 * j + 2] * L.Hxp[3 * k + 2];
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++) v[21 + j] = (B[3 * j] * L.bp[0] + B[3 * j + 1] * L.bp[1]) + B[3 * j + 2] * L.bp[2];
}

// the back-substitution of one point for the pose step dx: dp = Dinv (bp - Hxp^T dx), and the point's part of the gain's denominator
ORBFE_HD inline void ba_backsub(const BaPoint& L, double lam, const double (&dx)[6], double (&dp)[3], double& part)
{
    double Dinv[6], c[3];
    ba_dinv(L, lam, Dinv);
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) {
        double acc = 0.0;
        ORBFE_UNROLL
        for (int j = 0; j < 6; j++) acc = acc + L.Hxp[3 * j + k] * dx[j];
        c[k] = L.bp[k] - acc;
    }
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) dp[k] = (Dinv[sym_ix(k, 0)] * c[0] + Dinv[sym_ix(k, 1)] * c[1]) + Dinv[sym_ix(k, 2)] * c[2];
    part = ((dp[0] * ((lam * dp[0]) + L.bp[0])) + (dp[1] * ((lam * dp[1]) + L.bp[1]))) + (dp[2] * ((lam * dp[2]) + L.bp[2]));
}

// chi2 of the two edges of one point and whether its depth is positive in either frame
ORBFE_HD inline void ba_chi2(const PoseCam& G, const BaObs& O, const double (&Ra)[9], const double (&ta)[3], const double (&R)[9],
                             const double (&t)[3], const double (&X)[3], double& chiA, double& chiB, bool& frontA, bool& frontB)
{
    double x, y, z, e0, e1;
    EdgeD E{X[0], X[1], X[2], O.ox1, O.oy1, O.w1};
    edge_residual(G, E, Ra, ta, x, y, z, e0, e1, chiA);
    frontA = z > 0.0;
    E.ox = O.ox2;
    E.oy = O.oy2;
    E.w = O.w2;
    edge_residual(G, E, R, t, x, y, z, e0, e1, chiB);
    frontB = z > 0.0;
}

// rho0(edge 0) + rho0(edge 1) of one point
ORBFE_HD inline double ba_cost(const PoseCam& G, const BaObs& O, const double (&Ra)[9], const double (&ta)[3], const double (&R)[9],
                               const double (&t)[3], const double (&X)[3], bool huber)
{
    double chiA, chiB, ra, rb, rho1;
    bool fa, fb;
    ba_chi2(G, O, Ra, ta, R, t, X, chiA, chiB, fa, fb);
    robust(chiA, G.delta, huber, ra, rho1);
    robust(chiB, G.delta, huber, rb, rho1);
    return ra + rb;
}

}  // namespace orbfe

// poseopt_math.h -- what one thread computes for one edge of PoseOptimization (SPEC DECISION S14): the residual, the robust kernel, the
// 28 terms of H, b and the cost, and the pose update exp(dx) . (R, t).  Contraction is off in every including unit.
// No HIP here: kernels_poseopt.hip and tests/cpp/poseopt.cpp (as host C++) read this one text.
#pragma once
#include <cmath>

#include "host_device.h"
#include "mat3d.h"
#include "spec_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

constexpr int kNV = 28;                    // 21 of H (upper triangle, row by row), 6 of b, sum rho0

struct EdgeD {
    double X, Y, Z, ox, oy, w;
};

// the pinhole intrinsics and the Huber delta as the edges use them
struct PoseCam {
    double fx, fy, cx, cy, delta;
};

// Xc, the residual and chi2 of one edge at (R, t) (Pinhole.cpp:33-39)
ORBFE_HD inline void edge_residual(const PoseCam& G, const EdgeD& E, const double (&R)[9], const double (&t)[3], double& x,
                                   double& y, double& z, double& e0, double& e1, double& chi2)
{
    x = ((R[0] * E.X + R[1] * E.Y) + R[2] * E.Z) + t[0];
    y = ((R[3] * E.X + R[4] * E.Y) + R[5] * E.Z) + t[1];
    z = ((R[6] * E.X + R[7] * E.Y) + R[8] * E.Z) + t[2];
    const double u = G.fx * x / z + G.cx;
    const double v = G.fy * y / z + G.cy;
    e0 = E.ox - u;
    e1 = E.oy - v;
    chi2 = e0 * (E.w * e0) + e1 * (E.w * e1);
}

ORBFE_HD inline void robust(double chi2, double delta, bool huber, double& rho0, double& rho1)
{
    if (!huber || chi2 <= delta * delta) {
        rho0 = chi2;
        rho1 = 1.0;
    } else {
        const double s = sqrt(chi2);
        rho0 = 2.0 * s * delta - delta * delta;
        rho1 = delta / s;
    }
}

// the 28 terms of one active edge
ORBFE_HD inline void edge_terms(const PoseCam& G, const EdgeD& E, const double (&R)[9], const double (&t)[3], bool huber,
                                double (&v)[kNV])
{
    double x, y, z, e0, e1, chi2, rho0, rho1;
    edge_residual(G, E, R, t, x, y, z, e0, e1, chi2);
    robust(chi2, G.delta, huber, rho0, rho1);
    // J = -projectJac(Xc) SE3deriv (OptimizableTypes.cpp:57-62, Pinhole.cpp:69-79); the structural zeros are not multiplied
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
    for (int j = 0; j < 6; j++)
        ORBFE_UNROLL
        for (int k = j; k < 6; k++) v[at++] = (J0[j] * ww) * J0[k] + (J1[j] * ww) * J1[k];
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++) v[21 + j] = -(J0[j] * we0 + J1[j] * we1);
    v[27] = rho0;
}

// exp(dx) . (R, t) -> (Rn, tn): SE3Quat::exp as published, kept as matrices (S14)
ORBFE_HD inline void apply_update(const double (&dx)[6], const double (&R)[9], const double (&t)[3], double (&Rn)[9], double (&tn)[3])
{
    const double om[3] = {dx[0], dx[1], dx[2]}, up[3] = {dx[3], dx[4], dx[5]};
    const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
    const double Om[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    double Om2[9], Re[9], V[9];
    mul3d(Om, Om, Om2);
    if (theta < 1e-5) {
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) {
            Re[i] = (I[i] + Om[i]) + 0.5 * Om2[i];
            V[i] = (I[i] + 0.5 * Om[i]) + Om2[i] / 6.0;
        }
    } else {
        double s, c;
        spec_sincos64(theta, s, c);
        const double A = s / theta;
        const double B = (1.0 - c) / (theta * theta);
        const double C = (theta - s) / (theta * theta * theta);
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) {
            Re[i] = (I[i] + A * Om[i]) + B * Om2[i];
            V[i] = (I[i] + B * Om[i]) + C * Om2[i];
        }
    }
    double Rt[3], Vu[3];
    mul3d(Re, R, Rn);
    matvec3(Re, t, Rt);
    matvec3(V, up, Vu);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) tn[i] = Rt[i] + Vu[i];
}

}  // namespace orbfe

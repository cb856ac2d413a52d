// poseimu_math.h -- what one thread computes in PoseInertialOptimizationLastKeyFrame (SPEC DECISION S19): the four SO(3) functions of
// src/G2oTypes.cc:777-854 as binary64 sequences on spec_math.h's sin / cos / acos, the mono edge with the camera-body extrinsics
// (:375-395), the inertial edge (:514-594) and the two random-walk edges reduced to the columns of the free vertices, the assembly
// of the 15 x 15 system and ImuCamPose::Update (:192-220).  Contraction is off in every including unit.
// No HIP here: kernels_poseimu.hip and tests/cpp/pose_inertial.cpp (as host C++) read this one text.
// `Link` is orbfe_imu_link (include/orbfe.h) or anything with its fields: the constants are read where they are used.
#pragma once
#include <cmath>

#include "host_device.h"
#include "mat3d.h"
#include "poseopt_math.h"
#include "spec_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

constexpr int kImuN = 15;                  // rotation, translation, velocity, gyro bias, accelerometer bias: 3 each
constexpr int kImuState = 21;              // Rwb (9), twb, v, bg, ba

struct ImuState {
    double Rwb[9], twb[3], v[3], bg[3], ba[3];
    double Rcw[9], tcw[3];                 // the camera pose that goes with (Rwb, twb); the caller's own before the first update
};

// entry (a, c), a <= c, of a symmetric 9 x 9 kept as its upper triangle, row by row
ORBFE_HD constexpr int tri9(int a, int c) { return a * 9 - a * (a - 1) / 2 + (c - a); }
ORBFE_HD constexpr int sym9(int a, int c) { return a <= c ? tri9(a, c) : tri9(c, a); }
// entry (j, k), j <= k, of S14's 21 terms
ORBFE_HD constexpr int tri6(int j, int k) { return j * 6 - j * (j - 1) / 2 + (k - j); }

ORBFE_HD inline void hat3(double x, double y, double z, double (&W)[9])
{
    W[0] = 0.0; W[1] = -z; W[2] = y;
    W[3] = z; W[4] = 0.0; W[5] = -x;
    W[6] = -y; W[7] = x; W[8] = 0.0;
}

ORBFE_HD inline double eye3(int i) { return (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0; }

// ExpSO3 (:782-798) without NormalizeRotation (S19, departure 1)
ORBFE_HD inline void exp_so3(const double (&w)[3], double (&R)[9])
{
    const double d2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double d = sqrt(d2);
    double W[9], W2[9];
    hat3(w[0], w[1], w[2], W);
    mul3d(W, W, W2);
    if (d < 1e-5) {
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) R[i] = (eye3(i) + W[i]) + 0.5 * W2[i];
    } else {
        double s, c;
        spec_sincos64(d, s, c);
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) R[i] = (eye3(i) + W[i] * s / d) + W2[i] * (1.0 - c) / d2;
    }
}

// LogSO3 (:800-814)
ORBFE_HD inline void log_so3(const double (&R)[9], double (&w)[3])
{
    const double tr = (R[0] + R[4]) + R[8];
    w[0] = (R[7] - R[5]) / 2.0;
    w[1] = (R[2] - R[6]) / 2.0;
    w[2] = (R[3] - R[1]) / 2.0;
    const double costheta = (tr - 1.0) * 0.5;
    if (costheta > 1.0 || costheta < -1.0) return;
    const double theta = spec_acos64(costheta);
    double s, c;
    spec_sincos64(theta, s, c);
    if (fabs(s) < 1e-5) return;
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}

// InverseRightJacobianSO3 (:821-832)
ORBFE_HD inline void inverse_right_jacobian_so3(const double (&v)[3], double (&J)[9])
{
    const double d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double d = sqrt(d2);
    if (d < 1e-5) {
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) J[i] = eye3(i);
        return;
    }
    double W[9], W2[9], s, c;
    hat3(v[0], v[1], v[2], W);
    mul3d(W, W, W2);
    spec_sincos64(d, s, c);
    const double k = 1.0 / d2 - (1.0 + c) / (2.0 * d * s);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) J[i] = (eye3(i) + W[i] / 2.0) + W2[i] * k;
}

// RightJacobianSO3 (:839-854).  Only a fixed vertex's column of EdgeInertial uses it (:575), so the solver does not; it is pinned
// here with the other three for the last-frame variant.
ORBFE_HD inline void right_jacobian_so3(const double (&v)[3], double (&J)[9])
{
    const double d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double d = sqrt(d2);
    if (d < 1e-5) {
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) J[i] = eye3(i);
        return;
    }
    double W[9], W2[9], s, c;
    hat3(v[0], v[1], v[2], W);
    mul3d(W, W, W2);
    spec_sincos64(d, s, c);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) J[i] = (eye3(i) - W[i] * (1.0 - c) / d2) + W2[i] * (d - s) / (d2 * d);
}

// the 28 terms of one active mono edge (EdgeMonoOnlyPose, :375-395): S14's residual and kernel, the Jacobian
// projectJac(Xc) Rcb [-[Xb]x | I] with the sign as written; the structural zeros of projectJac and of SE3deriv are not multiplied
ORBFE_HD inline void imu_edge_terms(const PoseCam& G, const EdgeD& E, const double (&Rcw)[9], const double (&tcw)[3],
                                    const double (&Rcb)[9], const double (&tbc)[3], bool huber, double (&v)[kNV])
{
    double x, y, z, e0, e1, chi2, rho0, rho1;
    edge_residual(G, E, Rcw, tcw, x, y, z, e0, e1, chi2);
    robust(chi2, G.delta, huber, rho0, rho1);
    const double xb = ((Rcb[0] * x + Rcb[3] * y) + Rcb[6] * z) + tbc[0];   // Rbc = Rcb^T
    const double yb = ((Rcb[1] * x + Rcb[4] * y) + Rcb[7] * z) + tbc[1];
    const double zb = ((Rcb[2] * x + Rcb[5] * y) + Rcb[8] * z) + tbc[2];
    const double zz = z * z;
    const double a = G.fx / z;
    const double b = -G.fx * x / zz;
    const double c = G.fy / z;
    const double d = -G.fy * y / zz;
    double P0[3], P1[3];                   // projectJac(Xc) Rcb
    ORBFE_UNROLL
    for (int j = 0; j < 3; j++) {
        P0[j] = a * Rcb[j] + b * Rcb[6 + j];
        P1[j] = c * Rcb[3 + j] + d * Rcb[6 + j];
    }
    const double J0[6] = {P0[1] * -zb + P0[2] * yb, P0[0] * zb + P0[2] * -xb, P0[0] * -yb + P0[1] * xb, P0[0], P0[1], P0[2]};
    const double J1[6] = {P1[1] * -zb + P1[2] * yb, P1[0] * zb + P1[2] * -xb, P1[0] * -yb + P1[1] * xb, P1[0], P1[1], P1[2]};
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

// The inertial edge at the state S: its error e9 = (er, ev, ep) (:514-534) and J9^T info9 J9, -J9^T (info9 e9) over the nine
// columns of the free pose and velocity (:584-593).  J9 has three 3 x 3 blocks: invJr at rows 0-2 / columns 0-2, Rbw1 Rwb2 at rows
// 6-8 / columns 3-5, Rbw1 at rows 3-5 / columns 6-8; nothing else is multiplied.  Block (p, q), p <= q, of the product is
// B_p^T (info9[rows of p][rows of q] B_q), two 3 x 3 products; H9 is its upper triangle, row by row.
template <class Link>
ORBFE_HD inline void inertial_edge(const Link& K, double gravity, const ImuState& S, double (&H9)[45], double (&b9)[9], double (&e9)[9])
{
    double Rwb1[9], Rbw1[9], dR[9], dRt[9], A[9], eR[9];
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        Rwb1[i] = (double)K.Rwb1[i];
        dR[i] = (double)K.dR[i];
    }
    transpose3d(Rwb1, Rbw1);
    transpose3d(dR, dRt);
    mul3d(dRt, Rbw1, A);
    mul3d(A, S.Rwb, eR);
    double er[3];
    log_so3(eR, er);
    const double dt = (double)K.dt;
    const double g[3] = {0.0, 0.0, -gravity};
    double a[3], c[3], ra[3], rc[3];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        a[i] = (S.v[i] - (double)K.v1[i]) - g[i] * dt;
        c[i] = ((S.twb[i] - (double)K.twb1[i]) - (double)K.v1[i] * dt) - g[i] * dt * dt / 2.0;
    }
    matvec3(Rbw1, a, ra);
    matvec3(Rbw1, c, rc);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        e9[i] = er[i];
        e9[3 + i] = ra[i] - (double)K.dV[i];
        e9[6 + i] = rc[i] - (double)K.dP[i];
    }
    double B[3][9];                        // the blocks of J9 by column block
    inverse_right_jacobian_so3(er, B[0]);
    mul3d(Rbw1, S.Rwb, B[1]);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[2][i] = Rbw1[i];
    double Or[9];                          // -(info9 e9)
    ORBFE_UNROLL
    for (int r = 0; r < 9; r++) {
        double acc = K.info9[9 * r] * e9[0];
        ORBFE_UNROLL
        for (int q = 1; q < 9; q++) acc = acc + K.info9[9 * r + q] * e9[q];
        Or[r] = -acc;
    }
    ORBFE_UNROLL
    for (int p = 0; p < 3; p++) {
        const int rp = p == 0 ? 0 : (p == 1 ? 6 : 3);
        double Bt[9];
        transpose3d(B[p], Bt);
        ORBFE_UNROLL
        for (int i = 0; i < 3; i++) b9[3 * p + i] = (Bt[3 * i] * Or[rp] + Bt[3 * i + 1] * Or[rp + 1]) + Bt[3 * i + 2] * Or[rp + 2];
        ORBFE_UNROLL
        for (int q = p; q < 3; q++) {
            const int rq = q == 0 ? 0 : (q == 1 ? 6 : 3);
            double W[9], T[9], Hb[9];
            ORBFE_UNROLL
            for (int i = 0; i < 3; i++)
                ORBFE_UNROLL
                for (int j = 0; j < 3; j++) W[3 * i + j] = K.info9[9 * (rp + i) + (rq + j)];
            mul3d(W, B[q], T);
            mul3d(Bt, T, Hb);
            ORBFE_UNROLL
            for (int i = 0; i < 3; i++)
                ORBFE_UNROLL
                for (int j = 0; j < 3; j++)
                    if (q > p || j >= i) H9[tri9(3 * p + i, 3 * q + j)] = Hb[3 * i + j];
        }
    }
}

// The system of one iteration from the tree's 28 mono sums and the three other edges.  Order of the additions (S19): the mono sum
// first, the inertial term added to it -- H9[(j, k)] = acc + H9 for j <= k < 6, b[j] = acc[21 + j] + b9[j] for j < 6; b[6 .. 8] = b9;
// the random-walk edges (Jacobian I) give b[9 + i] = -(infoG (bg - bg1))_i, b[12 + i] = -(infoA (ba - ba1))_i, sums in column order.
// H is H9 in rows / columns 0-8 and the upper triangles of infoG and infoA, mirrored, in 9-11 and 12-14 (expand15).
template <class Link>
ORBFE_HD inline void imu_system(const Link& K, double gravity, const ImuState& S, const double (&acc)[kNV], double (&H9)[45],
                                double (&b)[kImuN])
{
    double b9[9], e9[9];
    inertial_edge(K, gravity, S, H9, b9, e9);
    ORBFE_UNROLL
    for (int j = 0; j < 6; j++) {
        ORBFE_UNROLL
        for (int k = j; k < 6; k++) H9[tri9(j, k)] = acc[tri6(j, k)] + H9[tri9(j, k)];
        b[j] = acc[21 + j] + b9[j];
    }
    ORBFE_UNROLL
    for (int j = 6; j < 9; j++) b[j] = b9[j];
    double eg[3], ea[3];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        eg[i] = S.bg[i] - (double)K.bg1[i];
        ea[i] = S.ba[i] - (double)K.ba1[i];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        b[9 + i] = -((K.infoG[3 * i] * eg[0] + K.infoG[3 * i + 1] * eg[1]) + K.infoG[3 * i + 2] * eg[2]);
        b[12 + i] = -((K.infoA[3 * i] * ea[0] + K.infoA[3 * i + 1] * ea[1]) + K.infoA[3 * i + 2] * ea[2]);
    }
}

// entry (i, j) of the 15 x 15 matrix of imu_system
template <class Link>
ORBFE_HD inline double imu_entry(const Link& K, const double (&H9)[45], int i, int j)
{
    if (i < 9 && j < 9) return H9[sym9(i, j)];
    if (i >= 9 && i < 12 && j >= 9 && j < 12) return i <= j ? K.infoG[3 * (i - 9) + (j - 9)] : K.infoG[3 * (j - 9) + (i - 9)];
    if (i >= 12 && j >= 12) return i <= j ? K.infoA[3 * (i - 12) + (j - 12)] : K.infoA[3 * (j - 12) + (i - 12)];
    return 0.0;
}

// ImuCamPose::Update (:192-220) and the three additive vertices; NormalizeRotation is not applied (S19, departure 1)
template <class Link>
ORBFE_HD inline void imu_update(const Link& K, const double (&dx)[kImuN], ImuState& S)
{
    const double ur[3] = {dx[0], dx[1], dx[2]}, ut[3] = {dx[3], dx[4], dx[5]};
    double Rut[3], E[9], Rn[9];
    matvec3(S.Rwb, ut, Rut);
    exp_so3(ur, E);
    mul3d(S.Rwb, E, Rn);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        S.twb[i] = S.twb[i] + Rut[i];
        S.v[i] = S.v[i] + dx[6 + i];
        S.bg[i] = S.bg[i] + dx[9 + i];
        S.ba[i] = S.ba[i] + dx[12 + i];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) S.Rwb[i] = Rn[i];
    double Rcb[9], Rbw[9], t[3], tbw[3], ct[3];
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) Rcb[i] = (double)K.Rcb[i];
    transpose3d(S.Rwb, Rbw);
    matvec3(Rbw, S.twb, t);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) tbw[i] = -t[i];
    mul3d(Rcb, Rbw, S.Rcw);
    matvec3(Rcb, tbw, ct);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) S.tcw[i] = ct[i] + (double)K.tcb[i];
}

// what the scoring after a round decides for one edge (:3686-3715): chi2 and the depth are those of edge_residual at the state
ORBFE_HD inline bool imu_edge_is_outlier(double chi2, double z, bool close, float thr, float thrClose)
{
    const float c = (float)chi2;
    return (c > thr && !close) || (close && c > thrClose) || !(z > 0.0);
}

}  // namespace orbfe

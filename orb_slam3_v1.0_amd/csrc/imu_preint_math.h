// imu_preint_math.h -- Tracking::PreintegrateIMU (src/Tracking.cc:242-277), IMU::Preintegrated (src/ImuTypes.cc:36-39, 86-107, 149-237,
// 285-312), Tracking::PredictStateIMU (src/Tracking.cc:293-350) with Frame::SetImuPoseVelocity (src/Frame.cc:221-238) and the
// informations of the inertial links (src/G2oTypes.cc:500-508; src/Optimizer.cc:3645,3652,4046,4053): SPEC DECISION S22.
// ONE text for kernels_imu_preint.hip (a wave), tests/cpp/imu_preint.cpp (one thread) and the host entry points, written over an
// executor X (marginalize.h: each / sync).  Inside one each() no item reads what another item of it writes.  Everything indexed at run
// time lives in PreintWork (LDS on the device).  binary32 where the C++ is float, binary64 where it is double; one IEEE operation per
// operator, left to right; a 3-term dot product is (a0 b0 + a1 b1) + a2 b2.  Contraction is off in every including unit.
#pragma once
#include <cmath>

#include "host_device.h"
#include "jacobi.h"
#include "marginalize.h"
#include "mat3d.h"
#include "poseimu_math.h"
#include "spec_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

constexpr int kPreintChunk = 32;           // steps staged at a time
constexpr int kPreintRecFloats = 298;      // dT .. C of a record
constexpr int kPreintFromKeyFrame = 0, kPreintFromFrame = 1;
constexpr float kPreintEps = 1e-4f;        // ImuTypes.cc:34
constexpr double kPreintClamp = 1e-12;     // G2oTypes.cc:505

// the float block of orbfe_imu_preint (include/orbfe.h), field for field
struct PreintRec {
    float dT;
    float bg[3], ba[3];
    float dR[9], dV[3], dP[3];
    float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    float avgA[3], avgW[3];
    float C[225];
};

struct PreintStep {
    float a[3], w[3];
    float dt, reserved;
};

struct PreintWork {
    PreintRec rec[2];                      // the key-frame record, the frame record
    PreintStep steps[kPreintChunk];
    float cov[6], walk[6];                 // the diagonals of Calib::Cov and Calib::CovWalk
    float A[9][9], B[9][6];                // of one step; A is block lower triangular, B has the blocks (0,0) (1,1) (2,1)
    float T[9][9];                         // A C
    double M[9][9], L[9][9], X[9][9], V[9][9];
    double c[4], s[4];
    int skip[4];
    int ok, pad;
};

ORBFE_HD inline void matvec3f(const float (&A)[9], const float (&x)[3], float (&o)[3])
{
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) o[i] = (A[3 * i] * x[0] + A[3 * i + 1] * x[1]) + A[3 * i + 2] * x[2];
}

ORBFE_HD inline void hat3f(const float (&v)[3], float (&W)[9])
{
    W[0] = 0.0f; W[1] = -v[2]; W[2] = v[1];
    W[3] = v[2]; W[4] = 0.0f; W[5] = -v[0];
    W[6] = -v[1]; W[7] = v[0]; W[8] = 0.0f;
}

ORBFE_HD inline float eye3f(int i) { return (i == 0 || i == 4 || i == 8) ? 1.0f : 0.0f; }

// NormalizeRotation (ImuTypes.cc:36-39).  Stated departure: the polar factor (float)(A (V diag(1 / sqrt(lambda_k)) V^T)) with V, lambda
// from jacobi3 on A^T A, everything in binary64 and rounded once per entry -- U V^T of the SVD in exact arithmetic for a full-rank A.
ORBFE_HD inline void normalize_rotation(const float (&A)[9], float (&R)[9])
{
    double Ad[9], G[3][3], V[3][3];
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) Ad[i] = (double)A[i];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) G[i][j] = (Ad[i] * Ad[j] + Ad[3 + i] * Ad[3 + j]) + Ad[6 + i] * Ad[6 + j];
    jacobi3(G, V);
    double is[3], P[9], Rd[9];
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) is[k] = 1.0 / sqrt(G[k][k]);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) P[3 * i + j] = ((V[i][0] * is[0]) * V[j][0] + (V[i][1] * is[1]) * V[j][1]) + (V[i][2] * is[2]) * V[j][2];
    mul3d(Ad, P, Rd);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) R[i] = (float)Rd[i];
}

// IntegratedRotation (ImuTypes.cc:86-107): v = (w - bg) dt; sin / cos are (float) of spec_sincos64((double) d)
ORBFE_HD inline void integrated_rotation(const float (&v)[3], float (&dR)[9], float (&rJ)[9], bool& small)
{
    const float d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const float d = sqrtf(d2);
    float W[9], W2[9];
    hat3f(v, W);
    small = d < kPreintEps;
    if (small) {
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) {
            dR[i] = eye3f(i) + W[i];
            rJ[i] = eye3f(i);
        }
        return;
    }
    mul3(W, W, W2);
    double sd, cd;
    spec_sincos64((double)d, sd, cd);
    const float s = (float)sd, c = (float)cd;
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        dR[i] = (eye3f(i) + W[i] * s / d) + W2[i] * (1.0f - c) / d2;
        rJ[i] = (eye3f(i) - W[i] * (1.0f - c) / d2) + W2[i] * (d - s) / (d2 * d);
    }
}

// Preintegrated::Initialize (ImuTypes.cc:149-168)
template <class Exec>
ORBFE_HD inline void preint_initialize(Exec& X, PreintRec& R, const float* bg, const float* ba)
{
    X.each(kPreintRecFloats, [&](int t) {
        float* f = &R.dT;
        float v = 0.0f;
        if (t >= 1 && t < 4) v = bg[t - 1];
        else if (t >= 4 && t < 7) v = ba[t - 4];
        else if (t >= 7 && t < 16) v = eye3f(t - 7);
        f[t] = v;
    });
}

// step i of PreintegrateIMU's loop (Tracking.cc:242-277) from samples i and i + 1; n = the number of steps.  Returns the branch.
template <class Sample>
ORBFE_HD inline int preint_step_from_samples(const Sample* S, int n, int i, double tPrev, double tCur, PreintStep& o)
{
    const Sample &p = S[i], &q = S[i + 1];
    int branch;
    float r = 0.0f;
    if (i == 0 && i < n - 1) {
        const float tab = (float)(q.t - p.t), tini = (float)(p.t - tPrev);
        r = tini / tab;
        o.dt = (float)(q.t - tPrev);
        branch = 0;
    } else if (i < n - 1) {
        o.dt = (float)(q.t - p.t);
        branch = 1;
    } else if (i > 0 && i == n - 1) {
        const float tab = (float)(q.t - p.t), tend = (float)(q.t - tCur);
        r = tend / tab;
        o.dt = (float)(tCur - p.t);
        branch = 2;
    } else {
        o.dt = (float)(tCur - tPrev);
        branch = 3;
    }
    ORBFE_UNROLL
    for (int k = 0; k < 3; k++) {
        if (branch == 0 || branch == 2) {
            o.a[k] = ((p.a[k] + q.a[k]) - (q.a[k] - p.a[k]) * r) * 0.5f;
            o.w[k] = ((p.w[k] + q.w[k]) - (q.w[k] - p.w[k]) * r) * 0.5f;
        } else if (branch == 1) {
            o.a[k] = (p.a[k] + q.a[k]) * 0.5f;
            o.w[k] = (p.w[k] + q.w[k]) * 0.5f;
        } else {
            o.a[k] = p.a[k];
            o.w[k] = p.w[k];
        }
    }
    o.reserved = 0.0f;
    return branch;
}

// the 3 x 3 chain of IntegrateNewMeasurement (ImuTypes.cc:179-237) in the reference's order; leaves A and B of the step in W.
// Returns whether IntegratedRotation took its small-angle branch.
ORBFE_HD inline bool preint_chain(PreintRec& R, PreintWork& W, const PreintStep& st)
{
    const float dt = st.dt;
    float acc[3], accW[3], dR[9], JRg[9];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        acc[i] = st.a[i] - R.ba[i];
        accW[i] = st.w[i] - R.bg[i];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        dR[i] = R.dR[i];
        JRg[i] = R.JRg[i];
    }
    float Ra[3], hdR[9], hRa[3];
    matvec3f(dR, acc, Ra);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) hdR[i] = 0.5f * dR[i];
    matvec3f(hdR, acc, hRa);
    const float dTn = R.dT + dt;
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        R.avgA[i] = (R.dT * R.avgA[i] + Ra[i] * dt) / dTn;
        R.avgW[i] = (R.dT * R.avgW[i] + accW[i] * dt) / dTn;
        R.dP[i] = (R.dP[i] + R.dV[i] * dt) + hRa[i] * dt * dt;
        R.dV[i] = R.dV[i] + Ra[i] * dt;
    }
    float Wacc[9], dRdt[9], ndRdt[9], hh[9], nhh[9], A10[9], A20[9], K1[9], K2[9];
    hat3f(acc, Wacc);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        dRdt[i] = dR[i] * dt;
        ndRdt[i] = -dR[i] * dt;
        hh[i] = hdR[i] * dt * dt;
        nhh[i] = -0.5f * dR[i] * dt * dt;
    }
    mul3(ndRdt, Wacc, A10);
    mul3(nhh, Wacc, A20);
    mul3(hh, Wacc, K1);
    mul3(K1, JRg, K2);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        R.JPa[i] = (R.JPa[i] + R.JVa[i] * dt) - hh[i];
        R.JPg[i] = (R.JPg[i] + R.JVg[i] * dt) - K2[i];
        R.JVa[i] = R.JVa[i] - dRdt[i];
    }
    mul3(dRdt, Wacc, K1);
    mul3(K1, JRg, K2);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) R.JVg[i] = R.JVg[i] - K2[i];
    float v[3], dRi[9], rJ[9], dRiT[9], prod[9], nR[9];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) v[i] = accW[i] * dt;
    bool small;
    integrated_rotation(v, dRi, rJ, small);
    mul3(dR, dRi, prod);
    normalize_rotation(prod, nR);
    transpose3(dRi, dRiT);
    mul3(dRiT, JRg, K1);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        R.dR[i] = nR[i];
        R.JRg[i] = K1[i] - rJ[i] * dt;
    }
    R.dT = dTn;
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) {
            const int e = 3 * i + j;
            const float I = i == j ? 1.0f : 0.0f;
            W.A[i][j] = dRiT[e];
            W.A[i][3 + j] = 0.0f;
            W.A[i][6 + j] = 0.0f;
            W.A[3 + i][j] = A10[e];
            W.A[3 + i][3 + j] = I;
            W.A[3 + i][6 + j] = 0.0f;
            W.A[6 + i][j] = A20[e];
            W.A[6 + i][3 + j] = i == j ? dt : 0.0f;
            W.A[6 + i][6 + j] = I;
            W.B[i][j] = rJ[e] * dt;
            W.B[i][3 + j] = 0.0f;
            W.B[3 + i][j] = 0.0f;
            W.B[3 + i][3 + j] = dRdt[e];
            W.B[6 + i][j] = 0.0f;
            W.B[6 + i][3 + j] = hh[e];
        }
    return small;
}

// IntegrateNewMeasurement.  The covariance: T = A C over the block columns bk <= bi of A in ascending order, each block a 3-term dot
// product, the blocks' results added left to right; U = T A^T over bk <= bj the same way; B Nga B^T where the two rows share a block
// column of B (bk = 0 for rows 0-2, bk = 1 for rows 3-8), ((B_ik n_k) B_jk) as a 3-term dot product; C' = U + that, or U alone.  Then
// the six diagonal entries of C.block<6,6>(9,9) take NgaWalk.  An absent block is never multiplied.
template <class Exec>
ORBFE_HD inline void preint_integrate(Exec& X, PreintWork& W, PreintRec& R, const PreintStep& st, bool* small = nullptr)
{
    X.each(1, [&](int) {
        const bool sm = preint_chain(R, W, st);
        if (small) *small = sm;
    });
    X.each(81, [&](int t) {
        const int i = t / 9, j = t % 9, bi = i / 3;
        float acc = 0.0f;
        for (int bk = 0; bk <= bi; bk++) {
            const int k = 3 * bk;
            const float term = (W.A[i][k] * R.C[15 * k + j] + W.A[i][k + 1] * R.C[15 * (k + 1) + j]) + W.A[i][k + 2] * R.C[15 * (k + 2) + j];
            acc = bk == 0 ? term : acc + term;
        }
        W.T[i][j] = acc;
    });
    X.each(87, [&](int t) {
        if (t >= 81) {
            const int k = 9 + (t - 81);
            R.C[15 * k + k] = R.C[15 * k + k] + W.walk[t - 81];
            return;
        }
        const int i = t / 9, j = t % 9, bi = i / 3, bj = j / 3;
        float acc = 0.0f;
        for (int bk = 0; bk <= bj; bk++) {
            const int k = 3 * bk;
            const float term = (W.T[i][k] * W.A[j][k] + W.T[i][k + 1] * W.A[j][k + 1]) + W.T[i][k + 2] * W.A[j][k + 2];
            acc = bk == 0 ? term : acc + term;
        }
        if ((bi == 0) == (bj == 0)) {
            const int k = bi == 0 ? 0 : 3;
            const float q = ((W.B[i][k] * W.cov[k]) * W.B[j][k] + (W.B[i][k + 1] * W.cov[k + 1]) * W.B[j][k + 1]) +
                            (W.B[i][k + 2] * W.cov[k + 2]) * W.B[j][k + 2];
            acc = acc + q;
        }
        R.C[15 * i + j] = acc;
    });
}

// GetDeltaRotation / Velocity / Position (bg, ba) (ImuTypes.cc:285-312); the rotation is S20's departure, then rounded and normalised
ORBFE_HD inline void preint_deltas(const PreintRec& R, const float* bg, const float* ba, float (&dRb)[9], float (&dVb)[3], float (&dPb)[3])
{
    float dbg[3], dba[3], rot[3], t1[3], t2[3], t3[3], t4[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        dbg[i] = bg[i] - R.bg[i];
        dba[i] = ba[i] - R.ba[i];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        JRg[i] = R.JRg[i];
        JVg[i] = R.JVg[i];
        JVa[i] = R.JVa[i];
        JPg[i] = R.JPg[i];
        JPa[i] = R.JPa[i];
    }
    matvec3f(JRg, dbg, rot);
    matvec3f(JVg, dbg, t1);
    matvec3f(JVa, dba, t2);
    matvec3f(JPg, dbg, t3);
    matvec3f(JPa, dba, t4);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        dVb[i] = (R.dV[i] + t1[i]) + t2[i];
        dPb[i] = (R.dP[i] + t3[i]) + t4[i];
    }
    const double rd[3] = {(double)rot[0], (double)rot[1], (double)rot[2]};
    double E[9], D[9], P[9];
    float Pf[9];
    exp_so3(rd, E);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) D[i] = (double)R.dR[i];
    mul3d(D, E, P);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) Pf[i] = (float)P[i];
    normalize_rotation(Pf, dRb);
}

// SetImuPoseVelocity (Frame.cc:221-238): Rcw = Rcb Rwb^T, tcw = Rcb (-(Rwb^T twb)) + tcb.  One text for the prediction below and for
// the pose TrackLocalMap hands on after the inertial optimisation (kernels_track_inertial.hip, SPEC DECISION S23).
ORBFE_HD inline void set_imu_pose(const float (&Rwb)[9], const float (&twb)[3], const float (&Rcb)[9], const float* tcb, float (&Rcw)[9],
                                  float (&tcw)[3])
{
    float Rbw[9], t[3], nt[3], ct[3];
    transpose3(Rwb, Rbw);
    mul3(Rcb, Rbw, Rcw);
    matvec3f(Rbw, twb, t);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) nt[i] = -t[i];
    matvec3f(Rcb, nt, ct);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) tcw[i] = ct[i] + tcb[i];
}

// PredictStateIMU (Tracking.cc:293-350) and SetImuPoseVelocity (Frame.cc:221-238).  s1 = Rwb1 (9) twb1 v1 bg1 ba1; out = Rcw (9) tcw
// Rwb twb v bg ba, the biases being the start's (:323, :345).
ORBFE_HD inline void preint_predict(const float* s1, const float (&dRb)[9], const float (&dVb)[3], const float (&dPb)[3], float t12,
                                    float gravity, const float* Rcb_, const float* tcb, float* out)
{
    float Rwb1[9], Rcb[9], prod[9], Rwb2[9], Rcw[9], rp[3], rv[3], twb2[3], v2[3], tcw[3];
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        Rwb1[i] = s1[i];
        Rcb[i] = Rcb_[i];
    }
    const float g[3] = {0.0f, 0.0f, -gravity};
    mul3(Rwb1, dRb, prod);
    normalize_rotation(prod, Rwb2);
    matvec3f(Rwb1, dPb, rp);
    matvec3f(Rwb1, dVb, rv);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        twb2[i] = ((s1[9 + i] + s1[12 + i] * t12) + 0.5f * t12 * t12 * g[i]) + rp[i];
        v2[i] = (s1[12 + i] + t12 * g[i]) + rv[i];
    }
    set_imu_pose(Rwb2, twb2, Rcb, tcb, Rcw, tcw);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        out[i] = Rcw[i];
        out[12 + i] = Rwb2[i];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        out[9 + i] = tcw[i];
        out[21 + i] = twb2[i];
        out[24 + i] = v2[i];
        out[27 + i] = s1[15 + i];
        out[30 + i] = s1[18 + i];
    }
}

// EdgeInertial's information (G2oTypes.cc:500-508) of C.block<9,9>(0,0) -> info9 (81, row-major); returns info_ok.
// Stated departures: the inverse is L D L^T without pivoting of the upper triangle, mirrored, solved against the nine unit vectors
// (Eigen: partial-pivot LU of the whole matrix); the eigen-decomposition is S12's n = 9 Jacobi sequence (Eigen:
// SelfAdjointEigenSolver).  Step k of the factor: row i > k takes l_ik = M_ik / d_k (0 when d_k == 0) and M_ij -= l_ik M_jk for
// j = k + 1 .. i.  Column c: z_i = e_i - sum_{j < i} l_ij z_j, j ascending; w_i = z_i / d_i (0 when d_i == 0); x_i = w_i -
// sum_{j > i} l_ji x_j, i descending, j ascending.  Then (X + X^T) / 2, the rounds of jacobi_rounds_block, lambda < 1e-12 -> 0 and
// V diag(lambda) V^T as sequential sums of (V_ik lambda_k) V_jk, k ascending.
template <class Exec>
ORBFE_HD inline bool preint_info9(Exec& X, PreintWork& W, const float* C, double* info9, int* clamped = nullptr)
{
    constexpr int N = 9;
    X.each(N * N, [&](int t) {
        const int i = t / N, j = t % N;
        W.M[i][j] = (double)C[15 * (i < j ? i : j) + (i < j ? j : i)];
    });
    for (int k = 0; k < N - 1; k++)
        X.each(N, [&](int i) {
            if (i <= k) return;
            const double dk = W.M[k][k];
            const double li = dk == 0.0 ? 0.0 : W.M[i][k] / dk;
            W.L[i][k] = li;
            for (int j = k + 1; j <= i; j++) W.M[i][j] = W.M[i][j] - li * W.M[j][k];
        });
    X.each(N, [&](int c) {
        for (int i = 0; i < N; i++) {
            double acc = i == c ? 1.0 : 0.0;
            for (int j = 0; j < i; j++) acc = acc - W.L[i][j] * W.X[j][c];
            W.X[i][c] = acc;
        }
        for (int i = 0; i < N; i++) {
            const double d = W.M[i][i];
            W.X[i][c] = d == 0.0 ? 0.0 : W.X[i][c] / d;
        }
        for (int i = N - 1; i >= 0; i--) {
            double acc = W.X[i][c];
            for (int j = i + 1; j < N; j++) acc = acc - W.L[j][i] * W.X[j][c];
            W.X[i][c] = acc;
        }
        if (c == 0) {
            bool pos = true;
            for (int i = 0; i < N; i++) pos = pos && W.M[i][i] > 0.0;
            W.ok = pos ? 1 : 0;
        }
    });
    const bool ok = W.ok != 0;
    X.each(N * N, [&](int t) {
        const int i = t / N, j = t % N;
        W.V[i][j] = i == j ? 1.0 : 0.0;
        W.M[i][j] = (W.X[i][j] + W.X[j][i]) / 2.0;
    });
    for (int sweep = 0; sweep < kTwoViewSweeps; sweep++)
        for (int r = 0; r < N; r++) {
            X.each(4, [&](int e) {
                int p, q;
                jacobi_round_pair(N, r, e, p, q);
                const double apq = W.M[p][q];
                const int skip = apq == 0.0;
                double c = 1.0, sn = 0.0;
                if (!skip) jacobi_angle(W.M[p][p], W.M[q][q], apq, c, sn);
                W.c[e] = c;
                W.s[e] = sn;
                W.skip[e] = skip;
            });
            X.each(4 * N, [&](int e) {   // columns p, q of M
                const int pr = e / N, k = e % N;
                if (W.skip[pr]) return;
                int p, q;
                jacobi_round_pair(N, r, pr, p, q);
                const double c = W.c[pr], sn = W.s[pr];
                const double a = W.M[k][p], b = W.M[k][q];
                W.M[k][p] = c * a - sn * b;
                W.M[k][q] = sn * a + c * b;
            });
            X.each(4 * N, [&](int e) {   // rows p, q of M; columns p, q of V
                const int pr = e / N, k = e % N;
                if (W.skip[pr]) return;
                int p, q;
                jacobi_round_pair(N, r, pr, p, q);
                const double c = W.c[pr], sn = W.s[pr];
                const double a = W.M[p][k], b = W.M[q][k];
                W.M[p][k] = c * a - sn * b;
                W.M[q][k] = sn * a + c * b;
                const double va = W.V[k][p], vb = W.V[k][q];
                W.V[k][p] = c * va - sn * vb;
                W.V[k][q] = sn * va + c * vb;
            });
        }
    X.each(N * N, [&](int t) {
        const int i = t / N, j = t % N;
        double acc = 0.0;
        for (int k = 0; k < N; k++) {
            const double lam = W.M[k][k] < kPreintClamp ? 0.0 : W.M[k][k];
            const double term = (W.V[i][k] * lam) * W.V[j][k];
            acc = k == 0 ? term : acc + term;
        }
        info9[N * i + j] = acc;
    });
    if (clamped) {
        int n = 0;
        for (int k = 0; k < N; k++) n += W.M[k][k] < kPreintClamp ? 1 : 0;
        *clamped = n;
    }
    return ok;
}

// C.block<3,3>(at, at).cast<double>().inverse() (Optimizer.cc:3645,3652,4046,4053): mat3d.h::inv3_sym of the upper triangle, mirrored
ORBFE_HD inline void preint_info3(const float* C, int at, double* o)
{
    const double a[6] = {(double)C[15 * at + at],           (double)C[15 * at + at + 1],       (double)C[15 * at + at + 2],
                         (double)C[15 * (at + 1) + at + 1], (double)C[15 * (at + 1) + at + 2], (double)C[15 * (at + 2) + at + 2]};
    double s[6];
    inv3_sym(a, s);
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    o[3] = s[1]; o[4] = s[3]; o[5] = s[4];
    o[6] = s[2]; o[7] = s[4]; o[8] = s[5];
}

// The prediction and the link of one frame.  `which` picks the record the prediction and the link are taken from (W.rec[0]: the
// key-frame record, W.rec[1]: the frame record); infoG / infoA always come from the key-frame record (Optimizer.cc:3645, :4046).
// LinkKf is orbfe_imu_link, LinkFree orbfe_imu_link_free; exactly one of the two pointers is read, by `which`.
template <class Exec, class LinkKf, class LinkFree>
ORBFE_HD inline void preint_predict_link(Exec& X, PreintWork& W, int which, const float* s1, float gravity, const float* Rcb, const float* tcb,
                                         const float* tbc, float* stateOut, LinkKf* lk, LinkFree* lf, int* infoOk, int* clamped = nullptr)
{
    const PreintRec& R = W.rec[which == kPreintFromFrame ? 1 : 0];
    const PreintRec& Rk = W.rec[0];
    double* info9 = which == kPreintFromFrame ? lf->info9 : lk->info9;
    const bool ok = preint_info9(X, W, R.C, info9, clamped);
    X.each(1, [&](int) {
        float dRb[9], dVb[3], dPb[3];
        preint_deltas(R, s1 + 15, s1 + 18, dRb, dVb, dPb);
        preint_predict(s1, dRb, dVb, dPb, R.dT, gravity, Rcb, tcb, stateOut);
        *infoOk = ok ? 1 : 0;
        if (which == kPreintFromFrame) {
            lf->struct_size = (int)sizeof(LinkFree);
            lf->reserved = 0;
            lf->reserved2 = 0.0f;
            lf->dt = R.dT;
            ORBFE_UNROLL
            for (int i = 0; i < 9; i++) {
                lf->Rwb1[i] = s1[i];
                lf->dR0[i] = R.dR[i];
                lf->JRg[i] = R.JRg[i];
                lf->JVg[i] = R.JVg[i];
                lf->JVa[i] = R.JVa[i];
                lf->JPg[i] = R.JPg[i];
                lf->JPa[i] = R.JPa[i];
                lf->Rcb[i] = Rcb[i];
            }
            ORBFE_UNROLL
            for (int i = 0; i < 3; i++) {
                lf->twb1[i] = s1[9 + i];
                lf->v1[i] = s1[12 + i];
                lf->bg1[i] = s1[15 + i];
                lf->ba1[i] = s1[18 + i];
                lf->dV0[i] = R.dV[i];
                lf->dP0[i] = R.dP[i];
                lf->bg0[i] = R.bg[i];
                lf->ba0[i] = R.ba[i];
                lf->tcb[i] = tcb[i];
                lf->tbc[i] = tbc[i];
            }
            preint_info3(Rk.C, 9, lf->infoG);
            preint_info3(Rk.C, 12, lf->infoA);
        } else {
            lk->struct_size = (int)sizeof(LinkKf);
            lk->reserved = 0;
            lk->dt = R.dT;
            ORBFE_UNROLL
            for (int i = 0; i < 9; i++) {
                lk->Rwb1[i] = s1[i];
                lk->dR[i] = dRb[i];
                lk->Rcb[i] = Rcb[i];
            }
            ORBFE_UNROLL
            for (int i = 0; i < 3; i++) {
                lk->twb1[i] = s1[9 + i];
                lk->v1[i] = s1[12 + i];
                lk->bg1[i] = s1[15 + i];
                lk->ba1[i] = s1[18 + i];
                lk->dV[i] = dVb[i];
                lk->dP[i] = dPb[i];
                lk->tcb[i] = tcb[i];
                lk->tbc[i] = tbc[i];
            }
            preint_info3(Rk.C, 9, lk->infoG);
            preint_info3(Rk.C, 12, lk->infoA);
        }
    });
}

}  // namespace orbfe

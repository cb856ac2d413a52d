// poseimu_prev_math.h -- Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:3846-4275) for the branch this fork takes,
// SPEC DECISION S20: 30 unknowns (the frame's and the previous frame's rotation, translation, velocity, gyro bias, accelerometer
// bias), the EdgeInertial with all six vertices free and preintegrated deltas that follow the unknown biases (src/G2oTypes.cc:514-594,
// src/ImuTypes.cc:278-312), EdgeGyroRW, EdgeAccRW, EdgePriorPoseImu under its Huber kernel (:720-760), the Gauss-Newton loop, the
// 30 x 30 Hessian and its marginalisation (marginalize.h).
// The whole call is ONE text, prev_solve, written over an executor X (see marginalize.h: each / sync) that also supplies what differs
// between one thread and a block: the tree sums over the mono edges, the scoring and the 30 x 30 solve.  kernels_poseimu_prev.hip runs
// it with a block, tests/cpp/pose_inertial_prev.cpp with one thread; what is indexed at run time lives in PrevWork (LDS on the device).
// `Link` is orbfe_imu_link_free, `Prior` orbfe_pose_imu_prior (include/orbfe.h) or anything with their fields.
// Contraction is off in every including unit.
#pragma once
#include <cmath>

#include "host_device.h"
#include "marginalize.h"
#include "poseimu_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// a loop over the present blocks stays a loop on the device: unrolled, its loads are hoisted together and the registers run out
#if defined(__HIPCC__)
#define ORBFE_PREV_LOOP _Pragma("nounroll")
#else
#define ORBFE_PREV_LOOP
#endif

namespace orbfe {

constexpr int kPrevN = 30;                 // solver order: the frame 0-14, the previous frame 15-29 (g2o vertex ids 0-3, 4-7)
constexpr int kPrevLd = 31;                // row stride of A and L in doubles: 62 words, rows of 30 lanes fall on 30 distinct bank pairs
constexpr int kPrevState = 42;             // the frame's 21 (Rwb, twb, v, bg, ba), then the previous frame's 21
constexpr int kPrevH = kPrevN * kPrevN;

struct PrevState {
    ImuState cur, prv;                     // prv.Rcw / prv.tcw are never read
};

struct PrevPar {
    double gravity, priorDelta;
    float chi2[4], chi2Close[4];
    float recoverChi2;
    int recoverBelow, recInit, iterations, nRounds, inlierThreshold;
};

struct PrevRoundsOut {
    int Ne, roundsRun, recovered, pad;
    int iterations[4], ok[4], nBad[4];
    double state[4][kPrevState];
    double priorChi2[4], priorWeight[4];
};

struct PrevOut {
    float* state;                          // 21
    double* H30;                           // 900, reference order
    double* Hprior;                        // 225, nullable: the marginalisation is skipped
    int* nInliers;
    int* accepted;
    PrevRoundsOut* rounds;                 // nullable
};

struct PrevWork {
    double acc[kNV];                       // the mono tree sums
    double J[3][8][9];                     // EdgeInertial's Jacobian by 3 x 3 block: row block (er, ev, ep), column block in the
                                           // reference's order (pose 1 rotation, translation, v1, bg1, ba1, pose 2 rotation, translation, v2)
    double Or9[9];                         // -(info9 e9)
    double H24[24][24], b24[24];           // J^T info9 J and -J^T info9 e9, reference order
    double Jp[2][9], Orw[15];              // the prior's two general blocks, w * -(H e)
    double pw[3];                          // the prior's chi2, its Huber weight, the weight in use
    double Hp[15][15], bp[15];
    double rwG[3], rwA[3];                 // infoG (bg2 - bg1), infoA (ba2 - ba1)
    double A[kPrevN][kPrevLd], L[kPrevN][kPrevLd];
    double b[kPrevN], dx[kPrevN], d[kPrevN];
    int perm[kPrevN];
    int ok, pad;
    double H30[kPrevH];
    MargWork mg;
};

// bit r of nibble c: row block r of column block c is present
ORBFE_HD inline bool prev_j_present(int r, int c)
{
    constexpr unsigned mask = 7u | (4u << 3) | (6u << 6) | (7u << 9) | (6u << 12) | (1u << 15) | (4u << 18) | (2u << 21);
    return ((mask >> (3 * c + r)) & 1u) != 0;
}
// solver index -> index in the reference's 24 of the inertial edge (-1: the frame's biases, which it does not touch)
ORBFE_HD inline int prev_ref24(int i) { return i < 9 ? 15 + i : (i < 15 ? -1 : i - 15); }
// t-th pair (p, q), p <= q < n, row by row
ORBFE_HD inline void prev_pair(int n, int t, int& p, int& q)
{
    p = 0;
    while (t >= n - p) { t -= n - p; p++; }
    q = p + t;
}

template <class Work>
ORBFE_HD inline void prev_store_block(Work& W, int r, int c, const double (&B)[9])
{
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) W.J[r][c][i] = B[i];
}

// EdgeInertial at the state: the deltas at the previous frame's biases (ImuTypes.cc:285-312), the error (:528-531) and the blocks of
// linearizeOplus (:558-593)
template <class Link, class Work>
ORBFE_HD inline void prev_inertial_lin(const Link& K, double gravity, const PrevState& S, Work& W)
{
    float dbg[3], dba[3];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        dbg[i] = (float)S.prv.bg[i] - K.bg0[i];
        dba[i] = (float)S.prv.ba[i] - K.ba0[i];
    }
    double dV[3], dP[3], rot[3], dbgd[3];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        const float vg = (K.JVg[3 * i] * dbg[0] + K.JVg[3 * i + 1] * dbg[1]) + K.JVg[3 * i + 2] * dbg[2];
        const float va = (K.JVa[3 * i] * dba[0] + K.JVa[3 * i + 1] * dba[1]) + K.JVa[3 * i + 2] * dba[2];
        const float pg = (K.JPg[3 * i] * dbg[0] + K.JPg[3 * i + 1] * dbg[1]) + K.JPg[3 * i + 2] * dbg[2];
        const float pa = (K.JPa[3 * i] * dba[0] + K.JPa[3 * i + 1] * dba[1]) + K.JPa[3 * i + 2] * dba[2];
        const float rl = (K.JRg[3 * i] * dbg[0] + K.JRg[3 * i + 1] * dbg[1]) + K.JRg[3 * i + 2] * dbg[2];
        dV[i] = (double)((K.dV0[i] + vg) + va);
        dP[i] = (double)((K.dP0[i] + pg) + pa);
        rot[i] = (double)rl;
        dbgd[i] = (double)dbg[i];
    }
    double dR0[9], JRg[9], E[9], dR[9];
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        dR0[i] = (double)K.dR0[i];
        JRg[i] = (double)K.JRg[i];
    }
    exp_so3(rot, E);
    mul3d(dR0, E, dR);   // S20's stated departure: binary64, no NormalizeRotation
    double Rbw1[9], Rbw2[9], dRt[9], T[9], eR[9], eRt[9], er[3];
    transpose3d(S.prv.Rwb, Rbw1);
    transpose3d(S.cur.Rwb, Rbw2);
    transpose3d(dR, dRt);
    mul3d(dRt, Rbw1, T);
    mul3d(T, S.cur.Rwb, eR);
    log_so3(eR, er);
    const double dt = (double)K.dt;
    const double g[3] = {0.0, 0.0, -gravity};
    double a[3], c[3], c2[3], ra[3], rc[3], rc2[3], e9[9];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        a[i] = (S.cur.v[i] - S.prv.v[i]) - g[i] * dt;
        const double base = (S.cur.twb[i] - S.prv.twb[i]) - S.prv.v[i] * dt;
        c[i] = base - g[i] * dt * dt / 2.0;     // computeError (:530-531)
        c2[i] = base - 0.5 * g[i] * dt * dt;    // linearizeOplus (:563-564)
    }
    matvec3(Rbw1, a, ra);
    matvec3(Rbw1, c, rc);
    matvec3(Rbw1, c2, rc2);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        e9[i] = er[i];
        e9[3 + i] = ra[i] - dV[i];
        e9[6 + i] = rc[i] - dP[i];
    }
    ORBFE_UNROLL
    for (int r = 0; r < 9; r++) {
        double acc = K.info9[9 * r] * e9[0];
        ORBFE_UNROLL
        for (int q = 1; q < 9; q++) acc = acc + K.info9[9 * r + q] * e9[q];
        W.Or9[r] = -acc;
    }
    double invJr[9], nInv[9], B[9], T2[9], Jr[9], rj[3];
    inverse_right_jacobian_so3(er, invJr);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) nInv[i] = -invJr[i];
    mul3d(nInv, Rbw2, T);
    mul3d(T, S.prv.Rwb, B);
    prev_store_block(W, 0, 0, B);          // -invJr Rwb2^T Rwb1
    hat3(ra[0], ra[1], ra[2], B);
    prev_store_block(W, 1, 0, B);
    hat3(rc2[0], rc2[1], rc2[2], B);
    prev_store_block(W, 2, 0, B);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -eye3(i);
    prev_store_block(W, 2, 1, B);          // -I
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -Rbw1[i];
    prev_store_block(W, 1, 2, B);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -Rbw1[i] * dt;
    prev_store_block(W, 2, 2, B);
    transpose3d(eR, eRt);
    mul3d(nInv, eRt, T);
    matvec3(JRg, dbgd, rj);
    right_jacobian_so3(rj, Jr);
    mul3d(T, Jr, T2);
    mul3d(T2, JRg, B);
    prev_store_block(W, 0, 3, B);          // -invJr eR^T Jr(JRg dbg) JRg
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -(double)K.JVg[i];
    prev_store_block(W, 1, 3, B);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -(double)K.JPg[i];
    prev_store_block(W, 2, 3, B);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -(double)K.JVa[i];
    prev_store_block(W, 1, 4, B);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) B[i] = -(double)K.JPa[i];
    prev_store_block(W, 2, 4, B);
    prev_store_block(W, 0, 5, invJr);
    mul3d(Rbw1, S.cur.Rwb, B);
    prev_store_block(W, 2, 6, B);
    prev_store_block(W, 1, 7, Rbw1);
}

// block pair (p, q), p <= q, of J^T info9 J: the present row blocks in ascending order (rp, then rq), each term
// J[rp][p]^T (info9[rp][rq] J[rq][q]); of a diagonal pair the upper triangle, mirrored
template <class Link, class Work>
ORBFE_HD inline void prev_inertial_pair(const Link& K, Work& W, int p, int q)
{
    double Hb[9];
    ORBFE_UNROLL
    for (int e = 0; e < 9; e++) Hb[e] = 0.0;
    bool first = true;
    ORBFE_PREV_LOOP
    for (int rp = 0; rp < 3; rp++) {
        if (!prev_j_present(rp, p)) continue;
        double Jp[9], Jt[9];
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) Jp[e] = W.J[rp][p][e];
        transpose3d(Jp, Jt);
        ORBFE_PREV_LOOP
        for (int rq = 0; rq < 3; rq++) {
            if (!prev_j_present(rq, q)) continue;
            double Om[9], Jq[9], T[9], M[9];
            ORBFE_UNROLL
            for (int i = 0; i < 3; i++)
                ORBFE_UNROLL
                for (int j = 0; j < 3; j++) Om[3 * i + j] = K.info9[9 * (3 * rp + i) + (3 * rq + j)];
            ORBFE_UNROLL
            for (int e = 0; e < 9; e++) Jq[e] = W.J[rq][q][e];
            mul3d(Om, Jq, T);
            mul3d(Jt, T, M);
            ORBFE_UNROLL
            for (int e = 0; e < 9; e++) Hb[e] = first ? M[e] : Hb[e] + M[e];
            first = false;
        }
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++)
            if (q > p || j >= i) {
                W.H24[3 * p + i][3 * q + j] = Hb[3 * i + j];
                W.H24[3 * q + j][3 * p + i] = Hb[3 * i + j];
            }
}

template <class Work>
ORBFE_HD inline void prev_inertial_b(Work& W, int c)
{
    double acc[3] = {0.0, 0.0, 0.0};
    bool first = true;
    ORBFE_PREV_LOOP
    for (int rp = 0; rp < 3; rp++) {
        if (!prev_j_present(rp, c)) continue;
        double Jp[9], Jt[9], t[3];
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) Jp[e] = W.J[rp][c][e];
        transpose3d(Jp, Jt);
        const double o[3] = {W.Or9[3 * rp], W.Or9[3 * rp + 1], W.Or9[3 * rp + 2]};
        matvec3(Jt, o, t);
        ORBFE_UNROLL
        for (int i = 0; i < 3; i++) acc[i] = first ? t[i] : acc[i] + t[i];
        first = false;
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) W.b24[3 * c + i] = acc[i];
}

// EdgePriorPoseImu at the state (:731-760): error, chi2 = e^T (H e), S14's robust with delta; unit: the weight in use is 1
template <class Prior, class Work>
ORBFE_HD inline void prev_prior_lin(const Prior& Pr, double delta, bool unit, const PrevState& S, Work& W)
{
    double Rp[9], Rpt[9], Rr[9], er[3], d[3], et[3], e[15];
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) Rp[i] = Pr.Rwb[i];
    transpose3d(Rp, Rpt);
    mul3d(Rpt, S.prv.Rwb, Rr);
    log_so3(Rr, er);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) d[i] = S.prv.twb[i] - Pr.twb[i];
    matvec3(Rpt, d, et);
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        e[i] = er[i];
        e[3 + i] = et[i];
        e[6 + i] = S.prv.v[i] - Pr.vwb[i];
        e[9 + i] = S.prv.bg[i] - Pr.bg[i];
        e[12 + i] = S.prv.ba[i] - Pr.ba[i];
    }
    double He[15];
    ORBFE_UNROLL
    for (int r = 0; r < 15; r++) {
        double acc = Pr.H[15 * r] * e[0];
        ORBFE_UNROLL
        for (int q = 1; q < 15; q++) acc = acc + Pr.H[15 * r + q] * e[q];
        He[r] = acc;
    }
    double chi2 = e[0] * He[0];
    ORBFE_UNROLL
    for (int r = 1; r < 15; r++) chi2 = chi2 + e[r] * He[r];
    double rho0, rho1;
    robust(chi2, delta, true, rho0, rho1);
    const double w = unit ? 1.0 : rho1;
    W.pw[0] = chi2;
    W.pw[1] = rho1;
    W.pw[2] = w;
    ORBFE_UNROLL
    for (int r = 0; r < 15; r++) W.Orw[r] = w * -He[r];
    double invJr[9];
    inverse_right_jacobian_so3(er, invJr);
    ORBFE_UNROLL
    for (int i = 0; i < 9; i++) {
        W.Jp[0][i] = invJr[i];
        W.Jp[1][i] = Rr[i];
    }
}

// block pair (p, q), p <= q < 5, of Jp^T (w H) Jp; the identity blocks (p, q >= 2) are not multiplied
template <class Prior, class Work>
ORBFE_HD inline void prev_prior_pair(const Prior& Pr, Work& W, int p, int q)
{
    const double w = W.pw[2];
    double Om[9], T[9], M[9];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++) Om[3 * i + j] = w * Pr.H[15 * (3 * p + i) + (3 * q + j)];
    if (q < 2) {
        double Jq[9];
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) Jq[e] = W.Jp[q][e];
        mul3d(Om, Jq, T);
    } else {
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) T[e] = Om[e];
    }
    if (p < 2) {
        double Jp[9], Jt[9];
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) Jp[e] = W.Jp[p][e];
        transpose3d(Jp, Jt);
        mul3d(Jt, T, M);
    } else {
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) M[e] = T[e];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++)
        ORBFE_UNROLL
        for (int j = 0; j < 3; j++)
            if (q > p || j >= i) {
                W.Hp[3 * p + i][3 * q + j] = M[3 * i + j];
                W.Hp[3 * q + j][3 * p + i] = M[3 * i + j];
            }
}

template <class Work>
ORBFE_HD inline void prev_prior_b(Work& W, int p)
{
    const double o[3] = {W.Orw[3 * p], W.Orw[3 * p + 1], W.Orw[3 * p + 2]};
    double t[3] = {o[0], o[1], o[2]};
    if (p < 2) {
        double Jp[9], Jt[9];
        ORBFE_UNROLL
        for (int e = 0; e < 9; e++) Jp[e] = W.Jp[p][e];
        transpose3d(Jp, Jt);
        matvec3(Jt, o, t);
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) W.bp[3 * p + i] = t[i];
}

template <class Link, class Work>
ORBFE_HD inline void prev_rw_lin(const Link& K, const PrevState& S, Work& W)
{
    double eg[3], ea[3];
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        eg[i] = S.cur.bg[i] - S.prv.bg[i];
        ea[i] = S.cur.ba[i] - S.prv.ba[i];
    }
    ORBFE_UNROLL
    for (int i = 0; i < 3; i++) {
        W.rwG[i] = (K.infoG[3 * i] * eg[0] + K.infoG[3 * i + 1] * eg[1]) + K.infoG[3 * i + 2] * eg[2];
        W.rwA[i] = (K.infoA[3 * i] * ea[0] + K.infoA[3 * i + 1] * ea[1]) + K.infoA[3 * i + 2] * ea[2];
    }
}

// the linearisation of the three non-mono edges at S into W: two phases
template <class Exec, class Link, class Prior>
ORBFE_HD inline void prev_linearize(Exec& X, const Link& K, const Prior& Pr, const PrevPar& G, bool unit, const PrevState& S, PrevWork& W)
{
    X.each(3, [&](int t) {
        if (t == 0) prev_inertial_lin(K, G.gravity, S, W);
        else if (t == 1) prev_prior_lin(Pr, G.priorDelta, unit, S, W);
        else prev_rw_lin(K, S, W);
    });
    X.each(64, [&](int t) {
        int p, q;
        if (t < 36) {
            prev_pair(8, t, p, q);
            prev_inertial_pair(K, W, p, q);
        } else if (t < 44) {
            prev_inertial_b(W, t - 36);
        } else if (t < 59) {
            prev_pair(5, t - 44, p, q);
            prev_prior_pair(Pr, W, p, q);
        } else {
            prev_prior_b(W, t - 59);
        }
    });
}

// a random-walk edge's share of entry (i, j) in solver order, i <= j: the frame's bias at `cur`, the previous frame's at `prv`;
// info's upper triangle, mirrored; the off-diagonal block pair carries -info
ORBFE_HD inline bool prev_rw_entry(const double* info, int cur, int prv, int i, int j, double& v)
{
    const bool ic = i >= cur && i < cur + 3, ip = i >= prv && i < prv + 3;
    const bool jc = j >= cur && j < cur + 3, jp = j >= prv && j < prv + 3;
    if (!(ic || ip) || !(jc || jp)) return false;
    const int a = ic ? i - cur : i - prv, b = jc ? j - cur : j - prv;
    const double s = info[3 * (a < b ? a : b) + (a < b ? b : a)];
    v = (ic == jc) ? s : -s;
    return true;
}

// entry (i, j) of the 30 x 30 system in solver order, in the reference's edge insertion order: the mono tree sum, the inertial edge,
// the gyro and the accelerometer random walk, the prior; +0.0 where no edge touches
template <class Link, class Work>
ORBFE_HD inline double prev_entry(const Link& K, const Work& W, int i0, int j0)
{
    const int i = i0 < j0 ? i0 : j0, j = i0 < j0 ? j0 : i0;
    bool has = false;
    double v = 0.0, t;
    if (j < 6) {
        v = W.acc[tri6(i, j)];
        has = true;
    }
    const int ri = prev_ref24(i), rj = prev_ref24(j);
    if (ri >= 0 && rj >= 0) {
        t = W.H24[ri][rj];
        v = has ? v + t : t;
        has = true;
    }
    if (prev_rw_entry(K.infoG, 9, 24, i, j, t)) {
        v = has ? v + t : t;
        has = true;
    }
    if (prev_rw_entry(K.infoA, 12, 27, i, j, t)) {
        v = has ? v + t : t;
        has = true;
    }
    if (i >= 15) {
        t = W.Hp[i - 15][j - 15];
        v = has ? v + t : t;
        has = true;
    }
    return has ? v : 0.0;
}

template <class Work>
ORBFE_HD inline double prev_rhs(const Work& W, int i)
{
    bool has = false;
    double v = 0.0, t;
    if (i < 6) {
        v = W.acc[21 + i];
        has = true;
    }
    const int ri = prev_ref24(i);
    if (ri >= 0) {
        t = W.b24[ri];
        v = has ? v + t : t;
        has = true;
    }
    if (i >= 9 && i < 12) { t = -W.rwG[i - 9]; v = has ? v + t : t; has = true; }
    if (i >= 24 && i < 27) { t = W.rwG[i - 24]; v = has ? v + t : t; has = true; }
    if (i >= 12 && i < 15) { t = -W.rwA[i - 12]; v = has ? v + t : t; has = true; }
    if (i >= 27) { t = W.rwA[i - 27]; v = has ? v + t : t; has = true; }
    if (i >= 15) { t = W.bp[i - 15]; v = has ? v + t : t; has = true; }
    return v;
}

// entry (r, c) of the Hessian handed out, reference order (:4216-4264): ((0 + inertial) + random walk) + prior) + T; the random-walk
// blocks are the informations as handed in, T the mono tree sum (upper triangle, mirrored)
template <class Link, class Work>
ORBFE_HD inline double prev_hessian_entry(const Link& K, const Work& W, int r, int c)
{
    double v = 0.0;
    if (r < 24 && c < 24) v = v + W.H24[r][c];
    const bool rg1 = r >= 9 && r < 12, rg2 = r >= 24 && r < 27, cg1 = c >= 9 && c < 12, cg2 = c >= 24 && c < 27;
    if ((rg1 || rg2) && (cg1 || cg2)) {
        const double s = K.infoG[3 * (rg1 ? r - 9 : r - 24) + (cg1 ? c - 9 : c - 24)];
        v = v + ((rg1 == cg1) ? s : -s);
    }
    const bool ra1 = r >= 12 && r < 15, ra2 = r >= 27, ca1 = c >= 12 && c < 15, ca2 = c >= 27;
    if ((ra1 || ra2) && (ca1 || ca2)) {
        const double s = K.infoA[3 * (ra1 ? r - 12 : r - 27) + (ca1 ? c - 12 : c - 27)];
        v = v + ((ra1 == ca1) ? s : -s);
    }
    if (r < 15 && c < 15) v = v + W.Hp[r][c];
    if (r >= 15 && r < 21 && c >= 15 && c < 21) {
        const int a = r - 15, b = c - 15;
        v = v + W.acc[tri6(a < b ? a : b, a < b ? b : a)];
    }
    return v;
}

template <class Link>
ORBFE_HD inline void prev_update(const Link& K, const PrevWork& W, PrevState& S)
{
    double d1[kImuN], d2[kImuN];
    ORBFE_UNROLL
    for (int i = 0; i < kImuN; i++) {
        d1[i] = W.dx[i];
        d2[i] = W.dx[kImuN + i];
    }
    imu_update(K, d1, S.cur);
    imu_update(K, d2, S.prv);
}

ORBFE_HD inline void prev_state_vector(const PrevState& S, double* o)
{
    ORBFE_UNROLL
    for (int h = 0; h < 2; h++) {
        const ImuState& s = h ? S.prv : S.cur;
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) o[21 * h + i] = s.Rwb[i];
        ORBFE_UNROLL
        for (int i = 0; i < 3; i++) {
            o[21 * h + 9 + i] = s.twb[i];
            o[21 * h + 12 + i] = s.v[i];
            o[21 * h + 15 + i] = s.bg[i];
            o[21 * h + 18 + i] = s.ba[i];
        }
    }
}

// The call.  X supplies, besides each / sync: leader() (one thread of the call), Ne(), mono_sums(huber, S.cur, W) -> W.acc over the
// edges whose flag is clear, solve(W) (A, b -> dx by ldlt_solve_n<30>; every pivot > 0), score(rnd, thr, thrClose, S.cur) -> nBad
// and recover(thr, S.cur) -> nBad, which keep the flags.
template <class Exec, class Link, class Prior>
ORBFE_HD inline void prev_solve(Exec& X, const Link& K, const Prior& Pr, const PrevPar& G, PrevState& S, PrevWork& W, const PrevOut& O)
{
    const int Ne = X.Ne();
    int nBad = 0, roundsRun = 0;
    for (int rnd = 0; rnd < G.nRounds; rnd++) {
        const bool huber = rnd <= 2;   // setRobustKernel(0) at it == 2, mono edges only (:4130)
        int nIt = 0;
        bool ok = true;
        for (int it = 0; it < G.iterations; it++) {
            nIt++;
            X.mono_sums(huber, S.cur, W);
            prev_linearize(X, K, Pr, G, false, S, W);
            X.each(kPrevH + kPrevN, [&](int t) {
                if (t < kPrevH) W.A[t / kPrevN][t % kPrevN] = prev_entry(K, W, t / kPrevN, t % kPrevN);
                else W.b[t - kPrevH] = prev_rhs(W, t - kPrevH);
            });
            ok = X.solve(W);
            if (!ok) break;   // the same bits in every thread: all leave or none
            X.each(1, [&](int) { prev_update(K, W, S); });   // one copy of the state: S may be shared by the threads
        }
        nBad = X.score(rnd, G.chi2[rnd], G.chi2Close[rnd], S.cur);
        roundsRun = rnd + 1;
        X.each(1, [&](int) { prev_prior_lin(Pr, G.priorDelta, false, S, W); });
        if (O.rounds && X.leader()) {
            PrevRoundsOut& I = *O.rounds;
            I.iterations[rnd] = nIt;
            I.ok[rnd] = ok ? 1 : 0;
            I.nBad[rnd] = nBad;
            prev_state_vector(S, I.state[rnd]);
            I.priorChi2[rnd] = W.pw[0];
            I.priorWeight[rnd] = W.pw[1];
        }
        if (Ne + 4 < 10) break;   // optimizer.edges().size() < 10 (:4168)
    }
    int recovered = 0;
    if (Ne - nBad < G.recoverBelow && !G.recInit) {   // (:4175-4203)
        recovered = 1;
        nBad = X.recover(G.recoverChi2, S.cur);
    }
    // the Hessian at the final state (:4216-4264) and its marginalisation (:4266)
    X.mono_sums(false, S.cur, W);
    prev_linearize(X, K, Pr, G, true, S, W);
    X.each(kPrevH, [&](int t) {
        const double v = prev_hessian_entry(K, W, t / kPrevN, t % kPrevN);
        W.H30[t] = v;
        O.H30[t] = v;
    });
    if (O.Hprior) marginalize_run(X, W.mg, W.H30, O.Hprior);
    if (X.leader()) {
        ORBFE_UNROLL
        for (int i = 0; i < 9; i++) O.state[i] = (float)S.cur.Rwb[i];
        ORBFE_UNROLL
        for (int i = 0; i < 3; i++) {
            O.state[9 + i] = (float)S.cur.twb[i];
            O.state[12 + i] = (float)S.cur.v[i];
            O.state[15 + i] = (float)S.cur.bg[i];
            O.state[18 + i] = (float)S.cur.ba[i];
        }
        const int valid = Ne - nBad;
        *O.nInliers = valid;
        *O.accepted = valid >= G.inlierThreshold ? 1 : 0;
        if (O.rounds) {
            O.rounds->Ne = Ne;
            O.rounds->roundsRun = roundsRun;
            O.rounds->recovered = recovered;
        }
    }
}

}  // namespace orbfe

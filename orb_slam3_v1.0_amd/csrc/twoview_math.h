// twoview_math.h -- what TwoViewReconstruction (SPEC DECISION S12) computes outside the teams of threads: the two terms of one match
// in CheckHomography / CheckFundamental, the ordered-integer image of a float that CheckRT's selection uses, and the plain C++
// host step between the two submissions (Normalize, the 3 x 3 SVD, the motion hypotheses of ReconstructH / DecomposeE).
// Contraction is off in every including unit.  No HIP here: kernels_twoview.hip and tests/cpp/two_view.cpp (as host C++) read this
// one text.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "host_device.h"
#include "jacobi.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

// CheckHomography's two terms of one match (:347-382); a rejected term is 0 and clears bIn
ORBFE_HD inline void homography_terms(const float (&H21)[9], const float (&H12)[9], float invSigmaSquare, float u1, float v1,
                                      float u2, float v2, float& term1, float& term2, bool& bIn)
{
    const float th = 5.991f;
    bIn = true;
    const float w2in1inv = (float)(1.0 / (double)((H12[6] * u2 + H12[7] * v2) + H12[8]));
    const float u2in1 = ((H12[0] * u2 + H12[1] * v2) + H12[2]) * w2in1inv;
    const float v2in1 = ((H12[3] * u2 + H12[4] * v2) + H12[5]) * w2in1inv;
    const float du1 = u1 - u2in1, dv1 = v1 - v2in1;
    const float squareDist1 = du1 * du1 + dv1 * dv1;
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; term1 = 0.0f; }
    else term1 = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)((H21[6] * u1 + H21[7] * v1) + H21[8]));
    const float u1in2 = ((H21[0] * u1 + H21[1] * v1) + H21[2]) * w1in2inv;
    const float v1in2 = ((H21[3] * u1 + H21[4] * v1) + H21[5]) * w1in2inv;
    const float du2 = u2 - u1in2, dv2 = v2 - v1in2;
    const float squareDist2 = du2 * du2 + dv2 * dv2;
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; term2 = 0.0f; }
    else term2 = th - chiSquare2;
}

// CheckFundamental's two terms of one match (:423-462)
ORBFE_HD inline void fundamental_terms(const float (&F)[9], float invSigmaSquare, float u1, float v1, float u2, float v2,
                                       float& term1, float& term2, bool& bIn)
{
    const float th = 3.841f, thScore = 5.991f;
    bIn = true;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const float c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; term1 = 0.0f; }
    else term1 = thScore - chiSquare1;
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; term2 = 0.0f; }
    else term2 = thScore - chiSquare2;
}

// order-preserving image of a float in the unsigned integers
ORBFE_HD inline unsigned ordered_key(float f)
{
    unsigned u;
    memcpy(&u, &f, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ORBFE_HD inline float ordered_key_inverse(unsigned k)
{
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// ---- the host step ----

// Normalize (:750-797): sequential binary32 sums over ALL keypoints of the frame in index order (Keypoint: orbfe_keypoint)
template <class Keypoint>
void normalize_points(int n, const Keypoint* kp, std::vector<float>& px, std::vector<float>& py, float (&T)[9])
{
    float meanX = 0.0f, meanY = 0.0f;
    for (int i = 0; i < n; i++) {
        meanX = meanX + kp[i].x;
        meanY = meanY + kp[i].y;
    }
    meanX = meanX / (float)n;
    meanY = meanY / (float)n;
    float meanDevX = 0.0f, meanDevY = 0.0f;
    px.resize((size_t)n);
    py.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        px[(size_t)i] = kp[i].x - meanX;
        py[(size_t)i] = kp[i].y - meanY;
        meanDevX = meanDevX + fabsf(px[(size_t)i]);
        meanDevY = meanDevY + fabsf(py[(size_t)i]);
    }
    meanDevX = meanDevX / (float)n;
    meanDevY = meanDevY / (float)n;
    const float sX = (float)(1.0 / (double)meanDevX);
    const float sY = (float)(1.0 / (double)meanDevY);
    for (int i = 0; i < n; i++) {
        px[(size_t)i] = px[(size_t)i] * sX;
        py[(size_t)i] = py[(size_t)i] * sY;
    }
    for (int i = 0; i < 9; i++) T[i] = 0.0f;
    T[0] = sX;
    T[4] = sY;
    T[2] = -meanX * sX;
    T[5] = -meanY * sY;
    T[8] = 1.0f;
}

// JacobiSVD of a 3 x 3 float matrix (:597, :919), S12: V and w^2 from the n = 3 sequence on A^T A (binary64), sorted by
// descending eigenvalue (lower index first among equals); u_i = A v_i / |A v_i| for i = 0, 1, u_2 = u_0 x u_1; every entry
// rounded to float.  w_i = sqrt(max(eigenvalue_i, 0)).  fullRank (:597): u_2 is negated when it points against A v_2, so that
// A = U diag(w) V^T holds with w >= 0 and s = det(U) det(V^T) of :603 carries the sign of det(A), as with any true SVD.
inline void svd3(const float (&A)[9], float (&U)[9], float (&w)[3], float (&V)[9], bool fullRank)
{
    double M[3][3], E[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
            for (int k = 0; k < 3; k++) acc = acc + (double)A[3 * k + i] * (double)A[3 * k + j];
            M[i][j] = acc;
        }
    jacobi3(M, E);
    int order[3] = {0, 1, 2};
    for (int a = 0; a < 2; a++)  // stable selection sort, descending
        for (int b = a + 1; b < 3; b++)
            if (M[order[b]][order[b]] > M[order[a]][order[a]]) {
                const int t = order[b];
                for (int k = b; k > a; k--) order[k] = order[k - 1];
                order[a] = t;
            }
    double v[3][3], u[3][3];  // [i] = i-th singular vector
    for (int i = 0; i < 3; i++) {
        const int c = order[i];
        const double lam = M[c][c];
        w[i] = (float)sqrt(lam > 0.0 ? lam : 0.0);
        for (int k = 0; k < 3; k++) v[i][k] = E[k][c];
    }
    for (int i = 0; i < 2; i++) {
        double av[3];
        for (int r = 0; r < 3; r++) av[r] = ((double)A[3 * r] * v[i][0] + (double)A[3 * r + 1] * v[i][1]) + (double)A[3 * r + 2] * v[i][2];
        const double nrm = sqrt((av[0] * av[0] + av[1] * av[1]) + av[2] * av[2]);
        for (int r = 0; r < 3; r++) u[i][r] = av[r] / nrm;
    }
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    if (fullRank) {
        double av[3];
        for (int r = 0; r < 3; r++) av[r] = ((double)A[3 * r] * v[2][0] + (double)A[3 * r + 1] * v[2][1]) + (double)A[3 * r + 2] * v[2][2];
        if ((av[0] * u[2][0] + av[1] * u[2][1]) + av[2] * u[2][2] < 0.0)
            for (int r = 0; r < 3; r++) u[2][r] = -u[2][r];
    }
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) {
            U[3 * r + i] = (float)u[i][r];
            V[3 * r + i] = (float)v[i][r];
        }
}

inline void normalize3(float (&t)[3])
{
    const float nrm = sqrtf((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    t[0] = t[0] / nrm;
    t[1] = t[1] / nrm;
    t[2] = t[2] / nrm;
}

inline void scale3(float s, const float (&A)[9], float (&O)[9])
{
    for (int i = 0; i < 9; i++) O[i] = s * A[i];
}

// DecomposeE (:916-940) and the hypothesis order of ReconstructF (:498-501): (R1, t) (R2, t) (R1, -t) (R2, -t)
inline int motion_hypotheses_f(const float (&F21)[9], const float (&K)[9], float (*R)[9], float (*t)[3])
{
    float Kt[9], tmp[9], E[9], U[9], w[3], V[9], Vt[9];
    transpose3(K, Kt);
    mul3(Kt, F21, tmp);
    mul3(tmp, K, E);  // :482
    svd3(E, U, w, V, false);
    transpose3(V, Vt);
    float tt[3] = {U[2], U[5], U[8]};
    normalize3(tt);
    const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float Wt[9], R1[9], R2[9];
    transpose3(W, Wt);
    mul3(U, W, tmp);
    mul3(tmp, Vt, R1);
    if (det3(R1) < 0.0f)
        for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    mul3(U, Wt, tmp);
    mul3(tmp, Vt, R2);
    if (det3(R2) < 0.0f)
        for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    for (int h = 0; h < 4; h++) {
        const float (&Rs)[9] = (h & 1) ? R2 : R1;
        for (int i = 0; i < 9; i++) R[h][i] = Rs[i];
        for (int i = 0; i < 3; i++) t[h][i] = h < 2 ? tt[i] : -tt[i];
    }
    return 4;
}

// ReconstructH up to the eight hypotheses (:594-702); 0 when the singular values are too close (:609)
inline int motion_hypotheses_h(const float (&H21)[9], const float (&K)[9], float (*R)[9], float (*t)[3])
{
    float invK[9], tmp[9], A[9], U[9], w[3], V[9], Vt[9];
    inv3(K, invK);
    mul3(invK, H21, tmp);
    mul3(tmp, K, A);  // :595
    svd3(A, U, w, V, true);
    transpose3(V, Vt);
    const float s = det3(U) * det3(Vt);  // :603
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;  // :609
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));  // :621-624
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);  // :627-630
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    float sU[9];
    scale3(s, U, sU);
    for (int i = 0; i < 4; i++) {  // :632-663
        const float Rp[9] = {ctheta, 0.0f, -stheta[i], 0.0f, 1.0f, 0.0f, stheta[i], 0.0f, ctheta};
        mul3(sU, Rp, tmp);
        mul3(tmp, Vt, R[i]);
        const float k = d1 - d3;
        const float tp[3] = {x1[i] * k, 0.0f * k, -x3[i] * k};
        for (int r = 0; r < 3; r++) t[i][r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
        normalize3(t[i]);
    }
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);  // :666-669
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    for (int i = 0; i < 4; i++) {  // :671-702
        const float Rp[9] = {cphi, 0.0f, sphi[i], 0.0f, -1.0f, 0.0f, sphi[i], 0.0f, -cphi};
        mul3(sU, Rp, tmp);
        mul3(tmp, Vt, R[4 + i]);
        const float k = d1 + d3;
        const float tp[3] = {x1[i] * k, 0.0f * k, x3[i] * k};
        for (int r = 0; r < 3; r++) t[4 + i][r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
        normalize3(t[4 + i]);
    }
    return 8;
}

// cos(1 degree) in binary64: "parallax > 1.0" is "(double)cos < kCosOneDegree" (S12: the one stated departure)
constexpr double kCosOneDegree = 0x1.ffec097f5af8ap-1;

}  // namespace orbfe

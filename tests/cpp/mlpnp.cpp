// A fresh MLPnPsolver + SetRansacParameters + one iterate() (src/MLPnPsolver.cpp) from a plain C++ program, two ways on the same inputs:
//   (a) the library through include/orbfe_adaptor.hpp's MLPnPsolver class (orbfe_mlpnp_ransac),
//   (b) SPEC DECISION S13 as a single-thread host loop (this file, -O2 -ffp-contract=off, one pinned core): every hypothesis in turn,
//       Refine for every candidate, the first success returns.
// (b) is the kernels' arithmetic written out for one CPU thread (the helpers below follow csrc/kernels_mlpnp.hip, device_math.h and
// jacobi.h line by line, so it is the latency yardstick, not an independent oracle -- that is tests/mlpnp_ref.py): its results
// must equal the library's bit for bit (host_same=1), and tests/test_mlpnp_cpp.py compares them with the numpy restatement
// without a GPU.
//   usage: mlpnp                                   -> library version (link test)
//          mlpnp <scene.bin> <out.bin> host        -> (b) only, its results to out.bin: no GPU needed
//          mlpnp <scene.bin> <out.bin> [reps]      -> (a) and (b); results of (a) to out.bin; medians of `reps` calls
// scene.bin: int32 n, n_points, total, min_set, model, n_levels, min_inliers_param, max_iterations, n_iterations; float64 probability;
//            float32 cam[8], precision, epsilon, th2, level_sigma2[n_levels]; keypoints (24 B each); int32 mp_index[n];
//            float32 points[n_points][3]; int32 sets[total][min_set]
// out.bin:   int32 solved, n_inliers, no_more, N, min_inliers, max_its, total, exit_kind, returning_iteration, n_candidates;
//            float32 Tcw[16]; uint8 inliers[n]; float64 hyp_Rt[total][12]; int32 hyp_inliers[total], hyp_planar[total],
//            hyp_gn_evals[total], hyp_gn_exit[total], candidates[nc]; float64 cand_Rt[nc][12]; int32 cand_inliers[nc], cand_planar[nc];
//            uint8 cand_mask[nc][N]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include <sched.h>

#include "orbfe_adaptor.hpp"

using namespace ORB_SLAM3;

namespace s13 {

constexpr int kSweeps3 = 10, kSweeps9 = 10, kSweeps12 = 12;
constexpr double kEps = 0x1p-52;
constexpr double kRankTol = 0x1.8p-51;

static float spec_atan2f(float y, float x)
{
    const float kPi = 0x1.921fb6p+1f, kPi2 = 0x1.921fb6p+0f, kPi4 = 0x1.921fb6p-1f;
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = ax > ay ? ax : ay;
    const float mn = ax > ay ? ay : ax;
    if (mx == 0.0f) return 0.0f;
    float t = mn / mx;  // correctly rounded (hipcc default: -fhip-fp32-correctly-rounded-divide-sqrt)
    float base = 0.0f;
    if (t > 0x1.a8279ap-2f) {
        t = (t - 1.0f) / (t + 1.0f);
        base = kPi4;
    }
    const float z = t * t;
    float p = 0x1.61e174p-4f * z;
    p = p + -0x1.1fe904p-3f;
    p = p * z;
    p = p + 0x1.99799ep-3f;
    p = p * z;
    p = p + -0x1.555556p-2f;
    float r = p * z;
    r = r * t;
    r = r + t;
    r = base + r;
    if (ay > ax) r = kPi2 - r;
    if (x < 0.0f) r = kPi - r;
    if (y < 0.0f) r = -r;
    return r;
}


// cos/sin of an angle given in degrees (src/cuda/Orb_gpu.cu:327-329)
static void cos_sin_deg(float deg, float& c, float& s)
{
    float kf = deg * 0x1.6c16c2p-7f;
    kf = kf + 0.5f;
    const int k = (int)kf;
    const float r = deg - 90.0f * (float)k;
    const float x = r * 0x1.1df46ap-6f;
    const float z = x * x;
    float p = -0x1.9b7856p-13f * z;
    p = p + 0x1.110e32p-7f;
    p = p * z;
    p = p + -0x1.555558p-3f;
    float sn = p * z;
    sn = sn * x;
    sn = sn + x;
    float q = 0x1.9bfe2ep-16f * z;
    q = q + -0x1.6c134p-10f;
    q = q * z;
    q = q + 0x1.555554p-5f;
    float cs = q * z;
    cs = cs * z;
    float h = 0.5f * z;
    h = 1.0f - h;
    cs = cs + h;
    switch (k & 3) {
    case 0: c = cs; s = sn; break;
    case 1: c = -sn; s = cs; break;
    case 2: c = -cs; s = -sn; break;
    default: c = sn; s = -cs; break;
    }
}


template <class Frustum>
static void camera_project(const Frustum& F, float x, float y, float z, float& u, float& v)
{
    if (F.camera_model == 0) {
        u = F.fx * x / z + F.cx;
        v = F.fy * y / z + F.cy;
        return;
    }
    const float x2_plus_y2 = x * x + y * y;
    const float theta = spec_atan2f(sqrtf(x2_plus_y2), z);
    const float psi = spec_atan2f(y, x);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = (((theta + F.k1 * theta3) + F.k2 * theta5) + F.k3 * theta7) + F.k4 * theta9;
    float deg = psi * 0x1.ca5dc2p+5f;  // 180 / pi
    if (deg < 0.0f) deg = deg + 360.0f;
    float c, s;
    cos_sin_deg(deg, c, s);
    u = F.fx * r * c + F.cx;
    v = F.fy * r * s + F.cy;
}


struct CamP {
    float fx, fy, cx, cy, k1, k2, k3, k4;
    int camera_model;
};

static CamP cam_of(const float (&c)[8], int model)
{
    return CamP{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], model};
}

static void cam_unproject(const CamP& C, float precision, float u, float v, float& rx, float& ry)
{
    const float pwx = (u - C.cx) / C.fx;
    const float pwy = (v - C.cy) / C.fy;
    rx = pwx;
    ry = pwy;
    if (C.camera_model == 0) return;  // Pinhole::unproject (src/CameraModels/Pinhole.cpp:57-60)
    // KannalaBrandt8::unproject (:115-142): Newton on theta (1 + k1 theta^2 + ...) = theta_d
    float scale = 1.0f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    const float kHalfPi = 0x1.921fb6p+0f;
    theta_d = fminf(fmaxf(-kHalfPi, theta_d), kHalfPi);
    if (theta_d > 1e-8f) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
            const float k0t2 = C.k1 * theta2, k1t4 = C.k2 * theta4, k2t6 = C.k3 * theta6, k3t8 = C.k4 * theta8;
            const float num = theta * ((((1.0f + k0t2) + k1t4) + k2t6) + k3t8) - theta_d;
            const float den = (((1.0f + 3.0f * k0t2) + 5.0f * k1t4) + 7.0f * k2t6) + 9.0f * k3t8;
            const float fix = num / den;
            theta = theta - fix;
            if (fabsf(fix) < precision) break;
        }
        float c, sn;
        cos_sin_deg(theta * 0x1.ca5dc2p+5f, c, sn);  // theta in [0, pi/2] as degrees
        scale = (sn / c) / theta_d;
    }
    rx = pwx * scale;
    ry = pwy * scale;
}


// ---- SPEC DECISION S13: binary64 sin / cos / acos / cbrt as sequences of + - x / sqrt and the exact floor / frexp / ldexp ----
// (ocml and glibc differ in the last place).  The same constants and operation order as tests/mlpnp_ref.py sincos64 / acos64 /
// cbrt64 (tests/test_mlpnp_cpp.py compares every result of this file with the restatement's).
constexpr double kTwoOverPi = 0x1.45f306dc9c883p-1;
constexpr double kPio2_1 = 0x1.921fb54400000p+0, kPio2_2 = 0x1.0b4611a600000p-34, kPio2_3 = 0x1.3198a2e037073p-69;  // pi / 2 in three parts (33 + 33 + 53 bits)
constexpr double kPio2Hi = 0x1.921fb54442d18p+0, kPio2Lo = 0x1.1a62633145c07p-54, kPiHi = 0x1.921fb54442d18p+1, kPiLo = 0x1.1a62633145c07p-53;
constexpr double kSinC[9] = {-0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19, -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57};  // (-1)^k / (2k + 1)!, k = 1 .. 9
constexpr double kCosC[10] = {-0x1.0000000000000p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37, 0x1.ae7f3e733b81fp-45, -0x1.6827863b97d97p-53, 0x1.e542ba4020225p-62};  // (-1)^k / (2k)!, k = 1 .. 10
constexpr double kAsinC[28] = {0x1.5555555555555p-3, 0x1.3333333333333p-4, 0x1.6db6db6db6db7p-5, 0x1.f1c71c71c71c7p-6, 0x1.6e8ba2e8ba2e9p-6, 0x1.1c4ec4ec4ec4fp-6, 0x1.c99999999999ap-7, 0x1.7a87878787878p-7, 0x1.3fde50d79435ep-7, 0x1.12ef3cf3cf3cfp-7, 0x1.df3bd37a6f4dfp-8, 0x1.a6863d70a3d71p-8, 0x1.782dda12f684cp-8, 0x1.51ba308d3dcb1p-8, 0x1.31683bdef7bdfp-8, 0x1.15ee9d45d1746p-8, 0x1.fcaf8fb6db6dbp-9, 0x1.d3d2a8e0dd67dp-9, 0x1.b026f57b13b14p-9, 0x1.90cb77f60c7cep-9, 0x1.750de64d7d05fp-9, 0x1.5c5f56efaaaabp-9, 0x1.464c0950f7d47p-9, 0x1.3275586c5f2f0p-9, 0x1.208d3570ae5a6p-9, 0x1.1052bc5fa960ap-9, 0x1.018f963c229bfp-9, 0x1.e82be60d9127ep-10};  // (2k)! / (4^k k!^2 (2k + 1)), k = 1 .. 28
constexpr double kCbrtA = 0.75, kCbrtB = 0.22;
constexpr int kCbrtNewton = 6;

template <int N>
static double horner64(double z, const double (&c)[N])
{
    double p = c[N - 1];
    for (int k = N - 2; k >= 0; k--) p = p * z + c[k];
    return p;
}

// sin x and cos x for 0 <= x < 2^20 (NaN elsewhere): k = floor(x * 2/pi + 0.5), r = ((x - k P1) - k P2) - k P3, Taylor polynomials
// of r by Horner in z = r * r, picked and signed by the quadrant k mod 4
static void spec_sincos64(double x, double& s, double& c)
{
    if (!(x >= 0.0 && x < 1048576.0)) { s = NAN; c = NAN; return; }
    const double k = floor(x * kTwoOverPi + 0.5);
    const double r = ((x - k * kPio2_1) - k * kPio2_2) - k * kPio2_3;
    const double z = r * r;
    const double sn = r + (r * z) * horner64(z, kSinC);
    const double cs = 1.0 + z * horner64(z, kCosC);
    const double q = k - 4.0 * floor(k * 0.25);
    if (q == 0.0) { s = sn; c = cs; }
    else if (q == 1.0) { s = cs; c = -sn; }
    else if (q == 2.0) { s = -sn; c = -cs; }
    else { s = -cs; c = sn; }
}

// acos on [-1, 1] (NaN outside): |x| <= 0.5: pi/2 - asin x; else 2 asin(sqrt((1 - |x|) / 2)), reflected about pi for x < 0;
// asin t = t + (t z) P(z), z = t * t
static double spec_acos64(double x)
{
    const double ax = fabs(x);
    if (ax <= 0.5) {
        const double z = x * x;
        const double a = x + (x * z) * horner64(z, kAsinC);
        return (kPio2Hi - a) + kPio2Lo;
    }
    const double z = (1.0 - ax) * 0.5;
    const double sq = sqrt(z);
    const double a = sq + (sq * z) * horner64(z, kAsinC);
    const double r = 2.0 * a;
    return x < 0.0 ? (kPiHi - r) + kPiLo : r;
}

// cube root of x > 0 (0, inf and NaN are returned as they are): x = m 2^e, e + 3000 = 3 q + r, a = m 2^r in [0.5, 4),
// y = 0.75 + 0.22 a, six Newton steps, result y 2^(q - 1000)
static double spec_cbrt64(double x)
{
    if (!(x > 0.0 && x < INFINITY)) return x;
    int e;
    const double m = frexp(x, &e);
    const int e3 = e + 3000;
    const int q = e3 / 3;
    const int r = e3 - 3 * q;
    const double a = ldexp(m, r);
    double y = kCbrtA + kCbrtB * a;
    for (int i = 0; i < kCbrtNewton; i++) y = y - ((y * y) * y - a) / (3.0 * (y * y));
    return ldexp(y, q - 1000);
}

// the rotation angle of every Jacobi sequence here (S10): c, s from M[p][p], M[q][q], M[p][q] != 0
static void jacobi_angle(double app, double aqq, double apq, double& c, double& sn)
{
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    sn = t * c;
}

// S12, n = 3: kSweeps3 cyclic sweeps in the pair order (0,1) (0,2) (1,2); M becomes (nearly) diagonal, V its eigenvectors
template <int P, int Q>
static void jacobi3_rotate(double (&M)[3][3], double (&V)[3][3])
{
    const double apq = M[P][Q];
    if (apq == 0.0) return;
    double c, sn;
    jacobi_angle(M[P][P], M[Q][Q], apq, c, sn);
    for (int k = 0; k < 3; k++) {
        const double mkp = M[k][P], mkq = M[k][Q];
        M[k][P] = c * mkp - sn * mkq;
        M[k][Q] = sn * mkp + c * mkq;
    }
    for (int k = 0; k < 3; k++) {
        const double mpk = M[P][k], mqk = M[Q][k];
        M[P][k] = c * mpk - sn * mqk;
        M[Q][k] = sn * mpk + c * mqk;
    }
    for (int k = 0; k < 3; k++) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - sn * vkq;
        V[k][Q] = sn * vkp + c * vkq;
    }
}

static void jacobi3(double (&M)[3][3], double (&V)[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps3; sweep++) {
        jacobi3_rotate<0, 1>(M, V);
        jacobi3_rotate<0, 2>(M, V);
        jacobi3_rotate<1, 2>(M, V);
    }
}


// the pairs of round r.  n = 12 (11 rounds of 6): {r, 11} and {(r + k) mod 11, (r - k) mod 11}, k = 1 .. 5 (the circle method);
// n = 9 (9 rounds of 4, S12): the pairs {i, j}, i < j, i + j == r (mod 9), in ascending i
static void jacobi_round_pair(int n, int r, int slot, int& p, int& q)
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


// ---- 3 x 3 binary64 helpers, row-major ----
static double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static double norm3(const double* a) { return sqrt(dot3(a, a)); }
static void matvec3(const double* R, const double* x, double* o)
{
    for (int i = 0; i < 3; i++) o[i] = (R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2];
}
static void mul3d(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
static void transpose3d(const double* A, double* T)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}
static double det3d(const double* a)
{
    const double c00 = a[4] * a[8] - a[5] * a[7];
    const double c10 = a[5] * a[6] - a[3] * a[8];
    const double c20 = a[3] * a[7] - a[4] * a[6];
    return (a[0] * c00 + a[1] * c10) + a[2] * c20;
}
static void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// eigen-decomposition of the symmetric G (row-major, destroyed) by the n = 3 sequence; order[] = the columns stably sorted by
// ascending (descending) eigenvalue
static void eig3_sorted(const double* G, bool descending, double (&lam)[3], double (&E)[3][3], int (&order)[3])
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
static void polar3(const double* A, double* R)
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

static void skew3(const double* w, double* K)
{
    K[0] = 0.0; K[1] = -w[2]; K[2] = w[1];
    K[3] = w[2]; K[4] = 0.0; K[5] = -w[0];
    K[6] = -w[1]; K[7] = w[0]; K[8] = 0.0;
}

// rodrigues2rot (:659-674) and, when D is given, dR / dw_k from the closed form (the limit [e_k]x for |w| <= eps)
static void rodrigues2rot(const double* w, double* R, double (*D)[9])
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
static void rot2rodrigues(const double* R, double* om)
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
static void point_rows(const double* R, const double (*D)[9], const double* T, const double* X, const double* nr,
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

// A x = b for symmetric 6 x 6 A (destroyed) by L D L^T with diagonal pivoting (S13)
static void ldlt_solve6(double (&A)[6][6], const double (&b)[6], double (&x)[6])
{
    double L[6][6], d[6];
    int perm[6];
    for (int i = 0; i < 6; i++) {
        perm[i] = i;
        for (int j = 0; j < 6; j++) L[i][j] = 0.0;
    }
    for (int k = 0; k < 6; k++) {
        int best = k;
        for (int i = k + 1; i < 6; i++)
            if (fabs(A[i][i]) > fabs(A[best][best])) best = i;
        for (int j = 0; j < 6; j++) { const double t = A[k][j]; A[k][j] = A[best][j]; A[best][j] = t; }
        for (int i = 0; i < 6; i++) { const double t = A[i][k]; A[i][k] = A[i][best]; A[i][best] = t; }
        for (int j = 0; j < 6; j++) { const double t = L[k][j]; L[k][j] = L[best][j]; L[best][j] = t; }
        { const int t = perm[k]; perm[k] = perm[best]; perm[best] = t; }
        const double dk = A[k][k];
        d[k] = dk;
        double col[6];
        for (int i = 0; i < 6; i++) col[i] = A[i][k];
        for (int i = k + 1; i < 6; i++) {
            const double li = dk == 0.0 ? 0.0 : col[i] / dk;
            L[i][k] = li;
            for (int j = k + 1; j <= i; j++) {
                const double val = A[i][j] - li * col[j];
                A[i][j] = val;
                A[j][i] = val;
            }
        }
    }
    double z[6], w[6], xs[6];
    for (int i = 0; i < 6; i++) {
        double acc = b[perm[i]];
        for (int j = 0; j < i; j++) acc = acc - L[i][j] * z[j];
        z[i] = acc;
    }
    for (int i = 0; i < 6; i++) w[i] = d[i] == 0.0 ? 0.0 : z[i] / d[i];
    for (int i = 5; i >= 0; i--) {
        double acc = w[i];
        for (int j = i + 1; j < 6; j++) acc = acc - L[j][i] * xs[j];
        xs[i] = acc;
    }
    for (int i = 0; i < 6; i++) x[perm[i]] = xs[i];
}


struct Pose {
    double R[9], t[3];
    int planar, gnEvals, gnExit;
};

struct Corr {
    std::vector<double> X, f, nr, ns;   // [N][3]
    std::vector<float> p2d, x32, maxErr;
};

// the fixed Jacobi sequence on the symmetric n x n M (n = 12 or 9, stride 12): M becomes (nearly) diagonal, V its eigenvectors
static void jacobi_rounds(double (*M)[12], double (*V)[12], int n)
{
    const int np = n == 12 ? 6 : 4, nr = n == 12 ? 11 : 9, sweeps = n == 12 ? kSweeps12 : kSweeps9;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < sweeps; sweep++)
        for (int r = 0; r < nr; r++) {
            int P[6], Q[6], skip[6];
            double c[6], s[6];
            for (int e = 0; e < np; e++) {  // the angles, from M as it stands at the start of the round
                jacobi_round_pair(n, r, e, P[e], Q[e]);
                const double apq = M[P[e]][Q[e]];
                skip[e] = apq == 0.0;
                c[e] = 1.0; s[e] = 0.0;
                if (!skip[e]) jacobi_angle(M[P[e]][P[e]], M[Q[e]][Q[e]], apq, c[e], s[e]);
            }
            for (int e = 0; e < np; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < n; k++) {
                    const double a = M[k][P[e]], b = M[k][Q[e]];
                    M[k][P[e]] = c[e] * a - s[e] * b;
                    M[k][Q[e]] = s[e] * a + c[e] * b;
                }
            }
            for (int e = 0; e < np; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < n; k++) {
                    const double a = M[P[e]][k], b = M[Q[e]][k];
                    M[P[e]][k] = c[e] * a - s[e] * b;
                    M[Q[e]][k] = s[e] * a + c[e] * b;
                    const double va = V[k][P[e]], vb = V[k][Q[e]];
                    V[k][P[e]] = c[e] * va - s[e] * vb;
                    V[k][Q[e]] = s[e] * va + c[e] * vb;
                }
            }
        }
}

// computePose (:355-657) on the points idx[0 .. n-1]
static void compute_pose(const Corr& C, const int* idx, int n, Pose& out)
{
    double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
            for (int p = 0; p < n; p++) acc = acc + C.X[3 * (size_t)idx[p] + i] * C.X[3 * (size_t)idx[p] + j];
            G[3 * i + j] = acc;
        }
    double lam[3], E[3][3], eigenRot[9];
    int order[3];
    eig3_sorted(G, false, lam, E, order);
    double mx = fabs(lam[0]);
    for (int i = 1; i < 3; i++) mx = fabs(lam[i]) > mx ? fabs(lam[i]) : mx;
    int rank = 0;
    for (int i = 0; i < 3; i++) rank += fabs(lam[i]) > kRankTol * mx;
    const bool planar = rank == 2;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) eigenRot[3 * i + j] = E[j][order[i]];
    const int nc = planar ? 9 : 12;
    std::vector<double> A((size_t)2 * n * 12, 0.0);
    for (int p = 0; p < n; p++) {
        const double* X = &C.X[3 * (size_t)idx[p]];
        double P3[3];
        matvec3(eigenRot, X, P3);
        for (int h = 0; h < 2; h++) {
            const double* nv = h ? &C.ns[3 * (size_t)idx[p]] : &C.nr[3 * (size_t)idx[p]];
            double* row = &A[(size_t)(2 * p + h) * 12];
            for (int i = 0; i < 3; i++) {
                if (!planar) {
                    for (int j = 0; j < 3; j++) row[3 * i + j] = nv[i] * X[j];
                    row[9 + i] = nv[i];
                } else {
                    row[2 * i] = nv[i] * P3[1];
                    row[2 * i + 1] = nv[i] * P3[2];
                    row[6 + i] = nv[i];
                }
            }
        }
    }
    double M[12][12], V[12][12];
    for (int i = 0; i < nc; i++)
        for (int j = 0; j < nc; j++) {
            double acc = 0.0;
            for (int k = 0; k < 2 * n; k++) acc = acc + A[(size_t)k * 12 + i] * A[(size_t)k * 12 + j];
            M[i][j] = acc;
        }
    jacobi_rounds(M, V, nc);
    int bi = 0;
    for (int i = 1; i < nc; i++)
        if (M[i][i] < M[bi][bi]) bi = i;
    double res[12];
    for (int k = 0; k < 12; k++) res[k] = k < nc ? V[k][bi] : 0.0;
    double X6[6][3], f6[6][3];
    for (int p = 0; p < 6; p++)
        for (int k = 0; k < 3; k++) { X6[p][k] = C.X[3 * (size_t)idx[p] + k]; f6[p][k] = C.f[3 * (size_t)idx[p] + k]; }
    double R0[9], t0[3];
    if (!planar) {
        double tmp[9], cn[3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) tmp[3 * i + j] = res[3 * j + i];
        for (int j = 0; j < 3; j++) cn[j] = sqrt((tmp[j] * tmp[j] + tmp[3 + j] * tmp[3 + j]) + tmp[6 + j] * tmp[6 + j]);
        const double scale = 1.0 / spec_cbrt64(fabs((cn[0] * cn[1]) * cn[2]));
        double Rp[9], ts[3], tt[3], tinv[3], err[2];
        polar3(tmp, Rp);
        for (int i = 0; i < 3; i++) ts[i] = scale * res[9 + i];
        matvec3(Rp, ts, tt);
        transpose3d(Rp, R0);
        matvec3(R0, tt, tinv);
        for (int i = 0; i < 3; i++) tinv[i] = -tinv[i];
        for (int s = 0; s < 2; s++) {
            double e = 0.0;
            for (int p = 0; p < 6; p++) {
                double v[3];
                matvec3(R0, X6[p], v);
                for (int i = 0; i < 3; i++) v[i] = v[i] + (s ? -tinv[i] : tinv[i]);
                const double nv = norm3(v);
                for (int i = 0; i < 3; i++) v[i] = v[i] / nv;
                e = e + (1.0 - dot3(v, f6[p]));
            }
            err[s] = e;
        }
        for (int i = 0; i < 3; i++) t0[i] = err[0] < err[1] ? tinv[i] : -tinv[i];
    } else {
        const double c1[3] = {res[0], res[2], res[4]}, c2[3] = {res[1], res[3], res[5]};
        double tmp[9];
        cross3(c1, c2, tmp);
        for (int k = 0; k < 3; k++) { tmp[3 + k] = c1[k]; tmp[6 + k] = c2[k]; }
        const double n1 = sqrt((tmp[1] * tmp[1] + tmp[4] * tmp[4]) + tmp[7] * tmp[7]);
        const double n2 = sqrt((tmp[2] * tmp[2] + tmp[5] * tmp[5]) + tmp[8] * tmp[8]);
        const double scale = 1.0 / sqrt(fabs(n1 * n2));
        double Rp[9], eT[9], Rq[9], R1[9], R2[9], t[3];
        polar3(tmp, Rp);
        transpose3d(eigenRot, eT);
        mul3d(eT, Rp, Rq);
        for (int i = 0; i < 3; i++) t[i] = scale * res[6 + i];
        transpose3d(Rq, R1);
        for (int k = 0; k < 9; k++) R1[k] = -R1[k];
        if (det3d(R1) < 0.0)
            for (int i = 0; i < 3; i++) R1[3 * i + 2] = -R1[3 * i + 2];
        for (int i = 0; i < 3; i++) { R2[3 * i] = -R1[3 * i]; R2[3 * i + 1] = -R1[3 * i + 1]; R2[3 * i + 2] = R1[3 * i + 2]; }
        double best = 0.0;
        for (int c = 0; c < 4; c++) {
            const double* Rc = c < 2 ? R1 : R2;
            double val = 0.0;
            for (int p = 0; p < 6; p++) {
                double v[3];
                matvec3(Rc, X6[p], v);
                for (int i = 0; i < 3; i++) v[i] = v[i] + ((c & 1) ? -t[i] : t[i]);
                const double nv = norm3(v);
                for (int i = 0; i < 3; i++) v[i] = v[i] / nv;
                val = val + (1.0 - dot3(v, f6[p]));
            }
            if (c == 0 || val < best) {
                best = val;
                for (int k = 0; k < 9; k++) R0[k] = Rc[k];
                for (int i = 0; i < 3; i++) t0[i] = (c & 1) ? -t[i] : t[i];
            }
        }
    }
    double x[6];
    rot2rodrigues(R0, x);
    for (int i = 0; i < 3; i++) x[3 + i] = t0[i];
    out.gnEvals = 0;
    out.gnExit = 0;
    std::vector<double> J((size_t)2 * n * 6), r((size_t)2 * n);
    for (int it = 0; it < 5; it++) {
        double R[9], D[3][9];
        rodrigues2rot(x, R, D);
        for (int p = 0; p < n; p++)
            point_rows(R, D, x + 3, &C.X[3 * (size_t)idx[p]], &C.nr[3 * (size_t)idx[p]], &C.ns[3 * (size_t)idx[p]], &J[(size_t)12 * p], r[(size_t)2 * p],
                       &J[(size_t)12 * p + 6], r[(size_t)2 * p + 1]);
        double A6[6][6], g6[6], dx[6];
        for (int i = 0; i < 6; i++) {
            for (int j = 0; j < 6; j++) {
                double acc = 0.0;
                for (int k = 0; k < 2 * n; k++) acc = acc + J[(size_t)6 * k + i] * J[(size_t)6 * k + j];
                A6[i][j] = acc;
            }
            double acc = 0.0;
            for (int k = 0; k < 2 * n; k++) acc = acc + J[(size_t)6 * k + i] * r[(size_t)k];
            g6[i] = acc;
        }
        ldlt_solve6(A6, g6, dx);
        out.gnEvals++;
        double mxd = fabs(dx[0]), mnd = fabs(dx[0]);
        for (int i = 1; i < 6; i++) {
            mxd = fabs(dx[i]) > mxd ? fabs(dx[i]) : mxd;
            mnd = fabs(dx[i]) < mnd ? fabs(dx[i]) : mnd;
        }
        if (mxd > 5.0 || mnd > 1.0) { out.gnExit = 1; break; }
        double maxDl = 0.0;
        for (int k = 0; k < 2 * n; k++) {
            const double* Jk = &J[(size_t)6 * k];
            const double dl = fabs(((((Jk[0] * dx[0] + Jk[1] * dx[1]) + Jk[2] * dx[2]) + Jk[3] * dx[3]) + Jk[4] * dx[4]) + Jk[5] * dx[5]);
            if (k == 0) maxDl = dl;
            else if (dl > maxDl) maxDl = dl;
        }
        for (int i = 0; i < 6; i++) x[i] = x[i] - dx[i];
        if (maxDl < 1e-5) { out.gnExit = 2; break; }
    }
    rodrigues2rot(x, out.R, nullptr);
    for (int i = 0; i < 3; i++) out.t[i] = x[3 + i];
    out.planar = planar ? 1 : 0;
}

struct Result {
    int solved = 0, nInliers = 0, noMore = 1, N = 0, minInliers = 0, maxIts = 0, total = 0, exitKind = 0, retIt = -1, nCand = 0;
    float Tcw[16];
    std::vector<uint8_t> inliers;
    std::vector<double> hypRt, candRt;
    std::vector<int> hypInl, hypPlanar, hypEvals, hypExit, cands, candInl, candPlanar;
    std::vector<uint8_t> candMask;
};

static int check_inliers(const orbfe_mlpnp_params& P, const Corr& C, int N, const Pose& T, uint8_t* mask)
{
    const CamP cam = cam_of(P.cam, P.camera_model);
    int cnt = 0;
    for (int m = 0; m < N; m++) {
        const float X = C.x32[3 * (size_t)m], Y = C.x32[3 * (size_t)m + 1], Z = C.x32[3 * (size_t)m + 2];
        const float xc = (float)(((T.R[0] * (double)X + T.R[1] * (double)Y) + T.R[2] * (double)Z) + T.t[0]);
        const float yc = (float)(((T.R[3] * (double)X + T.R[4] * (double)Y) + T.R[5] * (double)Z) + T.t[1]);
        const float zc = (float)(((T.R[6] * (double)X + T.R[7] * (double)Y) + T.R[8] * (double)Z) + T.t[2]);
        float u, v;
        camera_project(cam, xc, yc, zc, u, v);
        const float distX = C.p2d[2 * (size_t)m] - u;
        const float distY = C.p2d[2 * (size_t)m + 1] - v;
        const float error2 = distX * distX + distY * distY;
        mask[m] = error2 < C.maxErr[(size_t)m];
        cnt += mask[m];
    }
    return cnt;
}

static void ransac(const orbfe_mlpnp_params& P, const float* sigma2, const std::vector<KeyPoint>& kp, const std::vector<int>& mpIndex,
                   const std::vector<float>& points, const int* sets, Result& o)
{
    const int n = (int)kp.size();
    std::vector<int> first;
    for (int i = 0; i < n; i++)
        if (mpIndex[(size_t)i] >= 0) first.push_back(i);
    const int N = (int)first.size();
    o = Result();
    o.N = N;
    for (int i = 0; i < 16; i++) o.Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    o.inliers.assign((size_t)n, 0);
    orbfe_mlpnp_plan(&P, N, &o.minInliers, &o.maxIts, &o.total);
    if (o.total == 0) return;
    const int total = o.total, ms = P.min_set;
    Corr C;
    C.X.resize((size_t)3 * N); C.f.resize((size_t)3 * N); C.nr.resize((size_t)3 * N); C.ns.resize((size_t)3 * N);
    C.p2d.resize((size_t)2 * N); C.x32.resize((size_t)3 * N); C.maxErr.resize((size_t)N);
    const CamP cam = cam_of(P.cam, P.camera_model);
    for (int c = 0; c < N; c++) {
        const KeyPoint& k = kp[(size_t)first[(size_t)c]];
        const float* X = &points[(size_t)3 * mpIndex[(size_t)first[(size_t)c]]];
        float rx, ry;
        cam_unproject(cam, P.kb_precision, k.pt.x, k.pt.y, rx, ry);
        const double f[3] = {(double)rx, (double)ry, 1.0};
        const double nrm = norm3(f);
        const double alpha = f[0] >= 0.0 ? -nrm : nrm;
        const double v[3] = {f[0] - alpha, f[1], f[2]};
        const double beta = 2.0 / dot3(v, v);
        for (int j = 0; j < 3; j++) {
            const double w = beta * v[j];
            C.f[3 * (size_t)c + j] = f[j];
            C.nr[3 * (size_t)c + j] = (j == 1 ? 1.0 : 0.0) - w * v[1];
            C.ns[3 * (size_t)c + j] = (j == 2 ? 1.0 : 0.0) - w * v[2];
            C.X[3 * (size_t)c + j] = (double)X[j];
            C.x32[3 * (size_t)c + j] = X[j];
        }
        C.p2d[2 * (size_t)c] = k.pt.x; C.p2d[2 * (size_t)c + 1] = k.pt.y;
        C.maxErr[(size_t)c] = sigma2[k.octave] * P.th2;
    }
    o.hypRt.assign((size_t)total * 12, 0.0);
    o.hypInl.assign((size_t)total, 0); o.hypPlanar.assign((size_t)total, 0); o.hypEvals.assign((size_t)total, 0); o.hypExit.assign((size_t)total, 0);
    o.exitKind = ORBFE_MLPNP_EXIT_FAILED;
    std::vector<uint8_t> mask((size_t)N), bestMask((size_t)N), refMask((size_t)N);
    std::vector<int> sel;
    int best = 0, winner = -1, last = -1;
    Pose winPose, lastPose;
    for (int it = 0; it < total; it++) {  // (:116-203); every hypothesis is evaluated so that the whole info block can be compared
        Pose T;
        compute_pose(C, sets + (size_t)it * ms, ms, T);
        const int cnt = check_inliers(P, C, N, T, mask.data());
        std::memcpy(&o.hypRt[(size_t)it * 12], T.R, sizeof T.R);
        std::memcpy(&o.hypRt[(size_t)it * 12 + 9], T.t, sizeof T.t);
        o.hypInl[(size_t)it] = cnt; o.hypPlanar[(size_t)it] = T.planar; o.hypEvals[(size_t)it] = T.gnEvals; o.hypExit[(size_t)it] = T.gnExit;
        if (!(cnt >= o.minInliers && cnt > best)) continue;  // a qualifying hypothesis that sets no new best re-runs a Refine that failed
        best = cnt;
        sel.clear();
        for (int m = 0; m < N; m++)
            if (mask[(size_t)m]) sel.push_back(m);
        Pose Rf;
        compute_pose(C, sel.data(), (int)sel.size(), Rf);
        const int rc = check_inliers(P, C, N, Rf, refMask.data());
        o.cands.push_back(it);
        o.candRt.insert(o.candRt.end(), Rf.R, Rf.R + 9);
        o.candRt.insert(o.candRt.end(), Rf.t, Rf.t + 3);
        o.candInl.push_back(rc); o.candPlanar.push_back(Rf.planar);
        o.candMask.insert(o.candMask.end(), refMask.begin(), refMask.end());
        last = it; lastPose = T; bestMask = mask;
        if (winner < 0 && rc > o.minInliers) {
            winner = it; winPose = Rf;
            o.nInliers = rc;
            for (int m = 0; m < N; m++) o.inliers[(size_t)first[(size_t)m]] = refMask[(size_t)m];
        }
    }
    o.nCand = (int)o.cands.size();
    const Pose* ret = nullptr;
    if (winner >= 0) { o.exitKind = ORBFE_MLPNP_EXIT_REFINED; o.retIt = winner; o.noMore = 0; ret = &winPose; }
    else if (last >= 0) {
        o.exitKind = ORBFE_MLPNP_EXIT_BEST_UNREFINED; o.retIt = last; ret = &lastPose;
        o.nInliers = best;
        for (int m = 0; m < N; m++) o.inliers[(size_t)first[(size_t)m]] = bestMask[(size_t)m];
    }
    if (!ret) return;
    o.solved = 1;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o.Tcw[4 * i + j] = (float)ret->R[3 * i + j];
        o.Tcw[4 * i + 3] = (float)ret->t[i];
    }
}

}  // namespace s13

template <class T>
static void put(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

static void write_result(const char* path, const s13::Result& r)
{
    std::ofstream f(path, std::ios::binary);
    const int head[10] = {r.solved, r.nInliers, r.noMore, r.N, r.minInliers, r.maxIts, r.total, r.exitKind, r.retIt, r.nCand};
    put(f, head, 10); put(f, r.Tcw, 16); put(f, r.inliers.data(), r.inliers.size());
    put(f, r.hypRt.data(), r.hypRt.size()); put(f, r.hypInl.data(), r.hypInl.size()); put(f, r.hypPlanar.data(), r.hypPlanar.size());
    put(f, r.hypEvals.data(), r.hypEvals.size()); put(f, r.hypExit.data(), r.hypExit.size()); put(f, r.cands.data(), r.cands.size());
    put(f, r.candRt.data(), r.candRt.size()); put(f, r.candInl.data(), r.candInl.size()); put(f, r.candPlanar.data(), r.candPlanar.size());
    put(f, r.candMask.data(), r.candMask.size());
}

static int same(const s13::Result& a, const s13::Result& b)
{
    auto eq = [](const auto& x, const auto& y) { return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0]))); };
    return a.solved == b.solved && a.nInliers == b.nInliers && a.noMore == b.noMore && a.N == b.N && a.minInliers == b.minInliers &&
           a.maxIts == b.maxIts && a.total == b.total && a.exitKind == b.exitKind && a.retIt == b.retIt && a.nCand == b.nCand &&
           !std::memcmp(a.Tcw, b.Tcw, sizeof a.Tcw) && eq(a.inliers, b.inliers) && eq(a.hypRt, b.hypRt) && eq(a.hypInl, b.hypInl) &&
           eq(a.hypPlanar, b.hypPlanar) && eq(a.hypEvals, b.hypEvals) && eq(a.hypExit, b.hypExit) && eq(a.cands, b.cands) &&
           eq(a.candRt, b.candRt) && eq(a.candInl, b.candInl) && eq(a.candPlanar, b.candPlanar) && eq(a.candMask, b.candMask);
}

template <class F>
static double median_us(int reps, F&& fn)
{
    std::vector<double> t;
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream in(argv[1], std::ios::binary);
    int head[9];
    double prob;
    float fl[11];
    in.read(reinterpret_cast<char*>(head), sizeof head);
    in.read(reinterpret_cast<char*>(&prob), sizeof prob);
    in.read(reinterpret_cast<char*>(fl), sizeof fl);
    const int n = head[0], nPoints = head[1], total = head[2], minSet = head[3], nLevels = head[5];
    if (!in || n < 0 || nPoints < 0 || total < 0 || total > 4096 || minSet < 6 || minSet > 64 || nLevels < 1 || nLevels > 32) {
        std::fprintf(stderr, "bad scene header\n");
        return 2;
    }
    float sigma2[32] = {0};
    in.read(reinterpret_cast<char*>(sigma2), (std::streamsize)(nLevels * 4));
    std::vector<KeyPoint> kp((size_t)n);
    std::vector<int> mpIndex((size_t)n), sets((size_t)total * minSet);
    std::vector<float> points((size_t)nPoints * 3);
    in.read(reinterpret_cast<char*>(kp.data()), (std::streamsize)(kp.size() * sizeof(KeyPoint)));
    in.read(reinterpret_cast<char*>(mpIndex.data()), (std::streamsize)(mpIndex.size() * 4));
    in.read(reinterpret_cast<char*>(points.data()), (std::streamsize)(points.size() * 4));
    in.read(reinterpret_cast<char*>(sets.data()), (std::streamsize)(sets.size() * 4));
    if (!in) { std::fprintf(stderr, "short scene file\n"); return 2; }
    orbfe_mlpnp_params P = ORBFE_MLPNP_PARAMS_INIT;
    P.camera_model = head[4];
    for (int i = 0; i < 8; i++) P.cam[i] = fl[i];
    P.kb_precision = fl[8]; P.epsilon = fl[9]; P.th2 = fl[10];
    P.probability = prob; P.min_inliers = head[6]; P.max_iterations = head[7]; P.n_iterations = head[8]; P.min_set = minSet;

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = argc > 3 && !hostOnly ? std::max(std::atoi(argv[3]), 1) : 1;
    s13::Result host;
    s13::ransac(P, sigma2, kp, mpIndex, points, sets.data(), host);
    if (host.total != total) { std::fprintf(stderr, "the scene holds %d sets, the plan asks for %d\n", total, host.total); return 2; }
    if (hostOnly) {
        write_result(argv[2], host);
        std::printf("mlpnp host N=%d total=%d solved=%d exit=%d it=%d\n", host.N, host.total, host.solved, host.exitKind, host.retIt);
        return 0;
    }

    ORBextractor ex(500, 20000, 1.2f, nLevels, 20, 7, 320, 240);  // the handle (its mvLevelSigma2); the extractor itself is not used
    std::vector<std::array<float, 3>> world((size_t)nPoints);
    for (int i = 0; i < nPoints; i++) world[(size_t)i] = {points[(size_t)3 * i], points[(size_t)3 * i + 1], points[(size_t)3 * i + 2]};
    std::vector<const std::array<float, 3>*> matched((size_t)n, nullptr);
    for (int i = 0; i < n; i++)
        if (mpIndex[(size_t)i] >= 0) matched[(size_t)i] = &world[(size_t)mpIndex[(size_t)i]];
    std::array<float, 8> camArr;
    for (int i = 0; i < 8; i++) camArr[(size_t)i] = fl[i];
    s13::Result lib;
    auto call = [&](bool withInfo) {
        MLPnPsolver solver(ex, kp, matched, P.camera_model, camArr, P.kb_precision);
        solver.SetRansacParameters(P.probability, P.min_inliers, P.max_iterations, P.min_set, P.epsilon, P.th2);
        bool noMore = false;
        std::vector<bool> vbInliers;
        int nInliers = 0;
        std::array<float, 16> Tout{};
        orbfe_mlpnp_info info;
        std::memset(&info, 0, sizeof info);
        info.struct_size = (int)sizeof info;
        const int N = solver.correspondences();
        std::vector<uint8_t> hypPlanar((size_t)total + 1), candPlanar((size_t)total + 1);
        if (withInfo) {
            lib = s13::Result();
            lib.hypRt.assign((size_t)total * 12, 0.0); lib.hypInl.assign((size_t)total, 0); lib.hypEvals.assign((size_t)total, 0);
            lib.hypExit.assign((size_t)total, 0); lib.cands.assign((size_t)total + 1, 0); lib.candRt.assign((size_t)(total + 1) * 12, 0.0);
            lib.candInl.assign((size_t)total + 1, 0); lib.candMask.assign((size_t)(total + 1) * (N + 1), 0);
            info.hyp_Rt = lib.hypRt.data(); info.hyp_inliers = lib.hypInl.data(); info.hyp_planar = hypPlanar.data();
            info.hyp_gn_evals = lib.hypEvals.data(); info.hyp_gn_exit = lib.hypExit.data(); info.candidates = lib.cands.data();
            info.cand_Rt = lib.candRt.data(); info.cand_inliers = lib.candInl.data(); info.cand_planar = candPlanar.data();
            info.cand_mask = lib.candMask.data();
        }
        const bool ok = solver.iterate(P.n_iterations, noMore, vbInliers, nInliers, Tout, withInfo ? &info : nullptr, &sets);
        if (!withInfo) return;
        lib.solved = ok; lib.nInliers = nInliers; lib.noMore = noMore; lib.N = info.N; lib.minInliers = info.min_inliers; lib.maxIts = info.max_its;
        lib.total = info.total_iterations; lib.exitKind = info.exit_kind; lib.retIt = info.returning_iteration; lib.nCand = info.n_candidates;
        std::memcpy(lib.Tcw, Tout.data(), sizeof lib.Tcw);
        lib.inliers.assign((size_t)n, 0);
        for (size_t i = 0; i < vbInliers.size(); i++) lib.inliers[i] = vbInliers[i];
        lib.hypPlanar.assign(hypPlanar.begin(), hypPlanar.begin() + total);
        lib.cands.resize((size_t)lib.nCand); lib.candRt.resize((size_t)lib.nCand * 12); lib.candInl.resize((size_t)lib.nCand);
        lib.candPlanar.assign(candPlanar.begin(), candPlanar.begin() + lib.nCand);
        lib.candMask.resize((size_t)lib.nCand * N);
    };
    call(true);
    write_result(argv[2], lib);
    const int hostSame = same(lib, host);
    // a second iterate() on one solver is refused
    int refused = 0;
    {
        MLPnPsolver solver(ex, kp, matched, P.camera_model, camArr, P.kb_precision);
        solver.SetRansacParameters(P.probability, P.min_inliers, P.max_iterations, P.min_set, P.epsilon, P.th2);
        bool nm; std::vector<bool> vb; int ni; std::array<float, 16> T{};
        solver.iterate(P.n_iterations, nm, vb, ni, T, nullptr, &sets);
        try { solver.iterate(P.n_iterations, nm, vb, ni, T, nullptr, &sets); } catch (const std::logic_error&) { refused = 1; }
    }
    cpu_set_t one;
    CPU_ZERO(&one);
    CPU_SET(sched_getcpu(), &one);
    sched_setaffinity(0, sizeof one, &one);
    const double tCall = median_us(reps, [&] { call(false); });
    s13::Result tmp;
    const double tHost = median_us(reps, [&] { s13::ransac(P, sigma2, kp, mpIndex, points, sets.data(), tmp); });
    std::printf("mlpnp N=%d total=%d solved=%d exit=%d it=%d candidates=%d\n", lib.N, lib.total, lib.solved, lib.exitKind, lib.retIt, lib.nCand);
    std::printf("mlpnp_latency_us call=%.1f host_one_thread=%.1f host_same=%d second_iterate_refused=%d\n", tCall, tHost, hostSame, refused);
    return hostSame && refused ? 0 : 1;
}

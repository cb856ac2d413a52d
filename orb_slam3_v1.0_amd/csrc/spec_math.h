// spec_math.h -- the pinned sequences that the kernels and plain host C++ share: the fp32 atan2 and cos/sin of SPEC DECISION S5, the
// camera projection of S8 and the binary64 sin / cos / acos / cbrt of S13.  Every operation is a single IEEE-754
// operation; every including unit is built with -ffp-contract=off, so no FMA is formed.  No HIP here: tests/cpp/*.cpp include this
// text as host C++ instead of copying it (device_math.h adds what needs the device's intrinsics).
#pragma once
#include <cmath>

#include "host_device.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

ORBFE_HD inline float spec_atan2f(float y, float x)
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
ORBFE_HD inline void cos_sin_deg(float deg, float& c, float& s)
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

// GeometricCamera::project of the two camera models (src/CameraModels/Pinhole.cpp:41-47,
// src/CameraModels/KannalaBrandt8.cpp:66-83), same operation sequence as oracle/match_oracle.c camera_project.
// `Frustum` is orbfe_frustum (include/orbfe.h); a template keeps this header free of the C ABI include.
template <class Frustum>
ORBFE_HD inline void camera_project(const Frustum& F, float x, float y, float z, float& u, float& v)
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

// ---- SPEC DECISION S13: binary64 sin / cos / acos / cbrt as sequences of + - x / sqrt and the exact floor / frexp / ldexp ----
// (ocml and glibc differ in the last place).  The same constants and operation order as tests/mlpnp_ref.py sincos64 / acos64 /
// cbrt64; tests/test_mlpnp.py compares the tables below with the restatement's.
constexpr double kTwoOverPi = 0x1.45f306dc9c883p-1;
constexpr double kPio2_1 = 0x1.921fb54400000p+0, kPio2_2 = 0x1.0b4611a600000p-34, kPio2_3 = 0x1.3198a2e037073p-69;  // pi / 2 in three parts (33 + 33 + 53 bits)
constexpr double kPio2Hi = 0x1.921fb54442d18p+0, kPio2Lo = 0x1.1a62633145c07p-54, kPiHi = 0x1.921fb54442d18p+1, kPiLo = 0x1.1a62633145c07p-53;
constexpr double kSinC[9] = {-0x1.5555555555555p-3, 0x1.1111111111111p-7, -0x1.a01a01a01a01ap-13, 0x1.71de3a556c734p-19, -0x1.ae64567f544e4p-26, 0x1.6124613a86d09p-33, -0x1.ae7f3e733b81fp-41, 0x1.952c77030ad4ap-49, -0x1.2f49b46814157p-57};  // (-1)^k / (2k + 1)!, k = 1 .. 9
constexpr double kCosC[10] = {-0x1.0000000000000p-1, 0x1.5555555555555p-5, -0x1.6c16c16c16c17p-10, 0x1.a01a01a01a01ap-16, -0x1.27e4fb7789f5cp-22, 0x1.1eed8eff8d898p-29, -0x1.93974a8c07c9dp-37, 0x1.ae7f3e733b81fp-45, -0x1.6827863b97d97p-53, 0x1.e542ba4020225p-62};  // (-1)^k / (2k)!, k = 1 .. 10
constexpr double kAsinC[28] = {0x1.5555555555555p-3, 0x1.3333333333333p-4, 0x1.6db6db6db6db7p-5, 0x1.f1c71c71c71c7p-6, 0x1.6e8ba2e8ba2e9p-6, 0x1.1c4ec4ec4ec4fp-6, 0x1.c99999999999ap-7, 0x1.7a87878787878p-7, 0x1.3fde50d79435ep-7, 0x1.12ef3cf3cf3cfp-7, 0x1.df3bd37a6f4dfp-8, 0x1.a6863d70a3d71p-8, 0x1.782dda12f684cp-8, 0x1.51ba308d3dcb1p-8, 0x1.31683bdef7bdfp-8, 0x1.15ee9d45d1746p-8, 0x1.fcaf8fb6db6dbp-9, 0x1.d3d2a8e0dd67dp-9, 0x1.b026f57b13b14p-9, 0x1.90cb77f60c7cep-9, 0x1.750de64d7d05fp-9, 0x1.5c5f56efaaaabp-9, 0x1.464c0950f7d47p-9, 0x1.3275586c5f2f0p-9, 0x1.208d3570ae5a6p-9, 0x1.1052bc5fa960ap-9, 0x1.018f963c229bfp-9, 0x1.e82be60d9127ep-10};  // (2k)! / (4^k k!^2 (2k + 1)), k = 1 .. 28
constexpr double kCbrtA = 0.75, kCbrtB = 0.22;
constexpr int kCbrtNewton = 6;

template <int N>
ORBFE_HD inline double horner64(double z, const double (&c)[N])
{
    double p = c[N - 1];
    ORBFE_UNROLL
    for (int k = N - 2; k >= 0; k--) p = p * z + c[k];
    return p;
}

// sin x and cos x for 0 <= x < 2^20 (NaN elsewhere): k = floor(x * 2/pi + 0.5), r = ((x - k P1) - k P2) - k P3, Taylor polynomials
// of r by Horner in z = r * r, picked and signed by the quadrant k mod 4
ORBFE_HD inline void spec_sincos64(double x, double& s, double& c)
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
ORBFE_HD inline double spec_acos64(double x)
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
ORBFE_HD inline double spec_cbrt64(double x)
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

// ---- SPEC DECISION S26: MapPoint::UpdateDepth (src/MapPoint.cc:458-472) in binary32 ----
// dist = |Pos - centre| as sqrt((x x + y y) + z z), every operation rounded once (sqrtf and the division are correctly rounded on both
// sides); max = dist * sf[level], min = max / sf[nLevels - 1]
ORBFE_HD inline float spec_point_distance(float px, float py, float pz, float cx, float cy, float cz)
{
    const float x = px - cx, y = py - cy, z = pz - cz;
    const float xx = x * x, yy = y * y, zz = z * z;
    const float s = xx + yy;
    return sqrtf(s + zz);
}
ORBFE_HD inline void spec_update_depth(float dist, float levelScale, float lastScale, float& minDistance, float& maxDistance)
{
    maxDistance = dist * levelScale;
    minDistance = maxDistance / lastScale;
}

}  // namespace orbfe

// device_math.h -- the pinned fp32 sequences of SPEC DECISION S5 for gfx950.
// Replaces atan2f (src/cuda/Angle_gpu.cu:73) and cosf/sinf (src/cuda/Orb_gpu.cu:329) of the
// reference, whose last bits depend on the CUDA math library.  Every operation is a single
// IEEE-754 fp32 op; the translation unit is compiled with -ffp-contract=off so no FMA is formed.
// The sequences that host C++ shares (spec_atan2f, cos_sin_deg, camera_project, the binary64 block of S13) are in spec_math.h; what
// is left here needs the device's intrinsics.
#pragma once
#include <hip/hip_runtime.h>

#include "spec_math.h"

#pragma clang fp contract(off)

namespace orbfe {

__device__ __forceinline__ int reflect101(int i, int n)
{
    // BORDER_REFLECT_101 for any offset (period 2n-2); n >= 2 on every pyramid level
    const int p = 2 * n - 2;
    i = i % p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// REFLECT_101 for overshoots smaller than n (one bounce, no modulo), clamped so that the result is
// always a valid index even in a caller's don't-care region
__device__ __forceinline__ int reflect_near(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * n - 2 - i : i;
    return min(max(i, 0), n - 1);
}

// src/cuda/Angle_gpu.cu:73-75
__device__ __forceinline__ float atan2_deg(float m01, float m10)
{
    const float kPi = 0x1.921fb6p+1f;
    float d = spec_atan2f(m01, m10);
    if (d < 0.0f) d = d + 2.0f * kPi;
    d = d * (180.0f / kPi);
    return d;
}

// SPEC DECISION S8: natural logarithm of MapPoint::PredictScale (src/MapPoint.cc:580), same operation
// sequence as oracle/match_oracle.c orc_spec_logf: x = m * 2^e, m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s)
// with s = (m-1)/(m+1) as a degree-4 polynomial in s^2; contraction is off for this translation unit.
__device__ __forceinline__ float spec_logf(float x)
{
    if (!(x > 0.0f)) return -INFINITY;
    if (x > 3.0e38f) return INFINITY;
    int e;
    float m = frexpf(x, &e);
    if (m < 0x1.6a09e6p-1f) {
        m = m * 2.0f;
        e -= 1;
    }
    const float s = __fdiv_rn(m - 1.0f, m + 1.0f);
    const float z = s * s;
    float p = 0x1.c71c72p-4f;
    p = p * z + 0x1.24924ap-3f;
    p = p * z + 0x1.99999ap-3f;
    p = p * z + 0x1.555556p-2f;
    p = p * z;
    const float t = s + s;
    const float r = t + t * p;
    const float ef = (float)e;
    return ef * 0x1.62ep-1f + (r + ef * 0x1.0bfbe8p-15f);
}

// MapPoint::PredictScale (src/MapPoint.cc:580-612) on the pinned logarithm, SPEC DECISION S8
__device__ __forceinline__ int predict_scale(float maxDistance, float dist, float logScaleFactor, int nLevels)
{
    const float ratio = __fdiv_rn(maxDistance, dist);
    const float q = __fdiv_rn(spec_logf(ratio), logScaleFactor);
    int lvl;
    if (!(q > 0.0f)) lvl = 0;
    else if (q >= (float)nLevels) lvl = nLevels - 1;
    else {
        lvl = (int)ceilf(q);
        if (lvl >= nLevels) lvl = nLevels - 1;
    }
    return lvl;
}

// R * (X, Y, Z) + t for a row-major 3 x 3 R, in the parenthesisation SPEC DECISION S8 pins: ((r0 X + r1 Y) + r2 Z) + t
__device__ __forceinline__ void rigid_transform(const float (&R)[9], const float (&t)[3], float X, float Y, float Z, float& x,
                                                float& y, float& z)
{
    x = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0];
    y = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
    z = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
}

}  // namespace orbfe

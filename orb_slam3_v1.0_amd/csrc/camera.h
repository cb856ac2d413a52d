// camera.h -- GeometricCamera::unproject of the two camera models (SPEC DECISION S10), shared by kernels_match_tri.hip and
// kernels_mlpnp.hip.  Same sequence as oracle/match_oracle.c kb8_unproject; contraction is off in every including unit.
// No HIP here: tests/cpp/mlpnp.cpp includes this text as host C++.
#pragma once
#include "spec_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace orbfe {

struct CamP {
    float fx, fy, cx, cy, k1, k2, k3, k4;
    int camera_model;
};

ORBFE_HD inline CamP cam_of(const float (&c)[8], int model)
{
    return CamP{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], model};
}

ORBFE_HD inline void cam_unproject(const CamP& C, float precision, float u, float v, float& rx, float& ry)
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

}  // namespace orbfe

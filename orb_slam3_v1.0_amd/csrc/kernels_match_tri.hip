// kernels_match_tri.hip -- ORBmatcher::SearchForTriangulation on gfx950.
//
// Replaces src/ORBmatcher.cc:441-676 for one pinhole camera per key frame (callers src/LocalMapping.cc:488, up
// to 30 neighbour key frames per new key frame) and Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:104-131).
// This fork never sets vbMatched2, so every key-frame-1 feature picks its partner independently of the others:
// one thread per feature of key frame 1 walks the features of key frame 2 that share its vocabulary node
// (sequentially, so the "dist > bestDist -> continue" rule keeps the LAST candidate among equal distances, as in
// the reference), then one block applies the rotation histogram (ComputeThreeMaxima).  Distances are __popcll
// over 4 x 64-bit words; the geometric gates are SPEC DECISION S8 binary32 arithmetic.
#include <algorithm>
#include <cstring>

#include <vector>

#include "match_common.h"
#include "device_math.h"
#include "camera.h"
#include "keyframe.h"
#include "jacobi.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

struct TriArgs {
    int nPos1;                    // entries of idx1 (features of key frame 1 that sit in a shared node)
    const int* idx1;              // [nPos1]
    const int* grp1;              // [nPos1] group of every entry
    const int* off2;              // [G + 1]
    const int* idx2;
    const orbfe_keypoint* kp1;
    const orbfe_keypoint* kp2;
    const uint8_t* desc1;
    const uint8_t* desc2;
    const uint8_t* hasMP1;
    const uint8_t* hasMP2;
    const uint8_t* stereo1;       // or null
    const uint8_t* stereo2;
    const float* sf2;
    float F12[9];
    float epx, epy;
    int onlyStereo, coarse, checkOrientation;
    int model1, model2, kf1HasCamera2;
    float cam1[8], cam2[8], kbPrecision;
    float R12[9], t12[3];
    float sigma2_1[kMaxLevels];
    int n1;
    int* match12;                 // [n1]
    int* binOf;                   // [n1]
    int* nMatches;
};


// ---- KannalaBrandt8::epipolarConstrain (src/CameraModels/KannalaBrandt8.cpp:216-220 -> TriangulateMatches :306-370) ----
// SPEC DECISION S10.  binary32, one operation per line, no contraction, except the null vector of the 4x4 system, which the
// reference takes from an Eigen JacobiSVD (not reproducible): here A^T A in binary64, eight cyclic Jacobi sweeps in the
// fixed pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), eigenvector of the smallest eigenvalue (lowest index on ties).
// tan(theta) of unproject is sin / cos of the S5 sequences.  Same sequence as oracle/match_oracle.c kb8_epipolar.
__device__ inline bool kb8_epipolar(const CamP& C1, const CamP& C2, float precision, float u1, float v1, float u2, float v2,
                                    const float (&R12)[9], const float (&t12)[3], float sigmaLevel, float unc)
{
    float r1x, r1y, r2x, r2y;
    cam_unproject(C1, precision, u1, v1, r1x, r1y);  // rays (x, y, 1)
    cam_unproject(C2, precision, u2, v2, r2x, r2y);
    // parallax (:313-319)
    const float r21x = (R12[0] * r2x + R12[1] * r2y) + R12[2];
    const float r21y = (R12[3] * r2x + R12[4] * r2y) + R12[5];
    const float r21z = (R12[6] * r2x + R12[7] * r2y) + R12[8];
    const float dot = (r1x * r21x + r1y * r21y) + r21z;
    const float n1 = sqrtf((r1x * r1x + r1y * r1y) + 1.0f);
    const float n2 = sqrtf((r21x * r21x + r21y * r21y) + r21z * r21z);
    const float cosParallax = dot / (n1 * n2);
    if ((double)cosParallax > 0.9998) return false;
    // Tcw2 = [R21 | -R21 t12], R21 = R12^T (:333-336)
    float R21[9], tc[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R21[3 * i + j] = R12[3 * j + i];
    for (int i = 0; i < 3; i++) tc[i] = -((R21[3 * i] * t12[0] + R21[3 * i + 1] * t12[1]) + R21[3 * i + 2] * t12[2]);
    // A (:401-405) with Tcw1 = [I | 0]
    float A[4][4];
    A[0][0] = -1.0f; A[0][1] = 0.0f; A[0][2] = r1x; A[0][3] = 0.0f;
    A[1][0] = 0.0f; A[1][1] = -1.0f; A[1][2] = r1y; A[1][3] = 0.0f;
    for (int j = 0; j < 3; j++) {
        A[2][j] = r2x * R21[6 + j] - R21[j];
        A[3][j] = r2y * R21[6 + j] - R21[3 + j];
    }
    A[2][3] = r2x * tc[2] - tc[0];
    A[3][3] = r2y * tc[2] - tc[1];
    double M[4][4], vv[4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc = acc + (double)A[k][i] * (double)A[k][j];
            M[i][j] = acc;
        }
    sym4_min_eigenvector(M, vv);
    const float X = (float)(vv[0] / vv[3]), Y = (float)(vv[1] / vv[3]), Z = (float)(vv[2] / vv[3]);
    if (!(Z > 0.0f)) return false;  // :343-346 (NaN fails, as a comparison "<= 0" on NaN would pass in the reference: S10)
    const float z2 = ((R21[6] * X + R21[7] * Y) + R21[8] * Z) + tc[2];
    if (!(z2 > 0.0f)) return false;  // :348-351
    float pu, pv;
    camera_project(C1, X, Y, Z, pu, pv);  // :354-361
    const float e1x = pu - u1, e1y = pv - v1;
    if ((double)(e1x * e1x + e1y * e1y) > 5.991 * (double)sigmaLevel) return false;
    const float X2 = ((R21[0] * X + R21[1] * Y) + R21[2] * Z) + tc[0];
    const float Y2 = ((R21[3] * X + R21[4] * Y) + R21[5] * Z) + tc[1];
    camera_project(C2, X2, Y2, z2, pu, pv);  // :363-371
    const float e2x = pu - u2, e2y = pv - v2;
    if ((double)(e2x * e2x + e2y * e2y) > 5.991 * (double)unc) return false;
    return Z > 0.0001f;  // :218-219
}

__global__ __launch_bounds__(256) void tri_match_kernel(TriArgs A)
{
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= A.nPos1) return;
    const int idx1 = A.idx1[pos];
    if (A.hasMP1[idx1]) return;  // :506-509
    const bool bStereo1 = A.stereo1 && A.stereo1[idx1];
    if (A.onlyStereo && !bStereo1) return;
    const orbfe_keypoint k1 = A.kp1[idx1];
    unsigned long long d4[4];
    const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(A.desc1 + (size_t)idx1 * 32);
    d4[0] = dp[0]; d4[1] = dp[1]; d4[2] = dp[2]; d4[3] = dp[3];
    // epipolar line of k1 in image 2, Pinhole.cpp:112-114
    const float a = (k1.x * A.F12[0] + k1.y * A.F12[3]) + A.F12[6];
    const float b = (k1.x * A.F12[1] + k1.y * A.F12[4]) + A.F12[7];
    const float c = (k1.x * A.F12[2] + k1.y * A.F12[5]) + A.F12[8];
    const float den = a * a + b * b;
    const int g = A.grp1[pos];
    int bestDist = ORBFE_TH_LOW, bestIdx2 = -1;
    for (int i2 = A.off2[g]; i2 < A.off2[g + 1]; i2++) {
        const int idx2 = A.idx2[i2];
        if (A.hasMP2[idx2]) continue;  // :531
        const bool bStereo2 = A.stereo2 && A.stereo2[idx2];
        if (A.onlyStereo && !bStereo2) continue;
        const int dist = hamming256(reinterpret_cast<const uint2*>(A.desc2 + (size_t)idx2 * 32), d4);
        if (dist > ORBFE_TH_LOW || dist > bestDist) continue;  // :545
        const orbfe_keypoint k2 = A.kp2[idx2];
        if (!bStereo1 && !bStereo2 && !A.kf1HasCamera2) {  // :551-565
            const float distex = A.epx - k2.x, distey = A.epy - k2.y;
            const float err = distex * distex + distey * distey;
            if (err < 100 * A.sf2[k2.octave]) continue;
        }
        bool ok = false;
        if (A.model1 == ORBFE_CAMERA_KANNALA_BRANDT8) {  // block-uniform
            if (!A.coarse)  // (the reference evaluates it either way; its result is only used without bCoarse)
                ok = kb8_epipolar(cam_of(A.cam1, A.model1), cam_of(A.cam2, A.model2), A.kbPrecision, k1.x, k1.y, k2.x, k2.y, A.R12,
                                  A.t12, A.sigma2_1[k1.octave], 1.0f);
        } else {
            const float num = (a * k2.x + b * k2.y) + c;
            if (den != 0) {
                const float dsqr = num * num / den;
                ok = (double)dsqr < 3.84 * 1.0;
            }
        }
        if (A.coarse || ok) {
            bestIdx2 = idx2;
            bestDist = dist;
        }
    }
    if (bestIdx2 >= 0) {
        A.match12[idx1] = bestIdx2;
        if (A.checkOrientation) A.binOf[idx1] = rotation_bin(k1.angle, A.kp2[bestIdx2].angle);
    }
}

// rotation filter (match_common.h) over the features of key frame 1; single block
__global__ __launch_bounds__(256) void tri_finalize_kernel(TriArgs A)
{
    rotation_filter_block(
        A.n1, A.checkOrientation, [&](int j) { return A.match12[j] >= 0; }, [&](int j) { return A.binOf[j]; },
        [&](int j) { A.match12[j] = -1; }, A.nMatches);
}

// ---------------------------------------------------------------------------------------------
// One key frame against K neighbours in ONE launch (LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:455-488: up to
// 30 SearchForTriangulation calls per new key frame).  Key frames are RESIDENT in HBM (keyframe.h): keypoints,
// descriptors and the FeatureVector as "features sorted by (vocabulary node, index)" + the list of distinct nodes, so a
// call moves only what changes between calls -- the has-map-point flags and the per-pair geometry.  blockIdx.y = neighbour,
// one thread per feature of key frame 1: binary search of its node in the neighbour's node list (staged in LDS), then the
// sequential walk of that node's features exactly as tri_match_kernel does.
// The rotation histogram is NOT applied here: between two neighbours the host turns matches into map points
// (:500-700), and a feature of key frame 1 that received one is skipped for all later neighbours (:506-509) -- which also
// changes their histograms.  The kernel therefore returns the RAW match and its rotation bin per (neighbour, feature),
// computed from the has-map-point flags at the time of the call; orbfe_triangulation_select applies "skip the features
// that got a map point meanwhile", the histogram and ComputeThreeMaxima for one neighbour at a time on the host.  Exact:
// vbMatched2 is never set in this fork (:485,537), so every feature of key frame 1 chooses on its own and dropping one
// never changes another's choice.
// ---------------------------------------------------------------------------------------------
struct TriNeighbour {  // device-side argument block of one (key frame 1, neighbour) pair
    const orbfe_keypoint* kp2;
    const uint8_t* desc2;
    const uint8_t* stereo2;   // or null
    const float* sf2;
    const int* nodeList2;     // [G2] distinct vocabulary nodes of the neighbour, ascending
    const int* nodeOff2;      // [G2 + 1]
    const int* order2;        // features of the neighbour sorted by (node, index)
    const uint8_t* hasMP2;    // [n2] flags of THIS call
    int G2, n2;
    float F12[9];
    float epx, epy;
    int onlyStereo, coarse, checkOrientation;
    int model1, model2, kf1HasCamera2;
    float cam1[8], cam2[8], kbPrecision;
    float R12[9], t12[3];
    float sigma2_1[kMaxLevels];
};

constexpr int kTriNodeLds = 4096;  // distinct nodes of a neighbour staged in LDS (more: the search reads global memory)

__global__ __launch_bounds__(256) void tri_batch_kernel(const TriNeighbour* __restrict__ nbs, int n1,
                                                        const orbfe_keypoint* __restrict__ kp1, const uint8_t* __restrict__ desc1,
                                                        const int* __restrict__ node1, const uint8_t* __restrict__ stereo1,
                                                        const uint8_t* __restrict__ hasMP1, int* __restrict__ rawMatch,
                                                        uint8_t* __restrict__ rawBin)
{
    __shared__ int sNodes[kTriNodeLds];
    const int k = blockIdx.y;
    const TriNeighbour& A = nbs[k];
    const int G2 = A.G2;
    const bool nodesInLds = G2 <= kTriNodeLds;  // block-uniform
    if (nodesInLds)
        for (int g = threadIdx.x; g < G2; g += 256) sNodes[g] = A.nodeList2[g];
    __syncthreads();
    const int idx1 = blockIdx.x * 256 + threadIdx.x;
    if (idx1 >= n1) return;
    int bestDist = ORBFE_TH_LOW, bestIdx2 = -1, bin = 0;
    const int nid = node1[idx1];
    const bool bStereo1 = stereo1 && stereo1[idx1];
    if (nid >= 0 && !hasMP1[idx1] && !(A.onlyStereo && !bStereo1)) {  // :506-509
        int lo = 0, hi = G2;  // lower bound of nid in the neighbour's node list
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int v = nodesInLds ? sNodes[mid] : A.nodeList2[mid];
            if (v < nid) lo = mid + 1;
            else hi = mid;
        }
        const bool shared = lo < G2 && (nodesInLds ? sNodes[lo] : A.nodeList2[lo]) == nid;
        if (shared) {
            const orbfe_keypoint k1 = kp1[idx1];
            unsigned long long d4[4];
            const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(desc1 + (size_t)idx1 * 32);
            d4[0] = dp[0]; d4[1] = dp[1]; d4[2] = dp[2]; d4[3] = dp[3];
            const float a = (k1.x * A.F12[0] + k1.y * A.F12[3]) + A.F12[6];  // Pinhole.cpp:112-114
            const float b = (k1.x * A.F12[1] + k1.y * A.F12[4]) + A.F12[7];
            const float c = (k1.x * A.F12[2] + k1.y * A.F12[5]) + A.F12[8];
            const float den = a * a + b * b;
            for (int i2 = A.nodeOff2[lo]; i2 < A.nodeOff2[lo + 1]; i2++) {
                const int idx2 = A.order2[i2];
                if (A.hasMP2[idx2]) continue;  // :531
                const bool bStereo2 = A.stereo2 && A.stereo2[idx2];
                if (A.onlyStereo && !bStereo2) continue;
                const int dist = hamming256(reinterpret_cast<const uint2*>(A.desc2 + (size_t)idx2 * 32), d4);
                if (dist > ORBFE_TH_LOW || dist > bestDist) continue;  // :545
                const orbfe_keypoint k2 = A.kp2[idx2];
                if (!bStereo1 && !bStereo2 && !A.kf1HasCamera2) {  // :551-565
                    const float distex = A.epx - k2.x, distey = A.epy - k2.y;
                    const float err = distex * distex + distey * distey;
                    if (err < 100 * A.sf2[k2.octave]) continue;
                }
                bool ok = false;
                if (A.model1 == ORBFE_CAMERA_KANNALA_BRANDT8) {  // block-uniform
                    if (!A.coarse)
                        ok = kb8_epipolar(cam_of(A.cam1, A.model1), cam_of(A.cam2, A.model2), A.kbPrecision, k1.x, k1.y, k2.x, k2.y,
                                          A.R12, A.t12, A.sigma2_1[k1.octave], 1.0f);
                } else {
                    const float num = (a * k2.x + b * k2.y) + c;
                    if (den != 0) {
                        const float dsqr = num * num / den;
                        ok = (double)dsqr < 3.84 * 1.0;
                    }
                }
                if (A.coarse || ok) {
                    bestIdx2 = idx2;
                    bestDist = dist;
                }
            }
            // :619-627 (the bin is computed always; select uses it only with checkOrientation)
            if (bestIdx2 >= 0) bin = rotation_bin(k1.angle, A.kp2[bestIdx2].angle);
        }
    }
    rawMatch[(size_t)k * n1 + idx1] = bestIdx2;
    rawBin[(size_t)k * n1 + idx1] = (uint8_t)bin;
}

// ---------------------------------------------------------------------------------------------
// "Triangulate each match" of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:571-705) for monocular key frames
// (bStereo1 == bStereo2 == bRight2 == false: the stereo branches :583-586,603-614,651-661,676-686 are unreachable), and
// GeometricTools::Triangulate (src/GeometricTools.cc:47-66).  SPEC DECISION S11: binary32, one operation per line, left to
// right, no contraction; comparisons against the reference's double literals in binary64 on the promoted float; the null
// vector of A by the S10 sequence (sym4_min_eigenvector on A^T A in binary64).  The verdict and the point of a pair depend
// only on the two keypoints, the two poses and the two cameras, so every raw partner of every neighbour is evaluated at
// once and orbfe_triangulation_select's replay only looks the result up.
// ---------------------------------------------------------------------------------------------
struct NewPtNeighbour {  // device-side geometry block of one (key frame 1, neighbour) pair
    const orbfe_keypoint* kp2;
    const float* sf2;
    float tcw1[12], tcw2[12];  // row-major 3 x 4
    float twc1[3], twc2[3];
    int model1, model2;
    float cam1[8], cam2[8], kbPrecision;
    float sigma2_1[kMaxLevels], sigma2_2[kMaxLevels];
    float ratioFactor;
    int inertial, farPoints;
    float thFar;
};

__device__ inline int newpoint_eval(const NewPtNeighbour& G, const orbfe_keypoint& k1, const orbfe_keypoint& k2,
                                    const float* __restrict__ sf1, float& X, float& Y, float& Z)
{
    const float (&T1)[12] = G.tcw1;
    const float (&T2)[12] = G.tcw2;
    const CamP C1 = cam_of(G.cam1, G.model1), C2 = cam_of(G.cam2, G.model2);
    X = 0.0f; Y = 0.0f; Z = 0.0f;
    float x1, y1, x2, y2;
    cam_unproject(C1, G.kbPrecision, k1.x, k1.y, x1, y1);  // xn = (x, y, 1), :572-573
    cam_unproject(C2, G.kbPrecision, k2.x, k2.y, x2, y2);
    // ray = Rwc xn with Rwc = Rcw^T (:575-576)
    const float r1x = (T1[0] * x1 + T1[4] * y1) + T1[8] * 1.0f;
    const float r1y = (T1[1] * x1 + T1[5] * y1) + T1[9] * 1.0f;
    const float r1z = (T1[2] * x1 + T1[6] * y1) + T1[10] * 1.0f;
    const float r2x = (T2[0] * x2 + T2[4] * y2) + T2[8] * 1.0f;
    const float r2y = (T2[1] * x2 + T2[5] * y2) + T2[9] * 1.0f;
    const float r2z = (T2[2] * x2 + T2[6] * y2) + T2[10] * 1.0f;
    const float dot = (r1x * r2x + r1y * r2y) + r1z * r2z;
    const float n1 = sqrtf((r1x * r1x + r1y * r1y) + r1z * r1z);
    const float n2 = sqrtf((r2x * r2x + r2y * r2y) + r2z * r2z);
    const float cosParallax = dot / (n1 * n2);  // :577
    const double limit = G.inertial ? 0.9996 : 0.9998;
    if (!(cosParallax > 0.0f && (double)cosParallax < limit)) return ORBFE_NEWPT_LOW_PARALLAX;  // :596-597, :615-618
    // GeometricTools::Triangulate (src/GeometricTools.cc:49-53)
    float A[4][4];
    for (int j = 0; j < 4; j++) {
        A[0][j] = x1 * T1[8 + j] - T1[j];
        A[1][j] = y1 * T1[8 + j] - T1[4 + j];
        A[2][j] = x2 * T2[8 + j] - T2[j];
        A[3][j] = y2 * T2[8 + j] - T2[4 + j];
    }
    double M[4][4], vv[4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc = acc + (double)A[k][i] * (double)A[k][j];
            M[i][j] = acc;
        }
    sym4_min_eigenvector(M, vv);
    if (vv[3] == 0.0) return ORBFE_NEWPT_AT_INFINITY;  // :59
    X = (float)(vv[0] / vv[3]);
    Y = (float)(vv[1] / vv[3]);
    Z = (float)(vv[2] / vv[3]);
    const float z1 = ((T1[8] * X + T1[9] * Y) + T1[10] * Z) + T1[11];  // :627
    if (!(z1 > 0.0f)) return ORBFE_NEWPT_BEHIND_1;  // NaN fails (S10)
    const float z2 = ((T2[8] * X + T2[9] * Y) + T2[10] * Z) + T2[11];  // :631
    if (!(z2 > 0.0f)) return ORBFE_NEWPT_BEHIND_2;
    const float xc1 = ((T1[0] * X + T1[1] * Y) + T1[2] * Z) + T1[3];  // :637-638
    const float yc1 = ((T1[4] * X + T1[5] * Y) + T1[6] * Z) + T1[7];
    float pu, pv;
    camera_project(C1, xc1, yc1, z1, pu, pv);  // :643
    const float e1x = pu - k1.x, e1y = pv - k1.y;
    if ((double)(e1x * e1x + e1y * e1y) > 5.991 * (double)G.sigma2_1[k1.octave]) return ORBFE_NEWPT_REPROJECTION_1;  // :647
    const float xc2 = ((T2[0] * X + T2[1] * Y) + T2[2] * Z) + T2[3];  // :665-666
    const float yc2 = ((T2[4] * X + T2[5] * Y) + T2[6] * Z) + T2[7];
    camera_project(C2, xc2, yc2, z2, pu, pv);  // :670
    const float e2x = pu - k2.x, e2y = pv - k2.y;
    if ((double)(e2x * e2x + e2y * e2y) > 5.991 * (double)G.sigma2_2[k2.octave]) return ORBFE_NEWPT_REPROJECTION_2;  // :673
    // scale consistency (:689-705)
    const float d1x = X - G.twc1[0], d1y = Y - G.twc1[1], d1z = Z - G.twc1[2];
    const float dist1 = sqrtf((d1x * d1x + d1y * d1y) + d1z * d1z);
    const float d2x = X - G.twc2[0], d2y = Y - G.twc2[1], d2z = Z - G.twc2[2];
    const float dist2 = sqrtf((d2x * d2x + d2y * d2y) + d2z * d2z);
    if (dist1 == 0.0f || dist2 == 0.0f) return ORBFE_NEWPT_ZERO_DISTANCE;  // :695
    if (G.farPoints && (dist1 >= G.thFar || dist2 >= G.thFar)) return ORBFE_NEWPT_FAR;  // :698
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = sf1[k1.octave] / G.sf2[k2.octave];
    if (ratioDist * G.ratioFactor < ratioOctave || ratioDist > ratioOctave * G.ratioFactor) return ORBFE_NEWPT_SCALE;  // :704
    return ORBFE_NEWPT_ACCEPTED;
}

// One thread per (neighbour blockIdx.y, entry): entry = feature i1 of key frame 1 with partner[k * n + i1] (the raw matches of
// tri_batch_kernel, launched behind it on the same stream), or, with idx1List, pair p = (idx1List[p], partner[p]) of an
// explicit list.  The chain is ~48 dependent binary64 Jacobi rotations: latency, not throughput, so blocks are one wave wide
// to spread the entries with a partner over as many CUs as there are.
__global__ __launch_bounds__(64) void newpoints_kernel(const NewPtNeighbour* __restrict__ nbs, int n,
                                                       const orbfe_keypoint* __restrict__ kp1, const float* __restrict__ sf1,
                                                       const int* __restrict__ idx1List, const int* __restrict__ partner,
                                                       float* __restrict__ x3d, uint8_t* __restrict__ verdict)
{
    const int k = blockIdx.y;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n) return;
    const NewPtNeighbour& G = nbs[k];
    const size_t o = (size_t)k * n + e;
    const int i2 = partner[o];
    float X = 0.0f, Y = 0.0f, Z = 0.0f;
    int v = ORBFE_NEWPT_NO_PARTNER;
    if (i2 >= 0) {
        const int i1 = idx1List ? idx1List[e] : e;
        const orbfe_keypoint k1 = kp1[i1];
        const orbfe_keypoint k2 = G.kp2[i2];
        v = newpoint_eval(G, k1, k2, sf1, X, Y, Z);  // (0, 0, 0) where no point exists
    }
    x3d[3 * o] = X;
    x3d[3 * o + 1] = Y;
    x3d[3 * o + 2] = Z;
    verdict[o] = (uint8_t)v;
}

void fill_newpt(NewPtNeighbour& G, const KeyFrameDev* F2, const orbfe_newpoint_params& Q)
{
    G.kp2 = F2->kp;
    G.sf2 = F2->sf;
    for (int i = 0; i < 12; i++) { G.tcw1[i] = Q.tcw1[i]; G.tcw2[i] = Q.tcw2[i]; }
    for (int i = 0; i < 3; i++) { G.twc1[i] = Q.twc1[i]; G.twc2[i] = Q.twc2[i]; }
    G.model1 = Q.camera_model1;
    G.model2 = Q.camera_model2;
    for (int i = 0; i < 8; i++) { G.cam1[i] = Q.cam1[i]; G.cam2[i] = Q.cam2[i]; }
    G.kbPrecision = Q.kb_precision;
    for (int i = 0; i < kMaxLevels; i++) { G.sigma2_1[i] = Q.level_sigma2_1[i]; G.sigma2_2[i] = Q.level_sigma2_2[i]; }
    G.ratioFactor = Q.ratio_factor;
    G.inertial = Q.inertial;
    G.farPoints = Q.far_points;
    G.thFar = Q.th_far_points;
}

const char* const kNewPtSizeErr =
    "orbfe_newpoint_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";

}  // namespace

int match_triangulation_run(MatchScratch& m, hipStream_t s, int G, const int* off1, const int* idx1, const int* off2,
                            const int* idx2, int n1, const orbfe_keypoint* kp1, const uint8_t* desc1, const uint8_t* hasMP1,
                            const uint8_t* stereo1, int n2, const orbfe_keypoint* kp2, const uint8_t* desc2,
                            const uint8_t* hasMP2, const uint8_t* stereo2, const float* sf2, int nLevels2,
                            const orbfe_tri_params* P, int* matches12, int* nMatches, std::string& err)
{
    for (int i = 0; i < n1; i++) matches12[i] = -1;
    *nMatches = 0;
    if (G == 0 || n1 == 0 || n2 == 0) return ORBFE_OK;
    const int nPos1 = off1[G], nPos2 = off2[G];
    for (int g = 0; g < G; g++)
        if (off1[g + 1] < off1[g] || off2[g + 1] < off2[g]) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < nPos1; i++)
        if (idx1[i] < 0 || idx1[i] >= n1) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < nPos2; i++)
        if (idx2[i] < 0 || idx2[i] >= n2) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < n2; i++)
        if (kp2[i].octave < 0 || kp2[i].octave >= nLevels2) return ORBFE_ERR_INVALID_ARG;  // indexes mvScaleFactors
    if (nPos1 == 0) return ORBFE_OK;

    Staging st;
    const auto bIdx1 = st.in<int>(nPos1);
    const auto bGrp1 = st.in<int>(nPos1);
    const auto bOff2 = st.in<int>((size_t)G + 1);
    const auto bIdx2 = st.in<int>(std::max(nPos2, 1));
    const auto bKp1 = st.in<orbfe_keypoint>(n1);
    const auto bKp2 = st.in<orbfe_keypoint>(n2);
    const auto bD1 = st.in<uint8_t>((size_t)n1 * 32);
    const auto bD2 = st.in<uint8_t>((size_t)n2 * 32);
    const auto bH1 = st.in<uint8_t>(n1);
    const auto bH2 = st.in<uint8_t>(n2);
    const auto bS1 = st.in<uint8_t>(n1);
    const auto bS2 = st.in<uint8_t>(n2);
    const auto bSf = st.in<float>(nLevels2);
    const auto bMatch = st.out<int>(n1);
    const auto bBin = st.scratch<int>(n1);   // between the two pieces that come down, as the layout always had it
    const auto bNM = st.out<int>(1);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bIdx1, idx1);
    int* grp = st.host(bGrp1);
    for (int g = 0; g < G; g++)
        for (int i = off1[g]; i < off1[g + 1]; i++) grp[i] = g;
    st.put(bOff2, off2);
    st.put(bIdx2, idx2, nPos2);
    st.put(bKp1, kp1);
    st.put(bKp2, kp2);
    st.put(bD1, desc1);
    st.put(bD2, desc2);
    st.put(bH1, hasMP1);
    st.put(bH2, hasMP2);
    st.put(bS1, stereo1);
    st.put(bS2, stereo2);
    st.put(bSf, sf2);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;

    TriArgs A{};
    A.nPos1 = nPos1;
    A.idx1 = st.dev(bIdx1);
    A.grp1 = st.dev(bGrp1);
    A.off2 = st.dev(bOff2);
    A.idx2 = st.dev(bIdx2);
    A.kp1 = st.dev(bKp1);
    A.kp2 = st.dev(bKp2);
    A.desc1 = st.dev(bD1);
    A.desc2 = st.dev(bD2);
    A.hasMP1 = st.dev(bH1);
    A.hasMP2 = st.dev(bH2);
    A.stereo1 = stereo1 ? st.dev(bS1) : nullptr;
    A.stereo2 = stereo2 ? st.dev(bS2) : nullptr;
    A.sf2 = st.dev(bSf);
    for (int i = 0; i < 9; i++) A.F12[i] = P->f12[i];
    A.epx = P->ep_x;
    A.epy = P->ep_y;
    A.onlyStereo = P->only_stereo;
    A.coarse = P->coarse;
    A.checkOrientation = P->check_orientation;
    A.model1 = P->camera_model1;
    A.model2 = P->camera_model2;
    A.kf1HasCamera2 = P->kf1_has_camera2;
    for (int i = 0; i < 8; i++) {
        A.cam1[i] = P->cam1[i];
        A.cam2[i] = P->cam2[i];
    }
    A.kbPrecision = P->kb_precision;
    for (int i = 0; i < 9; i++) A.R12[i] = P->r12[i];
    for (int i = 0; i < 3; i++) A.t12[i] = P->t12[i];
    for (int i = 0; i < kMaxLevels; i++) A.sigma2_1[i] = P->level_sigma2_1[i];
    if (P->camera_model1 == ORBFE_CAMERA_KANNALA_BRANDT8)
        for (int i = 0; i < n1; i++)
            if (kp1[i].octave < 0 || kp1[i].octave >= kMaxLevels) return ORBFE_ERR_INVALID_ARG;  // indexes mvLevelSigma2
    A.n1 = n1;
    A.match12 = st.dev(bMatch);
    A.binOf = st.dev(bBin);
    A.nMatches = st.dev(bNM);
    const dim3 blk(256);
    hipLaunchKernelGGL(fill_kernel, dim3((n1 + 255) / 256), blk, 0, s, A.match12, -1, (size_t)n1);
    hipLaunchKernelGGL(tri_match_kernel, dim3((nPos1 + 63) / 64), dim3(64), 0, s, A);
    hipLaunchKernelGGL(tri_finalize_kernel, dim3(1), blk, 0, s, A);
    MCHK(hipGetLastError());
    if ((rc = fetch_span(st, s, bMatch.off, bMatch.end(), err)) != ORBFE_OK) return rc;
    if ((rc = fetch_span(st, s, bNM.off, bNM.end(), err)) != ORBFE_OK) return rc;
    MCHK(hipStreamSynchronize(s));
    st.get(bMatch, matches12);
    *nMatches = *st.res(bNM);
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------
// resident key frames (keyframe.h)
// ---------------------------------------------------------------------------------------------
int keyframe_create(int n, const orbfe_keypoint* kp, const uint8_t* desc, const int* nodeId, const uint8_t* stereo,
                    const float* sf, int nLevels, hipStream_t s, KeyFrameDev** out, std::string& err)
{
    *out = nullptr;
    if (n < 0 || nLevels < 1 || nLevels > kMaxLevels || (n > 0 && (!kp || !desc || !nodeId)) || !sf) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (kp[i].octave < 0 || kp[i].octave >= nLevels) return ORBFE_ERR_INVALID_ARG;  // indexes mvScaleFactors / mvLevelSigma2
    // FeatureVector as sorted arrays: features with a node, by (node, feature index) -- DBoW2 appends the features of a
    // node in index order (TemplatedVocabulary.h:1157-1170), so this IS the order the reference walks them in
    std::vector<int> order;
    order.reserve((size_t)n);
    for (int i = 0; i < n; i++)
        if (nodeId[i] >= 0) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return nodeId[a] < nodeId[b]; });
    std::vector<int> nodeList, nodeOff;
    for (size_t p = 0; p < order.size(); p++)
        if (p == 0 || nodeId[order[p]] != nodeId[order[p - 1]]) {
            nodeList.push_back(nodeId[order[p]]);
            nodeOff.push_back((int)p);
        }
    nodeOff.push_back((int)order.size());
    Carver c;
    const size_t oKp = c.take((size_t)std::max(n, 1) * sizeof(orbfe_keypoint));
    const size_t oDesc = c.take((size_t)std::max(n, 1) * 32);
    const size_t oNode = c.take((size_t)std::max(n, 1) * sizeof(int));
    const size_t oStereo = c.take((size_t)std::max(n, 1));
    const size_t oSf = c.take((size_t)kMaxLevels * sizeof(float));
    const size_t oOrder = c.take((order.size() + 1) * sizeof(int));
    const size_t oList = c.take((nodeList.size() + 1) * sizeof(int));
    const size_t oOff = c.take(nodeOff.size() * sizeof(int));
    std::vector<uint8_t> img(c.off, 0);
    if (n) {
        memcpy(&img[oKp], kp, (size_t)n * sizeof(orbfe_keypoint));
        memcpy(&img[oDesc], desc, (size_t)n * 32);
        memcpy(&img[oNode], nodeId, (size_t)n * sizeof(int));
        if (stereo) memcpy(&img[oStereo], stereo, (size_t)n);
    }
    memcpy(&img[oSf], sf, (size_t)nLevels * sizeof(float));
    if (!order.empty()) memcpy(&img[oOrder], order.data(), order.size() * sizeof(int));
    if (!nodeList.empty()) memcpy(&img[oList], nodeList.data(), nodeList.size() * sizeof(int));
    memcpy(&img[oOff], nodeOff.data(), nodeOff.size() * sizeof(int));
    KeyFrameDev* K = new (std::nothrow) KeyFrameDev();
    if (!K) return ORBFE_ERR_OUT_OF_MEMORY;
    if (hipMalloc(&K->block, c.off) != hipSuccess) {
        (void)hipGetLastError();
        delete K;
        err = "hipMalloc(key frame) failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    if (copy_sync(K->block, img.data(), c.off, hipMemcpyHostToDevice, s) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(K->block);
        delete K;
        err = "upload of the key frame failed";
        return ORBFE_ERR_HIP;
    }
    uint8_t* b = static_cast<uint8_t*>(K->block);
    K->n = n;
    K->nLevels = nLevels;
    K->G = (int)nodeList.size();
    K->hasStereo = stereo != nullptr;
    K->kp = reinterpret_cast<const orbfe_keypoint*>(b + oKp);
    K->desc = b + oDesc;
    K->node = reinterpret_cast<const int*>(b + oNode);
    K->stereo = stereo ? b + oStereo : nullptr;
    K->sf = reinterpret_cast<const float*>(b + oSf);
    K->order = reinterpret_cast<const int*>(b + oOrder);
    K->nodeList = reinterpret_cast<const int*>(b + oList);
    K->nodeOff = reinterpret_cast<const int*>(b + oOff);
    K->bytes = c.off;
    *out = K;
    return ORBFE_OK;
}

void keyframe_destroy(KeyFrameDev* K)
{
    if (!K) return;
    if (K->block) (void)hipFree(K->block);
    match_scratch_free(K->gridMem);  // the cell tables of keyframe_set_grid, if any
    delete K;
}

int match_triangulation_batch_run(MatchScratch& m, hipStream_t s, const KeyFrameDev* kf1, const uint8_t* hasMP1, int K,
                                  const KeyFrameDev* const* kf2, const uint8_t* const* hasMP2, const orbfe_tri_params* P,
                                  int* rawMatch, uint8_t* rawBin, std::string& err, const orbfe_newpoint_params* NP, float* x3d,
                                  uint8_t* verdict)
{
    const int n1 = kf1->n;
    if (!NP && (K == 0 || n1 == 0)) return ORBFE_OK;
    for (int k = 0; k < K; k++) {
        if (!kf2[k] || (!hasMP2[k] && kf2[k]->n > 0)) return ORBFE_ERR_INVALID_ARG;
        if (P[k].struct_size != (int)sizeof(orbfe_tri_params)) {
            err = "orbfe_tri_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
            return ORBFE_ERR_INVALID_ARG;
        }
        if (NP && NP[k].struct_size != (int)sizeof(orbfe_newpoint_params)) {
            err = kNewPtSizeErr;
            return ORBFE_ERR_INVALID_ARG;
        }
        if (NP && (kf1->hasStereo || kf2[k]->hasStereo)) {
            err = "orbfe_create_new_points_batch: monocular key frames only (the stereo branches of CreateNewMapPoints are not built)";
            return ORBFE_ERR_UNSUPPORTED;
        }
    }
    if (K == 0 || n1 == 0) return ORBFE_OK;
    // one pinned block up: [argument blocks | has_mp1 | has_mp2 of every neighbour]; one block down: [raw match | raw bin]
    Carver in;
    const size_t oArgs = in.take((size_t)K * sizeof(TriNeighbour));
    const size_t oH1 = in.take((size_t)n1);
    std::vector<size_t> oH2((size_t)K);
    for (int k = 0; k < K; k++) oH2[(size_t)k] = in.take((size_t)std::max(kf2[k]->n, 1));
    const size_t oGeo = NP ? in.take((size_t)K * sizeof(NewPtNeighbour)) : 0;
    const size_t inBytes = in.off;
    Carver sc = in;
    const size_t oMatch = sc.take((size_t)K * n1 * sizeof(int));
    const size_t oBin = sc.take((size_t)K * n1);
    const size_t oVerdict = NP ? sc.take((size_t)K * n1) : 0;
    const size_t oX3d = NP ? sc.take((size_t)K * n1 * 3 * sizeof(float)) : 0;
    const size_t outBytes = sc.off - oMatch;
    int rc = ensure(m, sc.off, inBytes + outBytes + 256, err);
    if (rc != ORBFE_OK) return rc;
    uint8_t* hp = static_cast<uint8_t*>(m.hpin);
    uint8_t* dp = static_cast<uint8_t*>(m.d);
    TriNeighbour* args = reinterpret_cast<TriNeighbour*>(hp + oArgs);
    memcpy(hp + oH1, hasMP1, (size_t)n1);
    for (int k = 0; k < K; k++) {
        const KeyFrameDev* F = kf2[k];
        if (F->n) memcpy(hp + oH2[(size_t)k], hasMP2[k], (size_t)F->n);
        TriNeighbour& A = args[k];
        A.kp2 = F->kp; A.desc2 = F->desc; A.stereo2 = F->stereo; A.sf2 = F->sf;
        A.nodeList2 = F->nodeList; A.nodeOff2 = F->nodeOff; A.order2 = F->order;
        A.hasMP2 = dp + oH2[(size_t)k];
        A.G2 = F->G; A.n2 = F->n;
        const orbfe_tri_params& Q = P[k];
        for (int i = 0; i < 9; i++) A.F12[i] = Q.f12[i];
        A.epx = Q.ep_x; A.epy = Q.ep_y;
        A.onlyStereo = Q.only_stereo; A.coarse = Q.coarse; A.checkOrientation = Q.check_orientation;
        A.model1 = Q.camera_model1; A.model2 = Q.camera_model2; A.kf1HasCamera2 = Q.kf1_has_camera2;
        for (int i = 0; i < 8; i++) { A.cam1[i] = Q.cam1[i]; A.cam2[i] = Q.cam2[i]; }
        A.kbPrecision = Q.kb_precision;
        for (int i = 0; i < 9; i++) A.R12[i] = Q.r12[i];
        for (int i = 0; i < 3; i++) A.t12[i] = Q.t12[i];
        for (int i = 0; i < kMaxLevels; i++) A.sigma2_1[i] = Q.level_sigma2_1[i];
        if (NP) fill_newpt(reinterpret_cast<NewPtNeighbour*>(hp + oGeo)[k], F, NP[k]);
    }
    MCHK(hipMemcpyAsync(dp, hp, inBytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(tri_batch_kernel, dim3((n1 + 255) / 256, K), dim3(256), 0, s, reinterpret_cast<const TriNeighbour*>(dp + oArgs), n1,
                       kf1->kp, kf1->desc, kf1->node, kf1->stereo, dp + oH1, reinterpret_cast<int*>(dp + oMatch), dp + oBin);
    if (NP)  // every raw partner's geometry, behind the search on the same stream: one submission, one download
        hipLaunchKernelGGL(newpoints_kernel, dim3((n1 + 63) / 64, K), dim3(64), 0, s, reinterpret_cast<const NewPtNeighbour*>(dp + oGeo), n1,
                           kf1->kp, kf1->sf, static_cast<const int*>(nullptr), reinterpret_cast<const int*>(dp + oMatch),
                           reinterpret_cast<float*>(dp + oX3d), dp + oVerdict);
    MCHK(hipGetLastError());
    uint8_t* hOut = hp + inBytes;
    MCHK(hipMemcpyAsync(hOut, dp + oMatch, outBytes, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    memcpy(rawMatch, hOut, (size_t)K * n1 * sizeof(int));
    memcpy(rawBin, hOut + (oBin - oMatch), (size_t)K * n1);
    if (NP) {
        memcpy(verdict, hOut + (oVerdict - oMatch), (size_t)K * n1);
        memcpy(x3d, hOut + (oX3d - oMatch), (size_t)K * n1 * 3 * sizeof(float));
    }
    return ORBFE_OK;
}

int triangulate_pairs_run(MatchScratch& m, hipStream_t s, const KeyFrameDev* kf1, const KeyFrameDev* kf2,
                          const orbfe_newpoint_params* NP, int nPairs, const int* idx1, const int* idx2, float* x3d, uint8_t* verdict,
                          std::string& err)
{
    if (NP->struct_size != (int)sizeof(orbfe_newpoint_params)) {
        err = kNewPtSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    if (kf1->hasStereo || kf2->hasStereo) {
        err = "orbfe_triangulate_pairs: monocular key frames only (the stereo branches of CreateNewMapPoints are not built)";
        return ORBFE_ERR_UNSUPPORTED;
    }
    for (int p = 0; p < nPairs; p++)
        if (idx1[p] < 0 || idx1[p] >= kf1->n || idx2[p] < 0 || idx2[p] >= kf2->n) return ORBFE_ERR_INVALID_ARG;
    if (nPairs == 0) return ORBFE_OK;
    Staging st;
    const auto bGeo = st.in<NewPtNeighbour>(1);
    const auto bI1 = st.in<int>(nPairs);
    const auto bI2 = st.in<int>(nPairs);
    const auto bVerdict = st.out<uint8_t>(nPairs);
    const auto bX3d = st.out<float>((size_t)nPairs * 3);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    fill_newpt(*st.host(bGeo), kf2, *NP);
    st.put(bI1, idx1);
    st.put(bI2, idx2);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    hipLaunchKernelGGL(newpoints_kernel, dim3((nPairs + 63) / 64, 1), dim3(64), 0, s, st.dev(bGeo), nPairs, kf1->kp, kf1->sf, st.dev(bI1),
                       st.dev(bI2), st.dev(bX3d), st.dev(bVerdict));
    if ((rc = download(st, s, err)) != ORBFE_OK) return rc;
    st.get(bVerdict, verdict);
    st.get(bX3d, x3d);
    return ORBFE_OK;
}

}  // namespace orbfe

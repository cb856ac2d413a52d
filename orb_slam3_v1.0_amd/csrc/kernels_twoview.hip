// kernels_twoview.hip -- TwoViewReconstruction::Reconstruct on gfx950 (src/TwoViewReconstruction.cc:40-127; the call:
// src/Tracking.cc:616 -> Pinhole::ReconstructWithTwoViews, src/CameraModels/Pinhole.cpp:81-88).
//
// SPEC DECISION S12: binary32 where the C++ is float, one operation per line, left to right, no
// contraction, the C++'s own promotions kept; the null vectors of the 16 x 9 / 8 x 9 systems by a fixed Jacobi sequence on
// A^T A in binary64 (10 sweeps of 9 rounds of 4 disjoint pairs); the 3 x 3 decompositions by the n = 3 sequence of jacobi.h.
// tests/twoview_ref.py is the normative restatement; every byte this file produces is compared with it.
//
//   twoview_hypothesis_kernel  2 x iterations blocks of one wave: ComputeH21 / ComputeF21 (:230-306), the denormalisation
//                              (:164-166, :215-217) and CheckHomography / CheckFundamental over all matches (:308-471)
//   twoview_select_kernel      one wave: "first iteration with the strictly largest score" (:170-175, :221-226) for both models
//   twoview_check_rt_kernel    one block per motion hypothesis: CheckRT (:799-914)
// The decompositions between the two submissions (ReconstructH :594-702, DecomposeE :916-940) and the selection rules
// (:503-580, :705-746) run on the host (two_view_run).  The per-match terms and that host step are in twoview_math.h, host-safe text
// that tests/cpp/two_view.cpp includes; this file holds what the teams of threads do and the host call.
#include <algorithm>
#include <cstring>
#include <vector>

#include "match_common.h"
#include "jacobi.h"
#include "twoview_math.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

struct TwoViewArgs {
    int N, iterations, words;        // words = ceil(N / 64) ballot words per hypothesis
    const float* pts;                // [N][4] u1 v1 u2 v2 of every match (mvKeys1 / mvKeys2 through mvMatches12)
    const float* npts;               // [N][4] the same through Normalize (vPn1 / vPn2)
    const int* sets;                 // [iterations][8] mvSets
    float T1[9], T2inv[9], T2t[9];
    float invSigmaSquare;            // (float)(1.0 / (sigma * sigma)), :338,:414
    float* scores;                   // [2 * iterations] H iterations, then F iterations
    float* mats;                     // [2 * iterations][9] H21i / F21i
    unsigned long long* masks;       // [2 * iterations][words] vbCurrentInliers, bit m % 64 of word m / 64
};

// One wave per RANSAC hypothesis; all 2 x iterations waves are resident at once, so the call's latency is one hypothesis's.
// M = A^T A and V live in LDS (run-time indices there cost nothing; in registers they would go to scratch).  A Jacobi round is
// four angle chains (binary64 divide / square root) in four lanes, then three phases of 36 independent element pairs each.
__global__ __launch_bounds__(64) void twoview_hypothesis_kernel(TwoViewArgs G)
{
    __shared__ float sA[16][9];
    __shared__ double sM[9][9], sV[9][9];
    __shared__ double sC[4], sS[4];
    __shared__ int sSkip[4];
    __shared__ int sP[9][4], sQ[9][4];
    __shared__ float sTerm[128];
    const int lane = threadIdx.x;
    const bool isF = (int)blockIdx.x >= G.iterations;
    const int it = isF ? (int)blockIdx.x - G.iterations : (int)blockIdx.x;
    const int rows = isF ? 8 : 16;

    // round r holds the pairs {i, j}, i < j, i + j == r (mod 9), in ascending i
    if (lane < 36) {
        const int r = lane / 4, slot = lane % 4;
        int cnt = 0;
        for (int i = 0; i < 9; i++) {
            const int j = (r - i + 9) % 9;
            if (i < j) {
                if (cnt == slot) { sP[r][slot] = i; sQ[r][slot] = j; }
                cnt++;
            }
        }
    }
    if (lane < 8) {
        const int idx = G.sets[it * 8 + lane];
        const float u1 = G.npts[4 * idx], v1 = G.npts[4 * idx + 1], u2 = G.npts[4 * idx + 2], v2 = G.npts[4 * idx + 3];
        if (!isF) {  // :243-261
            float* r0 = sA[2 * lane];
            float* r1 = sA[2 * lane + 1];
            r0[0] = 0.0f; r0[1] = 0.0f; r0[2] = 0.0f; r0[3] = -u1; r0[4] = -v1; r0[5] = -1.0f;
            r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
            r1[0] = u1; r1[1] = v1; r1[2] = 1.0f; r1[3] = 0.0f; r1[4] = 0.0f; r1[5] = 0.0f;
            r1[6] = -u2 * u1; r1[7] = -u2 * v1; r1[8] = -u2;
        } else {  // :285-293
            float* r0 = sA[lane];
            r0[0] = u2 * u1; r0[1] = u2 * v1; r0[2] = u2; r0[3] = v2 * u1; r0[4] = v2 * v1; r0[5] = v2;
            r0[6] = u1; r0[7] = v1; r0[8] = 1.0f;
        }
    }
    __syncthreads();
    for (int e = lane; e < 81; e += 64) {
        const int i = e / 9, j = e % 9;
        double acc = 0.0;
        for (int k = 0; k < rows; k++) acc = acc + (double)sA[k][i] * (double)sA[k][j];
        sM[i][j] = acc;
        sV[i][j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();

    const int pr = lane / 9, kk = lane % 9;  // phase work item: pair slot pr (lanes 0..35), element kk
    for (int sweep = 0; sweep < kTwoViewSweeps; sweep++) {
        for (int r = 0; r < 9; r++) {
            if (lane < 4) {  // the four angles, from M as it stands at the start of the round
                const int p = sP[r][lane], q = sQ[r][lane];
                const double apq = sM[p][q];
                const int skip = apq == 0.0;
                double c = 1.0, sn = 0.0;
                if (!skip) jacobi_angle(sM[p][p], sM[q][q], apq, c, sn);
                sC[lane] = c; sS[lane] = sn; sSkip[lane] = skip;
            }
            __syncthreads();
            const bool work = lane < 36 && !sSkip[pr < 4 ? pr : 0];
            const int p = work ? sP[r][pr] : 0, q = work ? sQ[r][pr] : 0;
            const double c = work ? sC[pr] : 1.0, sn = work ? sS[pr] : 0.0;
            if (work) {  // columns p, q of M
                const double a = sM[kk][p], b = sM[kk][q];
                sM[kk][p] = c * a - sn * b;
                sM[kk][q] = sn * a + c * b;
            }
            __syncthreads();
            if (work) {  // rows p, q of M; columns p, q of V
                const double a = sM[p][kk], b = sM[q][kk];
                sM[p][kk] = c * a - sn * b;
                sM[q][kk] = sn * a + c * b;
                const double va = sV[kk][p], vb = sV[kk][q];
                sV[kk][p] = c * va - sn * vb;
                sV[kk][q] = sn * va + c * vb;
            }
            __syncthreads();
        }
    }

    // column of V at the smallest diagonal entry, lowest index on ties; every lane keeps its own copy from here on
    int bi = 0;
    double best = sM[0][0];
    for (int i = 1; i < 9; i++) {
        const double d = sM[i][i];
        if (d < best) { best = d; bi = i; }
    }
    float Xn[9];
#pragma unroll
    for (int k = 0; k < 9; k++) Xn[k] = (float)sV[k][bi];

    float X21[9], X12[9], tmp[9];
    if (!isF) {  // H21i = T2inv * Hn * T1; H12i = H21i.inverse() (:164-166)
        mul3(G.T2inv, Xn, tmp);
        mul3(tmp, G.T1, X21);
        inv3(X21, X12);
    } else {  // Fn = rank 2 (:300-305); F21i = T2t * Fn * T1 (:215-217)
        float Fn[9];
        rank2_f(Xn, Fn);
        mul3(G.T2t, Fn, tmp);
        mul3(tmp, G.T1, X21);
#pragma unroll
        for (int k = 0; k < 9; k++) X12[k] = 0.0f;
    }

    // score over ALL matches: 64 matches per step, their two terms through LDS, summed in match order (every lane runs the same
    // sequential sum, first-image term first; a rejected term is +0, which leaves a score that is never negative unchanged)
    float score = 0.0f;
    for (int base = 0; base < G.N; base += 64) {
        const int m = base + lane;
        float t1 = 0.0f, t2 = 0.0f;
        bool bIn = false;
        if (m < G.N) {
            const float4 pt = reinterpret_cast<const float4*>(G.pts)[m];
            if (!isF) homography_terms(X21, X12, G.invSigmaSquare, pt.x, pt.y, pt.z, pt.w, t1, t2, bIn);
            else fundamental_terms(X21, G.invSigmaSquare, pt.x, pt.y, pt.z, pt.w, t1, t2, bIn);
        }
        const unsigned long long word = __ballot(bIn);
        if (lane == 0) G.masks[(size_t)blockIdx.x * G.words + base / 64] = word;
        sTerm[2 * lane] = t1;
        sTerm[2 * lane + 1] = t2;
        __syncthreads();
        const int cnt = 2 * min(64, G.N - base);
        for (int k = 0; k < cnt; k++) score = score + sTerm[k];
        __syncthreads();
    }
    if (lane == 0) G.scores[blockIdx.x] = score;
#pragma unroll
    for (int k = 0; k < 9; k++)
        if (lane == k) G.mats[(size_t)blockIdx.x * 9 + k] = X21[k];
}

struct TwoViewSel {
    int N, iterations, words;
    const float* scores;
    const float* mats;
    const unsigned long long* masks;
    float* winMat;     // [2][9]
    float* winScore;   // [2]
    int* winIt;        // [2], -1 when no hypothesis scored above 0
    uint8_t* winMask;  // [2][N]
};

// "if (currentScore > score)" over the iterations in order, from score = 0: the first iteration with the strictly largest score
__global__ __launch_bounds__(64) void twoview_select_kernel(TwoViewSel S)
{
    const int lane = threadIdx.x;
    for (int model = 0; model < 2; model++) {
        float best = 0.0f;
        int bestIt = 0x7fffffff;
        for (int it = lane; it < S.iterations; it += 64) {
            const float sc = S.scores[model * S.iterations + it];
            if (sc > best) { best = sc; bestIt = it; }  // ascending within the lane: keeps the first of equals
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ob = __shfl_xor(best, d);
            const int oi = __shfl_xor(bestIt, d);
            if (ob > best || (ob == best && oi < bestIt)) { best = ob; bestIt = oi; }
        }
        const bool any = bestIt != 0x7fffffff;
        if (lane < 9) S.winMat[model * 9 + lane] = any ? S.mats[(size_t)(model * S.iterations + bestIt) * 9 + lane] : 0.0f;
        if (lane == 0) {
            S.winScore[model] = any ? best : 0.0f;
            S.winIt[model] = any ? bestIt : -1;
        }
        const unsigned long long* mk = S.masks + (size_t)(model * S.iterations + (any ? bestIt : 0)) * S.words;
        for (int m = lane; m < S.N; m += 64) S.winMask[(size_t)model * S.N + m] = any ? (uint8_t)((mk[m / 64] >> (m % 64)) & 1ull) : (uint8_t)0;
    }
}

struct RtHyp {
    float R[9], t[3];
    float P2[12];   // K [R | t], row-major 3 x 4 (:824-827)
    float O2[3];    // -R^T t (:829)
};

struct CheckRtArgs {
    int N;
    const float* pts;        // [N][4]
    const uint8_t* inlier;   // [N] vbMatchesInliers of the model in use
    float fx, fy, cx, cy, th2;
    RtHyp hyp[8];
    uint8_t* flags;          // [nHyp][N]
    float* cosv;             // [nHyp][N]
    float* x3d;              // [nHyp][N][3]
    int* nGood;              // [8]
    float* cosSel;           // [8]
};

// CheckRT's loop body (:838-900) for one inlier match: bit 0 = counted in nGood, bit 1 = vbGood
__device__ inline int check_rt_eval(const CheckRtArgs& A, const RtHyp& H, float u1, float v1, float u2, float v2, float& X, float& Y,
                                    float& Z, float& cosParallax)
{
    // GeometricTools::Triangulate (src/GeometricTools.cc:49-53) with P1 = K [I | 0]: rows as S11
    const float P1[12] = {A.fx, 0.0f, A.cx, 0.0f, 0.0f, A.fy, A.cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    float Am[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        Am[0][j] = u1 * P1[8 + j] - P1[j];
        Am[1][j] = v1 * P1[8 + j] - P1[4 + j];
        Am[2][j] = u2 * H.P2[8 + j] - H.P2[j];
        Am[3][j] = v2 * H.P2[8 + j] - H.P2[4 + j];
    }
    double M[4][4], vv[4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc = acc + (double)Am[k][i] * (double)Am[k][j];
            M[i][j] = acc;
        }
    sym4_min_eigenvector(M, vv);
    X = (float)(vv[0] / vv[3]);
    Y = (float)(vv[1] / vv[3]);
    Z = (float)(vv[2] / vv[3]);
    cosParallax = 0.0f;
    if (!isfinite(X) || !isfinite(Y) || !isfinite(Z)) return 0;  // :848-852
    const float dist1 = sqrtf((X * X + Y * Y) + Z * Z);  // normal1 = p3dC1 - O1, O1 = 0 (:855-856)
    const float n2x = X - H.O2[0], n2y = Y - H.O2[1], n2z = Z - H.O2[2];
    const float dist2 = sqrtf((n2x * n2x + n2y * n2y) + n2z * n2z);
    cosParallax = ((X * n2x + Y * n2y) + Z * n2z) / (dist1 * dist2);  // :861
    const bool lowParallax = !((double)cosParallax < 0.99998);
    if (Z <= 0.0f && !lowParallax) return 0;  // :864
    const float X2 = ((H.R[0] * X + H.R[1] * Y) + H.R[2] * Z) + H.t[0];  // :868
    const float Y2 = ((H.R[3] * X + H.R[4] * Y) + H.R[5] * Z) + H.t[1];
    const float Z2 = ((H.R[6] * X + H.R[7] * Y) + H.R[8] * Z) + H.t[2];
    if (Z2 <= 0.0f && !lowParallax) return 0;  // :870
    const float invZ1 = (float)(1.0 / (double)Z);  // :875
    const float im1x = (A.fx * X) * invZ1 + A.cx;
    const float im1y = (A.fy * Y) * invZ1 + A.cy;
    const float e1x = im1x - u1, e1y = im1y - v1;
    const float squareError1 = e1x * e1x + e1y * e1y;
    if (squareError1 > A.th2) return 0;  // :881
    const float invZ2 = (float)(1.0 / (double)Z2);  // :886
    const float im2x = (A.fx * X2) * invZ2 + A.cx;
    const float im2y = (A.fy * Y2) * invZ2 + A.cy;
    const float e2x = im2x - u2, e2y = im2y - v2;
    const float squareError2 = e2x * e2x + e2y * e2y;
    if (squareError2 > A.th2) return 0;  // :892
    return lowParallax ? 1 : 3;  // :895-900
}

// blockIdx.x = motion hypothesis; threads stride over the matches.  Then nGood and the cosine at rank min(50, nGood - 1) of the
// ascending survivors' cosines (:903-908) by a bitwise radix select over their ordered-integer images: exact, O(32 N).
constexpr int kRtThreads = 1024;  // one match per thread up to 1024 matches: the S11 chain (~40 us) is paid once, not per stride

__global__ __launch_bounds__(kRtThreads) void twoview_check_rt_kernel(CheckRtArgs A)
{
    __shared__ int sGood;
    __shared__ unsigned sCount;
    const int hyp = blockIdx.x, tid = threadIdx.x;
    const RtHyp& H = A.hyp[hyp];
    uint8_t* flags = A.flags + (size_t)hyp * A.N;
    float* cosv = A.cosv + (size_t)hyp * A.N;
    float* x3d = A.x3d + (size_t)hyp * A.N * 3;
    if (tid == 0) sGood = 0;
    __syncthreads();
    int local = 0;
    for (int m = tid; m < A.N; m += kRtThreads) {
        int f = 0;
        float X = 0.0f, Y = 0.0f, Z = 0.0f, cp = 0.0f;
        if (A.inlier[m]) {
            const float4 pt = reinterpret_cast<const float4*>(A.pts)[m];
            f = check_rt_eval(A, H, pt.x, pt.y, pt.z, pt.w, X, Y, Z, cp);
        }
        if (!(f & 1)) { X = 0.0f; Y = 0.0f; Z = 0.0f; cp = 0.0f; }
        flags[m] = (uint8_t)f;
        cosv[m] = cp;
        x3d[3 * m] = X; x3d[3 * m + 1] = Y; x3d[3 * m + 2] = Z;
        local += f & 1;
    }
    if (local) atomicAdd(&sGood, local);
    __syncthreads();
    const int nGood = sGood;
    if (nGood == 0) {
        if (tid == 0) { A.nGood[hyp] = 0; A.cosSel[hyp] = 1.0f; }  // parallax = 0 (:910-911)
        return;
    }
    int rank = min(50, nGood - 1);
    unsigned prefix = 0, known = 0;
    for (int bit = 31; bit >= 0; bit--) {
        if (tid == 0) sCount = 0;
        __syncthreads();
        unsigned c = 0;
        for (int m = tid; m < A.N; m += kRtThreads)
            if (flags[m] & 1) {
                const unsigned key = ordered_key(cosv[m]);
                if ((key & known) == prefix && !((key >> bit) & 1u)) c++;
            }
        if (c) atomicAdd(&sCount, c);
        __syncthreads();
        const int zeros = (int)sCount;
        if (rank >= zeros) { rank -= zeros; prefix |= 1u << bit; }
        known |= 1u << bit;
        __syncthreads();
    }
    if (tid == 0) { A.nGood[hyp] = nGood; A.cosSel[hyp] = ordered_key_inverse(prefix); }
}

constexpr char kTwoViewSizeErr[] =
    "orbfe_two_view_params / orbfe_two_view_info struct_size does not match this library (rebuild the caller against include/orbfe.h)";

}  // namespace

int two_view_run(MatchScratch& m, hipStream_t s, const orbfe_two_view_params* P, int n1, const orbfe_keypoint* kp1, int n2,
                 const orbfe_keypoint* kp2, const int* matches12, const int* sets, int* reconstructed, float* R21, float* t21,
                 float* p3d, uint8_t* triangulated, orbfe_two_view_info* info, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_two_view_params) || (info && info->struct_size != (int)sizeof(orbfe_two_view_info))) {
        err = kTwoViewSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    const int iterations = P->iterations;
    if (iterations < 1 || iterations > 4096 || P->min_parallax_deg != 1.0f) return ORBFE_ERR_INVALID_ARG;
    std::vector<int> first, second;  // mvMatches12 (:48-60)
    for (int i = 0; i < n1; i++)
        if (matches12[i] >= 0) {
            if (matches12[i] >= n2) return ORBFE_ERR_INVALID_ARG;
            first.push_back(i);
            second.push_back(matches12[i]);
        }
    const int N = (int)first.size();

    *reconstructed = 0;
    for (int i = 0; i < 9; i++) R21[i] = 0.0f;
    for (int i = 0; i < 3; i++) t21[i] = 0.0f;
    if (n1 > 0) {
        memset(p3d, 0, (size_t)n1 * 3 * sizeof(float));
        memset(triangulated, 0, (size_t)n1);
    }
    orbfe_two_view_info local;
    memset(&local, 0, sizeof local);
    if (info) {  // keep the caller's buffers, clear the rest
        local.scores = info->scores; local.inliers_H = info->inliers_H; local.inliers_F = info->inliers_F;
        local.rt_flags = info->rt_flags; local.rt_x3d = info->rt_x3d; local.rt_cos = info->rt_cos;
    }
    orbfe_two_view_info& I = local;
    I.struct_size = (int)sizeof(orbfe_two_view_info);
    I.n_matches = N;
    I.best_it_H = -1;
    I.best_it_F = -1;
    I.best_hypothesis = -1;
    for (int i = 0; i < 8; i++) I.cos_parallax[i] = 1.0f;
    struct Publish {  // the info block goes out on every path
        orbfe_two_view_info* dst;
        orbfe_two_view_info* src;
        ~Publish() { if (dst) *dst = *src; }
    } publish{info, &local};
    if (N < 8) {
        I.exit_line = 62;
        return ORBFE_OK;
    }
    if (!sets) return ORBFE_ERR_INVALID_ARG;
    for (int it = 0; it < iterations; it++)
        for (int j = 0; j < 8; j++) {
            const int v = sets[it * 8 + j];
            if (v < 0 || v >= N) return ORBFE_ERR_INVALID_ARG;
            for (int k = 0; k < j; k++)
                if (sets[it * 8 + k] == v) return ORBFE_ERR_INVALID_ARG;
        }

    std::vector<float> nx1, ny1, nx2, ny2;
    float T1[9], T2[9], T2inv[9], T2t[9];
    normalize_points(n1, kp1, nx1, ny1, T1);
    normalize_points(n2, kp2, nx2, ny2, T2);
    inv3(T2, T2inv);
    transpose3(T2, T2t);
    const float K[9] = {P->fx, 0.0f, P->cx, 0.0f, P->fy, P->cy, 0.0f, 0.0f, 1.0f};
    const float sigma2 = P->sigma * P->sigma;

    const int words = (N + 63) / 64;
    const int nHyp2 = 2 * iterations;
    // up: [pts | npts | sets]; device only: [mats | masks]; result block 1: [scores | winMat | winScore | winIt | winMask];
    // result block 2: [nGood | cosSel | flags | cos | x3d]
    Carver c;
    const size_t oPts = c.take((size_t)N * 4 * sizeof(float));
    const size_t oNpts = c.take((size_t)N * 4 * sizeof(float));
    const size_t oSets = c.take((size_t)iterations * 8 * sizeof(int));
    const size_t inBytes = c.off;
    const size_t oMats = c.take((size_t)nHyp2 * 9 * sizeof(float));
    const size_t oMasks = c.take((size_t)nHyp2 * words * sizeof(unsigned long long));
    const size_t oScores = c.take((size_t)nHyp2 * sizeof(float));
    const size_t oWinMat = c.take(18 * sizeof(float));
    const size_t oWinScore = c.take(2 * sizeof(float));
    const size_t oWinIt = c.take(2 * sizeof(int));
    const size_t oWinMask = c.take((size_t)2 * N);
    const size_t res1Bytes = c.off - oScores;
    const size_t oGood = c.take(8 * sizeof(int));
    const size_t oCosSel = c.take(8 * sizeof(float));
    const size_t oFlags = c.take((size_t)8 * N);
    const size_t oCos = c.take((size_t)8 * N * sizeof(float));
    const size_t oX3d = c.take((size_t)8 * N * 3 * sizeof(float));
    const size_t res2Bytes = c.off - oGood;
    const size_t hRes1 = inBytes, hRes2 = inBytes + res1Bytes;
    int rc = ensure(m, c.off, inBytes + res1Bytes + res2Bytes + 256, err);
    if (rc != ORBFE_OK) return rc;
    uint8_t* hp = static_cast<uint8_t*>(m.hpin);
    uint8_t* dp = static_cast<uint8_t*>(m.d);
    float* hPts = reinterpret_cast<float*>(hp + oPts);
    float* hNpts = reinterpret_cast<float*>(hp + oNpts);
    for (int i = 0; i < N; i++) {
        const int a = first[(size_t)i], b = second[(size_t)i];
        hPts[4 * i] = kp1[a].x; hPts[4 * i + 1] = kp1[a].y; hPts[4 * i + 2] = kp2[b].x; hPts[4 * i + 3] = kp2[b].y;
        hNpts[4 * i] = nx1[(size_t)a]; hNpts[4 * i + 1] = ny1[(size_t)a]; hNpts[4 * i + 2] = nx2[(size_t)b]; hNpts[4 * i + 3] = ny2[(size_t)b];
    }
    memcpy(hp + oSets, sets, (size_t)iterations * 8 * sizeof(int));

    // ---- submission 1: all hypotheses, the two winners ----
    MCHK(hipMemcpyAsync(dp, hp, inBytes, hipMemcpyHostToDevice, s));
    TwoViewArgs G;
    G.N = N; G.iterations = iterations; G.words = words;
    G.pts = reinterpret_cast<const float*>(dp + oPts);
    G.npts = reinterpret_cast<const float*>(dp + oNpts);
    G.sets = reinterpret_cast<const int*>(dp + oSets);
    for (int i = 0; i < 9; i++) { G.T1[i] = T1[i]; G.T2inv[i] = T2inv[i]; G.T2t[i] = T2t[i]; }
    G.invSigmaSquare = (float)(1.0 / (double)sigma2);
    G.scores = reinterpret_cast<float*>(dp + oScores);
    G.mats = reinterpret_cast<float*>(dp + oMats);
    G.masks = reinterpret_cast<unsigned long long*>(dp + oMasks);
    hipLaunchKernelGGL(twoview_hypothesis_kernel, dim3(nHyp2), dim3(64), 0, s, G);
    TwoViewSel S;
    S.N = N; S.iterations = iterations; S.words = words;
    S.scores = G.scores; S.mats = G.mats; S.masks = G.masks;
    S.winMat = reinterpret_cast<float*>(dp + oWinMat);
    S.winScore = reinterpret_cast<float*>(dp + oWinScore);
    S.winIt = reinterpret_cast<int*>(dp + oWinIt);
    S.winMask = dp + oWinMask;
    hipLaunchKernelGGL(twoview_select_kernel, dim3(1), dim3(64), 0, s, S);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(hp + hRes1, dp + oScores, res1Bytes, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const uint8_t* r1 = hp + hRes1;
    const float* winMat = reinterpret_cast<const float*>(r1 + (oWinMat - oScores));
    const float* winScore = reinterpret_cast<const float*>(r1 + (oWinScore - oScores));
    const int* winIt = reinterpret_cast<const int*>(r1 + (oWinIt - oScores));
    const uint8_t* winMask = r1 + (oWinMask - oScores);
    if (I.scores) memcpy(I.scores, r1, (size_t)nHyp2 * sizeof(float));
    if (I.inliers_H) memcpy(I.inliers_H, winMask, (size_t)N);
    if (I.inliers_F) memcpy(I.inliers_F, winMask + N, (size_t)N);
    float H21[9], F21[9];
    for (int i = 0; i < 9; i++) { H21[i] = winMat[i]; F21[i] = winMat[9 + i]; I.H21[i] = H21[i]; I.F21[i] = F21[i]; }
    const float SH = winScore[0], SF = winScore[1];
    I.SH = SH; I.SF = SF;
    I.best_it_H = winIt[0]; I.best_it_F = winIt[1];

    // ---- host step (:110-126) ----
    if (SH + SF == 0.0f) {
        I.exit_line = 110;
        return ORBFE_OK;
    }
    const float RH = SH / (SH + SF);
    I.RH = RH;
    const bool useH = (double)RH > 0.40;
    I.model = useH ? ORBFE_TWO_VIEW_MODEL_HOMOGRAPHY : ORBFE_TWO_VIEW_MODEL_FUNDAMENTAL;
    const uint8_t* inl = useH ? winMask : winMask + N;
    int nInliers = 0;
    for (int i = 0; i < N; i++) nInliers += inl[i] != 0;
    const int nHyp = useH ? motion_hypotheses_h(H21, K, I.hyp_R, I.hyp_t) : motion_hypotheses_f(F21, K, I.hyp_R, I.hyp_t);
    I.n_hypotheses = nHyp;
    if (nHyp == 0) {
        I.exit_line = 609;
        return ORBFE_OK;
    }

    // ---- submission 2: CheckRT for every motion hypothesis ----
    CheckRtArgs A;
    A.N = N;
    A.pts = G.pts;
    A.inlier = dp + oWinMask + (useH ? 0 : N);
    A.fx = P->fx; A.fy = P->fy; A.cx = P->cx; A.cy = P->cy;
    A.th2 = (float)(4.0 * (double)sigma2);
    for (int h = 0; h < nHyp; h++) {
        RtHyp& Hh = A.hyp[h];
        for (int i = 0; i < 9; i++) Hh.R[i] = I.hyp_R[h][i];
        for (int i = 0; i < 3; i++) Hh.t[i] = I.hyp_t[h][i];
        for (int i = 0; i < 3; i++)  // P2 = K * [R | t]
            for (int j = 0; j < 4; j++) {
                const float x0 = j < 3 ? Hh.R[j] : Hh.t[0], x1 = j < 3 ? Hh.R[3 + j] : Hh.t[1], x2 = j < 3 ? Hh.R[6 + j] : Hh.t[2];
                Hh.P2[4 * i + j] = (K[3 * i] * x0 + K[3 * i + 1] * x1) + K[3 * i + 2] * x2;
            }
        for (int i = 0; i < 3; i++) Hh.O2[i] = ((-Hh.R[i]) * Hh.t[0] + (-Hh.R[3 + i]) * Hh.t[1]) + (-Hh.R[6 + i]) * Hh.t[2];
    }
    for (int h = nHyp; h < 8; h++) memset(&A.hyp[h], 0, sizeof(RtHyp));
    A.flags = dp + oFlags;
    A.cosv = reinterpret_cast<float*>(dp + oCos);
    A.x3d = reinterpret_cast<float*>(dp + oX3d);
    A.nGood = reinterpret_cast<int*>(dp + oGood);
    A.cosSel = reinterpret_cast<float*>(dp + oCosSel);
    hipLaunchKernelGGL(twoview_check_rt_kernel, dim3(nHyp), dim3(kRtThreads), 0, s, A);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(hp + hRes2, dp + oGood, res2Bytes, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const uint8_t* r2 = hp + hRes2;
    const int* nGood = reinterpret_cast<const int*>(r2);
    const float* cosSel = reinterpret_cast<const float*>(r2 + (oCosSel - oGood));
    const uint8_t* flags = r2 + (oFlags - oGood);
    const float* cosv = reinterpret_cast<const float*>(r2 + (oCos - oGood));
    const float* x3d = reinterpret_cast<const float*>(r2 + (oX3d - oGood));
    for (int h = 0; h < nHyp; h++) { I.n_good[h] = nGood[h]; I.cos_parallax[h] = cosSel[h]; }
    if (I.rt_flags) { memset(I.rt_flags, 0, (size_t)8 * N); memcpy(I.rt_flags, flags, (size_t)nHyp * N); }
    if (I.rt_cos) { memset(I.rt_cos, 0, (size_t)8 * N * sizeof(float)); memcpy(I.rt_cos, cosv, (size_t)nHyp * N * sizeof(float)); }
    if (I.rt_x3d) { memset(I.rt_x3d, 0, (size_t)8 * N * 3 * sizeof(float)); memcpy(I.rt_x3d, x3d, (size_t)nHyp * N * 3 * sizeof(float)); }

    // ---- the selection rules ----
    int bestHyp = -1;
    if (!useH) {  // :503-580
        const int maxGood = std::max(nGood[0], std::max(nGood[1], std::max(nGood[2], nGood[3])));
        const int nMinGood = std::max((int)(0.9 * nInliers), P->min_triangulated);
        int nsimilar = 0;
        for (int h = 0; h < 4; h++)
            if (nGood[h] > 0.7 * maxGood) nsimilar++;
        if (maxGood < nMinGood || nsimilar > 1) {
            I.exit_line = 528;
            return ORBFE_OK;
        }
        int pick = 3;
        if (maxGood == nGood[0]) pick = 0;
        else if (maxGood == nGood[1]) pick = 1;
        else if (maxGood == nGood[2]) pick = 2;
        if (nGood[pick] > 0 && (double)cosSel[pick] < kCosOneDegree) bestHyp = pick;  // parallax > minParallax
        if (bestHyp < 0) {
            I.exit_line = 580;
            return ORBFE_OK;
        }
    } else {  // :705-746
        int bestGood = 0, secondBestGood = 0, bestIdx = -1;
        for (int h = 0; h < 8; h++) {
            if (nGood[h] > bestGood) {
                secondBestGood = bestGood;
                bestGood = nGood[h];
                bestIdx = h;
            } else if (nGood[h] > secondBestGood) {
                secondBestGood = nGood[h];
            }
        }
        const bool parallaxOk = bestIdx >= 0 && (double)cosSel[bestIdx] <= kCosOneDegree;  // bestParallax >= minParallax
        if (secondBestGood < 0.75 * bestGood && parallaxOk && bestGood > P->min_triangulated && bestGood > 0.9 * nInliers) bestHyp = bestIdx;
        if (bestHyp < 0) {
            I.exit_line = 746;
            return ORBFE_OK;
        }
    }
    I.best_hypothesis = bestHyp;
    *reconstructed = 1;
    for (int i = 0; i < 9; i++) R21[i] = I.hyp_R[bestHyp][i];
    for (int i = 0; i < 3; i++) t21[i] = I.hyp_t[bestHyp][i];
    for (int mIdx = 0; mIdx < N; mIdx++) {
        const int f = flags[(size_t)bestHyp * N + mIdx];
        const int i1 = first[(size_t)mIdx];
        if (f & 1)
            for (int k = 0; k < 3; k++) p3d[3 * i1 + k] = x3d[((size_t)bestHyp * N + mIdx) * 3 + k];
        triangulated[i1] = (uint8_t)((f >> 1) & 1);
    }
    return ORBFE_OK;
}

}  // namespace orbfe

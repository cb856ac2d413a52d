// kernels_poseopt.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:765-1067; the calls: src/Tracking.cc:869,935) on gfx950 for the
// branch this fork takes: one camera, mvuRight < 0, EdgeSE3ProjectXYZOnlyPose (src/OptimizableTypes.cpp:49-63), pinhole
// (src/CameraModels/Pinhole.cpp:33-39,69-79).
//
// SPEC DECISION S14: binary64 where the C++ is double, one operation per operator, no contraction; every sum
// over edges is a fixed pairwise tree over P = the smallest power of two >= N_e (+0.0 for the padding and for inactive edges); the
// Levenberg loop and SE3Quat::exp are restated from g2o's published algorithm; the 6 x 6 solve is S13's ldlt_solve6, sin / cos are
// spec_math.h's sequences.  tests/poseopt_ref.py is the normative restatement; every byte this file produces is compared with it.
// What one thread computes for one edge (poseopt_math.h) is host-safe text that tests/cpp/poseopt.cpp includes; this file holds the
// loop around the tree and the host calls; the tree itself (block_tree.h) is shared with the kernels of S17 and S19.
//
// pose_opt_kernel: ONE block per frame runs the whole call -- the compaction of the matched keypoints into edges, four rounds, every
// iteration and every trial -- with no host step and no second launch.
//   Mapping of the tree: the block has T threads (64 when P <= 64 in the host call, else 256); thread t owns the aligned run of
//   r = max(1, P / T) edges [t r, (t + 1) r).  Levels 0 .. log2 r - 1 of the tree are summed inside the thread (r <= 4: the edge data
//   stays in registers and the run is unrolled; above that the run is walked with a binary-counter stack and the edge data is read
//   back from L2), the next up to 6 levels inside the wave (DPP quad swaps, row_half_mirror, row_mirror, then two lane-xor
//   exchanges, so every lane ends with the wave's sum), the last levels across the waves through a double-buffered LDS block that
//   every thread reads.  Levels above log2 P are not taken: adding a padding +0.0 would turn a -0.0 sum into +0.0.
//   Every thread then holds H, b and the cost and runs the 6 x 6 solve, exp and the accept / reject rule redundantly: no result is
//   passed between threads except through the sums, so one barrier per sum is the only synchronisation (none for a 64-thread block).
// Every loop has a static trip bound (rounds <= 4, iterations <= 64, 10 trials, the fixed steps of ldlt_solve6); NaN follows the
// comparisons as written and can neither be accepted nor make a loop spin.
#include <cfloat>
#include <cstring>
#include <vector>

#include "match_common.h"
#include "block_tree.h"
#include "ldlt.h"
#include "poseopt_math.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

constexpr int kPoseOptThreads = kTreeThreads;
constexpr int kPoseOptMaxWaves = kTreeMaxWaves;
constexpr int kPoseOptTrials = 10;

struct PoseOptRounds {   // what the kernel reports per call (host call only)
    int Ne, roundsRun;
    int iterations[4], trials[4], nBad[4], exitKind[4];
    double pose[4][12], lambda[4], chi2[4];
};

struct PoseOptArgs {
    int nSingle;                 // the keypoint count when dN == nullptr
    const int* dN;               // [batch]
    int kpStride;
    const orbfe_keypoint* kp;    // [batch][kpStride]
    const int* match;            // [batch][kpStride]
    int nPoints;
    const float* pts;            // records of ptRec floats, x y z first
    size_t ptFrameFloats;        // FLOATS between two frames' points (0: shared); PoseImuArgs::ptFrameStride counts records
    int ptRec;
    const float* poseIn;         // [batch][12]
    float* poseOut;              // [batch][12]
    uint8_t* outlier;            // [batch][kpStride]
    int* nInliers;               // [batch]
    int* edgeIdx;                // [batch][kpStride] scratch: edge -> keypoint
    PoseOptRounds* rounds;       // nullable
    uint8_t* roundOutlier;       // nullable, [4][N_e]
    PoseCam cam;
    float chi2Thr;
    int iterations, nRounds, nLevels;
    float invSigma2[kMaxLevels];
};

struct PoseOptShared {
    double part[2][kPoseOptMaxWaves][kNV];
    int waveCount[kPoseOptMaxWaves];
};

// the frame as one thread sees it: where its run of edges is and how to fetch one
struct FrameView {
    const orbfe_keypoint* kp;
    const int* match;
    const float* pts;
    const int* edgeIdx;
    uint8_t* outlier;
    int Ne, first;   // first edge of this thread's run
};

__device__ __forceinline__ EdgeD load_edge(const PoseOptArgs& G, const FrameView& F, int c, int& kpIndex)
{
    const int i = F.edgeIdx[c];
    kpIndex = i;
    const orbfe_keypoint k = F.kp[i];
    const float* p = F.pts + (size_t)F.match[i] * G.ptRec;
    EdgeD E;
    E.ox = (double)k.x;
    E.oy = (double)k.y;
    E.w = (double)G.invSigma2[k.octave];
    E.X = (double)p[0];
    E.Y = (double)p[1];
    E.Z = (double)p[2];
    return E;
}

template <int RUN>
__device__ void pose_opt_frame(const PoseOptArgs& G, PoseOptShared& S, const TreeShape& T, const FrameView& F, const double (&R0)[9],
                               const double (&t0)[3], int frame)
{
    constexpr int NR = RUN > 0 ? RUN : 1;
    EdgeD E[NR];
    int kpOf[NR];
    bool act[NR];
    if (RUN > 0) {
#pragma unroll
        for (int k = 0; k < NR; k++) {
            act[k] = F.first + k < F.Ne;
            kpOf[k] = 0;
            E[k] = EdgeD{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (act[k]) E[k] = load_edge(G, F, F.first + k, kpOf[k]);
        }
    }
    // edge k of the run and whether it takes part (RUN = 0: the flag of the last round lives in the output array)
    auto fetch = [&](int k, EdgeD& e, int& kpIndex) -> bool {
        if (RUN > 0) {
            e = E[k];
            kpIndex = kpOf[k];
            return act[k];
        }
        const int c = F.first + k;
        if (c >= F.Ne) return false;
        e = load_edge(G, F, c, kpIndex);
        return F.outlier[kpIndex] == 0;
    };
    int flip = 0, nBadLast = 0;
    double R[9], t[3];
    int roundsRun = 0;
    for (int rnd = 0; rnd < G.nRounds; rnd++) {
        const bool huber = rnd <= 2;   // (:993-994)
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = R0[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = t0[i];   // every round restarts from the frame's pose (:961-962)
        double lam = 0.0, ni = 2.0, cur = 0.0;
        int nIt = 0, nTr = 0, exitKind = ORBFE_POSE_OPT_EXIT_RAN_ALL;
        for (int it = 0; it < G.iterations; it++) {
            nIt++;
            double acc[kNV];
            run_tree<RUN, kNV>(T.run, acc, [&](int k, double (&v)[kNV]) {
                EdgeD e;
                int ki;
                if (fetch(k, e, ki)) edge_terms(G.cam, e, R, t, huber, v);
                else {
#pragma unroll
                    for (int q = 0; q < kNV; q++) v[q] = 0.0;
                }
            });
            block_tree<kNV>(S, T, flip, acc);
            cur = acc[27];
            double b[6], diag[6];
            {
                int at = 0;
#pragma unroll
                for (int j = 0; j < 6; j++) {
                    diag[j] = acc[at];
                    at += 6 - j;
                    b[j] = acc[21 + j];
                }
            }
            if (it == 0) {
                double m = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++)
                    if (fabs(diag[j]) > m) m = fabs(diag[j]);
                lam = 1e-5 * m;
                ni = 2.0;
            }
            double rho = 0.0;
            int q = 0;
            while (q < kPoseOptTrials) {
                double A[6][6], dx[6];
                {
                    int at = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++)
#pragma unroll
                        for (int k = j; k < 6; k++) {
                            A[j][k] = acc[at];
                            A[k][j] = acc[at];
                            at++;
                        }
#pragma unroll
                    for (int j = 0; j < 6; j++) A[j][j] = diag[j] + lam;
                }
                bool ok;
                ldlt_solve6(A, b, dx, &ok);
                double Rn[9], tn[3];
                apply_update(dx, R, t, Rn, tn);
                double one[1];
                run_tree<RUN, 1>(T.run, one, [&](int k, double (&v)[1]) {
                    EdgeD e;
                    int ki;
                    v[0] = 0.0;
                    if (fetch(k, e, ki)) {
                        double x, y, z, e0, e1, chi2, rho0, rho1;
                        edge_residual(G.cam, e, Rn, tn, x, y, z, e0, e1, chi2);
                        robust(chi2, G.cam.delta, huber, rho0, rho1);
                        v[0] = rho0;
                    }
                });
                block_tree<1>(S, T, flip, one);
                double tmp = one[0];
                if (!ok) tmp = DBL_MAX;
                double scale = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) scale = scale + dx[j] * (lam * dx[j] + b[j]);
                scale = scale + 1e-3;
                rho = (cur - tmp) / scale;
                nTr++;
                q++;
                if (rho > 0.0 && fabs(tmp) <= DBL_MAX) {
#pragma unroll
                    for (int i = 0; i < 9; i++) R[i] = Rn[i];
#pragma unroll
                    for (int i = 0; i < 3; i++) t[i] = tn[i];
                    const double tt = 2.0 * rho - 1.0;
                    const double alpha = 1.0 - (tt * tt) * tt;
                    double sf = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;   // std::min(alpha, 2/3)
                    sf = (1.0 / 3.0) < sf ? sf : (1.0 / 3.0);                // std::max(1/3, .)
                    lam = lam * sf;
                    ni = 2.0;
                    cur = tmp;
                } else {
                    lam = lam * ni;
                    ni = ni * 2.0;
                }
                if (!(rho < 0.0)) break;
            }
            if (q == kPoseOptTrials) { exitKind = ORBFE_POSE_OPT_EXIT_TRIALS; break; }
            if (rho == 0.0) { exitKind = ORBFE_POSE_OPT_EXIT_RHO_ZERO; break; }
        }
        // the flags of the round on fresh errors at its final pose (:967-995; S14)
        double bad[1];
        run_tree<RUN, 1>(T.run, bad, [&](int k, double (&v)[1]) {
            v[0] = 0.0;
            const int c = F.first + k;
            if (c >= F.Ne) return;
            EdgeD e;
            int ki;
            if (RUN > 0) {
                e = E[k];
                ki = kpOf[k];
            } else {
                e = load_edge(G, F, c, ki);
            }
            double x, y, z, e0, e1, chi2;
            edge_residual(G.cam, e, R, t, x, y, z, e0, e1, chi2);
            const bool out = (float)chi2 > G.chi2Thr;
            if (RUN > 0) act[k] = !out;
            F.outlier[ki] = out ? 1 : 0;
            if (G.roundOutlier) G.roundOutlier[(size_t)rnd * F.Ne + c] = out ? 1 : 0;
            v[0] = out ? 1.0 : 0.0;
        });
        block_tree<1>(S, T, flip, bad);   // counts up to 65536 are exact in binary64
        nBadLast = (int)bad[0];
        roundsRun = rnd + 1;
        if (G.rounds && threadIdx.x == 0) {
            PoseOptRounds& I = *G.rounds;
            I.iterations[rnd] = nIt;
            I.trials[rnd] = nTr;
            I.nBad[rnd] = nBadLast;
            I.exitKind[rnd] = exitKind;
            for (int i = 0; i < 9; i++) I.pose[rnd][i] = R[i];
            for (int i = 0; i < 3; i++) I.pose[rnd][9 + i] = t[i];
            I.lambda[rnd] = lam;
            I.chi2[rnd] = cur;
        }
        if (F.Ne < 10) break;   // (:1055)
    }
    if (threadIdx.x == 0) {
        float* o = G.poseOut + (size_t)frame * 12;
        for (int i = 0; i < 9; i++) o[i] = (float)R[i];
        for (int i = 0; i < 3; i++) o[9 + i] = (float)t[i];
        G.nInliers[frame] = F.Ne - nBadLast;
        if (G.rounds) {
            G.rounds->Ne = F.Ne;
            G.rounds->roundsRun = roundsRun;
        }
    }
}

__global__ __launch_bounds__(kPoseOptThreads) void pose_opt_kernel(PoseOptArgs G)
{
    __shared__ PoseOptShared S;
    const int frame = blockIdx.x, tid = threadIdx.x, nT = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63, nWaves = nT >> 6;
    int n = G.dN ? G.dN[frame] : G.nSingle;
    n = n < 0 ? 0 : (n > G.kpStride ? G.kpStride : n);
    const size_t base = (size_t)frame * G.kpStride;
    FrameView F;
    F.kp = G.kp + base;
    F.match = G.match + base;
    F.pts = G.pts + (size_t)frame * G.ptFrameFloats;
    F.outlier = G.outlier + base;
    int* edgeIdx = G.edgeIdx + base;
    F.edgeIdx = edgeIdx;
    // edges = the matched keypoints in keypoint order: each thread counts a contiguous chunk, the counts are scanned, the indices written
    const int per = (n + nT - 1) / nT;
    const int lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    auto is_edge = [&](int i) {
        const int m = F.match[i];
        const int o = F.kp[i].octave;
        return m >= 0 && m < G.nPoints && o >= 0 && o < G.nLevels;
    };
    int cnt = 0;
    for (int i = lo; i < hi; i++) {
        F.outlier[i] = 0;
        cnt += is_edge(i) ? 1 : 0;
    }
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if (lane == 63) S.waveCount[wave] = incl;
    __syncthreads();
    int before = 0, Ne = 0;
    for (int w = 0; w < nWaves; w++) {
        const int c = S.waveCount[w];
        if (w < wave) before += c;
        Ne += c;
    }
    int at = before + incl - cnt;
    for (int i = lo; i < hi; i++)
        if (is_edge(i)) edgeIdx[at++] = i;
    __syncthreads();   // the index list is read by other threads of this block
    F.Ne = Ne;

    double R0[9], t0[3];
    const float* pin = G.poseIn + (size_t)frame * 12;
    for (int i = 0; i < 9; i++) R0[i] = (double)pin[i];
    for (int i = 0; i < 3; i++) t0[i] = (double)pin[9 + i];
    if (Ne < 3) {   // (:949)
        if (tid == 0) {
            for (int i = 0; i < 12; i++) G.poseOut[(size_t)frame * 12 + i] = pin[i];
            G.nInliers[frame] = 0;
            if (G.rounds) {
                G.rounds->Ne = Ne;
                G.rounds->roundsRun = 0;
            }
        }
        return;
    }
    int P = 1, lg = 0;
    while (P < Ne) { P <<= 1; lg++; }
    TreeShape T;
    T.run = P > nT ? P / nT : 1;
    int lgRun = 0;
    while ((1 << lgRun) < T.run) lgRun++;
    const int lgThreads = lg - lgRun;   // log2 of the threads that own edges
    T.lvWave = lgThreads < 6 ? lgThreads : 6;
    T.lvCross = lgThreads - T.lvWave;
    F.first = tid * T.run;
    if (T.run == 1) pose_opt_frame<1>(G, S, T, F, R0, t0, frame);
    else if (T.run == 2) pose_opt_frame<2>(G, S, T, F, R0, t0, frame);
    else if (T.run == 4) pose_opt_frame<4>(G, S, T, F, R0, t0, frame);
    else pose_opt_frame<0>(G, S, T, F, R0, t0, frame);
}

constexpr char kPoseOptSizeErr[] =
    "orbfe_pose_opt_params / orbfe_pose_opt_info struct_size does not match this library (rebuild the caller against include/orbfe.h)";

void fill_args(PoseOptArgs& G, const orbfe_pose_opt_params* P, const float* invLevelSigma2, int nLevels)
{
    memset(&G, 0, sizeof G);
    fill_pose_cam(G.cam, P->cam, P->huber_delta2);
    G.chi2Thr = P->chi2_threshold;
    G.iterations = P->iterations;
    G.nRounds = P->rounds;
    G.nLevels = nLevels;
    for (int i = 0; i < kMaxLevels; i++) G.invSigma2[i] = i < nLevels ? invLevelSigma2[i] : 0.0f;
}

}  // namespace

// struct sizes, the unsupported branches and the ranges: no device is touched
int pose_opt_check(const orbfe_pose_opt_params* P, const orbfe_pose_opt_info* info, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_pose_opt_params) || (info && info->struct_size != (int)sizeof(orbfe_pose_opt_info))) {
        err = kPoseOptSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    const int rc = solver_check_common(P, "orbfe_pose_optimization", "branch of PoseOptimization is", "S14", err);
    if (rc != ORBFE_OK) return rc;
    if (P->rounds < 1 || P->rounds > 4 || !(P->chi2_threshold >= 0.0f)) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// Everything of the host call that needs no device: the refusals, the outputs of a call that runs nothing, the edge list.
// *Ne < 3 (:949): the call is complete, nothing is launched.
int pose_opt_begin(const orbfe_pose_opt_params* P, int nLevels, int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints,
                   const float* Rcw, const float* tcw, float* TcwOut, uint8_t* outlier, int* nInliers, orbfe_pose_opt_info* info,
                   std::vector<int>& first, std::string& err)
{
    const int crc = pose_opt_check(P, info, err);
    if (crc != ORBFE_OK) return crc;
    const int rc = pose_edge_list(nLevels, n, kp, mpIndex, nPoints, first);
    if (rc != ORBFE_OK) return rc;
    const int Ne = (int)first.size();
    *nInliers = 0;
    fill_tcw(Rcw, tcw, TcwOut);
    if (n > 0) memset(outlier, 0, (size_t)n);
    uint8_t* infoOutlier = info ? info->outlier : nullptr;
    if (info) {
        memset(info, 0, sizeof *info);
        info->struct_size = (int)sizeof(orbfe_pose_opt_info);
        info->outlier = infoOutlier;
        info->N_e = Ne;
    }
    return ORBFE_OK;
}

// the device part of the host call, for the edge list `first` (>= 3 entries) of pose_opt_begin
int pose_opt_run(MatchScratch& m, hipStream_t s, const orbfe_pose_opt_params* P, const float* invLevelSigma2, int nLevels, int n,
                 const orbfe_keypoint* kp, const int* mpIndex, const float* points, const float* Rcw, const float* tcw,
                 const std::vector<int>& first, float* TcwOut, uint8_t* outlier, int* nInliers, orbfe_pose_opt_info* info, std::string& err)
{
    const int Ne = (int)first.size();
    if (Ne < 3) return ORBFE_ERR_INVALID_ARG;

    // the unit's blocks (EdgeStaging, match_common.h): up [pose]; down [pose | nInliers | rounds]
    EdgeStaging st(n, first, nullptr);
    const auto bPose = st.in<float>(12);
    st.inputs_done();
    const auto bPoseOut = st.out<float>(12);
    const auto bNInl = st.out<int>(1);
    const auto bRounds = st.out<PoseOptRounds>(1);
    int rc = st.stage(m, kp, first, mpIndex, points, nullptr, err);
    if (rc != ORBFE_OK) return rc;
    float* hPose = st.host(bPose);
    for (int i = 0; i < 9; i++) hPose[i] = Rcw[i];
    for (int i = 0; i < 3; i++) hPose[9 + i] = tcw[i];
    rc = st.upload(s, bRounds, err);
    if (rc != ORBFE_OK) return rc;

    PoseOptArgs G;
    fill_args(G, P, invLevelSigma2, nLevels);
    st.set_args(G, bNInl, bRounds);
    G.poseIn = st.dev(bPose);
    G.poseOut = st.dev(bPoseOut);
    hipLaunchKernelGGL(pose_opt_kernel, dim3(1), dim3(Ne <= 64 ? 64 : kPoseOptThreads), 0, s, G);
    rc = st.download(s, outlier, err);
    if (rc != ORBFE_OK) return rc;
    const float* pose = st.res(bPoseOut);
    const PoseOptRounds* I = st.res(bRounds);
    fill_tcw(pose, pose + 9, TcwOut);
    *nInliers = *st.res(bNInl);
    if (info) {
        info->rounds_run = I->roundsRun;
        memcpy(info->iterations, I->iterations, sizeof I->iterations);
        memcpy(info->trials, I->trials, sizeof I->trials);
        memcpy(info->n_bad, I->nBad, sizeof I->nBad);
        memcpy(info->exit_kind, I->exitKind, sizeof I->exitKind);
        memcpy(info->pose, I->pose, sizeof I->pose);
        memcpy(info->lambda, I->lambda, sizeof I->lambda);
        memcpy(info->chi2, I->chi2, sizeof I->chi2);
        st.round_rows(info->outlier, I->roundsRun);
    }
    return ORBFE_OK;
}

int pose_opt_batch_device(MatchScratch& m, hipStream_t s, const orbfe_pose_opt_params* P, const float* invLevelSigma2, int nLevels,
                          int batch, const orbfe_keypoint* dKp, const int* dN, int kpStride, const int* dMatch, int nMapPoints,
                          const orbfe_world_point* dPoints, int pointStrideFrames, const float* dPoseIn, float* dPoseOut,
                          uint8_t* dOutlier, int* dNInliers, std::string& err)
{
    const int crc = pose_opt_check(P, nullptr, err);
    if (crc != ORBFE_OK) return crc;
    if (kpStride > kPoseMaxKp) return ORBFE_ERR_INVALID_ARG;
    int rc = ensure(m, (size_t)batch * kpStride * sizeof(int), 0, err);
    if (rc != ORBFE_OK) return rc;
    PoseOptArgs G;
    fill_args(G, P, invLevelSigma2, nLevels);
    G.dN = dN;
    G.kpStride = kpStride;
    G.kp = dKp;
    G.match = dMatch;
    G.nPoints = nMapPoints;
    G.pts = reinterpret_cast<const float*>(dPoints);
    G.ptRec = (int)(sizeof(orbfe_world_point) / sizeof(float));
    G.ptFrameFloats = (size_t)pointStrideFrames * G.ptRec;
    G.poseIn = dPoseIn;
    G.poseOut = dPoseOut;
    G.outlier = dOutlier;
    G.nInliers = dNInliers;
    G.edgeIdx = static_cast<int*>(m.d);
    hipLaunchKernelGGL(pose_opt_kernel, dim3(batch), dim3(kPoseOptThreads), 0, s, G);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

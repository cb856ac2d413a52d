// kernels_poseimu_prev.hip -- Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:3846-4275; the call: src/Tracking.cc:946)
// on gfx950 for the branch this fork takes: one pinhole camera, EdgeMonoOnlyPose, one EdgeInertial with all six vertices free,
// EdgeGyroRW, EdgeAccRW and EdgePriorPoseImu; 30 unknowns; the 30 x 30 Hessian and Optimizer::Marginalize (:2882-2962).
//
// SPEC DECISION S20.  tests/pose_inertial_prev_ref.py is the normative restatement; every byte this file
// produces is compared with it.  The call itself is poseimu_prev_math.h's prev_solve, one text for this kernel and for the host
// yardstick (tests/cpp/pose_inertial_prev.cpp); this file holds what a block does differently from one thread.
//
// pose_prev_kernel: ONE block of kTreeThreads per frame runs the whole call with no host step and no second launch.
//   The mono edges go through S19's tree with S19's item mapping (block_tree.h).
//   Everything indexed at run time -- the Jacobian blocks, the 24 x 24 and 15 x 15 edge Hessians, the 30 x 30 system and its factor,
//   the matrices of the marginalisation -- lives in LDS (PrevWork, about 39 KB): LDS takes dynamic indices without scratch memory.
//   A phase of prev_solve spreads its items over the block and ends on a barrier; the block-uniform values between phases (the
//   pivot, the rotation angle, ok) are read by every thread from LDS, so every branch is taken by all threads or by none.
//   The 30 x 30 solve is S19's row-per-lane scheme on LDS rows (block_ldlt30): lane i of wave 0 owns row i of A and of L.
//   The marginalisation runs with the 15 x 15 matrices in LDS; item k of a rotation owns index k of its loops.
// Every loop has a static trip bound; NaN follows the comparisons as written.
#include <cstring>
#include <vector>

#include "match_common.h"
#include "block_tree.h"
#include "poseimu_prev_math.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

struct PosePrevArgs {
    int nSingle;                 // the keypoint count when dN == nullptr
    const int* dN;               // [batch]
    int kpStride;
    const orbfe_keypoint* kp;    // [batch][kpStride]
    const int* match;            // [batch][kpStride]
    int nPoints;
    const float* pts;            // records of ptRec floats, x y z first
    const float* depth;          // one float per point record
    size_t ptFrameStride;        // records between two frames' points (0: shared)
    int ptRec;
    const orbfe_imu_link_free* link;   // [batch]
    const orbfe_pose_imu_prior* prior; // [batch]
    const float* stateIn;        // [batch][33]
    float* stateOut;             // [batch][21]
    double* H30;                 // [batch][900]
    double* Hprior;              // [batch][225], nullable
    uint8_t* outlier;            // [batch][kpStride]
    int* nInliers;               // [batch]
    int* accepted;               // [batch]
    int* edgeIdx;                // [batch][kpStride] scratch: edge -> keypoint
    PrevRoundsOut* rounds;       // nullable
    uint8_t* roundOutlier;       // nullable, [4][N_e]
    PoseCam cam;
    PrevPar par;
    int nLevels;
    float closeDepth;
    float invSigma2[kMaxLevels];
};

struct PosePrevShared {
    double part[2][kTreeMaxWaves][kNV];
    int waveCount[kTreeMaxWaves];
    PrevWork work;
    PrevState state;             // one copy for the block: every thread reads it, one thread updates it between barriers
};

struct PrevFrameView {
    const orbfe_keypoint* kp;
    const int* match;
    const float* pts;
    const float* depth;
    const int* edgeIdx;
    uint8_t* outlier;
    int Ne;
};

__device__ __forceinline__ EdgeD load_edge(const PosePrevArgs& G, const PrevFrameView& F, int c, int& kpIndex, float& depth)
{
    const int i = F.edgeIdx[c];
    kpIndex = i;
    const orbfe_keypoint k = F.kp[i];
    const int m = F.match[i];
    const float* p = F.pts + (size_t)m * G.ptRec;
    depth = F.depth[m];
    EdgeD E;
    E.ox = (double)k.x;
    E.oy = (double)k.y;
    E.w = (double)G.invSigma2[k.octave];
    E.X = (double)p[0];
    E.Y = (double)p[1];
    E.Z = (double)p[2];
    return E;
}

template <int NV, class Term>
__device__ __forceinline__ void prev_run_tree(const TreeShape& T, double (&out)[NV], Term term)
{
    if (T.run == 1) term(0, out);
    else wave_run_tree<NV>(T.run, out, term);
}

// A x = b for the symmetric 30 x 30 W.A (destroyed) -> W.dx, W.ok: ldlt_solve_n<30> (ldlt.h) operation for operation.  Called by every
// thread of the block.  Lane i < 30 of wave 0 owns row i of A and of L in LDS.  At step k every thread scans the diagonal k .. 29 in
// order and keeps the first of equals ('>'), so `best` is block-uniform; rows k and best are exchanged column by column (lane j takes
// column j), then the two columns row by row; lane i > k takes l_i = A[i][k] / d_k and its row of the trailing block, A_ij - l_i A[j][k]
// for j = k + 1 .. i, and stores the mirror as the indexed text does -- column k is not written in step k, and an entry is written by
// one lane only.  The forward substitution keeps each sum in the indexed text's order: lane i subtracts l_ij z_j for j = 0 .. i - 1 in
// turn and z_j is read from lane j; the back substitution runs on wave-uniform values, L's column i read from lane i's registers.
__device__ __forceinline__ bool block_ldlt30(PrevWork& W)
{
    constexpr int N = kPrevN;
    const int tid = threadIdx.x;
    const bool row = tid < N;
    for (int t = tid; t < N * kPrevLd; t += blockDim.x) (&W.L[0][0])[t] = 0.0;
    if (row) W.perm[tid] = tid;
    __syncthreads();
    for (int k = 0; k < N; k++) {
        int best = k;
        double bestAbs = fabs(W.A[k][k]);
        for (int i = k + 1; i < N; i++) {
            const double v = fabs(W.A[i][i]);
            if (v > bestAbs) { best = i; bestAbs = v; }
        }
        __syncthreads();   // the diagonal is read before a swap rewrites it
        if (best != k) {
            if (row) {
                const double a = W.A[k][tid], l = W.L[k][tid];
                W.A[k][tid] = W.A[best][tid];
                W.A[best][tid] = a;
                W.L[k][tid] = W.L[best][tid];
                W.L[best][tid] = l;
            }
            if (tid == 64) {
                const int p = W.perm[k];
                W.perm[k] = W.perm[best];
                W.perm[best] = p;
            }
            __syncthreads();
            if (row) {
                const double a = W.A[tid][k];
                W.A[tid][k] = W.A[tid][best];
                W.A[tid][best] = a;
            }
            __syncthreads();
        }
        const double dk = W.A[k][k];
        if (tid == 0) W.d[k] = dk;
        if (row && tid > k) {
            const double li = dk == 0.0 ? 0.0 : W.A[tid][k] / dk;
            W.L[tid][k] = li;
            for (int j = k + 1; j <= tid; j++) {
                const double val = W.A[tid][j] - li * W.A[j][k];
                W.A[tid][j] = val;
                W.A[j][tid] = val;
            }
        }
        __syncthreads();
    }
    if (tid < 64) {   // wave 0, all 64 lanes active
        const int r = row ? tid : 0;
        double acc = row ? W.b[W.perm[r]] : 0.0;
        for (int j = 0; j < N; j++) {
            const double zj = readlane_f64(acc, j);
            const double l = W.L[r][j];
            if (row && tid > j) acc = acc - l * zj;
        }
        const double dr = W.d[r];
        const double w = dr == 0.0 ? 0.0 : acc / dr;
        double col[N];   // L[j][lane]: column `lane` of L, compile-time indices
#pragma unroll
        for (int j = 0; j < N; j++) col[j] = W.L[j][r];
        double xs = 0.0;   // xs[lane], known from step i = lane on
        for (int i = N - 1; i >= 0; i--) {   // every lane runs row `lane`'s sum over the xs known so far; lane i's is complete
            double a = w;
#pragma unroll
            for (int j = 1; j < N; j++) {
                const double xj = readlane_f64(xs, j);
                const double nx = a - col[j] * xj;
                a = j > i ? nx : a;
            }
            xs = tid == i ? a : xs;
        }
        if (row) W.dx[W.perm[tid]] = xs;
        if (tid == 0) {
            bool pos = true;
            for (int i = 0; i < N; i++) pos = pos && W.d[i] > 0.0;
            W.ok = pos ? 1 : 0;
        }
    }
    __syncthreads();
    return W.ok != 0;
}

// what a block does where one thread loops (poseimu_prev_math.h)
struct BlockExec {
    const PosePrevArgs& G;
    PosePrevShared& Sh;
    const TreeShape& T;
    const PrevFrameView& F;
    const orbfe_imu_link_free& K;
    int flip;

    template <class Fn>
    __device__ __forceinline__ void each(int n, Fn f)
    {
        for (int t = threadIdx.x; t < n; t += blockDim.x) f(t);
        __syncthreads();
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ bool leader() const { return threadIdx.x == 0; }
    __device__ __forceinline__ int Ne() const { return F.Ne; }
    __device__ __forceinline__ int item(int c) const { return ((threadIdx.x >> 6) * T.run + c) * 64 + (threadIdx.x & 63); }

    __device__ __forceinline__ void mono_sums(bool huber, const ImuState& S, PrevWork& W)
    {
        double acc[kNV];
        prev_run_tree<kNV>(T, acc, [&](int c, double (&v)[kNV]) {
            const int e = item(c);
            bool on = e < F.Ne;
            EdgeD E = EdgeD{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (on) {
                int ki;
                float dep;
                E = load_edge(G, F, e, ki, dep);
                on = F.outlier[ki] == 0;
            }
            if (on) {
                double Rcb[9], tbc[3];
#pragma unroll
                for (int i = 0; i < 9; i++) Rcb[i] = (double)K.Rcb[i];
#pragma unroll
                for (int i = 0; i < 3; i++) tbc[i] = (double)K.tbc[i];
                imu_edge_terms(G.cam, E, S.Rcw, S.tcw, Rcb, tbc, huber, v);
            } else {
#pragma unroll
                for (int q = 0; q < kNV; q++) v[q] = 0.0;
            }
        });
        block_tree<kNV>(Sh, T, flip, acc);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < kNV; q++) W.acc[q] = acc[q];
        }
        __syncthreads();
    }

    __device__ __forceinline__ bool solve(PrevWork& W) { return block_ldlt30(W); }

    // the flags of the round on fresh errors at its final state (:4100-4128; S19's departure 2)
    __device__ __forceinline__ int score(int rnd, float thr, float thrClose, const ImuState& S)
    {
        double bad[1];
        prev_run_tree<1>(T, bad, [&](int c, double (&v)[1]) {
            v[0] = 0.0;
            const int e = item(c);
            if (e >= F.Ne) return;
            int ki;
            float dep;
            const EdgeD E = load_edge(G, F, e, ki, dep);
            double x, y, z, e0, e1, chi2;
            edge_residual(G.cam, E, S.Rcw, S.tcw, x, y, z, e0, e1, chi2);
            const bool out = imu_edge_is_outlier(chi2, z, dep < G.closeDepth, thr, thrClose);
            F.outlier[ki] = out ? 1 : 0;
            if (G.roundOutlier) G.roundOutlier[(size_t)rnd * F.Ne + e] = out ? 1 : 0;
            v[0] = out ? 1.0 : 0.0;
        });
        block_tree<1>(Sh, T, flip, bad);   // counts up to 65536 are exact in binary64
        return (int)bad[0];
    }

    __device__ __forceinline__ int recover(float thr, const ImuState& S)
    {
        double bad[1];
        prev_run_tree<1>(T, bad, [&](int c, double (&v)[1]) {
            v[0] = 0.0;
            const int e = item(c);
            if (e >= F.Ne) return;
            int ki;
            float dep;
            const EdgeD E = load_edge(G, F, e, ki, dep);
            double x, y, z, e0, e1, chi2;
            edge_residual(G.cam, E, S.Rcw, S.tcw, x, y, z, e0, e1, chi2);
            const bool good = (float)chi2 < thr;
            if (good) F.outlier[ki] = 0;
            v[0] = good ? 0.0 : 1.0;
        });
        block_tree<1>(Sh, T, flip, bad);
        return (int)bad[0];
    }
};

__global__ __launch_bounds__(kTreeThreads) void pose_prev_kernel(PosePrevArgs G)
{
    __shared__ PosePrevShared S;
    const int frame = blockIdx.x, tid = threadIdx.x, nT = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63, nWaves = nT >> 6;
    int n = G.dN ? G.dN[frame] : G.nSingle;
    n = n < 0 ? 0 : (n > G.kpStride ? G.kpStride : n);
    const size_t base = (size_t)frame * G.kpStride;
    PrevFrameView F;
    F.kp = G.kp + base;
    F.match = G.match + base;
    F.pts = G.pts + (size_t)frame * G.ptFrameStride * G.ptRec;
    F.depth = G.depth + (size_t)frame * G.ptFrameStride;
    F.outlier = G.outlier + base;
    int* edgeIdx = G.edgeIdx + base;
    F.edgeIdx = edgeIdx;
    // edges = the matched keypoints in keypoint order: each thread counts a contiguous chunk, the counts are scanned, the indices written
    // (pose_imu_kernel's prologue, repeated: see there)
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
    __syncthreads();   // the index list and the cleared flags are read by other threads of this block
    F.Ne = Ne;

    int P = 1, lg = 0;
    while (P < Ne) { P <<= 1; lg++; }
    TreeShape T;
    if (P > kTreeThreads) {   // the waves walk chunks: the six wave levels are taken per chunk, inside prev_run_tree
        T.run = P / kTreeThreads;
        T.lvWave = 0;
        T.lvCross = 2;
    } else {
        T.run = 1;
        T.lvWave = lg < 6 ? lg : 6;
        T.lvCross = lg - T.lvWave;
    }

    const orbfe_imu_link_free& K = G.link[frame];
    const orbfe_pose_imu_prior& Pr = G.prior[frame];
    PrevState& St = S.state;
    if (tid == 0) {
        const float* in = G.stateIn + (size_t)frame * kImuStateIn;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            St.cur.Rcw[i] = (double)in[i];
            St.cur.Rwb[i] = (double)in[12 + i];
            St.prv.Rwb[i] = (double)K.Rwb1[i];
            St.prv.Rcw[i] = 0.0;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            St.cur.tcw[i] = (double)in[9 + i];
            St.cur.twb[i] = (double)in[21 + i];
            St.cur.v[i] = (double)in[24 + i];
            St.cur.bg[i] = (double)in[27 + i];
            St.cur.ba[i] = (double)in[30 + i];
            St.prv.twb[i] = (double)K.twb1[i];
            St.prv.v[i] = (double)K.v1[i];
            St.prv.bg[i] = (double)K.bg1[i];
            St.prv.ba[i] = (double)K.ba1[i];
            St.prv.tcw[i] = 0.0;
        }
    }
    __syncthreads();
    BlockExec X{G, S, T, F, K, 0};
    PrevOut O;
    O.state = G.stateOut + (size_t)frame * kImuState;
    O.H30 = G.H30 + (size_t)frame * kPrevH;
    O.Hprior = G.Hprior ? G.Hprior + (size_t)frame * (kMargN * kMargN) : nullptr;
    O.nInliers = G.nInliers + frame;
    O.accepted = G.accepted + frame;
    O.rounds = G.rounds;
    prev_solve(X, K, Pr, G.par, St, S.work, O);
}

constexpr char kPosePrevSizeErr[] =
    "orbfe_pose_inertial_prev_params / orbfe_imu_link_free / orbfe_pose_imu_prior / orbfe_pose_inertial_prev_info struct_size does not "
    "match this library (rebuild the caller against include/orbfe.h)";

void fill_args(PosePrevArgs& G, const orbfe_pose_inertial_prev_params* P, const float* invLevelSigma2, int nLevels)
{
    fill_inertial_args(G, G.par, P, invLevelSigma2, nLevels);
    G.par.priorDelta = P->prior_huber_delta;
    G.par.inlierThreshold = P->inlier_threshold;
}

}  // namespace

// struct sizes, the unsupported branches and the ranges: no device is touched
int pose_prev_check(const orbfe_pose_inertial_prev_params* P, const orbfe_imu_link_free* link, const orbfe_pose_imu_prior* prior,
                    const orbfe_pose_inertial_prev_info* info, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_pose_inertial_prev_params) || (link && link->struct_size != (int)sizeof(orbfe_imu_link_free)) ||
        (prior && prior->struct_size != (int)sizeof(orbfe_pose_imu_prior)) ||
        (info && info->struct_size != (int)sizeof(orbfe_pose_inertial_prev_info))) {
        err = kPosePrevSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    const int rc = solver_check_common(P, "orbfe_pose_inertial_optimization_last_frame", "branch of PoseInertialOptimizationLastFrame is",
                                       "S20", err);
    if (rc != ORBFE_OK) return rc;
    if (P->rounds < 1 || P->rounds > 4 || !(P->close_factor >= 0.0) || P->recover_below < 0 || !(P->prior_huber_delta > 0.0))
        return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++)
        if (!(P->chi2[i] >= 0.0f)) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// Everything of the host call that needs no device: the refusals and the edge list.
int pose_prev_begin(const orbfe_pose_inertial_prev_params* P, const orbfe_imu_link_free* link, const orbfe_pose_imu_prior* prior, int nLevels,
                    int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints, orbfe_pose_inertial_prev_info* info,
                    std::vector<int>& first, std::string& err)
{
    const int crc = pose_prev_check(P, link, prior, info, err);
    if (crc != ORBFE_OK) return crc;
    return pose_edge_list(nLevels, n, kp, mpIndex, nPoints, first);
}

// the device part of the host call, for the edge list `first` of pose_prev_begin (it may be empty)
int pose_prev_run(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_prev_params* P, const orbfe_imu_link_free* link,
                  const orbfe_pose_imu_prior* prior, const float* invLevelSigma2, int nLevels, int n, const orbfe_keypoint* kp,
                  const int* mpIndex, const float* points, const float* trackDepth, const float* stateIn, const std::vector<int>& first,
                  float* stateOut, double* H30out, double* HpriorOut, uint8_t* outlier, int* nInliers, int* accepted,
                  orbfe_pose_inertial_prev_info* info, std::string& err)
{
    // the unit's blocks (EdgeStaging, match_common.h): up [state | link | prior]; down [state | nInliers, accepted | rounds | H30 | Hprior]
    EdgeStaging st(n, first, trackDepth);
    const auto bState = st.in<float>(kImuStateIn);
    const auto bLink = st.in<orbfe_imu_link_free>(1);
    const auto bPrior = st.in<orbfe_pose_imu_prior>(1);
    st.inputs_done();
    const auto bStateOut = st.out<float>(kImuState);
    const auto bNInl = st.out<int>(2);  // nInliers, accepted
    const auto bRounds = st.out<PrevRoundsOut>(1);
    const auto bH = st.out<double>(kPrevH);
    const auto bHp = st.out<double>(kMargN * kMargN);
    int rc = st.stage(m, kp, first, mpIndex, points, trackDepth, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bState, stateIn);
    st.put(bLink, link);
    st.put(bPrior, prior);
    rc = st.upload(s, bRounds, err);
    if (rc != ORBFE_OK) return rc;

    PosePrevArgs G;
    fill_args(G, P, invLevelSigma2, nLevels);
    st.set_args(G, bNInl, bRounds);
    G.depth = st.dev(st.bDepth);
    G.link = st.dev(bLink);
    G.prior = st.dev(bPrior);
    G.stateIn = st.dev(bState);
    G.stateOut = st.dev(bStateOut);
    G.H30 = st.dev(bH);
    G.Hprior = HpriorOut ? st.dev(bHp) : nullptr;
    G.accepted = G.nInliers + 1;
    hipLaunchKernelGGL(pose_prev_kernel, dim3(1), dim3(kTreeThreads), 0, s, G);
    rc = st.download(s, outlier, err);
    if (rc != ORBFE_OK) return rc;
    st.get(bStateOut, stateOut);
    *nInliers = st.res(bNInl)[0];
    *accepted = st.res(bNInl)[1];
    st.get(bH, H30out);
    st.get(bHp, HpriorOut);
    if (info) {
        const PrevRoundsOut* I = st.res(bRounds);
        fill_inertial_info(info, I, st);
        memcpy(info->prior_chi2, I->priorChi2, sizeof I->priorChi2);
        memcpy(info->prior_weight, I->priorWeight, sizeof I->priorWeight);
    }
    return ORBFE_OK;
}

int pose_prev_batch_device(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_prev_params* P, const float* invLevelSigma2,
                           int nLevels, int batch, const orbfe_imu_link_free* dLinks, const orbfe_pose_imu_prior* dPriors,
                           const orbfe_keypoint* dKp, const int* dN, int kpStride, const int* dMatch, int nMapPoints,
                           const orbfe_world_point* dPoints, int pointStrideFrames, const float* dTrackDepth, const float* dStateIn,
                           float* dStateOut, double* dH30, double* dHprior, uint8_t* dOutlier, int* dNInliers, int* dAccepted,
                           std::string& err)
{
    const int crc = pose_prev_check(P, nullptr, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return crc;
    if (kpStride > kPoseMaxKp) return ORBFE_ERR_INVALID_ARG;
    int rc = ensure(m, (size_t)batch * kpStride * sizeof(int), 0, err);
    if (rc != ORBFE_OK) return rc;
    PosePrevArgs G;
    fill_args(G, P, invLevelSigma2, nLevels);
    G.dN = dN;
    G.kpStride = kpStride;
    G.kp = dKp;
    G.match = dMatch;
    G.nPoints = nMapPoints;
    G.pts = reinterpret_cast<const float*>(dPoints);
    G.depth = dTrackDepth;
    G.ptRec = (int)(sizeof(orbfe_world_point) / sizeof(float));
    G.ptFrameStride = (size_t)pointStrideFrames;
    G.link = dLinks;
    G.prior = dPriors;
    G.stateIn = dStateIn;
    G.stateOut = dStateOut;
    G.H30 = dH30;
    G.Hprior = dHprior;
    G.outlier = dOutlier;
    G.nInliers = dNInliers;
    G.accepted = dAccepted;
    G.edgeIdx = static_cast<int*>(m.d);
    hipLaunchKernelGGL(pose_prev_kernel, dim3(batch), dim3(kTreeThreads), 0, s, G);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

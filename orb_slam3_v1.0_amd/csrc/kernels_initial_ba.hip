// kernels_initial_ba.hip -- the bundle adjustment of the initial map: Optimizer::GlobalBundleAdjustemnt(map, 20) as
// CreateInitialMapMonocular calls it (src/Tracking.cc:698 -> src/Optimizer.cc:60-369) on gfx950, for the one shape that call has: two
// key frames of which the first is fixed, N points each seen once in either frame, EdgeSE3ProjectXYZ
// (src/OptimizableTypes.cpp:139-160), pinhole.
//
// SPEC DECISION S17: S14's rules (binary64 where the C++ is double, one operation per operator, no contraction,
// every sum over points a fixed pairwise tree over P = the smallest power of two >= N) and S14's text for the residual, Huber, the pose
// Jacobian, exp, the Levenberg loop and the 6 x 6 solve; new is the point side -- the 2 x 3 point Jacobian, the per-point 3 x 3 blocks
// and their inverses, the Schur reduction to ONE 6 x 6 system (one pose is free) and the back-substitution.  tests/initial_ba_ref.py
// is the normative restatement; every byte this file produces is compared with it.  What one thread computes for one point
// (initial_ba_math.h) is host-safe text that tests/cpp/initial_ba.cpp includes; this file holds the mapping, the loop and the host call.
//
// initial_ba_kernel: ONE block runs the whole call -- every iteration, every trial, the final chi2 -- with no host step and no second
// launch.  An iteration is one build (sum of 28 values, with the maximum behind lambda_0 folded into the same exchange) and per trial
// one Schur sum (27 values) and one trial sum (the cost and the point part of the gain's denominator, one exchange).
//   Mapping of the tree.  P <= 512: S14's -- thread t owns the aligned run of r = max(1, P / T) <= 2 points, whose linearisation (27
//   doubles a point) and position stay in registers between the build and every trial of the iteration; run_tree / block_tree of
//   block_tree.h.  (A run of 4 would hold 264 VGPRs of point state next to the 6 x 6 solve.  Observed once, with that
//   instantiation compiled alone for gfx950: 256 VGPRs + 256 AGPRs, 181 VGPR spills, 640 bytes of scratch a lane; no test keeps the
//   figure.  This kernel is to use no scratch memory.)  P > 512: a point's state is parked in the arena (field-major, so a wave reads
//   consecutive words) and the run is walked by the WAVE, not the thread: wave w owns the aligned run of P / 256 >= 4 chunks of 64
//   consecutive points, lane l takes point l of the chunk, the chunk is summed by the six wave levels, and the chunk sums are
//   combined by a binary counter whose stack level j lives in lane j's registers (written under lane == j, read with readlane).
//   A thread-owned run needs that stack per thread -- 8 levels of 28 doubles, dynamically indexed -- which is scratch memory
//   (pose_opt_kernel pays 2304 bytes a lane for it); the wave-owned run adds the same pairs in the same order with every register
//   index a compile-time one.
//   Every thread then holds the sums and runs the 6 x 6 solve, exp and the accept / reject rule redundantly, as in S14.
// Every loop has a static trip bound (iterations <= 64, 10 trials, chunks <= 256, counter levels <= 8); NaN follows the comparisons as
// written and can neither be accepted nor make a loop spin.
#include <cfloat>
#include <cstring>
#include <vector>

#include "match_common.h"
#include "block_tree.h"
#include "ldlt.h"
#include "initial_ba_math.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

constexpr int kBaMaxKp = 65536;
constexpr int kBaTrials = 10;
constexpr int kBaMaxIterations = 64;
constexpr int kBaRegisterP = 2 * kTreeThreads;   // the largest P whose points stay in registers
constexpr int kBaState = kBaNL + 6;              // parked doubles a point: its linearisation, its position, its trial position

struct BaDeviceInfo {   // what the kernel reports per call
    int nIterations, nTrials, exitKind, pad;
    int trials[kBaMaxIterations];
    double cost[kBaMaxIterations], lambda[kBaMaxIterations], pose[12];
};

struct BaArgs {
    int N, P;
    const float* obs;     // [N][6]: x1 y1 w1 x2 y2 w2
    const float* x0;      // [N][3]
    double* park;         // [kBaState][P] when P > kBaRegisterP
    float* xOut;          // [N][3]
    double* chi2;         // [2][N]
    uint8_t* front;       // [2][N]
    BaDeviceInfo* info;
    double Ra[9], ta[3], R0[9], t0[3];
    PoseCam cam;
    int iterations, huber;
};

struct BaShared {
    double part[2][kTreeMaxWaves][kNV + 1];
};

// The part of a sum below the exchange.  RUN = 1, 2: the thread's run (run_tree).  RUN = 0: the wave's run of T.run chunks:
// term(c, v) fills the values of this lane's point of chunk c, the six wave levels sum the chunk, and the binary counter adds chunk
// 2i to chunk 2i + 1 first, then pairs of pairs; level j of its stack is held by lane j.
// The walk is block_tree.h's wave_run_tree written out: calling it re-numbers this kernel's registers and moved its time (r20).
template <int RUN, int NV, class Term>
__device__ __forceinline__ void ba_run_tree(const TreeShape& T, double (&out)[NV], Term term)
{
    if (RUN > 0) {
        run_tree<RUN, NV>(T.run, out, term);
        return;
    }
    const int lane = threadIdx.x & 63;
    double st[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) st[k] = 0.0;
    for (int c = 0; c < T.run; c++) {
        term(c, out);
        for (int l = 0; l < 6; l++) {
#pragma unroll
            for (int k = 0; k < NV; k++) out[k] = wave_level_add(out[k], l);
        }
        int lvl = 0;
        for (int m = c; m & 1; m >>= 1, lvl++) {
#pragma unroll
            for (int k = 0; k < NV; k++) out[k] = readlane_f64(st[k], lvl) + out[k];
        }
        if (c + 1 < T.run && lane == lvl) {
#pragma unroll
            for (int k = 0; k < NV; k++) st[k] = out[k];
        }
    }
}

template <int RUN>
__device__ __forceinline__ void initial_ba_run(const BaArgs& G, BaShared& S, const TreeShape& T)
{
    constexpr int NR = RUN > 0 ? RUN : 1;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool huber = G.huber != 0;
    const size_t P = (size_t)G.P;
    BaPoint Lr[NR];
    double Xr[NR][3], Xt[NR][3];
    // the point this thread takes as item k of its run (RUN > 0) or of its wave's chunk k (RUN = 0)
    auto index = [&](int k) -> int { return RUN > 0 ? tid * RUN + k : (wave * T.run + k) * 64 + lane; };
    auto load_obs = [&](int p) -> BaObs {
        const float* o = G.obs + (size_t)p * 6;
        return BaObs{(double)o[0], (double)o[1], (double)o[2], (double)o[3], (double)o[4], (double)o[5]};
    };
    auto get_lin = [&](int k, int p, BaPoint& L) {
        if (RUN > 0) {
            L = Lr[k];
            return;
        }
        const double* q = G.park + p;
#pragma unroll
        for (int i = 0; i < 6; i++) L.Hpp[i] = q[(size_t)i * P];
#pragma unroll
        for (int i = 0; i < 3; i++) L.bp[i] = q[(size_t)(6 + i) * P];
#pragma unroll
        for (int i = 0; i < 18; i++) L.Hxp[i] = q[(size_t)(9 + i) * P];
    };
    auto put_lin = [&](int k, int p, const BaPoint& L) {
        if (RUN > 0) {
            Lr[k] = L;
            return;
        }
        double* q = G.park + p;
#pragma unroll
        for (int i = 0; i < 6; i++) q[(size_t)i * P] = L.Hpp[i];
#pragma unroll
        for (int i = 0; i < 3; i++) q[(size_t)(6 + i) * P] = L.bp[i];
#pragma unroll
        for (int i = 0; i < 18; i++) q[(size_t)(9 + i) * P] = L.Hxp[i];
    };
    // slot 0: the point's position, slot 1: its position in the trial
    auto get_x = [&](int slot, int k, int p, double (&X)[3]) {
#pragma unroll
        for (int i = 0; i < 3; i++) X[i] = RUN > 0 ? (slot ? Xt[k][i] : Xr[k][i]) : G.park[(size_t)(kBaNL + 3 * slot + i) * P + p];
    };
    auto put_x = [&](int slot, int k, int p, const double (&X)[3]) {
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (RUN > 0) (slot ? Xt[k][i] : Xr[k][i]) = X[i];
            else G.park[(size_t)(kBaNL + 3 * slot + i) * P + p] = X[i];
        }
    };
    // f(k, p) for every point of this thread, k a compile-time value when RUN > 0
    auto each_point = [&](auto f) {
        if (RUN > 0) {
#pragma unroll
            for (int k = 0; k < NR; k++)
                if (index(k) < G.N) f(k, index(k));
        } else {
            for (int k = 0; k < T.run; k++)
                if (index(k) < G.N) f(k, index(k));
        }
    };
#pragma unroll
    for (int k = 0; k < NR; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            Xr[k][i] = 0.0;
            Xt[k][i] = 0.0;
        }
    each_point([&](int k, int p) {
        const double X[3] = {(double)G.x0[3 * (size_t)p], (double)G.x0[3 * (size_t)p + 1], (double)G.x0[3 * (size_t)p + 2]};
        put_x(0, k, p, X);
    });

    int flip = 0;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = G.R0[i];
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = G.t0[i];
    double lam = 0.0, ni = 2.0, cur = 0.0;
    int nIt = 0, nTr = 0, exitKind = ORBFE_POSE_OPT_EXIT_RAN_ALL;
    for (int it = 0; it < G.iterations; it++) {
        nIt++;
        double acc[kNV + 1];
        {
            double sum[kNV], mx = 0.0;
            ba_run_tree<RUN, kNV>(T, sum, [&](int k, double (&v)[kNV]) {
                const int p = index(k);
                if (p < G.N) {
                    double X[3];
                    BaPoint L;
                    get_x(0, k, p, X);
                    ba_build(G.cam, load_obs(p), G.Ra, G.ta, R, t, X, huber, L, v);
                    put_lin(k, p, L);
                    mx = ba_diag_max(L, mx);
                } else {
#pragma unroll
                    for (int q = 0; q < kNV; q++) v[q] = 0.0;
                }
            });
#pragma unroll
            for (int q = 0; q < kNV; q++) acc[q] = sum[q];
            acc[kNV] = mx;
        }
        block_tree<kNV, 1>(S, T, flip, acc);   // 28 sums and the maximum behind lambda_0 in one exchange
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
                if (diag[j] > m) m = diag[j];
            if (acc[kNV] > m) m = acc[kNV];
            lam = 1e-5 * m;
            ni = 2.0;
        }
        double rho = 0.0;
        int q = 0;
        while (q < kBaTrials) {
            double sc[kBaNS];
            ba_run_tree<RUN, kBaNS>(T, sc, [&](int k, double (&v)[kBaNS]) {
                const int p = index(k);
                if (p < G.N) {
                    BaPoint L;
                    get_lin(k, p, L);
                    ba_schur(L, lam, v);
                } else {
#pragma unroll
                    for (int i = 0; i < kBaNS; i++) v[i] = 0.0;
                }
            });
            block_tree<kBaNS>(S, T, flip, sc);
            double A[6][6], g[6], dx[6];
            {
                int at = 0;
#pragma unroll
                for (int j = 0; j < 6; j++)
#pragma unroll
                    for (int k = j; k < 6; k++) {
                        const double val = j == k ? (diag[j] + lam) - sc[at] : acc[at] - sc[at];
                        A[j][k] = val;
                        A[k][j] = val;
                        at++;
                    }
#pragma unroll
                for (int j = 0; j < 6; j++) g[j] = b[j] - sc[21 + j];
            }
            bool ok;
            ldlt_solve6(A, g, dx, &ok);
            double Rn[9], tn[3];
            apply_update(dx, R, t, Rn, tn);
            double tr[kBaNT];
            ba_run_tree<RUN, kBaNT>(T, tr, [&](int k, double (&v)[kBaNT]) {
                const int p = index(k);
                v[0] = 0.0;
                v[1] = 0.0;
                if (p < G.N) {
                    BaPoint L;
                    double X[3], dp[3];
                    get_lin(k, p, L);
                    get_x(0, k, p, X);
                    ba_backsub(L, lam, dx, dp, v[1]);
                    const double Xn[3] = {X[0] + dp[0], X[1] + dp[1], X[2] + dp[2]};
                    put_x(1, k, p, Xn);
                    v[0] = ba_cost(G.cam, load_obs(p), G.Ra, G.ta, Rn, tn, Xn, huber);
                }
            });
            block_tree<kBaNT>(S, T, flip, tr);
            double tmp = tr[0];
            if (!ok) tmp = DBL_MAX;
            double scale = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) scale = scale + dx[j] * ((lam * dx[j]) + b[j]);
            scale = (scale + tr[1]) + 1e-3;
            rho = (cur - tmp) / scale;
            nTr++;
            q++;
            if (rho > 0.0 && fabs(tmp) <= DBL_MAX) {
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = Rn[i];
#pragma unroll
                for (int i = 0; i < 3; i++) t[i] = tn[i];
                each_point([&](int k, int p) {   // a thread reads and writes its own points only: no barrier
                    double X[3];
                    get_x(1, k, p, X);
                    put_x(0, k, p, X);
                });
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
        if (tid == 0) {
            G.info->trials[it] = q;
            G.info->cost[it] = cur;
            G.info->lambda[it] = lam;
        }
        if (q == kBaTrials) { exitKind = ORBFE_POSE_OPT_EXIT_TRIALS; break; }
        if (rho == 0.0) { exitKind = ORBFE_POSE_OPT_EXIT_RHO_ZERO; break; }
    }
    each_point([&](int k, int p) {
        double X[3], chiA, chiB;
        bool fa, fb;
        get_x(0, k, p, X);
        ba_chi2(G.cam, load_obs(p), G.Ra, G.ta, R, t, X, chiA, chiB, fa, fb);
        G.chi2[p] = chiA;
        G.chi2[(size_t)G.N + p] = chiB;
        G.front[p] = fa ? 1 : 0;
        G.front[(size_t)G.N + p] = fb ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 3; i++) G.xOut[3 * (size_t)p + i] = (float)X[i];
    });
    if (tid == 0) {
        BaDeviceInfo& I = *G.info;
        I.nIterations = nIt;
        I.nTrials = nTr;
        I.exitKind = exitKind;
        for (int i = 0; i < 9; i++) I.pose[i] = R[i];
        for (int i = 0; i < 3; i++) I.pose[9 + i] = t[i];
    }
}

__global__ __launch_bounds__(kTreeThreads) void initial_ba_kernel(BaArgs G)
{
    __shared__ BaShared S;
    const int nT = blockDim.x;
    int lg = 0;
    while ((1 << lg) < G.P) lg++;
    TreeShape T;
    if (G.P > kBaRegisterP) {   // the waves walk chunks: the six wave levels are taken per chunk, inside ba_run_tree
        T.run = G.P / kTreeThreads;
        T.lvWave = 0;
        T.lvCross = 2;
        initial_ba_run<0>(G, S, T);
        return;
    }
    T.run = G.P > nT ? G.P / nT : 1;
    int lgRun = 0;
    while ((1 << lgRun) < T.run) lgRun++;
    const int lgThreads = lg - lgRun;   // log2 of the threads that own points
    T.lvWave = lgThreads < 6 ? lgThreads : 6;
    T.lvCross = lgThreads - T.lvWave;
    if (T.run == 1) initial_ba_run<1>(G, S, T);
    else initial_ba_run<2>(G, S, T);
}

constexpr char kBaSizeErr[] =
    "orbfe_initial_ba_params / orbfe_initial_ba_info struct_size does not match this library (rebuild the caller against include/orbfe.h)";

}  // namespace

// struct sizes, the unsupported branches and the ranges: no device is touched
int initial_ba_check(const orbfe_initial_ba_params* P, const orbfe_initial_ba_info* info, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_initial_ba_params) || (info && info->struct_size != (int)sizeof(orbfe_initial_ba_info))) {
        err = kBaSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    static_assert(kBaMaxIterations == 64, "solver_check_common's range");
    const int rc = solver_check_common(P, "orbfe_initial_bundle_adjustment", "edges of BundleAdjustment are", "S17", err);
    if (rc != ORBFE_OK) return rc;
    if (P->robust != 0 && P->robust != 1) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// Everything of the call that needs no device: the refusals, the point list, the outputs of a call that runs nothing.
int initial_ba_begin(const orbfe_initial_ba_params* P, int nLevels, int n1, const orbfe_keypoint* kp1, int n2, const orbfe_keypoint* kp2,
                     const int* matches12, const float* points, const float* Rcw2, const float* tcw2, float* TcwOut, float* pointsOut,
                     orbfe_initial_ba_info* info, std::vector<int>& first, std::string& err)
{
    const int crc = initial_ba_check(P, info, err);
    if (crc != ORBFE_OK) return crc;
    if (n1 > kBaMaxKp || n2 > kBaMaxKp) return ORBFE_ERR_INVALID_ARG;
    first.clear();
    for (int i = 0; i < n1; i++) {
        const int m = matches12[i];
        if (m < 0) continue;
        if (m >= n2 || kp1[i].octave < 0 || kp1[i].octave >= nLevels || kp2[m].octave < 0 || kp2[m].octave >= nLevels)
            return ORBFE_ERR_INVALID_ARG;
        first.push_back(i);
    }
    fill_tcw(Rcw2, tcw2, TcwOut);
    if (n1 > 0 && pointsOut != points) memmove(pointsOut, points, (size_t)n1 * 3 * sizeof(float));
    if (info) {
        double* chi2 = info->chi2;
        uint8_t* front = info->depth_positive;
        memset(info, 0, sizeof *info);
        info->struct_size = (int)sizeof(orbfe_initial_ba_info);
        info->chi2 = chi2;
        info->depth_positive = front;
        info->N = (int)first.size();
        for (int i = 0; i < 9; i++) info->pose[i] = (double)Rcw2[i];
        for (int i = 0; i < 3; i++) info->pose[9 + i] = (double)tcw2[i];
    }
    return ORBFE_OK;
}

// the device part of the call, for the point list `first` (>= 1 entry) of initial_ba_begin
int initial_ba_run_host(MatchScratch& m, hipStream_t s, const orbfe_initial_ba_params* P, const float* invLevelSigma2,
                        const orbfe_keypoint* kp1, const orbfe_keypoint* kp2, const int* matches12, const float* points, const float* Rcw1,
                        const float* tcw1, const float* Rcw2, const float* tcw2, const std::vector<int>& first, float* TcwOut,
                        float* pointsOut, orbfe_initial_ba_info* info, std::string& err)
{
    const int N = (int)first.size();
    if (N < 1) return ORBFE_ERR_INVALID_ARG;
    int Pw = 1;
    while (Pw < N) Pw <<= 1;
    const bool parked = Pw > kBaRegisterP;

    // up: [obs | x0]; device only: [park]; down: [info | xOut | chi2 | front]
    Staging st;
    const auto bObs = st.in<float>((size_t)N * 6);
    const auto bX0 = st.in<float>((size_t)N * 3);
    const auto bPark = st.scratch<double>(parked ? (size_t)kBaState * Pw : 0);
    const auto bInfo = st.out<BaDeviceInfo>(1);
    const auto bXOut = st.out<float>((size_t)N * 3);
    const auto bChi2 = st.out<double>((size_t)2 * N);
    const auto bFront = st.out<uint8_t>((size_t)2 * N);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    float* hObs = st.host(bObs);
    float* hX0 = st.host(bX0);
    for (int p = 0; p < N; p++) {
        const int i = first[(size_t)p];
        const orbfe_keypoint& a = kp1[i];
        const orbfe_keypoint& b = kp2[matches12[i]];
        float* o = hObs + 6 * (size_t)p;
        o[0] = a.x;
        o[1] = a.y;
        o[2] = invLevelSigma2[a.octave];
        o[3] = b.x;
        o[4] = b.y;
        o[5] = invLevelSigma2[b.octave];
        for (int k = 0; k < 3; k++) hX0[3 * (size_t)p + k] = points[3 * (size_t)i + k];
    }
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    MCHK(hipMemsetAsync(st.dev(bInfo), 0, sizeof(BaDeviceInfo), s));

    BaArgs G;
    memset(&G, 0, sizeof G);
    G.N = N;
    G.P = Pw;
    G.obs = st.dev(bObs);
    G.x0 = st.dev(bX0);
    G.park = parked ? st.dev(bPark) : nullptr;
    G.xOut = st.dev(bXOut);
    G.chi2 = st.dev(bChi2);
    G.front = st.dev(bFront);
    G.info = st.dev(bInfo);
    for (int i = 0; i < 9; i++) {
        G.Ra[i] = (double)Rcw1[i];
        G.R0[i] = (double)Rcw2[i];
    }
    for (int i = 0; i < 3; i++) {
        G.ta[i] = (double)tcw1[i];
        G.t0[i] = (double)tcw2[i];
    }
    fill_pose_cam(G.cam, P->cam, P->huber_delta2);
    G.iterations = P->iterations;
    G.huber = P->robust;
    hipLaunchKernelGGL(initial_ba_kernel, dim3(1), dim3(Pw <= 64 ? 64 : kTreeThreads), 0, s, G);
    if ((rc = download(st, s, err)) != ORBFE_OK) return rc;
    const BaDeviceInfo* I = st.res(bInfo);
    const float* xOut = st.res(bXOut);
    fill_tcw(I->pose, I->pose + 9, TcwOut);
    for (int p = 0; p < N; p++)
        for (int k = 0; k < 3; k++) pointsOut[3 * (size_t)first[(size_t)p] + k] = xOut[3 * (size_t)p + k];
    if (info) {
        info->n_iterations = I->nIterations;
        info->n_trials = I->nTrials;
        info->exit_kind = I->exitKind;
        memcpy(info->trials, I->trials, sizeof I->trials);
        memcpy(info->cost, I->cost, sizeof I->cost);
        memcpy(info->lambda, I->lambda, sizeof I->lambda);
        memcpy(info->pose, I->pose, sizeof I->pose);
        st.get(bChi2, info->chi2);
        st.get(bFront, info->depth_positive);
    }
    return ORBFE_OK;
}

}  // namespace orbfe

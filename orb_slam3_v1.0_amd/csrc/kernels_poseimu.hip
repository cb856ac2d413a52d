// kernels_poseimu.hip -- Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:3447-3844; the call: src/Tracking.cc:952)
// on gfx950 for the branch this fork takes: one pinhole camera, EdgeMonoOnlyPose (src/G2oTypes.cc:375-395), one EdgeInertial
// (:514-594) against the fixed last key frame, EdgeGyroRW and EdgeAccRW; 15 unknowns.
//
// SPEC DECISION S19: S14's rules -- binary64 where the C++ is double, one operation per operator, no
// contraction, every sum over mono edges the fixed pairwise tree over P = the smallest power of two >= N_e -- and a Gauss-Newton loop
// restated from g2o's published algorithm: build, solve H dx = b by L D L^T with diagonal pivoting, stop the round when a pivot is
// not positive, else update.  tests/pose_inertial_ref.py is the normative restatement; every byte this file produces is compared
// with it.  What one thread computes (poseimu_math.h) is host-safe text that tests/cpp/pose_inertial.cpp includes; this file holds
// the mapping, the wave form of the 15 x 15 solve, the loop and the host calls.
//
// pose_imu_kernel: ONE block of kTreeThreads per frame runs the whole call -- the compaction of the matched keypoints into edges,
// four rounds, every iteration, the scoring, the recovery and the Hessian -- with no host step and no second launch.
//   Mapping of the tree: item e = (wave * run + c) * 64 + lane.  P <= 256: run = 1, thread t takes edge t; the levels inside the
//   wave and across the waves are block_tree's.  P >= 512: S17's wave-walked run (wave_run_tree of block_tree.h) -- wave w owns the
//   aligned run of P / 256 chunks of 64 consecutive edges, the chunk is summed by the six wave levels and the chunk sums are combined by
//   a binary counter whose stack level j lives in lane j's registers.  No thread owns a run, so nothing needs a dynamically indexed stack: no scratch
//   memory.  An edge is read back from L2 whenever it is needed (24 + 16 bytes); its flag lives in the output array, which only the
//   lane that takes the edge reads and writes.
//   The 15 x 15 solve is mapped onto one wave (wave_ldlt15) and every wave runs it redundantly on the same sums, so no result is
//   passed between waves except through the tree; every thread then holds dx and updates its copy of the state.
// Every loop has a static trip bound (rounds <= 4, iterations <= 64, chunks <= 256, counter levels <= 8, the fixed steps of the
// solve); NaN follows the comparisons as written: a non-finite system has a pivot that is not > 0 and ends the round.
#include <cstring>
#include <vector>

#include "match_common.h"
#include "block_tree.h"
#include "poseimu_math.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

struct PoseImuRounds {   // what the kernel reports per call (host call only)
    int Ne, roundsRun, recovered, pad;
    int iterations[4], ok[4], nBad[4];
    double state[4][kImuState];
};

struct PoseImuArgs {
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
    const orbfe_imu_link* link;  // [batch]
    const float* stateIn;        // [batch][33]
    float* stateOut;             // [batch][21]
    double* Hout;                // [batch][225]
    uint8_t* outlier;            // [batch][kpStride]
    int* nInliers;               // [batch]
    int* edgeIdx;                // [batch][kpStride] scratch: edge -> keypoint
    PoseImuRounds* rounds;       // nullable
    uint8_t* roundOutlier;       // nullable, [4][N_e]
    PoseCam cam;
    double gravity;
    float chi2[4], chi2Close[4];
    float closeDepth, recoverChi2;
    int recoverBelow, recInit, iterations, nRounds, nLevels;
    float invSigma2[kMaxLevels];
};

struct PoseImuShared {
    double part[2][kTreeMaxWaves][kNV];
    int waveCount[kTreeMaxWaves];
};

struct ImuFrameView {
    const orbfe_keypoint* kp;
    const int* match;
    const float* pts;
    const float* depth;
    const int* edgeIdx;
    uint8_t* outlier;
    int Ne;
};

__device__ __forceinline__ EdgeD load_edge(const PoseImuArgs& G, const ImuFrameView& F, int c, int& kpIndex, float& depth)
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

// The part of a sum below block_tree's exchange.  run = 1: the thread's one item.  run > 1: the wave's run of chunks.
template <int NV, class Term>
__device__ __forceinline__ void imu_run_tree(const TreeShape& T, double (&out)[NV], Term term)
{
    if (T.run == 1) term(0, out);
    else wave_run_tree<NV>(T.run, out, term);
}

// row `lane` of the 15 x 15 matrix of imu_system (lanes >= 15: zeros); every register index is a compile-time one
__device__ __forceinline__ void lane_row(const orbfe_imu_link& K, const double (&H9)[45], int lane, double (&a)[kImuN])
{
#pragma unroll
    for (int j = 0; j < kImuN; j++) {
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < kImuN; i++) {
            const int bi = i < 9 ? 0 : (i < 12 ? 1 : 2), bj = j < 9 ? 0 : (j < 12 ? 1 : 2);
            if (bi == bj) v = lane == i ? imu_entry(K, H9, i, j) : v;
        }
        a[j] = v;
    }
}

// v[idx] for a per-lane idx (0.0 for idx >= 15) with compile-time register indices: the bit patterns of the candidates are masked
// and or-ed.  (A chain of selects between the elements is rewritten by the compiler into one load through a selected address,
// which puts the array into scratch memory.)
__device__ __forceinline__ double pick15(const double (&v)[kImuN], int idx)
{
    unsigned long long u = 0ull;
#pragma unroll
    for (int j = 0; j < kImuN; j++) u |= idx == j ? (unsigned long long)__double_as_longlong(v[j]) : 0ull;
    return __longlong_as_double((long long)u);
}

// A x = b for the symmetric 15 x 15 A on one wave, all 64 lanes active: ldlt_solve_n<15> (ldlt.h) operation for operation.
// Lane i < 15 owns row i of A (a[], destroyed) and of L; b and x are wave-uniform.  At step k the pivot search reads the diagonal
// of lanes k .. 14 in order and keeps the first of equals ('>'); rows k and `best` are exchanged through lane reads with the
// wave-uniform index `best` (of A the columns >= k, of L the columns < k: the others are never read again, resp. still zero), the
// two columns by selects; d_k is broadcast from lane k and the pivot column col_j = A[j][k] and l_j from lane j.  Entry (i, j) of the
// trailing block is A_ij - l_i col_j for j <= i, as in the indexed text; lane i also keeps the mirror A_ij = A_ji - l_j col_i for
// j > i, the value the indexed text stores there.  The substitutions keep each sum in the indexed text's order: lane i subtracts
// l_ij z_j for j = 0 .. i - 1 in turn and z_i is read from it; the back substitution reads L's column from the lanes.
__device__ __forceinline__ void wave_ldlt15(int lane, double (&a)[kImuN], const double (&b)[kImuN], double (&x)[kImuN], bool& positive)
{
    constexpr int N = kImuN;
    double l[N], d[N];
    int p = lane;   // perm[lane]
#pragma unroll
    for (int j = 0; j < N; j++) l[j] = 0.0;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const double ad = fabs(pick15(a, lane));   // |A[lane][lane]|
        int best = k;
        double bestAbs = readlane_f64(ad, k);
#pragma unroll
        for (int i = k + 1; i < N; i++) {
            const double v = readlane_f64(ad, i);
            if (v > bestAbs) { best = i; bestAbs = v; }
        }
        best = __builtin_amdgcn_readfirstlane(best);
        if (best != k) {   // wave-uniform
#pragma unroll
            for (int j = k; j < N; j++) {
                const double fromBest = readlane_f64(a[j], best), fromK = readlane_f64(a[j], k);
                a[j] = lane == k ? fromBest : (lane == best ? fromK : a[j]);
            }
#pragma unroll
            for (int j = 0; j < k; j++) {
                const double fromBest = readlane_f64(l[j], best), fromK = readlane_f64(l[j], k);
                l[j] = lane == k ? fromBest : (lane == best ? fromK : l[j]);
            }
            const int pBest = __builtin_amdgcn_readlane(p, best), pK = __builtin_amdgcn_readlane(p, k);
            p = lane == k ? pBest : (lane == best ? pK : p);
#pragma unroll
            for (int i = k + 1; i < N; i++) {
                const bool sw = best == i;
                const double ak = a[k], ai = a[i];
                a[k] = sw ? ai : ak;
                a[i] = sw ? ak : ai;
            }
        }
        const double dk = readlane_f64(a[k], k);
        d[k] = dk;
        const double colMine = a[k];   // A[lane][k]
        const double li = dk == 0.0 ? 0.0 : colMine / dk;
        const bool below = lane > k;
        l[k] = below ? li : l[k];
#pragma unroll
        for (int j = k + 1; j < N; j++) {
            const double colJ = readlane_f64(colMine, j), lJ = readlane_f64(li, j);
            const bool mine = j <= lane;
            const double f = mine ? li : lJ, g = mine ? colJ : colMine;
            const double val = a[j] - f * g;
            a[j] = below ? val : a[j];
        }
    }
    const double bp = pick15(b, p);   // b[perm[lane]]
    double z[N], xs[N];
    {
        double acc = bp;
#pragma unroll
        for (int i = 0; i < N; i++) {
            z[i] = readlane_f64(acc, i);
            acc = acc - l[i] * z[i];
        }
    }
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double acc = d[i] == 0.0 ? 0.0 : z[i] / d[i];
#pragma unroll
        for (int j = i + 1; j < N; j++) acc = acc - readlane_f64(l[i], j) * xs[j];
        xs[i] = acc;
    }
    int perm[N];
#pragma unroll
    for (int i = 0; i < N; i++) perm[i] = __builtin_amdgcn_readlane(p, i);
#pragma unroll
    for (int j = 0; j < N; j++) {   // x[perm[i]] = xs[i]
        double v = xs[0];
#pragma unroll
        for (int i = 1; i < N; i++) v = perm[i] == j ? xs[i] : v;
        x[j] = v;
    }
    bool pos = true;
#pragma unroll
    for (int i = 0; i < N; i++) pos = pos && d[i] > 0.0;
    positive = pos;
}

__device__ __forceinline__ void pose_imu_frame(const PoseImuArgs& G, PoseImuShared& Sh, const TreeShape& T, const ImuFrameView& F,
                               const orbfe_imu_link& K, int frame)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    ImuState S;
    {
        const float* in = G.stateIn + (size_t)frame * kImuStateIn;
#pragma unroll
        for (int i = 0; i < 9; i++) S.Rcw[i] = (double)in[i];
#pragma unroll
        for (int i = 0; i < 3; i++) S.tcw[i] = (double)in[9 + i];
#pragma unroll
        for (int i = 0; i < 9; i++) S.Rwb[i] = (double)in[12 + i];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            S.twb[i] = (double)in[21 + i];
            S.v[i] = (double)in[24 + i];
            S.bg[i] = (double)in[27 + i];
            S.ba[i] = (double)in[30 + i];
        }
    }
    double Rcb[9], tbc[3];
#pragma unroll
    for (int i = 0; i < 9; i++) Rcb[i] = (double)K.Rcb[i];
#pragma unroll
    for (int i = 0; i < 3; i++) tbc[i] = (double)K.tbc[i];
    auto item = [&](int c) -> int { return (wave * T.run + c) * 64 + lane; };
    // the 28 sums over the edges whose flag is clear
    auto mono_sums = [&](bool huber, double (&acc)[kNV], int& flip) {
        imu_run_tree<kNV>(T, acc, [&](int c, double (&v)[kNV]) {
            const int e = item(c);
            bool on = e < F.Ne;
            EdgeD E = EdgeD{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (on) {
                int ki;
                float dep;
                E = load_edge(G, F, e, ki, dep);
                on = F.outlier[ki] == 0;
            }
            if (on) imu_edge_terms(G.cam, E, S.Rcw, S.tcw, Rcb, tbc, huber, v);
            else {
#pragma unroll
                for (int q = 0; q < kNV; q++) v[q] = 0.0;
            }
        });
        block_tree<kNV>(Sh, T, flip, acc);
    };
    int flip = 0, nBadLast = 0, roundsRun = 0;
    for (int rnd = 0; rnd < G.nRounds; rnd++) {
        const bool huber = rnd <= 2;   // (:3717-3718)
        int nIt = 0;
        bool ok = true;
        for (int it = 0; it < G.iterations; it++) {
            nIt++;
            double acc[kNV], H9[45], b[kImuN], a[kImuN], dx[kImuN];
            mono_sums(huber, acc, flip);
            imu_system(K, G.gravity, S, acc, H9, b);
            lane_row(K, H9, lane, a);
            wave_ldlt15(lane, a, b, dx, ok);
            if (!ok) break;   // the same bits in every thread: all leave or none
            imu_update(K, dx, S);
        }
        // the flags of the round on fresh errors at its final state (:3680-3715; S19)
        const float thr = G.chi2[rnd], thrClose = G.chi2Close[rnd];
        double bad[1];
        imu_run_tree<1>(T, bad, [&](int c, double (&v)[1]) {
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
        nBadLast = (int)bad[0];
        roundsRun = rnd + 1;
        if (G.rounds && tid == 0) {
            PoseImuRounds& I = *G.rounds;
            I.iterations[rnd] = nIt;
            I.ok[rnd] = ok ? 1 : 0;
            I.nBad[rnd] = nBadLast;
#pragma unroll
            for (int i = 0; i < 9; i++) I.state[rnd][i] = S.Rwb[i];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                I.state[rnd][9 + i] = S.twb[i];
                I.state[rnd][12 + i] = S.v[i];
                I.state[rnd][15 + i] = S.bg[i];
                I.state[rnd][18 + i] = S.ba[i];
            }
        }
        if (F.Ne + 3 < 10) break;   // optimizer.edges().size() < 10 (:3757)
    }
    int recovered = 0;
    if (F.Ne - nBadLast < G.recoverBelow && !G.recInit) {   // (:3765-3792)
        recovered = 1;
        double bad[1];
        imu_run_tree<1>(T, bad, [&](int c, double (&v)[1]) {
            v[0] = 0.0;
            const int e = item(c);
            if (e >= F.Ne) return;
            int ki;
            float dep;
            const EdgeD E = load_edge(G, F, e, ki, dep);
            double x, y, z, e0, e1, chi2;
            edge_residual(G.cam, E, S.Rcw, S.tcw, x, y, z, e0, e1, chi2);
            const bool good = (float)chi2 < G.recoverChi2;
            if (good) F.outlier[ki] = 0;
            v[0] = good ? 0.0 : 1.0;
        });
        block_tree<1>(Sh, T, flip, bad);
        nBadLast = (int)bad[0];
    }
    // the Hessian at the final state (:3800-3837): no robust weight
    double acc[kNV], H9[45], b9[9], e9[9];
    mono_sums(false, acc, flip);
    inertial_edge(K, G.gravity, S, H9, b9, e9);
    if (tid == 0) {
        double* Ho = G.Hout + (size_t)frame * (kImuN * kImuN);
        for (int i = 0; i < kImuN * kImuN; i++) Ho[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 9; i++)
#pragma unroll
            for (int j = i; j < 9; j++) {
                double h = H9[tri9(i, j)];
                if (j < 6) h = h + acc[tri6(i, j)];
                Ho[kImuN * i + j] = h;
                Ho[kImuN * j + i] = h;
            }
#pragma unroll
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                Ho[kImuN * (9 + i) + (9 + j)] = K.infoG[3 * i + j];
                Ho[kImuN * (12 + i) + (12 + j)] = K.infoA[3 * i + j];
            }
        float* o = G.stateOut + (size_t)frame * kImuState;
#pragma unroll
        for (int i = 0; i < 9; i++) o[i] = (float)S.Rwb[i];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            o[9 + i] = (float)S.twb[i];
            o[12 + i] = (float)S.v[i];
            o[15 + i] = (float)S.bg[i];
            o[18 + i] = (float)S.ba[i];
        }
        G.nInliers[frame] = F.Ne - nBadLast;
        if (G.rounds) {
            G.rounds->Ne = F.Ne;
            G.rounds->roundsRun = roundsRun;
            G.rounds->recovered = recovered;
        }
    }
}

__global__ __launch_bounds__(kTreeThreads) void pose_imu_kernel(PoseImuArgs G)
{
    __shared__ PoseImuShared S;
    const int frame = blockIdx.x, tid = threadIdx.x, nT = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63, nWaves = nT >> 6;
    int n = G.dN ? G.dN[frame] : G.nSingle;
    n = n < 0 ? 0 : (n > G.kpStride ? G.kpStride : n);
    const size_t base = (size_t)frame * G.kpStride;
    ImuFrameView F;
    F.kp = G.kp + base;
    F.match = G.match + base;
    F.pts = G.pts + (size_t)frame * G.ptFrameStride * G.ptRec;
    F.depth = G.depth + (size_t)frame * G.ptFrameStride;
    F.outlier = G.outlier + base;
    int* edgeIdx = G.edgeIdx + base;
    F.edgeIdx = edgeIdx;
    // edges = the matched keypoints in keypoint order: each thread counts a contiguous chunk, the counts are scanned, the indices written
    // (pose_opt_kernel's prologue, repeated: as a shared function it re-numbers both kernels' registers and moved their times, r20)
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
    if (P > kTreeThreads) {   // the waves walk chunks: the six wave levels are taken per chunk, inside imu_run_tree
        T.run = P / kTreeThreads;
        T.lvWave = 0;
        T.lvCross = 2;
    } else {
        T.run = 1;
        T.lvWave = lg < 6 ? lg : 6;
        T.lvCross = lg - T.lvWave;
    }
    pose_imu_frame(G, S, T, F, G.link[frame], frame);
}

constexpr char kPoseImuSizeErr[] =
    "orbfe_pose_inertial_params / orbfe_imu_link / orbfe_pose_inertial_info struct_size does not match this library (rebuild the caller "
    "against include/orbfe.h)";

void fill_args(PoseImuArgs& G, const orbfe_pose_inertial_params* P, const float* invLevelSigma2, int nLevels)
{
    fill_inertial_args(G, G, P, invLevelSigma2, nLevels);
}

}  // namespace

// struct sizes, the unsupported branches and the ranges: no device is touched
int pose_imu_check(const orbfe_pose_inertial_params* P, const orbfe_imu_link* link, const orbfe_pose_inertial_info* info, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_pose_inertial_params) || (link && link->struct_size != (int)sizeof(orbfe_imu_link)) ||
        (info && info->struct_size != (int)sizeof(orbfe_pose_inertial_info))) {
        err = kPoseImuSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    const int rc = solver_check_common(P, "orbfe_pose_inertial_optimization", "branch of PoseInertialOptimizationLastKeyFrame is", "S19", err);
    if (rc != ORBFE_OK) return rc;
    if (P->rounds < 1 || P->rounds > 4 || !(P->close_factor >= 0.0) || P->recover_below < 0) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++)
        if (!(P->chi2[i] >= 0.0f)) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// Everything of the host call that needs no device: the refusals and the edge list.
int pose_imu_begin(const orbfe_pose_inertial_params* P, const orbfe_imu_link* link, int nLevels, int n, const orbfe_keypoint* kp,
                   const int* mpIndex, int nPoints, orbfe_pose_inertial_info* info, std::vector<int>& first, std::string& err)
{
    const int crc = pose_imu_check(P, link, info, err);
    if (crc != ORBFE_OK) return crc;
    return pose_edge_list(nLevels, n, kp, mpIndex, nPoints, first);
}

// the device part of the host call, for the edge list `first` of pose_imu_begin (it may be empty)
int pose_imu_run(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_params* P, const orbfe_imu_link* link,
                 const float* invLevelSigma2, int nLevels, int n, const orbfe_keypoint* kp, const int* mpIndex, const float* points,
                 const float* trackDepth, const float* stateIn, const std::vector<int>& first, float* stateOut, double* Hout,
                 uint8_t* outlier, int* nInliers, orbfe_pose_inertial_info* info, std::string& err)
{
    // the unit's blocks (EdgeStaging, match_common.h): up [state | link]; down [state | nInliers | rounds | H]
    EdgeStaging st(n, first, trackDepth);
    const auto bState = st.in<float>(kImuStateIn);
    const auto bLink = st.in<orbfe_imu_link>(1);
    st.inputs_done();
    const auto bStateOut = st.out<float>(kImuState);
    const auto bNInl = st.out<int>(1);
    const auto bRounds = st.out<PoseImuRounds>(1);
    const auto bH = st.out<double>(kImuN * kImuN);
    int rc = st.stage(m, kp, first, mpIndex, points, trackDepth, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bState, stateIn);
    st.put(bLink, link);
    rc = st.upload(s, bRounds, err);
    if (rc != ORBFE_OK) return rc;

    PoseImuArgs G;
    fill_args(G, P, invLevelSigma2, nLevels);
    st.set_args(G, bNInl, bRounds);
    G.depth = st.dev(st.bDepth);
    G.link = st.dev(bLink);
    G.stateIn = st.dev(bState);
    G.stateOut = st.dev(bStateOut);
    G.Hout = st.dev(bH);
    hipLaunchKernelGGL(pose_imu_kernel, dim3(1), dim3(kTreeThreads), 0, s, G);
    rc = st.download(s, outlier, err);
    if (rc != ORBFE_OK) return rc;
    st.get(bStateOut, stateOut);
    *nInliers = *st.res(bNInl);
    st.get(bH, Hout);
    if (info) fill_inertial_info(info, st.res(bRounds), st);
    return ORBFE_OK;
}

int pose_imu_batch_device(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_params* P, const float* invLevelSigma2, int nLevels,
                          int batch, const orbfe_imu_link* dLinks, const orbfe_keypoint* dKp, const int* dN, int kpStride,
                          const int* dMatch, int nMapPoints, const orbfe_world_point* dPoints, int pointStrideFrames,
                          const float* dTrackDepth, const float* dStateIn, float* dStateOut, double* dHout, uint8_t* dOutlier,
                          int* dNInliers, std::string& err)
{
    const int crc = pose_imu_check(P, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return crc;
    if (kpStride > kPoseMaxKp) return ORBFE_ERR_INVALID_ARG;
    int rc = ensure(m, (size_t)batch * kpStride * sizeof(int), 0, err);
    if (rc != ORBFE_OK) return rc;
    PoseImuArgs G;
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
    G.stateIn = dStateIn;
    G.stateOut = dStateOut;
    G.Hout = dHout;
    G.outlier = dOutlier;
    G.nInliers = dNInliers;
    G.edgeIdx = static_cast<int*>(m.d);
    hipLaunchKernelGGL(pose_imu_kernel, dim3(batch), dim3(kTreeThreads), 0, s, G);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

// kernels_mlpnp.hip -- a fresh MLPnPsolver + SetRansacParameters + one iterate() on gfx950 (src/MLPnPsolver.cpp; the call:
// Tracking::TrackReferenceKeyFrame, src/Tracking.cc:838-845).
//
// SPEC DECISION S13: binary64 where the C++ is double, binary32 where it is float, one operation per
// operator, no contraction, every sum sequential from 0.0 in ascending order; the null vector of A^T A by a fixed Jacobi sequence
// (12 sweeps of 11 rounds of 6 disjoint pairs; the planar branch's 9 x 9 by S12's sequence), the 3 x 3 decompositions by the n = 3
// sequence of jacobi.h, sin / cos / acos / cbrt by the sequences of spec_math.h, the Jacobian by the chain rule, the 6 x 6 solve
// by L D L^T with diagonal pivoting (ldlt.h).  tests/mlpnp_ref.py is the normative restatement; every byte this file produces is
// compared with it.  What one thread computes on its own (mat3d.h and the headers above) is host-safe text that tests/cpp/mlpnp.cpp
// includes; this file holds what a team of threads does together.
//
//   mlpnp_prep_kernel        one thread per correspondence: bearing (S10 unproject), its null-space basis, the world point in binary64
//   mlpnp_hypothesis_kernel  one wave per RANSAC hypothesis: computePose (:355-657) on its min-set, CheckInliers (:261-292) over all
//   mlpnp_refine_kernel      one block per hypothesis; a block whose hypothesis is no candidate (a strict prefix maximum among the
//                            qualifying counts) leaves at once, the others run Refine (:294-352): computePose on the inlier set,
//                            CheckInliers.  All candidates are refined speculatively; the host applies "the first success returns".
// One submission, one synchronisation, no host step between the launches.
#include <cstring>
#include <vector>

#include "match_common.h"
#include "camera.h"
#include "jacobi.h"
#include "ldlt.h"
#include "mat3d.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

constexpr int kMlpnpChunk = 64;            // points staged per pass of a sequential sum
constexpr int kMlpnpRefineThreads = 256;
constexpr int kMlpnpMaxWords = 1024;       // inlier mask words a refine block indexes from LDS: N <= 65536

struct MlpnpCorr {   // per correspondence, [N]
    const double* X;     // [N][3] world point
    const double* f;     // [N][3] bearing (x, y, 1)
    const double* nr;    // [N][3] null-space basis
    const double* ns;    // [N][3]
};

struct MlpnpArgs {
    int N, minSet, words, minInliers;
    CamP cam;
    float precision, th2;
    float sigma2[kMaxLevels];
    const float* kp;       // [N][2] (upload)
    const int* octave;     // [N]
    const float* pts;      // [N][3]
    const int* sets;       // [total][minSet]
    double* X; double* f; double* nr; double* ns; float* maxErr;
    double* hypRt;         // [total][12]
    int* hypCount;         // [total]
    int* hypMeta;          // [total][3] planar, GN evaluations, GN exit
    unsigned long long* hypMask;   // [total][words]
    double* candRt;        // [total][12]
    int* candCount;        // [total], -1 = no candidate
    int* candPlanar;       // [total]
    unsigned long long* candMask;  // [total][words]
};

// what a team shares while it computes one pose
struct PoseWork {
    JacobiTeamWork J;
    double rows[2 * kMlpnpChunk][12];
    double acc[48];
    double X6[6][3], f6[6][3];
    unsigned long long maxBits;
    int firstNan;
};

// computePose (:355-657) on the n points indexOf(0 .. n-1) of C, by the whole block sharing W.  Every thread returns the same R (row-major),
// t, planar flag, Gauss-Newton evaluations and exit kind (0: it_cnt == maxIt, 1: :743, 2: :747).
template <class IndexOf>
__device__ inline void compute_pose(PoseWork& W, const MlpnpCorr& C, int n, IndexOf indexOf, double (&Rout)[9], double (&tout)[3],
                                    int& planarOut, int& gnEvals, int& gnExit)
{
    const int tid = threadIdx.x, nth = blockDim.x;
    const int chunks = (n + kMlpnpChunk - 1) / kMlpnpChunk;
    // ---- planarity (:380-388): points3 points3^T, not centred ----
    for (int e = tid; e < 9; e += nth) W.acc[e] = 0.0;
    __syncthreads();
    for (int ch = 0; ch < chunks; ch++) {
        const int base = ch * kMlpnpChunk, cnt = (n - base < kMlpnpChunk ? n - base : kMlpnpChunk);
        for (int t = tid; t < cnt; t += nth) {
            const int idx = indexOf(base + t);
            for (int k = 0; k < 3; k++) W.rows[t][k] = C.X[3 * (size_t)idx + k];
            if (ch == 0 && t < 6)
                for (int k = 0; k < 3; k++) { W.X6[t][k] = C.X[3 * (size_t)idx + k]; W.f6[t][k] = C.f[3 * (size_t)idx + k]; }
        }
        __syncthreads();
        for (int e = tid; e < 9; e += nth) {
            double acc = W.acc[e];
            const int i = e / 3, j = e % 3;
            for (int k = 0; k < cnt; k++) acc = acc + W.rows[k][i] * W.rows[k][j];
            W.acc[e] = acc;
        }
        __syncthreads();
    }
    double eigenRot[9];
    bool planar;
    {
        double G[9], lam[3], E[3][3];
        int order[3];
        for (int e = 0; e < 9; e++) G[e] = W.acc[e];
        eig3_sorted(G, false, lam, E, order);
        double mx = fabs(lam[0]);
        for (int i = 1; i < 3; i++) mx = fabs(lam[i]) > mx ? fabs(lam[i]) : mx;
        int rank = 0;
        for (int i = 0; i < 3; i++) rank += fabs(lam[i]) > kRankTol * mx;
        planar = rank == 2;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) eigenRot[3 * i + j] = E[j][order[i]];
    }
    __syncthreads();  // (W.acc is reused below)
    // ---- A^T A (:437-520) ----
    const int nc = planar ? 9 : 12;
    for (int e = tid; e < nc * nc; e += nth) W.J.M[e / nc][e % nc] = 0.0;
    __syncthreads();
    for (int ch = 0; ch < chunks; ch++) {
        const int base = ch * kMlpnpChunk, cnt = (n - base < kMlpnpChunk ? n - base : kMlpnpChunk);
        for (int t = tid; t < cnt; t += nth) {
            const int idx = indexOf(base + t);
            const double* X = C.X + 3 * (size_t)idx;
            for (int h = 0; h < 2; h++) {
                const double* nv = (h ? C.ns : C.nr) + 3 * (size_t)idx;
                double* row = W.rows[2 * t + h];
                if (!planar) {
                    for (int i = 0; i < 3; i++) {
                        for (int j = 0; j < 3; j++) row[3 * i + j] = nv[i] * X[j];
                        row[9 + i] = nv[i];
                    }
                } else {
                    double P3[3];
                    matvec3(eigenRot, X, P3);  // (:396-397)
                    for (int i = 0; i < 3; i++) {
                        row[2 * i] = nv[i] * P3[1];
                        row[2 * i + 1] = nv[i] * P3[2];
                        row[6 + i] = nv[i];
                    }
                }
            }
        }
        __syncthreads();
        for (int e = tid; e < nc * nc; e += nth) {
            const int i = e / nc, j = e % nc;
            double acc = W.J.M[i][j];
            for (int k = 0; k < 2 * cnt; k++) acc = acc + W.rows[k][i] * W.rows[k][j];
            W.J.M[i][j] = acc;
        }
        __syncthreads();
    }
    jacobi_rounds_block(W.J, nc);
    double res[12];
    {
        int bi = 0;
        double best = W.J.M[0][0];
        for (int i = 1; i < nc; i++) {
            const double dd = W.J.M[i][i];
            if (dd < best) { best = dd; bi = i; }
        }
        for (int k = 0; k < 12; k++) res[k] = k < nc ? W.J.V[k][bi] : 0.0;
    }
    double R0[9], t0[3];
    if (!planar) {  // (:595-635)
        double tmp[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) tmp[3 * i + j] = res[3 * j + i];
        double cn[3];
        for (int j = 0; j < 3; j++) cn[j] = sqrt((tmp[j] * tmp[j] + tmp[3 + j] * tmp[3 + j]) + tmp[6 + j] * tmp[6 + j]);
        const double prod = fabs((cn[0] * cn[1]) * cn[2]);
        const double scale = 1.0 / spec_cbrt64(prod);
        double Rp[9], ts[3], tt[3], tinv[3];
        polar3(tmp, Rp);
        for (int i = 0; i < 3; i++) ts[i] = scale * res[9 + i];
        matvec3(Rp, ts, tt);
        transpose3d(Rp, R0);  // S13: the inverse of [Rout | +-tout] is [Rout^T | -+Rout^T tout]
        matvec3(R0, tt, tinv);
        for (int i = 0; i < 3; i++) tinv[i] = -tinv[i];
        double err[2];
        for (int s = 0; s < 2; s++) {
            double e = 0.0;
            for (int p = 0; p < 6; p++) {
                double v[3];
                matvec3(R0, W.X6[p], v);
                for (int i = 0; i < 3; i++) v[i] = v[i] + (s ? -tinv[i] : tinv[i]);
                const double nv = norm3(v);
                for (int i = 0; i < 3; i++) v[i] = v[i] / nv;
                e = e + (1.0 - dot3(v, W.f6[p]));
            }
            err[s] = e;
        }
        for (int i = 0; i < 3; i++) t0[i] = err[0] < err[1] ? tinv[i] : -tinv[i];
    } else {  // (:533-592)
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
        for (int c = 0; c < 4; c++) {  // (:577-590): the first minimum
            const double* Rc = c < 2 ? R1 : R2;
            double val = 0.0;
            for (int p = 0; p < 6; p++) {
                double v[3];
                matvec3(Rc, W.X6[p], v);
                for (int i = 0; i < 3; i++) v[i] = v[i] + ((c & 1) ? -t[i] : t[i]);
                const double nv = norm3(v);
                for (int i = 0; i < 3; i++) v[i] = v[i] / nv;
                val = val + (1.0 - dot3(v, W.f6[p]));
            }
            if (c == 0 || val < best) {
                best = val;
                for (int k = 0; k < 9; k++) R0[k] = Rc[k];
                for (int i = 0; i < 3; i++) t0[i] = (c & 1) ? -t[i] : t[i];
            }
        }
    }
    // ---- Gauss-Newton (:693-757) ----
    double x[6];
    rot2rodrigues(R0, x);
    for (int i = 0; i < 3; i++) x[3 + i] = t0[i];
    gnEvals = 0;
    gnExit = 0;
    for (int it = 0; it < 5; it++) {
        double R[9], D[3][9];
        rodrigues2rot(x, R, D);
        __syncthreads();  // (the previous pass's readers of W.acc / W.maxBits are done)
        for (int e = tid; e < 42; e += nth) W.acc[e] = 0.0;
        if (tid == 0) { W.maxBits = 0ull; W.firstNan = 0; }
        __syncthreads();
        for (int ch = 0; ch < chunks; ch++) {
            const int base = ch * kMlpnpChunk, cnt = (n - base < kMlpnpChunk ? n - base : kMlpnpChunk);
            for (int t = tid; t < cnt; t += nth) {
                const int idx = indexOf(base + t);
                double* a = W.rows[2 * t];
                double* b = W.rows[2 * t + 1];
                point_rows(R, D, x + 3, C.X + 3 * (size_t)idx, C.nr + 3 * (size_t)idx, C.ns + 3 * (size_t)idx, a, a[6], b, b[6]);
            }
            __syncthreads();
            for (int e = tid; e < 42; e += nth) {  // J^T J (36) and J^T r (6)
                const int i = e < 36 ? e / 6 : e - 36, j = e < 36 ? e % 6 : 6;
                double acc = W.acc[e];
                for (int k = 0; k < 2 * cnt; k++) acc = acc + W.rows[k][i] * W.rows[k][j];
                W.acc[e] = acc;
            }
            __syncthreads();
        }
        double A6[6][6], g6[6], dx[6];
        for (int i = 0; i < 6; i++) {
            for (int j = 0; j < 6; j++) A6[i][j] = W.acc[6 * i + j];
            g6[i] = W.acc[36 + i];
        }
        ldlt_solve6(A6, g6, dx);
        gnEvals++;
        double mx = fabs(dx[0]), mn = fabs(dx[0]);
        for (int i = 1; i < 6; i++) {
            mx = fabs(dx[i]) > mx ? fabs(dx[i]) : mx;
            mn = fabs(dx[i]) < mn ? fabs(dx[i]) : mn;
        }
        if (mx > 5.0 || mn > 1.0) { gnExit = 1; break; }  // (:743)
        for (int ch = 0; ch < chunks; ch++) {  // max |Jac dx| (:746-747)
            const int base = ch * kMlpnpChunk, cnt = (n - base < kMlpnpChunk ? n - base : kMlpnpChunk);
            for (int t = tid; t < cnt; t += nth) {
                const int idx = indexOf(base + t);
                double J[2][6], r0, r1;
                point_rows(R, D, x + 3, C.X + 3 * (size_t)idx, C.nr + 3 * (size_t)idx, C.ns + 3 * (size_t)idx, J[0], r0, J[1], r1);
                for (int h = 0; h < 2; h++) {
                    const double dl = fabs(((((J[h][0] * dx[0] + J[h][1] * dx[1]) + J[h][2] * dx[2]) + J[h][3] * dx[3]) + J[h][4] * dx[4]) +
                                           J[h][5] * dx[5]);
                    if (dl != dl) {
                        if (base + t == 0 && h == 0) W.firstNan = 1;
                    } else {
                        atomicMax(&W.maxBits, nonneg_bits(dl));
                    }
                }
            }
        }
        __syncthreads();
        double maxDl;
        {
            const unsigned long long u = W.maxBits;
            memcpy(&maxDl, &u, sizeof u);
        }
        const bool converged = !W.firstNan && maxDl < 1e-5;
        for (int i = 0; i < 6; i++) x[i] = x[i] - dx[i];
        if (converged) { gnExit = 2; break; }
    }
    rodrigues2rot(x, Rout, nullptr);
    for (int i = 0; i < 3; i++) tout[i] = x[3 + i];
    planarOut = planar ? 1 : 0;
    __syncthreads();
}

// CheckInliers (:261-292) of one correspondence
__device__ __forceinline__ bool is_inlier(const MlpnpArgs& G, const double (&R)[9], const double (&t)[3], int m)
{
    const float X = G.pts[3 * (size_t)m], Y = G.pts[3 * (size_t)m + 1], Z = G.pts[3 * (size_t)m + 2];
    const float xc = (float)(((R[0] * (double)X + R[1] * (double)Y) + R[2] * (double)Z) + t[0]);
    const float yc = (float)(((R[3] * (double)X + R[4] * (double)Y) + R[5] * (double)Z) + t[1]);
    const float zc = (float)(((R[6] * (double)X + R[7] * (double)Y) + R[8] * (double)Z) + t[2]);
    float u, v;
    camera_project(G.cam, xc, yc, zc, u, v);
    const float distX = G.kp[2 * (size_t)m] - u;
    const float distY = G.kp[2 * (size_t)m + 1] - v;
    const float error2 = distX * distX + distY * distY;
    return error2 < G.maxErr[m];
}

// the inlier pass of a block of whole waves: mask words and the count (every thread returns it)
__device__ inline int inlier_pass(const MlpnpArgs& G, const double (&R)[9], const double (&t)[3], unsigned long long* mask, int* sCount)
{
    const int tid = threadIdx.x;
    if (tid == 0) *sCount = 0;
    __syncthreads();
    int local = 0;
    for (int base = 0; base < G.N; base += blockDim.x) {
        const int m = base + tid;
        const bool in = m < G.N && is_inlier(G, R, t, m);
        const unsigned long long word = __ballot(in);
        if ((tid & 63) == 0 && m < G.N) {
            mask[m / 64] = word;
            local += __popcll(word);
        }
    }
    if (local) atomicAdd(sCount, local);
    __syncthreads();
    return *sCount;
}

__device__ inline MlpnpCorr corr_of(const MlpnpArgs& G)
{
    return MlpnpCorr{G.X, G.f, G.nr, G.ns};
}

// the constructor's work for correspondence c (:73-90) and mvMaxError (:258)
__device__ inline void prep_corr(const MlpnpArgs& G, int c)
{
    float rx, ry;
    cam_unproject(G.cam, G.precision, G.kp[2 * (size_t)c], G.kp[2 * (size_t)c + 1], rx, ry);
    const double f[3] = {(double)rx, (double)ry, 1.0};  // (:78-80): unproject(kp.pt) / z, not of unit length
    // columns 1 and 2 of the Householder reflector of f (S13)
    const double nrm = norm3(f);
    const double alpha = f[0] >= 0.0 ? -nrm : nrm;
    const double v[3] = {f[0] - alpha, f[1], f[2]};
    const double beta = 2.0 / dot3(v, v);
    for (int k = 0; k < 3; k++) {
        const double w = beta * v[k];
        G.f[3 * (size_t)c + k] = f[k];
        G.nr[3 * (size_t)c + k] = (k == 1 ? 1.0 : 0.0) - w * v[1];
        G.ns[3 * (size_t)c + k] = (k == 2 ? 1.0 : 0.0) - w * v[2];
        G.X[3 * (size_t)c + k] = (double)G.pts[3 * (size_t)c + k];
    }
    G.maxErr[c] = G.sigma2[G.octave[c]] * G.th2;
}

__global__ __launch_bounds__(256) void mlpnp_prep_kernel(MlpnpArgs G)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < G.N) prep_corr(G, c);
}

__global__ __launch_bounds__(64) void mlpnp_hypothesis_kernel(MlpnpArgs G)
{
    __shared__ PoseWork W;
    __shared__ int sCount;
    const int it = blockIdx.x;
    const MlpnpCorr C = corr_of(G);
    const int* set = G.sets + (size_t)it * G.minSet;
    double R[9], t[3];
    int planar, evals, kind;
    compute_pose(W, C, G.minSet, [set](int k) { return set[k]; }, R, t, planar, evals, kind);
    const int count = inlier_pass(G, R, t, G.hypMask + (size_t)it * G.words, &sCount);
    if (threadIdx.x < 9) G.hypRt[(size_t)it * 12 + threadIdx.x] = R[threadIdx.x];
    else if (threadIdx.x < 12) G.hypRt[(size_t)it * 12 + threadIdx.x] = t[threadIdx.x - 9];
    if (threadIdx.x == 0) {
        G.hypCount[it] = count;
        G.hypMeta[3 * it] = planar;
        G.hypMeta[3 * it + 1] = evals;
        G.hypMeta[3 * it + 2] = kind;
    }
}

__global__ __launch_bounds__(kMlpnpRefineThreads) void mlpnp_refine_kernel(MlpnpArgs G)
{
    __shared__ PoseWork W;
    __shared__ int sCount, sBeaten;
    __shared__ int sPrefix[kMlpnpMaxWords + 1];
    const int it = blockIdx.x, tid = threadIdx.x;
    // candidate: a qualifying count that no earlier hypothesis reaches (:169-172)
    const int mine = G.hypCount[it];
    if (tid == 0) sBeaten = 0;
    __syncthreads();
    if (mine >= G.minInliers) {
        int beaten = 0;
        for (int j = tid; j < it; j += blockDim.x) beaten |= G.hypCount[j] >= mine;
        if (beaten) sBeaten = 1;
    }
    __syncthreads();
    if (mine < G.minInliers || sBeaten) {
        if (tid == 0) G.candCount[it] = -1;
        return;
    }
    // Refine (:294-352): the hypothesis's inliers in ascending order
    const unsigned long long* mask = G.hypMask + (size_t)it * G.words;
    if (tid == 0) {
        int acc = 0;
        for (int w = 0; w < G.words; w++) { sPrefix[w] = acc; acc += __popcll(mask[w]); }
        sPrefix[G.words] = acc;
    }
    __syncthreads();
    const int words = G.words;
    const int* prefix = sPrefix;
    auto indexOf = [mask, words, prefix](int k) {
        int lo = 0, hi = words - 1;  // the last word whose prefix count is <= k
        while (lo < hi) {
            const int mid = (lo + hi + 1) / 2;
            if (prefix[mid] <= k) lo = mid; else hi = mid - 1;
        }
        unsigned long long w = mask[lo];
        for (int r = k - prefix[lo]; r > 0; r--) w &= w - 1;
        return lo * 64 + __ffsll((long long)w) - 1;
    };
    const MlpnpCorr C = corr_of(G);
    double R[9], t[3];
    int planar, evals, kind;
    compute_pose(W, C, mine, indexOf, R, t, planar, evals, kind);
    const int count = inlier_pass(G, R, t, G.candMask + (size_t)it * G.words, &sCount);
    if (tid < 9) G.candRt[(size_t)it * 12 + tid] = R[tid];
    else if (tid < 12) G.candRt[(size_t)it * 12 + tid] = t[tid - 9];
    if (tid == 0) {
        G.candCount[it] = count;
        G.candPlanar[it] = planar;
    }
}

constexpr char kMlpnpSizeErr[] =
    "orbfe_mlpnp_params / orbfe_mlpnp_info struct_size does not match this library (rebuild the caller against include/orbfe.h)";

bool mlpnp_params_ok(const orbfe_mlpnp_params* P)
{
    return (P->camera_model == ORBFE_CAMERA_PINHOLE || P->camera_model == ORBFE_CAMERA_KANNALA_BRANDT8) && P->probability > 0.0 &&
           P->probability < 1.0 && P->min_inliers >= 0 && P->max_iterations >= 1 && P->max_iterations <= 4096 && P->min_set >= 6 &&
           P->min_set <= 64 && P->epsilon > 0.0f && P->epsilon <= 1.0f && P->n_iterations >= 0 && P->n_iterations <= 4096;
}

}  // namespace

// SetRansacParameters (:224-259) and the pass count of a first iterate(n_iterations) (:106-116); host only
int mlpnp_plan(const orbfe_mlpnp_params* P, int N, int* minInliers, int* maxIts, int* total)
{
    if (P->struct_size != (int)sizeof(orbfe_mlpnp_params) || !mlpnp_params_ok(P) || N < 0) return ORBFE_ERR_INVALID_ARG;
    float eps = P->epsilon;
    int nMin = (int)((float)N * eps);
    if (nMin < P->min_inliers) nMin = P->min_inliers;
    if (nMin < P->min_set) nMin = P->min_set;
    *minInliers = nMin;
    *maxIts = 0;
    *total = 0;
    if (N < nMin) return ORBFE_OK;
    if (eps < (float)nMin / (float)N) eps = (float)nMin / (float)N;
    double nIt;
    if (nMin == N) nIt = 1.0;
    else {
        const double den = log(1.0 - pow((double)eps, 3.0));
        const double num = log(1.0 - P->probability);
        nIt = den != 0.0 ? ceil(num / den) : INFINITY;
    }
    int its = !(nIt < (double)P->max_iterations) ? P->max_iterations : (int)nIt;
    if (its < 1) its = 1;
    *maxIts = its;
    *total = its > P->n_iterations ? its : P->n_iterations;
    return ORBFE_OK;
}

int mlpnp_run(MatchScratch& m, hipStream_t s, const orbfe_mlpnp_params* P, const float* levelSigma2, int nLevels, int n,
              const orbfe_keypoint* kp, const int* mpIndex, int nPoints, const float* points, const int* sets, int nSets, int* solved,
              float* Tcw, uint8_t* inliers, int* nInliers, int* noMore, orbfe_mlpnp_info* info, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_mlpnp_params) || (info && info->struct_size != (int)sizeof(orbfe_mlpnp_info))) {
        err = kMlpnpSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    if (!mlpnp_params_ok(P) || n > 64 * kMlpnpMaxWords) return ORBFE_ERR_INVALID_ARG;
    std::vector<int> first;  // mvKeyPointIndices (:67-94)
    if (!matched_keypoints(n, kp, mpIndex, nPoints, nLevels, first)) return ORBFE_ERR_INVALID_ARG;
    const int N = (int)first.size();
    int minInliers, maxIts, total;
    const int prc = mlpnp_plan(P, N, &minInliers, &maxIts, &total);
    if (prc != ORBFE_OK) return prc;

    *solved = 0;
    *nInliers = 0;
    *noMore = 1;
    for (int i = 0; i < 16; i++) Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;  // Tout.setIdentity() (:101)
    if (n > 0) memset(inliers, 0, (size_t)n);
    orbfe_mlpnp_info local;
    memset(&local, 0, sizeof local);
    if (info) local = *info;
    orbfe_mlpnp_info& I = local;
    I.struct_size = (int)sizeof(orbfe_mlpnp_info);
    I.N = N; I.min_inliers = minInliers; I.max_its = maxIts; I.total_iterations = total;
    I.exit_kind = ORBFE_MLPNP_EXIT_ABORT;
    I.returning_iteration = -1;
    I.n_candidates = 0;
    struct Publish {  // the info block goes out on every path
        orbfe_mlpnp_info* dst;
        orbfe_mlpnp_info* src;
        ~Publish() { if (dst) *dst = *src; }
    } publish{info, &local};
    if (total == 0) return ORBFE_OK;  // (:106-111)
    if (nSets != total || !sets) return ORBFE_ERR_INVALID_ARG;
    const int minSet = P->min_set;
    for (int it = 0; it < total; it++)
        for (int j = 0; j < minSet; j++) {
            const int v = sets[(size_t)it * minSet + j];
            if (v < 0 || v >= N) return ORBFE_ERR_INVALID_ARG;
            for (int k = 0; k < j; k++)
                if (sets[(size_t)it * minSet + k] == v) return ORBFE_ERR_INVALID_ARG;
        }

    const int words = (N + 63) / 64;
    // up: [kp | octave | pts | sets]; device only: [X | f | nr | ns | maxErr]; result block: [hypRt | candRt | hypCount | hypMeta |
    // candCount | candPlanar | hypMask | candMask]
    Carver c;
    const size_t oKp = c.take((size_t)N * 2 * sizeof(float));
    const size_t oOct = c.take((size_t)N * sizeof(int));
    const size_t oPts = c.take((size_t)N * 3 * sizeof(float));
    const size_t oSets = c.take((size_t)total * minSet * sizeof(int));
    const size_t inBytes = c.off;
    const size_t oX = c.take((size_t)N * 3 * sizeof(double));
    const size_t oF = c.take((size_t)N * 3 * sizeof(double));
    const size_t oNr = c.take((size_t)N * 3 * sizeof(double));
    const size_t oNs = c.take((size_t)N * 3 * sizeof(double));
    const size_t oMaxErr = c.take((size_t)N * sizeof(float));
    const size_t oHypRt = c.take((size_t)total * 12 * sizeof(double));
    const size_t oCandRt = c.take((size_t)total * 12 * sizeof(double));
    const size_t oHypCount = c.take((size_t)total * sizeof(int));
    const size_t oHypMeta = c.take((size_t)total * 3 * sizeof(int));
    const size_t oCandCount = c.take((size_t)total * sizeof(int));
    const size_t oCandPlanar = c.take((size_t)total * sizeof(int));
    const size_t oHypMask = c.take((size_t)total * words * sizeof(unsigned long long));
    const size_t oCandMask = c.take((size_t)total * words * sizeof(unsigned long long));
    const size_t resBytes = c.off - oHypRt;
    int rc = ensure(m, c.off, inBytes + resBytes + 256, err);
    if (rc != ORBFE_OK) return rc;
    uint8_t* hp = static_cast<uint8_t*>(m.hpin);
    uint8_t* dp = static_cast<uint8_t*>(m.d);
    float* hKp = reinterpret_cast<float*>(hp + oKp);
    int* hOct = reinterpret_cast<int*>(hp + oOct);
    float* hPts = reinterpret_cast<float*>(hp + oPts);
    for (int cI = 0; cI < N; cI++) {
        const int i = first[(size_t)cI];
        hKp[2 * cI] = kp[i].x; hKp[2 * cI + 1] = kp[i].y;
        hOct[cI] = kp[i].octave;
        for (int k = 0; k < 3; k++) hPts[3 * cI + k] = points[3 * (size_t)mpIndex[i] + k];
    }
    memcpy(hp + oSets, sets, (size_t)total * minSet * sizeof(int));

    MCHK(hipMemcpyAsync(dp, hp, inBytes, hipMemcpyHostToDevice, s));
    MlpnpArgs G;
    G.N = N; G.minSet = minSet; G.words = words; G.minInliers = minInliers;
    G.cam = CamP{P->cam[0], P->cam[1], P->cam[2], P->cam[3], P->cam[4], P->cam[5], P->cam[6], P->cam[7], P->camera_model};
    G.precision = P->kb_precision;
    G.th2 = P->th2;
    for (int i = 0; i < kMaxLevels; i++) G.sigma2[i] = i < nLevels ? levelSigma2[i] : 0.0f;
    G.kp = reinterpret_cast<const float*>(dp + oKp);
    G.octave = reinterpret_cast<const int*>(dp + oOct);
    G.pts = reinterpret_cast<const float*>(dp + oPts);
    G.sets = reinterpret_cast<const int*>(dp + oSets);
    G.X = reinterpret_cast<double*>(dp + oX);
    G.f = reinterpret_cast<double*>(dp + oF);
    G.nr = reinterpret_cast<double*>(dp + oNr);
    G.ns = reinterpret_cast<double*>(dp + oNs);
    G.maxErr = reinterpret_cast<float*>(dp + oMaxErr);
    G.hypRt = reinterpret_cast<double*>(dp + oHypRt);
    G.candRt = reinterpret_cast<double*>(dp + oCandRt);
    G.hypCount = reinterpret_cast<int*>(dp + oHypCount);
    G.hypMeta = reinterpret_cast<int*>(dp + oHypMeta);
    G.candCount = reinterpret_cast<int*>(dp + oCandCount);
    G.candPlanar = reinterpret_cast<int*>(dp + oCandPlanar);
    G.hypMask = reinterpret_cast<unsigned long long*>(dp + oHypMask);
    G.candMask = reinterpret_cast<unsigned long long*>(dp + oCandMask);
    hipLaunchKernelGGL(mlpnp_prep_kernel, dim3((N + 255) / 256), dim3(256), 0, s, G);
    hipLaunchKernelGGL(mlpnp_hypothesis_kernel, dim3(total), dim3(64), 0, s, G);
    hipLaunchKernelGGL(mlpnp_refine_kernel, dim3(total), dim3(kMlpnpRefineThreads), 0, s, G);
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(hp + inBytes, dp + oHypRt, resBytes, hipMemcpyDeviceToHost, s));
    MCHK(hipStreamSynchronize(s));
    const uint8_t* r = hp + inBytes;
    const double* hypRt = reinterpret_cast<const double*>(r);
    const double* candRt = reinterpret_cast<const double*>(r + (oCandRt - oHypRt));
    const int* hypCount = reinterpret_cast<const int*>(r + (oHypCount - oHypRt));
    const int* hypMeta = reinterpret_cast<const int*>(r + (oHypMeta - oHypRt));
    const int* candCount = reinterpret_cast<const int*>(r + (oCandCount - oHypRt));
    const int* candPlanar = reinterpret_cast<const int*>(r + (oCandPlanar - oHypRt));
    const unsigned long long* hypMask = reinterpret_cast<const unsigned long long*>(r + (oHypMask - oHypRt));
    const unsigned long long* candMask = reinterpret_cast<const unsigned long long*>(r + (oCandMask - oHypRt));

    if (I.hyp_Rt) memcpy(I.hyp_Rt, hypRt, (size_t)total * 12 * sizeof(double));
    if (I.hyp_inliers) memcpy(I.hyp_inliers, hypCount, (size_t)total * sizeof(int));
    for (int it = 0; it < total; it++) {
        if (I.hyp_planar) I.hyp_planar[it] = (uint8_t)hypMeta[3 * it];
        if (I.hyp_gn_evals) I.hyp_gn_evals[it] = hypMeta[3 * it + 1];
        if (I.hyp_gn_exit) I.hyp_gn_exit[it] = hypMeta[3 * it + 2];
    }
    // the loop (:116-222) on what came back: the candidates in iteration order, the first whose Refine succeeds returns (:335)
    int nCand = 0, winner = -1, last = -1;
    for (int it = 0; it < total; it++) {
        if (candCount[it] < 0) continue;
        if (I.candidates) I.candidates[nCand] = it;
        if (I.cand_Rt) memcpy(I.cand_Rt + (size_t)nCand * 12, candRt + (size_t)it * 12, 12 * sizeof(double));
        if (I.cand_inliers) I.cand_inliers[nCand] = candCount[it];
        if (I.cand_planar) I.cand_planar[nCand] = (uint8_t)candPlanar[it];
        if (I.cand_mask)
            for (int cI = 0; cI < N; cI++) I.cand_mask[(size_t)nCand * N + cI] = (uint8_t)((candMask[(size_t)it * words + cI / 64] >> (cI % 64)) & 1ull);
        if (winner < 0 && candCount[it] > minInliers) winner = it;
        last = it;
        nCand++;
    }
    I.n_candidates = nCand;
    const double* Rt;
    const unsigned long long* mask;
    if (winner >= 0) {
        I.exit_kind = ORBFE_MLPNP_EXIT_REFINED;
        I.returning_iteration = winner;
        Rt = candRt + (size_t)winner * 12;
        mask = candMask + (size_t)winner * words;
        *nInliers = candCount[winner];
        *noMore = 0;
    } else if (last >= 0) {  // (:204-219)
        I.exit_kind = ORBFE_MLPNP_EXIT_BEST_UNREFINED;
        I.returning_iteration = last;
        Rt = hypRt + (size_t)last * 12;
        mask = hypMask + (size_t)last * words;
        *nInliers = hypCount[last];
    } else {
        I.exit_kind = ORBFE_MLPNP_EXIT_FAILED;
        return ORBFE_OK;
    }
    *solved = 1;
    fill_tcw(Rt, Rt + 9, Tcw);
    for (int cI = 0; cI < N; cI++)
        if ((mask[cI / 64] >> (cI % 64)) & 1ull) inliers[first[(size_t)cI]] = 1;
    return ORBFE_OK;
}

}  // namespace orbfe

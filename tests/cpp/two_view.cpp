// TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:40-127) from a plain C++ program, three ways on the same
// inputs:
//   (a) the library through include/orbfe_adaptor.hpp's TwoViewReconstruction class (orbfe_two_view_reconstruct),
//   (b) SPEC DECISION S12 as a single-thread host loop (this file, -O2 -ffp-contract=off, one pinned core),
//   (c) the same loop with FindHomography and FindFundamental on two threads (two pinned cores), as :102-107 runs them.
// (b) / (c) are the library's arithmetic for one or two CPU threads, so they are the latency yardstick, not an independent oracle --
// that is tests/twoview_ref.py.  Shared with the library, as the same text compiled for the host (-I csrc): the 3 x 3 helpers, the
// Jacobi angle, the n = 3 and n = 4 sequences and the rank-2 step (jacobi.h); the per-match terms, the ordered keys, Normalize, the
// 3 x 3 SVD and the motion hypotheses (twoview_math.h).  Restated here: only the one-thread ordering of what the teams of threads do in
// csrc/kernels_twoview.hip (null9, find_model and its score sums, check_rt) and the selection rules of the host call (reconstruct).
// Their results must equal the library's bit for bit (host_same=1), and tests/test_twoview_cpp.py compares them with the numpy
// restatement without a GPU.
//   usage: two_view                                   -> library version (link test)
//          two_view <scene.bin> <out.bin> host        -> (b) and (c) only, results of (b) to out.bin: no GPU needed
//          two_view <scene.bin> <out.bin> [reps]      -> (a), (b), (c); results of (a) to out.bin; medians of `reps` calls
// scene.bin: int32 n1, n2, iterations; float32 fx, fy, cx, cy, sigma; keypoints of frame 1 and 2 (24 B each); int32 matches12[n1];
//            int32 sets[iterations][8]
// out.bin:   int32 reconstructed, model, exit_line, best_it_H, best_it_F, n_hypotheses, best_hypothesis, n_good[8];
//            float32 SH, SF, RH, H21[9], F21[9], cos_parallax[8], R21[9], t21[3], scores[2 * iterations], p3d[n1][3]; uint8 triangulated[n1]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <thread>

#include <sched.h>

#include "orbfe_adaptor.hpp"
#include "jacobi.h"
#include "twoview_math.h"

using namespace ORB_SLAM3;

namespace s12 {

using namespace orbfe;   // csrc/jacobi.h, twoview_math.h: the library's own text of everything outside the teams of threads, compiled for the host

// S12 at n = 9: round r = the pairs {i, j}, i < j, i + j == r (mod 9), ascending i; angles from M at the start of the round, then
// the column phase of all four pairs, the row phase of all four, V's column phase
static void null9(const float (*A)[9], int rows, float (&out)[9])
{
    double M[9][9], V[9][9];
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) {
            double acc = 0.0;
            for (int k = 0; k < rows; k++) acc = acc + (double)A[k][i] * (double)A[k][j];
            M[i][j] = acc;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < kTwoViewSweeps; sweep++)
        for (int r = 0; r < 9; r++) {
            int P[4], Q[4], np = 0;
            double C[4], S[4];
            bool skip[4];
            for (int i = 0; i < 9; i++) {
                const int j = (r - i + 9) % 9;
                if (i < j) { P[np] = i; Q[np] = j; np++; }
            }
            for (int e = 0; e < 4; e++) {
                const double apq = M[P[e]][Q[e]];
                skip[e] = apq == 0.0;
                C[e] = 1.0; S[e] = 0.0;
                if (!skip[e]) jacobi_angle(M[P[e]][P[e]], M[Q[e]][Q[e]], apq, C[e], S[e]);
            }
            for (int e = 0; e < 4; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < 9; k++) {
                    const double a = M[k][P[e]], b = M[k][Q[e]];
                    M[k][P[e]] = C[e] * a - S[e] * b;
                    M[k][Q[e]] = S[e] * a + C[e] * b;
                }
            }
            for (int e = 0; e < 4; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < 9; k++) {
                    const double a = M[P[e]][k], b = M[Q[e]][k];
                    M[P[e]][k] = C[e] * a - S[e] * b;
                    M[Q[e]][k] = S[e] * a + C[e] * b;
                }
            }
            for (int e = 0; e < 4; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < 9; k++) {
                    const double a = V[k][P[e]], b = V[k][Q[e]];
                    V[k][P[e]] = C[e] * a - S[e] * b;
                    V[k][Q[e]] = S[e] * a + C[e] * b;
                }
            }
        }
    int bi = 0;  // the column of the smallest diagonal entry, lowest index on ties
    for (int i = 1; i < 9; i++)
        if (M[i][i] < M[bi][bi]) bi = i;
    for (int k = 0; k < 9; k++) out[k] = (float)V[k][bi];
}
struct Pt { float u1, v1, u2, v2; };

// CheckHomography (:308-384) / CheckFundamental (:386-471): the two terms of every match in match order, first-image term first.  A
// rejected term is +0.0f, and adding it leaves the score as it is: the score starts at +0.0f and no term is negative, so it is never -0.0f.
static float check_homography(const float (&H21)[9], const float (&H12)[9], const std::vector<Pt>& pts, float invSigmaSquare, std::vector<uint8_t>& in)
{
    float score = 0.0f;
    for (size_t i = 0; i < pts.size(); i++) {
        const Pt& p = pts[i];
        float term1, term2;
        bool bIn;
        homography_terms(H21, H12, invSigmaSquare, p.u1, p.v1, p.u2, p.v2, term1, term2, bIn);
        score = score + term1;
        score = score + term2;
        in[i] = bIn;
    }
    return score;
}
static float check_fundamental(const float (&F)[9], const std::vector<Pt>& pts, float invSigmaSquare, std::vector<uint8_t>& in)
{
    float score = 0.0f;
    for (size_t i = 0; i < pts.size(); i++) {
        const Pt& p = pts[i];
        float term1, term2;
        bool bIn;
        fundamental_terms(F, invSigmaSquare, p.u1, p.v1, p.u2, p.v2, term1, term2, bIn);
        score = score + term1;
        score = score + term2;
        in[i] = bIn;
    }
    return score;
}

struct Model {
    float score = 0.0f, M[9] = {0};
    int it = -1;
    std::vector<uint8_t> inliers;
};
struct Shared {
    int iterations = 0;
    std::vector<Pt> pts, npts;
    const int* sets = nullptr;
    float T1[9], T2inv[9], T2t[9], invSigmaSquare;
};

// FindHomography (:129-177) / FindFundamental (:180-228)
static void find_model(const Shared& S, bool isF, Model& best, float* scores)
{
    const size_t N = S.pts.size();
    best = Model();
    best.inliers.assign(N, 0);
    std::vector<uint8_t> cur(N);
    for (int it = 0; it < S.iterations; it++) {
        float A[16][9], X[9], X21[9], X12[9], tmp[9];
        for (int j = 0; j < 8; j++) {
            const Pt& p = S.npts[(size_t)S.sets[it * 8 + j]];
            if (!isF) {
                const float r0[9] = {0.0f, 0.0f, 0.0f, -p.u1, -p.v1, -1.0f, p.v2 * p.u1, p.v2 * p.v1, p.v2};
                const float r1[9] = {p.u1, p.v1, 1.0f, 0.0f, 0.0f, 0.0f, -p.u2 * p.u1, -p.u2 * p.v1, -p.u2};
                std::memcpy(A[2 * j], r0, sizeof r0);
                std::memcpy(A[2 * j + 1], r1, sizeof r1);
            } else {
                const float r0[9] = {p.u2 * p.u1, p.u2 * p.v1, p.u2, p.v2 * p.u1, p.v2 * p.v1, p.v2, p.u1, p.v1, 1.0f};
                std::memcpy(A[j], r0, sizeof r0);
            }
        }
        null9(A, isF ? 8 : 16, X);
        float sc;
        if (!isF) {
            mul3(S.T2inv, X, tmp);
            mul3(tmp, S.T1, X21);
            inv3(X21, X12);
            sc = check_homography(X21, X12, S.pts, S.invSigmaSquare, cur);
        } else {
            float Fn[9];
            rank2_f(X, Fn);
            mul3(S.T2t, Fn, tmp);
            mul3(tmp, S.T1, X21);
            sc = check_fundamental(X21, S.pts, S.invSigmaSquare, cur);
        }
        scores[it] = sc;
        if (sc > best.score) {
            best.score = sc;
            best.it = it;
            std::memcpy(best.M, X21, sizeof X21);
            best.inliers = cur;
        }
    }
}

// CheckRT (:799-914): flags (bit 0 counted, bit 1 vbGood), x3d, -> nGood, cosine at rank min(50, nGood - 1)
static int check_rt(const float (&R)[9], const float (&t)[3], const float (&K)[9], const std::vector<Pt>& pts, const std::vector<uint8_t>& inl, float th2,
                    std::vector<uint8_t>& flags, std::vector<float>& x3d, float& cosSel)
{
    const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const float P1[12] = {fx, 0.0f, cx, 0.0f, 0.0f, fy, cy, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
    float P2[12], O2[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            const float x0 = j < 3 ? R[j] : t[0], x1 = j < 3 ? R[3 + j] : t[1], x2 = j < 3 ? R[6 + j] : t[2];
            P2[4 * i + j] = (K[3 * i] * x0 + K[3 * i + 1] * x1) + K[3 * i + 2] * x2;
        }
    for (int i = 0; i < 3; i++) O2[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];
    const size_t N = pts.size();
    flags.assign(N, 0);
    x3d.assign(3 * N, 0.0f);
    std::vector<unsigned> keys;
    for (size_t m = 0; m < N; m++) {
        if (!inl[m]) continue;
        const Pt& p = pts[m];
        float A[4][4];
        for (int j = 0; j < 4; j++) {
            A[0][j] = p.u1 * P1[8 + j] - P1[j];
            A[1][j] = p.v1 * P1[8 + j] - P1[4 + j];
            A[2][j] = p.u2 * P2[8 + j] - P2[j];
            A[3][j] = p.v2 * P2[8 + j] - P2[4 + j];
        }
        double M[4][4], vv[4];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                double acc = 0.0;
                for (int k = 0; k < 4; k++) acc = acc + (double)A[k][i] * (double)A[k][j];
                M[i][j] = acc;
            }
        sym4_min_eigenvector(M, vv);
        const float X = (float)(vv[0] / vv[3]), Y = (float)(vv[1] / vv[3]), Z = (float)(vv[2] / vv[3]);
        if (!std::isfinite(X) || !std::isfinite(Y) || !std::isfinite(Z)) continue;
        const float dist1 = std::sqrt((X * X + Y * Y) + Z * Z);
        const float nx = X - O2[0], ny = Y - O2[1], nz = Z - O2[2];
        const float dist2 = std::sqrt((nx * nx + ny * ny) + nz * nz);
        const float cosP = ((X * nx + Y * ny) + Z * nz) / (dist1 * dist2);
        const bool low = !((double)cosP < 0.99998);
        if (Z <= 0.0f && !low) continue;
        const float X2 = ((R[0] * X + R[1] * Y) + R[2] * Z) + t[0], Y2 = ((R[3] * X + R[4] * Y) + R[5] * Z) + t[1];
        const float Z2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + t[2];
        if (Z2 <= 0.0f && !low) continue;
        const float invZ1 = (float)(1.0 / (double)Z);
        const float e1x = ((fx * X) * invZ1 + cx) - p.u1, e1y = ((fy * Y) * invZ1 + cy) - p.v1;
        if (e1x * e1x + e1y * e1y > th2) continue;
        const float invZ2 = (float)(1.0 / (double)Z2);
        const float e2x = ((fx * X2) * invZ2 + cx) - p.u2, e2y = ((fy * Y2) * invZ2 + cy) - p.v2;
        if (e2x * e2x + e2y * e2y > th2) continue;
        flags[m] = low ? 1 : 3;
        x3d[3 * m] = X; x3d[3 * m + 1] = Y; x3d[3 * m + 2] = Z;
        keys.push_back(ordered_key(cosP));
    }
    const int nGood = (int)keys.size();
    cosSel = 1.0f;
    if (nGood > 0) {
        const size_t idx = (size_t)std::min(50, nGood - 1);
        std::nth_element(keys.begin(), keys.begin() + idx, keys.end());
        cosSel = ordered_key_inverse(keys[idx]);
    }
    return nGood;
}

struct Result {
    int reconstructed = 0, model = 0, exit_line = 62, itH = -1, itF = -1, nHyp = 0, bestHyp = -1, nGood[8] = {0};
    float SH = 0, SF = 0, RH = 0, H21[9] = {0}, F21[9] = {0}, cosSel[8], R21[9] = {0}, t21[3] = {0};
    std::vector<float> scores, p3d;
    std::vector<uint8_t> tri;
};

static void reconstruct(const orbfe_two_view_params& P, const std::vector<KeyPoint>& k1, const std::vector<KeyPoint>& k2,
                        const std::vector<int>& m12, const int* sets, bool twoThreads, Result& out)
{
    out = Result();
    for (float& c : out.cosSel) c = 1.0f;
    const int n1 = (int)k1.size();
    out.scores.assign((size_t)2 * P.iterations, 0.0f);
    out.p3d.assign((size_t)3 * n1, 0.0f);
    out.tri.assign((size_t)n1, 0);
    std::vector<int> first;
    for (int i = 0; i < n1; i++)
        if (m12[i] >= 0) first.push_back(i);
    const size_t N = first.size();
    if (N < 8) return;
    Shared S;
    S.iterations = P.iterations;
    S.sets = sets;
    std::vector<float> x1, y1, x2, y2;
    float T2[9];
    normalize_points((int)k1.size(), reinterpret_cast<const orbfe_keypoint*>(k1.data()), x1, y1, S.T1);
    normalize_points((int)k2.size(), reinterpret_cast<const orbfe_keypoint*>(k2.data()), x2, y2, T2);
    inv3(T2, S.T2inv);
    transpose3(T2, S.T2t);
    const float sigma2 = P.sigma * P.sigma;
    S.invSigmaSquare = (float)(1.0 / (double)sigma2);
    S.pts.resize(N); S.npts.resize(N);
    for (size_t m = 0; m < N; m++) {
        const int a = first[m], b = m12[a];
        S.pts[m] = Pt{k1[a].pt.x, k1[a].pt.y, k2[b].pt.x, k2[b].pt.y};
        S.npts[m] = Pt{x1[a], y1[a], x2[b], y2[b]};
    }
    Model H, F;
    if (twoThreads) {  // :102-107
        auto pinned = [](int cpu, auto fn) {
            return std::thread([cpu, fn] {
                cpu_set_t set;
                CPU_ZERO(&set);
                CPU_SET(cpu, &set);
                (void)sched_setaffinity(0, sizeof set, &set);
                fn();
            });
        };
        cpu_set_t mine;
        CPU_ZERO(&mine);
        (void)sched_getaffinity(0, sizeof mine, &mine);
        int cpus[2] = {-1, -1}, nc = 0;
        for (int c = 0; c < CPU_SETSIZE && nc < 2; c++)
            if (CPU_ISSET(c, &mine)) cpus[nc++] = c;
        if (nc < 2) cpus[1] = cpus[0];
        std::thread tH = pinned(cpus[0], [&] { find_model(S, false, H, out.scores.data()); });
        std::thread tF = pinned(cpus[1], [&] { find_model(S, true, F, out.scores.data() + P.iterations); });
        tH.join();
        tF.join();
    } else {
        find_model(S, false, H, out.scores.data());
        find_model(S, true, F, out.scores.data() + P.iterations);
    }
    out.SH = H.score; out.SF = F.score; out.itH = H.it; out.itF = F.it;
    std::memcpy(out.H21, H.M, sizeof H.M);
    std::memcpy(out.F21, F.M, sizeof F.M);
    if (out.SH + out.SF == 0.0f) { out.exit_line = 110; return; }
    out.RH = out.SH / (out.SH + out.SF);
    const bool useH = (double)out.RH > 0.40;
    out.model = useH ? 1 : 2;
    const std::vector<uint8_t>& inl = useH ? H.inliers : F.inliers;
    int nInl = 0;
    for (uint8_t b : inl) nInl += b != 0;
    const float K[9] = {P.fx, 0.0f, P.cx, 0.0f, P.fy, P.cy, 0.0f, 0.0f, 1.0f};
    float R[8][9], t[8][3];
    out.nHyp = useH ? motion_hypotheses_h(out.H21, K, R, t) : motion_hypotheses_f(out.F21, K, R, t);
    if (out.nHyp == 0) { out.exit_line = 609; return; }
    const float th2 = (float)(4.0 * (double)sigma2);
    std::vector<uint8_t> flags[8];
    std::vector<float> x3d[8];
    for (int h = 0; h < out.nHyp; h++) out.nGood[h] = check_rt(R[h], t[h], K, S.pts, inl, th2, flags[h], x3d[h], out.cosSel[h]);
    int best = -1;
    const int* g = out.nGood;
    if (!useH) {
        const int maxGood = std::max(g[0], std::max(g[1], std::max(g[2], g[3])));
        const int nMinGood = std::max((int)(0.9 * nInl), P.min_triangulated);
        int nsimilar = 0;
        for (int h = 0; h < 4; h++) nsimilar += g[h] > 0.7 * maxGood;
        if (maxGood < nMinGood || nsimilar > 1) { out.exit_line = 528; return; }
        const int pick = maxGood == g[0] ? 0 : maxGood == g[1] ? 1 : maxGood == g[2] ? 2 : 3;
        if (g[pick] > 0 && (double)out.cosSel[pick] < kCosOneDegree) best = pick;
        if (best < 0) { out.exit_line = 580; return; }
    } else {
        int bestGood = 0, second = 0, bi = -1;
        for (int h = 0; h < 8; h++) {
            if (g[h] > bestGood) { second = bestGood; bestGood = g[h]; bi = h; }
            else if (g[h] > second) second = g[h];
        }
        const bool ok = bi >= 0 && (double)out.cosSel[bi] <= kCosOneDegree;
        if (second < 0.75 * bestGood && ok && bestGood > P.min_triangulated && bestGood > 0.9 * nInl) best = bi;
        if (best < 0) { out.exit_line = 746; return; }
    }
    out.reconstructed = 1;
    out.exit_line = 0;
    out.bestHyp = best;
    std::memcpy(out.R21, R[best], sizeof out.R21);
    std::memcpy(out.t21, t[best], sizeof out.t21);
    for (size_t m = 0; m < N; m++) {
        const int f = flags[best][m], i1 = first[m];
        if (f & 1) std::memcpy(&out.p3d[3 * (size_t)i1], &x3d[best][3 * m], 12);
        out.tri[(size_t)i1] = (uint8_t)((f >> 1) & 1);
    }
}

}  // namespace s12

template <class F>
static double median_us(F fn, int reps)
{
    std::vector<double> v((size_t)reps);
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        v[(size_t)i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    std::sort(v.begin(), v.end());
    return v[(size_t)reps / 2];
}

static void write_result(const char* path, const s12::Result& r)
{
    std::ofstream out(path, std::ios::binary);
    const int head[7] = {r.reconstructed, r.model, r.exit_line, r.itH, r.itF, r.nHyp, r.bestHyp};
    out.write(reinterpret_cast<const char*>(head), sizeof head);
    out.write(reinterpret_cast<const char*>(r.nGood), sizeof r.nGood);
    const float s3[3] = {r.SH, r.SF, r.RH};
    out.write(reinterpret_cast<const char*>(s3), sizeof s3);
    out.write(reinterpret_cast<const char*>(r.H21), sizeof r.H21);
    out.write(reinterpret_cast<const char*>(r.F21), sizeof r.F21);
    out.write(reinterpret_cast<const char*>(r.cosSel), sizeof r.cosSel);
    out.write(reinterpret_cast<const char*>(r.R21), sizeof r.R21);
    out.write(reinterpret_cast<const char*>(r.t21), sizeof r.t21);
    out.write(reinterpret_cast<const char*>(r.scores.data()), (std::streamsize)(r.scores.size() * 4));
    out.write(reinterpret_cast<const char*>(r.p3d.data()), (std::streamsize)(r.p3d.size() * 4));
    out.write(reinterpret_cast<const char*>(r.tri.data()), (std::streamsize)r.tri.size());
}

static bool same(const s12::Result& a, const s12::Result& b)
{
    return a.reconstructed == b.reconstructed && a.model == b.model && a.exit_line == b.exit_line && a.itH == b.itH && a.itF == b.itF &&
           a.nHyp == b.nHyp && a.bestHyp == b.bestHyp && !std::memcmp(a.nGood, b.nGood, sizeof a.nGood) && !std::memcmp(&a.SH, &b.SH, 4) &&
           !std::memcmp(&a.SF, &b.SF, 4) && !std::memcmp(&a.RH, &b.RH, 4) && !std::memcmp(a.H21, b.H21, sizeof a.H21) &&
           !std::memcmp(a.F21, b.F21, sizeof a.F21) && !std::memcmp(a.cosSel, b.cosSel, sizeof a.cosSel) &&
           !std::memcmp(a.R21, b.R21, sizeof a.R21) && !std::memcmp(a.t21, b.t21, sizeof a.t21) && a.scores.size() == b.scores.size() &&
           !std::memcmp(a.scores.data(), b.scores.data(), a.scores.size() * 4) && a.p3d.size() == b.p3d.size() &&
           !std::memcmp(a.p3d.data(), b.p3d.data(), a.p3d.size() * 4) && a.tri == b.tri;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "drawsets")) {  // drawsets N iterations: a fresh process's first mvSets, one set per line; no GPU
        const int N = std::atoi(argv[2]), iterations = std::atoi(argv[3]);
        if (N < 8 || iterations < 1) return 2;
        const std::vector<int> sets = TwoViewReconstruction::DrawSets(N, iterations);
        for (int it = 0; it < iterations; it++)
            for (int j = 0; j < 8; j++) std::printf("%d%c", sets[(size_t)it * 8 + j], j == 7 ? '\n' : ' ');
        return 0;
    }
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream in(argv[1], std::ios::binary);
    int head[3];
    float cam[5];
    in.read(reinterpret_cast<char*>(head), sizeof head);
    in.read(reinterpret_cast<char*>(cam), sizeof cam);
    const int n1 = head[0], n2 = head[1], iterations = head[2];
    if (!in || n1 < 0 || n2 < 0 || iterations < 1 || iterations > 4096) { std::fprintf(stderr, "bad scene header\n"); return 2; }
    std::vector<KeyPoint> k1((size_t)n1), k2((size_t)n2);
    std::vector<int> m12((size_t)n1), sets((size_t)iterations * 8);
    in.read(reinterpret_cast<char*>(k1.data()), (std::streamsize)(k1.size() * sizeof(KeyPoint)));
    in.read(reinterpret_cast<char*>(k2.data()), (std::streamsize)(k2.size() * sizeof(KeyPoint)));
    in.read(reinterpret_cast<char*>(m12.data()), (std::streamsize)(m12.size() * 4));
    in.read(reinterpret_cast<char*>(sets.data()), (std::streamsize)(sets.size() * 4));
    if (!in) { std::fprintf(stderr, "short scene file\n"); return 2; }
    orbfe_two_view_params P = ORBFE_TWO_VIEW_PARAMS_INIT;
    P.fx = cam[0]; P.fy = cam[1]; P.cx = cam[2]; P.cy = cam[3]; P.sigma = cam[4]; P.iterations = iterations;
    int N = 0;
    for (int m : m12) N += m >= 0;

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = argc > 3 && !hostOnly ? std::max(std::atoi(argv[3]), 1) : 1;
    s12::Result one, two;
    s12::reconstruct(P, k1, k2, m12, sets.data(), false, one);
    s12::reconstruct(P, k1, k2, m12, sets.data(), true, two);
    const int threadsSame = same(one, two);
    if (hostOnly) {
        write_result(argv[2], one);
        std::printf("two_view host N=%d iterations=%d reconstructed=%d model=%d exit=%d threads_same=%d\n", N, iterations, one.reconstructed,
                    one.model, one.exit_line, threadsSame);
        return threadsSame ? 0 : 1;
    }

    ORBextractor ex(500, 20000, 1.2f, 4, 20, 7, 320, 240);  // the handle; the extractor itself is not used
    TwoViewReconstruction tvr(ex, P.fx, P.fy, P.cx, P.cy, P.sigma, iterations);
    s12::Result lib;
    std::array<float, 9> R21{};
    std::array<float, 3> t21{};
    std::vector<std::array<float, 3>> vP3D;
    std::vector<bool> vbTri;
    orbfe_two_view_info info;
    std::memset(&info, 0, sizeof info);
    info.struct_size = (int)sizeof info;
    lib.scores.assign((size_t)2 * iterations, 0.0f);
    info.scores = lib.scores.data();
    auto call = [&] { return tvr.Reconstruct(k1, k2, m12, R21, t21, vP3D, vbTri, &info, &sets); };
    const bool ok = call();
    lib.reconstructed = ok; lib.model = info.model; lib.exit_line = info.exit_line; lib.itH = info.best_it_H; lib.itF = info.best_it_F;
    lib.nHyp = info.n_hypotheses; lib.bestHyp = info.best_hypothesis;
    std::memcpy(lib.nGood, info.n_good, sizeof lib.nGood);
    lib.SH = info.SH; lib.SF = info.SF; lib.RH = info.RH;
    std::memcpy(lib.H21, info.H21, sizeof lib.H21);
    std::memcpy(lib.F21, info.F21, sizeof lib.F21);
    std::memcpy(lib.cosSel, info.cos_parallax, sizeof lib.cosSel);
    lib.p3d.assign((size_t)3 * n1, 0.0f);
    lib.tri.assign((size_t)n1, 0);
    if (ok) {
        std::memcpy(lib.R21, R21.data(), sizeof lib.R21);
        std::memcpy(lib.t21, t21.data(), sizeof lib.t21);
        for (int i = 0; i < n1; i++) {
            std::memcpy(&lib.p3d[3 * (size_t)i], vP3D[(size_t)i].data(), 12);
            lib.tri[(size_t)i] = vbTri[(size_t)i];
        }
    }
    write_result(argv[2], lib);
    const int hostSame = same(lib, one) && threadsSame;

    // three alternations of (a), (b), (c); the middle of the three medians
    double a[3], b[3], c[3];
    {
        cpu_set_t mine;  // (b) is one thread on one core: stay on the core we are on
        CPU_ZERO(&mine);
        (void)sched_getaffinity(0, sizeof mine, &mine);
        for (int round = 0; round < 3; round++) {
            a[round] = median_us([&] { (void)call(); }, reps);
            cpu_set_t pin;
            CPU_ZERO(&pin);
            CPU_SET(sched_getcpu(), &pin);
            (void)sched_setaffinity(0, sizeof pin, &pin);
            b[round] = median_us([&] { s12::reconstruct(P, k1, k2, m12, sets.data(), false, one); }, std::max(reps / 20, 3));
            (void)sched_setaffinity(0, sizeof mine, &mine);
            c[round] = median_us([&] { s12::reconstruct(P, k1, k2, m12, sets.data(), true, two); }, std::max(reps / 20, 3));
        }
    }
    std::sort(a, a + 3);
    std::sort(b, b + 3);
    std::sort(c, c + 3);
    std::printf("two_view N=%d iterations=%d reconstructed=%d model=%d exit=%d\n", N, iterations, lib.reconstructed, lib.model, lib.exit_line);
    std::printf("two_view_latency_us call=%.1f host_one_thread=%.1f host_two_threads=%.1f host_same=%d\n", a[1], b[1], c[1], hostSame);
    std::printf("two_view_rounds_us call=%.1f,%.1f,%.1f host_one_thread=%.1f,%.1f,%.1f host_two_threads=%.1f,%.1f,%.1f\n", a[0], a[1], a[2],
                b[0], b[1], b[2], c[0], c[1], c[2]);
    return hostSame ? 0 : 1;
}

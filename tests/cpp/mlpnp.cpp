// A fresh MLPnPsolver + SetRansacParameters + one iterate() (src/MLPnPsolver.cpp) from a plain C++ program, two ways on the same inputs:
//   (a) the library through include/orbfe_adaptor.hpp's MLPnPsolver class (orbfe_mlpnp_ransac),
//   (b) SPEC DECISION S13 as a single-thread host loop (this file, -O2 -ffp-contract=off, one pinned core): every hypothesis in turn,
//       Refine for every candidate, the first success returns.
// (b) is the kernels' arithmetic for one CPU thread, so it is the latency yardstick, not an independent oracle -- that is
// tests/mlpnp_ref.py.  Shared with the kernels, as the same text compiled for the host (-I csrc): everything one thread computes on
// its own -- spec_math.h, camera.h, jacobi.h, mat3d.h, ldlt.h.  Restated here: only the one-thread ordering of what a team of threads
// does in csrc/kernels_mlpnp.hip (jacobi_rounds, compute_pose, check_inliers, ransac).  Its results must equal the library's bit for
// bit (host_same=1), and tests/test_mlpnp_cpp.py compares them with the numpy restatement without a GPU.
//   usage: mlpnp                                   -> library version (link test)
//          mlpnp <scene.bin> <out.bin> host        -> (b) only, its results to out.bin: no GPU needed
//          mlpnp <scene.bin> <out.bin> [reps]      -> (a) and (b); results of (a) to out.bin; medians of `reps` calls
// scene.bin: int32 n, n_points, total, min_set, model, n_levels, min_inliers_param, max_iterations, n_iterations; float64 probability;
//            float32 cam[8], precision, epsilon, th2, level_sigma2[n_levels]; keypoints (24 B each); int32 mp_index[n];
//            float32 points[n_points][3]; int32 sets[total][min_set]
// out.bin:   int32 solved, n_inliers, no_more, N, min_inliers, max_its, total, exit_kind, returning_iteration, n_candidates;
//            float32 Tcw[16]; uint8 inliers[n]; float64 hyp_Rt[total][12]; int32 hyp_inliers[total], hyp_planar[total],
//            hyp_gn_evals[total], hyp_gn_exit[total], candidates[nc]; float64 cand_Rt[nc][12]; int32 cand_inliers[nc], cand_planar[nc];
//            uint8 cand_mask[nc][N]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include <sched.h>

#include "orbfe_adaptor.hpp"
#include "camera.h"
#include "jacobi.h"
#include "ldlt.h"
#include "mat3d.h"

using namespace ORB_SLAM3;

namespace s13 {

using namespace orbfe;   // csrc/*.h: the kernels' own text of everything one thread computes alone, compiled for the host

struct Pose {
    double R[9], t[3];
    int planar, gnEvals, gnExit;
};

struct Corr {
    std::vector<double> X, f, nr, ns;   // [N][3]
    std::vector<float> p2d, x32, maxErr;
};

// the fixed Jacobi sequence on the symmetric n x n M (n = 12 or 9, stride 12): M becomes (nearly) diagonal, V its eigenvectors
static void jacobi_rounds(double (*M)[12], double (*V)[12], int n)
{
    const int np = n == 12 ? 6 : 4, nr = n == 12 ? 11 : 9, sweeps = n == 12 ? kMlpnpSweeps : kTwoViewSweeps;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < sweeps; sweep++)
        for (int r = 0; r < nr; r++) {
            int P[6], Q[6], skip[6];
            double c[6], s[6];
            for (int e = 0; e < np; e++) {  // the angles, from M as it stands at the start of the round
                jacobi_round_pair(n, r, e, P[e], Q[e]);
                const double apq = M[P[e]][Q[e]];
                skip[e] = apq == 0.0;
                c[e] = 1.0; s[e] = 0.0;
                if (!skip[e]) jacobi_angle(M[P[e]][P[e]], M[Q[e]][Q[e]], apq, c[e], s[e]);
            }
            for (int e = 0; e < np; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < n; k++) {
                    const double a = M[k][P[e]], b = M[k][Q[e]];
                    M[k][P[e]] = c[e] * a - s[e] * b;
                    M[k][Q[e]] = s[e] * a + c[e] * b;
                }
            }
            for (int e = 0; e < np; e++) {
                if (skip[e]) continue;
                for (int k = 0; k < n; k++) {
                    const double a = M[P[e]][k], b = M[Q[e]][k];
                    M[P[e]][k] = c[e] * a - s[e] * b;
                    M[Q[e]][k] = s[e] * a + c[e] * b;
                    const double va = V[k][P[e]], vb = V[k][Q[e]];
                    V[k][P[e]] = c[e] * va - s[e] * vb;
                    V[k][Q[e]] = s[e] * va + c[e] * vb;
                }
            }
        }
}

// computePose (:355-657) on the points idx[0 .. n-1]
static void compute_pose(const Corr& C, const int* idx, int n, Pose& out)
{
    double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double acc = 0.0;
            for (int p = 0; p < n; p++) acc = acc + C.X[3 * (size_t)idx[p] + i] * C.X[3 * (size_t)idx[p] + j];
            G[3 * i + j] = acc;
        }
    double lam[3], E[3][3], eigenRot[9];
    int order[3];
    eig3_sorted(G, false, lam, E, order);
    double mx = fabs(lam[0]);
    for (int i = 1; i < 3; i++) mx = fabs(lam[i]) > mx ? fabs(lam[i]) : mx;
    int rank = 0;
    for (int i = 0; i < 3; i++) rank += fabs(lam[i]) > kRankTol * mx;
    const bool planar = rank == 2;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) eigenRot[3 * i + j] = E[j][order[i]];
    const int nc = planar ? 9 : 12;
    std::vector<double> A((size_t)2 * n * 12, 0.0);
    for (int p = 0; p < n; p++) {
        const double* X = &C.X[3 * (size_t)idx[p]];
        double P3[3];
        matvec3(eigenRot, X, P3);
        for (int h = 0; h < 2; h++) {
            const double* nv = h ? &C.ns[3 * (size_t)idx[p]] : &C.nr[3 * (size_t)idx[p]];
            double* row = &A[(size_t)(2 * p + h) * 12];
            for (int i = 0; i < 3; i++) {
                if (!planar) {
                    for (int j = 0; j < 3; j++) row[3 * i + j] = nv[i] * X[j];
                    row[9 + i] = nv[i];
                } else {
                    row[2 * i] = nv[i] * P3[1];
                    row[2 * i + 1] = nv[i] * P3[2];
                    row[6 + i] = nv[i];
                }
            }
        }
    }
    double M[12][12], V[12][12];
    for (int i = 0; i < nc; i++)
        for (int j = 0; j < nc; j++) {
            double acc = 0.0;
            for (int k = 0; k < 2 * n; k++) acc = acc + A[(size_t)k * 12 + i] * A[(size_t)k * 12 + j];
            M[i][j] = acc;
        }
    jacobi_rounds(M, V, nc);
    int bi = 0;
    for (int i = 1; i < nc; i++)
        if (M[i][i] < M[bi][bi]) bi = i;
    double res[12];
    for (int k = 0; k < 12; k++) res[k] = k < nc ? V[k][bi] : 0.0;
    double X6[6][3], f6[6][3];
    for (int p = 0; p < 6; p++)
        for (int k = 0; k < 3; k++) { X6[p][k] = C.X[3 * (size_t)idx[p] + k]; f6[p][k] = C.f[3 * (size_t)idx[p] + k]; }
    double R0[9], t0[3];
    if (!planar) {
        double tmp[9], cn[3];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) tmp[3 * i + j] = res[3 * j + i];
        for (int j = 0; j < 3; j++) cn[j] = sqrt((tmp[j] * tmp[j] + tmp[3 + j] * tmp[3 + j]) + tmp[6 + j] * tmp[6 + j]);
        const double scale = 1.0 / spec_cbrt64(fabs((cn[0] * cn[1]) * cn[2]));
        double Rp[9], ts[3], tt[3], tinv[3], err[2];
        polar3(tmp, Rp);
        for (int i = 0; i < 3; i++) ts[i] = scale * res[9 + i];
        matvec3(Rp, ts, tt);
        transpose3d(Rp, R0);
        matvec3(R0, tt, tinv);
        for (int i = 0; i < 3; i++) tinv[i] = -tinv[i];
        for (int s = 0; s < 2; s++) {
            double e = 0.0;
            for (int p = 0; p < 6; p++) {
                double v[3];
                matvec3(R0, X6[p], v);
                for (int i = 0; i < 3; i++) v[i] = v[i] + (s ? -tinv[i] : tinv[i]);
                const double nv = norm3(v);
                for (int i = 0; i < 3; i++) v[i] = v[i] / nv;
                e = e + (1.0 - dot3(v, f6[p]));
            }
            err[s] = e;
        }
        for (int i = 0; i < 3; i++) t0[i] = err[0] < err[1] ? tinv[i] : -tinv[i];
    } else {
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
        for (int c = 0; c < 4; c++) {
            const double* Rc = c < 2 ? R1 : R2;
            double val = 0.0;
            for (int p = 0; p < 6; p++) {
                double v[3];
                matvec3(Rc, X6[p], v);
                for (int i = 0; i < 3; i++) v[i] = v[i] + ((c & 1) ? -t[i] : t[i]);
                const double nv = norm3(v);
                for (int i = 0; i < 3; i++) v[i] = v[i] / nv;
                val = val + (1.0 - dot3(v, f6[p]));
            }
            if (c == 0 || val < best) {
                best = val;
                for (int k = 0; k < 9; k++) R0[k] = Rc[k];
                for (int i = 0; i < 3; i++) t0[i] = (c & 1) ? -t[i] : t[i];
            }
        }
    }
    double x[6];
    rot2rodrigues(R0, x);
    for (int i = 0; i < 3; i++) x[3 + i] = t0[i];
    out.gnEvals = 0;
    out.gnExit = 0;
    std::vector<double> J((size_t)2 * n * 6), r((size_t)2 * n);
    for (int it = 0; it < 5; it++) {
        double R[9], D[3][9];
        rodrigues2rot(x, R, D);
        for (int p = 0; p < n; p++)
            point_rows(R, D, x + 3, &C.X[3 * (size_t)idx[p]], &C.nr[3 * (size_t)idx[p]], &C.ns[3 * (size_t)idx[p]], &J[(size_t)12 * p], r[(size_t)2 * p],
                       &J[(size_t)12 * p + 6], r[(size_t)2 * p + 1]);
        double A6[6][6], g6[6], dx[6];
        for (int i = 0; i < 6; i++) {
            for (int j = 0; j < 6; j++) {
                double acc = 0.0;
                for (int k = 0; k < 2 * n; k++) acc = acc + J[(size_t)6 * k + i] * J[(size_t)6 * k + j];
                A6[i][j] = acc;
            }
            double acc = 0.0;
            for (int k = 0; k < 2 * n; k++) acc = acc + J[(size_t)6 * k + i] * r[(size_t)k];
            g6[i] = acc;
        }
        ldlt_solve6(A6, g6, dx);
        out.gnEvals++;
        double mxd = fabs(dx[0]), mnd = fabs(dx[0]);
        for (int i = 1; i < 6; i++) {
            mxd = fabs(dx[i]) > mxd ? fabs(dx[i]) : mxd;
            mnd = fabs(dx[i]) < mnd ? fabs(dx[i]) : mnd;
        }
        if (mxd > 5.0 || mnd > 1.0) { out.gnExit = 1; break; }
        double maxDl = 0.0;
        for (int k = 0; k < 2 * n; k++) {
            const double* Jk = &J[(size_t)6 * k];
            const double dl = fabs(((((Jk[0] * dx[0] + Jk[1] * dx[1]) + Jk[2] * dx[2]) + Jk[3] * dx[3]) + Jk[4] * dx[4]) + Jk[5] * dx[5]);
            if (k == 0) maxDl = dl;
            else if (dl > maxDl) maxDl = dl;
        }
        for (int i = 0; i < 6; i++) x[i] = x[i] - dx[i];
        if (maxDl < 1e-5) { out.gnExit = 2; break; }
    }
    rodrigues2rot(x, out.R, nullptr);
    for (int i = 0; i < 3; i++) out.t[i] = x[3 + i];
    out.planar = planar ? 1 : 0;
}

struct Result {
    int solved = 0, nInliers = 0, noMore = 1, N = 0, minInliers = 0, maxIts = 0, total = 0, exitKind = 0, retIt = -1, nCand = 0;
    float Tcw[16];
    std::vector<uint8_t> inliers;
    std::vector<double> hypRt, candRt;
    std::vector<int> hypInl, hypPlanar, hypEvals, hypExit, cands, candInl, candPlanar;
    std::vector<uint8_t> candMask;
};

static int check_inliers(const orbfe_mlpnp_params& P, const Corr& C, int N, const Pose& T, uint8_t* mask)
{
    const CamP cam = cam_of(P.cam, P.camera_model);
    int cnt = 0;
    for (int m = 0; m < N; m++) {
        const float X = C.x32[3 * (size_t)m], Y = C.x32[3 * (size_t)m + 1], Z = C.x32[3 * (size_t)m + 2];
        const float xc = (float)(((T.R[0] * (double)X + T.R[1] * (double)Y) + T.R[2] * (double)Z) + T.t[0]);
        const float yc = (float)(((T.R[3] * (double)X + T.R[4] * (double)Y) + T.R[5] * (double)Z) + T.t[1]);
        const float zc = (float)(((T.R[6] * (double)X + T.R[7] * (double)Y) + T.R[8] * (double)Z) + T.t[2]);
        float u, v;
        camera_project(cam, xc, yc, zc, u, v);
        const float distX = C.p2d[2 * (size_t)m] - u;
        const float distY = C.p2d[2 * (size_t)m + 1] - v;
        const float error2 = distX * distX + distY * distY;
        mask[m] = error2 < C.maxErr[(size_t)m];
        cnt += mask[m];
    }
    return cnt;
}

static void ransac(const orbfe_mlpnp_params& P, const float* sigma2, const std::vector<KeyPoint>& kp, const std::vector<int>& mpIndex,
                   const std::vector<float>& points, const int* sets, Result& o)
{
    const int n = (int)kp.size();
    std::vector<int> first;
    for (int i = 0; i < n; i++)
        if (mpIndex[(size_t)i] >= 0) first.push_back(i);
    const int N = (int)first.size();
    o = Result();
    o.N = N;
    for (int i = 0; i < 16; i++) o.Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    o.inliers.assign((size_t)n, 0);
    orbfe_mlpnp_plan(&P, N, &o.minInliers, &o.maxIts, &o.total);
    if (o.total == 0) return;
    const int total = o.total, ms = P.min_set;
    Corr C;
    C.X.resize((size_t)3 * N); C.f.resize((size_t)3 * N); C.nr.resize((size_t)3 * N); C.ns.resize((size_t)3 * N);
    C.p2d.resize((size_t)2 * N); C.x32.resize((size_t)3 * N); C.maxErr.resize((size_t)N);
    const CamP cam = cam_of(P.cam, P.camera_model);
    for (int c = 0; c < N; c++) {
        const KeyPoint& k = kp[(size_t)first[(size_t)c]];
        const float* X = &points[(size_t)3 * mpIndex[(size_t)first[(size_t)c]]];
        float rx, ry;
        cam_unproject(cam, P.kb_precision, k.pt.x, k.pt.y, rx, ry);
        const double f[3] = {(double)rx, (double)ry, 1.0};
        const double nrm = norm3(f);
        const double alpha = f[0] >= 0.0 ? -nrm : nrm;
        const double v[3] = {f[0] - alpha, f[1], f[2]};
        const double beta = 2.0 / dot3(v, v);
        for (int j = 0; j < 3; j++) {
            const double w = beta * v[j];
            C.f[3 * (size_t)c + j] = f[j];
            C.nr[3 * (size_t)c + j] = (j == 1 ? 1.0 : 0.0) - w * v[1];
            C.ns[3 * (size_t)c + j] = (j == 2 ? 1.0 : 0.0) - w * v[2];
            C.X[3 * (size_t)c + j] = (double)X[j];
            C.x32[3 * (size_t)c + j] = X[j];
        }
        C.p2d[2 * (size_t)c] = k.pt.x; C.p2d[2 * (size_t)c + 1] = k.pt.y;
        C.maxErr[(size_t)c] = sigma2[k.octave] * P.th2;
    }
    o.hypRt.assign((size_t)total * 12, 0.0);
    o.hypInl.assign((size_t)total, 0); o.hypPlanar.assign((size_t)total, 0); o.hypEvals.assign((size_t)total, 0); o.hypExit.assign((size_t)total, 0);
    o.exitKind = ORBFE_MLPNP_EXIT_FAILED;
    std::vector<uint8_t> mask((size_t)N), bestMask((size_t)N), refMask((size_t)N);
    std::vector<int> sel;
    int best = 0, winner = -1, last = -1;
    Pose winPose, lastPose;
    for (int it = 0; it < total; it++) {  // (:116-203); every hypothesis is evaluated so that the whole info block can be compared
        Pose T;
        compute_pose(C, sets + (size_t)it * ms, ms, T);
        const int cnt = check_inliers(P, C, N, T, mask.data());
        std::memcpy(&o.hypRt[(size_t)it * 12], T.R, sizeof T.R);
        std::memcpy(&o.hypRt[(size_t)it * 12 + 9], T.t, sizeof T.t);
        o.hypInl[(size_t)it] = cnt; o.hypPlanar[(size_t)it] = T.planar; o.hypEvals[(size_t)it] = T.gnEvals; o.hypExit[(size_t)it] = T.gnExit;
        if (!(cnt >= o.minInliers && cnt > best)) continue;  // a qualifying hypothesis that sets no new best re-runs a Refine that failed
        best = cnt;
        sel.clear();
        for (int m = 0; m < N; m++)
            if (mask[(size_t)m]) sel.push_back(m);
        Pose Rf;
        compute_pose(C, sel.data(), (int)sel.size(), Rf);
        const int rc = check_inliers(P, C, N, Rf, refMask.data());
        o.cands.push_back(it);
        o.candRt.insert(o.candRt.end(), Rf.R, Rf.R + 9);
        o.candRt.insert(o.candRt.end(), Rf.t, Rf.t + 3);
        o.candInl.push_back(rc); o.candPlanar.push_back(Rf.planar);
        o.candMask.insert(o.candMask.end(), refMask.begin(), refMask.end());
        last = it; lastPose = T; bestMask = mask;
        if (winner < 0 && rc > o.minInliers) {
            winner = it; winPose = Rf;
            o.nInliers = rc;
            for (int m = 0; m < N; m++) o.inliers[(size_t)first[(size_t)m]] = refMask[(size_t)m];
        }
    }
    o.nCand = (int)o.cands.size();
    const Pose* ret = nullptr;
    if (winner >= 0) { o.exitKind = ORBFE_MLPNP_EXIT_REFINED; o.retIt = winner; o.noMore = 0; ret = &winPose; }
    else if (last >= 0) {
        o.exitKind = ORBFE_MLPNP_EXIT_BEST_UNREFINED; o.retIt = last; ret = &lastPose;
        o.nInliers = best;
        for (int m = 0; m < N; m++) o.inliers[(size_t)first[(size_t)m]] = bestMask[(size_t)m];
    }
    if (!ret) return;
    o.solved = 1;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) o.Tcw[4 * i + j] = (float)ret->R[3 * i + j];
        o.Tcw[4 * i + 3] = (float)ret->t[i];
    }
}

}  // namespace s13

template <class T>
static void put(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

static void write_result(const char* path, const s13::Result& r)
{
    std::ofstream f(path, std::ios::binary);
    const int head[10] = {r.solved, r.nInliers, r.noMore, r.N, r.minInliers, r.maxIts, r.total, r.exitKind, r.retIt, r.nCand};
    put(f, head, 10); put(f, r.Tcw, 16); put(f, r.inliers.data(), r.inliers.size());
    put(f, r.hypRt.data(), r.hypRt.size()); put(f, r.hypInl.data(), r.hypInl.size()); put(f, r.hypPlanar.data(), r.hypPlanar.size());
    put(f, r.hypEvals.data(), r.hypEvals.size()); put(f, r.hypExit.data(), r.hypExit.size()); put(f, r.cands.data(), r.cands.size());
    put(f, r.candRt.data(), r.candRt.size()); put(f, r.candInl.data(), r.candInl.size()); put(f, r.candPlanar.data(), r.candPlanar.size());
    put(f, r.candMask.data(), r.candMask.size());
}

static int same(const s13::Result& a, const s13::Result& b)
{
    auto eq = [](const auto& x, const auto& y) { return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0]))); };
    return a.solved == b.solved && a.nInliers == b.nInliers && a.noMore == b.noMore && a.N == b.N && a.minInliers == b.minInliers &&
           a.maxIts == b.maxIts && a.total == b.total && a.exitKind == b.exitKind && a.retIt == b.retIt && a.nCand == b.nCand &&
           !std::memcmp(a.Tcw, b.Tcw, sizeof a.Tcw) && eq(a.inliers, b.inliers) && eq(a.hypRt, b.hypRt) && eq(a.hypInl, b.hypInl) &&
           eq(a.hypPlanar, b.hypPlanar) && eq(a.hypEvals, b.hypEvals) && eq(a.hypExit, b.hypExit) && eq(a.cands, b.cands) &&
           eq(a.candRt, b.candRt) && eq(a.candInl, b.candInl) && eq(a.candPlanar, b.candPlanar) && eq(a.candMask, b.candMask);
}

template <class F>
static double median_us(int reps, F&& fn)
{
    std::vector<double> t;
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main(int argc, char** argv)
{
    if (argc == 6 && !std::strcmp(argv[1], "drawsets")) {  // drawsets seed N total minSet: the min-sets a process draws after srand(seed); no GPU
        const int N = std::atoi(argv[3]), total = std::atoi(argv[4]), minSet = std::atoi(argv[5]);
        if (minSet < 1 || N < minSet || total < 1) return 2;
        srand((unsigned)std::atoi(argv[2]));  // MLPnPsolver never seeds: in the reference TwoViewReconstruction's SeedRandOnce(0) came before it
        const std::vector<int> sets = MLPnPsolver::DrawSets(N, total, minSet);
        for (int it = 0; it < total; it++)
            for (int j = 0; j < minSet; j++) std::printf("%d%c", sets[(size_t)it * minSet + j], j == minSet - 1 ? '\n' : ' ');
        return 0;
    }
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream in(argv[1], std::ios::binary);
    int head[9];
    double prob;
    float fl[11];
    in.read(reinterpret_cast<char*>(head), sizeof head);
    in.read(reinterpret_cast<char*>(&prob), sizeof prob);
    in.read(reinterpret_cast<char*>(fl), sizeof fl);
    const int n = head[0], nPoints = head[1], total = head[2], minSet = head[3], nLevels = head[5];
    if (!in || n < 0 || nPoints < 0 || total < 0 || total > 4096 || minSet < 6 || minSet > 64 || nLevels < 1 || nLevels > 32) {
        std::fprintf(stderr, "bad scene header\n");
        return 2;
    }
    float sigma2[32] = {0};
    in.read(reinterpret_cast<char*>(sigma2), (std::streamsize)(nLevels * 4));
    std::vector<KeyPoint> kp((size_t)n);
    std::vector<int> mpIndex((size_t)n), sets((size_t)total * minSet);
    std::vector<float> points((size_t)nPoints * 3);
    in.read(reinterpret_cast<char*>(kp.data()), (std::streamsize)(kp.size() * sizeof(KeyPoint)));
    in.read(reinterpret_cast<char*>(mpIndex.data()), (std::streamsize)(mpIndex.size() * 4));
    in.read(reinterpret_cast<char*>(points.data()), (std::streamsize)(points.size() * 4));
    in.read(reinterpret_cast<char*>(sets.data()), (std::streamsize)(sets.size() * 4));
    if (!in) { std::fprintf(stderr, "short scene file\n"); return 2; }
    orbfe_mlpnp_params P = ORBFE_MLPNP_PARAMS_INIT;
    P.camera_model = head[4];
    for (int i = 0; i < 8; i++) P.cam[i] = fl[i];
    P.kb_precision = fl[8]; P.epsilon = fl[9]; P.th2 = fl[10];
    P.probability = prob; P.min_inliers = head[6]; P.max_iterations = head[7]; P.n_iterations = head[8]; P.min_set = minSet;

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = argc > 3 && !hostOnly ? std::max(std::atoi(argv[3]), 1) : 1;
    s13::Result host;
    s13::ransac(P, sigma2, kp, mpIndex, points, sets.data(), host);
    if (host.total != total) { std::fprintf(stderr, "the scene holds %d sets, the plan asks for %d\n", total, host.total); return 2; }
    if (hostOnly) {
        write_result(argv[2], host);
        std::printf("mlpnp host N=%d total=%d solved=%d exit=%d it=%d\n", host.N, host.total, host.solved, host.exitKind, host.retIt);
        return 0;
    }

    ORBextractor ex(500, 20000, 1.2f, nLevels, 20, 7, 320, 240);  // the handle (its mvLevelSigma2); the extractor itself is not used
    std::vector<std::array<float, 3>> world((size_t)nPoints);
    for (int i = 0; i < nPoints; i++) world[(size_t)i] = {points[(size_t)3 * i], points[(size_t)3 * i + 1], points[(size_t)3 * i + 2]};
    std::vector<const std::array<float, 3>*> matched((size_t)n, nullptr);
    for (int i = 0; i < n; i++)
        if (mpIndex[(size_t)i] >= 0) matched[(size_t)i] = &world[(size_t)mpIndex[(size_t)i]];
    std::array<float, 8> camArr;
    for (int i = 0; i < 8; i++) camArr[(size_t)i] = fl[i];
    s13::Result lib;
    auto call = [&](bool withInfo) {
        MLPnPsolver solver(ex, kp, matched, P.camera_model, camArr, P.kb_precision);
        solver.SetRansacParameters(P.probability, P.min_inliers, P.max_iterations, P.min_set, P.epsilon, P.th2);
        bool noMore = false;
        std::vector<bool> vbInliers;
        int nInliers = 0;
        std::array<float, 16> Tout{};
        orbfe_mlpnp_info info;
        std::memset(&info, 0, sizeof info);
        info.struct_size = (int)sizeof info;
        const int N = solver.correspondences();
        std::vector<uint8_t> hypPlanar((size_t)total + 1), candPlanar((size_t)total + 1);
        if (withInfo) {
            lib = s13::Result();
            lib.hypRt.assign((size_t)total * 12, 0.0); lib.hypInl.assign((size_t)total, 0); lib.hypEvals.assign((size_t)total, 0);
            lib.hypExit.assign((size_t)total, 0); lib.cands.assign((size_t)total + 1, 0); lib.candRt.assign((size_t)(total + 1) * 12, 0.0);
            lib.candInl.assign((size_t)total + 1, 0); lib.candMask.assign((size_t)(total + 1) * (N + 1), 0);
            info.hyp_Rt = lib.hypRt.data(); info.hyp_inliers = lib.hypInl.data(); info.hyp_planar = hypPlanar.data();
            info.hyp_gn_evals = lib.hypEvals.data(); info.hyp_gn_exit = lib.hypExit.data(); info.candidates = lib.cands.data();
            info.cand_Rt = lib.candRt.data(); info.cand_inliers = lib.candInl.data(); info.cand_planar = candPlanar.data();
            info.cand_mask = lib.candMask.data();
        }
        const bool ok = solver.iterate(P.n_iterations, noMore, vbInliers, nInliers, Tout, withInfo ? &info : nullptr, &sets);
        if (!withInfo) return;
        lib.solved = ok; lib.nInliers = nInliers; lib.noMore = noMore; lib.N = info.N; lib.minInliers = info.min_inliers; lib.maxIts = info.max_its;
        lib.total = info.total_iterations; lib.exitKind = info.exit_kind; lib.retIt = info.returning_iteration; lib.nCand = info.n_candidates;
        std::memcpy(lib.Tcw, Tout.data(), sizeof lib.Tcw);
        lib.inliers.assign((size_t)n, 0);
        for (size_t i = 0; i < vbInliers.size(); i++) lib.inliers[i] = vbInliers[i];
        lib.hypPlanar.assign(hypPlanar.begin(), hypPlanar.begin() + total);
        lib.cands.resize((size_t)lib.nCand); lib.candRt.resize((size_t)lib.nCand * 12); lib.candInl.resize((size_t)lib.nCand);
        lib.candPlanar.assign(candPlanar.begin(), candPlanar.begin() + lib.nCand);
        lib.candMask.resize((size_t)lib.nCand * N);
    };
    call(true);
    write_result(argv[2], lib);
    const int hostSame = same(lib, host);
    // a second iterate() on one solver is refused
    int refused = 0;
    {
        MLPnPsolver solver(ex, kp, matched, P.camera_model, camArr, P.kb_precision);
        solver.SetRansacParameters(P.probability, P.min_inliers, P.max_iterations, P.min_set, P.epsilon, P.th2);
        bool nm; std::vector<bool> vb; int ni; std::array<float, 16> T{};
        solver.iterate(P.n_iterations, nm, vb, ni, T, nullptr, &sets);
        try { solver.iterate(P.n_iterations, nm, vb, ni, T, nullptr, &sets); } catch (const std::logic_error&) { refused = 1; }
    }
    cpu_set_t one;
    CPU_ZERO(&one);
    CPU_SET(sched_getcpu(), &one);
    sched_setaffinity(0, sizeof one, &one);
    const double tCall = median_us(reps, [&] { call(false); });
    s13::Result tmp;
    const double tHost = median_us(reps, [&] { s13::ransac(P, sigma2, kp, mpIndex, points, sets.data(), tmp); });
    std::printf("mlpnp N=%d total=%d solved=%d exit=%d it=%d candidates=%d\n", lib.N, lib.total, lib.solved, lib.exitKind, lib.retIt, lib.nCand);
    std::printf("mlpnp_latency_us call=%.1f host_one_thread=%.1f host_same=%d second_iterate_refused=%d\n", tCall, tHost, hostSame, refused);
    return hostSame && refused ? 0 : 1;
}

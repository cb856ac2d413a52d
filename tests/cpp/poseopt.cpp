// Optimizer::PoseOptimization (src/Optimizer.cc:765-1067) from a plain C++ program, two ways on the same inputs:
//   (a) the library through include/orbfe_adaptor.hpp's PoseOptimizer::PoseOptimization wrapper (orbfe_pose_optimization),
//   (b) SPEC DECISION S14 as a single-thread host loop (this file, -O2 -ffp-contract=off, one pinned core).
// (b) is the kernel's arithmetic for one CPU thread, so it is the latency yardstick, not an independent oracle -- that is
// tests/poseopt_ref.py.  Shared with the kernel, as the same text compiled for the host (-I csrc): the edge arithmetic and the pose
// update (poseopt_math.h), the 3 x 3 products (mat3d.h), sin / cos (spec_math.h), the 6 x 6 solve (ldlt.h).  Restated here: only the
// one-thread ordering of what the block does in csrc/kernels_poseopt.hip -- the tree sums, walked with a binary-counter stack over all
// P slots (the same additions as the kernel's tree), and the Levenberg loop around them.  Its results must equal the library's bit for
// bit (host_same=1), and tests/test_poseopt_cpp.py compares them with the numpy restatement without a GPU.
//   usage: poseopt                                   -> library version (link test)
//          poseopt <scene.bin> <out.bin> host [reps] -> (b) only, its results to out.bin: no GPU needed; with reps, the median
//          poseopt <scene.bin> <out.bin> [reps]      -> (a) and (b); results of (a) to out.bin; medians of `reps` calls
// scene.bin: int32 n, n_points, n_levels, iterations, rounds; float64 huber_delta2; float32 cam[8], chi2_threshold,
//            inv_level_sigma2[n_levels], Rcw[9], tcw[3]; keypoints (24 B each); int32 mp_index[n]; float32 points[n_points][3]
// out.bin:   int32 n_inliers, N_e, rounds_run, iterations[4], trials[4], n_bad[4], exit_kind[4]; float32 Tcw[16]; uint8 outlier[n];
//            float64 pose[4][12], lambda[4], chi2[4]; uint8 round_outlier[4][N_e]
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>

#include <sched.h>

#include "orbfe_adaptor.hpp"
#include "ldlt.h"
#include "poseopt_math.h"

// The translation unit that binds src/Tracking.cc:869,935 keeps including the reference's Optimizer.h for its other entry points
// (:698, :946, :952): a class of that name must compile beside the adaptor.
namespace ORB_SLAM3 {
class Optimizer {
public:
    static int PoseInertialOptimizationLastFrame() { return 0; }
};
}  // namespace ORB_SLAM3

using namespace ORB_SLAM3;

namespace s14 {

using namespace orbfe;   // csrc/ldlt.h, mat3d.h, spec_math.h, poseopt_math.h: the kernel's own text of what one thread computes for one edge

constexpr int kTrials = 10, kStack = 17;

struct Problem {
    PoseCam cam;
    float chi2Thr;
    int iterations, rounds;
    std::vector<EdgeD> E;
    std::vector<int> kpOf;
    std::vector<uint8_t> active;
    int P;
};

// T(v) over the P slots: v(2i) + v(2i + 1) first, then pairs of pairs (a binary counter over the slot index)
template <int NV, class Term>
static void tree(int P, double (&out)[NV], Term term)
{
    double st[kStack][NV];
    for (int i = 0; i < P; i++) {
        term(i, out);
        int lvl = 0;
        for (int m = i; m & 1; m >>= 1, lvl++)
            for (int k = 0; k < NV; k++) out[k] = st[lvl][k] + out[k];
        if (i + 1 < P)
            for (int k = 0; k < NV; k++) st[lvl][k] = out[k];
    }
}

struct Result {
    int nInliers = 0, Ne = 0, roundsRun = 0;
    int iterations[4] = {0, 0, 0, 0}, trials[4] = {0, 0, 0, 0}, nBad[4] = {0, 0, 0, 0}, exitKind[4] = {0, 0, 0, 0};
    float Tcw[16];
    std::vector<uint8_t> outlier;
    double pose[4][12], lambda[4], chi2[4];
    std::vector<uint8_t> roundOutlier;
};

static void run(Problem& G, const float* Rcw, const float* tcw, int n, Result& out)
{
    const int Ne = (int)G.E.size();
    out = Result();
    std::memset(out.pose, 0, sizeof out.pose);
    std::memset(out.lambda, 0, sizeof out.lambda);
    std::memset(out.chi2, 0, sizeof out.chi2);
    out.Ne = Ne;
    out.outlier.assign((size_t)n, 0);
    out.roundOutlier.assign((size_t)4 * Ne, 0);
    for (int i = 0; i < 16; i++) out.Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out.Tcw[4 * i + j] = Rcw[3 * i + j];
        out.Tcw[4 * i + 3] = tcw[i];
    }
    if (Ne < 3) return;
    int P = 1;
    while (P < Ne) P <<= 1;
    G.P = P;
    G.active.assign((size_t)Ne, 1);
    double R0[9], t0[3], R[9] = {0.0}, t[3] = {0.0};
    for (int i = 0; i < 9; i++) R0[i] = (double)Rcw[i];
    for (int i = 0; i < 3; i++) t0[i] = (double)tcw[i];
    int nBadLast = 0;
    for (int rnd = 0; rnd < G.rounds; rnd++) {
        const bool huber = rnd <= 2;
        for (int i = 0; i < 9; i++) R[i] = R0[i];
        for (int i = 0; i < 3; i++) t[i] = t0[i];
        double lam = 0.0, ni = 2.0, cur = 0.0;
        int nIt = 0, nTr = 0, exitKind = ORBFE_POSE_OPT_EXIT_RAN_ALL;
        for (int it = 0; it < G.iterations; it++) {
            nIt++;
            double acc[kNV];
            tree<kNV>(P, acc, [&](int c, double (&v)[kNV]) {
                if (c < Ne && G.active[(size_t)c]) edge_terms(G.cam, G.E[(size_t)c], R, t, huber, v);
                else
                    for (int q = 0; q < kNV; q++) v[q] = 0.0;
            });
            cur = acc[27];
            double b[6], diag[6];
            {
                int at = 0;
                for (int j = 0; j < 6; j++) {
                    diag[j] = acc[at];
                    at += 6 - j;
                    b[j] = acc[21 + j];
                }
            }
            if (it == 0) {
                double m = 0.0;
                for (int j = 0; j < 6; j++)
                    if (std::fabs(diag[j]) > m) m = std::fabs(diag[j]);
                lam = 1e-5 * m;
                ni = 2.0;
            }
            double rho = 0.0;
            int q = 0;
            while (q < kTrials) {
                double A[6][6], dx[6];
                {
                    int at = 0;
                    for (int j = 0; j < 6; j++)
                        for (int k = j; k < 6; k++) {
                            A[j][k] = acc[at];
                            A[k][j] = acc[at];
                            at++;
                        }
                    for (int j = 0; j < 6; j++) A[j][j] = diag[j] + lam;
                }
                bool ok;
                ldlt_solve6(A, b, dx, &ok);
                double Rn[9], tn[3];
                apply_update(dx, R, t, Rn, tn);
                double one[1];
                tree<1>(P, one, [&](int c, double (&v)[1]) {
                    v[0] = 0.0;
                    if (c < Ne && G.active[(size_t)c]) {
                        double x, y, z, e0, e1, chi2, rho0, rho1;
                        edge_residual(G.cam, G.E[(size_t)c], Rn, tn, x, y, z, e0, e1, chi2);
                        robust(chi2, G.cam.delta, huber, rho0, rho1);
                        v[0] = rho0;
                    }
                });
                double tmp = one[0];
                if (!ok) tmp = DBL_MAX;
                double scale = 0.0;
                for (int j = 0; j < 6; j++) scale = scale + dx[j] * (lam * dx[j] + b[j]);
                scale = scale + 1e-3;
                rho = (cur - tmp) / scale;
                nTr++;
                q++;
                if (rho > 0.0 && std::fabs(tmp) <= DBL_MAX) {
                    for (int i = 0; i < 9; i++) R[i] = Rn[i];
                    for (int i = 0; i < 3; i++) t[i] = tn[i];
                    const double tt = 2.0 * rho - 1.0;
                    const double alpha = 1.0 - (tt * tt) * tt;
                    double sf = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;
                    sf = (1.0 / 3.0) < sf ? sf : (1.0 / 3.0);
                    lam = lam * sf;
                    ni = 2.0;
                    cur = tmp;
                } else {
                    lam = lam * ni;
                    ni = ni * 2.0;
                }
                if (!(rho < 0.0)) break;
            }
            if (q == kTrials) { exitKind = ORBFE_POSE_OPT_EXIT_TRIALS; break; }
            if (rho == 0.0) { exitKind = ORBFE_POSE_OPT_EXIT_RHO_ZERO; break; }
        }
        int nBad = 0;
        for (int c = 0; c < Ne; c++) {
            double x, y, z, e0, e1, chi2;
            edge_residual(G.cam, G.E[(size_t)c], R, t, x, y, z, e0, e1, chi2);
            const bool bad = (float)chi2 > G.chi2Thr;
            G.active[(size_t)c] = bad ? 0 : 1;
            out.outlier[(size_t)G.kpOf[(size_t)c]] = bad ? 1 : 0;
            out.roundOutlier[(size_t)rnd * Ne + c] = bad ? 1 : 0;
            nBad += bad ? 1 : 0;
        }
        nBadLast = nBad;
        out.roundsRun = rnd + 1;
        out.iterations[rnd] = nIt;
        out.trials[rnd] = nTr;
        out.nBad[rnd] = nBad;
        out.exitKind[rnd] = exitKind;
        for (int i = 0; i < 9; i++) out.pose[rnd][i] = R[i];
        for (int i = 0; i < 3; i++) out.pose[rnd][9 + i] = t[i];
        out.lambda[rnd] = lam;
        out.chi2[rnd] = cur;
        if (Ne < 10) break;
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out.Tcw[4 * i + j] = (float)R[3 * i + j];
        out.Tcw[4 * i + 3] = (float)t[i];
    }
    out.nInliers = Ne - nBadLast;
}

}  // namespace s14

namespace {

struct MapPoint {
    std::array<float, 3> pos;
    std::array<float, 3> GetWorldPos() const { return pos; }
};

struct Frame {
    int mNumKeypoints = 0;
    std::shared_ptr<std::vector<KeyPoint>> mvKeysUn;
    std::vector<std::shared_ptr<MapPoint>> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvuRight;
    void* mpCamera2 = nullptr;
    float Rcw[9], tcw[3];
    float Tcw[16];
};

template <class T>
void rd(std::ifstream& f, T* p, size_t n)
{
    f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T)));
}

template <class T>
void wr(std::ofstream& f, const T* p, size_t n)
{
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

void write_result(const char* path, const s14::Result& r, int n)
{
    std::ofstream f(path, std::ios::binary);
    const int head[3] = {r.nInliers, r.Ne, r.roundsRun};
    wr(f, head, 3);
    wr(f, r.iterations, 4);
    wr(f, r.trials, 4);
    wr(f, r.nBad, 4);
    wr(f, r.exitKind, 4);
    wr(f, r.Tcw, 16);
    wr(f, r.outlier.data(), (size_t)n);
    wr(f, &r.pose[0][0], 48);
    wr(f, r.lambda, 4);
    wr(f, r.chi2, 4);
    wr(f, r.roundOutlier.data(), r.roundOutlier.size());
}

bool same(const s14::Result& a, const s14::Result& b)
{
    return a.nInliers == b.nInliers && a.Ne == b.Ne && a.roundsRun == b.roundsRun && !std::memcmp(a.iterations, b.iterations, 16) &&
           !std::memcmp(a.trials, b.trials, 16) && !std::memcmp(a.nBad, b.nBad, 16) && !std::memcmp(a.exitKind, b.exitKind, 16) &&
           !std::memcmp(a.Tcw, b.Tcw, 64) && a.outlier == b.outlier && !std::memcmp(a.pose, b.pose, sizeof a.pose) &&
           !std::memcmp(a.lambda, b.lambda, 32) && !std::memcmp(a.chi2, b.chi2, 32) && a.roundOutlier == b.roundOutlier;
}

double median(std::vector<double>& v)
{
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int head[5];
    rd(f, head, 5);
    const int n = head[0], nPoints = head[1], nLevels = head[2];
    double delta2;
    rd(f, &delta2, 1);
    float cam[8], thr, Rcw[9], tcw[3];
    rd(f, cam, 8);
    rd(f, &thr, 1);
    std::vector<float> invSigma2((size_t)nLevels);
    rd(f, invSigma2.data(), (size_t)nLevels);
    rd(f, Rcw, 9);
    rd(f, tcw, 3);
    std::vector<KeyPoint> keys((size_t)n);
    static_assert(sizeof(KeyPoint) == 24, "keypoint record");
    rd(f, keys.data(), (size_t)n);
    std::vector<int> mpIndex((size_t)n);
    rd(f, mpIndex.data(), (size_t)n);
    std::vector<float> points((size_t)nPoints * 3);
    rd(f, points.data(), points.size());
    if (!f) { std::fprintf(stderr, "short scene file\n"); return 2; }

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = hostOnly ? (argc > 4 ? std::atoi(argv[4]) : 0) : (argc > 3 ? std::atoi(argv[3]) : 1);

    cpu_set_t set;
    CPU_ZERO(&set);
    CPU_SET(sched_getcpu(), &set);
    sched_setaffinity(0, sizeof set, &set);  // one pinned core

    s14::Problem G;
    G.cam = orbfe::PoseCam{(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3], (double)(float)std::sqrt(delta2)};
    G.chi2Thr = thr;
    G.iterations = head[3];
    G.rounds = head[4];
    s14::Result host;
    auto host_call = [&]() {
        G.E.clear();
        G.kpOf.clear();
        for (int i = 0; i < n; i++) {
            if (mpIndex[(size_t)i] < 0) continue;
            const float* p = &points[3 * (size_t)mpIndex[(size_t)i]];
            G.E.push_back(orbfe::EdgeD{(double)p[0], (double)p[1], (double)p[2], (double)keys[(size_t)i].pt.x, (double)keys[(size_t)i].pt.y,
                                     (double)invSigma2[(size_t)keys[(size_t)i].octave]});
            G.kpOf.push_back(i);
        }
        s14::run(G, Rcw, tcw, n, host);
    };
    host_call();
    std::vector<double> tHost;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        host_call();
        tHost.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    if (hostOnly) {
        write_result(argv[2], host, n);
        std::printf("poseopt_latency_us host_one_thread=%.1f\n", median(tHost));
        return 0;
    }

    // (a) the library through the adaptor
    ORBextractor ex(1000, 16000, 1.2f, nLevels, 20, 7, 752, 480);
    Frame F;
    F.mNumKeypoints = n;
    F.mvKeysUn = std::make_shared<std::vector<KeyPoint>>(keys);
    F.mvpMapPoints.assign((size_t)n, nullptr);
    F.mvbOutlier.assign((size_t)n, false);
    F.mvuRight.assign((size_t)n, -1.0f);
    for (int i = 0; i < n; i++)
        if (mpIndex[(size_t)i] >= 0) {
            const float* p = &points[3 * (size_t)mpIndex[(size_t)i]];
            F.mvpMapPoints[(size_t)i] = std::make_shared<MapPoint>(MapPoint{{p[0], p[1], p[2]}});
        }
    std::memcpy(F.Rcw, Rcw, sizeof Rcw);
    std::memcpy(F.tcw, tcw, sizeof tcw);
    for (int i = 0; i < 16; i++) F.Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) F.Tcw[4 * i + j] = Rcw[3 * i + j];
        F.Tcw[4 * i + 3] = tcw[i];
    }
    std::array<float, 8> camA;
    for (int i = 0; i < 8; i++) camA[(size_t)i] = cam[i];
    auto getPose = [](Frame* fr, float* R, float* t) {
        std::memcpy(R, fr->Rcw, sizeof fr->Rcw);
        std::memcpy(t, fr->tcw, sizeof fr->tcw);
    };
    auto setPose = [](Frame* fr, const float* T) { std::memcpy(fr->Tcw, T, sizeof fr->Tcw); };
    s14::Result lib;
    orbfe_pose_opt_info info;
    std::vector<double> tLib;
    for (int r = 0; r < std::max(reps, 1) + 1; r++) {
        lib = s14::Result();
        lib.roundOutlier.assign((size_t)4 * host.Ne, 0);
        std::memset(&info, 0, sizeof info);
        info.struct_size = (int)sizeof info;
        info.outlier = lib.roundOutlier.data();
        const auto t0 = std::chrono::steady_clock::now();
        lib.nInliers = PoseOptimizer::PoseOptimization(ex, &F, ORBFE_CAMERA_PINHOLE, camA, getPose, setPose, &info);
        if (r > 0) tLib.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    lib.Ne = info.N_e;
    lib.roundsRun = info.rounds_run;
    std::memcpy(lib.iterations, info.iterations, 16);
    std::memcpy(lib.trials, info.trials, 16);
    std::memcpy(lib.nBad, info.n_bad, 16);
    std::memcpy(lib.exitKind, info.exit_kind, 16);
    std::memcpy(lib.pose, info.pose, sizeof lib.pose);
    std::memcpy(lib.lambda, info.lambda, 32);
    std::memcpy(lib.chi2, info.chi2, 32);
    std::memcpy(lib.Tcw, F.Tcw, 64);
    lib.outlier.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) lib.outlier[(size_t)i] = F.mvbOutlier[(size_t)i] ? 1 : 0;
    write_result(argv[2], lib, n);
    std::printf("poseopt_latency_us call=%.1f host_one_thread=%.1f host_same=%d\n", median(tLib), median(tHost), same(lib, host) ? 1 : 0);
    return 0;
}

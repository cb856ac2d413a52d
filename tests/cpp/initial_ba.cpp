// The bundle adjustment of the initial map (src/Tracking.cc:698-729 -> src/Optimizer.cc:60-369) from a plain C++ program, two ways on
// the same inputs:
//   (a) the library through include/orbfe_adaptor.hpp's InitialMapAdjuster::Adjust (orbfe_initial_bundle_adjustment, then the median
//       depth and the rescale on the host),
//   (b) the single-thread host loop of SPEC DECISION S17 below: the work the call takes off the tracking thread, and the yardstick of
//       tests/tools/initial_ba_latency.py.
// Shared with the kernel, as the same text compiled for the host (-I csrc): what one thread computes for one point
// (initial_ba_math.h, poseopt_math.h), the 3 x 3 helpers (mat3d.h), sin / cos (spec_math.h), the 6 x 6 solve (ldlt.h).  Restated here:
// only the one-thread ordering of what the block does in csrc/kernels_initial_ba.hip -- the tree sums, walked with a binary-counter
// stack over all P slots -- and the Levenberg loop around them; the median depth and the rescale are the adaptor's own
// InitialMapAdjuster::MedianDepthScale in both.  Every byte of (a) and (b) must agree (host_same=1), and
// tests/test_initial_ba_cpp.py compares them with the numpy restatement (tests/initial_ba_ref.py) without a GPU.
//   usage: initial_ba                                      -> library version (link test)
//          initial_ba <scene.bin> <out.bin> host [reps]    -> (b) only, its results to out.bin: no GPU needed; with reps, the median
//          initial_ba <scene.bin> <out.bin> [reps]         -> (a) and (b); results of (a) to out.bin; medians of `reps` calls
// scene.bin: int32 n1, n2, n_levels, iterations, robust, inertial; float64 huber_delta2; float32 cam[8], inv_level_sigma2[n_levels],
//            Rcw1[9], tcw1[3], Rcw2[9], tcw2[3]; keypoints 1 (24 B each), keypoints 2; int32 matches12[n1]; float32 points[n1][3]
// out.bin:   int32 N, iterations, trials, exit_kind, it_trials[64]; float32 Tcw2[16], points[n1][3]; float64 cost[64], lambda[64],
//            pose[12], chi2[2][N]; uint8 depth_positive[2][N]; then the adaptor's step: int32 ok; float32 median, tcw2[3], points[n1][3]
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
#include "initial_ba_math.h"

using namespace ORB_SLAM3;

namespace s17 {

using namespace orbfe;   // csrc/ldlt.h, mat3d.h, spec_math.h, poseopt_math.h, initial_ba_math.h: the kernel's own text

constexpr int kTrials = 10, kStack = 17;

struct Problem {
    PoseCam cam;
    int iterations, robust;
    double Ra[9], ta[3], R0[9], t0[3];
    std::vector<BaObs> O;
    std::vector<double> X0;   // [N][3]
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
    int N = 0, iterations = 0, trials = 0, exitKind = 0;
    int itTrials[64];
    float Tcw[16];
    std::vector<float> points;   // [n1][3]
    double cost[64], lambda[64], pose[12];
    std::vector<double> chi2;    // [2][N]
    std::vector<uint8_t> front;  // [2][N]
    // the adaptor's step
    int ok = 0;
    float median = 0.0f, tcw2[3] = {0.0f, 0.0f, 0.0f};
    std::vector<float> scaled;   // [n1][3]
};

// the loop of S17 on the N points of G; X (N x 3) ends as the adjusted positions
static void run(const Problem& G, std::vector<double>& X, Result& out)
{
    const int N = (int)G.O.size();
    std::memset(out.itTrials, 0, sizeof out.itTrials);
    std::memset(out.cost, 0, sizeof out.cost);
    std::memset(out.lambda, 0, sizeof out.lambda);
    out.N = N;
    X = G.X0;
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = G.R0[i];
    for (int i = 0; i < 3; i++) t[i] = G.t0[i];
    out.chi2.assign((size_t)2 * N, 0.0);
    out.front.assign((size_t)2 * N, 0);
    if (N > 0) {
        int P = 1;
        while (P < N) P <<= 1;
        const bool huber = G.robust != 0;
        std::vector<BaPoint> L((size_t)N);
        std::vector<double> Xt((size_t)3 * N);
        double lam = 0.0, ni = 2.0, cur = 0.0;
        int nIt = 0, nTr = 0, exitKind = ORBFE_POSE_OPT_EXIT_RAN_ALL;
        auto at3 = [](std::vector<double>& v, int p) -> double(&)[3] { return *reinterpret_cast<double(*)[3]>(&v[3 * (size_t)p]); };
        for (int it = 0; it < G.iterations; it++) {
            nIt++;
            double acc[kNV], mx = 0.0;
            tree<kNV>(P, acc, [&](int p, double (&v)[kNV]) {
                if (p < N) {
                    ba_build(G.cam, G.O[(size_t)p], G.Ra, G.ta, R, t, at3(X, p), huber, L[(size_t)p], v);
                    mx = ba_diag_max(L[(size_t)p], mx);
                } else
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
                    if (diag[j] > m) m = diag[j];
                if (mx > m) m = mx;
                lam = 1e-5 * m;
                ni = 2.0;
            }
            double rho = 0.0;
            int q = 0;
            while (q < kTrials) {
                double sc[kBaNS];
                tree<kBaNS>(P, sc, [&](int p, double (&v)[kBaNS]) {
                    if (p < N) ba_schur(L[(size_t)p], lam, v);
                    else
                        for (int i = 0; i < kBaNS; i++) v[i] = 0.0;
                });
                double A[6][6], g[6], dx[6];
                {
                    int at = 0;
                    for (int j = 0; j < 6; j++)
                        for (int k = j; k < 6; k++) {
                            const double val = j == k ? (diag[j] + lam) - sc[at] : acc[at] - sc[at];
                            A[j][k] = val;
                            A[k][j] = val;
                            at++;
                        }
                    for (int j = 0; j < 6; j++) g[j] = b[j] - sc[21 + j];
                }
                bool ok;
                ldlt_solve6(A, g, dx, &ok);
                double Rn[9], tn[3];
                apply_update(dx, R, t, Rn, tn);
                double tr[kBaNT] = {0.0, 0.0};
                tree<kBaNT>(P, tr, [&](int p, double (&v)[kBaNT]) {
                    v[0] = 0.0;
                    v[1] = 0.0;
                    if (p < N) {
                        double dp[3];
                        const double(&Xp)[3] = at3(X, p);
                        ba_backsub(L[(size_t)p], lam, dx, dp, v[1]);
                        double(&Xn)[3] = at3(Xt, p);
                        for (int i = 0; i < 3; i++) Xn[i] = Xp[i] + dp[i];
                        v[0] = ba_cost(G.cam, G.O[(size_t)p], G.Ra, G.ta, Rn, tn, Xn, huber);
                    }
                });
                double tmp = tr[0];
                if (!ok) tmp = DBL_MAX;
                double scale = 0.0;
                for (int j = 0; j < 6; j++) scale = scale + dx[j] * ((lam * dx[j]) + b[j]);
                scale = (scale + tr[1]) + 1e-3;
                rho = (cur - tmp) / scale;
                nTr++;
                q++;
                if (rho > 0.0 && std::fabs(tmp) <= DBL_MAX) {
                    for (int i = 0; i < 9; i++) R[i] = Rn[i];
                    for (int i = 0; i < 3; i++) t[i] = tn[i];
                    X = Xt;
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
            out.itTrials[it] = q;
            out.cost[it] = cur;
            out.lambda[it] = lam;
            if (q == kTrials) { exitKind = ORBFE_POSE_OPT_EXIT_TRIALS; break; }
            if (rho == 0.0) { exitKind = ORBFE_POSE_OPT_EXIT_RHO_ZERO; break; }
        }
        for (int p = 0; p < N; p++) {
            bool fa, fb;
            ba_chi2(G.cam, G.O[(size_t)p], G.Ra, G.ta, R, t, at3(X, p), out.chi2[(size_t)p], out.chi2[(size_t)N + p], fa, fb);
            out.front[(size_t)p] = fa ? 1 : 0;
            out.front[(size_t)N + p] = fb ? 1 : 0;
        }
        out.iterations = nIt;
        out.trials = nTr;
        out.exitKind = exitKind;
    }
    for (int i = 0; i < 9; i++) out.pose[i] = R[i];
    for (int i = 0; i < 3; i++) out.pose[9 + i] = t[i];
    for (int i = 0; i < 16; i++) out.Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out.Tcw[4 * i + j] = (float)R[3 * i + j];
        out.Tcw[4 * i + 3] = (float)t[i];
    }
}

}  // namespace s17

namespace {

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

void write_result(const char* path, const s17::Result& r)
{
    std::ofstream f(path, std::ios::binary);
    const int head[4] = {r.N, r.iterations, r.trials, r.exitKind};
    wr(f, head, 4);
    wr(f, r.itTrials, 64);
    wr(f, r.Tcw, 16);
    wr(f, r.points.data(), r.points.size());
    wr(f, r.cost, 64);
    wr(f, r.lambda, 64);
    wr(f, r.pose, 12);
    wr(f, r.chi2.data(), r.chi2.size());
    wr(f, r.front.data(), r.front.size());
    wr(f, &r.ok, 1);
    wr(f, &r.median, 1);
    wr(f, r.tcw2, 3);
    wr(f, r.scaled.data(), r.scaled.size());
}

// every byte, except that two NaNs are equal whatever their payloads (those differ between the host and the GPU)
template <class T>
bool same_values(const T* a, const T* b, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (std::memcmp(&a[i], &b[i], sizeof(T)) && !(a[i] != a[i] && b[i] != b[i])) return false;
    return true;
}

template <class T>
bool same_values(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && same_values(a.data(), b.data(), a.size());
}

bool same(const s17::Result& a, const s17::Result& b)
{
    return a.N == b.N && a.iterations == b.iterations && a.trials == b.trials && a.exitKind == b.exitKind &&
           !std::memcmp(a.itTrials, b.itTrials, sizeof a.itTrials) && same_values(a.Tcw, b.Tcw, 16) && same_values(a.points, b.points) &&
           same_values(a.cost, b.cost, 64) && same_values(a.lambda, b.lambda, 64) && same_values(a.pose, b.pose, 12) &&
           same_values(a.chi2, b.chi2) && a.front == b.front && a.ok == b.ok && same_values(&a.median, &b.median, 1) &&
           same_values(a.tcw2, b.tcw2, 3) && same_values(a.scaled, b.scaled);
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
    int head[6];
    rd(f, head, 6);
    const int n1 = head[0], n2 = head[1], nLevels = head[2];
    const bool inertial = head[5] != 0;
    double delta2;
    rd(f, &delta2, 1);
    float cam[8], Rcw1[9], tcw1[3], Rcw2[9], tcw2[3];
    rd(f, cam, 8);
    std::vector<float> invSigma2((size_t)nLevels);
    rd(f, invSigma2.data(), (size_t)nLevels);
    rd(f, Rcw1, 9);
    rd(f, tcw1, 3);
    rd(f, Rcw2, 9);
    rd(f, tcw2, 3);
    static_assert(sizeof(KeyPoint) == 24, "keypoint record");
    std::vector<KeyPoint> keys1((size_t)n1), keys2((size_t)n2);
    rd(f, keys1.data(), (size_t)n1);
    rd(f, keys2.data(), (size_t)n2);
    std::vector<int> matches((size_t)n1);
    rd(f, matches.data(), (size_t)n1);
    std::vector<float> points((size_t)n1 * 3);
    rd(f, points.data(), points.size());
    if (!f) { std::fprintf(stderr, "short scene file\n"); return 2; }

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = hostOnly ? (argc > 4 ? std::atoi(argv[4]) : 0) : (argc > 3 ? std::atoi(argv[3]) : 1);

    cpu_set_t set;
    CPU_ZERO(&set);
    CPU_SET(sched_getcpu(), &set);
    sched_setaffinity(0, sizeof set, &set);  // one pinned core

    s17::Problem G;
    G.cam = orbfe::PoseCam{(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3], (double)(float)std::sqrt(delta2)};
    G.iterations = head[3];
    G.robust = head[4];
    for (int i = 0; i < 9; i++) {
        G.Ra[i] = (double)Rcw1[i];
        G.R0[i] = (double)Rcw2[i];
    }
    for (int i = 0; i < 3; i++) {
        G.ta[i] = (double)tcw1[i];
        G.t0[i] = (double)tcw2[i];
    }
    s17::Result host;
    std::vector<double> X;
    // (b): the point list, the loop, and the adaptor's host step on its results
    auto host_call = [&]() {
        G.O.clear();
        G.X0.clear();
        std::vector<int> first;
        for (int i = 0; i < n1; i++) {
            const int m = matches[(size_t)i];
            if (m < 0) continue;
            const KeyPoint &a = keys1[(size_t)i], &b = keys2[(size_t)m];
            G.O.push_back(orbfe::BaObs{(double)a.pt.x, (double)a.pt.y, (double)invSigma2[(size_t)a.octave], (double)b.pt.x, (double)b.pt.y,
                                       (double)invSigma2[(size_t)b.octave]});
            for (int k = 0; k < 3; k++) G.X0.push_back((double)points[3 * (size_t)i + k]);
            first.push_back(i);
        }
        s17::run(G, X, host);
        host.points = points;
        for (size_t p = 0; p < first.size(); p++)
            for (int k = 0; k < 3; k++) host.points[3 * (size_t)first[p] + k] = (float)X[3 * p + (size_t)k];
        // the median depth and the rescale: the adaptor's own host step, on the host loop's results
        host.scaled = host.points;
        for (int i = 0; i < 3; i++) host.tcw2[i] = host.Tcw[4 * i + 3];
        host.ok = InitialMapAdjuster::MedianDepthScale(matches, host.scaled, Rcw1, tcw1, host.tcw2, inertial, &host.median) ? 1 : 0;
    };
    host_call();
    std::vector<double> tHost;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        host_call();
        tHost.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    if (hostOnly) {
        write_result(argv[2], host);
        std::printf("initial_ba_latency_us host_one_thread=%.1f iterations=%d trials=%d\n", median(tHost), host.iterations, host.trials);
        return 0;
    }

    // (a) the library through the adaptor; a second, unscaled call fills the fields the adaptor does not return
    ORBextractor ex(1000, 16000, 1.2f, nLevels, 20, 7, 752, 480);
    std::array<float, 8> camA;
    for (int i = 0; i < 8; i++) camA[(size_t)i] = cam[i];
    s17::Result lib;
    orbfe_initial_ba_info info;
    std::vector<double> tLib;
    float R2[9], t2[3];
    for (int r = 0; r < std::max(reps, 1) + 1; r++) {
        lib = s17::Result();
        lib.chi2.assign((size_t)2 * host.N, 0.0);
        lib.front.assign((size_t)2 * host.N, 0);
        lib.scaled = points;
        std::memcpy(R2, Rcw2, sizeof R2);
        std::memcpy(t2, tcw2, sizeof t2);
        std::memset(&info, 0, sizeof info);
        info.struct_size = (int)sizeof info;
        info.chi2 = lib.chi2.data();
        info.depth_positive = lib.front.data();
        const auto t0 = std::chrono::steady_clock::now();
        lib.ok = InitialMapAdjuster::Adjust(ex, ORBFE_CAMERA_PINHOLE, camA, keys1, keys2, matches, lib.scaled, Rcw1, tcw1, R2, t2, inertial,
                                            &lib.median, &info)
                     ? 1
                     : 0;
        if (r > 0) tLib.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::memcpy(lib.tcw2, t2, sizeof t2);
    lib.N = info.N;
    lib.iterations = info.n_iterations;
    lib.trials = info.n_trials;
    lib.exitKind = info.exit_kind;
    std::memcpy(lib.itTrials, info.trials, sizeof lib.itTrials);
    std::memcpy(lib.cost, info.cost, sizeof lib.cost);
    std::memcpy(lib.lambda, info.lambda, sizeof lib.lambda);
    std::memcpy(lib.pose, info.pose, sizeof lib.pose);
    {   // the unscaled pose and points: the C call itself
        orbfe_initial_ba_params p = ORBFE_INITIAL_BA_PARAMS_INIT;
        for (int i = 0; i < 8; i++) p.cam[i] = cam[i];
        lib.points.assign(points.size(), 0.0f);
        const int rc = orbfe_initial_bundle_adjustment(ex.handle(), &p, n1, reinterpret_cast<const orbfe_keypoint*>(keys1.data()), n2,
                                                       reinterpret_cast<const orbfe_keypoint*>(keys2.data()), matches.data(), points.data(), Rcw1,
                                                       tcw1, Rcw2, tcw2, lib.Tcw, lib.points.data(), nullptr);
        if (rc != ORBFE_OK) { std::fprintf(stderr, "orbfe_initial_bundle_adjustment: %d\n", rc); return 3; }
    }
    write_result(argv[2], lib);
    std::printf("initial_ba_latency_us call=%.1f host_one_thread=%.1f host_same=%d iterations=%d trials=%d\n", median(tLib), median(tHost),
                same(lib, host) ? 1 : 0, host.iterations, host.trials);
    return 0;
}

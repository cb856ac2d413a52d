// Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:3447-3844) from a plain C++ program, two ways on the same inputs:
//   (a) the library through include/orbfe_adaptor.hpp's PoseOptimizer::PoseInertialOptimizationLastKeyFrame wrapper,
//   (b) SPEC DECISION S19 as a single-thread host loop (this file, -ffp-contract=off, one pinned core).
// (b) is the kernel's arithmetic for one CPU thread, so it is the latency yardstick, not an independent oracle -- that is
// tests/pose_inertial_ref.py.  Shared with the kernel, as the same text compiled for the host (-I csrc): the SO(3) functions, the
// edges, the assembly and the update (poseimu_math.h), S14's residual and kernel (poseopt_math.h), the 3 x 3 products (mat3d.h),
// sin / cos / acos (spec_math.h), the 15 x 15 solve (ldlt.h ldlt_solve_n).  Restated here: only the one-thread ordering of what the
// block does in csrc/kernels_poseimu.hip -- the tree sums, walked with a binary-counter stack over all P slots, and the loop.
//   usage: pose_inertial                                   -> library version (link test)
//          pose_inertial ldlt                              -> ldlt_solve_n<6> against ldlt_solve6, byte for byte
//          pose_inertial so3 <in.bin> <out.bin>            -> the four SO(3) functions on the file's inputs
//          pose_inertial <scene.bin> <out.bin> host [reps] -> (b) only, its results to out.bin: no GPU needed; with reps, the median
//          pose_inertial <scene.bin> <out.bin> [reps]      -> (a) and (b); results of (a) to out.bin; medians of `reps` calls
// scene.bin: int32 n, n_points, n_levels, iterations, rounds, rec_init, recover_below; float64 huber_delta2, close_factor;
//            float32 cam[8], chi2[4], close_depth, recover_chi2, gravity, inv_level_sigma2[n_levels]; the link: float32[52] (Rwb1 ..
//            tbc in the order of orbfe_imu_link), float64[99] (info9, infoG, infoA); float32 state[33] (Rcw, tcw, Rwb, twb, v, bg, ba);
//            keypoints (24 B each); int32 mp_index[n]; float32 points[n_points][3], track_depth[n_points]
// out.bin:   int32 n_inliers, N_e, rounds_run, recovered, iterations[4], ok[4], n_bad[4]; float32 state[21]; float64 H[225];
//            uint8 outlier[n]; float64 round_state[4][21]; uint8 round_outlier[4][N_e]
// so3 in:    int32 nv, nm; float64 v[nv][3], R[nm][9];  out: float64 per v: exp (9), inverse right Jacobian (9), right Jacobian (9);
//            per R: log (3)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>

#include <sched.h>

#include "orbfe_adaptor.hpp"
#include "ldlt.h"
#include "poseimu_math.h"

using namespace ORB_SLAM3;

namespace s19 {

using namespace orbfe;   // csrc/ldlt.h, mat3d.h, spec_math.h, poseopt_math.h, poseimu_math.h: the kernel's own one-thread text

constexpr int kStack = 17;

struct Problem {
    PoseCam cam;
    orbfe_pose_inertial_params prm;
    orbfe_imu_link link;
    std::vector<EdgeD> E;
    std::vector<int> kpOf;
    std::vector<uint8_t> close, bad;
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
    int nInliers = 0, Ne = 0, roundsRun = 0, recovered = 0;
    int iterations[4] = {0, 0, 0, 0}, ok[4] = {0, 0, 0, 0}, nBad[4] = {0, 0, 0, 0};
    float state[21];
    double H[225];
    std::vector<uint8_t> outlier;
    double roundState[4][21];
    std::vector<uint8_t> roundOutlier;
};

static void run(Problem& G, const float* in, int n, Result& out)
{
    const int Ne = (int)G.E.size();
    out = Result();
    std::memset(out.state, 0, sizeof out.state);
    std::memset(out.H, 0, sizeof out.H);
    std::memset(out.roundState, 0, sizeof out.roundState);
    out.Ne = Ne;
    out.outlier.assign((size_t)n, 0);
    out.roundOutlier.assign((size_t)4 * Ne, 0);
    int P = 1;
    while (P < Ne) P <<= 1;
    G.bad.assign((size_t)Ne, 0);
    const orbfe_pose_inertial_params& prm = G.prm;
    const orbfe_imu_link& K = G.link;
    const double gravity = (double)prm.gravity;
    ImuState S;
    for (int i = 0; i < 9; i++) S.Rcw[i] = (double)in[i];
    for (int i = 0; i < 3; i++) S.tcw[i] = (double)in[9 + i];
    for (int i = 0; i < 9; i++) S.Rwb[i] = (double)in[12 + i];
    for (int i = 0; i < 3; i++) {
        S.twb[i] = (double)in[21 + i];
        S.v[i] = (double)in[24 + i];
        S.bg[i] = (double)in[27 + i];
        S.ba[i] = (double)in[30 + i];
    }
    double Rcb[9], tbc[3];
    for (int i = 0; i < 9; i++) Rcb[i] = (double)K.Rcb[i];
    for (int i = 0; i < 3; i++) tbc[i] = (double)K.tbc[i];
    auto mono_sums = [&](bool huber, double (&acc)[kNV]) {
        tree<kNV>(P, acc, [&](int c, double (&v)[kNV]) {
            if (c < Ne && !G.bad[(size_t)c]) imu_edge_terms(G.cam, G.E[(size_t)c], S.Rcw, S.tcw, Rcb, tbc, huber, v);
            else
                for (int q = 0; q < kNV; q++) v[q] = 0.0;
        });
    };
    auto chi2_of = [&](int c, double& z) {
        double x, y, e0, e1, chi2;
        edge_residual(G.cam, G.E[(size_t)c], S.Rcw, S.tcw, x, y, z, e0, e1, chi2);
        return chi2;
    };
    int nBad = 0;
    for (int rnd = 0; rnd < prm.rounds; rnd++) {
        const bool huber = rnd <= 2;
        int nIt = 0;
        bool ok = true;
        for (int it = 0; it < prm.iterations; it++) {
            nIt++;
            double acc[kNV], H9[45], b[kImuN], A[kImuN][kImuN], dx[kImuN];
            mono_sums(huber, acc);
            imu_system(K, gravity, S, acc, H9, b);
            for (int i = 0; i < kImuN; i++)
                for (int j = 0; j < kImuN; j++) A[i][j] = imu_entry(K, H9, i, j);
            ldlt_solve_n<kImuN>(A, b, dx, &ok);
            if (!ok) break;
            imu_update(K, dx, S);
        }
        const float thr = prm.chi2[rnd], thrClose = (float)(prm.close_factor * (double)prm.chi2[rnd]);
        nBad = 0;
        for (int c = 0; c < Ne; c++) {
            double z;
            const double chi2 = chi2_of(c, z);
            const bool o = imu_edge_is_outlier(chi2, z, G.close[(size_t)c] != 0, thr, thrClose);
            G.bad[(size_t)c] = o ? 1 : 0;
            out.roundOutlier[(size_t)rnd * Ne + c] = o ? 1 : 0;
            nBad += o ? 1 : 0;
        }
        out.iterations[rnd] = nIt;
        out.ok[rnd] = ok ? 1 : 0;
        out.nBad[rnd] = nBad;
        for (int i = 0; i < 9; i++) out.roundState[rnd][i] = S.Rwb[i];
        for (int i = 0; i < 3; i++) {
            out.roundState[rnd][9 + i] = S.twb[i];
            out.roundState[rnd][12 + i] = S.v[i];
            out.roundState[rnd][15 + i] = S.bg[i];
            out.roundState[rnd][18 + i] = S.ba[i];
        }
        out.roundsRun = rnd + 1;
        if (Ne + 3 < 10) break;
    }
    if (Ne - nBad < prm.recover_below && !prm.rec_init) {
        out.recovered = 1;
        nBad = 0;
        for (int c = 0; c < Ne; c++) {
            double z;
            if ((float)chi2_of(c, z) < prm.recover_chi2) G.bad[(size_t)c] = 0;
            else nBad++;
        }
    }
    double acc[kNV], H9[45], b9[9], e9[9];
    mono_sums(false, acc);
    inertial_edge(K, gravity, S, H9, b9, e9);
    for (int i = 0; i < 9; i++)
        for (int j = i; j < 9; j++) {
            double h = H9[tri9(i, j)];
            if (j < 6) h = h + acc[tri6(i, j)];
            out.H[kImuN * i + j] = h;
            out.H[kImuN * j + i] = h;
        }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            out.H[kImuN * (9 + i) + (9 + j)] = K.infoG[3 * i + j];
            out.H[kImuN * (12 + i) + (12 + j)] = K.infoA[3 * i + j];
        }
    for (int i = 0; i < 9; i++) out.state[i] = (float)S.Rwb[i];
    for (int i = 0; i < 3; i++) {
        out.state[9 + i] = (float)S.twb[i];
        out.state[12 + i] = (float)S.v[i];
        out.state[15 + i] = (float)S.bg[i];
        out.state[18 + i] = (float)S.ba[i];
    }
    for (int c = 0; c < Ne; c++) out.outlier[(size_t)G.kpOf[(size_t)c]] = G.bad[(size_t)c];
    out.nInliers = Ne - nBad;
}

// ldlt_solve_n<6> against ldlt_solve6 on positive definite, indefinite and singular matrices: every byte of x and the flag
static int ldlt_check()
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(int64_t)(s >> 11) / 9007199254740992.0 - 0.5;
    };
    int cases = 0, same = 0, positives = 0;
    for (int kind = 0; kind < 3; kind++)
        for (int rep = 0; rep < 200; rep++) {
            double M[6][6], A[6][6], A6[6][6], An[6][6], b[6], x6[6], xn[6];
            for (auto& row : M)
                for (double& v : row) v = rnd();
            const int rank = kind == 2 ? 3 + rep % 3 : 6;   // singular: rank 3, 4 or 5
            for (int i = 0; i < 6; i++)
                for (int j = 0; j < 6; j++) {
                    double acc = 0.0;
                    for (int k = 0; k < rank; k++) acc += (kind == 1 && k % 2 ? -1.0 : 1.0) * M[i][k] * M[j][k];
                    A[i][j] = acc;
                }
            if (kind == 2 && rep % 2)   // exact zeros on the diagonal: the dk == 0 branch
                for (int j = 0; j < 6; j++) A[5][j] = A[j][5] = 0.0;
            for (int i = 0; i < 6; i++) {
                b[i] = rnd();
                for (int j = 0; j < 6; j++) A6[i][j] = An[i][j] = A[std::min(i, j)][std::max(i, j)];
            }
            bool p6 = false, pn = true;
            ldlt_solve6(A6, b, x6, &p6);
            ldlt_solve_n<6>(An, b, xn, &pn);
            cases++;
            positives += p6 ? 1 : 0;
            same += (!std::memcmp(x6, xn, sizeof x6) && p6 == pn) ? 1 : 0;
        }
    std::printf("ldlt_same=%d cases=%d same=%d positive=%d\n", cases == same ? 1 : 0, cases, same, positives);
    return cases == same ? 0 : 1;
}

}  // namespace s19

namespace {

struct MapPoint {
    std::array<float, 3> pos;
    float mTrackDepth;
    std::array<float, 3> GetWorldPos() const { return pos; }
};

struct Frame {
    int mNumKeypoints = 0;
    std::shared_ptr<std::vector<KeyPoint>> mvKeysUn;
    std::vector<std::shared_ptr<MapPoint>> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    std::vector<float> mvuRight;
    void* mpCamera2 = nullptr;
    float in[33], out[21];
    double H[225];
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

void write_result(const char* path, const s19::Result& r, int n)
{
    std::ofstream f(path, std::ios::binary);
    const int head[4] = {r.nInliers, r.Ne, r.roundsRun, r.recovered};
    wr(f, head, 4);
    wr(f, r.iterations, 4);
    wr(f, r.ok, 4);
    wr(f, r.nBad, 4);
    wr(f, r.state, 21);
    wr(f, r.H, 225);
    wr(f, r.outlier.data(), (size_t)n);
    wr(f, &r.roundState[0][0], 84);
    wr(f, r.roundOutlier.data(), r.roundOutlier.size());
}

bool same(const s19::Result& a, const s19::Result& b)
{
    return a.nInliers == b.nInliers && a.Ne == b.Ne && a.roundsRun == b.roundsRun && a.recovered == b.recovered &&
           !std::memcmp(a.iterations, b.iterations, 16) && !std::memcmp(a.ok, b.ok, 16) && !std::memcmp(a.nBad, b.nBad, 16) &&
           !std::memcmp(a.state, b.state, sizeof a.state) && !std::memcmp(a.H, b.H, sizeof a.H) && a.outlier == b.outlier &&
           !std::memcmp(a.roundState, b.roundState, sizeof a.roundState) && a.roundOutlier == b.roundOutlier;
}

double median(std::vector<double>& v)
{
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

int so3_mode(const char* inPath, const char* outPath)
{
    std::ifstream f(inPath, std::ios::binary);
    int head[2];
    rd(f, head, 2);
    std::vector<double> v((size_t)head[0] * 3), R((size_t)head[1] * 9);
    rd(f, v.data(), v.size());
    rd(f, R.data(), R.size());
    if (!f) { std::fprintf(stderr, "short so3 file\n"); return 2; }
    std::ofstream o(outPath, std::ios::binary);
    for (int i = 0; i < head[0]; i++) {
        const double w[3] = {v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]};
        double M[9];
        orbfe::exp_so3(w, M);
        wr(o, M, 9);
        orbfe::inverse_right_jacobian_so3(w, M);
        wr(o, M, 9);
        orbfe::right_jacobian_so3(w, M);
        wr(o, M, 9);
    }
    for (int i = 0; i < head[1]; i++) {
        double M[9], w[3];
        std::memcpy(M, &R[9 * (size_t)i], sizeof M);
        orbfe::log_so3(M, w);
        wr(o, w, 3);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "ldlt")) return s19::ldlt_check();
    if (argc == 4 && !std::strcmp(argv[1], "so3")) return so3_mode(argv[2], argv[3]);
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int head[7];
    rd(f, head, 7);
    const int n = head[0], nPoints = head[1], nLevels = head[2];
    s19::Problem G;
    orbfe_pose_inertial_params prm = ORBFE_POSE_INERTIAL_PARAMS_INIT;
    prm.iterations = head[3];
    prm.rounds = head[4];
    prm.rec_init = head[5];
    prm.recover_below = head[6];
    rd(f, &prm.huber_delta2, 1);
    rd(f, &prm.close_factor, 1);
    rd(f, prm.cam, 8);
    rd(f, prm.chi2, 4);
    rd(f, &prm.close_depth, 1);
    rd(f, &prm.recover_chi2, 1);
    rd(f, &prm.gravity, 1);
    std::vector<float> invSigma2((size_t)nLevels);
    rd(f, invSigma2.data(), (size_t)nLevels);
    orbfe_imu_link link;
    std::memset(&link, 0, sizeof link);
    link.struct_size = (int)sizeof link;
    static_assert(offsetof(orbfe_imu_link, info9) - offsetof(orbfe_imu_link, Rwb1) == 52 * sizeof(float), "the link's floats are contiguous");
    rd(f, link.Rwb1, 52);
    rd(f, link.info9, 99);
    float in[33];
    rd(f, in, 33);
    std::vector<KeyPoint> keys((size_t)n);
    static_assert(sizeof(KeyPoint) == 24, "keypoint record");
    rd(f, keys.data(), (size_t)n);
    std::vector<int> mpIndex((size_t)n);
    rd(f, mpIndex.data(), (size_t)n);
    std::vector<float> points((size_t)nPoints * 3), depth((size_t)nPoints);
    rd(f, points.data(), points.size());
    rd(f, depth.data(), depth.size());
    if (!f) { std::fprintf(stderr, "short scene file\n"); return 2; }

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = hostOnly ? (argc > 4 ? std::atoi(argv[4]) : 0) : (argc > 3 ? std::atoi(argv[3]) : 1);

    cpu_set_t set;
    CPU_ZERO(&set);
    CPU_SET(sched_getcpu(), &set);
    sched_setaffinity(0, sizeof set, &set);  // one pinned core

    G.cam = orbfe::PoseCam{(double)prm.cam[0], (double)prm.cam[1], (double)prm.cam[2], (double)prm.cam[3],
                           (double)(float)std::sqrt(prm.huber_delta2)};
    G.prm = prm;
    G.link = link;
    s19::Result host;
    auto host_call = [&]() {
        G.E.clear();
        G.kpOf.clear();
        G.close.clear();
        for (int i = 0; i < n; i++) {
            if (mpIndex[(size_t)i] < 0) continue;
            const float* p = &points[3 * (size_t)mpIndex[(size_t)i]];
            G.E.push_back(orbfe::EdgeD{(double)p[0], (double)p[1], (double)p[2], (double)keys[(size_t)i].pt.x, (double)keys[(size_t)i].pt.y,
                                     (double)invSigma2[(size_t)keys[(size_t)i].octave]});
            G.kpOf.push_back(i);
            G.close.push_back(depth[(size_t)mpIndex[(size_t)i]] < prm.close_depth ? 1 : 0);
        }
        s19::run(G, in, n, host);
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
        std::printf("pose_inertial_latency_us host_one_thread=%.1f\n", median(tHost));
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
            F.mvpMapPoints[(size_t)i] = std::make_shared<MapPoint>(MapPoint{{p[0], p[1], p[2]}, depth[(size_t)mpIndex[(size_t)i]]});
        }
    std::memcpy(F.in, in, sizeof in);
    std::array<float, 8> camA;
    for (int i = 0; i < 8; i++) camA[(size_t)i] = prm.cam[i];
    auto getState = [](Frame* fr, float* s) { std::memcpy(s, fr->in, sizeof fr->in); };
    auto setState = [](Frame* fr, const float* s, const double* H) {
        std::memcpy(fr->out, s, sizeof fr->out);
        std::memcpy(fr->H, H, sizeof fr->H);
    };
    s19::Result lib;
    orbfe_pose_inertial_info info;
    std::vector<double> tLib;
    for (int r = 0; r < std::max(reps, 1) + 1; r++) {
        lib = s19::Result();
        lib.roundOutlier.assign((size_t)4 * host.Ne, 0);
        std::memset(&info, 0, sizeof info);
        info.struct_size = (int)sizeof info;
        info.outlier = lib.roundOutlier.data();
        const auto t0 = std::chrono::steady_clock::now();
        lib.nInliers = PoseOptimizer::PoseInertialOptimizationLastKeyFrame(ex, &F, prm.rec_init != 0, ORBFE_CAMERA_PINHOLE, camA, link, getState,
                                                                           setState, &info);
        if (r > 0) tLib.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    lib.Ne = info.N_e;
    lib.roundsRun = info.rounds_run;
    lib.recovered = info.recovered;
    std::memcpy(lib.iterations, info.iterations, 16);
    std::memcpy(lib.ok, info.ok, 16);
    std::memcpy(lib.nBad, info.n_bad, 16);
    std::memcpy(lib.roundState, info.state, sizeof lib.roundState);
    std::memcpy(lib.state, F.out, sizeof lib.state);
    std::memcpy(lib.H, F.H, sizeof lib.H);
    lib.outlier.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) lib.outlier[(size_t)i] = F.mvbOutlier[(size_t)i] ? 1 : 0;
    write_result(argv[2], lib, n);
    std::printf("pose_inertial_latency_us call=%.1f host_one_thread=%.1f host_same=%d\n", median(tLib), median(tHost), same(lib, host) ? 1 : 0);
    return 0;
}

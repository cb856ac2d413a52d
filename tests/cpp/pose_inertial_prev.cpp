// Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:3846-4275) from a plain C++ program, two ways on the same inputs:
//   (a) the library through the C ABI (orbfe_pose_inertial_optimization_last_frame) and through include/orbfe_adaptor.hpp's
//       PoseOptimizer::PoseInertialOptimizationLastFrame wrapper,
//   (b) SPEC DECISION S20 as a single-thread host loop (this file, -ffp-contract=off, one pinned core).
// (b) is the kernel's own text for one CPU thread -- csrc/poseimu_prev_math.h's prev_solve and csrc/marginalize.h over an executor
// that runs every phase item by item -- so it is the latency yardstick, not an independent oracle; that is
// tests/pose_inertial_prev_ref.py.  Restated here: only what a block does differently from one thread -- the tree sums, walked with a
// binary-counter stack over all P slots, the scoring loops, and the 30 x 30 solve as ldlt.h's indexed ldlt_solve_n<30>.
//   usage: pose_inertial_prev                                   -> library version (link test)
//          pose_inertial_prev ldlt30 <in.bin> <out.bin>         -> ldlt_solve_n<30> on the file's systems
//          pose_inertial_prev marg <in.bin> <out.bin>           -> orbfe_marginalize_pose_imu on the file's 30 x 30 matrices
//          pose_inertial_prev <scene.bin> <out.bin> host [reps] -> (b) only, its results to out.bin: no GPU needed; with reps, the median
//          pose_inertial_prev <scene.bin> <out.bin> [reps]      -> (a) and (b); results of (a) to out.bin; medians of `reps` calls, and
//                                                                  of the call without the marginalisation (Hprior_out == NULL)
// scene.bin: int32 n, n_points, n_levels, iterations, rounds, rec_init, recover_below, inlier_threshold; float64 huber_delta2,
//            close_factor, prior_huber_delta; float32 cam[8], chi2[4], close_depth, recover_chi2, gravity, inv_level_sigma2[n_levels];
//            the link: float32[104] (Rwb1 .. reserved2 in the order of orbfe_imu_link_free), float64[99] (info9, infoG, infoA); the
//            prior: float64[246] (Rwb, twb, vwb, bg, ba, H); float32 state[33] (Rcw, tcw, Rwb, twb, v, bg, ba); keypoints (24 B each);
//            int32 mp_index[n]; float32 points[n_points][3], track_depth[n_points]
// out.bin:   int32 n_inliers, accepted, N_e, rounds_run, recovered, iterations[4], ok[4], n_bad[4]; float32 state[21]; float64
//            H30[900], Hprior[225]; uint8 outlier[n]; float64 round_state[4][42], prior_chi2[4], prior_weight[4]; uint8
//            round_outlier[4][N_e]
// ldlt30 in: int32 count; per system float64 A[900], b[30];  out: per system float64 x[30], int32 positive
// marg in:   int32 count; float64 H[count][900];  out: float64 Hp[count][225]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include <sched.h>

#include "orbfe_adaptor.hpp"
#include "ldlt.h"
#include "poseimu_prev_math.h"

namespace s20 {

using namespace orbfe;

constexpr int kStack = 17;

struct Problem {
    PoseCam cam;
    PrevPar par;
    float closeDepth;
    orbfe_imu_link_free link;
    orbfe_pose_imu_prior prior;
    std::vector<EdgeD> E;
    std::vector<int> kpOf;
    std::vector<uint8_t> close, bad;
};

struct Result {
    int nInliers = 0, accepted = 0;
    PrevRoundsOut rounds;
    float state[21];
    double H30[900], Hprior[225];
    std::vector<uint8_t> outlier, roundOutlier;
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

// one thread where the kernel has a block
struct HostExec : SeqExec {
    Problem& G;
    Result& R;
    int P;
    double Rcb[9], tbc[3];
    HostExec(Problem& g, Result& r) : G(g), R(r)
    {
        P = 1;
        while (P < (int)G.E.size()) P <<= 1;
        for (int i = 0; i < 9; i++) Rcb[i] = (double)G.link.Rcb[i];
        for (int i = 0; i < 3; i++) tbc[i] = (double)G.link.tbc[i];
    }
    bool leader() const { return true; }
    int Ne() const { return (int)G.E.size(); }
    void mono_sums(bool huber, const ImuState& S, PrevWork& W)
    {
        const int Ne = (int)G.E.size();
        tree<kNV>(P, W.acc, [&](int c, double (&v)[kNV]) {
            if (c < Ne && !G.bad[(size_t)c]) imu_edge_terms(G.cam, G.E[(size_t)c], S.Rcw, S.tcw, Rcb, tbc, huber, v);
            else
                for (int q = 0; q < kNV; q++) v[q] = 0.0;
        });
    }
    bool solve(PrevWork& W)
    {
        static double A[kPrevN][kPrevN];
        double b[kPrevN], x[kPrevN];
        for (int i = 0; i < kPrevN; i++) {
            b[i] = W.b[i];
            for (int j = 0; j < kPrevN; j++) A[i][j] = W.A[i][j];
        }
        bool ok = true;
        ldlt_solve_n<kPrevN>(A, b, x, &ok);
        for (int i = 0; i < kPrevN; i++) W.dx[i] = x[i];
        return ok;
    }
    double chi2_of(int c, const ImuState& S, double& z)
    {
        double x, y, e0, e1, chi2;
        edge_residual(G.cam, G.E[(size_t)c], S.Rcw, S.tcw, x, y, z, e0, e1, chi2);
        return chi2;
    }
    int score(int rnd, float thr, float thrClose, const ImuState& S)
    {
        const int Ne = (int)G.E.size();
        int nBad = 0;
        for (int c = 0; c < Ne; c++) {
            double z;
            const double chi2 = chi2_of(c, S, z);
            const bool o = imu_edge_is_outlier(chi2, z, G.close[(size_t)c] != 0, thr, thrClose);
            G.bad[(size_t)c] = o ? 1 : 0;
            R.roundOutlier[(size_t)rnd * Ne + c] = o ? 1 : 0;
            nBad += o ? 1 : 0;
        }
        return nBad;
    }
    int recover(float thr, const ImuState& S)
    {
        const int Ne = (int)G.E.size();
        int nBad = 0;
        for (int c = 0; c < Ne; c++) {
            double z;
            if ((float)chi2_of(c, S, z) < thr) G.bad[(size_t)c] = 0;
            else nBad++;
        }
        return nBad;
    }
};

static void run(Problem& G, const float* in, int n, Result& out)
{
    const int Ne = (int)G.E.size();
    out.nInliers = out.accepted = 0;
    std::memset(&out.rounds, 0, sizeof out.rounds);
    std::memset(out.state, 0, sizeof out.state);
    std::memset(out.H30, 0, sizeof out.H30);
    std::memset(out.Hprior, 0, sizeof out.Hprior);
    out.outlier.assign((size_t)n, 0);
    out.roundOutlier.assign((size_t)4 * Ne, 0);
    G.bad.assign((size_t)Ne, 0);
    const orbfe_imu_link_free& K = G.link;
    static PrevWork W;
    PrevState S;
    std::memset(&S, 0, sizeof S);
    for (int i = 0; i < 9; i++) {
        S.cur.Rcw[i] = (double)in[i];
        S.cur.Rwb[i] = (double)in[12 + i];
        S.prv.Rwb[i] = (double)K.Rwb1[i];
    }
    for (int i = 0; i < 3; i++) {
        S.cur.tcw[i] = (double)in[9 + i];
        S.cur.twb[i] = (double)in[21 + i];
        S.cur.v[i] = (double)in[24 + i];
        S.cur.bg[i] = (double)in[27 + i];
        S.cur.ba[i] = (double)in[30 + i];
        S.prv.twb[i] = (double)K.twb1[i];
        S.prv.v[i] = (double)K.v1[i];
        S.prv.bg[i] = (double)K.bg1[i];
        S.prv.ba[i] = (double)K.ba1[i];
    }
    HostExec X(G, out);
    PrevOut O;
    O.state = out.state;
    O.H30 = out.H30;
    O.Hprior = out.Hprior;
    O.nInliers = &out.nInliers;
    O.accepted = &out.accepted;
    O.rounds = &out.rounds;
    prev_solve(X, K, G.prior, G.par, S, W, O);
    for (int c = 0; c < Ne; c++) out.outlier[(size_t)G.kpOf[(size_t)c]] = G.bad[(size_t)c];
}

}  // namespace s20

namespace {

using ORB_SLAM3::KeyPoint;

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
    double Hprior[225], H30[900];
    int applied = 0;
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

void write_result(const char* path, const s20::Result& r, int n)
{
    std::ofstream f(path, std::ios::binary);
    const int head[5] = {r.nInliers, r.accepted, r.rounds.Ne, r.rounds.roundsRun, r.rounds.recovered};
    wr(f, head, 5);
    wr(f, r.rounds.iterations, 4);
    wr(f, r.rounds.ok, 4);
    wr(f, r.rounds.nBad, 4);
    wr(f, r.state, 21);
    wr(f, r.H30, 900);
    wr(f, r.Hprior, 225);
    wr(f, r.outlier.data(), (size_t)n);
    wr(f, &r.rounds.state[0][0], 4 * 42);
    wr(f, r.rounds.priorChi2, 4);
    wr(f, r.rounds.priorWeight, 4);
    wr(f, r.roundOutlier.data(), r.roundOutlier.size());
}

bool same(const s20::Result& a, const s20::Result& b)
{
    return a.nInliers == b.nInliers && a.accepted == b.accepted && !std::memcmp(&a.rounds, &b.rounds, sizeof a.rounds) &&
           !std::memcmp(a.state, b.state, sizeof a.state) && !std::memcmp(a.H30, b.H30, sizeof a.H30) &&
           !std::memcmp(a.Hprior, b.Hprior, sizeof a.Hprior) && a.outlier == b.outlier && a.roundOutlier == b.roundOutlier;
}

double median(std::vector<double>& v)
{
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

int ldlt30_mode(const char* inPath, const char* outPath)
{
    std::ifstream f(inPath, std::ios::binary);
    int count = 0;
    rd(f, &count, 1);
    std::ofstream o(outPath, std::ios::binary);
    for (int c = 0; c < count; c++) {
        double A[30][30], b[30], x[30];
        rd(f, &A[0][0], 900);
        rd(f, b, 30);
        if (!f) { std::fprintf(stderr, "short ldlt30 file\n"); return 2; }
        bool pos = false;
        orbfe::ldlt_solve_n<30>(A, b, x, &pos);
        const int p = pos ? 1 : 0;
        wr(o, x, 30);
        wr(o, &p, 1);
    }
    return 0;
}

int marg_mode(const char* inPath, const char* outPath)
{
    std::ifstream f(inPath, std::ios::binary);
    int count = 0;
    rd(f, &count, 1);
    std::ofstream o(outPath, std::ios::binary);
    std::vector<double> H(900), Hp(225);
    for (int c = 0; c < count; c++) {
        rd(f, H.data(), 900);
        if (!f) { std::fprintf(stderr, "short marg file\n"); return 2; }
        if (orbfe_marginalize_pose_imu(H.data(), Hp.data()) != ORBFE_OK) return 3;
        wr(o, Hp.data(), 225);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "ldlt30")) return ldlt30_mode(argv[2], argv[3]);
    if (argc == 4 && !std::strcmp(argv[1], "marg")) return marg_mode(argv[2], argv[3]);
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int head[8];
    rd(f, head, 8);
    const int n = head[0], nPoints = head[1], nLevels = head[2];
    orbfe_pose_inertial_prev_params prm = ORBFE_POSE_INERTIAL_PREV_PARAMS_INIT;
    prm.iterations = head[3];
    prm.rounds = head[4];
    prm.rec_init = head[5];
    prm.recover_below = head[6];
    prm.inlier_threshold = head[7];
    rd(f, &prm.huber_delta2, 1);
    rd(f, &prm.close_factor, 1);
    rd(f, &prm.prior_huber_delta, 1);
    rd(f, prm.cam, 8);
    rd(f, prm.chi2, 4);
    rd(f, &prm.close_depth, 1);
    rd(f, &prm.recover_chi2, 1);
    rd(f, &prm.gravity, 1);
    std::vector<float> invSigma2((size_t)nLevels);
    rd(f, invSigma2.data(), (size_t)nLevels);
    orbfe_imu_link_free link;
    std::memset(&link, 0, sizeof link);
    link.struct_size = (int)sizeof link;
    static_assert(offsetof(orbfe_imu_link_free, info9) - offsetof(orbfe_imu_link_free, Rwb1) == 104 * sizeof(float), "the link's floats are contiguous");
    rd(f, link.Rwb1, 104);
    rd(f, link.info9, 99);
    orbfe_pose_imu_prior prior;
    std::memset(&prior, 0, sizeof prior);
    prior.struct_size = (int)sizeof prior;
    static_assert(sizeof(orbfe_pose_imu_prior) - offsetof(orbfe_pose_imu_prior, Rwb) == 246 * sizeof(double), "the prior's doubles are contiguous");
    rd(f, prior.Rwb, 246);
    float in[33];
    rd(f, in, 33);
    std::vector<orbfe_keypoint> keys((size_t)n);
    static_assert(sizeof(orbfe_keypoint) == 24, "keypoint record");
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

    s20::Problem G;
    G.cam = orbfe::PoseCam{(double)prm.cam[0], (double)prm.cam[1], (double)prm.cam[2], (double)prm.cam[3],
                           (double)(float)std::sqrt(prm.huber_delta2)};
    G.par.gravity = (double)prm.gravity;
    G.par.priorDelta = prm.prior_huber_delta;
    for (int i = 0; i < 4; i++) {
        G.par.chi2[i] = prm.chi2[i];
        G.par.chi2Close[i] = (float)(prm.close_factor * (double)prm.chi2[i]);
    }
    G.par.recoverChi2 = prm.recover_chi2;
    G.par.recoverBelow = prm.recover_below;
    G.par.recInit = prm.rec_init != 0;
    G.par.iterations = prm.iterations;
    G.par.nRounds = prm.rounds;
    G.par.inlierThreshold = prm.inlier_threshold;
    G.closeDepth = prm.close_depth;
    G.link = link;
    G.prior = prior;
    s20::Result host;
    auto host_call = [&]() {
        G.E.clear();
        G.kpOf.clear();
        G.close.clear();
        for (int i = 0; i < n; i++) {
            if (mpIndex[(size_t)i] < 0) continue;
            const float* p = &points[3 * (size_t)mpIndex[(size_t)i]];
            G.E.push_back(orbfe::EdgeD{(double)p[0], (double)p[1], (double)p[2], (double)keys[(size_t)i].x, (double)keys[(size_t)i].y,
                                     (double)invSigma2[(size_t)keys[(size_t)i].octave]});
            G.kpOf.push_back(i);
            G.close.push_back(depth[(size_t)mpIndex[(size_t)i]] < prm.close_depth ? 1 : 0);
        }
        s20::run(G, in, n, host);
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
        std::printf("pose_inertial_prev_latency_us host_one_thread=%.1f\n", median(tHost));
        return 0;
    }

    // (a) the library
    orbfe_params ep;
    std::memset(&ep, 0, sizeof ep);
    ep.n_features = 1000;
    ep.n_fast_features = 16000;
    ep.scale_factor = 1.2f;
    ep.n_levels = nLevels;
    ep.ini_th_fast = 20;
    ep.min_th_fast = 7;
    ep.image_width = 752;
    ep.image_height = 480;
    ep.device_id = 0;
    ep.max_batch = 1;
    orbfe_handle* h = nullptr;
    if (orbfe_create(&ep, &h) != ORBFE_OK) { std::fprintf(stderr, "orbfe_create failed\n"); return 3; }
    s20::Result lib;
    orbfe_pose_inertial_prev_info info;
    std::vector<double> tLib, tNoMarg;
    std::vector<uint8_t> outl((size_t)std::max(n, 1));
    for (int pass = 0; pass < 2; pass++)   // pass 1: with Hprior_out; pass 0: without
        for (int r = 0; r < std::max(reps, 1) + 1; r++) {
            lib.roundOutlier.assign((size_t)4 * host.rounds.Ne, 0);
            std::memset(&info, 0, sizeof info);
            info.struct_size = (int)sizeof info;
            info.outlier = lib.roundOutlier.data();
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = orbfe_pose_inertial_optimization_last_frame(
                h, &prm, &link, &prior, n, keys.data(), mpIndex.data(), nPoints, points.data(), depth.data(), in, in + 9, in + 12, in + 21,
                in + 24, in + 27, in + 30, lib.state, lib.state + 9, lib.state + 12, lib.state + 15, lib.state + 18, lib.H30,
                pass ? lib.Hprior : nullptr, outl.data(), &lib.nInliers, &lib.accepted, &info);
            if (rc != ORBFE_OK) { std::fprintf(stderr, "call failed: %d %s\n", rc, orbfe_last_error(h)); return 3; }
            if (r > 0) (pass ? tLib : tNoMarg).push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
    std::memset(&lib.rounds, 0, sizeof lib.rounds);
    lib.rounds.Ne = info.N_e;
    lib.rounds.roundsRun = info.rounds_run;
    lib.rounds.recovered = info.recovered;
    std::memcpy(lib.rounds.iterations, info.iterations, 16);
    std::memcpy(lib.rounds.ok, info.ok, 16);
    std::memcpy(lib.rounds.nBad, info.n_bad, 16);
    std::memcpy(lib.rounds.state, info.state, sizeof lib.rounds.state);
    std::memcpy(lib.rounds.priorChi2, info.prior_chi2, 32);
    std::memcpy(lib.rounds.priorWeight, info.prior_weight, 32);
    lib.outlier.assign(outl.begin(), outl.begin() + n);
    // (c) the same call through include/orbfe_adaptor.hpp's wrapper: it applies the results only when accepted, and returns 1000 without a prior
    int adaptorSame = 0;
    {
        ORB_SLAM3::ORBextractor ex(1000, 16000, 1.2f, nLevels, 20, 7, 752, 480);
        Frame F;
        F.mNumKeypoints = n;
        static_assert(sizeof(KeyPoint) == sizeof(orbfe_keypoint), "keypoint record");
        F.mvKeysUn = std::make_shared<std::vector<KeyPoint>>((size_t)n);
        if (n > 0) std::memcpy(static_cast<void*>(F.mvKeysUn->data()), keys.data(), (size_t)n * sizeof(orbfe_keypoint));
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
        auto setState = [](Frame* fr, const float* s, const double* Hp, const double* H30) {
            std::memcpy(fr->out, s, sizeof fr->out);
            std::memcpy(fr->Hprior, Hp, sizeof fr->Hprior);
            std::memcpy(fr->H30, H30, sizeof fr->H30);
            fr->applied++;
        };
        bool acc = false;
        const int none = ORB_SLAM3::PoseOptimizer::PoseInertialOptimizationLastFrame(ex, &F, prm.inlier_threshold, prm.rec_init != 0,
                                                                                   ORBFE_CAMERA_PINHOLE, camA, link, nullptr, getState, setState);
        const int got = ORB_SLAM3::PoseOptimizer::PoseInertialOptimizationLastFrame(ex, &F, prm.inlier_threshold, prm.rec_init != 0,
                                                                                  ORBFE_CAMERA_PINHOLE, camA, link, &prior, getState, setState,
                                                                                  nullptr, &acc);
        bool ok = none == 1000 && got == lib.nInliers && (acc ? 1 : 0) == lib.accepted && F.applied == lib.accepted;
        for (int i = 0; i < n; i++) ok = ok && (F.mvbOutlier[(size_t)i] ? 1 : 0) == lib.outlier[(size_t)i];
        if (lib.accepted)
            ok = ok && !std::memcmp(F.out, lib.state, sizeof F.out) && !std::memcmp(F.Hprior, lib.Hprior, sizeof F.Hprior) &&
                 !std::memcmp(F.H30, lib.H30, sizeof F.H30);
        adaptorSame = ok ? 1 : 0;
    }
    write_result(argv[2], lib, n);
    std::printf("pose_inertial_prev_adaptor_same=%d\n", adaptorSame);
    std::printf("pose_inertial_prev_latency_us call=%.1f call_without_marginalisation=%.1f host_one_thread=%.1f host_same=%d\n", median(tLib),
                median(tNoMarg), median(tHost), same(lib, host) ? 1 : 0);
    orbfe_destroy(h);
    return 0;
}

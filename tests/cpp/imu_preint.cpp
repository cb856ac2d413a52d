// imu_preint.cpp -- IMU preintegration, state prediction and the inertial links (SPEC DECISION S22) from a plain C++ program.
// (b) the single-thread host loop: csrc/imu_preint_math.h, the kernel's own text, run item by item (SeqExec).  `host` mode runs it
//     alone, with no library call: that is the build the sanitizer test runs.
// (a) the library: orbfe_imu_preintegrate_frame, orbfe_imu_predict and orbfe_imu_reintegrate through the C ABI; (a) must equal (b)
//     byte for byte, and the program prints the latency of either.
// (c) the same through include/orbfe_adaptor.hpp's ImuPreintegrator; (c) must equal (a).
// `inv9` mode: the L D L^T inverse of 9 x 9 matrices as preint_info9 takes it.
//   imu_preint.bin                          -> the library's version string
//   imu_preint.bin scene.bin out.bin host   -> (b) only
//   imu_preint.bin scene.bin out.bin REPS   -> (a) and (b)
//   imu_preint.bin inv9 in.bin out.bin
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "imu_preint_math.h"
#include "orbfe_adaptor.hpp"

namespace {

template <class T>
void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T))); }
template <class T>
void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

double median(std::vector<double> v)
{
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

struct Scene {
    int nSamples, which, kfSteps;
    double tPrev, tCur;
    orbfe_imu_noise noise;
    float frameBias[6], state1[21];
    orbfe_imu_predict_params par;
    orbfe_imu_preint kf;
    std::vector<orbfe_imu_sample> samples;
};

struct Result {
    int nSteps = 0, infoOk = 0;
    orbfe_imu_preint kf, frame, re;
    std::vector<orbfe_imu_step> steps;
    float state[33];
    orbfe_imu_link lk;
    orbfe_imu_link_free lf;
};

static_assert(sizeof(orbfe_imu_preint) == 8 + sizeof(orbfe::PreintRec), "the record's float block");

void rec_in(const orbfe_imu_preint& r, orbfe::PreintRec& R) { std::memcpy(&R, &r.dT, sizeof R); }
void rec_out(const orbfe::PreintRec& R, int nSteps, orbfe_imu_preint& r)
{
    r.struct_size = (int)sizeof r;
    r.n_steps = nSteps;
    std::memcpy(&r.dT, &R, sizeof R);
}

// (b)
void host_run(const Scene& S, Result& o)
{
    static orbfe::PreintWork W;
    orbfe::SeqExec X;
    for (int i = 0; i < 6; i++) {
        W.cov[i] = S.noise.cov[i];
        W.walk[i] = S.noise.cov_walk[i];
    }
    const int n = S.nSamples < 2 ? 0 : S.nSamples - 1;
    rec_in(S.kf, W.rec[0]);
    orbfe::preint_initialize(X, W.rec[1], S.frameBias, S.frameBias + 3);
    o.steps.resize((size_t)n);
    for (int c0 = 0; c0 < n; c0 += orbfe::kPreintChunk) {
        const int cnt = std::min(orbfe::kPreintChunk, n - c0);
        X.each(cnt, [&](int t) {
            orbfe::preint_step_from_samples(S.samples.data(), n, c0 + t, S.tPrev, S.tCur, W.steps[t]);
            std::memcpy(&o.steps[(size_t)(c0 + t)], &W.steps[t], sizeof(orbfe_imu_step));
        });
        for (int r = 0; r < 2; r++)
            for (int t = 0; t < cnt; t++) orbfe::preint_integrate(X, W, W.rec[r], W.steps[t]);
    }
    o.nSteps = n;
    rec_out(W.rec[0], S.kfSteps + n, o.kf);
    rec_out(W.rec[1], n, o.frame);
    std::memset(&o.lk, 0, sizeof o.lk);
    std::memset(&o.lf, 0, sizeof o.lf);
    orbfe::preint_predict_link(X, W, S.which, S.state1, S.par.gravity, S.par.Rcb, S.par.tcb, S.par.tbc, o.state, &o.lk, &o.lf, &o.infoOk);
    // Reintegrate of the frame's steps at the frame's bias: the frame record again
    orbfe::preint_initialize(X, W.rec[0], S.frameBias, S.frameBias + 3);
    for (int t = 0; t < n; t++) {
        orbfe::PreintStep st;
        std::memcpy(&st, &o.steps[(size_t)t], sizeof st);
        orbfe::preint_integrate(X, W, W.rec[0], st);
    }
    rec_out(W.rec[0], n, o.re);
}

void write_result(const char* path, const Scene& S, const Result& r)
{
    std::ofstream f(path, std::ios::binary);
    const int head[4] = {r.nSteps, r.infoOk, r.kf.n_steps, r.frame.n_steps};
    wr(f, head, 4);
    wr(f, &r.kf.dT, orbfe::kPreintRecFloats);
    wr(f, &r.frame.dT, orbfe::kPreintRecFloats);
    wr(f, &r.re.dT, orbfe::kPreintRecFloats);
    wr(f, r.steps.data(), r.steps.size());
    wr(f, r.state, 33);
    if (S.which == ORBFE_IMU_FROM_FRAME) wr(f, &r.lf, 1);
    else wr(f, &r.lk, 1);
}

bool same(const Scene& S, const Result& a, const Result& b)
{
    return a.nSteps == b.nSteps && a.infoOk == b.infoOk && !std::memcmp(&a.kf, &b.kf, sizeof a.kf) && !std::memcmp(&a.frame, &b.frame, sizeof a.frame) &&
           !std::memcmp(&a.re, &b.re, sizeof a.re) && a.steps.size() == b.steps.size() &&
           (a.steps.empty() || !std::memcmp(a.steps.data(), b.steps.data(), a.steps.size() * sizeof(orbfe_imu_step))) &&
           !std::memcmp(a.state, b.state, sizeof a.state) &&
           (S.which == ORBFE_IMU_FROM_FRAME ? !std::memcmp(&a.lf, &b.lf, sizeof a.lf) : !std::memcmp(&a.lk, &b.lk, sizeof a.lk));
}

// n matrices of 81 floats (the upper triangle is read) -> per matrix 81 doubles (the inverse before its symmetrisation) and ok
int inv9_mode(const char* in, const char* out)
{
    std::ifstream f(in, std::ios::binary);
    if (!f) return 2;
    int n = 0;
    rd(f, &n, 1);
    std::ofstream o(out, std::ios::binary);
    static orbfe::PreintWork W;
    orbfe::SeqExec X;
    for (int m = 0; m < n; m++) {
        float A[81], C[225];
        double info[81];
        rd(f, A, 81);
        std::memset(C, 0, sizeof C);
        for (int i = 0; i < 9; i++)
            for (int j = 0; j < 9; j++) C[15 * i + j] = A[9 * i + j];
        const int ok = orbfe::preint_info9(X, W, C, info) ? 1 : 0;
        (void)info;
        // preint_info9 leaves the plain inverse in W.X
        wr(o, &W.X[0][0], 81);
        wr(o, &ok, 1);
    }
    return f ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "inv9")) return inv9_mode(argv[2], argv[3]);
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    Scene S;
    int head[3];
    rd(f, head, 3);
    S.nSamples = head[0];
    S.which = head[1];
    S.kfSteps = head[2];
    rd(f, &S.tPrev, 1);
    rd(f, &S.tCur, 1);
    std::memset(&S.noise, 0, sizeof S.noise);
    S.noise.struct_size = (int)sizeof S.noise;
    rd(f, S.noise.cov, 6);
    rd(f, S.noise.cov_walk, 6);
    rd(f, S.frameBias, 6);
    rd(f, S.state1, 21);
    std::memset(&S.par, 0, sizeof S.par);
    S.par.struct_size = (int)sizeof S.par;
    S.par.which = S.which;
    rd(f, &S.par.gravity, 1);
    rd(f, S.par.Rcb, 9);
    rd(f, S.par.tcb, 3);
    rd(f, S.par.tbc, 3);
    S.kf.struct_size = (int)sizeof S.kf;
    S.kf.n_steps = S.kfSteps;
    rd(f, &S.kf.dT, orbfe::kPreintRecFloats);
    static_assert(sizeof(orbfe_imu_sample) == 32, "sample record");
    S.samples.resize((size_t)std::max(S.nSamples, 0));
    rd(f, S.samples.data(), S.samples.size());
    if (!f) { std::fprintf(stderr, "short scene file\n"); return 2; }

    const bool hostOnly = argc > 3 && !std::strcmp(argv[3], "host");
    const int reps = hostOnly ? (argc > 4 ? std::atoi(argv[4]) : 0) : (argc > 3 ? std::atoi(argv[3]) : 1);

    cpu_set_t set;
    CPU_ZERO(&set);
    CPU_SET(sched_getcpu(), &set);
    sched_setaffinity(0, sizeof set, &set);  // one pinned core

    Result host;
    host_run(S, host);
    std::vector<double> tHost;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        host_run(S, host);
        tHost.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    if (hostOnly) {
        write_result(argv[2], S, host);
        std::printf("imu_preint_latency_us host_one_thread=%.1f\n", median(tHost));
        return 0;
    }

    // (a) the library
    orbfe_params ep;
    std::memset(&ep, 0, sizeof ep);
    ep.n_features = 1000;
    ep.n_fast_features = 16000;
    ep.scale_factor = 1.2f;
    ep.n_levels = 8;
    ep.ini_th_fast = 20;
    ep.min_th_fast = 7;
    ep.image_width = 752;
    ep.image_height = 480;
    ep.device_id = 0;
    ep.max_batch = 1;
    orbfe_handle* h = nullptr;
    if (orbfe_create(&ep, &h) != ORBFE_OK) { std::fprintf(stderr, "orbfe_create failed\n"); return 3; }
    Result lib;
    std::vector<double> tLib;
    for (int r = 0; r < std::max(reps, 1) + 1; r++) {
        lib.kf = S.kf;
        std::memset(&lib.frame, 0, sizeof lib.frame);
        lib.frame.struct_size = (int)sizeof lib.frame;
        lib.steps.assign((size_t)std::max(S.nSamples - 1, 0), orbfe_imu_step{});
        std::memset(&lib.lk, 0, sizeof lib.lk);
        std::memset(&lib.lf, 0, sizeof lib.lf);
        const auto t0 = std::chrono::steady_clock::now();
        int rc = orbfe_imu_preintegrate_frame(h, &S.noise, S.nSamples, S.samples.data(), S.tPrev, S.tCur, S.frameBias, &lib.kf, &lib.frame,
                                              lib.steps.data(), &lib.nSteps);
        if (rc == ORBFE_OK)
            rc = orbfe_imu_predict(h, &S.par, S.state1, &lib.kf, &lib.frame, lib.state,
                                   S.which == ORBFE_IMU_FROM_FRAME ? static_cast<void*>(&lib.lf) : static_cast<void*>(&lib.lk), &lib.infoOk);
        if (rc != ORBFE_OK) { std::fprintf(stderr, "call failed: %d %s\n", rc, orbfe_last_error(h)); return 3; }
        if (r > 0) tLib.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    if (orbfe_imu_reintegrate(h, &S.noise, S.frameBias, lib.nSteps, lib.steps.data(), &lib.re) != ORBFE_OK) {
        std::fprintf(stderr, "reintegrate failed: %s\n", orbfe_last_error(h));
        return 3;
    }
    // (c) the adaptor: its own extractor, the same blocks
    int adaptorSame = 0;
    {
        ORB_SLAM3::ORBextractor ex(1000, 16000, 1.2f, 8, 20, 7, 752, 480);
        std::array<float, 6> cov, walk;
        for (int i = 0; i < 6; i++) {
            cov[(size_t)i] = S.noise.cov[i];
            walk[(size_t)i] = S.noise.cov_walk[i];
        }
        ORB_SLAM3::ImuPreintegrator pre(ex, cov, walk, S.par.gravity, S.par.Rcb, S.par.tcb, S.par.tbc);
        Result ad;
        ad.kf = S.kf;
        std::memset(&ad.lk, 0, sizeof ad.lk);
        std::memset(&ad.lf, 0, sizeof ad.lf);
        const bool any = pre.PreintegrateIMU(S.samples, S.tPrev, S.tCur, S.frameBias, ad.kf, ad.frame, &ad.steps);
        ad.nSteps = (int)ad.steps.size();
        const bool ok = S.which == ORBFE_IMU_FROM_FRAME ? pre.PredictStateIMU(S.state1, ad.kf, ad.frame, ad.state, ad.lf)
                                                        : pre.PredictStateIMU(S.state1, ad.kf, ad.state, ad.lk);
        ad.infoOk = ok ? 1 : 0;
        ad.re = pre.Reintegrate(S.frameBias, ad.steps);
        const orbfe_imu_preint fresh = pre.Fresh(S.frameBias);
        adaptorSame = any == (lib.nSteps > 0) && same(S, ad, lib) && fresh.n_steps == 0 && fresh.dR[0] == 1.0f && fresh.bg[0] == S.frameBias[0] &&
                              fresh.C[0] == 0.0f
                          ? 1
                          : 0;
    }
    write_result(argv[2], S, lib);
    std::printf("imu_preint_adaptor_same=%d\n", adaptorSame);
    std::printf("imu_preint_latency_us call=%.1f host_one_thread=%.1f steps=%d host_same=%d\n", median(tLib), median(tHost), lib.nSteps,
                same(S, lib, host) ? 1 : 0);
    orbfe_destroy(h);
    return 0;
}

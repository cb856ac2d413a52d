// kernels_imu_preint.hip -- Tracking::PreintegrateIMU, IMU::Preintegrated::IntegrateNewMeasurement / Reintegrate / MergePrevious,
// Tracking::PredictStateIMU and the informations of the two inertial links on gfx950.
//
// SPEC DECISION S22.  tests/imu_preint_ref.py is the normative restatement; every byte this file produces is
// compared with it.  The arithmetic is imu_preint_math.h, one text for these kernels, the host yardstick (tests/cpp/imu_preint.cpp)
// and nothing else; this file holds what a wave does differently from one thread.
//
// imu_frame_kernel / imu_reintegrate_kernel: ONE wave per record chain, one wave per block.  The step loop is sequential; what is
// parallel inside a step is the 81 entries of A C and of (A C) A^T + B Nga B^T, spread over the 64 lanes with the records, A, B and
// the product in LDS (PreintWork, about 7 KB a block, so a CU's 160 KB never bounds the occupancy).  The 3 x 3 chain of a step is
// wave-uniform work and runs on lane 0.  With one wave in a block the barrier that closes a phase is this wave's own: no wave waits
// for another, which several chains in one block would have needed either wave-local fences or equal step counts for.
// Samples turn into steps a chunk of kPreintChunk at a time in LDS.  The epilogue -- L D L^T inverse, the n = 9 Jacobi rounds, the
// rebuild, the prediction and the link -- runs on the same wave through the same executor.
// Every loop has a static or argument-given trip bound; NaN follows the comparisons as written.
#include <cstddef>
#include <cstring>

#include "match_common.h"
#include "imu_preint_math.h"

#pragma clang fp contract(off)

namespace orbfe {

static_assert(sizeof(orbfe_imu_sample) == 32, "orbfe_imu_sample");
static_assert(sizeof(orbfe_imu_step) == sizeof(PreintStep), "orbfe_imu_step");
static_assert(sizeof(PreintRec) == kPreintRecFloats * sizeof(float), "PreintRec");
static_assert(offsetof(orbfe_imu_preint, dT) == 8 && sizeof(orbfe_imu_preint) == 8 + sizeof(PreintRec), "orbfe_imu_preint");
static_assert(offsetof(orbfe_imu_preint, C) - offsetof(orbfe_imu_preint, dT) == offsetof(PreintRec, C), "orbfe_imu_preint float block");

namespace {

constexpr int kImuThreads = 64;
constexpr int kImuState1 = 21;

struct ImuArgs {
    const orbfe_imu_sample* samples;
    const int* off;              // [batch + 1]
    const double* tPrev;         // [batch]
    const double* tCur;          // [batch]
    const float* frameBias;      // [batch][6]
    const float* state1;         // [batch][21]
    orbfe_imu_preint* kf;        // [batch]
    orbfe_imu_preint* frame;     // [batch], nullable when nothing reads or writes it
    orbfe_imu_step* stepsOut;    // nullable
    int* nStepsOut;              // nullable, [batch]
    float* stateIn;              // [batch][33]
    void* links;                 // [batch] orbfe_imu_link or orbfe_imu_link_free
    int* infoOk;                 // [batch]
    int doPreint, doPredict, which;
    float gravity;
    float Rcb[9], tcb[3], tbc[3];
    float cov[6], walk[6];
};

struct ReintArgs {
    const orbfe_imu_step* steps;
    const int* off;              // [batch + 1]
    const float* bias;           // [batch][6]
    orbfe_imu_preint* out;       // [batch]
    float cov[6], walk[6];
};

// what a wave does where one thread loops (imu_preint_math.h); the block is this one wave
struct WaveExec {
    template <class Fn>
    __device__ __forceinline__ void each(int n, Fn f)
    {
        for (int t = threadIdx.x; t < n; t += kImuThreads) f(t);
        __syncthreads();
    }
    __device__ __forceinline__ void sync() { __syncthreads(); }
};

__device__ __forceinline__ void load_rec(WaveExec& X, PreintRec& R, const orbfe_imu_preint* src)
{
    const float* s = &src->dT;
    float* d = &R.dT;
    X.each(kPreintRecFloats, [&](int t) { d[t] = s[t]; });
}

__device__ __forceinline__ void store_rec(WaveExec& X, const PreintRec& R, orbfe_imu_preint* dst, int nSteps)
{
    float* d = &dst->dT;
    const float* s = &R.dT;
    X.each(kPreintRecFloats, [&](int t) { d[t] = s[t]; });
    if (threadIdx.x == 0) {
        dst->struct_size = (int)sizeof(orbfe_imu_preint);
        dst->n_steps = nSteps;
    }
}

__global__ __launch_bounds__(kImuThreads) void imu_frame_kernel(ImuArgs G)
{
    __shared__ PreintWork W;
    const int b = blockIdx.x;
    WaveExec X;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            W.cov[i] = G.cov[i];
            W.walk[i] = G.walk[i];
        }
    }
    X.sync();
    int nSteps = 0, base = 0;
    if (G.doPreint) {
        base = G.off[b];
        const int n = G.off[b + 1] - base;
        nSteps = n < 2 ? 0 : n - 1;
    }
    load_rec(X, W.rec[0], G.kf + b);
    if (nSteps > 0) preint_initialize(X, W.rec[1], G.frameBias + 6 * b, G.frameBias + 6 * b + 3);
    else if (G.frame) load_rec(X, W.rec[1], G.frame + b);
    if (nSteps > 0) {
        const orbfe_imu_sample* S = G.samples + base;
        const double tPrev = G.tPrev[b], tCur = G.tCur[b];
        for (int c0 = 0; c0 < nSteps; c0 += kPreintChunk) {
            const int cnt = nSteps - c0 < kPreintChunk ? nSteps - c0 : kPreintChunk;
            X.each(cnt, [&](int t) {
                PreintStep st;
                preint_step_from_samples(S, nSteps, c0 + t, tPrev, tCur, st);
                W.steps[t] = st;
                if (G.stepsOut) {
                    orbfe_imu_step o;
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        o.a[k] = st.a[k];
                        o.w[k] = st.w[k];
                    }
                    o.dt = st.dt;
                    o.reserved = 0.0f;
                    G.stepsOut[base + c0 + t] = o;
                }
            });
            for (int r = 0; r < 2; r++)
                for (int t = 0; t < cnt; t++) preint_integrate(X, W, W.rec[r], W.steps[t]);
        }
        const int before = G.kf[b].n_steps;
        store_rec(X, W.rec[0], G.kf + b, before + nSteps);
        store_rec(X, W.rec[1], G.frame + b, nSteps);
    }
    if (G.nStepsOut && threadIdx.x == 0) G.nStepsOut[b] = nSteps;
    if (!G.doPredict) return;
    orbfe_imu_link* lk = G.which == kPreintFromFrame ? nullptr : static_cast<orbfe_imu_link*>(G.links) + b;
    orbfe_imu_link_free* lf = G.which == kPreintFromFrame ? static_cast<orbfe_imu_link_free*>(G.links) + b : nullptr;
    preint_predict_link(X, W, G.which, G.state1 + (size_t)b * kImuState1, G.gravity, G.Rcb, G.tcb, G.tbc, G.stateIn + (size_t)b * kImuStateIn,
                        lk, lf, G.infoOk + b);
}

__global__ __launch_bounds__(kImuThreads) void imu_reintegrate_kernel(ReintArgs G)
{
    __shared__ PreintWork W;
    const int b = blockIdx.x;
    WaveExec X;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            W.cov[i] = G.cov[i];
            W.walk[i] = G.walk[i];
        }
    }
    X.sync();
    const int base = G.off[b];
    int n = G.off[b + 1] - base;
    n = n < 0 ? 0 : n;
    preint_initialize(X, W.rec[0], G.bias + 6 * b, G.bias + 6 * b + 3);
    for (int c0 = 0; c0 < n; c0 += kPreintChunk) {
        const int cnt = n - c0 < kPreintChunk ? n - c0 : kPreintChunk;
        X.each(cnt, [&](int t) {
            const orbfe_imu_step s = G.steps[base + c0 + t];
            PreintStep st;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                st.a[k] = s.a[k];
                st.w[k] = s.w[k];
            }
            st.dt = s.dt;
            st.reserved = 0.0f;
            W.steps[t] = st;
        });
        for (int t = 0; t < cnt; t++) preint_integrate(X, W, W.rec[0], W.steps[t]);
    }
    store_rec(X, W.rec[0], G.out + b, n);
}

constexpr char kImuSizeErr[] =
    "orbfe_imu_noise / orbfe_imu_preint / orbfe_imu_predict_params struct_size does not match this library (rebuild the caller against "
    "include/orbfe.h)";

void fill_noise(const orbfe_imu_noise* N, float* cov, float* walk)
{
    for (int i = 0; i < 6; i++) {
        cov[i] = N->cov[i];
        walk[i] = N->cov_walk[i];
    }
}

void fill_predict(ImuArgs& G, const orbfe_imu_predict_params* P)
{
    G.doPredict = 1;
    G.which = P->which;
    G.gravity = P->gravity;
    memcpy(G.Rcb, P->Rcb, sizeof G.Rcb);
    memcpy(G.tcb, P->tcb, sizeof G.tcb);
    memcpy(G.tbc, P->tbc, sizeof G.tbc);
}

size_t link_bytes(int which) { return which == kPreintFromFrame ? sizeof(orbfe_imu_link_free) : sizeof(orbfe_imu_link); }

}  // namespace

// struct sizes and ranges: no device is touched.  Any pointer may be NULL: it is not checked then.
int imu_check(const orbfe_imu_noise* noise, const orbfe_imu_predict_params* P, const orbfe_imu_preint* a, const orbfe_imu_preint* b,
              std::string& err)
{
    if ((noise && noise->struct_size != (int)sizeof(orbfe_imu_noise)) || (P && P->struct_size != (int)sizeof(orbfe_imu_predict_params)) ||
        (a && a->struct_size != (int)sizeof(orbfe_imu_preint)) || (b && b->struct_size != (int)sizeof(orbfe_imu_preint))) {
        err = kImuSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    if (P && P->which != ORBFE_IMU_FROM_KEYFRAME && P->which != ORBFE_IMU_FROM_FRAME) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// batch + 1 ascending offsets that start at or after 0
int imu_check_offsets(int batch, const int* off)
{
    if (batch < 1 || !off || off[0] < 0) return ORBFE_ERR_INVALID_ARG;
    for (int b = 0; b < batch; b++)
        if (off[b + 1] < off[b]) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

int imu_preintegrate_run(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, int n, const orbfe_imu_sample* samples, double tPrev,
                         double tCur, const float* frameBias, orbfe_imu_preint* kf, orbfe_imu_preint* frame, orbfe_imu_step* stepsOut,
                         int* nSteps, std::string& err)
{
    // up: [samples | tPrev, tCur | bias | off | kf]; down: [kf | frame | steps | nSteps]
    Staging st;
    const auto bSamples = st.in<orbfe_imu_sample>(n);
    const auto bTimes = st.in<double>(2);
    const auto bBias = st.in<float>(6);
    const auto bOff = st.in<int>(2);
    const auto bKf = st.inout<orbfe_imu_preint>(1);
    const auto bFrame = st.out<orbfe_imu_preint>(1);
    const auto bSteps = st.out<orbfe_imu_step>((size_t)(n - 1));
    const auto bN = st.out<int>(1);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bSamples, samples);
    const double times[2] = {tPrev, tCur};
    st.put(bTimes, times);
    st.put(bBias, frameBias);
    const int off[2] = {0, n};
    st.put(bOff, off);
    st.put(bKf, kf);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    ImuArgs G;
    memset(&G, 0, sizeof G);
    fill_noise(noise, G.cov, G.walk);
    G.doPreint = 1;
    G.samples = st.dev(bSamples);
    G.off = st.dev(bOff);
    G.tPrev = st.dev(bTimes);
    G.tCur = G.tPrev + 1;
    G.frameBias = st.dev(bBias);
    G.kf = st.dev(bKf);
    G.frame = st.dev(bFrame);
    G.stepsOut = st.dev(bSteps);
    G.nStepsOut = st.dev(bN);
    hipLaunchKernelGGL(imu_frame_kernel, dim3(1), dim3(kImuThreads), 0, s, G);
    if ((rc = download(st, s, err)) != ORBFE_OK) return rc;
    st.get(bKf, kf);
    st.get(bFrame, frame);
    st.get(bSteps, stepsOut);
    *nSteps = *st.res(bN);
    return ORBFE_OK;
}

int imu_reintegrate_run(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, const float* bias, int n, const orbfe_imu_step* steps,
                        orbfe_imu_preint* out, std::string& err)
{
    Staging st;
    const auto bSteps = st.in<orbfe_imu_step>(n);
    const auto bBias = st.in<float>(6);
    const auto bOff = st.in<int>(2);
    const auto bOut = st.out<orbfe_imu_preint>(1);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    if (n > 0) st.put(bSteps, steps);
    st.put(bBias, bias);
    const int off[2] = {0, n};
    st.put(bOff, off);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    ReintArgs G;
    memset(&G, 0, sizeof G);
    fill_noise(noise, G.cov, G.walk);
    G.steps = st.dev(bSteps);
    G.off = st.dev(bOff);
    G.bias = st.dev(bBias);
    G.out = st.dev(bOut);
    hipLaunchKernelGGL(imu_reintegrate_kernel, dim3(1), dim3(kImuThreads), 0, s, G);
    if ((rc = download_span(st, s, bOut.off, bOut.end(), err)) != ORBFE_OK) return rc;
    st.get(bOut, out);
    return ORBFE_OK;
}

int imu_predict_run(MatchScratch& m, hipStream_t s, const orbfe_imu_predict_params* P, const float* state1, const orbfe_imu_preint* kf,
                    const orbfe_imu_preint* frame, float* stateOut, void* linkOut, int* infoOk, std::string& err)
{
    Staging st;
    const auto bState1 = st.in<float>(kImuState1);
    const auto bKf = st.in<orbfe_imu_preint>(1);
    const auto bFrame = st.in<orbfe_imu_preint>(1);
    const auto bState = st.out<float>(kImuStateIn);
    const auto bLink = st.out<uint8_t>(link_bytes(P->which));
    const auto bOk = st.out<int>(1);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bState1, state1);
    st.put(bKf, kf);
    if (frame) st.put(bFrame, frame);
    else memset(st.host(bFrame), 0, sizeof(orbfe_imu_preint));
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    ImuArgs G;
    memset(&G, 0, sizeof G);
    fill_predict(G, P);
    G.state1 = st.dev(bState1);
    G.kf = st.dev(bKf);
    G.frame = st.dev(bFrame);
    G.stateIn = st.dev(bState);
    G.links = st.dev(bLink);
    G.infoOk = st.dev(bOk);
    hipLaunchKernelGGL(imu_frame_kernel, dim3(1), dim3(kImuThreads), 0, s, G);
    if ((rc = download(st, s, err)) != ORBFE_OK) return rc;
    st.get(bState, stateOut);
    st.get(bLink, linkOut);
    *infoOk = *st.res(bOk);
    return ORBFE_OK;
}

int imu_frame_batch_device(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, const orbfe_imu_predict_params* P, int batch,
                           const orbfe_imu_sample* dSamples, const int* sampleOff, const double* dTPrev, const double* dTCur,
                           const float* dFrameBias, const float* dState1, orbfe_imu_preint* dKf, orbfe_imu_preint* dFrame,
                           orbfe_imu_step* dStepsOut, float* dStateIn, void* dLinks, int* dInfoOk, std::string& err)
{
    const size_t offBytes = (size_t)(batch + 1) * sizeof(int);
    int rc = ensure(m, offBytes, 0, err);
    if (rc != ORBFE_OK) return rc;
    // pageable caller memory: the runtime takes its copy before it returns, so the caller's array is free again at once
    MCHK(hipMemcpyAsync(m.d, sampleOff, offBytes, hipMemcpyHostToDevice, s));
    ImuArgs G;
    memset(&G, 0, sizeof G);
    fill_noise(noise, G.cov, G.walk);
    fill_predict(G, P);
    G.doPreint = 1;
    G.samples = dSamples;
    G.off = static_cast<const int*>(m.d);
    G.tPrev = dTPrev;
    G.tCur = dTCur;
    G.frameBias = dFrameBias;
    G.state1 = dState1;
    G.kf = dKf;
    G.frame = dFrame;
    G.stepsOut = dStepsOut;
    G.stateIn = dStateIn;
    G.links = dLinks;
    G.infoOk = dInfoOk;
    hipLaunchKernelGGL(imu_frame_kernel, dim3(batch), dim3(kImuThreads), 0, s, G);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int imu_reintegrate_batch_device(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, int batch, const orbfe_imu_step* dSteps,
                                 const int* stepOff, const float* dBias, orbfe_imu_preint* dOut, std::string& err)
{
    const size_t offBytes = (size_t)(batch + 1) * sizeof(int);
    int rc = ensure(m, offBytes, 0, err);
    if (rc != ORBFE_OK) return rc;
    MCHK(hipMemcpyAsync(m.d, stepOff, offBytes, hipMemcpyHostToDevice, s));
    ReintArgs G;
    memset(&G, 0, sizeof G);
    fill_noise(noise, G.cov, G.walk);
    G.steps = dSteps;
    G.off = static_cast<const int*>(m.d);
    G.bias = dBias;
    G.out = dOut;
    hipLaunchKernelGGL(imu_reintegrate_kernel, dim3(batch), dim3(kImuThreads), 0, s, G);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

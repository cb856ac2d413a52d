// match_common.h -- pieces shared by the matcher translation units: descriptor distance, the rotation-consistency filter,
// wave64 reductions, scratch arenas; and the host pieces the solver units share (the edge list, Tcw, the camera, the refusal ladder, the staging of a pose call).
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "match.h"
#include "poseopt_math.h"
#include "staging.h"

namespace orbfe {

constexpr unsigned long long kKeyNone = ~0ull;

// ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1375-1391) as 4 x 64-bit popcounts
__device__ __forceinline__ int hamming256(const uint2* a, const unsigned long long* b4)
{
    const unsigned long long* a4 = reinterpret_cast<const unsigned long long*>(a);
    return __popcll(a4[0] ^ b4[0]) + __popcll(a4[1] ^ b4[1]) + __popcll(a4[2] ^ b4[2]) + __popcll(a4[3] ^ b4[3]);
}

// the same with the query's four words in registers
__device__ __forceinline__ int hamming256(const unsigned long long* a4, unsigned long long b0, unsigned long long b1,
                                          unsigned long long b2, unsigned long long b3)
{
    return __popcll(a4[0] ^ b0) + __popcll(a4[1] ^ b1) + __popcll(a4[2] ^ b2) + __popcll(a4[3] ^ b3);
}

// ---- rotation consistency (checkOrientation) of every ORBmatcher search ----
// the histogram bin of a match (src/ORBmatcher.cc:248-253 and its copies in every search): with HISTO_LENGTH bins and the
// factor 1 / HISTO_LENGTH the angles reach bins 0 .. 12 only; that is the reference's behaviour
__host__ __device__ __forceinline__ int rotation_bin(float angle1, float angle2)
{
    float rot = angle1 - angle2;
    if (rot < 0.0f) rot = rot + 360.0f;
    int bin = (int)roundf(rot * (1.0f / ORBFE_HISTO_LENGTH));
    if (bin == ORBFE_HISTO_LENGTH) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1328-1370) over hist[ORBFE_HISTO_LENGTH]: strict ">" keeps the lowest
// bins among equal counts; the 10 % tests compare in binary32
__host__ __device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < ORBFE_HISTO_LENGTH; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    ind1 = i1; ind2 = i2; ind3 = i3;
}

// The filter a search ends with (SearchByBoW :304-322, SearchForTriangulation :633-661, the relocalisation
// SearchByProjection :1287-1323), run by ONE block over entries 0 .. n-1: histogram of the matches' bins, three maxima,
// every match of another bin dropped, the number of survivors published.  alive(j): entry j is a match; binOf(j): its
// bin; drop(j): remove it.  Without checkOrientation only the count is taken.
template <class Alive, class BinOf, class Drop>
__device__ __forceinline__ void rotation_filter_block(int n, int checkOrientation, Alive alive, BinOf binOf, Drop drop,
                                                      int* nMatchesOut)
{
    __shared__ int hist[ORBFE_HISTO_LENGTH];
    __shared__ int sInd[3];
    __shared__ int sCount;
    const int tid = threadIdx.x;
    if (tid < ORBFE_HISTO_LENGTH) hist[tid] = 0;
    if (tid == 0) sCount = 0;
    __syncthreads();
    int local = 0;
    for (int j = tid; j < n; j += blockDim.x)
        if (alive(j)) {
            local++;
            if (checkOrientation) atomicAdd(&hist[binOf(j)], 1);
        }
    __syncthreads();
    if (tid == 0) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        if (checkOrientation) three_maxima(hist, ind1, ind2, ind3);
        sInd[0] = ind1; sInd[1] = ind2; sInd[2] = ind3;
    }
    __syncthreads();
    if (checkOrientation) {
        for (int j = tid; j < n; j += blockDim.x)
            if (alive(j)) {
                const int b = binOf(j);
                if (b != sInd[0] && b != sInd[1] && b != sInd[2]) {
                    drop(j);
                    local--;
                }
            }
    }
    if (local) atomicAdd(&sCount, local);
    __syncthreads();
    if (tid == 0) *nMatchesOut = sCount;
}

// ---- wave64 helpers ----
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl_xor(lo, m);
    hi = __shfl_xor(hi, m);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// merge two (smallest, second smallest) pairs of distinct keys
__device__ __forceinline__ void top2_merge(unsigned long long& k1, unsigned long long& k2, unsigned long long o1,
                                           unsigned long long o2)
{
    const unsigned long long lo = k1 < o1 ? k1 : o1;
    const unsigned long long hi = k1 < o1 ? o1 : k1;
    const unsigned long long s2 = k2 < o2 ? k2 : o2;
    k1 = lo;
    k2 = hi < s2 ? hi : s2;
}

// wave-wide top-2 (all 64 lanes receive the result)
__device__ __forceinline__ void wave_top2(unsigned long long& k1, unsigned long long& k2)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o1 = shfl_xor_u64(k1, d), o2 = shfl_xor_u64(k2, d);
        top2_merge(k1, k2, o1, o2);
    }
}

// wave64 minimum with DPP row operations (one VALU instruction per step instead of an LDS permute): quad swaps, row
// half-mirror and mirror leave every lane of a 16-lane row with the row minimum; row_bcast 15 / 31 fold the rows into lane
// 63, which is read back as a scalar.  Lanes a row mask leaves out receive the identity.  All 64 lanes must be active.
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xA, 0xF, false));  // row_bcast:15 into rows 1 and 3
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xC, 0xF, false));  // row_bcast:31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// wave-wide top-2 of 32-bit keys (all 64 lanes receive the result): the minimum, then the minimum with its owner's smallest
// key replaced by that lane's second.  Precondition: every lane holds its own (smallest, second smallest) pair, and keys are
// distinct across lanes except for the "none" value 0xffffffff.
__device__ __forceinline__ void wave_top2_u32(unsigned& k1, unsigned& k2)
{
    const unsigned m1 = wave_min_u32(k1);
    const unsigned m2 = wave_min_u32(k1 == m1 ? k2 : k1);
    k1 = m1;
    k2 = m2;
}

[[maybe_unused]] static __global__ void fill_kernel(int* p, int v, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// grow-only arenas
inline int ensure(MatchScratch& m, size_t dBytes, size_t hBytes, std::string& err)
{
    // an asynchronous *_device launch on another stream may still be using the arenas: wait before replacing them
    if ((dBytes > m.dBytes || hBytes > m.hBytes) && m.busy && (m.d || m.hpin)) (void)hipEventSynchronize(m.busy);
    if (dBytes > m.dBytes) {
        if (m.d) (void)hipFree(m.d);
        m.d = nullptr;
        m.dBytes = 0;
        const size_t want = dBytes + dBytes / 2;
        if (hipMalloc(&m.d, want) != hipSuccess) { err = "hipMalloc(match scratch) failed"; return ORBFE_ERR_OUT_OF_MEMORY; }
        m.dBytes = want;
    }
    if (hBytes > m.hBytes) {
        if (m.hpin) (void)hipHostFree(m.hpin);
        m.hpin = nullptr;
        m.hBytes = 0;
        const size_t want = hBytes + hBytes / 2;
        if (hipHostMalloc(&m.hpin, want) != hipSuccess) { err = "hipHostMalloc(match scratch) failed"; return ORBFE_ERR_OUT_OF_MEMORY; }
        m.hBytes = want;
    }
    return ORBFE_OK;
}

// mvKeyPointIndices of MLPnPsolver (src/MLPnPsolver.cpp:67-94) and the edge list of PoseOptimization: the keypoints that have a map
// point, in keypoint order.  false: a map point index or an octave is out of range.
inline bool matched_keypoints(int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints, int nLevels, std::vector<int>& first)
{
    first.clear();
    for (int i = 0; i < n; i++)
        if (mpIndex[i] >= 0) {
            if (mpIndex[i] >= nPoints || kp[i].octave < 0 || kp[i].octave >= nLevels) return false;
            first.push_back(i);
        }
    return true;
}

// row-major 4 x 4 Tcw = [R t; 0 0 0 1] from a row-major 3 x 3 R and t, rounded to float
template <class T>
inline void fill_tcw(const T* R, const T* t, float* Tcw)
{
    for (int i = 0; i < 16; i++) Tcw[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Tcw[4 * i + j] = (float)R[3 * i + j];
        Tcw[4 * i + 3] = (float)t[i];
    }
}

// ---- host side of the solvers (S14, S17, S19) ----
// the reference keeps the Huber delta in a float (deltaMono, thHuberMono, thHuber2D: Optimizer.cc:805, :3498, :139), setDelta takes a double
inline void fill_pose_cam(PoseCam& C, const float* cam, double huber_delta2)
{
    C.fx = (double)cam[0];
    C.fy = (double)cam[1];
    C.cx = (double)cam[2];
    C.cy = (double)cam[3];
    C.delta = (double)(float)sqrt(huber_delta2);
}

// the upload of the edge list `first`: hMatch[n] keypoint -> edge (-1: none); hPts[N_e][3] and, with trackDepth, hDepth[N_e] in edge order
inline void stage_edge_list(int n, const std::vector<int>& first, const int* mpIndex, const float* points, int* hMatch, float* hPts,
                            const float* trackDepth = nullptr, float* hDepth = nullptr)
{
    for (int i = 0; i < n; i++) hMatch[i] = -1;
    for (size_t c = 0; c < first.size(); c++) {
        const int i = first[c];
        hMatch[i] = (int)c;
        for (int k = 0; k < 3; k++) hPts[3 * c + k] = points[3 * (size_t)mpIndex[i] + k];
        if (trackDepth) hDepth[c] = trackDepth[mpIndex[i]];
    }
}

// the rungs every solver's refusal ladder has after the struct sizes: the branches that are not built, then the common ranges
template <class Params>
inline int solver_check_common(const Params* P, const char* entry, const char* built, const char* section, std::string& err)
{
    if (P->camera_model == ORBFE_CAMERA_KANNALA_BRANDT8 || P->stereo != 0) {
        err = std::string(entry) + ": only the mono pinhole " + built + " built (DESIGN.md " + section + ")";
        return ORBFE_ERR_UNSUPPORTED;
    }
    if (P->camera_model != ORBFE_CAMERA_PINHOLE || P->iterations < 1 || P->iterations > 64 || !(P->huber_delta2 > 0.0))
        return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

#define MCHK(call)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(e_); return ORBFE_ERR_HIP; } \
    } while (0)

// ---- a Staging (staging.h) on a handle's arenas ----
// the arenas for the finished layout, exactly as large as it is
inline int reserve(MatchScratch& m, Staging& st, std::string& err)
{
    if (!st.ordered) { err = "Staging: an input block taken behind scratch or results"; return ORBFE_ERR_INVALID_ARG; }
    const int rc = ensure(m, st.device_bytes(), st.host_bytes(), err);
    if (rc != ORBFE_OK) return rc;
    st.bind(static_cast<uint8_t*>(m.hpin), static_cast<uint8_t*>(m.d));
    return ORBFE_OK;
}
// bytes [from, to) of the inputs go up
inline int upload_span(const Staging& st, hipStream_t s, size_t from, size_t to, std::string& err)
{
    MCHK(hipMemcpyAsync(st.dp + from, st.hp + from, to - from, hipMemcpyHostToDevice, s));
    return ORBFE_OK;
}
// all inputs in one copy
inline int upload(const Staging& st, hipStream_t s, std::string& err) { return upload_span(st, s, 0, st.inBytes, err); }
// device bytes [from, to) of the result span come down to their mirror: the copy alone, for a call that brings down several pieces
inline int fetch_span(const Staging& st, hipStream_t s, size_t from, size_t to, std::string& err)
{
    MCHK(hipMemcpyAsync(st.hp + st.mirror(from), st.dp + from, to - from, hipMemcpyDeviceToHost, s));
    return ORBFE_OK;
}
// behind the launches: the launch error, one piece down, synchronise
inline int download_span(const Staging& st, hipStream_t s, size_t from, size_t to, std::string& err)
{
    MCHK(hipGetLastError());
    const int rc = fetch_span(st, s, from, to, err);
    if (rc != ORBFE_OK) return rc;
    MCHK(hipStreamSynchronize(s));
    return ORBFE_OK;
}
// the whole result span
inline int download(const Staging& st, hipStream_t s, std::string& err) { return download_span(st, s, st.oRes, st.oRes + st.resBytes, err); }

// ---- what the pose solvers' host halves share (S14, S19, S20): host text only, the kernels and their Args stay per unit (r20) ----
// what a *_begin does after its unit's check: the keypoint bound and the edge list
inline int pose_edge_list(int nLevels, int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints, std::vector<int>& first)
{
    if (n > kPoseMaxKp) return ORBFE_ERR_INVALID_ARG;
    if (!matched_keypoints(n, kp, mpIndex, nPoints, nLevels, first)) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// What a host-pointer pose call adds to Staging: the edge-list blocks, the fields the three Args name alike, the rounds record.
//   up [kp | match (edge order index into pts) | pts | depth (with trackDepth) | the unit's in()]; device only [edgeIdx];
//   down [the unit's out() | outlier | roundOutlier].
// The order of a call: the constructor, the unit's in() takes, inputs_done(), the unit's out() takes, stage(), the unit's put()s,
// upload(), set_args() and the unit's own fields, the launch, download(), then res() / get().
struct EdgeStaging : Staging {
    const int n, Ne;
    Block<orbfe_keypoint> bKp;
    Block<int> bMatch, bIdx;
    Block<float> bPts, bDepth;
    Block<uint8_t> bOutlier, bRoundOut;

    EdgeStaging(int n_, const std::vector<int>& first, const float* trackDepth) : n(n_), Ne((int)first.size())
    {
        bKp = in<orbfe_keypoint>(n);
        bMatch = in<int>(n);
        bPts = in<float>((size_t)Ne * 3);
        bDepth = in<float>(trackDepth ? Ne : 0);
    }
    void inputs_done() { bIdx = scratch<int>(n); }
    // the arenas for the finished layout, the keypoints and the edge list `first` in the pinned one
    int stage(MatchScratch& m, const orbfe_keypoint* kp, const std::vector<int>& first, const int* mpIndex, const float* points,
              const float* trackDepth, std::string& err)
    {
        bOutlier = out<uint8_t>(n);
        bRoundOut = out<uint8_t>((size_t)4 * Ne);
        const int rc = reserve(m, *this, err);
        if (rc != ORBFE_OK) return rc;
        put(bKp, kp);
        stage_edge_list(n, first, mpIndex, points, host(bMatch), host(bPts), trackDepth, host(bDepth));
        return ORBFE_OK;
    }
    // the inputs go up and the rounds record is zeroed
    template <class R>
    int upload(hipStream_t s, Block<R> rounds, std::string& err)
    {
        const int rc = orbfe::upload(*this, s, err);
        if (rc != ORBFE_OK) return rc;
        MCHK(hipMemsetAsync(dev(rounds), 0, rounds.bytes(), s));
        return ORBFE_OK;
    }
    // the fields the three Args name alike (dN stays null: one frame of n keypoints)
    template <class Args, class R>
    void set_args(Args& G, Block<int> nInl, Block<R> rounds) const
    {
        G.nSingle = n;
        G.kpStride = n;
        G.kp = dev(bKp);
        G.match = dev(bMatch);
        G.nPoints = Ne;
        G.pts = dev(bPts);
        G.ptRec = 3;
        G.outlier = dev(bOutlier);
        G.nInliers = dev(nInl);
        G.edgeIdx = dev(bIdx);
        G.rounds = dev(rounds);
        G.roundOutlier = dev(bRoundOut);
    }
    // behind the launch: the result span comes down in one copy; the keypoints' flags are unpacked
    int download(hipStream_t s, uint8_t* outlier, std::string& err)
    {
        const int rc = orbfe::download(*this, s, err);
        if (rc != ORBFE_OK) return rc;
        get(bOutlier, outlier);
        return ORBFE_OK;
    }
    // info->outlier [4][N_e]: the rows of the rounds that ran, zeros below
    void round_rows(uint8_t* out, int roundsRun) const
    {
        if (!out || Ne <= 0) return;
        memset(out, 0, (size_t)4 * Ne);
        get(bRoundOut, out, (size_t)roundsRun * Ne);
    }
};

// what the two inertial Args hold alike; R is where the unit keeps the loop's parameters (PoseImuArgs itself, PosePrevArgs::par)
template <class Args, class Par, class Params>
inline void fill_inertial_args(Args& G, Par& R, const Params* P, const float* invLevelSigma2, int nLevels)
{
    memset(&G, 0, sizeof G);
    fill_pose_cam(G.cam, P->cam, P->huber_delta2);
    R.gravity = (double)P->gravity;
    for (int i = 0; i < 4; i++) {
        R.chi2[i] = P->chi2[i];
        R.chi2Close[i] = (float)(P->close_factor * (double)P->chi2[i]);   // float chi2close = 1.5 * chi2Mono[it] (Optimizer.cc:3686, :4100)
    }
    G.closeDepth = P->close_depth;
    R.recoverChi2 = P->recover_chi2;
    R.recoverBelow = P->recover_below;
    R.recInit = P->rec_init != 0;
    R.iterations = P->iterations;
    R.nRounds = P->rounds;
    G.nLevels = nLevels;
    for (int i = 0; i < kMaxLevels; i++) G.invSigma2[i] = i < nLevels ? invLevelSigma2[i] : 0.0f;
}

// the fields orbfe_pose_inertial_info and orbfe_pose_inertial_prev_info share, from the unit's rounds record
template <class Info, class Rounds>
inline void fill_inertial_info(Info* info, const Rounds* I, const EdgeStaging& st)
{
    uint8_t* infoOutlier = info->outlier;
    memset(info, 0, sizeof *info);
    info->struct_size = (int)sizeof(Info);
    info->outlier = infoOutlier;
    info->N_e = I->Ne;
    info->rounds_run = I->roundsRun;
    info->recovered = I->recovered;
    memcpy(info->iterations, I->iterations, sizeof I->iterations);
    memcpy(info->ok, I->ok, sizeof I->ok);
    memcpy(info->n_bad, I->nBad, sizeof I->nBad);
    memcpy(info->state, I->state, sizeof I->state);
    st.round_rows(info->outlier, I->roundsRun);
}

}  // namespace orbfe

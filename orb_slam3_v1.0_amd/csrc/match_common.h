// match_common.h -- pieces shared by the matcher translation units: descriptor distance, the rotation-consistency filter,
// wave64 reductions, scratch arenas; and the host pieces the solver units share (the edge list, Tcw, the camera, the refusal ladder, the staging of a pose call).
#pragma once
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "match.h"
#include "poseopt_math.h"

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

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; }
};

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

// ---- what the pose solvers' host halves share (S14, S19, S20): host text only, the kernels and their Args stay per unit (r20) ----
// what a *_begin does after its unit's check: the keypoint bound and the edge list
inline int pose_edge_list(int nLevels, int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints, std::vector<int>& first)
{
    if (n > kPoseMaxKp) return ORBFE_ERR_INVALID_ARG;
    if (!matched_keypoints(n, kp, mpIndex, nPoints, nLevels, first)) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// The arenas of a host-pointer pose call, one upload and one download:
//   up [kp | match (edge order index into pts) | pts | depth (with trackDepth) | the unit's input blocks]; device only [edgeIdx];
//   down [the unit's result blocks | outlier | roundOutlier].
// The unit takes its own blocks from `c`, and the order of a call is fixed: the constructor, the unit's input takes, inputs_done(),
// the unit's result takes (the first of them is where the download starts), stage() -- which appends outlier and roundOutlier --,
// the unit's copies into host(), upload(), set_args() and the unit's own fields, the launch, download(), then res().
struct EdgeStaging {
    Carver c;
    const int n, Ne;
    size_t oKp, oMatch, oPts, oDepth, inBytes = 0, oIdx = 0, oRes = 0, oOutlier = 0, oRoundOut = 0, resBytes = 0;
    uint8_t *hp = nullptr, *dp = nullptr;

    EdgeStaging(int n_, const std::vector<int>& first, const float* trackDepth) : n(n_), Ne((int)first.size())
    {
        oKp = c.take((size_t)n * sizeof(orbfe_keypoint));
        oMatch = c.take((size_t)n * sizeof(int));
        oPts = c.take((size_t)Ne * 3 * sizeof(float));
        oDepth = c.take(trackDepth ? (size_t)Ne * sizeof(float) : 0);
    }
    void inputs_done()
    {
        inBytes = c.off;
        oIdx = c.take((size_t)n * sizeof(int));
        oRes = c.off;
    }
    // the arenas for the finished layout, the keypoints and the edge list `first` in the pinned one
    int stage(MatchScratch& m, const orbfe_keypoint* kp, const std::vector<int>& first, const int* mpIndex, const float* points,
              const float* trackDepth, std::string& err)
    {
        oOutlier = c.take((size_t)n);
        oRoundOut = c.take((size_t)4 * Ne);
        resBytes = c.off - oRes;
        const int rc = ensure(m, c.off + 256, inBytes + resBytes + 256, err);
        if (rc != ORBFE_OK) return rc;
        hp = static_cast<uint8_t*>(m.hpin);
        dp = static_cast<uint8_t*>(m.d);
        if (n > 0) memcpy(hp + oKp, kp, (size_t)n * sizeof(orbfe_keypoint));
        stage_edge_list(n, first, mpIndex, points, host<int>(oMatch), host<float>(oPts), trackDepth, host<float>(oDepth));
        return ORBFE_OK;
    }
    template <class T> T* host(size_t o) const { return reinterpret_cast<T*>(hp + o); }   // an input block, before the upload
    template <class T> T* dev(size_t o) const { return reinterpret_cast<T*>(dp + o); }
    template <class T> const T* res(size_t o) const { return reinterpret_cast<const T*>(hp + inBytes + (o - oRes)); }   // after download()

    // the inputs go up and the rounds record (roundsBytes at oRounds) is zeroed
    int upload(hipStream_t s, size_t oRounds, size_t roundsBytes, std::string& err)
    {
        MCHK(hipMemcpyAsync(dp, hp, inBytes, hipMemcpyHostToDevice, s));
        MCHK(hipMemsetAsync(dp + oRounds, 0, roundsBytes, s));
        return ORBFE_OK;
    }
    // the fields the three Args name alike (dN stays null: one frame of n keypoints)
    template <class Args>
    void set_args(Args& G, size_t oNInl, size_t oRounds) const
    {
        G.nSingle = n;
        G.kpStride = n;
        G.kp = dev<const orbfe_keypoint>(oKp);
        G.match = dev<const int>(oMatch);
        G.nPoints = Ne;
        G.pts = dev<const float>(oPts);
        G.ptRec = 3;
        G.outlier = dp + oOutlier;
        G.nInliers = dev<int>(oNInl);
        G.edgeIdx = dev<int>(oIdx);
        G.rounds = dev<typename std::remove_pointer<decltype(Args::rounds)>::type>(oRounds);
        G.roundOutlier = dp + oRoundOut;
    }
    // behind the launch: the result span comes down in one copy; the keypoints' flags are unpacked
    int download(hipStream_t s, uint8_t* outlier, std::string& err)
    {
        MCHK(hipGetLastError());
        MCHK(hipMemcpyAsync(hp + inBytes, dp + oRes, resBytes, hipMemcpyDeviceToHost, s));
        MCHK(hipStreamSynchronize(s));
        if (n > 0) memcpy(outlier, res<uint8_t>(oOutlier), (size_t)n);
        return ORBFE_OK;
    }
    // info->outlier [4][N_e]: the rows of the rounds that ran, zeros below
    void round_rows(uint8_t* out, int roundsRun) const
    {
        if (!out || Ne <= 0) return;
        memset(out, 0, (size_t)4 * Ne);
        memcpy(out, res<uint8_t>(oRoundOut), (size_t)roundsRun * Ne);
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

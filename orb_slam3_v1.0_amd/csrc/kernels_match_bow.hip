// kernels_match_bow.hip -- ORBmatcher::SearchByBoW on gfx950 (src/ORBmatcher.cc:133-327).
// A frame feature belongs to exactly one vocabulary node, so the
// greedy "already matched" skips (:188) never cross nodes: one wave walks the key-frame features of
// a node sequentially and scans the node's frame features in parallel (top-2 under the total order
// (distance, position in the node's list)); a single block then applies the rotation histogram.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "keyframe.h"
#include "match_common.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

// ------------------------------------------------------------------------------------------------
// SearchByBoW
// ------------------------------------------------------------------------------------------------
struct BowArgs {
    int G;
    const int *kfOff, *kfIdx, *fOff, *fIdx;
    const uint8_t *kfDesc, *fDesc, *kfHasMP;
    const float *kfAngle, *fAngle;
    int nF;
    int nLeft;       // F->Nleft: frame features >= nLeft belong to the right camera (-1: one camera)
    float nnRatio;
    int checkOrientation;
    int* matchOut;   // [nF], -1 initialised
    int* binOf;      // [nF]
    int* nMatches;   // [1]
};

// One vocabulary node shared by key frame and frame (:166-300): the key-frame features kfIdx[k0 .. k1e) of the node in
// DBoW2 order, sequentially (later ones skip frame features matched by earlier ones, :188); the node's frame features
// fList[0 .. fCount) scanned by the wave.  IdxT: the frame-side list lives in HBM (CSR from the host) or in LDS (built by
// the wave from the per-feature node ids); AngKF / AngF: orientation of a key-frame / frame feature.  kByIndex: ties of
// the top-2 are broken by the feature index instead of the position in fList -- the same order for a list in ascending
// index, and independent of the list's order otherwise (the device-built lists of bow_track_csr_kernel).
template <bool kByIndex, typename IdxT, typename AngKF, typename AngF>
__device__ __forceinline__ void bow_walk_node(const int* __restrict__ kfIdx, int k0, int k1e, const IdxT* fList, int fCount,
                                              const uint8_t* __restrict__ kfDesc, const uint8_t* __restrict__ kfHasMP,
                                              const uint8_t* __restrict__ fDesc, int nLeftArg, float nnRatio, int checkOrientation,
                                              int* matchOut, int* binOf, AngKF kfAngle, AngF fAngle, int lane)
{
    for (int iKF = k0; iKF < k1e; iKF++) {  // sequential: later KF features skip matched frame features (:188)
        const int realIdxKF = kfIdx[iKF];
        if (!kfHasMP[realIdxKF]) continue;
        unsigned long long d4[4];
        {
            const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(kfDesc + (size_t)realIdxKF * 32);
            d4[0] = dp[0]; d4[1] = dp[1]; d4[2] = dp[2]; d4[3] = dp[3];
        }
        // two camera sides (F->Nleft != -1, :205-233): separate best / second best for the left and the right features
        const int nLeft = nLeftArg < 0 ? 0x7fffffff : nLeftArg;
        unsigned long long k1 = kKeyNone, k2 = kKeyNone, r1 = kKeyNone, r2 = kKeyNone;
        for (int iF = lane; iF < fCount; iF += 64) {
            const int realIdxF = (int)fList[iF];
            if (matchOut[realIdxF] >= 0) continue;
            const int dist = hamming256(reinterpret_cast<const uint2*>(fDesc + (size_t)realIdxF * 32), d4);
            if (dist >= 256) continue;
            const unsigned long long key = ((unsigned long long)dist << 32) | (unsigned)(kByIndex ? realIdxF : iF);
            if (realIdxF < nLeft) {
                if (key < k1) { k2 = k1; k1 = key; }
                else if (key < k2) k2 = key;
            } else {
                if (key < r1) { r2 = r1; r1 = key; }
                else if (key < r2) r2 = key;
            }
        }
        wave_top2(k1, k2);
        if (nLeftArg >= 0) wave_top2(r1, r2);  // wave-uniform
        if (k1 == kKeyNone) continue;  // bestDist1 == 256 > TH_LOW: neither side is looked at (:237)
        const int bestDist1 = (int)(k1 >> 32);
        const int bestDist2 = k2 == kKeyNone ? 256 : (int)(k2 >> 32);
        if (bestDist1 <= ORBFE_TH_LOW) {  // :237
            bool wrote = false;
            if ((float)bestDist1 < nnRatio * (float)bestDist2) {  // :239
                const int bestIdxF = kByIndex ? (int)(k1 & 0xffffffffu) : (int)fList[(int)(k1 & 0xffffffffu)];
                if (lane == 0) {
                    matchOut[bestIdxF] = realIdxKF;
                    if (checkOrientation) binOf[bestIdxF] = rotation_bin(kfAngle(realIdxKF), fAngle(bestIdxF));
                }
                wrote = true;
            }
            // right camera (:263-286): accepted whenever its best distance passes TH_LOW (the ratio test is "|| true")
            if (r1 != kKeyNone && (int)(r1 >> 32) <= ORBFE_TH_LOW) {
                const int bestIdxFR = kByIndex ? (int)(r1 & 0xffffffffu) : (int)fList[(int)(r1 & 0xffffffffu)];
                if (lane == 0) {
                    matchOut[bestIdxFR] = realIdxKF;
                    if (checkOrientation) binOf[bestIdxFR] = rotation_bin(kfAngle(realIdxKF), fAngle(bestIdxFR));
                }
                wrote = true;
            }
            if (wrote) __threadfence_block();  // later iterations of this wave read matchOut
        }
    }
}

__global__ __launch_bounds__(256) void bow_match_kernel(BowArgs A)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= A.G) return;
    const int f0 = A.fOff[g];
    bow_walk_node<false>(A.kfIdx, A.kfOff[g], A.kfOff[g + 1], A.fIdx + f0, A.fOff[g + 1] - f0, A.kfDesc, A.kfHasMP, A.fDesc, A.nLeft,
                  A.nnRatio, A.checkOrientation, A.matchOut, A.binOf, [&](int i) { return A.kfAngle[i]; },
                  [&](int i) { return A.fAngle[i]; }, lane);
}

// rotation filter (match_common.h) over the frame's features; single block
__device__ __forceinline__ void bow_finalize_block(int* matchOut, const int* binOf, int nF, int checkOrientation, int* nMatches)
{
    rotation_filter_block(
        nF, checkOrientation, [&](int j) { return matchOut[j] >= 0; }, [&](int j) { return binOf[j]; },
        [&](int j) { matchOut[j] = -1; }, nMatches);
}

__global__ __launch_bounds__(256) void bow_finalize_kernel(BowArgs A)
{
    bow_finalize_block(A.matchOut, A.binOf, A.nF, A.checkOrientation, A.nMatches);
}

// ------------------------------------------------------------------------------------------------
// SearchByBoW of the frame the extraction chain has just produced against a key frame resident in HBM
// (Tracking::TrackReferenceKeyFrame, src/Tracking.cc:825-835): the frame's FeatureVector exists only as the node id of
// every feature (the vocabulary descent ran a kernel earlier, nothing has been on the host), so the wave of a key-frame
// node collects the node's frame features itself -- ascending feature index, the order DBoW2 stores them in
// (TemplatedVocabulary.h:1157-1170) -- into its LDS list and then walks the node exactly like the CSR kernel.
// A node the frame has no feature in is left after the collection (the lockstep walk of the two FeatureVectors,
// :150-165, only stops at shared nodes).
// ------------------------------------------------------------------------------------------------
// One wave per block, one vocabulary node of the key frame at a time.  The node ids of the frame's features are staged in
// LDS once per block.  For a node the wave gathers the frame side -- descriptors and orientations: the first 64 features in
// registers, the rest in LDS (two 16-byte halves, each its own array: conflict-free b128 reads); "matched" as a bit per
// feature in its owning lane --, loads the key-frame side 64 features at a time into registers (lane l holds feature l of
// the chunk) and walks it sequentially: one descriptor broadcast per step (readlane), distances, a DPP wave top-2.  No
// step of the walk waits on HBM, and for a node of <= 64 frame features none touches LDS.  (Computing every feature's two
// best candidates up front and replaying the order with scalar steps was measured: 220 us per call against 206 -- in a
// node where most features get matched a later feature has nearly always lost one of its two.)  Nodes with more than
// kBowNodeCap frame features (degenerate vocabularies: levelsup >= L puts a whole frame into one node) take the general walk.
constexpr int kBowNodeCap = 512;

__global__ __launch_bounds__(64) void bow_track_kernel(BowTrackArgs A)
{
    extern __shared__ uint4 sMem4[];
    const int lane = threadIdx.x;
    uint4* sLo = sMem4;
    uint4* sHi = sLo + kBowNodeCap;
    float* sAng = reinterpret_cast<float*>(sHi + kBowNodeCap);
    int* sNode = reinterpret_cast<int*>(sAng + kBowNodeCap);                    // [cap] node of every frame feature
    uint16_t* list = reinterpret_cast<uint16_t*>(sNode + A.cap);                // [cap] frame features of the current node
    const BowKfRef R = *A.ref;
    if ((int)blockIdx.x >= R.G) return;
    const int nF = min(*A.nF, A.cap);
    // stopped words (weight 0) never enter the FeatureVector (TemplatedVocabulary.h:1168-1172, 1196-1200): such a feature is in
    // no node and SearchByBoW cannot match it; -1 equals no key-frame node (keyframe_create keeps node >= 0 only)
    for (int i = lane; i < nF; i += 64) sNode[i] = A.weight[A.fLeaf[i]] > 0.0 ? A.fBow[2 * i + 1] : -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    constexpr unsigned kNone = 0xffffffffu;
    for (int g = blockIdx.x; g < R.G; g += gridDim.x) {
        const int nid = R.nodeList[g];
        const int k0 = R.nodeOff[g], cntK = R.nodeOff[g + 1] - k0;
        int cnt = 0;
        for (int base = 0; base < nF; base += 64) {
            const int i = base + lane;
            const bool hit = i < nF && sNode[i] == nid;
            const unsigned long long m = __ballot(hit);
            if (hit) list[cnt + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
            cnt += __popcll(m);
        }
        if (cnt == 0) continue;  // wave-uniform
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (cnt <= kBowNodeCap) {
            // frame side: the first 64 features of the node in registers (lane l holds list position l), the rest in LDS;
            // "matched" as one bit per 64-feature chunk in the owning lane (position p belongs to lane p & 63)
            uint4 lo0 = make_uint4(0, 0, 0, 0), hi0 = lo0;
            float ang0 = 0.f;
            int idx0 = 0;
            for (int p = lane; p < cnt; p += 64) {
                const int f = (int)list[p];
                const uint4* dp = reinterpret_cast<const uint4*>(A.fDesc + (size_t)f * 32);
                const uint4 lo = dp[0], hi = dp[1];
                const float ang = A.fKp[f].angle;
                if (p < 64) { lo0 = lo; hi0 = hi; ang0 = ang; idx0 = f; }
                else { sLo[p] = lo; sHi[p] = hi; sAng[p] = ang; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            unsigned taken = 0;  // bit c: list position c * 64 + lane is matched
            for (int kc = 0; kc < cntK; kc += 64) {
                const int nk = min(64, cntK - kc);
                const bool kOn = lane < nk;
                const int myK = kOn ? R.order[k0 + kc + lane] : 0;
                unsigned long long kd[4] = {0, 0, 0, 0};
                float kAng = 0.f;
                int kHas = 0;
                if (kOn) {
                    const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(R.desc + (size_t)myK * 32);
                    kd[0] = dp[0]; kd[1] = dp[1]; kd[2] = dp[2]; kd[3] = dp[3];
                    kAng = R.kp[myK].angle;
                    kHas = A.kfHasMP[myK];
                }
                for (int j = 0; j < nk; j++) {  // sequential: later KF features skip matched frame features (:188)
                    if (!__builtin_amdgcn_readlane(kHas, j)) continue;
                    const unsigned long long d0 = readlane_u64(kd[0], j), d1 = readlane_u64(kd[1], j), d2 = readlane_u64(kd[2], j),
                                             d3 = readlane_u64(kd[3], j);
                    unsigned k1 = kNone, k2 = kNone;
                    for (int p = lane, c = 0; p < cnt; p += 64, c++) {
                        if ((taken >> c) & 1u) continue;
                        const uint4 lo = c == 0 ? lo0 : sLo[p], hi = c == 0 ? hi0 : sHi[p];
                        const int dist = __popcll((((unsigned long long)lo.y << 32) | lo.x) ^ d0) + __popcll((((unsigned long long)lo.w << 32) | lo.z) ^ d1) +
                                         __popcll((((unsigned long long)hi.y << 32) | hi.x) ^ d2) + __popcll((((unsigned long long)hi.w << 32) | hi.z) ^ d3);
                        if (dist >= 256) continue;
                        const unsigned key = ((unsigned)dist << 16) | (unsigned)p;  // (distance, position in the node's list)
                        if (key < k1) { k2 = k1; k1 = key; }
                        else if (key < k2) k2 = key;
                    }
                    wave_top2_u32(k1, k2);
                    if (k1 == kNone) continue;  // bestDist1 == 256 > TH_LOW (:237)
                    const int bestDist1 = (int)(k1 >> 16);
                    const int bestDist2 = k2 == kNone ? 256 : (int)(k2 >> 16);
                    if (bestDist1 <= ORBFE_TH_LOW && (float)bestDist1 < A.nnRatio * (float)bestDist2) {  // :237-239
                        const int realIdxKF = __builtin_amdgcn_readlane(myK, j);
                        const float angKF = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(kAng), j));
                        const int pos = (int)(k1 & 0xffffu);
                        if (lane == (pos & 63)) {  // the owner of the position
                            const int c = pos >> 6;
                            taken |= 1u << c;
                            const int bestIdxF = c == 0 ? idx0 : (int)list[pos];
                            A.matchOut[bestIdxF] = realIdxKF;
                            if (A.checkOrientation) A.binOf[bestIdxF] = rotation_bin(angKF, c == 0 ? ang0 : sAng[pos]);
                        }
                    }
                }
            }
        } else {
            bow_walk_node<false>(R.order, k0, k0 + cntK, list, cnt, R.desc, A.kfHasMP, A.fDesc, -1, A.nnRatio, A.checkOrientation,
                          A.matchOut, A.binOf, [&](int i) { return R.kp[i].angle; }, [&](int i) { return A.fKp[i].angle; }, lane);
        }
        __builtin_amdgcn_wave_barrier();  // the LDS arrays are rewritten for the block's next node
    }
}

// Frames of more than kBowLdsCap features (the node ids and a 16-bit list of the frame no longer fit in LDS): the frame side
// of every key-frame node as a CSR in HBM, built on the device -- the group of every feature (binary search of its node in
// the key frame's ascending nodeList), a count per group, an exclusive scan, a scatter -- and walked one wave per group as
// bow_match_kernel walks the host's CSR.  The scatter's atomics leave a group's list in no particular order; the walk breaks
// ties by feature index, which is what the position in DBoW2's ascending list amounts to.
constexpr int kBowLdsCap = 7168;

__global__ __launch_bounds__(256) void bow_csr_count_kernel(BowTrackArgs A)
{
    const BowKfRef R = *A.ref;
    const int nF = min(*A.nF, A.cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nF; i += gridDim.x * blockDim.x) {
        int g = -1;
        if (A.weight[A.fLeaf[i]] > 0.0) {  // stopped words are in no node (as sNode of bow_track_kernel)
            const int nid = A.fBow[2 * i + 1];
            int lo = 0, hi = R.G;  // first entry >= nid
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (R.nodeList[mid] < nid) lo = mid + 1;
                else hi = mid;
            }
            if (lo < R.G && R.nodeList[lo] == nid) g = lo;
        }
        A.fGrp[i] = g;
        if (g >= 0) atomicAdd(&A.fCnt[g], 1);
    }
}

// fOff[0 .. G] = exclusive scan of the counts; the counts become the scatter's cursors (fCnt[g] = fOff[g]).  One block,
// each thread a contiguous run of groups.
__global__ __launch_bounds__(1024) void bow_csr_scan_kernel(BowTrackArgs A)
{
    __shared__ int sSum[1024];
    const int G = A.ref->G;
    const int t = threadIdx.x, per = (G + 1023) / 1024;
    const int b = min(G, t * per), e = min(G, b + per);
    int sum = 0;
    for (int g = b; g < e; g++) sum += A.fCnt[g];
    sSum[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? sSum[t - d] : 0;
        __syncthreads();
        sSum[t] += v;
        __syncthreads();
    }
    int off = sSum[t] - sum;
    for (int g = b; g < e; g++) {
        const int c = A.fCnt[g];
        A.fOff[g] = off;
        A.fCnt[g] = off;
        off += c;
    }
    if (t == 1023) A.fOff[G] = sSum[1023];
}

__global__ __launch_bounds__(256) void bow_csr_scatter_kernel(BowTrackArgs A)
{
    const int nF = min(*A.nF, A.cap);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nF; i += gridDim.x * blockDim.x) {
        const int g = A.fGrp[i];
        if (g >= 0) A.fIdx[atomicAdd(&A.fCnt[g], 1)] = i;
    }
}

__global__ __launch_bounds__(256) void bow_track_csr_kernel(BowTrackArgs A)
{
    const BowKfRef R = *A.ref;
    const int lane = threadIdx.x & 63;
    for (int g = blockIdx.x * 4 + (threadIdx.x >> 6); g < R.G; g += gridDim.x * 4) {  // wave-uniform
        const int f0 = A.fOff[g], cnt = A.fOff[g + 1] - f0;
        if (cnt == 0) continue;
        bow_walk_node<true>(R.order, R.nodeOff[g], R.nodeOff[g + 1], A.fIdx + f0, cnt, R.desc, A.kfHasMP, A.fDesc, -1, A.nnRatio,
                            A.checkOrientation, A.matchOut, A.binOf, [&](int i) { return R.kp[i].angle; },
                            [&](int i) { return A.fKp[i].angle; }, lane);
    }
}

__global__ __launch_bounds__(256) void bow_track_finalize_kernel(BowTrackArgs A)
{
    bow_finalize_block(A.matchOut, A.binOf, min(*A.nF, A.cap), A.checkOrientation, A.nMatches);
}

}  // namespace

int match_bow_run(MatchScratch& m, hipStream_t s, int G, const int* kfOff, const int* kfIdx, const int* fOff,
                  const int* fIdx, int nKF, const uint8_t* kfDesc, const float* kfAngle, const uint8_t* kfHasMP, int nF,
                  const uint8_t* fDesc, const float* fAngle, int nLeft, float nnRatio, int checkOrientation, int* matchOut,
                  int* nMatches, std::string& err)
{
    for (int i = 0; i < nF; i++) matchOut[i] = -1;
    *nMatches = 0;
    if (G == 0 || nF == 0 || nKF == 0) return ORBFE_OK;
    const int nKfIdx = kfOff[G], nFIdx = fOff[G];
    for (int g = 0; g < G; g++)
        if (kfOff[g + 1] < kfOff[g] || fOff[g + 1] < fOff[g]) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < nKfIdx; i++)
        if (kfIdx[i] < 0 || kfIdx[i] >= nKF) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < nFIdx; i++)
        if (fIdx[i] < 0 || fIdx[i] >= nF) return ORBFE_ERR_INVALID_ARG;

    Staging st;
    const auto bKfOff = st.in<int>((size_t)G + 1);
    const auto bFOff = st.in<int>((size_t)G + 1);
    const auto bKfIdx = st.in<int>(std::max(nKfIdx, 1));
    const auto bFIdx = st.in<int>(std::max(nFIdx, 1));
    const auto bKfDesc = st.in<uint8_t>((size_t)nKF * 32);
    const auto bFDesc = st.in<uint8_t>((size_t)nF * 32);
    const auto bKfHas = st.in<uint8_t>(nKF);
    const auto bKfAng = st.in<float>(nKF);
    const auto bFAng = st.in<float>(nF);
    const auto bMatch = st.out<int>(nF);
    const auto bBin = st.scratch<int>(nF);   // between the two pieces that come down, as the layout always had it
    const auto bNM = st.out<int>(1);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bKfOff, kfOff);
    st.put(bFOff, fOff);
    st.put(bKfIdx, kfIdx, nKfIdx);
    st.put(bFIdx, fIdx, nFIdx);
    st.put(bKfDesc, kfDesc);
    st.put(bFDesc, fDesc);
    st.put(bKfHas, kfHasMP);
    st.put(bKfAng, kfAngle);
    st.put(bFAng, fAngle);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;

    BowArgs A{};
    A.G = G;
    A.kfOff = st.dev(bKfOff);
    A.fOff = st.dev(bFOff);
    A.kfIdx = st.dev(bKfIdx);
    A.fIdx = st.dev(bFIdx);
    A.kfDesc = st.dev(bKfDesc);
    A.fDesc = st.dev(bFDesc);
    A.kfHasMP = st.dev(bKfHas);
    A.kfAngle = st.dev(bKfAng);
    A.fAngle = st.dev(bFAng);
    A.nF = nF;
    A.nLeft = nLeft;
    A.nnRatio = nnRatio;
    A.checkOrientation = checkOrientation;
    A.matchOut = st.dev(bMatch);
    A.binOf = st.dev(bBin);
    A.nMatches = st.dev(bNM);
    const dim3 blk(256);
    hipLaunchKernelGGL(fill_kernel, dim3((nF + 255) / 256), blk, 0, s, A.matchOut, -1, (size_t)nF);
    hipLaunchKernelGGL(bow_match_kernel, dim3((G + 3) / 4), blk, 0, s, A);
    hipLaunchKernelGGL(bow_finalize_kernel, dim3(1), blk, 0, s, A);
    MCHK(hipGetLastError());
    if ((rc = fetch_span(st, s, bMatch.off, bMatch.end(), err)) != ORBFE_OK) return rc;
    if ((rc = fetch_span(st, s, bNM.off, bNM.end(), err)) != ORBFE_OK) return rc;
    MCHK(hipStreamSynchronize(s));
    st.get(bMatch, matchOut);
    *nMatches = *st.res(bNM);
    return ORBFE_OK;
}


int bow_track_launch(hipStream_t s, const BowTrackArgs& A, std::string& err)
{
    if (A.cap <= 0 || A.cap >= (1 << 20) || A.capGroups < 0) {
        err = "bow_track_launch: frame capacity outside (0, 2^20)";
        return ORBFE_ERR_UNSUPPORTED;
    }
    const dim3 blk(256);
    // (A.matchOut arrives filled with -1: the vocabulary descent that runs before this wrote it)
    bool csr = A.cap > kBowLdsCap;
#ifdef ORBFE_DIAG
    if (getenv("ORBFE_BOW_CSR")) csr = true;  // liborbfe_diag.so only: the HBM lists on frames that fit in LDS
    if (csr) fprintf(stderr, "orbfe diag: bow_track_launch: node lists in HBM (cap %d, key-frame node capacity %d)\n", A.cap, A.capGroups);
#endif
    if (!csr) {  // 16-bit list entries; node ids + one list of cap entries in LDS (<= 61 KB)
        const size_t lds = (size_t)kBowNodeCap * (2 * sizeof(uint4) + sizeof(float)) + (size_t)A.cap * (sizeof(int) + sizeof(uint16_t));
        hipLaunchKernelGGL(bow_track_kernel, dim3(512), dim3(64), lds, s, A);
    } else {
        const dim3 grid((A.cap + 255) / 256);
        hipLaunchKernelGGL(fill_kernel, dim3((A.capGroups + 255) / 256), blk, 0, s, A.fCnt, 0, (size_t)A.capGroups);
        hipLaunchKernelGGL(bow_csr_count_kernel, grid, blk, 0, s, A);
        hipLaunchKernelGGL(bow_csr_scan_kernel, dim3(1), dim3(1024), 0, s, A);
        hipLaunchKernelGGL(bow_csr_scatter_kernel, grid, blk, 0, s, A);
        hipLaunchKernelGGL(bow_track_csr_kernel, dim3(512), blk, 0, s, A);
    }
    hipLaunchKernelGGL(bow_track_finalize_kernel, dim3(1), blk, 0, s, A);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

// kernels_covis_refresh.hip -- MapPoint::UpdateDepth (src/MapPoint.cc:440-474) and MapPoint::ComputeDistinctiveDescriptors (:343-417)
// for a list of points of the resident covisibility graph, written into the graph's own map records.  SPEC DECISION S26 (DESIGN.md
// section 2); tests/point_refresh_ref.py is the normative restatement.
//
// One call is two launches back to back on one stream.  No block waits on another, nothing spins.
//   refresh_wave_kernel   one wave per list entry.  A point that is outside the map, not selected, bad or without observers gets its
//              outputs at rest.  A point with more than 64 observers is appended to the rest list (one atomic counter; the order of the
//              list cannot show, every entry writes only its own outputs).  Otherwise lane j owns observer j: slot, index, the key
//              frame's bad and mn_id, and the descriptor at (slot, index) as 8 dwords straight from the key frame's row.  The median
//              of lane j's row is the element at position k of the sorted row, found by the nine steps over the value of
//              distinct_select.h; each step walks the collected lanes, broadcasting descriptor c from lane c (the lane index is
//              wave-uniform) at 8 xor + 8 popcount a comparison.  Nothing is stored per pair, no private array is indexed at run
//              time, no LDS.  The winner is the wave minimum of (median, mn_id, position); its lane writes the 32 bytes of the map's
//              descriptor.  Lane 0 does UpdateDepth with the arithmetic of spec_math.h.
//   refresh_rest_kernel   returns at once when the list is empty.  A block per listed point: the observers' descriptor rows (or "not
//              collected") go to LDS as one int each, rows are strided over the threads, descriptors are read through L2 as
//              distinct_kernel reads them, the block reduces the same key.
// The setters' scatter kernels and the index kernel behind orbfe_covis_add_keyframe* are one thread per element.
// Every loop is bounded by a stride or a count clamped to it; every slot, feature index, octave and reference slot read from a table is
// range-tested or clamped before it indexes, so a corrupt graph may give a wrong answer but no access outside the tables.  None of the
// kernels uses scratch memory or spills a register, none needs more than 64 VGPRs (tests/test_point_refresh_budget.py).
#include <algorithm>
#include <cstring>

#include "covis_refresh.h"
#include "distinct_select.h"
#include "match_common.h"
#include "spec_math.h"

namespace orbfe {

namespace {

constexpr int kT = kRefreshThreads;
constexpr int kNoIndex = -2;  // the index of the reference key frame's observation is undefined

struct RefreshArgs {
    CovisTables T;
    CovisRefresh R;
    orbfe_world_point* mapPts;
    uint8_t* mapDesc;
    int n, selectValue, what;
    const int* ids;
    const int* select;  // may be null
    RefreshOut out;
    int *counter, *otherCounter, *list;
};

__device__ __forceinline__ void refresh_outputs_at_rest(const RefreshOut& o, int e)
{
    if (o.status) o.status[e] = 0;
    if (o.minDistance) o.minDistance[e] = 0.0f;
    if (o.maxDistance) o.maxDistance[e] = 0.0f;
    if (o.bestSlot) o.bestSlot[e] = -1;
    if (o.bestIndex) o.bestIndex[e] = -1;
    if (o.bestMedian) o.bestMedian[e] = -1;
}

// is observer (slot, idx) collected (:366, :370)?  Fills mn_id and the row of its descriptor in R.desc (in descriptors).
__device__ __forceinline__ bool refresh_collected(const CovisTables& T, const CovisRefresh& R, int slot, int idx, int& mnId, size_t& row)
{
    if (slot < 0 || slot >= T.kfCap) return false;
    const CovisKf k = T.kf[slot];
    const int nf = min(R.nFeat[slot], T.kfStride);
    if (k.bad != 0 || idx < 0 || idx >= nf) return false;
    mnId = k.mnId;
    row = (size_t)slot * T.kfStride + idx;
    return true;
}

// UpdateDepth for one point by one thread.  refIdx: the index of r's observation, 0 when r is not an observer (:461), kNoIndex never.
// Returns whether the distances were written.
__device__ __forceinline__ bool refresh_depth(const RefreshArgs& A, int id, const orbfe_world_point& pt, int r, int refIdx, int e)
{
    const CovisTables& T = A.T;
    const CovisRefresh& R = A.R;
    bool done = false;
    float mn = 0.0f, mx = 0.0f;
    if (r >= 0 && r < T.kfCap && refIdx >= 0 && refIdx < min(R.nFeat[r], T.kfStride)) {
        const int level = min(max((int)R.octave[(size_t)r * T.kfStride + refIdx], 0), R.nLevels - 1);
        const float* c = R.centre + (size_t)r * 3;
        const float dist = spec_point_distance(pt.x, pt.y, pt.z, c[0], c[1], c[2]);
        spec_update_depth(dist, R.sf[level], R.sf[R.nLevels - 1], mn, mx);
        A.mapPts[id].min_distance = mn;
        A.mapPts[id].max_distance = mx;
        done = true;
    }
    if (A.out.minDistance) A.out.minDistance[e] = mn;
    if (A.out.maxDistance) A.out.maxDistance[e] = mx;
    return done;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(kT) void refresh_wave_kernel(RefreshArgs A)
{
    const CovisTables& T = A.T;
    const CovisRefresh& R = A.R;
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kRefreshWaves + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.otherCounter = 0;  // the next call's counter; nobody reads it in this call
    if (e >= A.n) return;
    // all of this is wave-uniform
    const int id = A.ids[e];
    bool live = (A.select == nullptr || A.select[e] == A.selectValue) && id >= 0 && id < T.cap;
    orbfe_world_point pt{};
    int cnt = 0;
    if (live) {
        pt = A.mapPts[id];
        cnt = min(max(T.obsCount[id], 0), T.obsStride);
        live = pt.bad == 0 && cnt > 0;
    }
    if (!live) {
        if (lane == 0) refresh_outputs_at_rest(A.out, e);
        return;
    }
    if (cnt > kRefreshWaveObs) {
        if (lane == 0) {
            const int at = atomicAdd(A.counter, 1);
            if (at < R.restCap) A.list[at] = e;
        }
        return;
    }
    const int r = R.refKf[id];
    int slot = -1, idx = -1;
    if (lane < cnt) {
        slot = T.obs[(size_t)id * T.obsStride + lane];
        idx = R.obsIdx[(size_t)id * T.obsStride + lane];
    }
    int status = 0;
    if (A.what & 1) {
        // the observation of r: the first lane that holds it (there is one per key frame); none: index 0, as written
        const unsigned long long holds = __ballot(lane < cnt && slot == r);
        int refIdx = 0;
        if (holds) refIdx = __shfl(idx, __ffsll((long long)holds) - 1);
        if (refIdx == -1) refIdx = kNoIndex;
        if (lane == 0) status |= refresh_depth(A, id, pt, r, refIdx, e) ? 1 : 0;
    } else if (lane == 0) {
        if (A.out.minDistance) A.out.minDistance[e] = 0.0f;
        if (A.out.maxDistance) A.out.maxDistance[e] = 0.0f;
    }
    int bestSlot = -1, bestIndex = -1, bestMedian = -1;
    if (A.what & 2) {
        int mnId = 0;
        size_t row = 0;
        const bool mine = refresh_collected(T, R, slot, idx, mnId, row);
        unsigned int d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0, d6 = 0, d7 = 0;
        if (mine) {
            const uint4* dp = reinterpret_cast<const uint4*>(R.desc + row * 32);
            const uint4 a = dp[0], b = dp[1];
            d0 = a.x; d1 = a.y; d2 = a.z; d3 = a.w;
            d4 = b.x; d5 = b.y; d6 = b.z; d7 = b.w;
        }
        const unsigned long long mask = __ballot(mine);
        const int N = __popcll(mask);
        if (N > 0) {
            const int k = distinct_median_position(N);
            const int median = distinct_kth_distance(k, [&](int v) {
                int c = 0;
                for (unsigned long long m = mask; m; m &= m - 1) {
                    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                    const unsigned int b0 = __builtin_amdgcn_readlane(d0, src), b1 = __builtin_amdgcn_readlane(d1, src);
                    const unsigned int b2 = __builtin_amdgcn_readlane(d2, src), b3 = __builtin_amdgcn_readlane(d3, src);
                    const unsigned int b4 = __builtin_amdgcn_readlane(d4, src), b5 = __builtin_amdgcn_readlane(d5, src);
                    const unsigned int b6 = __builtin_amdgcn_readlane(d6, src), b7 = __builtin_amdgcn_readlane(d7, src);
                    const int dist = __popc(d0 ^ b0) + __popc(d1 ^ b1) + __popc(d2 ^ b2) + __popc(d3 ^ b3) + __popc(d4 ^ b4) +
                                     __popc(d5 ^ b5) + __popc(d6 ^ b6) + __popc(d7 ^ b7);
                    c += dist <= v;
                }
                return c;
            });
            const unsigned long long key = mine ? distinct_pack_observer(median, mnId, lane) : kDistinctNoObserver;
            const unsigned long long best = wave_min_u64(key);
            if (mine && key == best) {  // one lane: the position is part of the key
                uint4* o = reinterpret_cast<uint4*>(A.mapDesc + (size_t)id * 32);
                o[0] = make_uint4(d0, d1, d2, d3);
                o[1] = make_uint4(d4, d5, d6, d7);
            }
            const int win = (int)(best & 0xfffu);
            bestSlot = __shfl(slot, win);
            bestIndex = __shfl(idx, win);
            bestMedian = (int)(best >> 44);
            status |= 2;
        }
    }
    if (lane == 0) {
        if (A.out.status) A.out.status[e] = status;
        if (A.out.bestSlot) A.out.bestSlot[e] = bestSlot;
        if (A.out.bestIndex) A.out.bestIndex[e] = bestIndex;
        if (A.out.bestMedian) A.out.bestMedian[e] = bestMedian;
    }
}

__global__ __launch_bounds__(kT) void refresh_rest_kernel(RefreshArgs A)
{
    const CovisTables& T = A.T;
    const CovisRefresh& R = A.R;
    __shared__ int sRow[kCovisMaxShort];  // per observer: the row of its descriptor in R.desc, -1 = not collected
    __shared__ unsigned long long sKey[kRefreshWaves];
    __shared__ int sN, sRefPos;
    const int listed = min(*A.counter, min(R.restCap, A.n));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = blockIdx.x; q < listed; q += gridDim.x) {   // block-uniform
        const int e = A.list[q];
        if (e < 0 || e >= A.n) continue;
        const int id = A.ids[e];
        if (id < 0 || id >= T.cap) continue;
        const int cnt = min(max(T.obsCount[id], 0), T.obsStride);  // <= kCovisMaxShort (orbfe_covis_create)
        const int r = R.refKf[id];
        if (tid == 0) {
            sN = 0;
            sRefPos = cnt;
        }
        __syncthreads();
        int mineN = 0;
        for (int j = tid; j < cnt; j += kT) {
            const int slot = T.obs[(size_t)id * T.obsStride + j], idx = R.obsIdx[(size_t)id * T.obsStride + j];
            int mnId = 0;
            size_t row = 0;
            const bool c = refresh_collected(T, R, slot, idx, mnId, row);  // kfCap x kfStride < 2^31 (orbfe_covis_enable_refresh)
            sRow[j] = c ? (int)row : -1;
            mineN += c;
            if (slot == r) atomicMin(&sRefPos, j);
        }
        for (int d = 32; d >= 1; d >>= 1) mineN += __shfl_xor(mineN, d);
        if (lane == 0 && mineN) atomicAdd(&sN, mineN);
        __syncthreads();
        const int N = sN, refPos = sRefPos;
        int status = 0;
        if (tid == 0) {
            if (A.what & 1) {
                const orbfe_world_point pt = A.mapPts[id];
                int refIdx = refPos < cnt ? R.obsIdx[(size_t)id * T.obsStride + refPos] : 0;
                if (refIdx == -1) refIdx = kNoIndex;
                status |= refresh_depth(A, id, pt, r, refIdx, e) ? 1 : 0;
            } else {
                if (A.out.minDistance) A.out.minDistance[e] = 0.0f;
                if (A.out.maxDistance) A.out.maxDistance[e] = 0.0f;
            }
        }
        unsigned long long best = kDistinctNoObserver;
        if ((A.what & 2) && N > 0) {
            const int k = distinct_median_position(N);
            unsigned long long key = kDistinctNoObserver;
            for (int i = tid; i < cnt; i += kT) {
                const int rowI = sRow[i];
                if (rowI < 0) continue;
                unsigned long long d4[4];
                const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(R.desc + (size_t)rowI * 32);
                d4[0] = dp[0]; d4[1] = dp[1]; d4[2] = dp[2]; d4[3] = dp[3];
                const int median = distinct_kth_distance(k, [&](int v) {
                    int c = 0;
                    for (int j = 0; j < cnt; j++) {
                        const int rowJ = sRow[j];
                        if (rowJ < 0) continue;
                        c += hamming256(reinterpret_cast<const uint2*>(R.desc + (size_t)rowJ * 32), d4) <= v;
                    }
                    return c;
                });
                const int slotI = T.obs[(size_t)id * T.obsStride + i];  // in range: the observer is collected
                const unsigned long long mineKey = distinct_pack_observer(median, T.kf[slotI].mnId, i);
                key = mineKey < key ? mineKey : key;
            }
            key = wave_min_u64(key);
            if (lane == 0) sKey[wave] = key;
            __syncthreads();
            for (int w = 0; w < kRefreshWaves; w++) best = sKey[w] < best ? sKey[w] : best;
            const int win = (int)(best & 0xfffu);  // < cnt: the key of a collected observer
            const int rowW = sRow[win];
            if (tid < 8 && rowW >= 0)
                reinterpret_cast<unsigned int*>(A.mapDesc + (size_t)id * 32)[tid] =
                    reinterpret_cast<const unsigned int*>(R.desc + (size_t)rowW * 32)[tid];
            if (tid == 0) {
                status |= 2;
                if (A.out.bestSlot) A.out.bestSlot[e] = T.obs[(size_t)id * T.obsStride + win];
                if (A.out.bestIndex) A.out.bestIndex[e] = R.obsIdx[(size_t)id * T.obsStride + win];
                if (A.out.bestMedian) A.out.bestMedian[e] = (int)(best >> 44);
            }
        } else if (tid == 0) {
            if (A.out.bestSlot) A.out.bestSlot[e] = -1;
            if (A.out.bestIndex) A.out.bestIndex[e] = -1;
            if (A.out.bestMedian) A.out.bestMedian[e] = -1;
        }
        if (tid == 0 && A.out.status) A.out.status[e] = status;
        __syncthreads();  // sRow, sKey, sN and sRefPos are reused by the next point
    }
}

// ---- the setters ----

__global__ __launch_bounds__(256) void refresh_set_features_kernel(CovisTables T, CovisRefresh R, int slot, int n,
                                                                   const orbfe_keypoint* __restrict__ kp, const uint8_t* __restrict__ desc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) R.nFeat[slot] = n;
    if (i >= n) return;
    const size_t row = (size_t)slot * T.kfStride + i;
    R.octave[row] = (uint8_t)min(max(kp[i].octave, 0), R.nLevels - 1);
    const uint2* src = reinterpret_cast<const uint2*>(desc + (size_t)i * 32);
    uint2* dst = reinterpret_cast<uint2*>(R.desc + row * 32);
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
}

__global__ __launch_bounds__(256) void refresh_scatter_centres_kernel(CovisRefresh R, int n, const int* __restrict__ slots,
                                                                      const float* __restrict__ twc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float* c = R.centre + (size_t)slots[i] * 3;
    c[0] = twc[3 * i];
    c[1] = twc[3 * i + 1];
    c[2] = twc[3 * i + 2];
}

__global__ __launch_bounds__(256) void refresh_scatter_indices_kernel(CovisTables T, CovisRefresh R, int n, const int* __restrict__ ids,
                                                                      const int* __restrict__ off, const int* __restrict__ idx)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = ids[i], o = off[i], cnt = off[i + 1] - o;
    for (int k = 0; k < cnt; k++) R.obsIdx[(size_t)p * T.obsStride + k] = idx ? idx[o + k] : -1;
}

__global__ __launch_bounds__(256) void refresh_scatter_ref_kernel(CovisRefresh R, int n, const int* __restrict__ ids,
                                                                  const int* __restrict__ ref)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    R.refKf[ids[i]] = ref[i];
}

// behind covis_add_keyframe_kernel: feature slot i that appended the key frame to its point's list stores i as that observation's index
__global__ __launch_bounds__(256) void refresh_index_added_kernel(CovisTables T, CovisRefresh R, int slot, int nFeatures,
                                                                  const int* __restrict__ pointIds, const int* __restrict__ added)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nFeatures || added[i] != 1) return;
    const int id = pointIds[i];
    if (id < 0 || id >= T.cap) return;
    const int cnt = min(max(T.obsCount[id], 0), T.obsStride);
    for (int k = cnt - 1; k >= 0; k--)   // it was appended: found at once
        if (T.obs[(size_t)id * T.obsStride + k] == slot) {
            R.obsIdx[(size_t)id * T.obsStride + k] = i;
            return;
        }
}

}  // namespace

int covis_set_features_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int slot, int n, const orbfe_keypoint* dKp,
                              const uint8_t* dDesc, std::string& err)
{
    hipLaunchKernelGGL(refresh_set_features_kernel, dim3((std::max(n, 1) + 255) / 256), dim3(256), 0, s, T, R, slot, n, dKp, dDesc);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_scatter_centres_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int n, const int* dSlots, const float* dTwc,
                                 std::string& err)
{
    (void)T;
    hipLaunchKernelGGL(refresh_scatter_centres_kernel, dim3((n + 255) / 256), dim3(256), 0, s, R, n, dSlots, dTwc);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_scatter_indices_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int n, const int* dIds, const int* dOff,
                                 const int* dIdx, std::string& err)
{
    hipLaunchKernelGGL(refresh_scatter_indices_kernel, dim3((n + 255) / 256), dim3(256), 0, s, T, R, n, dIds, dOff, dIdx);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_scatter_ref_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int n, const int* dIds, const int* dRef,
                             std::string& err)
{
    (void)T;
    hipLaunchKernelGGL(refresh_scatter_ref_kernel, dim3((n + 255) / 256), dim3(256), 0, s, R, n, dIds, dRef);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_index_added_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int slot, int nFeatures, const int* dPointIds,
                             const int* dAdded, std::string& err)
{
    if (nFeatures < 1) return ORBFE_OK;
    hipLaunchKernelGGL(refresh_index_added_kernel, dim3((nFeatures + 255) / 256), dim3(256), 0, s, T, R, slot, nFeatures, dPointIds, dAdded);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_refresh_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, orbfe_world_point* mapPts, uint8_t* mapDesc, int n,
                         const int* dIds, const int* dSelect, int selectValue, int what, const RefreshOut& out, std::string& err)
{
    RefreshArgs A;
    memset(&A, 0, sizeof A);
    A.T = T;
    A.R = R;
    A.mapPts = mapPts;
    A.mapDesc = mapDesc;
    A.n = n;
    A.selectValue = selectValue;
    A.what = what;
    A.ids = dIds;
    A.select = dSelect;
    A.out = out;
    A.counter = R.rest + (R.parity & 1);
    A.otherCounter = R.rest + ((R.parity & 1) ^ 1);
    A.list = R.rest + 2;
    hipLaunchKernelGGL(refresh_wave_kernel, dim3((n + kRefreshWaves - 1) / kRefreshWaves), dim3(kT), 0, s, A);
    MCHK(hipGetLastError());
    hipLaunchKernelGGL(refresh_rest_kernel, dim3(std::min(n, kRefreshRestBlocks)), dim3(kT), 0, s, A);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

// kernels_local_map.hip -- Tracking::UpdateLocalMap (src/Tracking.cc:1119-1324) for a batch of independent frames against the resident
// covisibility graph (orbfe_covis).  SPEC DECISION S24; tests/local_map_ref.py is the normative restatement.
//
// Four launches back to back on one stream, each ONE block per frame; no block waits on another, nothing spins.
//   local_votes_kernel<false>  votes: a thread per keypoint over its point's observation list into an LDS table keyed by key-frame
//              slot (open addressing, 2 * ORBFE_LOCAL_MAP_VOTE_TABLE entries).  The table takes ORBFE_LOCAL_MAP_VOTE_TABLE (512)
//              distinct key frames; the 513th makes the block mark the frame's row of counters in HBM as in use and leave.  Whether
//              that happens depends on the number of distinct key frames alone.
//              selection: max_local_kf rounds of a block-wide arg-best on (count descending, mn_id ascending, slot ascending); the
//              winner's count is zeroed.  Integer sums and a total order: the arrival order of the atomics cannot show.
//   local_votes_kernel<true>   the exact fallback: its blocks return at once unless the frame's row is marked; then the same votes
//              into that row (one int per key-frame slot, all zero when the call starts) and the same rounds over it.
//   local_list_kernel          one wave: first phase, expansion, temporal key frames, the list (<= ORBFE_LOCAL_KF_MAX) in LDS with a
//              membership bit per key-frame slot; candidates are tested 16 / 64 at a time with a ballot.  Every loop is bounded by
//              a stride or a parameter; a cyclic mPrevKF chain costs n_temporal steps.
//   local_points_kernel        ORBFE_LOCAL_MAP_BLOCK threads: the local key frames' feature counts are prefixed, the walk is
//              flattened to positions q, every valid slot does an integer min of q on its point's stamp (HBM, one word per point
//              and frame), the slots that hold their stamp are compacted in order, a chunk of ORBFE_LOCAL_MAP_BLOCK slots at a time,
//              with ballots.  Every stamp and counter touched is put back, so no table is ever cleared: the work is proportional to
//              the walk.  Bit 31 of a stamp is cleared by a voter (mark_voters_seen).
// Stamps and counters are read with agent-scope atomic loads: they are written by atomics that complete in L2, and a wave waits for
// its own before the barrier behind which the block's other waves read them.
// covis_*_kernel: the scatter of orbfe_covis_set_keyframes / _set_observations.  frame_points_kernel: a thread per keypoint.
// None of them uses scratch memory or spills a register (tests/test_local_map_budget.py); the vote loops are kept from unrolling for
// that (unrolled, the table insert spilled scalar registers).
#include "local_map.h"
#include "match_common.h"

namespace orbfe {

namespace {

constexpr int kT = kVoteThreads;
constexpr int kWaves = kT / 64;
constexpr int kPT = kPointsThreads;  // the points kernel's block: one chunk of the walk
constexpr int kPointsWaves = kPT / 64;
constexpr int kH = kVoteTableSlots;

#define LM_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
// this wave's stores and atomics have reached L2: in front of the barrier behind which other waves of the block load them
#define LM_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

struct LocalMapArgs {
    CovisTables T;
    const orbfe_world_point* mapPts;
    int maxLocalKf;
    const int* voteIds;
    const int* nVotes;
    int voteStride;
    int* localKfs;
    int* nLocalKfs;
    int* voteIdsOut;
    int* counters;  // [B][kfCap + 1]
};

struct LocalListArgs {
    CovisTables T;
    int nCovisible, nTemporal, inertial;
    const int* lastKf;
    int* localKfs;
    int* nLocalKfs;
    int bitmapWords;
};

struct LocalPointsArgs {
    CovisTables T;
    const orbfe_world_point* mapPts;
    int markVoters;
    const int* voteIds;
    const int* nVotes;
    int voteStride, M;
    const int* localKfs;
    const int* nLocalKfs;
    int* idsOut;
    int* nLocalPoints;
    unsigned* stamps;
    int* counters;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned vote_hash(int slot) { return ((unsigned)slot * 2654435761u) >> 22 & (kH - 1); }

// (count desc, mn_id asc) as one word to maximise; 0 = nothing
__device__ __forceinline__ unsigned long long rank_key(int count, int mnId)
{
    return ((unsigned long long)(unsigned)count << 32) | (unsigned)(0x7fffffff - mnId);
}

__device__ __forceinline__ bool better(unsigned long long k, int s, unsigned long long bk, int bs) { return k > bk || (k == bk && s < bs); }

}  // namespace

// ---- votes (:1164-1211), ranking and the first nKFs (:1213-1226) ----
// kHbm == false: the LDS table.  Where it fills, the block marks the frame's counter row as in use and leaves the frame to the
// kHbm == true launch behind it, whose blocks return at once for every other frame.
template <bool kHbm>
__global__ __launch_bounds__(kVoteThreads) void local_votes_kernel(LocalMapArgs G)
{
    __shared__ int keys[kHbm ? 1 : kH], counts[kHbm ? 1 : kH], keyMn[kHbm ? 1 : kH];
    __shared__ int sel[64];
    __shared__ unsigned long long waveKey[kWaves];
    __shared__ int waveSlot[kWaves];
    __shared__ int nDistinct, overflow, nSel, winner;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovisTables& T = G.T;
    const int n = clampi(G.nVotes[b], 0, G.voteStride);
    const size_t voteBase = (size_t)b * G.voteStride;
    int* counter = G.counters + (size_t)b * (T.kfCap + 1);  // the row's last word: the row is in use
    if (kHbm && counter[T.kfCap] == 0) return;               // block-uniform

    if (!kHbm)
        for (int e = tid; e < kH; e += kT) {
            keys[e] = -1;
            counts[e] = 0;
        }
    if (tid == 0) nDistinct = overflow = nSel = 0;
    __syncthreads();

    if (!kHbm) {
        for (int i = tid; i < n; i += kT) {
            const int p = G.voteIds[voteBase + i];
            int out = p;
            if (p >= 0 && p < T.cap) {
                if (G.mapPts[p].bad != 0) out = -1;
                else {
                    const int cnt = clampi(T.obsCount[p], 0, T.obsStride);
                    const int* __restrict__ ob = T.obs + (size_t)p * T.obsStride;
#pragma unroll 1
                    for (int k = 0; k < cnt; k++) {
                        const int slot = ob[k];
                        if ((unsigned)slot >= (unsigned)T.kfCap) continue;
                        unsigned pos = vote_hash(slot);
                        int probe = 0;
#pragma unroll 1
                        for (; probe < kH; probe++) {
                            const int was = atomicCAS(&keys[pos], -1, slot);
                            if (was == -1 && atomicAdd(&nDistinct, 1) >= kVoteTableKeys) overflow = 1;
                            if (was == -1 || was == slot) {
                                atomicAdd(&counts[pos], 1);
                                break;
                            }
                            pos = (pos + 1) & (kH - 1);
                        }
                        if (probe == kH) overflow = 1;
                    }
                }
            }
            if (G.voteIdsOut) G.voteIdsOut[voteBase + i] = out;
        }
        __syncthreads();
        if (overflow != 0) {  // block-uniform
            if (tid == 0) counter[T.kfCap] = 1;
            return;
        }
        for (int e = tid; e < kH; e += kT)
            if (counts[e] > 0) keyMn[e] = T.kf[keys[e]].mnId;
    } else {  // the same votes into the frame's counters (all zero when the call starts): the same sums
        const int* ids = G.voteIdsOut ? G.voteIdsOut : G.voteIds;  // the same but for the bad points, which do not vote
        for (int i = tid; i < n; i += kT) {
            const int p = ids[voteBase + i];
            if (p < 0 || p >= T.cap || G.mapPts[p].bad != 0) continue;
            const int cnt = clampi(T.obsCount[p], 0, T.obsStride);
            const int* __restrict__ ob = T.obs + (size_t)p * T.obsStride;
            for (int k = 0; k < cnt; k++)
                if ((unsigned)ob[k] < (unsigned)T.kfCap) atomicAdd(&counter[ob[k]], 1);
        }
        LM_DRAIN();
    }
    __syncthreads();

    const int nEntries = kHbm ? T.kfCap : kH;
    for (int r = 0; r < G.maxLocalKf; r++) {
        unsigned long long bk = 0;
        int bs = 0x7fffffff;
#pragma unroll 1
        for (int e = tid; e < nEntries; e += kT) {
            const int c = kHbm ? __hip_atomic_load(&counter[e], LM_RLX_AGENT) : counts[e];
            if (c > 0) {
                const int s = kHbm ? e : keys[e];
                const unsigned long long k = rank_key(c, kHbm ? T.kf[e].mnId : keyMn[e]);
                if (better(k, s, bk, bs)) { bk = k; bs = s; }
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long ok = __shfl_xor(bk, d);
            const int os = __shfl_xor(bs, d);
            if (better(ok, os, bk, bs)) { bk = ok; bs = os; }
        }
        if (lane == 0) {
            waveKey[wave] = bk;
            waveSlot[wave] = bs;
        }
        __syncthreads();
        if (tid == 0) {
            bk = waveKey[0];
            bs = waveSlot[0];
#pragma unroll
            for (int w = 1; w < kWaves; w++)
                if (better(waveKey[w], waveSlot[w], bk, bs)) { bk = waveKey[w]; bs = waveSlot[w]; }
            winner = bk != 0 ? bs : -1;
            if (bk != 0) {
                sel[nSel] = bs;
                nSel = nSel + 1;
                if (kHbm) __hip_atomic_store(&counter[bs], 0, LM_RLX_AGENT);
            }
        }
        if (kHbm) LM_DRAIN();
        __syncthreads();
        const int win = winner;
        if (win < 0) break;  // block-uniform
        if (!kHbm) {
            for (int e = tid; e < kH; e += kT)
                if (keys[e] == win) counts[e] = 0;
            __syncthreads();
        }
    }
    // (HBM counters that lost stay as they are: local_points_kernel puts them back to zero, told by the row's last word)
    // the selection in rank order, for local_list_kernel
    if (tid < 64) G.localKfs[(size_t)b * kLocalKfMax + tid] = tid < nSel ? sel[tid] : -1;
    if (tid == 0) G.nLocalKfs[b] = nSel;
}

// ---- the list: first phase, expansion, temporal key frames (:1226-1314); ONE wave per frame, every lane on the same path ----
__global__ __launch_bounds__(64) void local_list_kernel(LocalListArgs G)
{
    extern __shared__ unsigned inList[];  // one bit per key-frame slot
    __shared__ int list[kLocalKfMax];
    const int b = blockIdx.x, lane = threadIdx.x;
    const CovisTables& T = G.T;
    for (int w = lane; w < G.bitmapWords; w += 64) inList[w] = 0;
    __syncthreads();
    {
        int len = 0;  // wave-uniform
        auto listed = [&](int s) { return (inList[s >> 5] >> (s & 31)) & 1u; };
        auto append = [&](int s) {
            if (len < kLocalKfMax) {
                if (lane == 0) {
                    list[len] = s;
                    inList[s >> 5] |= 1u << (s & 31);
                }
                len++;
            }
        };
        {   // a bad key frame is skipped but has used its place among the nKFs (:1235)
            const int ns = clampi(G.nLocalKfs[b], 0, 64);
            const int s = lane < ns ? G.localKfs[(size_t)b * kLocalKfMax + lane] : -1;  // written by local_votes_kernel: a slot
            const bool good = s >= 0 && T.kf[s].bad == 0;
            const unsigned long long m = __ballot(good);
            if (good) {
                list[__popcll(m & ((1ull << lane) - 1))] = s;
                atomicOr(&inList[s >> 5], 1u << (s & 31));
            }
            len = __popcll(m);
        }
        const int nFirst = len;
        for (int i = 0; i < nFirst; i++) {
            const int s = list[i];
            const CovisKf rec = T.kf[s];
            // (a) GetBestCovisibilityKeyFrames(N): the first min(size, N) of the ordered list, bad ones included in the N
            const int nc = min(clampi(rec.nCovisible, 0, ORBFE_COVIS_MAX_COVISIBLE), G.nCovisible);
            int cand = -1;
            bool ok = false;
            if (lane < nc) {
                cand = T.covisible[(size_t)s * ORBFE_COVIS_MAX_COVISIBLE + lane];
                ok = (unsigned)cand < (unsigned)T.kfCap && T.kf[cand].bad == 0 && !listed(cand);
            }
            unsigned long long m = __ballot(ok);
            if (m) append(__shfl(cand, __ffsll((long long)m) - 1));
            // (b) the first child, in the caller's order
            const int nch = clampi(rec.nChildren, 0, T.childStride);
            for (int c0 = 0; c0 < nch; c0 += 64) {
                ok = false;
                if (c0 + lane < nch) {
                    cand = T.children[(size_t)s * T.childStride + c0 + lane];
                    ok = (unsigned)cand < (unsigned)T.kfCap && T.kf[cand].bad == 0 && !listed(cand);
                }
                m = __ballot(ok);
                if (m) {
                    append(__shfl(cand, __ffsll((long long)m) - 1));
                    break;
                }
            }
            // (c) the parent, no bad test; the break of :1292 leaves the OUTER loop
            const int par = rec.parent;
            if ((unsigned)par < (unsigned)T.kfCap && !listed(par)) {
                append(par);
                break;
            }
        }
        if (G.inertial) {
            int t = G.lastKf[b];
            for (int k = 0; k < G.nTemporal; k++) {
                if ((unsigned)t >= (unsigned)T.kfCap) break;
                if (listed(t)) break;  // as written (:1306-1312) t does not advance, so no later step can do anything either
                append(t);
                t = T.kf[t].prev;
            }
        }
        int* __restrict__ kfOut = G.localKfs + (size_t)b * kLocalKfMax;
        for (int i = lane; i < kLocalKfMax; i += 64) kfOut[i] = i < len ? list[i] : -1;
        if (lane == 0) G.nLocalKfs[b] = len;
    }
}

// ---- the points (:1135-1153): the list in reverse, slots ascending, first occurrence ----
__global__ __launch_bounds__(kPointsThreads) void local_points_kernel(LocalPointsArgs G)
{
    __shared__ int list[kLocalKfMax];
    __shared__ int prefix[kLocalKfMax + 1];
    __shared__ int waveCount[kPointsWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovisTables& T = G.T;
    const int n = clampi(G.nVotes[b], 0, G.voteStride);
    const size_t voteBase = (size_t)b * G.voteStride;
    unsigned* stamp = G.stamps + (size_t)b * T.cap;
    // mark_voters_seen: a point that voted has bit 31 of its stamp cleared (the bad ones are -1 in the list by now, or read as bad)
    if (G.markVoters)
        for (int i = tid; i < n; i += kPT) {
            const int p = G.voteIds[voteBase + i];
            if (p >= 0 && p < T.cap && G.mapPts[p].bad == 0) atomicAnd(&stamp[p], 0x7fffffffu);
        }
    LM_DRAIN();
    const int nl = clampi(G.nLocalKfs[b], 0, kLocalKfMax);
    for (int r = tid; r < nl; r += kPT) {
        const int s = G.localKfs[(size_t)b * kLocalKfMax + r];  // written by local_kfs_kernel: inside [0, kfCap)
        list[r] = s;
        prefix[nl - r] = clampi(T.kf[s].nFeatures, 0, T.kfStride);
    }
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        prefix[0] = 0;
        for (int r = 1; r <= nl; r++) {
            acc += prefix[r];
            prefix[r] = acc;
        }
    }
    __syncthreads();
    const int W = prefix[nl];
    // the id at walk position q, or -1 when the slot is empty, outside the map or holds a bad point
    auto walk = [&](int q) {
        int lo = 0, hi = nl;  // prefix[lo] <= q < prefix[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= q) lo = mid;
            else hi = mid;
        }
        const int id = T.kfPoints[(size_t)list[nl - 1 - lo] * T.kfStride + (q - prefix[lo])];
        return (id >= 0 && id < T.cap && G.mapPts[id].bad == 0) ? id : -1;
    };
    for (int q = tid; q < W; q += kPT) {
        const int id = walk(q);
        if (id >= 0) {
            const unsigned voted = __hip_atomic_load(&stamp[id], LM_RLX_AGENT) & 0x80000000u;  // fixed since the barrier behind the votes
            atomicMin(&stamp[id], (unsigned)q | voted);
        }
    }
    LM_DRAIN();
    __syncthreads();
    int* __restrict__ idsOut = G.idsOut + (size_t)b * G.M;
    int base = 0;  // block-uniform
    for (int q0 = 0; q0 < W; q0 += kPT) {
        const int q = q0 + tid;
        bool keep = false;
        int emit = 0;
        if (q < W) {
            const int id = walk(q);
            if (id >= 0) {
                const unsigned v = __hip_atomic_load(&stamp[id], LM_RLX_AGENT);
                keep = (v & 0x7fffffffu) == (unsigned)q;
                emit = (G.markVoters && !(v >> 31)) ? ~id : id;
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) waveCount[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kPointsWaves; w++) {
            before += w < wave ? waveCount[w] : 0;
            total += waveCount[w];
        }
        if (keep) {
            const int pos = base + before + __popcll(m & ((1ull << lane) - 1));
            if (pos < G.M) idsOut[pos] = emit;
        }
        base += total;
        __syncthreads();
    }
    for (int pos = base + tid; pos < G.M; pos += kPT) idsOut[pos] = ORBFE_NO_POINT;
    if (tid == 0) G.nLocalPoints[b] = base;
    // every stamp that was touched goes back to rest (the chunk loop ended with a barrier: nobody reads them any more)
    for (int q = tid; q < W; q += kPT) {
        const int id = walk(q);
        if (id >= 0) __hip_atomic_store(&stamp[id], kStampRest, LM_RLX_AGENT);
    }
    // the voters' marks, and the HBM vote counters where local_kfs_kernel used them: every one it touched is named by a voter
    int* counter = G.counters + (size_t)b * (T.kfCap + 1);
    const bool usedHbm = counter[T.kfCap] != 0;
    if (G.markVoters || usedHbm)
        for (int i = tid; i < n; i += kPT) {
            const int p = G.voteIds[voteBase + i];
            if (p < 0 || p >= T.cap || G.mapPts[p].bad != 0) continue;
            if (G.markVoters) __hip_atomic_store(&stamp[p], kStampRest, LM_RLX_AGENT);
            if (usedHbm) {
                const int cnt = clampi(T.obsCount[p], 0, T.obsStride);
                const int* __restrict__ ob = T.obs + (size_t)p * T.obsStride;
                for (int k = 0; k < cnt; k++)
                    if ((unsigned)ob[k] < (unsigned)T.kfCap) counter[ob[k]] = 0;
            }
        }
    __syncthreads();
    if (usedHbm && tid == 0) counter[T.kfCap] = 0;
}

// a slot that was never set: a bad key frame with mn_id == slot and nothing attached
__global__ __launch_bounds__(256) void covis_init_kernel(CovisTables T)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= T.kfCap) return;
    CovisKf k;
    k.mnId = s;
    k.bad = 1;
    k.parent = k.prev = -1;
    k.nFeatures = k.nCovisible = k.nChildren = k.pad = 0;
    T.kf[s] = k;
}

// one block per staged record; every slot, count and offset in it was checked on the host
__global__ __launch_bounds__(256) void covis_scatter_keyframes_kernel(CovisTables T, const int* __restrict__ block)
{
    const CovisStagedKf r = reinterpret_cast<const CovisStagedKf*>(block)[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) {
        CovisKf k;
        k.mnId = r.mnId;
        k.bad = r.bad;
        k.parent = r.parent;
        k.prev = r.prev;
        k.nFeatures = r.nFeatures >= 0 ? r.nFeatures : T.kf[r.slot].nFeatures;
        k.nCovisible = r.nCovisible;
        k.nChildren = r.nChildren;
        k.pad = 0;
        T.kf[r.slot] = k;
    }
    for (int j = tid; j < r.nFeatures; j += 256) T.kfPoints[(size_t)r.slot * T.kfStride + j] = block[r.oPoints + j];
    for (int j = tid; j < r.nCovisible; j += 256) T.covisible[(size_t)r.slot * ORBFE_COVIS_MAX_COVISIBLE + j] = block[r.oCovisible + j];
    for (int j = tid; j < r.nChildren; j += 256) T.children[(size_t)r.slot * T.childStride + j] = block[r.oChildren + j];
}

__global__ __launch_bounds__(256) void covis_scatter_observations_kernel(CovisTables T, int n, const int* __restrict__ ids,
                                                                         const int* __restrict__ off, const int* __restrict__ slots)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = ids[i], o = off[i], cnt = off[i + 1] - o;
    for (int k = 0; k < cnt; k++) T.obs[(size_t)p * T.obsStride + k] = slots[o + k];
    T.obsCount[p] = cnt;
}

__global__ __launch_bounds__(256) void frame_points_kernel(int kpStride, int M, int mapCap, const orbfe_world_point* __restrict__ mapPts,
                                                           const int* __restrict__ ids, const int* __restrict__ match,
                                                           const uint8_t* __restrict__ outlier, const int* __restrict__ nKp,
                                                           int* __restrict__ out)
{
    const int b = blockIdx.x, i = blockIdx.y * 256 + threadIdx.x;  // kp_stride <= 65536: at most 256 chunks
    if (i >= kpStride) return;
    const size_t at = (size_t)b * kpStride + i;
    int res = -1;
    if (i < nKp[b]) {
        const int m = match[at];
        if (m >= 0 && m < M && outlier[at] == 0) {
            const int id = ids[(size_t)b * M + m];
            if (id >= 0 && id < mapCap && mapPts[id].observations >= 1) res = id;
        }
    }
    out[at] = res;
}

// the parameter block alone: no handle, no device
int local_map_check(const orbfe_local_map_params* P, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_local_map_params)) {
        err = "orbfe_local_map_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    if (P->max_local_kf < 1 || P->max_local_kf > 64 || P->n_covisible < 0 || P->n_covisible > ORBFE_COVIS_MAX_COVISIBLE ||
        P->n_temporal < 0 || P->n_temporal > 32)
        return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

int covis_init_launch(hipStream_t s, const CovisTables& T, std::string& err)
{
    hipLaunchKernelGGL(covis_init_kernel, dim3((T.kfCap + 255) / 256), dim3(256), 0, s, T);
    MCHK(hipGetLastError());
    MCHK(hipMemsetAsync(T.obsCount, 0, (size_t)T.cap * sizeof(int), s));
    return ORBFE_OK;
}

int covis_scatter_keyframes_launch(hipStream_t s, const CovisTables& T, int n, const int* dBlock, std::string& err)
{
    hipLaunchKernelGGL(covis_scatter_keyframes_kernel, dim3(n), dim3(256), 0, s, T, dBlock);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_scatter_observations_launch(hipStream_t s, const CovisTables& T, int n, const int* dIds, const int* dOff, const int* dSlots,
                                      std::string& err)
{
    hipLaunchKernelGGL(covis_scatter_observations_kernel, dim3((n + 255) / 256), dim3(256), 0, s, T, n, dIds, dOff, dSlots);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int local_map_launch(hipStream_t s, const orbfe_local_map_params* P, int batch, int voteStride, const CovisTables& T,
                     const orbfe_world_point* mapPts, int M, const orbfe_local_map_io* io, unsigned* stamps, int* counters, std::string& err)
{
    LocalMapArgs G;
    memset(&G, 0, sizeof G);
    G.T = T;
    G.mapPts = mapPts;
    G.maxLocalKf = P->max_local_kf;
    G.voteIds = io->d_vote_ids;
    G.nVotes = io->d_n_votes;
    G.voteStride = voteStride;
    G.localKfs = io->d_local_kfs;
    G.nLocalKfs = io->d_n_local_kfs;
    G.voteIdsOut = io->d_vote_ids_out;
    G.counters = counters;
    hipLaunchKernelGGL(local_votes_kernel<false>, dim3(batch), dim3(kT), 0, s, G);
    MCHK(hipGetLastError());
    hipLaunchKernelGGL(local_votes_kernel<true>, dim3(batch), dim3(kT), 0, s, G);
    MCHK(hipGetLastError());
    LocalListArgs L;
    memset(&L, 0, sizeof L);
    L.T = T;
    L.nCovisible = P->n_covisible;
    L.nTemporal = P->n_temporal;
    L.inertial = P->inertial != 0;
    L.lastKf = io->d_last_kf;
    L.localKfs = io->d_local_kfs;
    L.nLocalKfs = io->d_n_local_kfs;
    L.bitmapWords = (T.kfCap + 31) / 32;
    hipLaunchKernelGGL(local_list_kernel, dim3(batch), dim3(64), (size_t)L.bitmapWords * sizeof(unsigned), s, L);
    MCHK(hipGetLastError());
    LocalPointsArgs Q;
    memset(&Q, 0, sizeof Q);
    Q.T = T;
    Q.mapPts = mapPts;
    Q.markVoters = P->mark_voters_seen != 0;
    Q.voteIds = io->d_vote_ids_out ? io->d_vote_ids_out : io->d_vote_ids;  // the same ids but for the bad ones, which do not count
    Q.nVotes = io->d_n_votes;
    Q.voteStride = voteStride;
    Q.M = M;
    Q.localKfs = io->d_local_kfs;
    Q.nLocalKfs = io->d_n_local_kfs;
    Q.idsOut = io->d_ids_out;
    Q.nLocalPoints = io->d_n_local_points;
    Q.stamps = stamps;
    Q.counters = counters;
    hipLaunchKernelGGL(local_points_kernel, dim3(batch), dim3(kPT), 0, s, Q);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int frame_points_launch(hipStream_t s, int batch, int kpStride, int M, int mapCap, const orbfe_world_point* mapPts, const int* dIds,
                        const int* dMatch, const uint8_t* dOutlier, const int* dN, int* dOut, std::string& err)
{
    hipLaunchKernelGGL(frame_points_kernel, dim3(batch, (kpStride + 255) / 256), dim3(256), 0, s, kpStride, M, mapCap, mapPts, dIds, dMatch,
                       dOutlier, dN, dOut);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

// kernels_covis_update.hip -- KeyFrame::UpdateConnections (src/KeyFrame.cc:459-553) with AddConnection (:191-204) and
// UpdateBestCovisibles (:206-228), and the graph part of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:338-361), on the resident
// covisibility graph.  SPEC DECISION S25; tests/covis_update_ref.py is the normative restatement.
//
// One key frame s of UpdateConnections is four launches back to back on one stream; the launches of the next key frame of a call follow
// in stream order, so each key frame meets the graph as the one before left it.  No block waits on another, nothing spins.
//   covis_count_kernel<false>  ONE block: a thread per feature slot of s walks its point's observation list into an LDS table keyed by
//              key-frame slot (the table of local_votes_kernel: open addressing, 2 * ORBFE_LOCAL_MAP_VOTE_TABLE entries, the 513th
//              distinct key marks the graph's counter row as in use and leaves).  Observers that are s or bad are not counted.  The
//              counted key frames are then appended, in no particular order, to the work block: slot, weight, mn_id.
//   covis_count_kernel<true>   returns at once unless the row is marked; then the same counts into the row (one int per key-frame slot,
//              all zero when the call starts), the same append, and every counter it read is put back to zero.
//   covis_select_kernel        ONE block: the threshold, the fallback to the largest count (lowest mn_id), the rank of every connected
//              key frame = the number of connected ones that precede it under the total order (weight, mn_id, slot) descending, so the
//              order of the appends cannot show; the ordered list goes to the caller's rows.  Then the check pass: a counted set
//              larger than conn_stride, a full row of a neighbour that does not hold s yet, a full children row of the new parent --
//              any of them sets the refuse word of the work block, and nothing of this key frame is written.
//   covis_apply_kernel         returns block-uniformly on the refuse word.  kApplyBlocks blocks of one wave walk the connected list,
//              a neighbour q per wave at a time: s is looked up in q's row with a ballot, the three-way rule of AddConnection is
//              applied, and where the row changed the best ORBFE_COVIS_MAX_COVISIBLE entries that are not bad NOW are selected by
//              rounds of a wave-wide arg-best, each round taking the best entry strictly behind the winner before it.  Rows of
//              different q are disjoint.  One more block writes the own lists of s, its parent and the parent's children row.
// covis_add_keyframe_kernel: ONE block.  Every valid feature slot does an integer min of its index on its point's stamp (the
// first-occurrence stamps of local_points_kernel, put back afterwards): the holder of the stamp is the LOWEST slot of that point.  The
// holders look for s in the observation list and test its capacity; behind a barrier, and only when no list is full, the same
// threads append.
// Stamps and counters are read with agent-scope atomic loads: they are written by atomics that complete in L2, and a wave waits for
// its own before the barrier behind which the block's other waves read them.  Every loop is bounded by a stride or a count clamped
// to it; every slot read from a table is range-tested before it indexes.  None of the kernels uses scratch memory or spills a register
// (tests/test_covis_update_budget.py); the table insert is kept from unrolling for that, as in kernels_local_map.hip.
#include "covis_update.h"
#include "match_common.h"

namespace orbfe {

namespace {

constexpr int kT = kUpdateThreads;
constexpr int kWaves = kT / 64;
constexpr int kH = kVoteTableSlots;
constexpr int kHead = ORBFE_COVIS_MAX_COVISIBLE;

#define CU_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
// this wave's stores and atomics have reached L2: in front of the barrier behind which other waves of the block load them
#define CU_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

struct CountArgs {
    CovisTables T;
    CovisConn C;
    const orbfe_world_point* mapPts;
    int s;
    int* counters;  // [kfCap + 1]
};

struct SelectArgs {
    CovisTables T;
    CovisConn C;
    int s, flag, minWeight;
    int *oSlots, *oWeights, *oCount, *oStatus;
};

struct ApplyArgs {
    CovisTables T;
    CovisConn C;
    int s, flag;
    const int *oSlots, *oWeights;
};

struct AddArgs {
    CovisTables T;
    int* connCount;  // null: connections not enabled
    const orbfe_world_point* mapPts;
    CovisKf rec;
    int s;
    const int* ids;
    int* added;
    int* status;
    unsigned* stamps;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned vote_hash(int slot) { return ((unsigned)slot * 2654435761u) >> 22 & (kH - 1); }

// the order of mvpOrderedConnectedKeyFrames (S25): weight descending, then mn_id descending, as one word; then slot descending
__device__ __forceinline__ unsigned long long order_key(int weight, int mnId) { return ((unsigned long long)(unsigned)weight << 32) | (unsigned)mnId; }
__device__ __forceinline__ bool precedes(unsigned long long ka, int sa, unsigned long long kb, int sb) { return ka > kb || (ka == kb && sa > sb); }

// the id at feature slot i of the new key frame, or -1: empty, outside the map, a bad point
__device__ __forceinline__ int point_at(const AddArgs& G, int i)
{
    const int p = G.ids[i];
    return (p >= 0 && p < G.T.cap && G.mapPts[p].bad == 0) ? p : -1;
}

// IsInKeyFrame: -1 when the observation list of p names s, its length otherwise
__device__ __forceinline__ int list_length_unless_listed(const CovisTables& T, int p, int s)
{
    const int n = clampi(T.obsCount[p], 0, T.obsStride);
    const int* __restrict__ ob = T.obs + (size_t)p * T.obsStride;
    bool found = false;
    for (int k = 0; k < n; k++) found = found || ob[k] == s;
    return found ? -1 : n;
}

}  // namespace

// ---- counting (:471-490) ----
template <bool kHbm>
__global__ __launch_bounds__(kUpdateThreads) void covis_count_kernel(CountArgs G)
{
    __shared__ int keys[kHbm ? 1 : kH], counts[kHbm ? 1 : kH];
    __shared__ int nDistinct, overflow, nOut;

    const int tid = threadIdx.x;
    const CovisTables& T = G.T;
    const int s = G.s, S = G.C.connStride;
    int* counter = G.counters;                      // the row's last word: the row is in use
    if (kHbm && counter[T.kfCap] == 0) return;      // block-uniform

    if (!kHbm)
        for (int e = tid; e < kH; e += kT) {
            keys[e] = -1;
            counts[e] = 0;
        }
    if (tid == 0) nDistinct = overflow = nOut = 0;
    __syncthreads();

    const int nf = clampi(T.kf[s].nFeatures, 0, T.kfStride);
    const int* __restrict__ pts = T.kfPoints + (size_t)s * T.kfStride;
    for (int i = tid; i < nf; i += kT) {
        const int p = pts[i];
        if (p < 0 || p >= T.cap || G.mapPts[p].bad != 0) continue;
        const int cnt = clampi(T.obsCount[p], 0, T.obsStride);
        const int* __restrict__ ob = T.obs + (size_t)p * T.obsStride;
#pragma unroll 1
        for (int k = 0; k < cnt; k++) {
            const int slot = ob[k];
            if ((unsigned)slot >= (unsigned)T.kfCap || slot == s || T.kf[slot].bad != 0) continue;  // :485
            if (kHbm) {
                atomicAdd(&counter[slot], 1);
                continue;
            }
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
    if (kHbm) CU_DRAIN();
    __syncthreads();
    if (!kHbm && overflow != 0) {  // block-uniform
        if (tid == 0) counter[T.kfCap] = 1;
        return;
    }

    // the counted key frames, in the order the appends arrive in: covis_select_kernel ranks them by a total order
    int* __restrict__ wSlot = G.C.work + kWorkHead;
    int* __restrict__ wWeight = wSlot + S;
    int* __restrict__ wMn = wWeight + S;
    const int nEntries = kHbm ? T.kfCap : kH;
#pragma unroll 1
    for (int e = tid; e < nEntries; e += kT) {
        const int c = kHbm ? __hip_atomic_load(&counter[e], CU_RLX_AGENT) : counts[e];
        if (c <= 0) continue;
        const int slot = kHbm ? e : keys[e];
        const int at = atomicAdd(&nOut, 1);
        if (at < S) {
            wSlot[at] = slot;
            wWeight[at] = c;
            wMn[at] = T.kf[slot].mnId;
        }
        if (kHbm) __hip_atomic_store(&counter[e], 0, CU_RLX_AGENT);
    }
    __syncthreads();
    if (tid == 0) {
        G.C.work[0] = nOut;  // may exceed S: the key frame is refused
        if (kHbm) counter[T.kfCap] = 0;
    }
}

// ---- selection (:498-526), the ordered list (:528-535) and the capacity check ----
__global__ __launch_bounds__(kUpdateThreads) void covis_select_kernel(SelectArgs G)
{
    __shared__ unsigned long long waveKey[kWaves];
    __shared__ int waveSlot[kWaves];
    __shared__ int nAbove, refuse, front, present, maxSlot;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CovisTables& T = G.T;
    const int s = G.s, S = G.C.connStride, th = G.minWeight;
    int* __restrict__ work = G.C.work;
    const int nC = work[0];
    if (nC <= 0 || nC > S) {  // block-uniform: no counts (:493), or more counted key frames than a row takes
        for (int i = tid; i < S; i += kT) {
            G.oSlots[i] = -1;
            G.oWeights[i] = 0;
        }
        if (tid == 0) {
            *G.oCount = 0;
            *G.oStatus = nC <= 0 ? ORBFE_COVIS_STATUS_NO_COUNTS : ORBFE_COVIS_STATUS_REFUSED;
            work[1] = 1;
            work[2] = 0;
        }
        return;
    }
    const int* __restrict__ wSlot = work + kWorkHead;
    const int* __restrict__ wWeight = wSlot + S;
    const int* __restrict__ wMn = wWeight + S;
    if (tid == 0) nAbove = refuse = present = 0;
    __syncthreads();

    // how many reach the threshold, and the largest count: lowest mn_id among equal maxima, then lowest slot
    {
        int above = 0, bs = 0x7fffffff;
        unsigned long long bk = 0;
        for (int i = tid; i < nC; i += kT) {
            const int w = wWeight[i], sl = wSlot[i];
            above += w >= th;
            const unsigned long long k = ((unsigned long long)(unsigned)w << 32) | (unsigned)(0x7fffffff - wMn[i]);
            if (k > bk || (k == bk && sl < bs)) { bk = k; bs = sl; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long ok = __shfl_xor(bk, d);
            const int os = __shfl_xor(bs, d);
            if (ok > bk || (ok == bk && os < bs)) { bk = ok; bs = os; }
        }
        if (above) atomicAdd(&nAbove, above);
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
                if (waveKey[w] > bk || (waveKey[w] == bk && waveSlot[w] < bs)) { bk = waveKey[w]; bs = waveSlot[w]; }
            maxSlot = bs;
        }
        __syncthreads();
    }
    const bool fallback = nAbove == 0;
    const int nConn = fallback ? 1 : nAbove;

    for (int i = tid; i < nC; i += kT) {
        const int w = wWeight[i], sl = wSlot[i];
        if (fallback ? sl != maxSlot : w < th) continue;
        const unsigned long long key = order_key(w, wMn[i]);
        int rank = 0;
        if (!fallback)
            for (int j = 0; j < nC; j++) {
                const int wj = wWeight[j];
                rank += wj >= th && precedes(order_key(wj, wMn[j]), wSlot[j], key, sl);
            }
        G.oSlots[rank] = sl;  // rank < nConn <= nC <= S
        G.oWeights[rank] = w;
        if (rank == 0) front = sl;
        // AddConnection would insert s into this key frame's row: is there room (sl is a table key: inside [0, kfCap))
        const int n = clampi(G.C.count[sl], 0, S);
        const int* __restrict__ row = G.C.slots + (size_t)sl * S;
        bool found = false;
        for (int k = 0; k < n; k++) found = found || row[k] == s;
        if (!found && n >= S) refuse = 1;
    }
    for (int i = nConn + tid; i < S; i += kT) {
        G.oSlots[i] = -1;
        G.oWeights[i] = 0;
    }
    CU_DRAIN();
    __syncthreads();
    if (G.flag & 1) {  // :545-550: the children row of the parent-to-be
        const int p = front;
        const int nch = clampi(T.kf[p].nChildren, 0, T.childStride);
        for (int c = tid; c < nch; c += kT)
            if (T.children[(size_t)p * T.childStride + c] == s) present = 1;
        __syncthreads();
        if (tid == 0 && present == 0 && nch >= T.childStride) refuse = 1;
        __syncthreads();
    }
    const int ref = refuse;  // block-uniform
    if (ref)
        for (int i = tid; i < nConn; i += kT) {
            G.oSlots[i] = -1;
            G.oWeights[i] = 0;
        }
    if (tid == 0) {
        *G.oCount = ref ? 0 : nConn;
        *G.oStatus = ref ? ORBFE_COVIS_STATUS_REFUSED : ORBFE_COVIS_STATUS_OK;
        work[1] = ref;
        work[2] = ref ? 0 : nConn;
    }
}

// ---- the reciprocal AddConnection + UpdateBestCovisibles (:191-228), the own lists (:537-543) and the parent (:545-550) ----
__global__ __launch_bounds__(64) void covis_apply_kernel(ApplyArgs G)
{
    const CovisTables& T = G.T;
    const int* __restrict__ work = G.C.work;
    if (work[1] != 0) return;  // block-uniform: refused, or nothing counted
    const int lane = threadIdx.x, s = G.s, S = G.C.connStride;
    const int nC = clampi(work[0], 0, S), nConn = clampi(work[2], 0, nC);

    if (blockIdx.x == kApplyBlocks) {  // the own lists: mConnectedKeyFrameWeights = KFcounter, the whole of it
        const int* __restrict__ wSlot = work + kWorkHead;
        const int* __restrict__ wWeight = wSlot + S;
        for (int i = lane; i < nC; i += 64) {
            G.C.slots[(size_t)s * S + i] = wSlot[i];
            G.C.weights[(size_t)s * S + i] = wWeight[i];
        }
        const int nh = min(nConn, kHead);
        if (lane < nh) T.covisible[(size_t)s * kHead + lane] = G.oSlots[lane];
        if (lane == 0) {
            G.C.count[s] = nC;
            T.kf[s].nCovisible = nh;
        }
        if ((G.flag & 1) && nConn > 0) {
            const int p = G.oSlots[0];
            if ((unsigned)p >= (unsigned)T.kfCap) return;
            const int nch = clampi(T.kf[p].nChildren, 0, T.childStride);
            bool found = false;  // wave-uniform
            for (int c0 = 0; c0 < nch; c0 += 64) {
                const bool hit = c0 + lane < nch && T.children[(size_t)p * T.childStride + c0 + lane] == s;
                if (__ballot(hit)) {
                    found = true;
                    break;
                }
            }
            if (lane == 0) {
                T.kf[s].parent = p;
                if (!found && nch < T.childStride) {  // (room was checked by covis_select_kernel)
                    T.children[(size_t)p * T.childStride + nch] = s;
                    T.kf[p].nChildren = nch + 1;
                }
            }
        }
        return;
    }

    for (int j = blockIdx.x; j < nConn; j += kApplyBlocks) {
        const int q = G.oSlots[j], w = G.oWeights[j];
        if ((unsigned)q >= (unsigned)T.kfCap) continue;
        int n = clampi(G.C.count[q], 0, S);
        int* __restrict__ row = G.C.slots + (size_t)q * S;
        int* __restrict__ rw = G.C.weights + (size_t)q * S;
        int at = -1, old = 0;  // wave-uniform
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool hit = k < n && row[k] == s;
            const int wk = hit ? rw[k] : 0;
            const unsigned long long m = __ballot(hit);
            if (m) {
                const int l = __ffsll((long long)m) - 1;
                at = k0 + l;
                old = __shfl(wk, l);
                break;
            }
        }
        if (at >= 0 && old == w) continue;  // the same weight: nothing happens to q at all (:199-200)
        if (at < 0) {
            if (n >= S) continue;  // (room was checked by covis_select_kernel)
            at = n;
            n = n + 1;
            if (lane == 0) {
                row[at] = s;
                rw[at] = w;
                G.C.count[q] = n;
            }
        } else if (lane == 0)
            rw[at] = w;
        // UpdateBestCovisibles: round r takes the best entry strictly behind the winner of round r - 1; entry `at` is read from the
        // registers, the others were not written
        unsigned long long prevKey = ~0ull;
        int prevSlot = 0x7fffffff, nh = 0;
#pragma unroll 1
        for (int r = 0; r < kHead; r++) {
            unsigned long long bk = 0;
            int bs = -1;
#pragma unroll 1
            for (int k = lane; k < n; k += 64) {
                const int sl = k == at ? s : row[k];
                if ((unsigned)sl >= (unsigned)T.kfCap || T.kf[sl].bad != 0) continue;
                const unsigned long long key = order_key(k == at ? w : rw[k], T.kf[sl].mnId);
                if (!precedes(prevKey, prevSlot, key, sl)) continue;
                if (bs < 0 || precedes(key, sl, bk, bs)) { bk = key; bs = sl; }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long ok = __shfl_xor(bk, d);
                const int os = __shfl_xor(bs, d);
                if (os >= 0 && (bs < 0 || precedes(ok, os, bk, bs))) { bk = ok; bs = os; }
            }
            if (bs < 0) break;  // wave-uniform
            if (lane == 0) T.covisible[(size_t)q * kHead + r] = bs;
            nh = r + 1;
            prevKey = bk;
            prevSlot = bs;
        }
        if (lane == 0) T.kf[q].nCovisible = nh;
    }
}

// ---- LocalMapping::ProcessNewKeyFrame, the graph part (:338-361) ----
__global__ __launch_bounds__(kAddThreads) void covis_add_keyframe_kernel(AddArgs G)
{
    __shared__ int refuse;
    const int tid = threadIdx.x, s = G.s;
    const CovisTables& T = G.T;
    const int nf = clampi(G.rec.nFeatures, 0, T.kfStride);
    unsigned* stamp = G.stamps;
    if (tid == 0) refuse = 0;
    for (int i = tid; i < nf; i += kAddThreads) {
        const int p = point_at(G, i);
        if (p >= 0) atomicMin(&stamp[p], (unsigned)i);
    }
    CU_DRAIN();
    __syncthreads();
    // the check pass: the lowest feature slot of every point speaks for it
    for (int i = tid; i < nf; i += kAddThreads) {
        const int p = point_at(G, i);
        if (p < 0 || __hip_atomic_load(&stamp[p], CU_RLX_AGENT) != (unsigned)i) continue;
        if (list_length_unless_listed(T, p, s) >= T.obsStride) refuse = 1;
    }
    __syncthreads();
    const int ref = refuse;  // block-uniform
    for (int i = tid; i < nf; i += kAddThreads) {
        const int raw = G.ids[i], p = point_at(G, i);
        int a = 0;
        if (p >= 0) {
            a = 2;  // :353-356, and the higher feature slot of a point held twice
            const int n = __hip_atomic_load(&stamp[p], CU_RLX_AGENT) == (unsigned)i ? list_length_unless_listed(T, p, s) : -1;
            if (n >= 0) {
                a = 1;
                if (!ref) {
                    T.obs[(size_t)p * T.obsStride + n] = s;
                    T.obsCount[p] = n + 1;
                }
            }
        }
        G.added[i] = ref ? 0 : a;
        if (!ref) T.kfPoints[(size_t)s * T.kfStride + i] = raw;
    }
    if (tid == 0) {
        if (!ref) {
            CovisKf k;  // a new key frame: no covisibles, no children
            k.mnId = G.rec.mnId;
            k.bad = G.rec.bad;
            k.parent = G.rec.parent;
            k.prev = G.rec.prev;
            k.nFeatures = nf;
            k.nCovisible = k.nChildren = k.pad = 0;
            T.kf[s] = k;
            if (G.connCount) G.connCount[s] = 0;
        }
        *G.status = ref ? ORBFE_COVIS_STATUS_REFUSED : ORBFE_COVIS_STATUS_OK;
    }
    __syncthreads();  // nobody reads a stamp any more
    for (int i = tid; i < nf; i += kAddThreads) {
        const int p = point_at(G, i);
        if (p >= 0) __hip_atomic_store(&stamp[p], kStampRest, CU_RLX_AGENT);
    }
}

// one thread per imported row; every slot, count and offset was checked on the host
__global__ __launch_bounds__(256) void covis_scatter_connections_kernel(CovisConn C, int n, const int* __restrict__ slots,
                                                                        const int* __restrict__ off, const int* __restrict__ conn,
                                                                        const int* __restrict__ weights)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = slots[i], o = off[i], cnt = off[i + 1] - o;
    for (int k = 0; k < cnt; k++) {
        C.slots[(size_t)s * C.connStride + k] = conn[o + k];
        C.weights[(size_t)s * C.connStride + k] = weights[o + k];
    }
    C.count[s] = cnt;
}

// the parameter block alone: no handle, no device
int covis_update_check(const orbfe_covis_update_params* P, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_covis_update_params)) {
        err = "orbfe_covis_update_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    if (P->min_weight < 1 || P->min_weight > kCovisMaxMinWeight) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

int covis_conn_init_launch(hipStream_t s, const CovisTables& T, const CovisConn& C, std::string& err)
{
    const size_t rows = (size_t)T.kfCap * C.connStride * sizeof(int);
    MCHK(hipMemsetAsync(C.slots, 0xff, rows, s));
    MCHK(hipMemsetAsync(C.weights, 0, rows, s));
    MCHK(hipMemsetAsync(C.count, 0, (size_t)T.kfCap * sizeof(int), s));
    MCHK(hipMemsetAsync(C.work, 0, ((size_t)kWorkHead + 3 * (size_t)C.connStride) * sizeof(int), s));
    return ORBFE_OK;
}

int covis_scatter_connections_launch(hipStream_t s, const CovisTables& T, const CovisConn& C, int n, const int* dSlots, const int* dOff,
                                     const int* dConn, const int* dWeights, std::string& err)
{
    (void)T;
    hipLaunchKernelGGL(covis_scatter_connections_kernel, dim3((n + 255) / 256), dim3(256), 0, s, C, n, dSlots, dOff, dConn, dWeights);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_update_launch(hipStream_t s, const CovisTables& T, const CovisConn& C, const orbfe_world_point* mapPts, int minWeight, int slot,
                        int flag, int* dSlots, int* dWeights, int* dCount, int* dStatus, int* counters, std::string& err)
{
    CountArgs A;
    memset(&A, 0, sizeof A);
    A.T = T;
    A.C = C;
    A.mapPts = mapPts;
    A.s = slot;
    A.counters = counters;
    hipLaunchKernelGGL(covis_count_kernel<false>, dim3(1), dim3(kT), 0, s, A);
    MCHK(hipGetLastError());
    hipLaunchKernelGGL(covis_count_kernel<true>, dim3(1), dim3(kT), 0, s, A);
    MCHK(hipGetLastError());
    SelectArgs B;
    memset(&B, 0, sizeof B);
    B.T = T;
    B.C = C;
    B.s = slot;
    B.flag = flag;
    B.minWeight = minWeight;
    B.oSlots = dSlots;
    B.oWeights = dWeights;
    B.oCount = dCount;
    B.oStatus = dStatus;
    hipLaunchKernelGGL(covis_select_kernel, dim3(1), dim3(kT), 0, s, B);
    MCHK(hipGetLastError());
    ApplyArgs D;
    memset(&D, 0, sizeof D);
    D.T = T;
    D.C = C;
    D.s = slot;
    D.flag = flag;
    D.oSlots = dSlots;
    D.oWeights = dWeights;
    hipLaunchKernelGGL(covis_apply_kernel, dim3(kApplyBlocks + 1), dim3(64), 0, s, D);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

int covis_add_keyframe_launch(hipStream_t s, const CovisTables& T, const CovisConn* conn, const orbfe_world_point* mapPts, const CovisKf& rec,
                              int slot, const int* dPointIds, int* dAdded, int* dStatus, unsigned* stamps, std::string& err)
{
    AddArgs A;
    memset(&A, 0, sizeof A);
    A.T = T;
    A.connCount = conn ? conn->count : nullptr;
    A.mapPts = mapPts;
    A.rec = rec;
    A.s = slot;
    A.ids = dPointIds;
    A.added = dAdded;
    A.status = dStatus;
    A.stamps = stamps;
    hipLaunchKernelGGL(covis_add_keyframe_kernel, dim3(1), dim3(kAddThreads), 0, s, A);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

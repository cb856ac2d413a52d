// block_tree.h -- the fixed pairwise tree of S14 / S17 / S19 over one block: what kernels_poseopt.hip, kernels_initial_ba.hip and
// kernels_poseimu.hip share of it.
// A sum over P = 2^m items (+0.0 for the padding) is taken level by level, item 2i with item 2i + 1 first, then pairs of pairs: the
// bottom levels inside a thread that owns an aligned run of items (run_tree), the next up to 6 levels inside the wave (wave_level_add:
// DPP quad swaps, row_half_mirror, row_mirror, then two lane-xor exchanges, so every lane ends with the wave's sum) -- or, for long
// runs, chunk by chunk by the wave with the six wave levels first (wave_run_tree) --, the last levels across the waves through a
// double-buffered LDS block that every thread reads (block_tree).  Levels above log2 P are not taken: adding a padding +0.0 would turn
// a -0.0 sum into +0.0.  Device code only; contraction is off in every including unit.
#pragma once
#include <hip/hip_runtime.h>

namespace orbfe {

constexpr int kTreeThreads = 256;
constexpr int kTreeMaxWaves = kTreeThreads / 64;
constexpr int kTreeStack = 8;              // log2(65536 / kTreeThreads): the deepest run of one thread

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// level l of the tree inside a wave: every lane adds the sum held by the other half of its 2^(l+1)-lane group.  All 64 lanes active.
__device__ __forceinline__ double wave_level_add(double v, int l)
{
    switch (l) {
    case 0: return v + dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    case 1: return v + dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    case 2: return v + dpp_f64<0x141>(v);   // row_half_mirror: a lane of the other quad, which holds that quad's sum
    case 3: return v + dpp_f64<0x140>(v);   // row_mirror
    case 4: return v + __shfl_xor(v, 16);
    default: return v + __shfl_xor(v, 32);
    }
}

// the shape of the tree for this block
struct TreeShape {
    int run;        // items per thread, or chunks per wave
    int lvWave;     // levels inside a wave (0 after wave_run_tree, which takes all six per chunk)
    int lvCross;    // levels across waves
};

// sums NV per-thread values over the block by the tree; every thread returns the sums.  S.part is [2][kTreeMaxWaves][>= NV + NM]
// doubles of LDS; `flip` is the block-uniform parity of the LDS buffer: a wave that writes buffer f again has passed the barrier of
// the sum in between, which every wave reaches only after it has read f.
// The NM values behind the sums (v[NV .. NV + NM), default none) travel in the same exchange and are reduced to their maximum over
// all threads of the block instead, found with '>': lanes and waves without items hold 0.0, and of values none of which is a NaN the
// maximum is the same bits in any order.
template <int NV, int NM = 0, class Shared, int NA>
__device__ __forceinline__ void block_tree(Shared& S, const TreeShape& T, int& flip, double (&v)[NA])
{
    static_assert(NA == NV + NM, "v holds the NV sums, then the NM maxima");
    for (int l = 0; l < T.lvWave; l++) {
#pragma unroll
        for (int k = 0; k < NV; k++) v[k] = wave_level_add(v[k], l);
    }
#pragma unroll
    for (int k = NV; k < NA; k++) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double o = __shfl_xor(v[k], d);
            if (o > v[k]) v[k] = o;
        }
    }
    if (blockDim.x == 64) {   // lanes past P hold sums of padding only: every lane takes lane 0's
#pragma unroll
        for (int k = 0; k < NV; k++)
            v[k] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v[k])), __builtin_amdgcn_readfirstlane(__double2loint(v[k])));
        return;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // This barrier sits inside loops (iterations, trials) whose trip counts depend on computed values.  It is reached by all threads
    // or by none because those values are bit-identical in every thread: each reads the same sums from LDS below and runs the same
    // contraction-free sequence on them.  Anything that made a thread's copy differ (a per-thread shortcut, a fast-math flag) would
    // hang the block here.
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NA; k++) S.part[flip][wave][k] = v[k];
    }
    __syncthreads();
    const int nw = 1 << T.lvCross;   // 1, 2 or 4
#pragma unroll
    for (int k = 0; k < NV; k++) {
        const double a = S.part[flip][0][k];
        if (nw == 1) v[k] = a;
        else if (nw == 2) v[k] = a + S.part[flip][1][k];
        else v[k] = (a + S.part[flip][1][k]) + (S.part[flip][2][k] + S.part[flip][3][k]);
    }
#pragma unroll
    for (int k = NV; k < NA; k++) {
        double m = S.part[flip][0][k];
#pragma unroll
        for (int w = 1; w < kTreeMaxWaves; w++) {
            const double o = S.part[flip][w][k];
            if (o > m) m = o;
        }
        v[k] = m;
    }
    flip ^= 1;
}

// The per-thread part of a sum: term(k, v) fills the NV values of the k-th item of the run (+0.0 when it is inactive or past the end).
// RUN = 1, 2, 4: unrolled; RUN = 0: a run of `run` = 2^m > 4 items walked with a binary counter, so that v(2i) + v(2i + 1) are
// added first, then pairs of pairs: the same tree.
template <int RUN, int NV, class Term>
__device__ __forceinline__ void run_tree(int run, double (&out)[NV], Term term)
{
    if (RUN == 1) {
        term(0, out);
    } else if (RUN == 2) {
        double b[NV];
        term(0, out);
        term(1, b);
#pragma unroll
        for (int k = 0; k < NV; k++) out[k] = out[k] + b[k];
    } else if (RUN == 4) {
        double b[NV], c[NV], d[NV];
        term(0, out);
        term(1, b);
        term(2, c);
        term(3, d);
#pragma unroll
        for (int k = 0; k < NV; k++) out[k] = (out[k] + b[k]) + (c[k] + d[k]);
    } else {
        double st[kTreeStack][NV];
        for (int i = 0; i < run; i++) {
            term(i, out);
            int lvl = 0;
            for (int m = i; m & 1; m >>= 1, lvl++) {
                for (int k = 0; k < NV; k++) out[k] = st[lvl][k] + out[k];
            }
            if (i + 1 < run)
                for (int k = 0; k < NV; k++) st[lvl][k] = out[k];
        }
    }
}

__device__ __forceinline__ double readlane_f64(double v, int lane)   // `lane` is wave-uniform
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The same part for a run of `run` chunks of 64 items walked by the WAVE: term(c, v) fills this lane's item of chunk c, the six wave
// levels sum the chunk, the binary counter adds chunk 2i to chunk 2i + 1 first; level j of its stack is held by lane j.  64 lanes active.
template <int NV, class Term>
__device__ __forceinline__ void wave_run_tree(int run, double (&out)[NV], Term term)
{
    const int lane = threadIdx.x & 63;
    double st[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) st[k] = 0.0;
    for (int c = 0; c < run; c++) {
        term(c, out);
        for (int l = 0; l < 6; l++) {
#pragma unroll
            for (int k = 0; k < NV; k++) out[k] = wave_level_add(out[k], l);
        }
        int lvl = 0;
        for (int m = c; m & 1; m >>= 1, lvl++) {
#pragma unroll
            for (int k = 0; k < NV; k++) out[k] = readlane_f64(st[k], lvl) + out[k];
        }
        if (c + 1 < run && lane == lvl) {
#pragma unroll
            for (int k = 0; k < NV; k++) st[k] = out[k];
        }
    }
}

}  // namespace orbfe

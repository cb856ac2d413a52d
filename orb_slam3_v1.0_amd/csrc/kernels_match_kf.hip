// kernels_match_kf.hip -- the key-frame searches of ORBmatcher on gfx950: the search part of both Fuse overloads
// (src/ORBmatcher.cc:678-836, 864-975), SearchBySim3 (:977-1200) and the relocalisation overload of SearchByProjection
// (:1202-1326).  Thread per map point on the per-level cell tables that kernels_match_proj.hip builds for a frame
// (proj_prepare_launch); the relocalisation overload is order-dependent and runs on the projection pipeline itself
// (proj_launch in kModeReloc) between its own projection and rotation-histogram kernels.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device_math.h"
#include "match_common.h"
#include "match_proj.h"
#include "keyframe.h"

#pragma clang fp contract(off)

namespace orbfe {

using namespace proj;

namespace {

// ---------------------------------------------------------------------------------------------
// The search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:678-836), SURVEY 8f row f2:
// thread per map point -- projection (SPEC DECISION S8 arithmetic, as frustum_kernel), KeyFrame::IsInImage,
// PredictScale, KeyFrame::GetFeaturesInArea through the per-level cell-range tables, the chi-square gate
// (:794-817) and the nearest descriptor under (distance, visit position) == the reference's strict "<" scan.
// ---------------------------------------------------------------------------------------------
// Candidate sink of the walk below (orbfe_fuse_search_keyframes): the visit positions (ranks) of the features that passed every
// gate, kept sorted -- the walk visits level lvl-1 before lvl, the reference's strict "<" sees them in rank order.  The slots are
// registers: the insertion is a fixed chain of compare-selects, never an array indexed at run time.
constexpr int kFuseCandMax = 16;
struct CandSink {
    uint32_t r[kFuseCandMax];
    int count;
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < kFuseCandMax; j++) r[j] = kKey32None;
        count = 0;
    }
    __device__ __forceinline__ void push(uint32_t rank)
    {
        count++;
#pragma unroll
        for (int j = 0; j < kFuseCandMax; j++) {  // the kFuseCandMax smallest ranks survive, ascending
            const uint32_t lo = min(r[j], rank);
            rank = max(r[j], rank);
            r[j] = lo;
        }
    }
};

// The per-point walk of ORBmatcher::Fuse(pKF, vpMapPoints, th) (:706-832) for ONE map point: shared by fuse_search_kernel
// (one target per launch) and fuse_neighbors_kernel (a table of targets).  src = the point's row of mpDesc.  CANDS: every
// feature that passes the gates also goes to `sink`.
template <bool GATHER, bool CANDS>
__device__ __forceinline__ void fuse_walk(const ProjArgs& A, const orbfe_frustum& F, float th, bool skipped,
                                          const orbfe_world_point& p, const uint8_t* __restrict__ mpDesc, int src,
                                          const float* __restrict__ invLevelSigma2, const float* __restrict__ uRight, int chi2Gate,
                                          const unsigned long long* __restrict__ rightDesc, int nRight, int& bestIdx, int& bestDist,
                                          CandSink& sink)
{
    bestIdx = -1;
    bestDist = 256;
    do {
        if (skipped || (!GATHER && p.skip) || p.bad) break;  // :706-721 (a resident entry's own skip member is per frame: ignored)
        const float X = p.x, Y = p.y, Z = p.z;
        float pcx, pcy, pcz;
        rigid_transform(F.rcw, F.tcw, X, Y, Z, pcx, pcy, pcz);
        if (pcz < 0.0f) break;  // :725
        const float invz = 1.0f / pcz;
        float u, v;
        camera_project(F, pcx, pcy, pcz, u, v);
        if (!(u >= F.min_x && u < F.max_x && v >= F.min_y && v < F.max_y)) break;  // KeyFrame::IsInImage
        const float ur = u - F.mbf * invz;
        const float maxD = 1.1f * p.max_distance, minD = 0.9f * p.min_distance;
        const float ox = X - F.twc[0], oy = Y - F.twc[1], oz = Z - F.twc[2];
        const float dist3D = sqrtf((ox * ox + oy * oy) + oz * oz);
        if (dist3D < minD || dist3D > maxD) break;  // :748
        const int lvl = predict_scale(p.max_distance, dist3D, F.log_scale_factor, F.n_levels);
        MpWindow w;
        w.valid = true;
        w.x = u;
        w.y = v;
        w.r = th * A.scaleFactors[lvl];  // :766
        window_cells(A.g, w);
        if (!w.valid) break;
        const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(mpDesc + (size_t)src * 32);
        const unsigned long long d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
        // 1 / sigma^2 of the two levels the walk visits (:787), read once
        const float invS2Lo = chi2Gate ? invLevelSigma2[max(lvl - 1, 0)] : 0.0f, invS2Hi = chi2Gate ? invLevelSigma2[lvl] : 0.0f;
        uint32_t best = kKey32None;
        window_walk(A, w, lvl, [&](int l, int sl, const int4& rq) {
            const float invS2 = l == lvl ? invS2Hi : invS2Lo;
            const float ex = u - __int_as_float(rq.z), ey = v - __int_as_float(rq.w);
            float kur = -1.0f;
            if (uRight) kur = uRight[A.order[rq.x]];
            if (!chi2Gate) {
                // the Sim3 overload (:864-975) has no reprojection gate
            } else if (kur >= 0) {  // :792-805
                const float er = ur - kur;
                const float e2 = (ex * ex + ey * ey) + er * er;
                if ((double)(e2 * invS2) > 7.8) return;
            } else {
                const float e2 = ex * ex + ey * ey;
                if ((double)(e2 * invS2) > 5.99) return;
            }
            if (CANDS) sink.push((uint32_t)rq.x);  // passed every gate of :787-820
            const unsigned long long* kd = A.descS + (size_t)sl * 4;
            if (rightDesc) {  // bRight (:820): the left feature passed the gates, its right twin's row is compared
                const int idx = A.order[rq.x];
                if (idx >= nRight) return;
                kd = rightDesc + (size_t)idx * 4;
            }
            best = min(best, make_key32(hamming256(kd, d0, d1, d2, d3), rq.x));
        });
        if (best != kKey32None) {
            bestIdx = A.order[best & kRankMask] + (rightDesc ? A.kpStride : 0);
            bestDist = (int)(best >> kRankBits);
        }
    } while (false);
}

// GATHER: the map points are entries ids[i] of a resident map of mapCap entries (orbfe_map): id >= 0 the entry, ~id (negative)
// the entry with this call's skip flag set, outside the map no point -- pts / mpDesc are then the map's arrays.
template <bool GATHER>
__global__ __launch_bounds__(256) void fuse_search_kernel(ProjArgs A, orbfe_frustum F, float th, int M,
                                                          const int* __restrict__ ids, int mapCap,
                                                          const orbfe_world_point* __restrict__ pts,
                                                          const uint8_t* __restrict__ mpDesc,
                                                          const float* __restrict__ invLevelSigma2,
                                                          const float* __restrict__ uRight, int chi2Gate,
                                                          const unsigned long long* __restrict__ rightDesc, int nRight,
                                                          int* __restrict__ bestIdxOut, int* __restrict__ bestDistOut)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (one wave per block for a single call: see fuse_search_run)
    if (i >= M) return;
    int src = i;
    bool skipped = false;
    if (GATHER) {
        const int id = ids[i];
        src = id < 0 ? ~id : id;
        skipped = id < 0 || src >= mapCap;
        if (src >= mapCap) src = 0;
    }
    const orbfe_world_point p = pts[src];
    int bestIdx, bestDist;
    CandSink none;
    fuse_walk<GATHER, false>(A, F, th, skipped, p, mpDesc, src, invLevelSigma2, uRight, chi2Gate, rightDesc, nRight, bestIdx, bestDist,
                             none);
    bestIdxOut[i] = bestIdx;
    bestDistOut[i] = bestDist;
}

// ---------------------------------------------------------------------------------------------
// orbfe_fuse_search_keyframes: the Fuse searches of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:819-824) into all K
// targets in ONE launch.  Grid (ceil(M / 64), K), one wave per block: the target is wave-uniform, its record comes out of a
// K-entry table in device memory through uniform addresses.  Per pair the walk is fuse_walk -- the single call's -- with the
// candidate sink: besides (bestIdx, bestDist) under the descriptor the map holds NOW, the features that passed every gate in
// visit order, so that the caller can redo the strict "<" scan on the host when a Replace changed the point's descriptor.
// ---------------------------------------------------------------------------------------------
struct FuseTarget {
    ProjArgs A;
    orbfe_frustum F;
    const float* invLevelSigma2;
    const float* uRight;
    int n;  // features of the target: 0 = no tables were built, nothing qualifies
};

template <bool CANDS>
__global__ __launch_bounds__(64) void fuse_neighbors_kernel(const FuseTarget* __restrict__ tab, float th, int M,
                                                            const int* __restrict__ ids, const uint8_t* __restrict__ skip,
                                                            int mapCap, const orbfe_world_point* __restrict__ pts,
                                                            const uint8_t* __restrict__ mpDesc, int* __restrict__ bestIdxOut,
                                                            int* __restrict__ bestDistOut, int candCap, int* __restrict__ candIdxOut,
                                                            int* __restrict__ candCountOut)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M) return;
    const int k = blockIdx.y;
    const size_t row = (size_t)k * M + i;
    const FuseTarget& T = tab[k];
    int id = ids[i];
    if (skip && skip[row]) id = id < 0 ? id : ~id;
    const int src = id < 0 ? ~id : id;
    int bestIdx = -1, bestDist = 256;
    CandSink sink;
    if (CANDS) sink.clear();
    if (id >= 0 && src < mapCap && T.n > 0) {  // skipped lanes leave at once
        const orbfe_world_point p = pts[src];
        fuse_walk<true, CANDS>(T.A, T.F, th, false, p, mpDesc, src, T.invLevelSigma2, T.uRight, 1, nullptr, -1, bestIdx, bestDist, sink);
    }
    bestIdxOut[row] = bestIdx;
    bestDistOut[row] = bestDist;
    if (CANDS) {
        candCountOut[row] = sink.count;
        int* out = candIdxOut + row * (size_t)candCap;
#pragma unroll
        for (int j = 0; j < kFuseCandMax; j++)
            if (j < candCap) out[j] = sink.r[j] != kKey32None ? T.A.order[sink.r[j]] : -1;
    }
}

// ---------------------------------------------------------------------------------------------
// One direction of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1017-1092, :1094-1170): thread per map point of
// the source key frame -- source pose, similarity, the pinhole expression the function writes out itself
// (:1038-1043), KeyFrame::IsInImage, PredictScale, KeyFrame::GetFeaturesInArea on the target key frame's tables
// (A), nearest descriptor on levels [l-1, l] under (distance, visit position), bestDist <= TH_HIGH.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sim3_search_kernel(ProjArgs A, orbfe_sim3_view D, float th, int n,
                                                          const orbfe_world_point* __restrict__ pts,
                                                          const uint8_t* __restrict__ mpDesc, int* __restrict__ vnMatch)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const orbfe_world_point p = pts[i];
    int bestIdx = -1;
    do {
        if (p.skip || p.bad) break;  // :1021-1025
        float ax, ay, az, bx, by, bz;
        rigid_transform(D.rcw, D.tcw, p.x, p.y, p.z, ax, ay, az);  // source pose, then the similarity
        rigid_transform(D.sr, D.t, ax, ay, az, bx, by, bz);
        if (bz < 0.0f) break;  // :1032
        const float invz = 1.0f / bz;
        const float x = bx * invz, y = by * invz;
        const float u = D.fx * x + D.cx, v = D.fy * y + D.cy;
        if (!(u >= D.min_x && u < D.max_x && v >= D.min_y && v < D.max_y)) break;  // KeyFrame::IsInImage
        const float maxD = 1.1f * p.max_distance, minD = 0.9f * p.min_distance;
        const float dist3D = sqrtf((bx * bx + by * by) + bz * bz);
        if (dist3D < minD || dist3D > maxD) break;  // :1052
        const int lvl = predict_scale(p.max_distance, dist3D, D.log_scale_factor, D.n_levels);
        MpWindow w;
        w.valid = true;
        w.x = u;
        w.y = v;
        w.r = th * A.scaleFactors[lvl];  // :1060
        window_cells(A.g, w);
        if (!w.valid) break;
        const unsigned long long* dp = reinterpret_cast<const unsigned long long*>(mpDesc + (size_t)i * 32);
        const unsigned long long d0 = dp[0], d1 = dp[1], d2 = dp[2], d3 = dp[3];
        uint32_t best = kKey32None;
        window_walk(A, w, lvl, [&](int, int sl, const int4& rq) {
            best = min(best, make_key32(hamming256(A.descS + (size_t)sl * 4, d0, d1, d2, d3), rq.x));
        });
        if (best != kKey32None && (int)(best >> kRankBits) <= ORBFE_TH_HIGH) bestIdx = A.order[best & kRankMask];  // :1088
    } while (false);
    vnMatch[i] = bestIdx;
}

// agreement check of SearchBySim3 (:1172-1189): match12[i1] = idx2 iff vnMatch2[vnMatch1[i1]] == i1
__global__ __launch_bounds__(256) void sim3_agree_kernel(int n1, const int* __restrict__ vn1, const int* __restrict__ vn2,
                                                         int* __restrict__ match12, int* __restrict__ nFound)
{
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    int hit = 0;
    if (i1 < n1) {
        const int idx2 = vn1[i1];
        int m = -1;
        if (idx2 >= 0 && vn2[idx2] == i1) {
            m = idx2;
            hit = 1;
        }
        match12[i1] = m;
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(nFound, __popcll(b));
}

// ---------------------------------------------------------------------------------------------
// Relocalisation overload SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, checkOrientation)
// (src/ORBmatcher.cc:1202-1326).  reloc_project_kernel is the per-map-point head (:1225-1253) and writes the
// matcher's input records; the greedy "first free best" scan is the projection pipeline in kModeReloc (every
// accepted point blocks its keypoint: observations = 1); reloc_finalize_kernel is the rotation histogram.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reloc_project_kernel(orbfe_frustum F, int M, const orbfe_world_point* __restrict__ pts,
                                                            orbfe_map_point* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const orbfe_world_point p = pts[i];
    orbfe_map_point o;
    o.proj_x = -1.0f;
    o.proj_y = -1.0f;
    o.view_cos = 1.0f;
    o.track_depth = 0.0f;
    o.level = 0;
    o.in_view = 0;
    o.bad = 0;
    o.observations = 1;  // any accepted map point occupies its keypoint (:1268 tests the pointer only)
    do {
        if (p.skip || p.bad) break;  // :1221-1225
        const float X = p.x, Y = p.y, Z = p.z;
        float pcx, pcy, pcz;
        rigid_transform(F.rcw, F.tcw, X, Y, Z, pcx, pcy, pcz);
        float u, v;
        camera_project(F, pcx, pcy, pcz, u, v);  // no depth test in this overload
        if (u < F.min_x || u > F.max_x) break;   // :1232-1235
        if (v < F.min_y || v > F.max_y) break;
        if (u != u || v != v) break;  // NaN passes the tests above; the reference's grid query is then empty
        const float ox = X - F.twc[0], oy = Y - F.twc[1], oz = Z - F.twc[2];
        const float dist3D = sqrtf((ox * ox + oy * oy) + oz * oz);
        const float maxD = 1.1f * p.max_distance, minD = 0.9f * p.min_distance;
        if (dist3D < minD || dist3D > maxD) break;  // :1245
        o.level = predict_scale(p.max_distance, dist3D, F.log_scale_factor, F.n_levels);
        o.proj_x = u;
        o.proj_y = v;
        o.in_view = 1;
    } while (false);
    out[i] = o;
}

// rotation filter over the claimed keypoints (match_common.h); single block
__global__ __launch_bounds__(256) void reloc_finalize_kernel(int n, const orbfe_keypoint* __restrict__ kp,
                                                             const float* __restrict__ kfAngle, int checkOrientation,
                                                             int* __restrict__ matchOut, int* __restrict__ nMatches)
{
    rotation_filter_block(
        n, checkOrientation, [&](int j) { return matchOut[j] >= 0; },
        [&](int j) { return rotation_bin(kfAngle[matchOut[j]], kp[j].angle); }, [&](int j) { matchOut[j] = -1; }, nMatches);
}

}  // namespace

int fuse_search_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* KF, const float* invLevelSigma2,
                    const float* uRight, const orbfe_frustum* F, float th, int M, const orbfe_world_point* pts,
                    const uint8_t* mpDesc, int chi2Gate, int nRight, int* bestIdxOut, int* bestDistOut, std::string& err)
{
    if (!chi2Gate) {
        invLevelSigma2 = nullptr;
        uRight = nullptr;
    }
    for (int i = 0; i < M; i++) {
        bestIdxOut[i] = -1;
        bestDistOut[i] = 256;
    }
    const int n = KF->n;
    if (n == 0 || M == 0) return ORBFE_OK;
    if (n >= (1 << 20) || KF->grid_cols > 65535 || KF->grid_rows > 32767 || KF->n_levels < 1 ||
        (long long)KF->grid_cols * KF->grid_rows > kMaxCells)
        return ORBFE_ERR_UNSUPPORTED;
    if (F->n_levels > KF->n_levels) return ORBFE_ERR_INVALID_ARG;  // predicted levels index the key frame's scale tables
    Staging st;
    const auto bKp = st.in<orbfe_keypoint>(n);
    const auto bDesc = st.in<uint8_t>((size_t)n * 32);
    const auto bPts = st.in<orbfe_world_point>(M);
    const auto bMpDesc = st.in<uint8_t>((size_t)M * 32);
    const auto bSf = st.in<float>(KF->n_levels);
    const auto bIs2 = st.in<float>(KF->n_levels);
    const auto bUr = st.in<float>(n);
    const auto bN = st.in<int>(1);
    const auto bRight = st.in<unsigned long long>((size_t)(nRight > 0 ? nRight : 0) * 4);  // rows NLeft .. of mDescriptors (bRight)
    const auto bMatch = st.scratch<int>(n);  // the grid kernel clears a match array
    const auto bBest = st.out<int>((size_t)M * 2);  // [bestIdx | bestDist]
    ProjArgs A{};
    A.B = 1; A.M = 1; A.kpStride = n;
    A.g = GridDesc{KF->grid_cols, KF->grid_rows, KF->min_x, KF->min_y, KF->grid_inv_w, KF->grid_inv_h};
    A.nnRatio = 1.0f;
    A.nLevels = KF->n_levels;
    const ProjTables T = proj_tables(st, A);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    proj_bind(st, T, A);
    st.put(bKp, KF->kp);
    st.put(bDesc, KF->desc);
    st.put(bPts, pts);
    st.put(bMpDesc, mpDesc);
    st.put(bSf, KF->scale_factors);
    st.put(bIs2, invLevelSigma2);
    st.put(bUr, uRight);
    st.put(bN, &n);
    st.put(bRight, KF->desc + (size_t)n * 32);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    A.kp = st.dev(bKp);
    A.desc = st.dev(bDesc);
    A.nKp = st.dev(bN);
    A.scaleFactors = st.dev(bSf);
    A.matchOut = st.dev(bMatch);
    proj_prepare_launch(s, A, false);
    int* dBest = st.dev(bBest);
    hipLaunchKernelGGL(fuse_search_kernel<false>, dim3((M + 63) / 64), dim3(64), 0, s, A, *F, th, M, nullptr, 0, st.dev(bPts),
                       st.dev(bMpDesc), st.dev(bIs2), uRight ? st.dev(bUr) : nullptr, chi2Gate, nRight >= 0 ? st.dev(bRight) : nullptr, nRight,
                       dBest, dBest + M);
    if ((rc = download_span(st, s, bBest.off, bBest.end(), err)) != ORBFE_OK) return rc;
    st.get(bBest, bestIdxOut, M);
    memcpy(bestDistOut, st.res(bBest) + M, (size_t)M * sizeof(int));
    return ORBFE_OK;
}

int keyframe_set_grid(KeyFrameDev* K, hipStream_t s, int gridCols, int gridRows, float minX, float minY, float invW, float invH,
                      const float* invLevelSigma2, const float* uRight, std::string& err)
{
    if (!K || !invLevelSigma2 || gridCols < 1 || gridRows < 1) return ORBFE_ERR_INVALID_ARG;
    const int n = K->n;
    if (n >= (1 << 20) || gridCols > 65535 || gridRows > 32767 || (long long)gridCols * gridRows > kMaxCells) return ORBFE_ERR_UNSUPPORTED;
    K->hasGrid = false;
    Carver in;
    const size_t oN = in.take(sizeof(int));
    const size_t oIs2 = in.take((size_t)K->nLevels * sizeof(float));
    const size_t oUr = in.take((size_t)std::max(n, 1) * sizeof(float));
    const size_t inBytes = in.off;
    const size_t oMatch = in.take((size_t)std::max(n, 1) * sizeof(int));  // the grid kernel clears a match array
    ProjArgs A{};
    A.B = 1; A.M = 1; A.kpStride = std::max(n, 1);
    A.g = GridDesc{gridCols, gridRows, minX, minY, invW, invH};
    A.nnRatio = 1.0f;
    A.nLevels = K->nLevels;
    int rc = proj_setup(K->gridMem, A, in, inBytes, err);
    if (rc != ORBFE_OK) return rc;
    uint8_t* hp = static_cast<uint8_t*>(K->gridMem.hpin);
    uint8_t* dp = static_cast<uint8_t*>(K->gridMem.d);
    memcpy(hp + oN, &n, sizeof(int));
    memcpy(hp + oIs2, invLevelSigma2, (size_t)K->nLevels * sizeof(float));
    if (uRight && n) memcpy(hp + oUr, uRight, (size_t)n * sizeof(float));
    MCHK(hipMemcpyAsync(dp, hp, inBytes, hipMemcpyHostToDevice, s));
    A.kp = K->kp;
    A.desc = K->desc;
    A.nKp = reinterpret_cast<const int*>(dp + oN);
    A.scaleFactors = K->sf;
    A.matchOut = reinterpret_cast<int*>(dp + oMatch);
    if (n) proj_prepare_launch(s, A, false);
    MCHK(hipGetLastError());
    MCHK(hipStreamSynchronize(s));
    (void)hipHostFree(K->gridMem.hpin);  // the staging block has done its work; the device arena stays with the key frame
    K->gridMem.hpin = nullptr;
    K->gridMem.hBytes = 0;
    K->grid = A;
    K->invLevelSigma2 = reinterpret_cast<const float*>(dp + oIs2);
    K->uRight = uRight ? reinterpret_cast<const float*>(dp + oUr) : nullptr;
    K->hasGrid = true;
    return ORBFE_OK;
}

int fuse_search_keyframe_run(MatchScratch& m, hipStream_t s, const KeyFrameDev* K, int mapCap, const orbfe_world_point* mapPts,
                             const uint8_t* mapDesc, int M, const int* ids, const orbfe_frustum* F, float th, int* bestIdxOut,
                             int* bestDistOut, std::string& err)
{
    for (int i = 0; i < M; i++) {
        bestIdxOut[i] = -1;
        bestDistOut[i] = 256;
    }
    if (!K->hasGrid) {
        err = "orbfe_fuse_search_keyframe: the key frame has no grid (orbfe_keyframe_set_grid)";
        return ORBFE_ERR_INVALID_ARG;
    }
    if (K->n == 0 || M == 0) return ORBFE_OK;
    if (F->n_levels > K->nLevels) return ORBFE_ERR_INVALID_ARG;  // predicted levels index the key frame's scale tables
    Staging st;
    const auto bIds = st.in<int>(M);
    const auto bBest = st.out<int>((size_t)M * 2);  // [bestIdx | bestDist]
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    st.put(bIds, ids);
    if ((rc = upload_span(st, s, bIds.off, bIds.end(), err)) != ORBFE_OK) return rc;
    int* dBest = st.dev(bBest);
    hipLaunchKernelGGL(fuse_search_kernel<true>, dim3((M + 63) / 64), dim3(64), 0, s, K->grid, *F, th, M, st.dev(bIds), mapCap, mapPts,
                       mapDesc, K->invLevelSigma2, K->uRight, 1, static_cast<const unsigned long long*>(nullptr), -1, dBest, dBest + M);
    if ((rc = download_span(st, s, bBest.off, bBest.end(), err)) != ORBFE_OK) return rc;
    st.get(bBest, bestIdxOut, M);
    memcpy(bestDistOut, st.res(bBest) + M, (size_t)M * sizeof(int));
    return ORBFE_OK;
}

int fuse_search_keyframes_run(MatchScratch& m, hipStream_t s, int K, const KeyFrameDev* const* kfs, const orbfe_frustum* frusta,
                              int mapCap, const orbfe_world_point* mapPts, const uint8_t* mapDesc, int M, const int* ids,
                              const uint8_t* skip, float th, int* bestIdxOut, int* bestDistOut, int candCap, int* candIdxOut,
                              int* candCountOut, std::string& err)
{
    const size_t KM = (size_t)K * M;
    Staging st;
    const auto bTab = st.in<FuseTarget>(K);
    const auto bIds = st.in<int>(M);
    const auto bSkip = st.in<uint8_t>(skip ? KM : 0);
    const auto bOut = st.out<int>(KM * (size_t)(candCap > 0 ? 3 + candCap : 2));  // [bestIdx | bestDist | candCount | candIdx]
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    FuseTarget* hTab = st.host(bTab);
    for (int k = 0; k < K; k++) {
        hTab[k].A = kfs[k]->grid;
        hTab[k].F = frusta[k];
        hTab[k].invLevelSigma2 = kfs[k]->invLevelSigma2;
        hTab[k].uRight = kfs[k]->uRight;
        hTab[k].n = kfs[k]->n;
    }
    st.put(bIds, ids);
    st.put(bSkip, skip);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;  // table, ids and skip flags in one copy
    int* dOut = st.dev(bOut);
    const FuseTarget* dTab = st.dev(bTab);
    const int* dIds = st.dev(bIds);
    const uint8_t* dSkip = skip ? st.dev(bSkip) : nullptr;
    const dim3 grid((M + 63) / 64, K);
    if (candCap > 0)
        hipLaunchKernelGGL(fuse_neighbors_kernel<true>, grid, dim3(64), 0, s, dTab, th, M, dIds, dSkip, mapCap, mapPts, mapDesc, dOut,
                           dOut + KM, candCap, dOut + 3 * KM, dOut + 2 * KM);
    else
        hipLaunchKernelGGL(fuse_neighbors_kernel<false>, grid, dim3(64), 0, s, dTab, th, M, dIds, dSkip, mapCap, mapPts, mapDesc, dOut,
                           dOut + KM, 0, static_cast<int*>(nullptr), static_cast<int*>(nullptr));
    if ((rc = download_span(st, s, bOut.off, bOut.end(), err)) != ORBFE_OK) return rc;
    const int* hOut = st.res(bOut);
    memcpy(bestIdxOut, hOut, KM * sizeof(int));
    memcpy(bestDistOut, hOut + KM, KM * sizeof(int));
    if (candCap > 0) {
        memcpy(candCountOut, hOut + 2 * KM, KM * sizeof(int));
        memcpy(candIdxOut, hOut + 3 * KM, KM * (size_t)candCap * sizeof(int));
    }
    return ORBFE_OK;
}

// src/ORBmatcher.cc:824-832 for one pair on the host: the strict "<" over the candidate list, which is in visit order
int fuse_select_host(const int* candIdx, int candCount, int candCap, const uint8_t* kfDesc, int nKf, const uint8_t* mpDesc,
                     int* bestIdx, int* bestDist)
{
    *bestIdx = -1;
    *bestDist = 256;
    if (candCount > candCap) return ORBFE_ERR_UNSUPPORTED;
    unsigned long long d[4];
    memcpy(d, mpDesc, 32);
    for (int j = 0; j < candCount; j++) {
        const int idx = candIdx[j];
        if (idx < 0 || idx >= nKf) return ORBFE_ERR_INVALID_ARG;
        unsigned long long q[4];
        memcpy(q, kfDesc + (size_t)idx * 32, 32);
        const int dist = __builtin_popcountll(q[0] ^ d[0]) + __builtin_popcountll(q[1] ^ d[1]) + __builtin_popcountll(q[2] ^ d[2]) +
                         __builtin_popcountll(q[3] ^ d[3]);
        if (dist < *bestDist) {
            *bestDist = dist;
            *bestIdx = idx;
        }
    }
    return ORBFE_OK;
}

namespace {

int view_unsupported(const orbfe_frame_view* V)
{
    return V->n >= (1 << 20) || V->grid_cols > 65535 || V->grid_rows > 32767 || V->n_levels < 1 ||
           (long long)V->grid_cols * V->grid_rows > kMaxCells;
}

// one key frame's inputs for the thread-per-point searches, and the match array the grid kernel clears
struct ViewBlocks { Block<orbfe_keypoint> kp; Block<uint8_t> desc; Block<float> sf; Block<int> n, match; };

ViewBlocks view_in(Staging& st, const orbfe_frame_view* V)
{
    ViewBlocks b;
    b.kp = st.in<orbfe_keypoint>(V->n);
    b.desc = st.in<uint8_t>((size_t)V->n * 32);
    b.sf = st.in<float>(V->n_levels);
    b.n = st.in<int>(1);
    return b;
}

void view_fill(const Staging& st, const ViewBlocks& b, const orbfe_frame_view* V)
{
    st.put(b.kp, V->kp);
    st.put(b.desc, V->desc);
    st.put(b.sf, V->scale_factors);
    st.put(b.n, &V->n);
}

void view_bind(ProjArgs& A, const Staging& st, const ViewBlocks& b)
{
    A.kp = st.dev(b.kp);
    A.desc = st.dev(b.desc);
    A.nKp = st.dev(b.n);
    A.scaleFactors = st.dev(b.sf);
    A.matchOut = st.dev(b.match);
}

ProjArgs view_args(const orbfe_frame_view* V)
{
    ProjArgs A{};
    A.B = 1; A.M = 1; A.kpStride = V->n;
    A.g = GridDesc{V->grid_cols, V->grid_rows, V->min_x, V->min_y, V->grid_inv_w, V->grid_inv_h};
    A.nnRatio = 1.0f;
    A.nLevels = V->n_levels;
    return A;
}

void view_prepare(hipStream_t s, const ProjArgs& A)
{
    proj_prepare_launch(s, A, false);
}

}  // namespace

int search_by_sim3_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* KF1, const orbfe_frame_view* KF2,
                       const orbfe_sim3_view* d12, const orbfe_sim3_view* d21, const orbfe_world_point* mp1,
                       const uint8_t* mpDesc1, const orbfe_world_point* mp2, const uint8_t* mpDesc2, float th,
                       int* match12Out, int* nFound, std::string& err)
{
    const int n1 = KF1->n, n2 = KF2->n;
    for (int i = 0; i < n1; i++) match12Out[i] = -1;
    *nFound = 0;
    if (n1 == 0 || n2 == 0) return ORBFE_OK;
    if (view_unsupported(KF1) || view_unsupported(KF2)) return ORBFE_ERR_UNSUPPORTED;
    // predicted levels index the target key frame's scale tables
    if (d12->n_levels > KF2->n_levels || d21->n_levels > KF1->n_levels || d12->n_levels < 1 || d21->n_levels < 1)
        return ORBFE_ERR_INVALID_ARG;
    Staging st;
    ViewBlocks v1 = view_in(st, KF1), v2 = view_in(st, KF2);
    const auto bP1 = st.in<orbfe_world_point>(n1);
    const auto bD1 = st.in<uint8_t>((size_t)n1 * 32);
    const auto bP2 = st.in<orbfe_world_point>(n2);
    const auto bD2 = st.in<uint8_t>((size_t)n2 * 32);
    v1.match = st.scratch<int>(n1);  // the grid kernels clear a match array each
    v2.match = st.scratch<int>(n2);
    const auto bVn1 = st.scratch<int>(n1);
    const auto bVn2 = st.scratch<int>(n2);
    const auto bOut = st.out<int>((size_t)n1 + 1);  // matches, then the count
    ProjArgs A1 = view_args(KF1), A2 = view_args(KF2);
    const ProjTables T1 = proj_tables(st, A1), T2 = proj_tables(st, A2);
    int rc = reserve(m, st, err);  // once, for both table sets
    if (rc != ORBFE_OK) return rc;
    proj_bind(st, T1, A1);
    proj_bind(st, T2, A2);
    view_fill(st, v1, KF1);
    view_fill(st, v2, KF2);
    st.put(bP1, mp1);
    st.put(bD1, mpDesc1);
    st.put(bP2, mp2);
    st.put(bD2, mpDesc2);
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    view_bind(A1, st, v1);
    view_bind(A2, st, v2);
    view_prepare(s, A1);
    view_prepare(s, A2);
    int *vn1 = st.dev(bVn1), *vn2 = st.dev(bVn2), *dOut = st.dev(bOut);
    // key frame 1's map points into key frame 2 (tables A2), then the other way round
    hipLaunchKernelGGL(sim3_search_kernel, dim3((n1 + 63) / 64), dim3(64), 0, s, A2, *d12, th, n1, st.dev(bP1), st.dev(bD1), vn1);
    hipLaunchKernelGGL(sim3_search_kernel, dim3((n2 + 63) / 64), dim3(64), 0, s, A1, *d21, th, n2, st.dev(bP2), st.dev(bD2), vn2);
    MCHK(hipMemsetAsync(dOut + n1, 0, sizeof(int), s));
    hipLaunchKernelGGL(sim3_agree_kernel, dim3((n1 + 255) / 256), dim3(256), 0, s, n1, vn1, vn2, dOut, dOut + n1);
    if ((rc = download_span(st, s, bOut.off, bOut.end(), err)) != ORBFE_OK) return rc;
    st.get(bOut, match12Out, n1);
    *nFound = st.res(bOut)[n1];
    return ORBFE_OK;
}

int match_projection_kf_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* F, const orbfe_frustum* Fr, int M,
                            const orbfe_world_point* pts, const uint8_t* mpDesc, const float* kfAngle,
                            const uint8_t* frameHasMP, float th, int checkOrientation, int* matchOut, int* nMatches,
                            std::string& err)
{
    const int n = F->n;
    for (int i = 0; i < n; i++) matchOut[i] = -1;
    *nMatches = 0;
    if (n == 0 || M == 0) return ORBFE_OK;
    if (view_unsupported(F)) return ORBFE_ERR_UNSUPPORTED;
    if (Fr->n_levels > F->n_levels || Fr->n_levels < 1) return ORBFE_ERR_INVALID_ARG;
    Staging st;
    ViewBlocks v = view_in(st, F);
    const auto bPts = st.in<orbfe_world_point>(M);
    const auto bMpDesc = st.in<uint8_t>((size_t)M * 32);
    const auto bAng = st.in<float>(M);
    const auto bObs = st.in<int>(n);
    v.match = st.out<int>((size_t)n + 1);  // matches, then the count
    const auto bMp = st.scratch<orbfe_map_point>(M);
    ProjArgs A = view_args(F);
    A.M = M;
    A.mode = kModeReloc;
    A.th = th;
    A.nnRatio = 3.0e38f;  // "best <= nnRatio * second" always holds: this overload has no ratio test
    const ProjTables T = proj_tables(st, A);
    int rc = reserve(m, st, err);
    if (rc != ORBFE_OK) return rc;
    proj_bind(st, T, A);
    view_fill(st, v, F);
    st.put(bPts, pts);
    st.put(bMpDesc, mpDesc);
    st.put(bAng, kfAngle);
    int* hObs = st.host(bObs);
    for (int i = 0; i < n; i++) hObs[i] = (frameHasMP && frameHasMP[i]) ? 1 : -1;  // :1268: an occupied slot is never a candidate
    if ((rc = upload(st, s, err)) != ORBFE_OK) return rc;
    view_bind(A, st, v);
    A.mps = st.dev(bMp);
    A.mpDesc = st.dev(bMpDesc);
    A.initObs = st.dev(bObs);
    A.nMatches = A.matchOut + n;
    hipLaunchKernelGGL(reloc_project_kernel, dim3((M + 255) / 256), dim3(256), 0, s, *Fr, M, st.dev(bPts), st.dev(bMp));
    rc = proj_launch(s, A, err);
    if (rc != ORBFE_OK) return rc;
    hipLaunchKernelGGL(reloc_finalize_kernel, dim3(1), dim3(256), 0, s, n, A.kp, st.dev(bAng), checkOrientation, A.matchOut, A.nMatches);
    if ((rc = download_span(st, s, v.match.off, v.match.end(), err)) != ORBFE_OK) return rc;
    st.get(v.match, matchOut, n);
    *nMatches = st.res(v.match)[n];
    return ORBFE_OK;
}

}  // namespace orbfe

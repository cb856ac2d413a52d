// kernels_track_inertial.hip -- Tracking::TrackLocalMap once the IMU is initialised (src/Tracking.cc:937-1035), for a batch of
// independent frames, as launches back to back on one stream:
//   imu_frame_kernel (S22)            PreintegrateIMU + PredictStateIMU, the inertial link
//   track_frustum_gather_kernel (S23) isInFrustum against the pose the prediction left in HBM; point rows and depths for the optimiser
//   the three matcher kernels         SearchByProjection
//   pose_imu_kernel (S19) or pose_prev_kernel (S20)
//   track_stats_kernel (S23)          the loop of :958-982 and the pose the frame is left with
// SPEC DECISION S23; tests/track_inertial_ref.py is the normative restatement of what is new here.  The stages
// keep their own texts and bytes: this file holds the statistics kernel and the order of the launches.
#include <algorithm>
#include <cstring>

#include "match_proj.h"
#include "imu_preint_math.h"

#pragma clang fp contract(off)

namespace orbfe {

namespace {

constexpr int kStatsThreads = 256;

struct TrackStatsArgs {
    const int* nKp;              // [B]
    int kpStride, M;
    const int* match;            // [B][kpStride]
    const uint8_t* outlier;      // [B][kpStride]
    const orbfe_map_point* mps;  // [B][M]
    const float* stateIn;        // [B][33]
    const float* stateOut;       // [B][21]
    int* accepted;               // [B]: read (frame kind) or written as 1 (key-frame kind)
    int fromFrame;
    int inlierThreshold;
    float Rcb[9], tcb[3];
    uint8_t* found;              // [B][M]
    int* matchesInliers;         // [B]
    int* tracked;                // [B]
    float* TcwOut;               // [B][12]
};

// One block per frame.  found[] is cleared, then every matched keypoint stores its verdict at its map point's slot (the matcher's
// claims are exact: a slot has at most one keypoint) and votes; the count is an integer sum, so its order does not matter.
__global__ __launch_bounds__(kStatsThreads) void track_stats_kernel(TrackStatsArgs G)
{
    __shared__ int waveCount[kStatsThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    uint8_t* __restrict__ found = G.found + (size_t)b * G.M;
    for (int i = tid; i < G.M; i += kStatsThreads) found[i] = 0;
    __syncthreads();
    int n = G.nKp[b];
    n = n < 0 ? 0 : (n > G.kpStride ? G.kpStride : n);
    const size_t base = (size_t)b * G.kpStride;
    const orbfe_map_point* __restrict__ mps = G.mps + (size_t)b * G.M;
    int count = 0;  // wave-uniform
    for (int i0 = 0; i0 < n; i0 += kStatsThreads) {
        const int i = i0 + tid;
        bool vote = false;
        if (i < n) {
            const int m = G.match[base + i];
            if (m >= 0 && m < G.M) {
                const bool in = G.outlier[base + i] == 0;
                found[m] = in ? 1 : 0;
                vote = in && mps[m].observations > 0;
            }
        }
        count += __popcll(__ballot(vote));
    }
    if ((tid & 63) == 0) waveCount[tid >> 6] = count;
    __syncthreads();
    if (tid != 0) return;
    int total = 0;
#pragma unroll
    for (int w = 0; w < kStatsThreads / 64; w++) total += waveCount[w];
    G.matchesInliers[b] = total;
    G.tracked[b] = total >= G.inlierThreshold ? 1 : 0;
    bool applied = true;
    if (G.fromFrame) applied = G.accepted[b] != 0;
    else G.accepted[b] = 1;
    float* __restrict__ T = G.TcwOut + (size_t)b * 12;
    if (applied) {
        const float* __restrict__ so = G.stateOut + (size_t)b * 21;
        float Rwb[9], twb[3], Rcb[9], Rcw[9], tcw[3];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            Rwb[k] = so[k];
            Rcb[k] = G.Rcb[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) twb[k] = so[9 + k];
        set_imu_pose(Rwb, twb, Rcb, G.tcb, Rcw, tcw);
#pragma unroll
        for (int k = 0; k < 9; k++) T[k] = Rcw[k];
#pragma unroll
        for (int k = 0; k < 3; k++) T[9 + k] = tcw[k];
    } else {  // the result is not applied (src/Optimizer.cc:4208): the frame keeps the predicted pose
        const float* __restrict__ si = G.stateIn + (size_t)b * 33;
#pragma unroll
        for (int k = 0; k < 12; k++) T[k] = si[k];
    }
}

constexpr char kTrackSizeErr[] =
    "orbfe_track_inertial_params / orbfe_track_inertial_io struct_size (outer or nested) does not match this library (rebuild the caller "
    "against include/orbfe.h)";

}  // namespace

// struct sizes, the branches that are not built and the ranges: no handle, no device
int track_inertial_check(const orbfe_track_inertial_params* P, std::string& err)
{
    if (P->struct_size != (int)sizeof(orbfe_track_inertial_params) || P->track.struct_size != (int)sizeof(orbfe_track_params)) {
        err = kTrackSizeErr;
        return ORBFE_ERR_INVALID_ARG;
    }
    int rc = imu_check(&P->noise, &P->predict, nullptr, nullptr, err);
    if (rc != ORBFE_OK) return rc;
    rc = P->predict.which == ORBFE_IMU_FROM_FRAME ? pose_prev_check(&P->pose_frame, nullptr, nullptr, nullptr, err)
                                                  : pose_imu_check(&P->pose_keyframe, nullptr, nullptr, err);
    if (rc != ORBFE_OK) return rc;
    rc = frustum_validate(&P->frustum);
    if (rc != ORBFE_OK) return rc;
    if (P->frustum.camera_model != ORBFE_CAMERA_PINHOLE) {
        err = "orbfe_track_inertial: only the mono pinhole chain is built (DESIGN.md S23)";
        return ORBFE_ERR_UNSUPPORTED;
    }
    if (P->track.grid_cols < 1 || P->track.grid_rows < 1) return ORBFE_ERR_INVALID_ARG;
    if (P->track.grid_cols > 65535 || P->track.grid_rows > 32767 || (long long)P->track.grid_cols * P->track.grid_rows > proj::kMaxCells)
        return ORBFE_ERR_UNSUPPORTED;
    return ORBFE_OK;
}

// The launches of one call.  The arena is laid out and grown HERE, before the first launch, so that none of the stages moves it:
//   [ sample offsets (S22) / edge lists (S19, S20): the two stages' own scratch at the arena's start, one after the other in stream
//     order | links | gathered descriptors | point rows | depths | the matcher's scratch ]
// *dLinksOut: where the links are (the host-pointer call downloads them).
int track_inertial_batch_device(MatchScratch& m, hipStream_t s, const orbfe_track_inertial_params* P, const float* dScaleFactors,
                                const float* invLevelSigma2, int nLevels, int batch, int kpStride, int mapCap,
                                const orbfe_world_point* mapPts, const uint8_t* mapDesc, int M, const orbfe_track_inertial_io* io,
                                void** dLinksOut, std::string& err)
{
    if (kpStride > kPoseMaxKp) return ORBFE_ERR_INVALID_ARG;
    const bool fromFrame = P->predict.which == ORBFE_IMU_FROM_FRAME;
    const size_t linkBytes = fromFrame ? sizeof(orbfe_imu_link_free) : sizeof(orbfe_imu_link);
    const size_t slots = (size_t)batch * std::max(M, 1);
    Carver c;
    c.take(std::max((size_t)(batch + 1) * sizeof(int), (size_t)batch * kpStride * sizeof(int)));
    const size_t oLinks = c.take((size_t)batch * linkBytes);
    const size_t oDesc = c.take(slots * ORBFE_DESC_BYTES);
    const size_t oRows = c.take(slots * sizeof(orbfe_world_point));
    const size_t oDepth = c.take(slots * sizeof(float));

    const orbfe_track_params& tp = P->track;
    proj::ProjArgs A{};
    A.B = batch; A.M = M; A.kpStride = kpStride;
    A.g = proj::GridDesc{tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y, tp.grid_inv_w, tp.grid_inv_h};
    A.th = tp.th; A.thFar = tp.th_far_points; A.nnRatio = tp.nn_ratio; A.farPoints = tp.far_points; A.bFactor = tp.th != 1.0;
    A.kp = io->d_kp; A.desc = io->d_desc; A.nKp = io->d_n; A.mps = io->d_mp_out; A.initObs = nullptr;
    A.scaleFactors = dScaleFactors; A.nLevels = nLevels;
    A.matchOut = io->d_match_out;
    A.nMatches = io->d_n_matches;
    int rc = proj::proj_setup(m, A, c, 64, err);
    if (rc != ORBFE_OK) return rc;
    uint8_t* dp = static_cast<uint8_t*>(m.d);
    void* dLinks = dp + oLinks;
    uint8_t* dDesc = dp + oDesc;
    orbfe_world_point* dRows = reinterpret_cast<orbfe_world_point*>(dp + oRows);
    float* dDepth = reinterpret_cast<float*>(dp + oDepth);
    A.mpDesc = dDesc;
    if (dLinksOut) *dLinksOut = dLinks;

    rc = imu_frame_batch_device(m, s, &P->noise, &P->predict, batch, io->d_samples, io->sample_off, io->d_t_prev, io->d_t_cur,
                                io->d_frame_bias, io->d_state1, io->d_kf, io->d_frame, io->d_steps_out, io->d_state_in, dLinks, io->d_info_ok,
                                err);
    if (rc != ORBFE_OK) return rc;
    rc = track_frustum_gather_launch(s, batch, &P->frustum, io->d_state_in, io->d_ids, M, mapCap, mapPts, mapDesc, io->d_mp_out, dDesc, dRows,
                                     dDepth, err);
    if (rc != ORBFE_OK) return rc;
    rc = proj::proj_launch(s, A, err);
    if (rc != ORBFE_OK) return rc;
    if (fromFrame)
        rc = pose_prev_batch_device(m, s, &P->pose_frame, invLevelSigma2, nLevels, batch, static_cast<const orbfe_imu_link_free*>(dLinks),
                                    io->d_priors, io->d_kp, io->d_n, kpStride, io->d_match_out, M, dRows, M, dDepth, io->d_state_in,
                                    io->d_state_out, io->d_H_out, io->d_Hprior_out, io->d_outlier, io->d_n_inliers, io->d_accepted, err);
    else
        rc = pose_imu_batch_device(m, s, &P->pose_keyframe, invLevelSigma2, nLevels, batch, static_cast<const orbfe_imu_link*>(dLinks),
                                   io->d_kp, io->d_n, kpStride, io->d_match_out, M, dRows, M, dDepth, io->d_state_in, io->d_state_out,
                                   io->d_H_out, io->d_outlier, io->d_n_inliers, err);
    if (rc != ORBFE_OK) return rc;

    TrackStatsArgs G;
    memset(&G, 0, sizeof G);
    G.nKp = io->d_n;
    G.kpStride = kpStride;
    G.M = M;
    G.match = io->d_match_out;
    G.outlier = io->d_outlier;
    G.mps = io->d_mp_out;
    G.stateIn = io->d_state_in;
    G.stateOut = io->d_state_out;
    G.accepted = io->d_accepted;
    G.fromFrame = fromFrame ? 1 : 0;
    G.inlierThreshold = P->inlier_threshold;
    memcpy(G.Rcb, P->predict.Rcb, sizeof G.Rcb);
    memcpy(G.tcb, P->predict.tcb, sizeof G.tcb);
    G.found = io->d_found;
    G.matchesInliers = io->d_matches_inliers;
    G.tracked = io->d_tracked;
    G.TcwOut = io->d_Tcw_out;
    hipLaunchKernelGGL(track_stats_kernel, dim3(batch), dim3(kStatsThreads), 0, s, G);
    MCHK(hipGetLastError());
    return ORBFE_OK;
}

}  // namespace orbfe

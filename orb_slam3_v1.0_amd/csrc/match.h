// match.h -- host entry points of the Hamming matchers (kernels_match.hip).
#pragma once
#include <string>
#include <vector>

#include "orbfe_internal.h"

namespace orbfe {

// device + pinned scratch reused across matcher calls (grown on demand, never shrunk)
struct MatchScratch {
    void* d = nullptr;      // device arena
    size_t dBytes = 0;
    void* hpin = nullptr;   // pinned host arena
    size_t hBytes = 0;
    hipEvent_t busy = nullptr;  // recorded behind the last launch that used the arenas (owned by the handle)
};

void match_scratch_free(MatchScratch& m);

constexpr int kPoseMaxKp = 65536;   // the pose kernels' bound on the keypoints (kp_stride) of one frame
constexpr int kImuStateIn = 33;     // what an inertial solver reads per frame: Rcw, tcw, Rwb, twb, v, bg, ba (it writes the last kImuState)

int match_projection_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* F, int M,
                         const orbfe_map_point* mps, const uint8_t* mpDesc, const int* initObs, float th,
                         int farPoints, float thFar, float nnRatio, int* matchOut, int* nMatches,
                         std::string& err);

int match_projection_batch_device(MatchScratch& m, hipStream_t s, int B, const orbfe_keypoint* dKp, const uint8_t* dDesc,
                                  const int* dN, int kpStride, int gridCols, int gridRows, float minX, float minY,
                                  float invW, float invH, const float* dScaleFactors, int nLevels, int M,
                                  const orbfe_map_point* dMps, const uint8_t* dMpDesc, const int* dInitObs, float th,
                                  int farPoints, float thFar, float nnRatio, int* dMatchOut, int* dNMatches,
                                  std::string& err);

int match_initialization_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* F1, const orbfe_frame_view* F2,
                             int windowSize, float nnRatio, int checkOrientation, int* matches12Out, int* nMatches,
                             std::string& err);

// the same matcher inside a captured per-frame chain (orbfe_track_initialization): frame 1 = a resident initial frame (n1
// keypoints, n0 of them on level 0, listed in index order in dList0), frame 2 = the fresh keypoints of the current frame on the
// device (count in *dN2, <= cap); `scratch` = init_track_scratch_bytes(n1, n0, cap) bytes of device memory
size_t init_track_scratch_bytes(int n1, int n0, int cap);
int init_track_launch(hipStream_t s, int n1, int n0, const orbfe_keypoint* dKp1, const uint8_t* dDesc1, const int* dList0,
                      const orbfe_keypoint* dKp2, const uint8_t* dDesc2, const int* dN2, int cap, int gridCols, int gridRows,
                      float minX, float minY, float invW, float invH, int windowSize, float nnRatio, int checkOrientation,
                      int* dMatches12, int* dNMatches, uint8_t* scratch, std::string& err);

int match_bow_run(MatchScratch& m, hipStream_t s, int G, const int* kfOff, const int* kfIdx, const int* fOff,
                  const int* fIdx, int nKF, const uint8_t* kfDesc, const float* kfAngle, const uint8_t* kfHasMP,
                  int nF, const uint8_t* fDesc, const float* fAngle, int nLeft, float nnRatio, int checkOrientation,
                  int* matchOut, int* nMatches, std::string& err);

// the search part of ORBmatcher::Fuse (kernels_match_kf.hip)
int fuse_search_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* KF, const float* invLevelSigma2,
                    const float* uRight, const orbfe_frustum* F, float th, int M, const orbfe_world_point* pts,
                    const uint8_t* mpDesc, int chi2Gate, int nRight, int* bestIdxOut, int* bestDistOut, std::string& err);
// ORBmatcher::SearchBySim3 and the relocalisation SearchByProjection overload (kernels_match_kf.hip)
int search_by_sim3_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* KF1, const orbfe_frame_view* KF2,
                       const orbfe_sim3_view* d12, const orbfe_sim3_view* d21, const orbfe_world_point* mp1,
                       const uint8_t* mpDesc1, const orbfe_world_point* mp2, const uint8_t* mpDesc2, float th,
                       int* match12Out, int* nFound, std::string& err);
int match_projection_kf_run(MatchScratch& m, hipStream_t s, const orbfe_frame_view* F, const orbfe_frustum* Fr, int M,
                            const orbfe_world_point* pts, const uint8_t* mpDesc, const float* kfAngle,
                            const uint8_t* frameHasMP, float th, int checkOrientation, int* matchOut, int* nMatches,
                            std::string& err);
// kernels_match_tri.hip
int match_triangulation_run(MatchScratch& m, hipStream_t s, int G, const int* off1, const int* idx1, const int* off2,
                            const int* idx2, int n1, const orbfe_keypoint* kp1, const uint8_t* desc1, const uint8_t* hasMP1,
                            const uint8_t* stereo1, int n2, const orbfe_keypoint* kp2, const uint8_t* desc2,
                            const uint8_t* hasMP2, const uint8_t* stereo2, const float* sf2, int nLevels2,
                            const orbfe_tri_params* P, int* matches12, int* nMatches, std::string& err);
// kernels_twoview.hip (TwoViewReconstruction::Reconstruct, SPEC DECISION S12)
int two_view_run(MatchScratch& m, hipStream_t s, const orbfe_two_view_params* P, int n1, const orbfe_keypoint* kp1, int n2,
                 const orbfe_keypoint* kp2, const int* matches12, const int* sets, int* reconstructed, float* R21, float* t21,
                 float* p3d, uint8_t* triangulated, orbfe_two_view_info* info, std::string& err);
// kernels_mlpnp.hip (MLPnPsolver: SetRansacParameters + one iterate, SPEC DECISION S13)
int mlpnp_plan(const orbfe_mlpnp_params* P, int N, int* minInliers, int* maxIts, int* total);
int mlpnp_run(MatchScratch& m, hipStream_t s, const orbfe_mlpnp_params* P, const float* levelSigma2, int nLevels, int n,
              const orbfe_keypoint* kp, const int* mpIndex, int nPoints, const float* points, const int* sets, int nSets, int* solved,
              float* Tcw, uint8_t* inliers, int* nInliers, int* noMore, orbfe_mlpnp_info* info, std::string& err);
// kernels_poseopt.hip (Optimizer::PoseOptimization, SPEC DECISION S14)
int pose_opt_check(const orbfe_pose_opt_params* P, const orbfe_pose_opt_info* info, std::string& err);
int pose_opt_begin(const orbfe_pose_opt_params* P, int nLevels, int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints,
                   const float* Rcw, const float* tcw, float* TcwOut, uint8_t* outlier, int* nInliers, orbfe_pose_opt_info* info,
                   std::vector<int>& first, std::string& err);
int pose_opt_run(MatchScratch& m, hipStream_t s, const orbfe_pose_opt_params* P, const float* invLevelSigma2, int nLevels, int n,
                 const orbfe_keypoint* kp, const int* mpIndex, const float* points, const float* Rcw, const float* tcw,
                 const std::vector<int>& first, float* TcwOut, uint8_t* outlier, int* nInliers, orbfe_pose_opt_info* info, std::string& err);
int pose_opt_batch_device(MatchScratch& m, hipStream_t s, const orbfe_pose_opt_params* P, const float* invLevelSigma2, int nLevels,
                          int batch, const orbfe_keypoint* dKp, const int* dN, int kpStride, const int* dMatch, int nMapPoints,
                          const orbfe_world_point* dPoints, int pointStrideFrames, const float* dPoseIn, float* dPoseOut,
                          uint8_t* dOutlier, int* dNInliers, std::string& err);
// kernels_poseimu.hip (Optimizer::PoseInertialOptimizationLastKeyFrame, SPEC DECISION S19)
int pose_imu_check(const orbfe_pose_inertial_params* P, const orbfe_imu_link* link, const orbfe_pose_inertial_info* info, std::string& err);
int pose_imu_begin(const orbfe_pose_inertial_params* P, const orbfe_imu_link* link, int nLevels, int n, const orbfe_keypoint* kp,
                   const int* mpIndex, int nPoints, orbfe_pose_inertial_info* info, std::vector<int>& first, std::string& err);
int pose_imu_run(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_params* P, const orbfe_imu_link* link,
                 const float* invLevelSigma2, int nLevels, int n, const orbfe_keypoint* kp, const int* mpIndex, const float* points,
                 const float* trackDepth, const float* stateIn, const std::vector<int>& first, float* stateOut, double* Hout,
                 uint8_t* outlier, int* nInliers, orbfe_pose_inertial_info* info, std::string& err);
int pose_imu_batch_device(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_params* P, const float* invLevelSigma2, int nLevels,
                          int batch, const orbfe_imu_link* dLinks, const orbfe_keypoint* dKp, const int* dN, int kpStride,
                          const int* dMatch, int nMapPoints, const orbfe_world_point* dPoints, int pointStrideFrames,
                          const float* dTrackDepth, const float* dStateIn, float* dStateOut, double* dHout, uint8_t* dOutlier,
                          int* dNInliers, std::string& err);
// kernels_poseimu_prev.hip (Optimizer::PoseInertialOptimizationLastFrame, SPEC DECISION S20)
int pose_prev_check(const orbfe_pose_inertial_prev_params* P, const orbfe_imu_link_free* link, const orbfe_pose_imu_prior* prior,
                    const orbfe_pose_inertial_prev_info* info, std::string& err);
int pose_prev_begin(const orbfe_pose_inertial_prev_params* P, const orbfe_imu_link_free* link, const orbfe_pose_imu_prior* prior, int nLevels,
                    int n, const orbfe_keypoint* kp, const int* mpIndex, int nPoints, orbfe_pose_inertial_prev_info* info,
                    std::vector<int>& first, std::string& err);
int pose_prev_run(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_prev_params* P, const orbfe_imu_link_free* link,
                  const orbfe_pose_imu_prior* prior, const float* invLevelSigma2, int nLevels, int n, const orbfe_keypoint* kp,
                  const int* mpIndex, const float* points, const float* trackDepth, const float* stateIn, const std::vector<int>& first,
                  float* stateOut, double* H30out, double* HpriorOut, uint8_t* outlier, int* nInliers, int* accepted,
                  orbfe_pose_inertial_prev_info* info, std::string& err);
int pose_prev_batch_device(MatchScratch& m, hipStream_t s, const orbfe_pose_inertial_prev_params* P, const float* invLevelSigma2,
                           int nLevels, int batch, const orbfe_imu_link_free* dLinks, const orbfe_pose_imu_prior* dPriors,
                           const orbfe_keypoint* dKp, const int* dN, int kpStride, const int* dMatch, int nMapPoints,
                           const orbfe_world_point* dPoints, int pointStrideFrames, const float* dTrackDepth, const float* dStateIn,
                           float* dStateOut, double* dH30, double* dHprior, uint8_t* dOutlier, int* dNInliers, int* dAccepted,
                           std::string& err);

// kernels_imu_preint.hip (IMU preintegration, state prediction and the inertial links, SPEC DECISION S22)
int imu_check(const orbfe_imu_noise* noise, const orbfe_imu_predict_params* P, const orbfe_imu_preint* a, const orbfe_imu_preint* b,
              std::string& err);
int imu_check_offsets(int batch, const int* off);
int imu_preintegrate_run(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, int n, const orbfe_imu_sample* samples, double tPrev,
                         double tCur, const float* frameBias, orbfe_imu_preint* kf, orbfe_imu_preint* frame, orbfe_imu_step* stepsOut,
                         int* nSteps, std::string& err);
int imu_reintegrate_run(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, const float* bias, int n, const orbfe_imu_step* steps,
                        orbfe_imu_preint* out, std::string& err);
int imu_predict_run(MatchScratch& m, hipStream_t s, const orbfe_imu_predict_params* P, const float* state1, const orbfe_imu_preint* kf,
                    const orbfe_imu_preint* frame, float* stateOut, void* linkOut, int* infoOk, std::string& err);
int imu_frame_batch_device(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, const orbfe_imu_predict_params* P, int batch,
                           const orbfe_imu_sample* dSamples, const int* sampleOff, const double* dTPrev, const double* dTCur,
                           const float* dFrameBias, const float* dState1, orbfe_imu_preint* dKf, orbfe_imu_preint* dFrame,
                           orbfe_imu_step* dStepsOut, float* dStateIn, void* dLinks, int* dInfoOk, std::string& err);
int imu_reintegrate_batch_device(MatchScratch& m, hipStream_t s, const orbfe_imu_noise* noise, int batch, const orbfe_imu_step* dSteps,
                                 const int* stepOff, const float* dBias, orbfe_imu_preint* dOut, std::string& err);

// kernels_initial_ba.hip (the bundle adjustment of the initial map, SPEC DECISION S17)
int initial_ba_check(const orbfe_initial_ba_params* P, const orbfe_initial_ba_info* info, std::string& err);
int initial_ba_begin(const orbfe_initial_ba_params* P, int nLevels, int n1, const orbfe_keypoint* kp1, int n2, const orbfe_keypoint* kp2,
                     const int* matches12, const float* points, const float* Rcw2, const float* tcw2, float* TcwOut, float* pointsOut,
                     orbfe_initial_ba_info* info, std::vector<int>& first, std::string& err);
int initial_ba_run_host(MatchScratch& m, hipStream_t s, const orbfe_initial_ba_params* P, const float* invLevelSigma2,
                        const orbfe_keypoint* kp1, const orbfe_keypoint* kp2, const int* matches12, const float* points, const float* Rcw1,
                        const float* tcw1, const float* Rcw2, const float* tcw2, const std::vector<int>& first, float* TcwOut,
                        float* pointsOut, orbfe_initial_ba_info* info, std::string& err);
// kernels_distinct.hip (MapPoint::ComputeDistinctiveDescriptors for a batch)
int distinctive_run(MatchScratch& m, hipStream_t s, int nSets, const int* setOff, const uint8_t* desc, int* bestIdx,
                    int* bestMedian, std::string& err);
// kernels_frustum.hip
int frustum_validate(const orbfe_frustum* F);
int frustum_launch(hipStream_t s, const orbfe_frustum* F, int n, const orbfe_world_point* dPts, orbfe_map_point* dOut,
                   float* dProjXR, std::string& err);
// the same with the frustum block resident in HBM (orbfe_track_frame: the launch is part of a captured hipGraph)
int frustum_launch_dev(hipStream_t s, const orbfe_frustum* dF, int n, const orbfe_world_point* dPts, orbfe_map_point* dOut,
                       float* dProjXR, std::string& err);

// resident map points (orbfe_map): gather by id + isInFrustum for B frames with their own frusta; scatter of updated entries
int frustum_gather_launch(hipStream_t s, int B, const orbfe_frustum* dF, const int* dIds, int M, int mapCap,
                          const orbfe_world_point* mapPts, const uint8_t* mapDesc, orbfe_map_point* dOut, uint8_t* dDescOut,
                          float* dProjXR, std::string& err);
// the same with the frustum of frame b built on the device from dStateIn[33 b ..) and the template *T, plus the point rows and depths
// the inertial pose optimisations read (SPEC DECISION S23); dDescOut / dRowOut 16-byte aligned
int track_frustum_gather_launch(hipStream_t s, int B, const orbfe_frustum* T, const float* dStateIn, const int* dIds, int M, int mapCap,
                                const orbfe_world_point* mapPts, const uint8_t* mapDesc, orbfe_map_point* dOut, uint8_t* dDescOut,
                                orbfe_world_point* dRowOut, float* dDepthOut, std::string& err);
// kernels_track_inertial.hip (Tracking::TrackLocalMap with the IMU for a batch of frames, SPEC DECISION S23)
int track_inertial_check(const orbfe_track_inertial_params* P, std::string& err);
int track_inertial_batch_device(MatchScratch& m, hipStream_t s, const orbfe_track_inertial_params* P, const float* dScaleFactors,
                                const float* invLevelSigma2, int nLevels, int batch, int kpStride, int mapCap,
                                const orbfe_world_point* mapPts, const uint8_t* mapDesc, int M, const orbfe_track_inertial_io* io,
                                void** dLinksOut, std::string& err);
int map_scatter_launch(hipStream_t s, int n, const int* dIds, const orbfe_world_point* dPts, const uint8_t* dDesc, int mapCap,
                       orbfe_world_point* mapPts, uint8_t* mapDesc, std::string& err);

}  // namespace orbfe

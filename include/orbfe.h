/*
 * orbfe.h -- C ABI of the MI355X-native ORB front-end (liborbfe.so).
 *
 * This is the drop-in boundary for ONE path of geoeo/ORB_SLAM3_V1.0: the per-frame ORB
 * extractor + Hamming matchers.  Each entry point names the reference interface it replaces
 * (paths relative to the reference repo).  Plain pointers and sizes only; no C++/torch types.
 * The reference-signature C++ wrapper lives in include/orbfe_adaptor.hpp; the binding a
 * maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Error behaviour: every function returns an orbfe_status (0 == ORBFE_OK); nothing in the
 * library calls exit()/abort() (the reference does: include/cuda/HelperCuda.h:44-50).
 * A frame with zero keypoints is NOT an error: n == 0 (the reference returns std::nullopt,
 * src/ORBextractor.cc:494-496); the adaptor maps it back to nullopt.
 *
 * Threading: one handle == one HIP stream == one caller at a time for the extract calls (same
 * as the reference).  The matcher calls take their own scratch from the
 * handle and are serialised per handle; use one handle per calling thread.
 *
 * Streams: the *_device entry points are asynchronous on the caller's stream but work in scratch the
 * handle owns (pyramid, candidate lists; the matcher arena).  The library orders consecutive users of
 * that scratch itself: it records an event behind every enqueue and makes the next enqueue on a
 * DIFFERENT stream wait for it, so mixing streams (or a *_device call followed by a host-pointer
 * call) is safe; it does not make two calls run concurrently.
 *
 * Input contract of the image entry points: rows `pitch` bytes apart, pitch < 2^24 and
 * pitch * (height - 1) + ((width + 3) & ~3) < 0x7ffffff0 (frames are addressed with 32-bit byte
 * offsets; larger ones are refused with ORBFE_ERR_INVALID_ARG); when the
 * base address, pitch and frame stride are multiples of 4 the kernels read whole dwords, i.e. up
 * to the 4-byte-rounded end of every row -- the buffer must extend to
 * pitch * (height - 1) + ((width + 3) & ~3) bytes per frame (any pitch >= that rounded width, or a
 * tight width that is a multiple of 4, satisfies it).
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_MAX_LEVELS 32
#define ORBFE_DESC_BYTES 32

typedef enum orbfe_status {
    ORBFE_OK = 0,
    ORBFE_ERR_INVALID_ARG = 1,   /* NULL pointer, size out of range, batch > max_batch ... */
    ORBFE_ERR_UNSUPPORTED = 2,   /* configuration outside what the kernels were built for */
    ORBFE_ERR_NO_DEVICE = 3,     /* no gfx950 device / HIP runtime failure at create */
    ORBFE_ERR_HIP = 4,           /* a HIP call failed; see orbfe_last_error() */
    ORBFE_ERR_OUT_OF_MEMORY = 5,
    ORBFE_ERR_INTERNAL = 6,      /* device-side guard tripped (capacity / round limit) */
    ORBFE_ERR_BUSY = 7           /* orbfe_stream_submit: every slot of the ring is in flight -- collect first */
} orbfe_status;

/* Layout-identical to ORB_SLAM3::KeyPoint (include/KeyPoint.h:7-12): 24 bytes, memcpy-able. */
typedef struct orbfe_keypoint {
    float x, y;     /* LEVEL pixel coordinates (the reference never rescales, S6) */
    int response;   /* FAST corner score (src/cuda/Fast_gpu.cu:193-216) */
    float size;     /* (int)(31 * invScaleFactor[octave]) (src/ORBextractor.cc:511,531) */
    int octave;
    float angle;    /* degrees in [0, 360] */
} orbfe_keypoint;

/* The 8 constructor arguments of ORBextractor::ORBextractor (include/ORBextractor.h:55-56,
 * src/ORBextractor.cc:82-149) plus placement / batching knobs that have no reference analogue. */
typedef struct orbfe_params {
    int n_features;        /* nFeatures      */
    int n_fast_features;   /* nFastFeatures  (per-level FAST candidate cap) */
    float scale_factor;    /* scaleFactor    */
    int n_levels;          /* nlevels        */
    int ini_th_fast;       /* iniThFAST      */
    int min_th_fast;       /* minThFAST      */
    int image_width;       /* imageWidth     */
    int image_height;      /* imageHeight    */
    int device_id;         /* HIP device ordinal (0 for one-process-per-GPU) */
    int max_batch;         /* frames per orbfe_extract_batch* call (>= 1); sizes the workspace */
} orbfe_params;

typedef struct orbfe_handle orbfe_handle;

/* -------------------------------------------------------------------------------------------
 * Extractor
 * ---------------------------------------------------------------------------------------- */

/* replaces ORBextractor::ORBextractor (src/ORBextractor.cc:82-149): scale tables, per-level
 * feature budget, pyramid + scratch allocation (AllocatePyramid :587-605, GpuFast::GpuFast
 * src/cuda/Fast_gpu.cu:321-332).  All device memory is allocated here, none per frame. */
int orbfe_create(const orbfe_params *params, orbfe_handle **out);
void orbfe_destroy(orbfe_handle *h);

/* replaces GetLevels / GetScaleFactor (include/ORBextractor.h:64-72) */
int orbfe_get_levels(const orbfe_handle *h);
float orbfe_get_scale_factor(const orbfe_handle *h);
/* replaces GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:74-92).  Each array holds n_levels floats;
 * any pointer may be NULL. */
int orbfe_get_scale_tables(const orbfe_handle *h, float *scale_factors, float *inv_scale_factors,
                           float *level_sigma2, float *inv_level_sigma2);
/* mnFeaturesPerLevel (src/ORBextractor.cc:112-124) and pyramid level sizes (:594-604) */
int orbfe_get_level_info(const orbfe_handle *h, int *features_per_level, int *level_width,
                         int *level_height);
/* upper bound on keypoints per frame: sum over levels of max(N_level + 3, 4 * nIni).  Output
 * arrays of the extract calls are sized with this stride. */
int orbfe_max_keypoints(const orbfe_handle *h);

/* replaces ORBextractor::extractFeatures(const cv::cuda::HostMem&) (include/ORBextractor.h:62,
 * src/ORBextractor.cc:543-585).  `gray` is a host pointer to an 8-bit image of the size given at
 * create, `pitch` bytes per row.  kp_out / desc_out hold orbfe_max_keypoints() entries; *n_out
 * receives the count (0 == the reference's nullopt); per_level_counts (n_levels ints) may be
 * NULL.  One H2D copy, one D2H copy, one host sync. */
int orbfe_extract(orbfe_handle *h, const uint8_t *gray, int pitch, orbfe_keypoint *kp_out,
                  uint8_t *desc_out, int *n_out, int *per_level_counts);

/* Batched many-frame mode (BASELINE config 4; no reference analogue).  Host pointers; frame b's
 * results start at kp_out + b*cap, desc_out + b*cap*32, per_level_counts + b*n_levels with
 * cap = orbfe_max_keypoints(). */
int orbfe_extract_batch(orbfe_handle *h, const uint8_t *const *grays, int pitch, int batch,
                        orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out,
                        int *per_level_counts);

/* Same, with everything already resident in HBM: d_gray points at `batch` frames
 * `frame_stride` bytes apart in device memory; all outputs are device pointers with the strides
 * above.  Asynchronous on `stream` (a hipStream_t; NULL == the handle's own stream); no host
 * sync is performed.  This is the entry bench.py times. */
int orbfe_extract_batch_device(orbfe_handle *h, const uint8_t *d_gray, size_t frame_stride,
                               int pitch, int batch, orbfe_keypoint *d_kp_out,
                               uint8_t *d_desc_out, int *d_n_out, int *d_per_level_counts,
                               void *stream);

/* Device-side guard flags of the LAST extract call (any entry point, any stream): waits for that
 * call, ORs the per-(frame, level) status words (candidate-array / node-table overflow, round
 * limit) into *flags_out (may be NULL) and returns ORBFE_ERR_INTERNAL when any is set.  The
 * host-pointer entry points check this themselves; callers of orbfe_extract_batch_device do it
 * here, outside their timed region. */
int orbfe_get_device_status(orbfe_handle *h, unsigned *flags_out);

/* -------------------------------------------------------------------------------------------
 * Pipelined host-pointer extraction (the reference's call shape -- a host image per frame,
 * src/Frame.cc:178-189 -- at stream rate): a ring of `slots` (>= 2) pinned + device buffers of
 * `slot_frames` (<= max_batch) frames each.  orbfe_stream_submit() enqueues upload, kernels and
 * result download of one slot on three HIP streams and returns without waiting;
 * orbfe_stream_collect() waits for the OLDEST submitted slot only and hands its results over.
 * Upload of slot i+1, kernels of slot i and download of slot i-1 overlap.  Pinned sources with a
 * 4-byte-aligned pitch are copied by the DMA engine straight from the caller's buffer; pageable
 * ones are re-pitched into the slot's pinned block by a small thread pool first.
 * Results are byte-identical to orbfe_extract_batch / orbfe_extract_batch_device.
 * Source lifetime: a pinned source may still be read by the DMA engine AFTER submit has returned
 * (pageable sources have been copied by then, but the caller cannot rely on which path ran):
 * every source frame must stay valid and UNCHANGED until the submission that carried it has been
 * collected -- a capture buffer recycled earlier gives torn frames and no error.
 * Threading: ONE producer thread may submit while ONE consumer thread collects (the reference feeds frames from a grabber
 * thread into the tracking thread, ros2_ws/src/mono-inertial/src/mono_inertial_node.cpp:207-210): the ring counters are
 * atomic, a slot belongs to its submission until that has been collected, and the copy pool is serialised between the
 * two.  Two threads submitting (or two collecting) at the same time, and destroy / orbfe_stream_enable_track while
 * another call is running, are not supported.
 * ---------------------------------------------------------------------------------------- */
typedef struct orbfe_stream orbfe_stream;
int orbfe_stream_create(orbfe_handle *h, int slots, int slot_frames, orbfe_stream **out);
void orbfe_stream_destroy(orbfe_stream *s);
/* enqueue `n` (1..slot_frames) frames; ORBFE_ERR_BUSY when `slots` submissions are uncollected */
int orbfe_stream_submit(orbfe_stream *s, const uint8_t *const *grays, int pitch, int n);
/* wait for the oldest submission; outputs as orbfe_extract_batch (strides cap / cap*32 / n_levels);
 * *n_frames receives how many frames that submission held.  ORBFE_ERR_INVALID_ARG when nothing
 * is in flight. */
int orbfe_stream_collect(orbfe_stream *s, orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out,
                         int *per_level_counts, int *n_frames);
/* the same without the copy: pointers into the slot's pinned result block (frame b at the strides
 * above), valid until the next orbfe_stream_submit() that reuses the slot (`slots` submissions
 * later) */
int orbfe_stream_collect_view(orbfe_stream *s, const orbfe_keypoint **kp, const uint8_t **desc,
                              const int **n, const int **per_level_counts, int *n_frames);
int orbfe_stream_in_flight(const orbfe_stream *s);

/* replaces the public members mvImagePyramid / mvBlurredImagePyramid
 * (include/ORBextractor.h:94-95): copies level `level` of frame `frame` of the LAST extract call
 * to host memory (out_pitch bytes per row).  Synchronises. */
int orbfe_get_pyramid_level(orbfe_handle *h, int frame, int level, int blurred, uint8_t *out,
                            int out_pitch);

/* Diagnostics for parity tests: FAST candidates of (frame, level) of the last extract call as
 * packed words (score << 24 | y << 12 | x), unordered; counters[4] = {survivors(low pass),
 * survivors with score >= iniThFAST, pre-NMS corners >= minThFAST, pre-NMS corners >= iniThFAST}.
 * Returns the number of words written (<= cap) through *n_out. */
int orbfe_debug_get_candidates(orbfe_handle *h, int frame, int level, uint32_t *packed, int cap,
                               int *n_out, int counters[4]);

/* Stage timing (HIP events on the launch stream).  While enabled, every extract call records
 * one event per stage boundary (a pool of 128 event sets; enabling resets the pool).
 * orbfe_get_stage_ms() synchronises on the recorded events and returns, per stage in the order of
 * orbfe_stage_name(), the SUM of elapsed milliseconds over the recorded calls; *n_calls receives
 * how many calls were summed (<= 128).  The last stage is the whole chain ("total").
 * A launch that takes the fused level build (one FAST launch per level that also writes the next
 * level; liborbfe_diag.so with ORBFE_FUSED_PYRAMID=1 only, as shipped no launch does) has no pyramid
 * launches: its "pyramid_resize" reads ~0 and "fast_nms_blur" covers the per-level launches. */
#define ORBFE_NUM_STAGES 5
int orbfe_set_stage_timing(orbfe_handle *h, int enabled);
int orbfe_get_stage_ms(orbfe_handle *h, float ms[ORBFE_NUM_STAGES], int *n_calls);
const char *orbfe_stage_name(int stage);

/* -------------------------------------------------------------------------------------------
 * Matcher
 * ---------------------------------------------------------------------------------------- */

#define ORBFE_TH_LOW 30        /* ORBmatcher::TH_LOW  (include/ORBmatcher.h:73) */
#define ORBFE_TH_HIGH 100      /* ORBmatcher::TH_HIGH (:74) */
#define ORBFE_HISTO_LENGTH 30  /* ORBmatcher::HISTO_LENGTH (:75) */

/* replaces ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1375-1391); host, no GPU. */
int orbfe_hamming(const uint8_t *a, const uint8_t *b);

/* What SearchByProjection reads from a Frame (include/Frame.h): keypoints, descriptors, the
 * static grid geometry (src/Frame.cc:101-105) and mvScaleFactors. */
typedef struct orbfe_frame_view {
    int n;                        /* mNumKeypoints */
    const orbfe_keypoint *kp;     /* mvKeysUn */
    const uint8_t *desc;          /* mDescriptors, n x 32 */
    int grid_cols, grid_rows;     /* mFrameGridCols / mFrameGridRows */
    float min_x, min_y;           /* mnMinX / mnMinY */
    float grid_inv_w, grid_inv_h; /* mfGridElementWidthInv / mfGridElementHeightInv */
    int n_levels;
    const float *scale_factors;   /* mvScaleFactors */
} orbfe_frame_view;

/* The MapPoint fields SearchByProjection reads (src/ORBmatcher.cc:36-59). */
typedef struct orbfe_map_point {
    float proj_x, proj_y;  /* mTrackProjX / mTrackProjY */
    float view_cos;        /* mTrackViewCos */
    float track_depth;     /* mTrackDepth */
    int level;             /* mnTrackScaleLevel */
    int in_view;           /* mbTrackInView */
    int bad;               /* isBad() */
    int observations;      /* Observations() */
} orbfe_map_point;

/* replaces ORBmatcher::SearchByProjection(Frame, vector<MapPoint>, th, bFarPoints, thFarPoints,
 * nnRatio, checkOrientation) (src/ORBmatcher.cc:31-123; callers src/Tracking.cc:1115), mono.
 * All pointers are HOST pointers.  init_obs[i] = -1 if F->mvpMapPoints[i] is empty on entry, else
 * the Observations() of the point it holds (may be NULL == all empty).  match_out[i] = index of
 * the map point this call writes into F->mvpMapPoints[i], or -1.  *n_matches = return value of
 * the reference function.  The greedy, order-dependent claim semantics are reproduced exactly. */
int orbfe_match_projection(orbfe_handle *h, const orbfe_frame_view *frame, int n_map_points,
                           const orbfe_map_point *map_points, const uint8_t *mp_desc,
                           const int *init_obs, float th, int far_points, float th_far_points,
                           float nn_ratio, int *match_out, int *n_matches);

/* Batched, HBM-resident form of the same function (no reference analogue; BASELINE configs 2/3):
 * frame b's keypoints / descriptors / counts are the outputs of orbfe_extract_batch_device
 * (stride kp_stride == orbfe_max_keypoints()), its map points are d_map_points[b*n_map_points ..],
 * scale factors are the handle's own mvScaleFactor.  All d_* pointers are device pointers;
 * d_init_obs may be NULL.  Fully asynchronous on `stream` (a hipStream_t; NULL == the handle's own
 * stream): three kernels are queued and no host synchronisation takes place; results are complete when
 * the stream reaches that point. */
int orbfe_match_projection_batch_device(orbfe_handle *h, int batch, const orbfe_keypoint *d_kp,
                                        const uint8_t *d_desc, const int *d_n, int kp_stride,
                                        int grid_cols, int grid_rows, float min_x, float min_y,
                                        float grid_inv_w, float grid_inv_h, int n_map_points,
                                        const orbfe_map_point *d_map_points, const uint8_t *d_mp_desc,
                                        const int *d_init_obs, float th, int far_points,
                                        float th_far_points, float nn_ratio, int *d_match_out,
                                        int *d_n_matches, void *stream);

/* replaces ORBmatcher::SearchByBoW(KeyFrame, Frame, matches, nnRatio, checkOrientation)
 * (src/ORBmatcher.cc:133-327; caller src/Tracking.cc:835), mono.  The merge-walk over the two
 * DBoW2::FeatureVector maps (:161-163,289-301) is done by the caller/adaptor and handed over as
 * CSR groups in ascending NodeId order: group g = KF features kf_idx[kf_off[g]..kf_off[g+1]) and
 * frame features f_idx[f_off[g]..f_off[g+1]).  kf_has_mp[i] != 0 iff KF feature i has a non-bad
 * map point.  match_out[j] (n_f ints) = KF feature whose map point goes to frame feature j, or
 * -1; *n_matches = the reference's return value (after the rotation-histogram filter). */
int orbfe_match_bow(orbfe_handle *h, int n_groups, const int *kf_off, const int *kf_idx,
                    const int *f_off, const int *f_idx, int n_kf, const uint8_t *kf_desc,
                    const float *kf_angle, const uint8_t *kf_has_mp, int n_f,
                    const uint8_t *f_desc, const float *f_angle, float nn_ratio,
                    int check_orientation, int *match_out, int *n_matches);

/* the same for a frame of a two-camera rig (F->Nleft != -1, src/ORBmatcher.cc:205-233,263-286): frame features
 * >= n_left belong to the right camera and keep their own best / second best; the right best is accepted whenever the
 * LEFT best passes TH_LOW and its own distance does too (the reference's ratio test there reads "|| true").
 * n_left == -1 is orbfe_match_bow. */
int orbfe_match_bow_rig(orbfe_handle *h, int n_groups, const int *kf_off, const int *kf_idx,
                    const int *f_off, const int *f_idx, int n_kf, const uint8_t *kf_desc,
                    const float *kf_angle, const uint8_t *kf_has_mp, int n_f,
                    const uint8_t *f_desc, const float *f_angle, int n_left, float nn_ratio,
                    int check_orientation, int *match_out, int *n_matches);

/* replaces ORBmatcher::SearchForInitialization(F1, F2, windowSize, nnRatio, checkOrientation)
 * (src/ORBmatcher.cc:329-439; caller src/Tracking.cc:605-607), mono.  HOST pointers.  Frame 1
 * contributes keypoints + descriptors; frame 2 additionally its grid (GetFeaturesInArea runs on
 * frame 2).  Only level-0 keypoints of frame 1 take part (:346-347).  matches12_out (f1->n ints)
 * receives vnMatches12 (index in frame 2 or -1), *n_matches the function's return value. */
int orbfe_match_initialization(orbfe_handle *h, const orbfe_frame_view *f1, const orbfe_frame_view *f2,
                               int window_size, float nn_ratio, int check_orientation,
                               int *matches12_out, int *n_matches);

/* -------------------------------------------------------------------------------------------
 * Map-point projection: Frame::isInFrustum for a batch
 * ---------------------------------------------------------------------------------------- */
#define ORBFE_CAMERA_PINHOLE 0
#define ORBFE_CAMERA_KANNALA_BRANDT8 1

/* what Frame::isInFrustum reads from the frame (src/Frame.cc:272-331) */
typedef struct orbfe_frustum {
    float rcw[9];             /* GetRcw(), row-major */
    float tcw[3];             /* GetTcw() */
    float twc[3];             /* GetTwc() (camera centre) */
    float min_x, max_x, min_y, max_y; /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float fx, fy, cx, cy;     /* mvParameters[0..3] (src/CameraModels/Pinhole.cpp:41-47, KannalaBrandt8.cpp:66-83) */
    float k1, k2, k3, k4;     /* KannalaBrandt8 mvParameters[4..7]; ignored by the pinhole model */
    float mbf;                /* stereo baseline * fx (mTrackProjXR) */
    float log_scale_factor;   /* mfLogScaleFactor (src/Frame.cc:75) */
    int n_levels;             /* mnScaleLevels */
    int camera_model;         /* ORBFE_CAMERA_PINHOLE or ORBFE_CAMERA_KANNALA_BRANDT8 */
} orbfe_frustum;

/* what it reads from a MapPoint, plus the two skip conditions of Tracking::SearchLocalPoints
 * (src/Tracking.cc:1066-1069) */
typedef struct orbfe_world_point {
    float x, y, z;            /* GetWorldPos() */
    float min_distance;       /* mfMinDistance (GetMinDistanceInvariance() == 0.9f * this) */
    float max_distance;       /* mfMaxDistance (GetMaxDistanceInvariance() == 1.1f * this) */
    int bad;                  /* isBad() */
    int observations;         /* Observations() (passed through to the matcher record) */
    int skip;                 /* mnLastFrameSeen == current frame id */
} orbfe_world_point;

/* replaces the isInFrustum loop of Tracking::SearchLocalPoints (src/Tracking.cc:1059-1077): out[i] holds
 * the fields the reference writes into the MapPoint (mTrackProjX/Y, mTrackViewCos, mTrackDepth,
 * mnTrackScaleLevel, mbTrackInView), i.e. the input records of orbfe_match_projection; proj_xr
 * (mTrackProjXR) may be NULL.  HOST pointers.  Points that fail keep in_view == 0; proj_x / proj_y are -1 unless
 * the projection landed inside the image bounds (as the reference leaves them). */
int orbfe_project_map_points(orbfe_handle *h, const orbfe_frustum *frustum, int n,
                             const orbfe_world_point *points, orbfe_map_point *out, float *proj_xr);
/* Same with DEVICE pointers, asynchronous on `stream` (NULL == the handle's stream): the output feeds
 * orbfe_match_projection_batch_device directly. */
int orbfe_project_map_points_device(orbfe_handle *h, const orbfe_frustum *frustum, int n,
                                    const orbfe_world_point *d_points, orbfe_map_point *d_out,
                                    float *d_proj_xr, void *stream);

/* -------------------------------------------------------------------------------------------
 * The tracking thread's per-frame chain as ONE submission
 * ---------------------------------------------------------------------------------------- */

/* the frame statics and call parameters SearchByProjection reads besides the map points (src/Frame.cc:101-105,
 * src/Tracking.cc:1108-1115); versioned by its size like orbfe_tri_params */
typedef struct orbfe_track_params {
    int struct_size;               /* sizeof(orbfe_track_params) at the caller's compile time */
    int grid_cols, grid_rows;      /* mFrameGridCols / mFrameGridRows */
    float min_x, min_y;            /* mnMinX / mnMinY */
    float grid_inv_w, grid_inv_h;  /* mfGridElementWidthInv / mfGridElementHeightInv */
    float th;                      /* 20 before the IMU is initialised, 40 after (src/Tracking.cc:1108-1113) */
    float nn_ratio;                /* 0.85 / 0.75 */
    int far_points;                /* bFarPoints */
    float th_far_points;           /* thFarPoints */
} orbfe_track_params;
#define ORBFE_TRACK_PARAMS_INIT {(int)sizeof(orbfe_track_params)}

/* What the tracking thread of this fork does with every frame once the IMU is initialised, in one call:
 *   Frame::Frame -> ExtractORB -> ORBextractor::extractFeatures          (src/Tracking.cc:152-173, src/Frame.cc:178-189)
 *   Tracking::SearchLocalPoints: isInFrustum for every local map point   (src/Tracking.cc:1059-1077, src/Frame.cc:272-333)
 *   ORBmatcher::SearchByProjection(mCurrentFrame, mvpLocalMapPoints, ...) (src/Tracking.cc:1108-1115)
 * The pose that isInFrustum needs does not depend on the frame's features here: TrackWithMotionModel is the IMU
 * prediction alone (src/Tracking.cc:908-923, PredictStateIMU :293), and the local map comes from the LAST frame's
 * matches (:1190), so image, predicted pose and local map points are all known when the frame arrives.
 * Equivalent to orbfe_extract + orbfe_project_map_points + orbfe_match_projection (frame view = the fresh keypoints
 * with the grid of `tp` and the extractor's own mvScaleFactors; init_obs == NULL: mvpMapPoints is empty at that point),
 * bit for bit -- but as ONE captured hipGraph: the host frame and one block [frustum | points | descriptors] go up,
 * memset + extraction kernels + frustum kernel + three matcher kernels run back to back with no host in between, ONE
 * result block comes back, one host synchronisation.
 * gray / pitch as orbfe_extract; points / mp_desc: n_points local map points (HOST pointers; mp_desc n_points x 32);
 * frustum->n_levels must not exceed the extractor's level count.
 * kp_out / desc_out / n_out / per_level_counts as orbfe_extract; mp_out (n_points records, may be NULL) and proj_xr_out
 * (may be NULL) as orbfe_project_map_points; match_out (orbfe_max_keypoints() ints; the first *n_out are meaningful)
 * and n_matches as orbfe_match_projection.  A frame without keypoints gives *n_out == 0 and *n_matches == 0.
 * Graphs are cached per (n_points rounded up to a bucket, input pitch, tp): a steady stream replays one graph. */
int orbfe_track_frame(orbfe_handle *h, const uint8_t *gray, int pitch, const orbfe_frustum *frustum,
                      const orbfe_track_params *tp, int n_points, const orbfe_world_point *points,
                      const uint8_t *mp_desc, orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out,
                      int *per_level_counts, orbfe_map_point *mp_out, float *proj_xr_out, int *match_out,
                      int *n_matches);

/* what ORBmatcher::SearchForTriangulation derives from the two key-frame poses (src/ORBmatcher.cc:448-465).
 * ABI: the block is versioned by its size.  struct_size must hold sizeof(orbfe_tri_params) of the header the CALLER was
 * compiled against (`orbfe_tri_params p = ORBFE_TRI_PARAMS_INIT;` zero-initialises the rest); the library refuses any
 * other value with ORBFE_ERR_INVALID_ARG instead of reading past a shorter block (the struct grew a camera-model tail in
 * round 2). */
typedef struct orbfe_tri_params {
    int struct_size;        /* sizeof(orbfe_tri_params) at the caller's compile time */
    float f12[9];           /* F12 = K1^-T [t12]x R12 K2^-1, row-major: the matrix Pinhole::epipolarConstrain
                             * rebuilds for every pair (src/CameraModels/Pinhole.cpp:106-109) */
    float ep_x, ep_y;       /* epipole: pKF2->mpCamera->project(T2w * Cw) (:451-454) */
    int only_stereo;        /* bOnlyStereo */
    int coarse;             /* bCoarse */
    int check_orientation;  /* checkOrientation */
    /* ---- camera models (zero-initialised == one pinhole camera per key frame, the fields above suffice) ---- */
    int camera_model1;      /* ORBFE_CAMERA_* of pKF1->mpCamera: KANNALA_BRANDT8 selects KannalaBrandt8::epipolarConstrain
                             * (src/CameraModels/KannalaBrandt8.cpp:216-220,306-370: triangulate the pair, both depths positive,
                             * both reprojection errors inside 5.991 sigma^2) instead of the F12 line test */
    int camera_model2;      /* ORBFE_CAMERA_* of pKF2->mpCamera (unproject / project of the second view) */
    float cam1[8], cam2[8]; /* mvParameters of the two cameras: fx fy cx cy k1 k2 k3 k4 */
    float kb_precision;     /* KannalaBrandt8::precision (Newton stop of unproject; the reference's default is 1e-6) */
    float r12[9], t12[3];   /* T12 = T1w * Tw2 (:466-468; in this fork also when the key frames carry a second camera:
                             * bRight1 / bRight2 are constants, :520,:549): rotation row-major, translation */
    float level_sigma2_1[ORBFE_MAX_LEVELS]; /* pKF1->mvLevelSigma2 (sigmaLevel of the first view; unc is 1.0, :603) */
    int kf1_has_camera2;    /* pKF1->mpCamera2 is set: the epipole gate (:551) is skipped */
} orbfe_tri_params;
#define ORBFE_TRI_PARAMS_INIT {(int)sizeof(orbfe_tri_params)}

/* replaces ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse,
 * checkOrientation) (src/ORBmatcher.cc:441-676; caller src/LocalMapping.cc:488), one pinhole camera per key
 * frame, or KannalaBrandt8 cameras (camera_model1 / camera_model2 of the parameter block: SPEC DECISION S10 -- the
 * reference triangulates with an Eigen JacobiSVD in binary32, which is not reproducible bit for bit; here the null vector
 * of the 4x4 system comes from a fixed cyclic-Jacobi sequence on A^T A in binary64, so the verdicts agree with the
 * reference except for pairs whose depth or reprojection error sits within rounding distance of a threshold).
 * The merge-walk over the two FeatureVectors (:489-617) is handed over as CSR groups in ascending
 * NodeId order (as for orbfe_match_bow).  has_mp* [i] != 0 iff GetMapPoint(i) is set; stereo* [i] != 0 iff
 * mvuRight[i] >= 0 (NULL == monocular); scale_factors2 = pKF2->mvScaleFactors (n_levels2 floats).
 * matches12_out[i1] (n1 ints) = index in key frame 2 or -1, i.e. vMatchedPairs = {(i1, matches12_out[i1])} in
 * ascending i1; *n_matches = the return value.  HOST pointers. */
int orbfe_match_triangulation(orbfe_handle *h, int n_groups, const int *kf1_off, const int *kf1_idx,
                              const int *kf2_off, const int *kf2_idx, int n1, const orbfe_keypoint *kp1,
                              const uint8_t *desc1, const uint8_t *has_mp1, const uint8_t *stereo1, int n2,
                              const orbfe_keypoint *kp2, const uint8_t *desc2, const uint8_t *has_mp2,
                              const uint8_t *stereo2, const float *scale_factors2, int n_levels2,
                              const orbfe_tri_params *params, int *matches12_out, int *n_matches);

/* -------------------------------------------------------------------------------------------
 * Map points resident in HBM + the extract-and-match form of the ring
 * ---------------------------------------------------------------------------------------- */
typedef struct orbfe_map orbfe_map;

/* A device-resident table of what isInFrustum and SearchByProjection read from a MapPoint (GetWorldPos, mfMinDistance,
 * mfMaxDistance, isBad, Observations: orbfe_world_point; GetDescriptor: 32 bytes), indexed by a caller-chosen id in
 * [0, capacity).  The local map of consecutive frames is nearly the same set of points (src/Tracking.cc:1117-1230), so a
 * frame names its points by id (4 bytes each) instead of shipping 64 bytes per point per frame across PCIe.
 * orbfe_map_update (HOST pointers) writes entries ids[0..n) -- new points, and points whose position / descriptor /
 * observation count changed; it is ordered behind everything submitted before it and returns when the table is updated.
 * The `skip` member of the records is ignored (it is per frame: see orbfe_stream_submit_track).
 * Lifetime: orbfe_map_destroy waits for the handle's stream, drops the graphs of orbfe_track_frame_map and detaches the map
 * from every ring it was given to (orbfe_stream_enable_track): that ring refuses later orbfe_stream_submit_track calls with
 * ORBFE_ERR_INVALID_ARG (collect what is in flight BEFORE destroying the map).  orbfe_destroy releases the device memory of the
 * maps and rings created from the handle; destroying them afterwards is safe and only frees the shell, any other call on them
 * returns ORBFE_ERR_INVALID_ARG. */
int orbfe_map_create(orbfe_handle *h, int capacity, orbfe_map **out);
void orbfe_map_destroy(orbfe_map *m);
int orbfe_map_update(orbfe_handle *h, orbfe_map *m, int n, const int *ids, const orbfe_world_point *points,
                     const uint8_t *desc);

/* Gives the ring what it needs to run the whole per-frame chain of orbfe_track_frame per slot: extraction, isInFrustum
 * of the frame's local map points against the frame's own pose, SearchByProjection -- H2D || extract + project + match ||
 * D2H.  max_points = the largest n_points a submission will carry.  Call once, before the first submission (a call that
 * fails with ORBFE_ERR_OUT_OF_MEMORY leaves the ring as it was and may be repeated). */
/* orbfe_track_frame with the local map points named by id out of the resident map (ids as orbfe_stream_submit_track:
 * id >= 0, ~id = skipped for this frame, outside the map = no point): 8 KB instead of 128 KB go up per frame at 2000
 * points.  mp_out / proj_xr_out / match_out index the id list.  Same results as orbfe_track_frame on the same points. */
int orbfe_track_frame_map(orbfe_handle *h, const uint8_t *gray, int pitch, const orbfe_frustum *frustum,
                          const orbfe_track_params *tp, const orbfe_map *map, int n_points, const int *ids,
                          orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out, int *per_level_counts,
                          orbfe_map_point *mp_out, float *proj_xr_out, int *match_out, int *n_matches);

int orbfe_stream_enable_track(orbfe_stream *s, orbfe_map *map, int max_points);
/* orbfe_stream_submit + per frame b: frusta[b] (pose, bounds, camera of THAT frame) and the ids of its n_points local
 * map points, ids[b * n_points + i]: id >= 0 = entry of the resident map; ~id (negative) = the same entry with
 * "mnLastFrameSeen == current frame" (src/Tracking.cc:1066, skipped); an id outside the map = no point.  tp as
 * orbfe_track_frame.  HOST pointers; everything is copied before the call returns except pinned frames (see above). */
int orbfe_stream_submit_track(orbfe_stream *s, const uint8_t *const *grays, int pitch, int n, const orbfe_track_params *tp,
                              const orbfe_frustum *frusta, int n_points, const int *ids);
/* orbfe_stream_collect + the matches of a submission made with orbfe_stream_submit_track: match_out[b * cap + i] =
 * position in frame b's id list of the map point written to mvpMapPoints[i], or -1 (cap = orbfe_max_keypoints());
 * n_matches[b] = the return value of SearchByProjection.  Byte-identical to orbfe_track_frame per frame. */
int orbfe_stream_collect_track(orbfe_stream *s, orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out, int *per_level_counts,
                               int *match_out, int *n_matches, int *n_frames);

/* -------------------------------------------------------------------------------------------
 * Key frames resident in HBM + the mapping thread's batched SearchForTriangulation
 * ---------------------------------------------------------------------------------------- */
typedef struct orbfe_keyframe orbfe_keyframe;

/* Uploads what the key-frame matchers read from a KeyFrame and what never changes after its construction
 * (src/KeyFrame.cc:33-80): mvKeysUn (n keypoints), mDescriptors (n x 32), mFeatVec as node_id[i] = the
 * DBoW2::FeatureVector key of feature i (the vocabulary node `levelsup` levels above its word, src/Frame.cc:483-495;
 * -1 = the feature is in no node: DBoW2 adds a feature to the FeatureVector only when its word's weight is > 0,
 * TemplatedVocabulary.h:1168-1172, so features on stopped words get -1), stereo[i] != 0 iff mvuRight[i] >= 0 (NULL == monocular), mvScaleFactors.
 * The features of a node are walked in ascending feature index, the order DBoW2 stores them in
 * (Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h:1157-1170).  HOST pointers; one upload, then the key frame stays
 * on the device until orbfe_keyframe_destroy.  Keypoint octaves must lie in [0, n_levels). */
int orbfe_keyframe_create(orbfe_handle *h, int n, const orbfe_keypoint *kp, const uint8_t *desc, const int *node_id,
                          const uint8_t *stereo, const float *scale_factors, int n_levels, orbfe_keyframe **out);
void orbfe_keyframe_destroy(orbfe_keyframe *kf);
int orbfe_keyframe_size(const orbfe_keyframe *kf);

/* replaces the K calls ORBmatcher::SearchForTriangulation(mpCurrentKeyFrame, pKF2, vMatchedIndices, false, bCoarse, true)
 * of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:455-488, up to 30 neighbours per new key frame) by ONE
 * launch: kf1 against kf2[0..K), params[k] as orbfe_match_triangulation's for the pair (kf1, kf2[k]),
 * has_mp1[i] / has_mp2[k][i] != 0 iff GetMapPoint(i) is set WHEN THE CALL IS MADE.
 * Between two neighbours the reference turns matches into new map points (:500-700); a feature of key frame 1 that
 * received one is skipped for the later neighbours (src/ORBmatcher.cc:506-509) and drops out of their rotation
 * histograms.  So this call returns, per neighbour k and feature i1 of key frame 1, the RAW partner
 * raw_match12[k * n1 + i1] (index in kf2[k] or -1) and its rotation bin raw_bin[k * n1 + i1] BEFORE the orientation
 * filter; the caller walks the neighbours in order and calls orbfe_triangulation_select with the has_mp1 flags as they
 * stand at that point.  That reproduces the K sequential calls exactly: vbMatched2 is never set in this fork
 * (src/ORBmatcher.cc:485,537), so every feature of key frame 1 chooses its partner independently of the others, and the
 * only state shared between neighbours is "idx1 already has a map point".  HOST pointers except the key frames. */
int orbfe_match_triangulation_batch(orbfe_handle *h, const orbfe_keyframe *kf1, const uint8_t *has_mp1, int K,
                                    const orbfe_keyframe *const *kf2, const uint8_t *const *has_mp2,
                                    const orbfe_tri_params *params, int *raw_match12, uint8_t *raw_bin);
/* host-only: vMatchedPairs / the return value of neighbour k's SearchForTriangulation call from the raw results of the
 * batch call and the CURRENT flags of key frame 1: features with has_mp1_now[i1] != 0 drop out (:506-509), then the
 * rotation histogram and ComputeThreeMaxima (:633-661, :1328-1370) when check_orientation.  raw_match12 / raw_bin point
 * at neighbour k's n1 entries.  matches12_out[i1] = index in key frame 2 or -1. */
int orbfe_triangulation_select(int n1, const int *raw_match12, const uint8_t *raw_bin, const uint8_t *has_mp1_now,
                               int check_orientation, int *matches12_out, int *n_matches);

/* -------------------------------------------------------------------------------------------
 * The second loop of LocalMapping::CreateNewMapPoints: "triangulate each match" (src/LocalMapping.cc:501-705)
 * ---------------------------------------------------------------------------------------- */
/* verdict of one pair, in the order of the reference's gates (SPEC DECISION S11) */
#define ORBFE_NEWPT_ACCEPTED        0   /* a new map point at x3d */
#define ORBFE_NEWPT_LOW_PARALLAX    1   /* cosParallaxRays <= 0 or >= 0.9998 (0.9996 inertial), :596,:615-618; no point */
#define ORBFE_NEWPT_AT_INFINITY     2   /* x3Dh(3) == 0, src/GeometricTools.cc:59; no point */
#define ORBFE_NEWPT_BEHIND_1        3   /* z1 <= 0, :627-629 */
#define ORBFE_NEWPT_BEHIND_2        4   /* z2 <= 0, :631-633 */
#define ORBFE_NEWPT_REPROJECTION_1  5   /* reprojection error in key frame 1 above 5.991 sigma^2, :643-648 */
#define ORBFE_NEWPT_REPROJECTION_2  6   /* ... in key frame 2, :670-674 */
#define ORBFE_NEWPT_ZERO_DISTANCE   7   /* dist1 == 0 || dist2 == 0, :695 */
#define ORBFE_NEWPT_FAR             8   /* mbFarPoints && (dist1 >= mThFarPoints || dist2 >= mThFarPoints), :698 */
#define ORBFE_NEWPT_SCALE           9   /* scale consistency, :701-705 */
#define ORBFE_NEWPT_NO_PARTNER      255 /* the batch search found no partner for this feature; no point */

/* what the triangulation loop reads besides the two key frames' keypoints and scale factors, for ONE pair (key frame 1,
 * neighbour).  Monocular key frames only (mvuRight < 0, NLeft == -1, no mpCamera2: bStereo1 == bStereo2 == bRight2 == false).
 * Versioned by struct_size like orbfe_tri_params. */
typedef struct orbfe_newpoint_params {
    int struct_size;         /* sizeof(orbfe_newpoint_params) at the caller's compile time */
    float tcw1[12];          /* GetPose().matrix3x4() of key frame 1, row-major 3 x 4 (eigTcw1, :432-436) */
    float tcw2[12];          /* ... of the neighbour (eigTcw2, :490-494) */
    float twc1[3], twc2[3];  /* GetTranslationInverse() of the two key frames (:440,:464): taken as given, not recomputed */
    int camera_model1;       /* ORBFE_CAMERA_* of pKF1->mpCamera / pKF2->mpCamera */
    int camera_model2;
    float cam1[8], cam2[8];  /* fx fy cx cy k1 k2 k3 k4 */
    float kb_precision;      /* KannalaBrandt8::precision */
    float level_sigma2_1[ORBFE_MAX_LEVELS]; /* mpCurrentKeyFrame->mvLevelSigma2 */
    float level_sigma2_2[ORBFE_MAX_LEVELS]; /* pKF2->mvLevelSigma2 */
    float ratio_factor;      /* 1.5f * mpCurrentKeyFrame->mfScaleFactor (:447) */
    int inertial;            /* mbInertial: parallax limit 0.9996 instead of 0.9998 (:597) */
    int far_points;          /* mbFarPoints */
    float th_far_points;     /* mThFarPoints */
} orbfe_newpoint_params;
#define ORBFE_NEWPOINT_PARAMS_INIT {(int)sizeof(orbfe_newpoint_params)}

/* orbfe_match_triangulation_batch + the geometry of src/LocalMapping.cc:571-705 for EVERY raw partner, in the same
 * submission (one upload, two launches back to back, one download, one synchronisation).  Arguments up to raw_bin as
 * orbfe_match_triangulation_batch (same bytes come back); np_params[k] describes the pair (kf1, kf2[k]).
 * verdict_out[k * n1 + i1] = ORBFE_NEWPT_* of the pair (i1, raw_match12[k * n1 + i1]); x3d_out[(k * n1 + i1) * 3 ..] = x3D of
 * that pair (three zeros where no point exists: verdicts 1, 2 and 255).  The verdict and the point of a pair depend only on
 * the two keypoints, the two poses and the two cameras, so the caller walks the neighbours in order, takes
 * orbfe_triangulation_select's matches with the flags as they stand and looks the verdict up: exactly the reference's loop.
 * A key frame created with stereo flags -> ORBFE_ERR_UNSUPPORTED (the stereo branches are not built).  HOST pointers
 * except the key frames. */
int orbfe_create_new_points_batch(orbfe_handle *h, const orbfe_keyframe *kf1, const uint8_t *has_mp1, int K,
                                  const orbfe_keyframe *const *kf2, const uint8_t *const *has_mp2,
                                  const orbfe_tri_params *tri_params, const orbfe_newpoint_params *np_params,
                                  int *raw_match12, uint8_t *raw_bin, float *x3d_out, uint8_t *verdict_out);
/* the geometry alone for n_pairs explicit pairs (idx1[p] in kf1, idx2[p] in kf2) of two resident key frames:
 * x3d_out[3 * p ..], verdict_out[p].  An index out of range -> ORBFE_ERR_INVALID_ARG.  HOST pointers. */
int orbfe_triangulate_pairs(orbfe_handle *h, const orbfe_keyframe *kf1, const orbfe_keyframe *kf2,
                            const orbfe_newpoint_params *np_params, int n_pairs, const int *idx1, const int *idx2,
                            float *x3d_out, uint8_t *verdict_out);

/* replaces the search part of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false)
 * (src/ORBmatcher.cc:678-836; callers src/LocalMapping.cc:822,852): per map point the projection into the
 * key frame, KeyFrame::IsInImage, PredictScale, KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:790-833), the
 * chi-square gate and the nearest descriptor.  points[i].skip carries "!pMP || pMP->IsInKeyFrame(pKF)".
 * inv_level_sigma2 = pKF->mvInvLevelSigma2 (KF->n_levels floats); u_right = pKF->mvuRight or NULL (monocular).
 * best_idx_out[i] / best_dist_out[i] = bestIdx / bestDist of :776-826 (-1 / 256 when nothing qualified); the
 * caller applies bestDist <= TH_LOW and the map-point graph edits (:829-849) in list order.  HOST pointers. */
int orbfe_fuse_search(orbfe_handle *h, const orbfe_frame_view *KF, const float *inv_level_sigma2,
                      const float *u_right, const orbfe_frustum *frustum, float th, int M,
                      const orbfe_world_point *points, const uint8_t *mp_desc, int *best_idx_out,
                      int *best_dist_out);

/* What the projection searches INTO a resident key frame read besides orbfe_keyframe_create's arrays: mGrid (the geometry of
 * orbfe_frame_view: grid_cols x grid_rows cells from (min_x, min_y) with the inverse cell sizes, src/KeyFrame.cc:33-80 copies them
 * from the Frame), mvInvLevelSigma2 (n_levels floats) and mvuRight (n floats, or NULL == monocular).  The per-level cell
 * tables are built here, ONCE, and stay with the key frame; calling it again replaces them.  HOST pointers; synchronises. */
int orbfe_keyframe_set_grid(orbfe_handle *h, orbfe_keyframe *kf, int grid_cols, int grid_rows, float min_x, float min_y,
                            float grid_inv_w, float grid_inv_h, const float *inv_level_sigma2, const float *u_right);

/* orbfe_fuse_search on RESIDENT data -- LocalMapping::SearchInNeighbors (src/LocalMapping.cc:764-860) calls
 * ORBmatcher::Fuse(pKFi, vpMapPointMatches) for every neighbour and Fuse(mpCurrentKeyFrame, vpFuseCandidates) once
 * (:822,:852): up to 2 x 30 calls per new key frame, every one of which re-uploaded its target key frame (56 B per feature)
 * and its map points (64 B each) through orbfe_fuse_search although both already sit in HBM.  Here the target is a key
 * frame of orbfe_keyframe_create with orbfe_keyframe_set_grid done, the map points are entries of an orbfe_map named by id:
 * ids[i] >= 0 = the entry; ~id (negative) = the entry with "!pMP || pMP->IsInKeyFrame(pKF)" for this call (skipped,
 * src/ORBmatcher.cc:706-721); an id outside the map = no point.  Up go the frustum and 4 bytes per map point, down come
 * best_idx_out[i] / best_dist_out[i] as orbfe_fuse_search (-1 / 256 when nothing qualified).  With this call the calls of one
 * SearchInNeighbors stay sequential (orbfe_fuse_search_keyframes below does all targets at once) -- between two of them the
 * caller replaces / adds map points (:829-849); descriptor and position changes reach the map through orbfe_map_update,
 * which is ordered in front of the next call.
 * Same results as orbfe_fuse_search on the same key frame, map points and flags (monocular / stereo left camera; the bRight
 * overload has no resident form). */
int orbfe_fuse_search_keyframe(orbfe_handle *h, const orbfe_keyframe *kf, const orbfe_map *map, int M, const int *ids,
                               const orbfe_frustum *frustum, float th, int *best_idx_out, int *best_dist_out);

/* orbfe_fuse_search_keyframe into ALL targets of one SearchInNeighbors loop (src/LocalMapping.cc:819-824) in one submission.
 * Everything a search does before it compares descriptors (projection, IsInImage, distance gate, PredictScale,
 * GetFeaturesInArea, level and chi-square gates, src/ORBmatcher.cc:724-820) reads only what the loop never changes; the skip
 * conditions only ever turn ON during the loop; the descriptor enters in the strict "<" scan alone (:824-832).  So the call
 * returns, per pair, the best candidate under the descriptor the map holds NOW and the gated candidates in visit order, and the
 * caller walks the targets in order: a pair skipped by now is masked on the host, a point whose descriptor changed since the
 * call (MapPoint::Replace -> ComputeDistinctiveDescriptors) gets its result from orbfe_fuse_select over its list.
 * rows k = 0..K-1: exactly orbfe_fuse_search_keyframe(h, kfs[k], map, M, ids_k, &frusta[k], th, ...) with
 * ids_k[i] = skip && skip[k*M+i] ? (ids[i] < 0 ? ids[i] : ~ids[i]) : ids[i]      -- ONE upload, ONE launch, ONE download, ONE sync.
 * best_idx_out / best_dist_out: K*M ints each (-1 / 256 when nothing qualified).
 * cand_cap in [0,16]; when > 0: cand_count_out[k*M+i] = number of features that passed every gate of :787-820 for the pair
 * (the TRUE count, it may exceed cand_cap), cand_idx_out[(k*M+i)*cand_cap + j] = the j-th of them in the reference's
 * visit order (the order in which the strict "<" of :828 sees them), -1 beyond the count.  HOST pointers except kfs / map.
 * Validation per target is the single call's (grid set, frusta[k].n_levels within the key frame's levels); K == 0 or M == 0
 * returns ORBFE_OK and writes nothing; a NULL among the required pointers or cand_cap outside [0,16] is ORBFE_ERR_INVALID_ARG
 * before anything is enqueued.  Targets may differ in feature count (0 included), grid, camera model and mono / stereo; the
 * same key frame may appear twice.  The bRight overload has no resident form. */
int orbfe_fuse_search_keyframes(orbfe_handle *h, int K, const orbfe_keyframe *const *kfs, const orbfe_frustum *frusta,
                                const orbfe_map *map, int M, const int *ids, const uint8_t *skip, float th,
                                int *best_idx_out, int *best_dist_out, int cand_cap, int *cand_idx_out, int *cand_count_out);

/* host-only, no handle: the scan of :824-832 for ONE pair over a candidate list of the call above, with a descriptor the
 * caller supplies (the point's descriptor NOW).  kf_desc = the target's mDescriptors (host, n_kf x 32).  Ties keep the
 * earlier entry; an empty list gives -1 / 256.  Returns ORBFE_ERR_UNSUPPORTED when cand_count > cand_cap (list truncated:
 * use orbfe_fuse_search_keyframe for that pair), ORBFE_ERR_INVALID_ARG for an index outside [0, n_kf). */
int orbfe_fuse_select(const int *cand_idx, int cand_count, int cand_cap, const uint8_t *kf_desc, int n_kf,
                      const uint8_t *mp_desc, int *best_idx, int *best_dist);

/* orbfe_fuse_search with bRight = true (src/ORBmatcher.cc:684-688,:820; callers src/LocalMapping.cc:824,854 when the key frame
 * has a second camera): frustum carries pKF->GetRightPose() / GetRightTranslationInverse() / mpCamera2; KF_left
 * describes the LEFT features (KF_left->n == pKF->NLeft -- they fill mGrid, and the level and chi-square gates read them,
 * as in the reference) while KF_left->desc is all of pKF->mDescriptors: NLeft + n_right rows.  The compared descriptor
 * row and best_idx_out are idx + NLeft (:820).  Where the reference would read a row beyond the matrix (idx >= n_right)
 * the candidate is skipped. */
int orbfe_fuse_search_right(orbfe_handle *h, const orbfe_frame_view *KF_left, int n_right, const float *inv_level_sigma2,
                            const float *u_right, const orbfe_frustum *frustum, float th, int M,
                            const orbfe_world_point *points, const uint8_t *mp_desc, int *best_idx_out,
                            int *best_dist_out);

/* replaces the search part of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:864-975;
 * no caller in this fork -- the loop-closing thread is gone -- but part of the class, include/ORBmatcher.h:69): the
 * same walk as orbfe_fuse_search without the chi-square gate.  The caller decomposes Scw as the reference does
 * (:867-868): frustum->rcw = Scw.rotationMatrix(), tcw = Scw.translation() / Scw.scale(), twc =
 * Tcw.inverse().translation(); points[i].skip carries "spAlreadyFound.count(pMP)".  The caller applies
 * bestDist <= TH_LOW, vpReplacePoint and the graph edits (:955-971) in list order.  HOST pointers. */
int orbfe_fuse_search_sim3(orbfe_handle *h, const orbfe_frame_view *KF, const orbfe_frustum *frustum, float th, int M,
                           const orbfe_world_point *points, const uint8_t *mp_desc, int *best_idx_out,
                           int *best_dist_out);

/* one search direction of ORBmatcher::SearchBySim3 */
typedef struct orbfe_sim3_view {
    float rcw[9], tcw[3];     /* pose of the key frame that owns the map points (T1w for 1->2, :986-987) */
    float sr[9], t[3];        /* the similarity into the other key frame as s*R (row-major) and t (S21 for 1->2) */
    float fx, fy, cx, cy;     /* pKF1's intrinsics -- the reference uses them for both directions (:979-982) */
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY of the TARGET key frame (KeyFrame::IsInImage) */
    float log_scale_factor;   /* mfLogScaleFactor of the target key frame */
    int n_levels;             /* mnScaleLevels of the target key frame */
} orbfe_sim3_view;

/* replaces ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (src/ORBmatcher.cc:977-1200; no caller in this
 * fork).  mp1 / mp_desc1: one record per feature of key frame 1 (KF1->n entries; skip = "no map point" or
 * vbAlreadyMatched1 of :1001-1012), mp2 / mp_desc2 likewise for key frame 2.  dir12 moves key frame 1's points
 * into key frame 2 (T1w, S21), dir21 the other way (T2w, S12).  match12_out[i1] (KF1->n ints) = feature of key
 * frame 2 whose map point the reference stores in vpMatches12[i1], or -1; *n_found = the return value.
 * HOST pointers. */
int orbfe_search_by_sim3(orbfe_handle *h, const orbfe_frame_view *KF1, const orbfe_frame_view *KF2,
                         const orbfe_sim3_view *dir12, const orbfe_sim3_view *dir21, const orbfe_world_point *mp1,
                         const uint8_t *mp_desc1, const orbfe_world_point *mp2, const uint8_t *mp_desc2, float th,
                         int *match12_out, int *n_found);

/* replaces ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, checkOrientation)
 * (src/ORBmatcher.cc:1202-1326, the relocalisation overload; no caller in this fork).  points / mp_desc / kf_angle:
 * one record per feature i of the key frame (skip = "no map point" or "in sAlreadyFound"; kf_angle[i] =
 * pKF->mvKeysUn[i].angle, may be NULL when check_orientation == 0); frustum = the current frame's pose, bounds,
 * camera and scale pyramid; frame_has_mp[i2] != 0 iff CurrentFrame->mvpMapPoints[i2] is set on entry (NULL == none).
 * match_out[i2] (frame->n ints) = key-frame feature whose map point this call leaves in
 * CurrentFrame->mvpMapPoints[i2], or -1; *n_matches = the return value.  The greedy order-dependent claims and the
 * rotation-histogram filter are reproduced exactly.  HOST pointers. */
int orbfe_match_projection_keyframe(orbfe_handle *h, const orbfe_frame_view *frame, const orbfe_frustum *frustum,
                                    int n_points, const orbfe_world_point *points, const uint8_t *mp_desc,
                                    const float *kf_angle, const uint8_t *frame_has_mp, float th,
                                    int check_orientation, int *match_out, int *n_matches);

/* replaces the selection loop of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:343-416; called after every
 * AddObservation / Fuse, src/LocalMapping.cc) for a batch of map points: set s holds the observed descriptors
 * desc[set_off[s] .. set_off[s+1]) (32 bytes each, in the order the reference collects them); best_idx_out[s] =
 * index inside the set of the descriptor with the least median distance to the rest (-1 for an empty set, the
 * reference returns early); best_median_out may be NULL.  HOST pointers. */
int orbfe_distinctive_descriptors(orbfe_handle *h, int n_sets, const int *set_off, const uint8_t *desc,
                                  int *best_idx_out, int *best_median_out);

/* -------------------------------------------------------------------------------------------
 * Node-side image preparation (honourable mention): undistort + resize + grey
 * ---------------------------------------------------------------------------------------- */
typedef struct orbfe_prep orbfe_prep;

/* Uploads the undistortion maps the node builds with cv::fisheye::initUndistortRectifyMap(..., CV_32F, map1, map2)
 * (ros2_ws/src/mono-inertial/src/mono_inertial_node.cpp:61-71): map1 / map2 hold src_h x src_w floats (x and y source
 * coordinates per undistorted pixel, row-major, no padding).  dst_w x dst_h is the size ImageGrabber resizes to
 * (m_width x m_height, image_grabber.hpp:102). */
int orbfe_prep_create(orbfe_handle *h, int src_w, int src_h, const float *map1, const float *map2, int dst_w,
                      int dst_h, orbfe_prep **out);
void orbfe_prep_destroy(orbfe_prep *p);

/* replaces ImageGrabber::ConvertImageToGPU (ros2_ws/src/mono-inertial/include/image_grabber.hpp:96-110):
 * cv::cuda::remap(INTER_CUBIC, BORDER_CONSTANT 0) + cv::cuda::resize(INTER_LINEAR) + cv::cuda::cvtColor(BGR2GRAY) in
 * one kernel.  bgr: src_h rows of src_w BGR pixels (3 bytes each), `pitch` bytes per row, HOST pointer (pinned buffers
 * are read by the DMA engine directly); gray_out: dst_h rows of dst_w bytes, HOST pointer.  Arithmetic: SPEC DECISION S9
 *  -- parity against OpenCV-CUDA is unpinned (third-party arithmetic, absent here). */
int orbfe_prepare_image(orbfe_handle *h, orbfe_prep *p, const uint8_t *bgr, int pitch, uint8_t *gray_out,
                        int gray_pitch);
/* Same with DEVICE pointers, asynchronous on `stream` (NULL == the handle's stream). */
int orbfe_prepare_image_device(orbfe_handle *h, orbfe_prep *p, const uint8_t *d_bgr, int pitch, uint8_t *d_gray,
                               int gray_pitch, void *stream);
/* ConvertImageToGPU followed by ORBextractor::extractFeatures (what the node and Frame::ExtractORB do back to back,
 * image_grabber.hpp:160 -> src/Frame.cc:178-189) without the grey image leaving the device: the prepared frame is
 * written straight into the extractor's level-0 rows.  The handle must have been created for dst_w x dst_h images.
 * gray_out (optional, may be NULL) receives the grey frame as well (the tracker keeps it for the viewer). */
int orbfe_prepare_and_extract(orbfe_handle *h, orbfe_prep *p, const uint8_t *bgr, int pitch, orbfe_keypoint *kp_out,
                              uint8_t *desc_out, int *n_out, int *per_level, uint8_t *gray_out, int gray_pitch);

/* -------------------------------------------------------------------------------------------
 * Vocabulary tree: the per-feature part of Frame::ComputeBoW
 * ---------------------------------------------------------------------------------------- */
typedef struct orbfe_vocab orbfe_vocab;

/* Uploads a DBoW2 vocabulary tree (TemplatedVocabulary::m_nodes,
 * Thirdparty/DBoW2/include/DBoW2/TemplatedVocabulary.h): node 0 is the root, child_idx[child_off[i] ..
 * child_off[i+1]) are the children of node i in DBoW2 order (a node without children is a leaf),
 * node_desc n_nodes x 32 bytes, word_id / weight per node (read at leaves), L = m_L. */
int orbfe_vocab_create(orbfe_handle *h, int n_nodes, const int *child_off, const int *child_idx,
                       const uint8_t *node_desc, const int *word_id, const double *weight, int L,
                       orbfe_vocab **out);
void orbfe_vocab_destroy(orbfe_vocab *v);
/* replaces TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (:1227-1270) for n
 * descriptors at once (HOST pointers): per feature the word id, its weight and the id of the node at
 * level L - levelsup.  The adaptor assembles BowVector / FeatureVector from these (:1136-1204). */
int orbfe_bow_transform(orbfe_handle *h, orbfe_vocab *v, const uint8_t *desc, int n, int levelsup,
                        int *word_id_out, int *node_id_out, double *weight_out);

/* -------------------------------------------------------------------------------------------
 * The tracking thread's chain of a frame tracked against its reference key frame, as ONE submission
 * ---------------------------------------------------------------------------------------- */
/* replaces, for one frame (Tracking::TrackReferenceKeyFrame, src/Tracking.cc:825-835 -- every frame while the map's IMU
 * is not initialised, :454-458):
 *   Frame::Frame -> ExtractORB -> ORBextractor::extractFeatures                    (src/Frame.cc:178-189)
 *   mCurrentFrame->ComputeBoW(): TemplatedVocabulary::transform per feature        (src/Frame.cc:483-495)
 *   ORBmatcher::SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches, nnRatio, true)   (src/ORBmatcher.cc:133-327)
 * gray / pitch / kp_out / desc_out / n_out / per_level_counts as orbfe_extract.  word_id_out / node_id_out / weight_out
 * (capacity orbfe_max_keypoints(); weight_out may be NULL) as orbfe_bow_transform on the frame's descriptors: the caller
 * assembles mBowVec / mFeatVec from them.  kf: the reference key frame, resident (orbfe_keyframe_create, whose node_id
 * came from the same vocabulary and levelsup); kf_has_mp[j] != 0 iff key-frame feature j has a map point that is not bad
 * as of this call (:182-187), orbfe_keyframe_size(kf) entries.  match_out[i] (capacity orbfe_max_keypoints()) = the
 * key-frame feature whose map point is written to vpMapPointMatches[i], or -1; n_matches = the return value.
 * The frame's descriptors never leave the device between extraction, descent and matching; nothing is decided on the
 * host in between.  A frame feature whose word has weight 0 (a stopped word) is in no node of mFeatVec
 * (TemplatedVocabulary.h:1168-1172,1196-1200) and takes no part in the matching, although its word_id_out / node_id_out /
 * weight_out (== 0) are still returned.  Results are byte-identical to orbfe_extract -> orbfe_bow_transform ->
 * orbfe_match_bow with the FeatureVectors of both sides (features with weight > 0 only), at every extractor configuration
 * orbfe_track_frame accepts (per-frame keypoint capacity below 2^20): frames of up to 7168 keypoints are matched from LDS,
 * larger ones from per-node lists built in device memory, in the same graph.  HOST pointers; gray may be pinned (read in
 * place) or pageable. */
int orbfe_track_reference_keyframe(orbfe_handle *h, const uint8_t *gray, int pitch, const orbfe_vocab *vocab, int levelsup,
                                   const orbfe_keyframe *kf, const uint8_t *kf_has_mp, float nn_ratio,
                                   int check_orientation, orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out,
                                   int *per_level_counts, int *word_id_out, int *node_id_out, double *weight_out,
                                   int *match_out, int *n_matches);

/* -------------------------------------------------------------------------------------------
 * The tracking thread's chain of a frame during monocular initialisation, as ONE submission
 * ---------------------------------------------------------------------------------------- */
typedef struct orbfe_init_frame orbfe_init_frame;

/* mInitialFrame of Tracking::MonocularInitialization (src/Tracking.cc:569-586: the first frame with more than FEAT_INIT_COUNT
 * keypoints becomes the reference every following frame is matched against until the map is initialised or the attempt is
 * reset, :588-602), resident in HBM: its mvKeysUn (n keypoints) and mDescriptors (n x 32).  HOST pointers; one upload.
 * The frame stays on the device until orbfe_init_frame_destroy (which waits for the device). */
int orbfe_init_frame_create(orbfe_handle *h, int n, const orbfe_keypoint *kp, const uint8_t *desc, orbfe_init_frame **out);
void orbfe_init_frame_destroy(orbfe_init_frame *f);
int orbfe_init_frame_size(const orbfe_init_frame *f);

/* replaces, for one frame while the map is being initialised (Tracking::MonocularInitialization, src/Tracking.cc:566-607):
 *   Frame::Frame -> ExtractORB -> ORBextractor::extractFeatures                                          (src/Frame.cc:178-189)
 *   ORBmatcher::SearchForInitialization(mInitialFrame, mCurrentFrame, windowSize, nnRatio, true)         (src/ORBmatcher.cc:329-439;
 *                                                                                          the call: src/Tracking.cc:603-607, 40 / 0.45)
 * gray / pitch / kp_out / desc_out / n_out / per_level_counts as orbfe_extract; tp: the CURRENT frame's grid statics
 * (GetFeaturesInArea runs on frame 2; th / nn_ratio / far_points of the block are not read); matches12_out
 * (orbfe_init_frame_size(f1) ints) = vnMatches12 (index in the current frame or -1), *n_matches = the function's return value.
 * The thresholds around the call (FEAT_INIT_COUNT, the 2 s time-out, :579,:588-598) stay with the caller.
 * One captured hipGraph per (initial frame, input pitch, parameters): extraction kernels, the matcher's kernels on the fresh
 * keypoints, ONE result block back, one synchronisation.  Byte-identical to orbfe_extract followed by
 * orbfe_match_initialization(f1, current frame).  HOST pointers; gray may be pinned (read in place) or pageable. */
int orbfe_track_initialization(orbfe_handle *h, const uint8_t *gray, int pitch, const orbfe_init_frame *f1,
                               const orbfe_track_params *tp, int window_size, float nn_ratio, int check_orientation,
                               orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out, int *per_level_counts,
                               int *matches12_out, int *n_matches);

/* -------------------------------------------------------------------------------------------
 * Two-view reconstruction: the line behind orbfe_track_initialization while the map is being initialised
 * ---------------------------------------------------------------------------------------- */
/* TwoViewReconstruction's constructor arguments and the two constants of Reconstruct (src/TwoViewReconstruction.cc:31-38,
 * :113,:120,:125); versioned by struct_size like orbfe_tri_params */
typedef struct orbfe_two_view_params {
    int struct_size;          /* sizeof(orbfe_two_view_params) at the caller's compile time */
    float fx, fy, cx, cy;     /* mK of the pinhole camera (src/CameraModels/Pinhole.cpp:81-88) */
    float sigma;              /* mSigma: 1.0 at both call sites */
    int iterations;           /* mMaxIterations: 200 at both call sites; [1, 4096] */
    float min_parallax_deg;   /* minParallax, :113: only 1.0 is built (the decision is a cosine comparison, S12) */
    int min_triangulated;     /* 50, :120,:125 */
} orbfe_two_view_params;
#define ORBFE_TWO_VIEW_PARAMS_INIT {(int)sizeof(orbfe_two_view_params), 0.f, 0.f, 0.f, 0.f, 1.0f, 200, 1.0f, 50}

#define ORBFE_TWO_VIEW_MODEL_NONE        0  /* fewer than 8 matches, or SH + SF == 0 (:110) */
#define ORBFE_TWO_VIEW_MODEL_HOMOGRAPHY  1  /* RH > 0.40: ReconstructH (:583-747) */
#define ORBFE_TWO_VIEW_MODEL_FUNDAMENTAL 2  /* ReconstructF (:473-581) */

/* every intermediate of one call (optional: info may be NULL).  struct_size as above; the pointer members are caller-owned
 * buffers, each may be NULL.  N = n_matches = the number of i with matches12[i] >= 0; match m is the m-th such i. */
typedef struct orbfe_two_view_info {
    int struct_size;          /* sizeof(orbfe_two_view_info) at the caller's compile time */
    int n_matches;            /* N (mvMatches12.size(), :62) */
    float SH, SF, RH;         /* :98,:111 (RH = 0 when SH + SF == 0) */
    int model;                /* ORBFE_TWO_VIEW_MODEL_* */
    int exit_line;            /* 0 = reconstructed; else the reference line of the `return false` taken (110, 528, 580, 609,
                                 746), or 62 for fewer than 8 matches */
    float H21[9], F21[9];     /* best models, row-major (zeros when no hypothesis scored above 0) */
    int best_it_H, best_it_F; /* their RANSAC iteration, -1 when none */
    int n_hypotheses;         /* motion hypotheses checked: 0, 4 (F) or 8 (H) */
    int best_hypothesis;      /* the one returned, -1 when not reconstructed */
    int n_good[8];            /* CheckRT's return value per hypothesis (:498-501, :719) */
    float cos_parallax[8];    /* cosine at rank min(50, nGood - 1) of the survivors' ascending cosines (:905-908); 1 when nGood == 0 */
    float hyp_R[8][9];        /* the motion hypotheses, R row-major (:498-501 order; :632-702 order) */
    float hyp_t[8][3];
    float *scores;            /* [2 * iterations]: currentScore of every H iteration, then of every F iteration */
    uint8_t *inliers_H;       /* [N] vbMatchesInliersH */
    uint8_t *inliers_F;       /* [N] vbMatchesInliersF */
    uint8_t *rt_flags;        /* [8][N]: bit 0 = counted in nGood, bit 1 = vbGood (cosParallax < 0.99998) */
    float *rt_x3d;            /* [8][N][3]: p3dC1 of the counted matches, zeros elsewhere */
    float *rt_cos;            /* [8][N]: cosParallax of the counted matches, zeros elsewhere */
} orbfe_two_view_info;

/* replaces TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:40-127; the call: src/Tracking.cc:616 ->
 * Pinhole::ReconstructWithTwoViews, src/CameraModels/Pinhole.cpp:81-88) for a pinhole K:
 *   Normalize (:750-797)                                   on the host, inside the call
 *   FindHomography / FindFundamental (:129-228): ComputeH21 / ComputeF21 (:230-306) and CheckHomography / CheckFundamental
 *   (:308-471) for all 2 x iterations hypotheses           one launch, one wave per hypothesis; a second picks the two winners
 *   ReconstructH / ReconstructF up to the hypotheses (:473-501, :583-702), DecomposeE (:916-940)       on the host
 *   CheckRT (:799-914) for the 4 or 8 motion hypotheses    one launch
 *   the selection rules (:503-580, :705-746)               on the host
 * Numerics: SPEC DECISION S12.  kp1 / kp2 = mvKeysUn of the reference and of the current frame,
 * matches12 (n1 ints) = vnMatches12 as orbfe_track_initialization returns it.  sets = iterations x 8 indices into the MATCH
 * list (mvSets, :75-94): an input, because the reference draws them from a rand() stream that belongs to the process
 * (Thirdparty/DBoW2/src/DUtils/Random.cpp:38-50; include/orbfe_adaptor.hpp draws them as the reference does).
 * *reconstructed = the function's return value; R21 (9, row-major) / t21 (3) = T21; p3d (n1 x 3) = vP3D and triangulated (n1)
 * = vbTriangulated, indexed by the keypoint of frame 1; all zeros when not reconstructed.
 * Fewer than 8 matches: *reconstructed = 0, ORBFE_OK, no GPU work (the reference indexes an empty vector there).
 * ORBFE_ERR_INVALID_ARG: a set index outside the match list or repeated inside a set, a match index outside frame 2,
 * iterations outside [1, 4096], min_parallax_deg != 1.0, a wrong struct_size (params or info).
 * KannalaBrandt8::ReconstructWithTwoViews undistorts with OpenCV first: its caller passes the undistorted points and K.
 * HOST pointers.  Two submissions and two synchronisations per call (the decompositions run between them). */
int orbfe_two_view_reconstruct(orbfe_handle *h, const orbfe_two_view_params *p, int n1, const orbfe_keypoint *kp1, int n2,
                               const orbfe_keypoint *kp2, const int *matches12, const int *sets, int *reconstructed,
                               float *R21, float *t21, float *p3d, uint8_t *triangulated, orbfe_two_view_info *info);

/* -------------------------------------------------------------------------------------------
 * MLPnP RANSAC pose: the line behind orbfe_track_reference_keyframe in Tracking::TrackReferenceKeyFrame
 * ---------------------------------------------------------------------------------------- */
/* the frame's camera (F->mpCamera) and the arguments of MLPnPsolver::SetRansacParameters (src/MLPnPsolver.cpp:224-259; the call
 * site passes 0.95, 50, 300, 12, 0.5, 5.991: src/Tracking.cc:840) plus iterate's nIterations (20, :845); versioned by struct_size */
typedef struct orbfe_mlpnp_params {
    int struct_size;          /* sizeof(orbfe_mlpnp_params) at the caller's compile time */
    int camera_model;         /* ORBFE_CAMERA_PINHOLE or ORBFE_CAMERA_KANNALA_BRANDT8 */
    float cam[8];             /* fx fy cx cy k1 k2 k3 k4 (mvParameters; k1 .. k4 are not read for a pinhole) */
    float kb_precision;       /* KannalaBrandt8::precision (1e-6), the Newton exit of unproject */
    double probability;       /* (0, 1) */
    int min_inliers;          /* >= 0 */
    int max_iterations;       /* [1, 4096] */
    int min_set;              /* [6, 64] */
    float epsilon;            /* (0, 1] */
    float th2;
    int n_iterations;         /* nIterations of iterate(): [0, 4096] */
} orbfe_mlpnp_params;
#define ORBFE_MLPNP_PARAMS_INIT {(int)sizeof(orbfe_mlpnp_params), 0, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 1e-6f, 0.95, 50, 300, 12, 0.5f, 5.991f, 20}

#define ORBFE_MLPNP_EXIT_ABORT          0  /* N < mRansacMinInliers (:106-111): no GPU work */
#define ORBFE_MLPNP_EXIT_REFINED        1  /* a Refine ended with more than mRansacMinInliers inliers (:189-200); the refined pose is returned */
#define ORBFE_MLPNP_EXIT_BEST_UNREFINED 2  /* no Refine succeeded, the last best hypothesis is returned as it is (:204-219) */
#define ORBFE_MLPNP_EXIT_FAILED         3  /* no hypothesis reached mRansacMinInliers */

/* every intermediate of one call (optional: info may be NULL).  struct_size as above; the pointer members are caller-owned
 * buffers, each may be NULL.  N = the number of i with mp_index[i] >= 0; correspondence c is the c-th such i.  T =
 * total_iterations.  A pose is R (9, row-major) then t (3) in binary64, as computePose leaves it in mRi / mti. */
typedef struct orbfe_mlpnp_info {
    int struct_size;          /* sizeof(orbfe_mlpnp_info) at the caller's compile time */
    int N;
    int min_inliers, max_its, total_iterations;   /* as orbfe_mlpnp_plan */
    int exit_kind;            /* ORBFE_MLPNP_EXIT_* */
    int returning_iteration;  /* the hypothesis whose (refined) pose is returned, -1 when none */
    int n_candidates;         /* hypotheses that set a new strict best among those with >= min_inliers inliers, in iteration order */
    double *hyp_Rt;           /* [T][12] */
    int *hyp_inliers;         /* [T] mnInliersi */
    uint8_t *hyp_planar;      /* [T] 1 = the planar branch of computePose (:388) */
    int *hyp_gn_evals;        /* [T] passes of mlpnp_gn's loop (:723) */
    int *hyp_gn_exit;         /* [T] 0 = it_cnt reached maxIt, 1 = the break of :743, 2 = the break of :747 */
    int *candidates;          /* [T] capacity, n_candidates written: their iterations */
    double *cand_Rt;          /* [T][12] capacity: the pose Refine's computePose leaves in `result` (:327) for each candidate */
    int *cand_inliers;        /* [T] capacity: the inliers of cand_Rt (mnRefinedInliers, had :330 scored `result`) */
    uint8_t *cand_planar;     /* [T] capacity */
    uint8_t *cand_mask;       /* [T][N] capacity: the inlier flags of cand_Rt per candidate */
} orbfe_mlpnp_info;

/* host only, no handle: SetRansacParameters' adjusted values for N correspondences -- *min_inliers = mRansacMinInliers, *max_its =
 * mRansacMaxIts -- and *total_iterations = the passes the loop of a fresh solver's first iterate(n_iterations) makes when no Refine
 * succeeds: max(mRansacMaxIts, n_iterations), or 0 (and *max_its = 0) when N < mRansacMinInliers.  binary64 with the platform's
 * log / pow / ceil.  The caller draws total_iterations min-sets. */
int orbfe_mlpnp_plan(const orbfe_mlpnp_params *p, int N, int *min_inliers, int *max_its, int *total_iterations);

/* replaces a fresh MLPnPsolver(F, vpMapPointMatches) + SetRansacParameters + one iterate(n_iterations, bNoMore, vbInliers, nInliers,
 * Tcw) (src/MLPnPsolver.cpp:56-352; the call: src/Tracking.cc:838-845).  Numerics: SPEC DECISION S13.
 * kp (n) = mvKeysUn of the frame (x, y and octave are read; the handle's mvLevelSigma2 gives sigma2); mp_index[i] = the row of
 * `points` that holds the world position (x y z floats, n_points rows) of the non-bad map point matched to keypoint i, or -1.
 * sets = n_sets x min_set indices into the CORRESPONDENCE list (:121-141): an input, because the reference draws them from a
 * rand() stream that belongs to the process (include/orbfe_adaptor.hpp draws them as the reference does); n_sets must equal
 * orbfe_mlpnp_plan's total_iterations for N.  *solved = the function's return value, Tcw (16, row-major; identity when not solved),
 * inliers (n, by keypoint), *n_inliers, *no_more = bNoMore.  N < min_inliers: *solved = 0, *no_more = 1, ORBFE_OK, no GPU work,
 * sets not read.  ORBFE_ERR_INVALID_ARG: a wrong struct_size (params or info), a parameter outside its range, n_sets != the plan's
 * total, a set index outside [0, N) or repeated inside a set, an mp_index >= n_points, an octave outside the handle's levels,
 * n > 65536.  HOST pointers.  One submission and one synchronisation per call.
 * NOT the reference's function in one respect ("Refine returns what it computes"): the reference's Refine never
 * copies its computePose result into mRi / mti (:323-335), so its CheckInliers re-scores the hypothesis and iterate returns the
 * first hypothesis with more than mRansacMinInliers inliers, unrefined.  This call adopts the refinement: with
 * ORBFE_MLPNP_EXIT_REFINED, Tcw / inliers / n_inliers are the refined pose's, and the returning iteration is the first strict-best
 * hypothesis whose REFINED pose has more than mRansacMinInliers inliers.  They differ from the reference's even in exact arithmetic;
 * the reference's own choice can be read from info (the first it with hyp_inliers[it] > min_inliers, pose hyp_Rt[it]). */
int orbfe_mlpnp_ransac(orbfe_handle *h, const orbfe_mlpnp_params *p, int n, const orbfe_keypoint *kp, const int *mp_index,
                       int n_points, const float *points, const int *sets, int n_sets, int *solved, float *Tcw,
                       uint8_t *inliers, int *n_inliers, int *no_more, orbfe_mlpnp_info *info);

/* -------------------------------------------------------------------------------------------
 * Motion-only pose optimisation: the line behind orbfe_mlpnp_ransac (src/Tracking.cc:869) and behind orbfe_track_frame
 * (src/Tracking.cc:935)
 * ---------------------------------------------------------------------------------------- */
/* the frame's camera and the constants of Optimizer::PoseOptimization (src/Optimizer.cc:765-1067); versioned by struct_size */
typedef struct orbfe_pose_opt_params {
    int struct_size;          /* sizeof(orbfe_pose_opt_params) at the caller's compile time */
    int camera_model;         /* ORBFE_CAMERA_PINHOLE; ORBFE_CAMERA_KANNALA_BRANDT8 -> ORBFE_ERR_UNSUPPORTED */
    float cam[8];             /* fx fy cx cy k1 k2 k3 k4 (mvParameters; only the first four are read) */
    float chi2_threshold;     /* chi2Mono[it] (:953), 5.991 in every round */
    double huber_delta2;      /* deltaMono = (float) sqrt(7.815) (:805): > 0 */
    int iterations;           /* its[it] (:956), 25 in every round: [1, 64] */
    int rounds;               /* 4 (:959): [1, 4]; the Huber kernel is dropped after round index 2 as written (:993) */
    int stereo;               /* 0; anything else (mvuRight >= 0, a second camera, the ToBody edges) -> ORBFE_ERR_UNSUPPORTED */
} orbfe_pose_opt_params;
#define ORBFE_POSE_OPT_PARAMS_INIT {(int)sizeof(orbfe_pose_opt_params), 0, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 5.991f, 7.815, 25, 4, 0}

#define ORBFE_POSE_OPT_EXIT_RAN_ALL  0  /* the round ran all its iterations */
#define ORBFE_POSE_OPT_EXIT_TRIALS   1  /* Terminate: 10 trials in one iteration */
#define ORBFE_POSE_OPT_EXIT_RHO_ZERO 2  /* Terminate: rho == 0 */

/* every intermediate of one orbfe_pose_optimization call (optional: info may be NULL).  Edge c is the c-th keypoint i with
 * mp_index[i] >= 0; a pose is R (9, row-major) then t (3) in binary64.  Entries of rounds that did not run are zero. */
typedef struct orbfe_pose_opt_info {
    int struct_size;          /* sizeof(orbfe_pose_opt_info) at the caller's compile time */
    int N_e;
    int rounds_run;
    int iterations[4];        /* Levenberg iterations started in the round */
    int trials[4];            /* damped solves tried in the round */
    int n_bad[4];             /* nBad after the round */
    int exit_kind[4];         /* ORBFE_POSE_OPT_EXIT_* */
    double pose[4][12];       /* the round's final pose */
    double lambda[4];         /* the damping the round ended with */
    double chi2[4];           /* the round's last accepted sum of rho0 (activeRobustChi2) */
    uint8_t *outlier;         /* [4][N_e], caller-owned, may be NULL: the flags after each round, by edge */
} orbfe_pose_opt_info;

/* replaces Optimizer::PoseOptimization(pFrame) (src/Optimizer.cc:765-1067; the calls: src/Tracking.cc:869 and :935) for the branch
 * this fork takes: one camera, mvuRight < 0, EdgeSE3ProjectXYZOnlyPose, pinhole.  Numerics: SPEC DECISION S14;
 * tests/poseopt_ref.py is the normative restatement and the call equals it byte for byte.
 * kp (n) = mvKeysUn (x, y, octave are read; the handle's mvInvLevelSigma2 is the information); mp_index[i] = the row of `points`
 * (x y z floats, n_points rows) of the map point matched to keypoint i, or -1.  Rcw (9, row-major) / tcw (3) = pFrame->GetPose().
 * Tcw_out (16, row-major) = the pose the reference hands to SetPose; outlier_out (n) = mvbOutlier; *n_inliers = the return value
 * (nInitialCorrespondences - nBad).  Fewer than 3 matched keypoints: *n_inliers = 0, Tcw_out = the input pose, no flags, ORBFE_OK
 * (:949); that return and every refusal below are decided from the arguments and the handle's level count before the device is touched.  Fewer than 10: one round (:1055).
 * The whole call -- four rounds, every iteration and every trial -- is ONE kernel launch of one block; one submission, one
 * synchronisation.  HOST pointers.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size (params or info), a parameter outside its range, an mp_index >= n_points, an octave
 * of a matched keypoint outside the handle's levels, n > 65536.  ORBFE_ERR_UNSUPPORTED: KannalaBrandt8 (its project() mixes
 * atan2f / sqrtf with binary64 while projectJac uses atan2: a binary64 atan2 sequence has to be pinned first), stereo != 0,
 * Of the inertial variants, PoseInertialOptimizationLastKeyFrame is orbfe_pose_inertial_optimization_last_keyframe below (S19);
 * PoseInertialOptimizationLastFrame is orbfe_pose_inertial_optimization_last_frame (S20).
 * NOT the reference's function in three stated respects:
 *   - g2o is an empty submodule in the reference tree: the Levenberg loop (OptimizationAlgorithmLevenberg + LinearSolverDense)
 *     and SE3Quat::exp are restated from the published algorithm and adopted as this project's definition; parity with a g2o
 *     build is unpinned, as S10-S13 are against Eigen;
 *   - the pose is kept as a rotation matrix where g2o keeps a quaternion, and the initial pose takes no quaternion round trip
 *     (:784); the matrix drifts from orthonormal by rounding only (measured: tests/test_poseopt.py);
 *   - the inlier flags are scored on fresh errors at the round's final pose; g2o leaves the errors of a rejected last trial in
 *     the active edges when a round ends on Terminate, and the reference reads those. */
int orbfe_pose_optimization(orbfe_handle *h, const orbfe_pose_opt_params *p, int n, const orbfe_keypoint *kp, const int *mp_index,
                            int n_points, const float *points, const float *Rcw, const float *tcw, float *Tcw_out,
                            uint8_t *outlier_out, int *n_inliers, orbfe_pose_opt_info *info);

/* Batched, HBM-resident form (no reference analogue: the batched mode's pose step): grid = batch, one block per frame.  Frame b's
 * keypoints d_kp[b * kp_stride ..] and count d_n[b] are orbfe_extract_batch_device's outputs (kp_stride <= 65536), d_match[b *
 * kp_stride ..] is orbfe_match_projection_batch_device's d_match_out (an index into frame b's points, or -1), frame b's points
 * are d_points[b * point_stride_frames ..] (n_map_points records; point_stride_frames == 0: one set shared by all frames; only
 * x y z are read).  d_pose_in / d_pose_out: 12 floats per frame, Rcw then tcw.  d_outlier: kp_stride bytes per frame, d_n[b] are
 * written.  d_n_inliers: one int per frame.  A match outside [0, n_map_points) or on a keypoint whose octave is outside the handle's
 * levels is no edge (the host call refuses such input; a device call cannot).  DEVICE pointers; asynchronous on `stream` (NULL ==
 * the handle's stream): one launch, no host synchronisation.  Frame b's results are byte-equal to orbfe_pose_optimization on the
 * same data. */
int orbfe_pose_optimization_batch_device(orbfe_handle *h, const orbfe_pose_opt_params *p, int batch, const orbfe_keypoint *d_kp,
                                         const int *d_n, int kp_stride, const int *d_match, int n_map_points,
                                         const orbfe_world_point *d_points, int point_stride_frames, const float *d_pose_in,
                                         float *d_pose_out, uint8_t *d_outlier, int *d_n_inliers, void *stream);

/* -------------------------------------------------------------------------------------------
 * Inertial pose optimisation against the last key frame: the line behind orbfe_track_frame once the IMU is initialised
 * (src/Tracking.cc:952)
 * ---------------------------------------------------------------------------------------- */
/* the frame's camera and the constants of Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:3447-3844); versioned
 * by struct_size */
typedef struct orbfe_pose_inertial_params {
    int struct_size;          /* sizeof(orbfe_pose_inertial_params) at the caller's compile time */
    int camera_model;         /* ORBFE_CAMERA_PINHOLE; ORBFE_CAMERA_KANNALA_BRANDT8 -> ORBFE_ERR_UNSUPPORTED */
    float cam[8];             /* fx fy cx cy k1 k2 k3 k4 (mvParameters; only the first four are read) */
    float chi2[4];            /* chi2Mono[it] (:3658): 12, 7.5, 5.991, 5.991; each >= 0 */
    double close_factor;      /* chi2close = (float)(1.5 * chi2Mono[it]) (:3686): >= 0 */
    float close_depth;        /* bClose = mTrackDepth < 10.f (:3701) */
    float recover_chi2;       /* chi2MonoOut = 24.f (:3768) */
    int recover_below;        /* the recovery runs when the last round left fewer inliers than this: 30 (:3765) */
    int iterations;           /* its[it] (:3661), 15 in every round: [1, 64] */
    int rounds;               /* 4 (:3669): [1, 4]; the Huber kernel is dropped after round index 2 as written (:3717) */
    int rec_init;             /* bRecInit: != 0 switches the recovery off (:3765) */
    double huber_delta2;      /* thHuberMono = (float) sqrt(5.991) (:3498): > 0 */
    float gravity;            /* IMU::GRAVITY_VALUE (include/ImuTypes.h): g = (0, 0, -gravity) */
    int stereo;               /* 0; anything else (mvuRight >= 0, a second camera, Nleft != -1) -> ORBFE_ERR_UNSUPPORTED */
} orbfe_pose_inertial_params;
#define ORBFE_POSE_INERTIAL_PARAMS_INIT {(int)sizeof(orbfe_pose_inertial_params), 0, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, \
                                         {12.f, 7.5f, 5.991f, 5.991f}, 1.5, 10.f, 24.f, 30, 15, 4, 0, 5.991, 9.81f, 0}

/* What the fixed vertices of the last key frame contribute, and the camera-body extrinsics: written whole by orbfe_imu_predict /
 * orbfe_imu_frame_batch_device with ORBFE_IMU_FROM_KEYFRAME (SPEC DECISION S22), or computed by the caller with the reference's own code.  3 x 3 and 9 x 9 matrices are row-major.  With pInt = pFrame->mpImuPreintegrated, pKF =
 * pFrame->mpLastKeyFrame and b1 = pKF's bias: dR / dV / dP = pInt->GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition(b1),
 * dt = pInt->dT, info9 = EdgeInertial(pInt).information() (the inverse of C.block<9,9>(0,0), symmetrised, eigenvalues below 1e-12
 * clamped to 0: src/G2oTypes.cc:500-508), infoG / infoA = C.block<3,3>(9,9) / (12,12) .cast<double>().inverse() (:3645,:3652). */
typedef struct orbfe_imu_link {
    int struct_size;          /* sizeof(orbfe_imu_link) at the caller's compile time */
    int reserved;             /* 0 */
    float Rwb1[9], twb1[3];   /* pKF->GetImuRotation(), GetImuPosition() */
    float v1[3];              /* pKF->GetVelocity() */
    float bg1[3], ba1[3];     /* pKF->GetGyroBias(), GetAccBias() */
    float dR[9], dV[3], dP[3];
    float dt;
    float Rcb[9], tcb[3];     /* mImuCalib.mTcb */
    float tbc[3];             /* mImuCalib.mTbc.translation() */
    double info9[81];
    double infoG[9], infoA[9];
} orbfe_imu_link;

/* every intermediate of one orbfe_pose_inertial_optimization_last_keyframe call (optional: info may be NULL).  Edge c is the c-th
 * keypoint i with mp_index[i] >= 0; a state is Rwb (9, row-major), twb, v, bg, ba in binary64.  Entries of rounds that did not run
 * are zero. */
typedef struct orbfe_pose_inertial_info {
    int struct_size;          /* sizeof(orbfe_pose_inertial_info) at the caller's compile time */
    int N_e;
    int rounds_run;
    int recovered;            /* 1: the recovery (:3765-3792) ran */
    int iterations[4];        /* Gauss-Newton iterations started in the round */
    int ok[4];                /* 0: the round ended on a solve whose pivots were not all positive (the state of before it is kept) */
    int n_bad[4];             /* nBad after the round */
    double state[4][21];      /* the round's final state */
    uint8_t *outlier;         /* [4][N_e], caller-owned, may be NULL: the flags after each round, by edge */
} orbfe_pose_inertial_info;

/* replaces Optimizer::PoseInertialOptimizationLastKeyFrame(pFrame, bRecInit) (src/Optimizer.cc:3447-3844; the call:
 * src/Tracking.cc:952) for the branch this fork takes: one pinhole camera, EdgeMonoOnlyPose edges, one EdgeInertial, EdgeGyroRW,
 * EdgeAccRW; 15 unknowns (pose rotation, pose translation, velocity, gyro bias, accelerometer bias).  Numerics: SPEC DECISION S19
 * (DESIGN.md section 2); tests/pose_inertial_ref.py is the normative restatement and the call equals it byte for byte.
 * kp (n) = mvKeysUn (x, y, octave are read; the handle's mvInvLevelSigma2 is the information); mp_index[i] = the row of `points`
 * (x y z floats, n_points rows) and of track_depth (mTrackDepth, n_points floats) of the map point matched to keypoint i, or -1.
 * Rcw (9) / tcw (3) = pFrame->GetPose(); Rwb / twb / v = GetImuRotation / GetImuPosition / GetVelocity; bg / ba = mImuBias.
 * Rwb_out .. ba_out: what the reference hands to SetImuPoseVelocity and mImuBias, as floats; H_out (225 doubles, row-major) = the
 * H it hands to new ConstraintPoseImu(..., H), raw: the eigenvalue clamp of that constructor stays with the caller.  outlier_out
 * (n) = mvbOutlier; *n_inliers = the return value (nInitialCorrespondences - nBad).  No matched keypoint at all is valid: the
 * inertial edges alone give a full-rank system (the reference has no early return).
 * The whole call -- four rounds, every iteration, the scoring, the recovery and the Hessian -- is ONE kernel launch of one block;
 * one submission, one synchronisation.  HOST pointers.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size (params, link or info), a parameter outside its range, an mp_index >= n_points, an
 * octave of a matched keypoint outside the handle's levels, n > 65536; decided from the arguments and the handle's level count
 * before the device is touched.  ORBFE_ERR_UNSUPPORTED: KannalaBrandt8 (S14's reason), stereo != 0.
 * PoseInertialOptimizationLastFrame (src/Tracking.cc:946) -- 30 unknowns, the EdgePriorPoseImu prior and Optimizer::Marginalize --
 * is orbfe_pose_inertial_optimization_last_frame below (S20); H_out is the 15 x 15 Hessian its first prior is made from.
 * NOT the reference's function in these stated respects:
 *   - g2o is an empty submodule in the reference tree: OptimizationAlgorithmGaussNewton + LinearSolverDense are restated from the
 *     published algorithm; parity with a g2o build is unpinned, as in S14 and S17;
 *   - NormalizeRotation (an SVD, in ExpSO3 and in every third Update) is not applied: Rwb drifts from orthonormal by rounding
 *     only (measured: tests/test_pose_inertial.py);
 *   - the flags are scored on fresh errors at the round's final state; g2o's active edges hold the errors of before the last update;
 *   - the input state takes no quaternion or Sophus round trip. */
int orbfe_pose_inertial_optimization_last_keyframe(orbfe_handle *h, const orbfe_pose_inertial_params *p, const orbfe_imu_link *link,
                                                   int n, const orbfe_keypoint *kp, const int *mp_index, int n_points,
                                                   const float *points, const float *track_depth, const float *Rcw, const float *tcw,
                                                   const float *Rwb, const float *twb, const float *v, const float *bg, const float *ba,
                                                   float *Rwb_out, float *twb_out, float *v_out, float *bg_out, float *ba_out,
                                                   double *H_out, uint8_t *outlier_out, int *n_inliers,
                                                   orbfe_pose_inertial_info *info);

/* Batched, HBM-resident form: grid = batch, one block per frame, one orbfe_imu_link (d_links[b]) and one state per frame.  Keypoints,
 * counts, matches and points are laid out as for orbfe_pose_optimization_batch_device; d_track_depth holds one float per point
 * record with the same frame stride (d_track_depth[b * point_stride_frames ..]; point_stride_frames == 0: shared).  d_state_in: 33
 * floats per frame -- Rcw (9), tcw (3), Rwb (9), twb, v, bg, ba; d_state_out: 21 floats per frame -- Rwb, twb, v, bg, ba; d_H_out:
 * 225 doubles per frame.  A match outside [0, n_map_points) or on a keypoint whose octave is outside the handle's levels is no edge.
 * DEVICE pointers; asynchronous on `stream` (NULL == the handle's stream): one launch, no host synchronisation.  Frame b's results
 * are byte-equal to orbfe_pose_inertial_optimization_last_keyframe on the same data.  d_links[b].struct_size cannot be checked by
 * a device call. */
int orbfe_pose_inertial_optimization_batch_device(orbfe_handle *h, const orbfe_pose_inertial_params *p, int batch,
                                                  const orbfe_imu_link *d_links, const orbfe_keypoint *d_kp, const int *d_n,
                                                  int kp_stride, const int *d_match, int n_map_points,
                                                  const orbfe_world_point *d_points, int point_stride_frames,
                                                  const float *d_track_depth, const float *d_state_in, float *d_state_out,
                                                  double *d_H_out, uint8_t *d_outlier, int *d_n_inliers, void *stream);

/* -------------------------------------------------------------------------------------------
 * Inertial pose optimisation against the last frame: the commonest tracking call once the IMU is initialised
 * (src/Tracking.cc:946)
 * ---------------------------------------------------------------------------------------- */
/* the frame's camera and the constants of Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:3846-4275); versioned by
 * struct_size */
typedef struct orbfe_pose_inertial_prev_params {
    int struct_size;          /* sizeof(orbfe_pose_inertial_prev_params) at the caller's compile time */
    int camera_model;         /* ORBFE_CAMERA_PINHOLE; ORBFE_CAMERA_KANNALA_BRANDT8 -> ORBFE_ERR_UNSUPPORTED */
    float cam[8];             /* fx fy cx cy k1 k2 k3 k4 (mvParameters; only the first four are read) */
    float chi2[4];            /* chi2Mono[it] (:4075): 5.991 four times; each >= 0 */
    double close_factor;      /* chi2close = (float)(1.5 * chi2Mono[it]) (:4100): >= 0 */
    float close_depth;        /* bClose = mTrackDepth < 10.f (:4107) */
    float recover_chi2;       /* chi2MonoOut = 24.f (:4178) */
    int recover_below;        /* the recovery runs when the last round left fewer inliers than this: 30 (:4175) */
    int iterations;           /* its[it] (:4077), 15 in every round: [1, 64] */
    int rounds;               /* 4 (:4085): [1, 4]; the mono edges' Huber kernel is dropped after round index 2 (:4130) */
    int rec_init;             /* bRecInit: != 0 switches the recovery off (:4175) */
    double huber_delta2;      /* thHuberMono = (float) sqrt(5.991) (:3897): > 0 */
    double prior_huber_delta; /* rkp->setDelta(5) (:4070): > 0; this kernel is never dropped */
    int inlier_threshold;     /* inlierThreshold: accepted = (return value >= inlier_threshold) (:4208); Tracking passes 8 */
    float gravity;            /* IMU::GRAVITY_VALUE (include/ImuTypes.h): g = (0, 0, -gravity) */
    int stereo;               /* 0; anything else (mvuRight >= 0, a second camera, Nleft != -1) -> ORBFE_ERR_UNSUPPORTED */
    int reserved;             /* 0 */
} orbfe_pose_inertial_prev_params;
#define ORBFE_POSE_INERTIAL_PREV_PARAMS_INIT {(int)sizeof(orbfe_pose_inertial_prev_params), 0, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, \
                                              {5.991f, 5.991f, 5.991f, 5.991f}, 1.5, 10.f, 24.f, 30, 15, 4, 0, 5.991, 5.0, 8, 9.81f, 0, 0}

/* The previous frame's state (free here, the start of its four vertices), the preintegration between the two frames at its own
 * bias with the Jacobians that carry it to another bias, and the camera-body extrinsics.  3 x 3 and 9 x 9 matrices are row-major.
 * With pInt = pFrame->mpImuPreintegratedFrame and pFp = pFrame->mpPrevFrame: Rwb1 .. ba1 = pFp's GetImuRotation / GetImuPosition /
 * GetVelocity / mImuBias; dR0 / dV0 / dP0 = pInt->dR / dV / dP; bg0 / ba0 = pInt->b (bwx bwy bwz / bax bay baz); JRg .. JPa and dt =
 * pInt's; info9 = EdgeInertial(pInt).information() (src/G2oTypes.cc:500-508); infoG / infoA = pFrame->mpImuPreintegrated->C
 * .block<3,3>(9,9) / (12,12) .cast<double>().inverse() (:4046, :4053).  orbfe_imu_predict / orbfe_imu_frame_batch_device with
 * ORBFE_IMU_FROM_FRAME write the block whole (SPEC DECISION S22). */
typedef struct orbfe_imu_link_free {
    int struct_size;          /* sizeof(orbfe_imu_link_free) at the caller's compile time */
    int reserved;             /* 0 */
    float Rwb1[9], twb1[3], v1[3], bg1[3], ba1[3];
    float dR0[9], dV0[3], dP0[3];
    float bg0[3], ba0[3];     /* the bias the preintegration was made at */
    float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    float dt;
    float Rcb[9], tcb[3];     /* mImuCalib.mTcb */
    float tbc[3];             /* mImuCalib.mTbc.translation() */
    float reserved2;          /* 0 */
    double info9[81];
    double infoG[9], infoA[9];
} orbfe_imu_link_free;

/* pFp->mpcpi, the prior on the previous frame's state (include/G2oTypes.h ConstraintPoseImu), as it stands -- H after the
 * constructor's eigenvalue clamp; row-major */
typedef struct orbfe_pose_imu_prior {
    int struct_size;          /* sizeof(orbfe_pose_imu_prior) at the caller's compile time */
    int reserved;             /* 0 */
    double Rwb[9], twb[3], vwb[3], bg[3], ba[3];
    double H[225];
} orbfe_pose_imu_prior;

/* every intermediate of one orbfe_pose_inertial_optimization_last_frame call (optional: info may be NULL).  A state is the frame's
 * Rwb (9, row-major), twb, v, bg, ba, then the previous frame's, in binary64.  Entries of rounds that did not run are zero. */
typedef struct orbfe_pose_inertial_prev_info {
    int struct_size;          /* sizeof(orbfe_pose_inertial_prev_info) at the caller's compile time */
    int N_e;
    int rounds_run;
    int recovered;            /* 1: the recovery (:4175-4203) ran */
    int iterations[4];        /* Gauss-Newton iterations started in the round */
    int ok[4];                /* 0: the round ended on a solve whose pivots were not all positive (the state of before it is kept) */
    int n_bad[4];             /* nBad after the round */
    double state[4][42];      /* the round's final state, both frames */
    double prior_chi2[4];     /* e^T H e of the prior edge at the round's final state */
    double prior_weight[4];   /* its Huber weight there: 1 while chi2 <= prior_huber_delta^2 */
    uint8_t *outlier;         /* [4][N_e], caller-owned, may be NULL: the flags after each round, by edge */
} orbfe_pose_inertial_prev_info;

/* replaces Optimizer::PoseInertialOptimizationLastFrame(pFrame, inlierThreshold, bRecInit) (src/Optimizer.cc:3846-4275; the call:
 * src/Tracking.cc:946) for the branch this fork takes: one pinhole camera, EdgeMonoOnlyPose edges, one EdgeInertial with all six
 * vertices free, EdgeGyroRW, EdgeAccRW, EdgePriorPoseImu; 30 unknowns.  Numerics: SPEC DECISION S20;
 * tests/pose_inertial_prev_ref.py is the normative restatement and the call equals it byte for byte.
 * Keypoints, matches, points, depths and the frame's state are those of orbfe_pose_inertial_optimization_last_keyframe.  The caller
 * returns 1000 itself when pFp->mpcpi is missing (:4057-4060).
 * ALL outputs are always written; the caller applies them only when *accepted != 0, as :4208 does.  Rwb_out .. ba_out: the frame's
 * state as floats; H30_out (900 doubles, row-major): the 30 x 30 Hessian of :4216-4264 in the reference's order (rows 0-14 the
 * previous frame, 15-29 the frame); Hprior_out (225 doubles; may be NULL: the marginalisation is skipped): Marginalize(H, 0, 14)
 * .block<15,15>(15,15), raw -- the eigenvalue clamp of new ConstraintPoseImu stays with the caller.  outlier_out (n) = mvbOutlier;
 * *n_inliers = the return value (nInitialCorrespondences - nBad); *accepted = (*n_inliers >= inlier_threshold).
 * One kernel launch of one block; one submission, one synchronisation.  HOST pointers.
 * ORBFE_ERR_INVALID_ARG / ORBFE_ERR_UNSUPPORTED: as for orbfe_pose_inertial_optimization_last_keyframe (the struct sizes of params,
 * link, prior and info).  NOT the reference's function in S19's four respects and in one more: the preintegrated
 * rotation at a new bias is dR0 ExpSO3(JRg dbg) in binary64 without NormalizeRotation, where the reference takes it in binary32
 * through Sophus and an SVD; and Optimizer::Marginalize's JacobiSVD is a pinned symmetric Jacobi eigen-decomposition. */
int orbfe_pose_inertial_optimization_last_frame(orbfe_handle *h, const orbfe_pose_inertial_prev_params *p,
                                                const orbfe_imu_link_free *link, const orbfe_pose_imu_prior *prior, int n,
                                                const orbfe_keypoint *kp, const int *mp_index, int n_points, const float *points,
                                                const float *track_depth, const float *Rcw, const float *tcw, const float *Rwb,
                                                const float *twb, const float *v, const float *bg, const float *ba, float *Rwb_out,
                                                float *twb_out, float *v_out, float *bg_out, float *ba_out, double *H30_out,
                                                double *Hprior_out, uint8_t *outlier_out, int *n_inliers, int *accepted,
                                                orbfe_pose_inertial_prev_info *info);

/* Batched, HBM-resident form: as orbfe_pose_inertial_optimization_batch_device, with one orbfe_imu_link_free (d_links[b]) and one
 * orbfe_pose_imu_prior (d_priors[b]) per frame; d_H30_out: 900 doubles per frame; d_Hprior_out: 225 doubles per frame (may be NULL);
 * d_accepted: one int per frame.  Frame b's results are byte-equal to orbfe_pose_inertial_optimization_last_frame on the same data. */
int orbfe_pose_inertial_optimization_last_frame_batch_device(orbfe_handle *h, const orbfe_pose_inertial_prev_params *p, int batch,
                                                             const orbfe_imu_link_free *d_links, const orbfe_pose_imu_prior *d_priors,
                                                             const orbfe_keypoint *d_kp, const int *d_n, int kp_stride,
                                                             const int *d_match, int n_map_points, const orbfe_world_point *d_points,
                                                             int point_stride_frames, const float *d_track_depth,
                                                             const float *d_state_in, float *d_state_out, double *d_H30_out,
                                                             double *d_Hprior_out, uint8_t *d_outlier, int *d_n_inliers,
                                                             int *d_accepted, void *stream);

/* Optimizer::Marginalize(H, 0, 14).block<15,15>(15,15) of a 30 x 30 row-major H on the HOST (no handle, no device): the same text
 * as the kernel's epilogue (csrc/marginalize.h), byte-equal to Hprior_out for the call's H30_out.  ORBFE_ERR_INVALID_ARG: a NULL. */
int orbfe_marginalize_pose_imu(const double *H, double *Hp);

/* -------------------------------------------------------------------------------------------
 * IMU preintegration, state prediction and the inertial links: what stands in front of orbfe_track_frame and the two inertial pose
 * optimisations once the IMU is initialised (src/Tracking.cc:163-350)
 * ---------------------------------------------------------------------------------------- */
/* IMU::Point (include/ImuTypes.h): 32 bytes */
typedef struct orbfe_imu_sample {
    double t;
    float a[3];
    float w[3];
} orbfe_imu_sample;

/* Preintegrated::integrable: one entry of mvMeasurements */
typedef struct orbfe_imu_step {
    float a[3];
    float w[3];
    float dt;
    float reserved;           /* 0 */
} orbfe_imu_step;

/* the diagonals of Calib::Cov (ng^2 x 3, na^2 x 3) and Calib::CovWalk (ngw^2 x 3, naw^2 x 3), scaled as src/Tracking.cc:116-123
 * does; versioned by struct_size */
typedef struct orbfe_imu_noise {
    int struct_size;          /* sizeof(orbfe_imu_noise) at the caller's compile time */
    int reserved;             /* 0 */
    float cov[6];
    float cov_walk[6];
} orbfe_imu_noise;

/* the whole state of IMU::Preintegrated except mvMeasurements (the caller keeps that list: the steps the calls hand out).  3 x 3
 * matrices and the 15 x 15 C are row-major; the floats from dT to C are one contiguous block.  Versioned by struct_size. */
typedef struct orbfe_imu_preint {
    int struct_size;          /* sizeof(orbfe_imu_preint) at the caller's compile time */
    int n_steps;              /* measurements integrated so far */
    float dT;
    float bg[3], ba[3];       /* b: bwx bwy bwz / bax bay baz */
    float dR[9], dV[3], dP[3];
    float JRg[9], JVg[9], JVa[9], JPg[9], JPa[9];
    float avgA[3], avgW[3];
    float C[225];
} orbfe_imu_preint;

#define ORBFE_IMU_FROM_KEYFRAME 0   /* the mbMapUpdated branch of PredictStateIMU (:301-325): the key-frame record, orbfe_imu_link */
#define ORBFE_IMU_FROM_FRAME    1   /* the other branch (:326-347): the frame record, orbfe_imu_link_free */

typedef struct orbfe_imu_predict_params {
    int struct_size;          /* sizeof(orbfe_imu_predict_params) at the caller's compile time */
    int which;                /* ORBFE_IMU_FROM_KEYFRAME or ORBFE_IMU_FROM_FRAME */
    float gravity;            /* IMU::GRAVITY_VALUE: g = (0, 0, -gravity) */
    float Rcb[9], tcb[3];     /* mImuCalib.mTcb */
    float tbc[3];             /* mImuCalib.mTbc.translation() */
} orbfe_imu_predict_params;

/* Tracking::PreintegrateIMU (src/Tracking.cc:234-290) for an already selected mvImuFromLastFrame of n_samples samples (the queue
 * pops of :201-232 stay with the caller), t_prev = mpPrevFrame->mTimeStamp, t_cur = mCurrentFrame->mTimeStamp.  The n_samples - 1
 * steps of :242-277 are integrated into *kf (mpImuPreintegratedFromLastKF) in place at that record's own bias, and into *frame, which
 * is first initialised at frame_bias (bwx bwy bwz bax bay baz of mLastFrame->mImuBias); steps_out (n_samples - 1 entries, may be
 * NULL) receives them for mvMeasurements; *n_steps = their number.  n_samples < 2: both records stay untouched and *n_steps = 0
 * (:235-238).  Numerics: SPEC DECISION S22; tests/imu_preint_ref.py is the normative restatement and the call
 * equals it byte for byte.  One kernel launch.  HOST pointers.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size (noise, either record), a NULL, n_samples < 0; decided before the device is touched.
 * NOT the reference's function in these stated respects: NormalizeRotation is the polar factor through a pinned
 * Jacobi eigen-decomposition, not Eigen's JacobiSVD; sin / cos of IntegratedRotation are the pinned binary64 sequences, rounded. */
int orbfe_imu_preintegrate_frame(orbfe_handle *h, const orbfe_imu_noise *noise, int n_samples, const orbfe_imu_sample *samples,
                                 double t_prev, double t_cur, const float *frame_bias, orbfe_imu_preint *kf, orbfe_imu_preint *frame,
                                 orbfe_imu_step *steps_out, int *n_steps);

/* Preintegrated::Initialize(bias) followed by IntegrateNewMeasurement over `steps` (src/ImuTypes.cc:149-237): Reintegrate() with the
 * record's own list, MergePrevious() with the two lists concatenated by the caller.  bias = bwx bwy bwz bax bay baz.  *out is written
 * whole (out->struct_size is set).  One kernel launch.  HOST pointers.  ORBFE_ERR_INVALID_ARG: a wrong struct_size, a NULL,
 * n_steps < 0. */
int orbfe_imu_reintegrate(orbfe_handle *h, const orbfe_imu_noise *noise, const float *bias, int n_steps, const orbfe_imu_step *steps,
                          orbfe_imu_preint *out);

/* Tracking::PredictStateIMU (src/Tracking.cc:293-350) with Frame::SetImuPoseVelocity (src/Frame.cc:221-238), and the inertial link the
 * pose optimisation behind it takes.  state1 (21 floats) = Rwb1 (9, row-major) twb1 v1 bg1 ba1 of the last key frame
 * (ORBFE_IMU_FROM_KEYFRAME) or of the last frame (ORBFE_IMU_FROM_FRAME).  state_out (33 floats) = Rcw tcw Rwb twb v bg ba, the
 * d_state_in of the batched pose optimisations, bg / ba being the start's (:323, :345).  link_out: an orbfe_imu_link with dR / dV / dP
 * = GetDelta*(b1) of *kf (ORBFE_IMU_FROM_KEYFRAME; `frame` may be NULL), or an orbfe_imu_link_free with the raw deltas, bias and
 * Jacobians of *frame and infoG / infoA of *kf's C (ORBFE_IMU_FROM_FRAME, src/Optimizer.cc:4046).  *info_ok = 1 when every pivot of
 * the covariance's factorisation was > 0; the link is written either way.  One kernel launch.  HOST pointers.
 * NOT the reference's function in these stated respects, besides those of orbfe_imu_preintegrate_frame: the
 * rotation at a new bias is S20's dR ExpSO3(JRg dbg) in binary64, then rounded and normalised; the covariance is inverted by L D L^T
 * without pivoting of its upper triangle, not Eigen's LU; the eigen-decomposition is S12's Jacobi sequence. */
int orbfe_imu_predict(orbfe_handle *h, const orbfe_imu_predict_params *p, const float *state1, const orbfe_imu_preint *kf,
                      const orbfe_imu_preint *frame, float *state_out, void *link_out, int *info_ok);

/* The three calls above for a batch of independent frames in ONE launch.  sample_off (batch + 1 ints, HOST: ascending, checked
 * here, passed on by one asynchronous copy): frame b owns d_samples[sample_off[b] .. sample_off[b + 1]).  DEVICE pointers otherwise:
 * d_t_prev / d_t_cur (one double per frame), d_frame_bias (6 floats per frame), d_state1 (21 floats per frame), d_kf (one record per
 * frame, in / out), d_frame (one record per frame, out; a frame with fewer than 2 samples leaves both records as they are and its
 * prediction reads them as they stand), d_steps_out (may be NULL; frame b's steps at d_steps_out[sample_off[b] ..]), d_state_in (33
 * floats per frame), d_links (orbfe_imu_link or orbfe_imu_link_free per frame, by p->which), d_info_ok (one int per frame).
 * d_state_in and d_links are what orbfe_pose_inertial_optimization_batch_device (ORBFE_IMU_FROM_KEYFRAME) and
 * orbfe_pose_inertial_optimization_last_frame_batch_device (ORBFE_IMU_FROM_FRAME) read.  Asynchronous on `stream` (NULL == the
 * handle's stream), no host synchronisation.  Frame b's bytes equal the three host-pointer calls on the same data.  The records'
 * struct_size cannot be checked by a device call.  ORBFE_ERR_INVALID_ARG: a wrong struct_size, a NULL, batch < 1, sample_off[0] < 0
 * or descending offsets. */
int orbfe_imu_frame_batch_device(orbfe_handle *h, const orbfe_imu_noise *noise, const orbfe_imu_predict_params *p, int batch,
                                 const orbfe_imu_sample *d_samples, const int *sample_off, const double *d_t_prev,
                                 const double *d_t_cur, const float *d_frame_bias, const float *d_state1, orbfe_imu_preint *d_kf,
                                 orbfe_imu_preint *d_frame, orbfe_imu_step *d_steps_out, float *d_state_in, void *d_links,
                                 int *d_info_ok, void *stream);

/* orbfe_imu_reintegrate for a batch of records in ONE launch: step_off (batch + 1 ints, HOST, as sample_off above), d_steps, d_bias (6
 * floats per record), d_out (one record per entry, written whole).  Asynchronous on `stream`. */
int orbfe_imu_reintegrate_batch_device(orbfe_handle *h, const orbfe_imu_noise *noise, int batch, const orbfe_imu_step *d_steps,
                                       const int *step_off, const float *d_bias, orbfe_imu_preint *d_out, void *stream);

/* -------------------------------------------------------------------------------------------
 * Tracking::TrackLocalMap once the IMU is initialised, for a batch of frames, resident in HBM (SPEC DECISION S23):
 *   PreintegrateIMU + PredictStateIMU                       (src/Tracking.cc:163-350)   orbfe_imu_frame_batch_device
 *   SearchLocalPoints: isInFrustum + SearchByProjection     (:1037-1117)                frustum from the predicted state, on the device
 *   PoseInertialOptimizationLastKeyFrame / ...LastFrame     (:952 / :946)               the S19 / S20 batch launch
 *   mnMatchesInliers, the tracked verdict, IncreaseFound    (:958-982)
 * as launches back to back on one stream: no host synchronisation and no copy in between.
 * ---------------------------------------------------------------------------------------- */
/* One block for the whole chain, versioned by struct_size; the nested blocks carry their own struct_size and are checked too.
 * predict.which chooses the link kind and with it the optimisation: ORBFE_IMU_FROM_KEYFRAME reads pose_keyframe, ORBFE_IMU_FROM_FRAME
 * reads pose_frame (the other one is not looked at). */
typedef struct orbfe_track_inertial_params {
    int struct_size;                            /* sizeof(orbfe_track_inertial_params) at the caller's compile time */
    int inlier_threshold;                       /* tracked = matches_inliers >= inlier_threshold; Tracking passes 8 */
    orbfe_track_params track;                   /* the frame grid and the parameters of SearchByProjection */
    orbfe_imu_noise noise;                      /* as orbfe_imu_frame_batch_device */
    orbfe_imu_predict_params predict;           /* as orbfe_imu_frame_batch_device */
    orbfe_frustum frustum;                      /* TEMPLATE: bounds, camera, mbf, log_scale_factor, n_levels, camera_model; its rcw /
                                                 * tcw / twc are ignored -- the pose is the predicted one, per frame, on the device */
    orbfe_pose_inertial_params pose_keyframe;   /* S19's block */
    orbfe_pose_inertial_prev_params pose_frame; /* S20's block */
} orbfe_track_inertial_params;

/* The pointers of orbfe_track_inertial_batch_device: DEVICE pointers except sample_off.  Versioned by struct_size.  With B = batch,
 * M = n_points and kp_stride as given to the call: */
typedef struct orbfe_track_inertial_io {
    int struct_size;                  /* sizeof(orbfe_track_inertial_io) at the caller's compile time */
    int reserved;                     /* 0 */
    /* ---- in: orbfe_imu_frame_batch_device's ---- */
    const orbfe_imu_sample *d_samples;
    const int *sample_off;            /* HOST, B + 1 ascending offsets into d_samples */
    const double *d_t_prev, *d_t_cur; /* one per frame */
    const float *d_frame_bias;        /* 6 per frame */
    const float *d_state1;            /* 21 per frame */
    orbfe_imu_preint *d_kf;           /* in / out, one per frame */
    orbfe_imu_preint *d_frame;        /* out (read as it stands by a frame with fewer than 2 samples), one per frame */
    orbfe_imu_step *d_steps_out;      /* may be NULL */
    /* ---- in: the frames as orbfe_extract_batch_device wrote them ---- */
    const orbfe_keypoint *d_kp;       /* B x kp_stride */
    const uint8_t *d_desc;            /* B x kp_stride x 32 */
    const int *d_n;                   /* B */
    /* ---- in: the local maps ---- */
    const int *d_ids;                 /* B x M: id >= 0, ~id = skipped for this frame, outside the map = no point; NULL only when M == 0 */
    const orbfe_pose_imu_prior *d_priors; /* one per frame with ORBFE_IMU_FROM_FRAME; NULL otherwise */
    /* ---- out ---- */
    float *d_state_in;                /* 33 per frame: the predicted Rcw tcw Rwb twb v bg ba */
    int *d_info_ok;                   /* one per frame */
    orbfe_map_point *d_mp_out;        /* B x M records; in_view is IncreaseVisible (:1073); NULL only when M == 0 */
    int *d_match_out;                 /* B x kp_stride: position in the frame's id list, or -1 */
    int *d_n_matches;                 /* B */
    float *d_state_out;               /* 21 per frame: the optimised Rwb twb v bg ba */
    double *d_H_out;                  /* 225 per frame (ORBFE_IMU_FROM_KEYFRAME) or 900 per frame (ORBFE_IMU_FROM_FRAME) */
    double *d_Hprior_out;             /* ORBFE_IMU_FROM_FRAME: 225 per frame, may be NULL; ignored otherwise */
    uint8_t *d_outlier;               /* B x kp_stride bytes, d_n[b] are written */
    int *d_n_inliers;                 /* B: the optimisation's return value */
    int *d_accepted;                  /* B: S20's verdict; written as 1 with ORBFE_IMU_FROM_KEYFRAME */
    uint8_t *d_found;                 /* B x M bytes: 1 where IncreaseFound() runs (:967), 0 elsewhere; NULL only when M == 0 */
    int *d_matches_inliers;           /* B: mnMatchesInliers (:969-976) */
    int *d_tracked;                   /* B: matches_inliers >= inlier_threshold */
    float *d_Tcw_out;                 /* 12 per frame, Rcw then tcw: SetImuPoseVelocity on the optimised Rwb / twb; the predicted pose
                                       * where ORBFE_IMU_FROM_FRAME did not accept (src/Optimizer.cc:4208) */
} orbfe_track_inertial_io;

/* The chain above for `batch` independent frames.  The frames' keypoints, descriptors and counts are orbfe_extract_batch_device's
 * outputs (kp_stride == orbfe_max_keypoints(), <= 65536); frame b's local map points are the entries d_ids[b * n_points ..] of the
 * resident `map`.  Numerics: SPEC DECISION S23 for the glue -- the frustum from the predicted state, the
 * hand-over of point rows and depths, the statistics, Tcw_out; S22, S8, the matcher's, S19 / S20 for the stages, whose bytes are those
 * of their own entry points: frame b's outputs equal orbfe_imu_preintegrate_frame + orbfe_imu_predict, orbfe_project_map_points with
 * the frustum of S23, orbfe_match_projection (init_obs == NULL: mvpMapPoints is empty when SearchLocalPoints starts, :908-923) and
 * orbfe_pose_inertial_optimization_last_keyframe / _last_frame (mp_index = the matches, the resident rows, track_depth of the
 * records), byte for byte.  Statistics (mono, mbOnlyTracking == false): for keypoint i < d_n[b] with m = match[i] >= 0,
 * found[m] = !outlier[i] and matches_inliers += (!outlier[i] && record[m].observations > 0).
 * Asynchronous on `stream` (NULL == the handle's stream): the S22 launch, the projection launch, the three matcher launches, the S19
 * or S20 launch and the statistics launch, back to back; no host synchronisation.  Gathered descriptors, point rows, depths and the
 * links live in the handle's matcher arena (grown on first use, ordered against its other users by the event hand-over).
 * n_points == 0 is valid: the inertial edges alone give a full-rank system.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size (outer or nested), a required NULL, batch < 1, n_points < 0, kp_stride outside [1, 65536],
 * descending sample_off, d_priors missing with ORBFE_IMU_FROM_FRAME, frustum.n_levels above the handle's, a map of another handle.
 * ORBFE_ERR_UNSUPPORTED: KannalaBrandt8 (frustum or pose block), stereo != 0.  All decided before the device is touched. */
int orbfe_track_inertial_batch_device(orbfe_handle *h, const orbfe_track_inertial_params *p, int batch, int kp_stride,
                                      const orbfe_map *map, int n_points, const orbfe_track_inertial_io *io, void *stream);

/* What orbfe_track_frame_inertial hands back besides the frame's features.  HOST pointers; versioned by struct_size.  Every pointer
 * is required except steps_out, link_out and Hprior_out; mp_out and found are required when n_points > 0. */
typedef struct orbfe_track_inertial_result {
    int struct_size;          /* sizeof(orbfe_track_inertial_result) at the caller's compile time */
    int n_steps;              /* out: steps integrated (n_samples - 1, or 0) */
    orbfe_imu_step *steps_out;/* n_samples - 1 entries, may be NULL */
    float *state_in;          /* 33 */
    void *link_out;           /* an orbfe_imu_link or orbfe_imu_link_free by predict.which, may be NULL */
    int info_ok;              /* out */
    int n_matches;            /* out */
    orbfe_map_point *mp_out;  /* n_points */
    int *match_out;           /* orbfe_max_keypoints() ints; the first *n_out are meaningful */
    float *state_out;         /* 21 */
    double *H_out;            /* 225 or 900 */
    double *Hprior_out;       /* 225, ORBFE_IMU_FROM_FRAME only, may be NULL */
    uint8_t *outlier;         /* orbfe_max_keypoints() bytes; the first *n_out are meaningful */
    uint8_t *found;           /* n_points */
    int n_inliers, accepted, matches_inliers, tracked;  /* out */
    float Tcw[12];            /* out */
} orbfe_track_inertial_result;

/* The same chain for ONE frame from host pointers, image in, results out: one upload (the frame, then samples, records, ids and prior
 * as one block), orbfe_extract's device path, the chain above with batch == 1, ONE result download and ONE synchronisation.  gray /
 * pitch, kp_out / desc_out / n_out / per_level_counts as orbfe_track_frame_map.  kf: in / out; frame: out (in, when n_samples < 2).
 * prior: required with ORBFE_IMU_FROM_FRAME.  Results equal orbfe_extract followed by orbfe_track_inertial_batch_device on that frame.
 * Refusals as the batch call's, plus the records' struct_size.  No graph capture. */
int orbfe_track_frame_inertial(orbfe_handle *h, const orbfe_track_inertial_params *p, const uint8_t *gray, int pitch, int n_samples,
                               const orbfe_imu_sample *samples, double t_prev, double t_cur, const float *frame_bias, const float *state1,
                               orbfe_imu_preint *kf, orbfe_imu_preint *frame, const orbfe_map *map, int n_points, const int *ids,
                               const orbfe_pose_imu_prior *prior, orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out,
                               int *per_level_counts, orbfe_track_inertial_result *res);

/* -------------------------------------------------------------------------------------------
 * Tracking::UpdateLocalMap from a resident covisibility graph (src/Tracking.cc:1119-1324; SPEC DECISION S24, DESIGN.md section 2;
 * tests/local_map_ref.py is the normative restatement).  UpdateLocalKeyFrames (:1157-1324) followed by UpdateLocalPoints
 * (:1129-1154) for a batch of independent frames: the output is the id list every per-frame chain takes as `ids` / `d_ids`.
 * ---------------------------------------------------------------------------------------- */
#define ORBFE_COVIS_MAX_COVISIBLE 16     /* ordered covisibles kept per key frame (the nodes ask for the best 5) */
#define ORBFE_LOCAL_KF_MAX 288           /* 4 * 64 + 32: first phase + three appended per first-phase key frame + the temporal ones */
#define ORBFE_NO_POINT 0x7fffffff        /* pad of an id row: outside every map and unchanged by ~, so every consumer reads "no point" */
#define ORBFE_LOCAL_MAP_BLOCK 1024       /* threads of the points kernel's block: the walk is resolved in chunks of this many slots */
#define ORBFE_LOCAL_MAP_VOTE_TABLE 512   /* distinct voted key frames the LDS vote table holds; above it, exact counters in HBM */

typedef struct orbfe_covis orbfe_covis;

/* The graph UpdateLocalMap walks, resident in HBM: per key frame slot in [0, kf_capacity) mnId, isBad(), the parent, mPrevKF, the
 * map point of every feature slot (GetMapPointMatches), the ordered covisibles (the head of mvpOrderedConnectedKeyFrames) and the
 * children in the caller's order; per point id of `map` (same ids, same capacity; the map's `bad` field is the points' isBad()) the
 * key frames that observe it.  The caller's key-frame slots stand for the key frames: mn_id must differ between slots.
 * A slot that was never set is a bad key frame with mn_id == slot, no features, no parent.
 * Device memory, all taken at create: 4 * (kf_capacity * (8 + 16 + child_stride + kf_stride) + capacity * (1 + obs_stride)) bytes
 * (10 000 key frames x 3000 slots: 120 MB).  Per-call scratch is kept with the graph and grows to the largest batch seen:
 * 4 * batch * (capacity + kf_capacity) bytes; batch * capacity above 2^28 is refused with ORBFE_ERR_OUT_OF_MEMORY.
 * kf_capacity in [1, 262144], kf_stride in [1, 2^20], obs_stride in [1, 4096], child_stride in [1, 4096].
 * Lifetime: as orbfe_map's.  orbfe_covis_destroy waits for the handle's stream; orbfe_destroy releases the device memory of the graphs
 * created from the handle, destroying them afterwards only frees the shell; destroying `map` first detaches it and every later call on
 * the graph returns ORBFE_ERR_INVALID_ARG. */
int orbfe_covis_create(orbfe_handle *h, const orbfe_map *map, int kf_capacity, int kf_stride, int obs_stride, int child_stride,
                       orbfe_covis **out);
void orbfe_covis_destroy(orbfe_covis *g);

/* one key frame as orbfe_covis_set_keyframes takes it; HOST pointers; versioned by struct_size */
typedef struct orbfe_covis_keyframe {
    int struct_size;          /* sizeof(orbfe_covis_keyframe) at the caller's compile time */
    int slot;                 /* [0, kf_capacity) */
    int mn_id;                /* KeyFrame::mnId, >= 0 */
    int bad;                  /* isBad() */
    int parent;               /* GetParent(): slot or -1 */
    int prev;                 /* mPrevKF: slot or -1 */
    int n_features;           /* <= kf_stride; ignored when point_ids == NULL */
    int n_covisible;          /* <= ORBFE_COVIS_MAX_COVISIBLE: the head of GetBestCovisibilityKeyFrames' list, bad ones included */
    int n_children;           /* <= child_stride; S24: their order here is the order of the expansion */
    int reserved;             /* 0 */
    const int *point_ids;     /* n_features ids, < 0 or outside the map = no point; NULL keeps the stored list and its length */
    const int *covisible;     /* n_covisible slots (or -1) */
    const int *children;      /* n_children slots (or -1) */
} orbfe_covis_keyframe;

/* Writes n key frames: one staged block, one upload, one scatter launch on the handle's stream, i.e. behind everything submitted
 * before on that stream; returns when the tables are updated.  This is where the mapping thread's changes reach the graph (the
 * mbMapUpdated moment).  Everything is validated on the host before the device is touched and nothing is written on a
 * refusal: ORBFE_ERR_INVALID_ARG for a wrong struct_size, a slot outside [0, kf_capacity) or named twice, mn_id < 0, a count above its
 * stride, a covisible / child / parent / prev slot outside [-1, kf_capacity), a missing list. */
int orbfe_covis_set_keyframes(orbfe_handle *h, orbfe_covis *g, int n, const orbfe_covis_keyframe *recs);
/* Sets the observation lists (MapPoint::GetObservations, key-frame slots) of n points in CSR form: point ids[i] is observed by
 * kf_slots[off[i] .. off[i + 1]); an empty range clears.  Ordering and validation as above: ORBFE_ERR_INVALID_ARG for an id outside the
 * map or named twice, descending offsets, a range longer than obs_stride, a slot outside [0, kf_capacity).  HOST pointers. */
int orbfe_covis_set_observations(orbfe_handle *h, orbfe_covis *g, int n, const int *ids, const int *off, const int *kf_slots);

typedef struct orbfe_local_map_params {
    int struct_size;          /* sizeof(orbfe_local_map_params) at the caller's compile time */
    int max_local_kf;         /* mMaxLocalKFCount, 1..64 (the nodes pass 10 / 15) */
    int n_covisible;          /* mCovisibilityKeyFrameNd, 0..ORBFE_COVIS_MAX_COVISIBLE (5) */
    int n_temporal;           /* mTemporalKeyFrameNd, 0..32 (10) */
    int inertial;             /* != 0: the temporal key frames of :1298-1314 are appended */
    int mark_voters_seen;     /* != 0: a point that voted is emitted as ~id (:1040-1056, the frame's own points are already matched) */
} orbfe_local_map_params;
#define ORBFE_LOCAL_MAP_PARAMS_INIT {(int)sizeof(orbfe_local_map_params), 10, 5, 10, 1, 0}

/* The pointers of orbfe_update_local_map_batch_device: DEVICE pointers.  Versioned by struct_size.  B = batch, M = n_points. */
typedef struct orbfe_local_map_io {
    int struct_size;          /* sizeof(orbfe_local_map_io) at the caller's compile time */
    int reserved;             /* 0 */
    const int *d_vote_ids;    /* B x vote_stride: the point id at every keypoint of the frame whose matches vote (the current frame
                               * before IMU initialisation, the last frame after it, :1164 / :1188); outside the map = no point */
    const int *d_n_votes;     /* B: keypoints of that frame (clamped to [0, vote_stride]) */
    const int *d_last_kf;     /* B: mCurrentFrame->mpLastKeyFrame as a slot, outside [0, kf_capacity) = none; read when inertial != 0 */
    int *d_ids_out;           /* B x M: the local map points in mvpLocalMapPoints order, then ORBFE_NO_POINT */
    int *d_n_local_points;    /* B: the true count, also when it exceeds M (nothing is written past slot M) */
    int *d_local_kfs;         /* B x ORBFE_LOCAL_KF_MAX: mvpLocalKeyFrames as slots, then -1 */
    int *d_n_local_kfs;       /* B */
    int *d_vote_ids_out;      /* B x vote_stride, may be NULL, may be d_vote_ids: entry i < n_votes is the input, or -1 where the
                               * point is bad (:1181, :1207); entries from n_votes on are not written */
} orbfe_local_map_io;

/* S24 for `batch` independent frames against one graph.  Per frame: every non-bad voter adds one to each key frame that observes it
 * (a point at two keypoints votes twice); the key frames are ranked by count descending, equal counts in ascending mn_id (S24 pins the
 * order std::sort leaves open); the first min(max_local_kf, voted) are taken, a bad one is skipped but uses its place; then, over
 * those in order: the first of the best n_covisible covisibles that is not bad and not yet listed, the first such child, and the
 * parent when not yet listed -- with no bad test, and ending the expansion (:1292); with `inertial`, last_kf and its mPrevKF chain
 * while they are new, at most n_temporal (:1303-1313, a listed one stops the chain as written).  The points: the list in REVERSE, every
 * feature slot ascending, first occurrence of a point that is not bad.
 * Asynchronous on `stream` (NULL == the handle's): four launches of a block per frame, back to back, no host synchronisation, no allocation unless
 * `batch` exceeds every earlier call's.  Results do not depend on `batch` or on the order the votes arrive in.  d_ids_out is laid out
 * as orbfe_track_inertial_batch_device and orbfe_match_projection_batch_device read d_ids.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size, a required NULL, batch < 1, n_points < 1, vote_stride < 1, a parameter outside its range,
 * a graph of another handle or whose map is gone; all decided before the device is touched.  ORBFE_ERR_OUT_OF_MEMORY: see above. */
int orbfe_update_local_map_batch_device(orbfe_handle *h, const orbfe_local_map_params *p, int batch, int vote_stride,
                                        orbfe_covis *covis, int n_points, const orbfe_local_map_io *io, void *stream);
/* The same for ONE frame from HOST pointers: one upload, the same launch, one download, one synchronisation.  n_votes >= 0 (vote_ids
 * may be NULL when it is 0); last_kf as d_last_kf; ids_out n_points ints, local_kfs ORBFE_LOCAL_KF_MAX ints; vote_ids_out n_votes ints
 * or NULL.  Results equal the batch call's with batch == 1. */
int orbfe_update_local_map(orbfe_handle *h, const orbfe_local_map_params *p, int n_votes, const int *vote_ids, int last_kf,
                           orbfe_covis *covis, int n_points, int *ids_out, int *n_local_points, int *local_kfs, int *n_local_kfs,
                           int *vote_ids_out);

/* The frame's mvpMapPoints as Track() leaves them behind TrackLocalMap (src/Tracking.cc:504-533), from what
 * orbfe_track_inertial_batch_device left in HBM: d_out[b][i] (B x kp_stride) = the id d_ids[b][d_match[b][i]] when keypoint i < d_n[b]
 * has a match inside [0, n_points), that id is inside the map, its Observations() >= 1 (:508) and d_outlier[b][i] == 0 (:531); -1
 * otherwise and for i >= d_n[b].  A thread per keypoint; asynchronous on `stream`.  With it frame k's results become frame k + 1's
 * id list without leaving HBM: this call -> orbfe_update_local_map_batch_device -> d_ids.
 * ORBFE_ERR_INVALID_ARG: a NULL, batch < 1, kp_stride < 1, n_points < 1, a map of another handle. */
int orbfe_frame_points_batch_device(orbfe_handle *h, const orbfe_map *map, int batch, int kp_stride, int n_points, const int *d_ids,
                                    const int *d_match, const uint8_t *d_outlier, const int *d_n, int *d_out, void *stream);

/* -------------------------------------------------------------------------------------------
 * Maintaining the resident graph on the device: KeyFrame::UpdateConnections (src/KeyFrame.cc:459-553) with AddConnection (:191-204)
 * and UpdateBestCovisibles (:206-228), and the graph part of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:338-361).
 * SPEC DECISION S25; tests/covis_update_ref.py is the normative restatement.  One graph is one map: the
 * reference's test GetMap() != mpMap (:485) has no counterpart.  Opt-in: a graph on which orbfe_covis_enable_connections was never
 * called holds and does exactly what it did before.
 * ---------------------------------------------------------------------------------------- */
#define ORBFE_COVIS_MAX_CONN_STRIDE 4096
#define ORBFE_COVIS_STATUS_OK 0          /* the key frame was processed */
#define ORBFE_COVIS_STATUS_NO_COUNTS 1   /* UpdateConnections: nobody shares a point with it (:493); nothing was written */
#define ORBFE_COVIS_STATUS_REFUSED 2     /* a row is full; nothing of that key frame (of that call, for add_keyframe) was written */

/* Allocates, per key-frame slot, the full mConnectedKeyFrameWeights as (slot, weight) pairs, up to conn_stride of them, and a count;
 * all rows empty.  The order of a row is not observable: no output depends on it.  Device memory: 4 * kf_capacity * (2 * conn_stride + 1)
 * + 12 * conn_stride + 32 bytes (10 000 key frames x 512: 41 MB), released with the graph.  conn_stride in [1, 4096].
 * ORBFE_ERR_INVALID_ARG: a NULL, a graph of another handle or whose map is gone, conn_stride outside its range, a second call on the
 * same graph.  Waits for the handle's stream. */
int orbfe_covis_enable_connections(orbfe_handle *h, orbfe_covis *g, int conn_stride);
/* Imports connection rows from the host in CSR form: key frame slots[i] is connected to conn_slots[off[i] .. off[i + 1]) with
 * weights[...]; an empty range clears the row.  Ordering and validation as orbfe_covis_set_observations, nothing is written on a
 * refusal: ORBFE_ERR_INVALID_ARG for connections not enabled, a slot outside [0, kf_capacity) or named twice, descending offsets, a
 * range longer than conn_stride, a connected slot outside [0, kf_capacity), a weight < 0.  HOST pointers. */
int orbfe_covis_set_connections(orbfe_handle *h, orbfe_covis *g, int n, const int *slots, const int *off, const int *conn_slots,
                                const int *weights);
/* Reads one key frame back to HOST memory, waiting for the handle's stream: rec receives the scalars (struct_size must be set by the
 * caller; slot, mn_id, bad, parent, prev, n_features, n_covisible, n_children; its pointers are set to NULL), covisible
 * ORBFE_COVIS_MAX_COVISIBLE ints (the first n_covisible are the stored head), children child_stride ints (the first n_children),
 * conn_slots / conn_weights conn_stride ints each and *n_conn (all three may be NULL; required NULL when connections are not
 * enabled).  ORBFE_ERR_INVALID_ARG: a NULL, a wrong struct_size, a slot outside [0, kf_capacity), a connection pointer on a graph
 * without connections. */
int orbfe_covis_get_keyframe(orbfe_handle *h, orbfe_covis *g, int slot, orbfe_covis_keyframe *rec, int *covisible, int *children,
                             int *conn_slots, int *conn_weights, int *n_conn);

typedef struct orbfe_covis_update_params {
    int struct_size;          /* sizeof(orbfe_covis_update_params) at the caller's compile time */
    int min_weight;           /* `th` of KeyFrame.cc:500: 50 in this fork (upstream 15); [1, 2^20] */
} orbfe_covis_update_params;
#define ORBFE_COVIS_UPDATE_PARAMS_INIT {(int)sizeof(orbfe_covis_update_params), 50}

/* The outputs of orbfe_covis_update_connections_device: DEVICE pointers, per processed key frame k.  Versioned by struct_size. */
typedef struct orbfe_covis_update_io {
    int struct_size;          /* sizeof(orbfe_covis_update_io) at the caller's compile time */
    int reserved;             /* 0 */
    int *d_slots;             /* n x conn_stride: mvpOrderedConnectedKeyFrames as slots, the whole list, then -1 */
    int *d_weights;           /* n x conn_stride: mvOrderedWeights, then 0 */
    int *d_count;             /* n: the length of the list; 0 unless status is ORBFE_COVIS_STATUS_OK */
    int *d_status;            /* n: ORBFE_COVIS_STATUS_* */
} orbfe_covis_update_io;

/* KeyFrame::UpdateConnections for the key frames slots[0 .. n), a HOST array, IN ORDER, each against the graph as the one before left
 * it (src/Tracking.cc:690-691 is n == 2), in one submission on `stream` with no host synchronisation in between.  flags (HOST):
 * flags[k] & 1 = mbFirstConnection && mnId != GetInitKFid() (:545).  For key frame s:
 *   counting   every feature slot of s whose id is inside the map and whose point is not bad adds one for every observer o of that
 *              point with o != s and o not bad; a point held at two feature slots counts twice.  No counts: status 1, nothing written.
 *   selection  every counted key frame with count >= min_weight is connected; if there is none, the one with the largest count, among
 *              equal maxima the lowest mn_id (S25 lets mn_id stand for the address the reference's map iterates by).
 *   own lists  the connection row of s becomes ALL counted key frames, those below min_weight included (:540, as written); the ordered
 *              list is the connected ones, weight descending, equal weights in DESCENDING mn_id, then descending slot (S25); its first
 *              ORBFE_COVIS_MAX_COVISIBLE become the stored head, the whole of it goes to io.
 *   reciprocal for each connected q (AddConnection): s absent from q's row: inserted; present with the same weight: nothing happens to
 *              q at all (a stale head stays stale); present with another weight: overwritten.  In the two changing cases q's head
 *              becomes the first ORBFE_COVIS_MAX_COVISIBLE of q's row ordered as above, without the key frames that are bad NOW.
 *   parent     with flags & 1: parent(s) = the front of the ordered list, and s is appended to that key frame's children unless there.
 *   capacity   more than conn_stride counted key frames, a full row of a q where an insert is due, or a full children row: decided
 *              before anything of that key frame is written; the graph is left untouched by it and status is 2.
 * Four launches per key frame; results do not depend on the arrival order of any atomic.  Not offered: EraseConnection / SetBadFlag,
 * mvOrderedWeights as resident state, loop and merge edges.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size, a NULL, n < 1, min_weight outside its range, a slot outside [0, kf_capacity), a graph of
 * another handle, whose map is gone or without connections; all decided before the device is touched. */
int orbfe_covis_update_connections_device(orbfe_handle *h, const orbfe_covis_update_params *p, orbfe_covis *g, int n, const int *slots,
                                          const int *flags, const orbfe_covis_update_io *io, void *stream);
/* The same for ONE key frame with HOST outputs: the same launches, one download, one synchronisation.  ordered_slots /
 * ordered_weights: conn_stride ints each.  Results equal the device call's with n == 1; ORBFE_ERR_OUT_OF_MEMORY when *status is 2. */
int orbfe_covis_update_connections(orbfe_handle *h, const orbfe_covis_update_params *p, orbfe_covis *g, int slot, int flag,
                                   int *ordered_slots, int *ordered_weights, int *count, int *status);

/* The graph part of LocalMapping::ProcessNewKeyFrame.  rec (HOST): the scalars slot, mn_id, bad, parent, prev of the new key frame; its
 * counts and lists are not read.  d_point_ids (DEVICE): n_features ids, < 0 or outside the map = no point -- the row
 * orbfe_frame_points_batch_device writes is accepted as it stands.  The call writes the key frame's record (no covisibles, no
 * children, an empty connection row) and point list, then, as :340-359, for every feature slot whose point is inside the map and
 * not bad appends the key frame to the point's observation list unless the list holds it already (IsInKeyFrame).  d_added[i]
 * (n_features ints): 1 where that happened (the host owes UpdateDepth / ComputeDistinctiveDescriptors for that point), 2 where the
 * point was already in the key frame (:353-356), 0 otherwise.  Of two feature slots with the same point the LOWEST adds and the other
 * reads 2, whatever the scheduling.  A full observation list (obs_stride) refuses the whole call before anything is written:
 * *d_status = 2 and d_added all 0; otherwise *d_status = 0.  The map's own records (observations, bad) are not touched: they stay
 * with orbfe_map_update.  One launch, asynchronous on `stream`; chained on one stream, this call -> orbfe_covis_update_connections_device
 * -> orbfe_update_local_map_batch_device is the whole path from a tracked frame to the next local map with no host table in between.
 * ORBFE_ERR_INVALID_ARG: a NULL, a wrong struct_size, a slot outside [0, kf_capacity), mn_id < 0, parent / prev outside
 * [-1, kf_capacity), n_features outside [0, kf_stride], a graph of another handle or whose map is gone. */
int orbfe_covis_add_keyframe_device(orbfe_handle *h, orbfe_covis *g, const orbfe_covis_keyframe *rec, const int *d_point_ids,
                                    int n_features, int *d_added, int *d_status, void *stream);
/* The same from HOST pointers, for a caller whose new key frame is host objects (include/orbfe_adaptor.hpp): one upload, the same
 * launch, one download, one synchronisation.  rec->point_ids / rec->n_features are the point row (NULL allowed when n_features == 0);
 * added: n_features ints.  Results equal the device call's; ORBFE_ERR_OUT_OF_MEMORY when *status is 2. */
int orbfe_covis_add_keyframe(orbfe_handle *h, orbfe_covis *g, const orbfe_covis_keyframe *rec, int *added, int *status);

/* -------------------------------------------------------------------------------------------
 * Refreshing map points from the resident graph: MapPoint::UpdateDepth (src/MapPoint.cc:440-474) and
 * MapPoint::ComputeDistinctiveDescriptors (:343-417), the two functions the mapping thread runs on every point a key frame adds or
 * touches (src/LocalMapping.cc:350-351, :718-720, :866-867) and every Optimizer entry point ends in.  They write the records every
 * per-frame chain reads: min_distance / max_distance (the frustum gate, PredictScale) and the 32-byte descriptor (SearchByProjection).
 * SPEC DECISION S26; tests/point_refresh_ref.py is the normative restatement.  Monocular key frames: one
 * observation per (point, key frame), no rightIndex.  Opt-in: a graph on which orbfe_covis_enable_refresh was never called holds and
 * does exactly what it did before.
 * ---------------------------------------------------------------------------------------- */
#define ORBFE_REFRESH_MAX_LEVELS 32
#define ORBFE_REFRESH_DEPTH 1            /* `what` bit 0: UpdateDepth; status bit 0: the distances were written */
#define ORBFE_REFRESH_DESCRIPTOR 2       /* `what` bit 1: ComputeDistinctiveDescriptors; status bit 1: the descriptor was written */

/* Allocates, all rows empty: per key-frame slot kf_stride descriptors of 32 bytes, kf_stride octaves of one byte, a feature count and
 * the camera centre GetTranslationInverse() (3 floats); per point of the map obs_stride feature indices parallel to the observation
 * list (all -1, the reference's leftIndex == -1) and mpRefKF as a slot (-1: none); per graph mvScaleFactors[0 .. n_levels) from
 * scale_factors (HOST).  Device memory: kf_capacity * (33 * kf_stride + 16) + 4 * capacity * (obs_stride + 1) + 128 bytes, released
 * with the graph (10 000 key frames x 3000 slots: 0.99 GB, 0.96 GB of it descriptors; a map of 200 000 points x 64 observations adds
 * 51 MB), plus 4 bytes per entry of the longest list a refresh call was given.  n_levels in [1, 32]; kf_capacity * kf_stride must
 * stay below 2^31.  ORBFE_ERR_INVALID_ARG: a NULL, a graph of another handle or whose map is gone, n_levels or the product outside
 * their range, a second call on the same graph.  Waits for the handle's stream. */
int orbfe_covis_enable_refresh(orbfe_handle *h, orbfe_covis *g, int n_levels, const float *scale_factors);
/* The setters: ordering and validation as orbfe_covis_set_observations (one staged block, one upload, on the handle's stream, return
 * when the tables are updated; everything validated on the host first, nothing written on a refusal).  All of them refuse a graph
 * without refresh state with ORBFE_ERR_INVALID_ARG.
 * set_features: the n keypoints (only `octave` is read) and n x 32 descriptor bytes of key frame `slot`, HOST pointers; n in
 *   [0, kf_stride], every octave in [0, n_levels), slot in [0, kf_capacity).  The count is stored: an index at or beyond it names no
 *   feature. */
int orbfe_covis_set_features(orbfe_handle *h, orbfe_covis *g, int slot, int n, const orbfe_keypoint *kp, const uint8_t *desc);
/* The same from the DEVICE arrays an extraction left in HBM, asynchronous on `stream` (NULL == the handle's stream): a tracked frame
 * promoted to key frame never leaves the device.  Octaves are clamped to [0, n_levels) on the device, not trusted. */
int orbfe_covis_set_features_device(orbfe_handle *h, orbfe_covis *g, int slot, const orbfe_keypoint *d_kp, const uint8_t *d_desc, int n,
                                    void *stream);
/* Camera centres (GetTranslationInverse(), 3 floats each, finite) of n key frames, HOST pointers; the mapping thread calls it after a
 * bundle adjustment.  ORBFE_ERR_INVALID_ARG: a slot outside [0, kf_capacity) or named twice, a non-finite value. */
int orbfe_covis_set_centres(orbfe_handle *h, orbfe_covis *g, int n, const int *slots, const float *twc);
/* orbfe_covis_set_observations plus the feature index of each observation, feat_idx[k] in [-1, kf_stride) parallel to kf_slots.  On a
 * graph with refresh state orbfe_covis_set_observations itself keeps working and writes -1 for every index of the points it names. */
int orbfe_covis_set_observations_indexed(orbfe_handle *h, orbfe_covis *g, int n, const int *ids, const int *off, const int *kf_slots,
                                         const int *feat_idx);
/* mpRefKF of n points as slots in [-1, kf_capacity); ids inside the map, none named twice. */
int orbfe_covis_set_ref_keyframes(orbfe_handle *h, orbfe_covis *g, int n, const int *ids, const int *ref_slots);
/* On a graph with refresh state orbfe_covis_add_keyframe_device / orbfe_covis_add_keyframe run one more launch behind their own: every
 * feature slot i with d_added[i] == 1 stores i as the index of the observation that was just appended.  The key frame's features are
 * set with set_features* before the refresh call; the order relative to add_keyframe does not matter.
 *
 * Reads one point back to HOST memory, waiting for the handle's stream: *n_obs, kf_slots / feat_idx (obs_stride ints each, the first
 * *n_obs are the list), *ref_slot, and the record and the 32 descriptor bytes of the graph's map (point / desc, either may be NULL).
 * ORBFE_ERR_INVALID_ARG: a NULL among the first four outputs, an id outside the map, a graph without refresh state. */
int orbfe_covis_get_point(orbfe_handle *h, orbfe_covis *g, int id, int *n_obs, int *kf_slots, int *feat_idx, int *ref_slot,
                          orbfe_world_point *point, uint8_t *desc);

/* The outputs of orbfe_covis_refresh_points_device: DEVICE pointers, one element per list entry, any of them may be NULL.  Every
 * entry of the list gets every output: one that was not processed, or whose bit is clear, reads status 0, distances 0.0f, slot /
 * index / median -1.  Versioned by struct_size. */
typedef struct orbfe_refresh_io {
    int struct_size;          /* sizeof(orbfe_refresh_io) at the caller's compile time */
    int reserved;             /* 0 */
    int *d_status;            /* bit 0: the distances were written; bit 1: the descriptor was written; 0: nothing happened */
    float *d_min_distance;    /* mfMinDistance as written */
    float *d_max_distance;    /* mfMaxDistance as written */
    int *d_best_slot;         /* the observer the descriptor came from */
    int *d_best_index;        /* its feature */
    int *d_best_median;       /* BestMedian (:408) */
} orbfe_refresh_io;

/* UpdateDepth (what & 1) and / or ComputeDistinctiveDescriptors (what & 2) for the points d_ids[0 .. n), a DEVICE list; an id outside
 * the map is no point.  d_select (DEVICE, may be NULL): entry i is processed only if d_select[i] == select_value -- the point row
 * given to orbfe_covis_add_keyframe_device with its d_added and 1 is LocalMapping::ProcessNewKeyFrame's :350-351 with no host in
 * between.  The call WRITES min_distance / max_distance and the descriptor of the graph's own orbfe_map records; bad, observations,
 * skip and the position are not touched.  The caller orders it against the chains that read the map exactly as it orders
 * orbfe_map_update: on the stream of those chains, or behind an event.  Asynchronous on `stream`, no host synchronisation, two
 * launches, no allocation beyond a list of n ints kept with the graph that grows to the largest n seen.
 *   both        a point whose map record is bad or whose observation list is empty is left alone (:352, :357, :448, :455).
 *   descriptor  collected: the observers that are not bad (:366) and whose index is not -1 (:370) and names a feature of the key frame
 *               (below the count of its set_features); none collected: nothing written.  With N collected, row i is the N Hamming
 *               distances from i, its own 0 included; its median is the element at position (size_t)(0.5 * (N - 1)) of the sorted
 *               row; the descriptor with the least median is copied to the map.  Among equal medians the observer with the lowest
 *               mn_id wins (S26: mn_id stands for the address the reference's map iterates by), then the earlier in the list.
 *   depth       r = the point's reference slot; dist = sqrt((x x + y y) + z z) of Pos - centre[r] in binary32, every operation
 *               rounded once; max = dist * sf[level], min = max / sf[n_levels - 1]; level = the octave of r's feature at the index
 *               of r's observation.  r not among the observers: index 0, as written (:461 default-constructs).  r is not tested for
 *               bad.  Undefined in the reference, here nothing written and bit 0 clear: r outside [0, kf_capacity), an index of -1,
 *               an index at or beyond r's feature count.
 * An id named twice gets the same values written twice.  Results do not depend on n, on the order of the list or on the arrival
 * order of any atomic.  Points with at most 64 observers take one wave each; the others a block each in the second launch.
 * ORBFE_ERR_INVALID_ARG: a NULL (h, g, d_ids, io), a wrong struct_size, n < 1, what outside 1..3, a graph of another handle, whose map
 * is gone or without refresh state; all decided before the device is touched. */
int orbfe_covis_refresh_points_device(orbfe_handle *h, orbfe_covis *g, int n, const int *d_ids, const int *d_select, int select_value,
                                      int what, const orbfe_refresh_io *io, void *stream);
/* The same from a HOST list with HOST outputs (n elements each, any may be NULL): one upload, the same launches, one download, one
 * synchronisation.  Results equal the device call's. */
int orbfe_covis_refresh_points(orbfe_handle *h, orbfe_covis *g, int n, const int *ids, int what, int *status, float *min_distance,
                               float *max_distance, int *best_slot, int *best_index, int *best_median);

/* -------------------------------------------------------------------------------------------
 * Bundle adjustment of the initial map: the line behind orbfe_two_view_reconstruct (src/Tracking.cc:698)
 * ---------------------------------------------------------------------------------------- */
/* the camera and the constants of Optimizer::GlobalBundleAdjustemnt(map, 20) (src/Optimizer.cc:60-369); versioned by struct_size */
typedef struct orbfe_initial_ba_params {
    int struct_size;          /* sizeof(orbfe_initial_ba_params) at the caller's compile time */
    int camera_model;         /* ORBFE_CAMERA_PINHOLE; ORBFE_CAMERA_KANNALA_BRANDT8 -> ORBFE_ERR_UNSUPPORTED */
    float cam[8];             /* fx fy cx cy k1 k2 k3 k4 (mvParameters; only the first four are read) */
    double huber_delta2;      /* thHuber2D = (float) sqrt(5.99) (:139; 5.99, not 5.991): > 0 */
    int robust;               /* bRobust (:185): 1 = every edge carries the Huber kernel, 0 = none does */
    int iterations;           /* nIterations, 20 (src/Tracking.cc:698): [1, 64] */
    int stereo;               /* 0; anything else (mvuRight >= 0, the ToBody edges) -> ORBFE_ERR_UNSUPPORTED */
} orbfe_initial_ba_params;
#define ORBFE_INITIAL_BA_PARAMS_INIT {(int)sizeof(orbfe_initial_ba_params), 0, {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 5.99, 1, 20, 0}

/* every intermediate of one orbfe_initial_bundle_adjustment call (optional: info may be NULL).  Point p is the p-th i, ascending,
 * with matches12[i] >= 0; edge 0 of a point is its observation in key frame 1, edge 1 the one in key frame 2.  Entries of
 * iterations that did not run are zero. */
typedef struct orbfe_initial_ba_info {
    int struct_size;          /* sizeof(orbfe_initial_ba_info) at the caller's compile time */
    int N;                    /* points */
    int n_iterations;         /* Levenberg iterations started */
    int n_trials;             /* damped solves tried, all iterations */
    int exit_kind;            /* ORBFE_POSE_OPT_EXIT_* */
    int trials[64];           /* damped solves tried in the iteration */
    double cost[64];          /* the sum of rho0 the iteration ended with (its last accepted trial's, else its build's) */
    double lambda[64];        /* the damping the iteration ended with */
    double pose[12];          /* the final pose 2: R (9, row-major) then t (3) in binary64 */
    double *chi2;             /* [2][N], caller-owned, may be NULL: chi2 of every edge at the final estimate, edge-major */
    uint8_t *depth_positive;  /* [2][N], caller-owned, may be NULL: isDepthPositive() of every edge at the final estimate */
} orbfe_initial_ba_info;

/* replaces Optimizer::GlobalBundleAdjustemnt(mpAtlas->GetCurrentMap(), 20) in CreateInitialMapMonocular (src/Tracking.cc:698 ->
 * src/Optimizer.cc:60-369), the only BundleAdjustment call this fork has: two key frames of which the first is fixed (:133), N map
 * points each observed once in either frame, EdgeSE3ProjectXYZ, pinhole, one Levenberg run with a Huber kernel and no outlier
 * rounds.  Numerics: SPEC DECISION S17; tests/initial_ba_ref.py is the normative restatement and the call
 * equals it byte for byte.
 * kp1 (n1) / kp2 (n2) = the two key frames' mvKeysUn (x, y, octave are read; the handle's mvInvLevelSigma2 is the information);
 * matches12 (n1) = vIniMatches (an index into kp2, or negative); points (n1 x 3 floats) = vIniP3D, read where matches12[i] >= 0.
 * Rcw1 / tcw1 = the fixed pose of key frame 1, Rcw2 / tcw2 = the start of key frame 2's (9 row-major / 3 floats each).
 * Tcw2_out (16, row-major) = the adjusted pose of key frame 2; points_out (n1 x 3) = the adjusted points, rows with
 * matches12[i] < 0 as they went in (points_out may be `points`).  The call returns values: where the reference puts them
 * (SetPose / SetWorldPos, or mTcwGBA / mPosGBA from the second map on) is the caller's matter, see INTEGRATION.md.
 * No match at all: ORBFE_OK, the outputs equal the inputs, nothing is launched.  That return and every refusal below are
 * decided from the arguments and the handle's level count before the device is touched.
 * The whole call -- every iteration and every trial -- is ONE kernel launch of one block; one submission, one synchronisation.
 * HOST pointers.
 * ORBFE_ERR_INVALID_ARG: a wrong struct_size (params or info), a parameter outside its range, a match >= n2, an octave of a
 * matched keypoint (either frame) outside the handle's levels, n1 or n2 > 65536.  ORBFE_ERR_UNSUPPORTED: KannalaBrandt8 (for
 * S14's reason), stereo != 0; more than two key frames and a free first pose are not offered at all.
 * NOT the reference's function in these stated respects: g2o is an empty submodule in the reference tree, so the
 * Levenberg loop, the Schur complement over the points and SE3Quat::exp are restated from the published algorithm (parity with
 * a g2o build is unpinned, as in S14); the poses are kept as matrices and take no quaternion round trip -- pose 1 is returned by
 * nobody, where the reference writes it back through a quaternion; the reference's edge order follows a std::map keyed by
 * pointer, here edge 0 comes first. */
int orbfe_initial_bundle_adjustment(orbfe_handle *h, const orbfe_initial_ba_params *p, int n1, const orbfe_keypoint *kp1, int n2,
                                    const orbfe_keypoint *kp2, const int *matches12, const float *points, const float *Rcw1,
                                    const float *tcw1, const float *Rcw2, const float *tcw2, float *Tcw2_out, float *points_out,
                                    orbfe_initial_ba_info *info);

/* -------------------------------------------------------------------------------------------
 * Multi-device pool: the batched many-frame mode with host frames, sharded over several GPUs
 * ---------------------------------------------------------------------------------------- */
/* A pool owns N members.  Member k is a handle made from *params with device_id = devices[k] (params->device_id is ignored),
 * plus one ring (orbfe_stream_*) of `slots` x `slot_frames`.  A device may appear more than once: two members on one GPU are
 * two handles with two rings.  Each MI355X has its own host link, so host frames go faster only with more devices; the
 * members' results travel down their own links straight into the caller's arrays, nothing is gathered through one device.
 * Sharding: frame i belongs to the member k whose orbfe_shard_range block holds i.  Each member pushes its block through its
 * own ring in chunks of slot_frames, on a worker thread of its own (one per member, made at create, joined at destroy):
 * it submits until the ring is full, then collects the oldest submission into the caller's arrays at the frames' absolute
 * offsets.  All members run at the same time; the calling thread sleeps until the last one is done.  A member whose block
 * is empty does nothing.
 * Outputs: exactly orbfe_extract_batch's layout with cap = orbfe_max_keypoints(orbfe_pool_member(p, 0)): frame i at
 * kp_out + i*cap, desc_out + i*cap*32, n_out[i], per_level_counts + i*n_levels (per_level_counts may be NULL) and, for
 * orbfe_pool_track, match_out + i*cap and n_matches[i].  Only the first n_out[i] entries of a frame are written.
 * Results are byte-identical to the single-handle calls whatever the member count and whether or not devices repeat.
 * Errors: argument errors are found on the calling thread before any member starts: ORBFE_ERR_INVALID_ARG, no output
 * written, no GPU work done.  A runtime failure (a HIP error, device guard flags at collect) lets every member first wait
 * for and drop what it submitted; the call then returns the status of the lowest-numbered failing member and
 * orbfe_pool_last_error() reads "member k (device d): <orbfe_last_error of that member>".  The pool stays usable.
 * Threading: one caller at a time per pool, as for a handle.  The calls are synchronous: source frames may be reused once
 * a call has returned.  Sources as for the ring: pinned frames are read in place by DMA, pageable ones go through a pool of
 * copy threads (max(1, 7 / n_devices) per member, so a pool takes no more threads than one ring). */
typedef struct orbfe_pool orbfe_pool;

/* host-only: the contiguous block [*lo, *hi) of n_frames that member k of n_members owns -- ceil(n_frames / n_members)
 * frames each, the first members take the remainder and the last ones may be empty; the same arithmetic as shard_range()
 * in python/orbfe/shard.py.  n_frames >= 0, 1 <= n_members, 0 <= k < n_members. */
int orbfe_shard_range(int n_frames, int k, int n_members, int *lo, int *hi);

/* 1 <= n_devices <= 16, 2 <= slots <= 64, 1 <= slot_frames <= params->max_batch.  A NULL pointer or a count or ordinal that
 * is negative or out of range gives ORBFE_ERR_INVALID_ARG before any HIP call; no GPU at all gives ORBFE_ERR_NO_DEVICE; an
 * ordinal >= the device count gives ORBFE_ERR_INVALID_ARG.  If a member fails to create, everything created so far is
 * released and that member's status is returned. */
int orbfe_pool_create(const orbfe_params *params, const int *devices, int n_devices, int slots, int slot_frames,
                      orbfe_pool **out);
/* joins the workers, then releases every member's ring, map and handle.  NULL is a no-op. */
void orbfe_pool_destroy(orbfe_pool *p);
int orbfe_pool_size(const orbfe_pool *p);
/* member k's handle, borrowed: for the getters (orbfe_max_keypoints, scale tables, level info, orbfe_last_error).  Other
 * calls on it only while the pool is idle; never orbfe_destroy it. */
orbfe_handle *orbfe_pool_member(const orbfe_pool *p, int k);
/* frames member k has processed since create */
long long orbfe_pool_member_frames(const orbfe_pool *p, int k);
/* message of the pool's last failing call ("" if none) */
const char *orbfe_pool_last_error(const orbfe_pool *p);

/* orbfe_extract_batch over n_frames (>= 1) host frames `pitch` bytes per row, any number of them (no max_batch limit). */
int orbfe_pool_extract(orbfe_pool *p, const uint8_t *const *grays, int pitch, int n_frames,
                       orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out, int *per_level_counts);

/* one orbfe_map of map_capacity per member, and orbfe_stream_enable_track(max_points) on every ring.  Once per pool: a
 * second call (or one while a pool call runs) gives ORBFE_ERR_INVALID_ARG.  Out of memory on any member releases what this
 * call made and leaves the pool as it was; the call may be repeated. */
int orbfe_pool_enable_track(orbfe_pool *p, int map_capacity, int max_points);
/* orbfe_map_update of the same entries on every member's map, the members in parallel; returns when all of them are
 * updated, so it is ordered before the next orbfe_pool_track.  ORBFE_ERR_INVALID_ARG before orbfe_pool_enable_track. */
int orbfe_pool_map_update(orbfe_pool *p, int n, const int *ids, const orbfe_world_point *points, const uint8_t *desc);
/* per frame i, what orbfe_track_frame_map(h, grays[i], pitch, &frusta[i], tp, map, n_points, ids + i*n_points, ...) gives
 * on one handle whose map holds the same entries: frusta[i] is frame i's pose, ids[i*n_points ..] its local map points
 * (id >= 0, ~id = skipped, outside the map = no point, as orbfe_stream_submit_track); n_points <= max_points.  Outputs as
 * orbfe_pool_extract plus match_out + i*cap / n_matches[i] as orbfe_stream_collect_track.  ORBFE_ERR_INVALID_ARG before
 * orbfe_pool_enable_track. */
int orbfe_pool_track(orbfe_pool *p, const uint8_t *const *grays, int pitch, int n_frames, const orbfe_track_params *tp,
                     const orbfe_frustum *frusta, int n_points, const int *ids,
                     orbfe_keypoint *kp_out, uint8_t *desc_out, int *n_out, int *per_level_counts,
                     int *match_out, int *n_matches);

/* -------------------------------------------------------------------------------------------
 * Misc
 * ---------------------------------------------------------------------------------------- */
const char *orbfe_status_string(int status);
/* The host-pointer entry points capture their launch sequence into a hipGraph the first time a shape is seen (on a throw-away
 * stream) and replay it afterwards.  On ROCm 7.2 a NULL-stream operation of ANOTHER thread of the process (a plain hipMemcpy /
 * hipMemset of the application) that meets a capture in flight is refused by the runtime with hipErrorStreamCaptureImplicit
 * and kills the capture: the library call then runs on plain launches and is unaffected, but the application's call has
 * failed.  An application that uses the NULL stream from other threads can switch capturing off (enable = 0: plain launches,
 * about 0.04 ms more per single-frame call) or make its first call of every shape before those threads start.  The
 * library itself never uses the NULL stream. */
int orbfe_set_graph_capture(orbfe_handle *h, int enable);
/* Priority of the handle's own HIP stream (the one every host-pointer entry point and every `stream == NULL` call runs on).
 * The reference runs tracking and local mapping on two threads (src/System.cc); with one handle each, high = 1 on the tracking
 * thread's handle lets its kernels be dispatched ahead of the mapping thread's whenever both have work queued (running waves
 * are not pre-empted).  The stream is re-created: call it while the handle is idle (nothing submitted and not yet collected),
 * typically right after orbfe_create.  high = 0 selects the lowest priority of the device's range. */
int orbfe_set_stream_priority(orbfe_handle *h, int high);
/* diagnostics: graphs this handle has captured so far, and captures that failed (e.g. invalidated by another thread's NULL-stream
 * call: the affected call ran on plain launches, its result is unaffected; after 8 failures IN A ROW a handle stops capturing
 * until orbfe_set_graph_capture(h, 1)) */
int orbfe_debug_graph_stats(orbfe_handle *h, int *captured, int *failed);
/* diagnostics (bench.py's `sustained.sclk_mhz`): one wave on `stream` (NULL == the handle's stream; asynchronous) stamps the shader-cycle
 * counter and the constant 100 MHz counter, sleeps for spin_us microseconds and stamps again: d_out[0] = shader cycles, d_out[1] =
 * 100 MHz ticks that went by (DEVICE pointer to two 64-bit words), i.e. the clock the chip held meanwhile is d_out[0] / d_out[1] x
 * 100 MHz.  Launched on a stream of its own beside a running workload it reads the clock THAT workload runs at. */
int orbfe_debug_clock_probe(orbfe_handle *h, int spin_us, unsigned long long *d_out, void *stream);
/* message of the last failing HIP call on this handle ("" if none) */
const char *orbfe_last_error(const orbfe_handle *h);
/* library / build identification, e.g. "orbfe 0.1 gfx950" */
const char *orbfe_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H */

"""orbfe -- ctypes binding of liborbfe.so (include/orbfe.h) with the reference's class names.

`ORBextractor` / `ORBmatcher` mirror include/ORBextractor.h:52-130 and include/ORBmatcher.h:36-84 of
geoeo/ORB_SLAM3_V1.0 (same constructor arguments, same method names, same results) so the parity
tests read like calls into the reference.  This module is plumbing: every result comes from the
HIP kernels behind the C ABI.  There is NO CPU fallback -- if liborbfe.so is missing or no gfx950
device is present the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.normpath(os.path.join(_HERE, "..", "..", "csrc"))
LIB_PATH = os.path.join(CSRC, "liborbfe.so")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"),
                     ("octave", "<i4"), ("angle", "<f4")])
MP_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("view_cos", "<f4"), ("track_depth", "<f4"),
                     ("level", "<i4"), ("in_view", "<i4"), ("bad", "<i4"), ("observations", "<i4")])
WP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("min_distance", "<f4"), ("max_distance", "<f4"),
                     ("bad", "<i4"), ("observations", "<i4"), ("skip", "<i4")])
NUM_STAGES = 5

STATUS = {0: "ORBFE_OK", 1: "ORBFE_ERR_INVALID_ARG", 2: "ORBFE_ERR_UNSUPPORTED", 3: "ORBFE_ERR_NO_DEVICE",
          4: "ORBFE_ERR_HIP", 5: "ORBFE_ERR_OUT_OF_MEMORY", 6: "ORBFE_ERR_INTERNAL", 7: "ORBFE_ERR_BUSY"}
ERR_INVALID_ARG, ERR_UNSUPPORTED = 1, 2
ERR_BUSY = 7


class OrbfeError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        super().__init__("%s: %s (%d) %s" % (where, STATUS.get(code, "?"), code, detail))


class Params(C.Structure):
    _fields_ = [("n_features", C.c_int), ("n_fast_features", C.c_int), ("scale_factor", C.c_float),
                ("n_levels", C.c_int), ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int),
                ("image_width", C.c_int), ("image_height", C.c_int), ("device_id", C.c_int),
                ("max_batch", C.c_int)]


class Frustum(C.Structure):
    """orbfe_frustum: what Frame::isInFrustum reads from the frame (src/Frame.cc:272-331)."""
    _fields_ = [("rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("twc", C.c_float * 3), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float),
                ("k4", C.c_float), ("mbf", C.c_float), ("log_scale_factor", C.c_float),
                ("n_levels", C.c_int), ("camera_model", C.c_int)]


class Sim3View(C.Structure):
    """orbfe_sim3_view: one search direction of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:977-1200)."""
    _fields_ = [("rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("sr", C.c_float * 9), ("t", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("log_scale_factor", C.c_float),
                ("n_levels", C.c_int)]


class TriParams(C.Structure):
    """orbfe_tri_params: F12, epipole and the three flags of SearchForTriangulation."""
    _fields_ = [("struct_size", C.c_int), ("f12", C.c_float * 9), ("ep_x", C.c_float), ("ep_y", C.c_float), ("only_stereo", C.c_int),
                ("coarse", C.c_int), ("check_orientation", C.c_int),
                ("camera_model1", C.c_int), ("camera_model2", C.c_int), ("cam1", C.c_float * 8), ("cam2", C.c_float * 8),
                ("kb_precision", C.c_float), ("r12", C.c_float * 9), ("t12", C.c_float * 3),
                ("level_sigma2_1", C.c_float * 32), ("kf1_has_camera2", C.c_int)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TriParams)


def fill_tri_cameras(P, cameras):
    """copy a cameras dict (see ORBmatcher.SearchForTriangulation) into the tail of an orbfe_tri_params"""
    P.camera_model1, P.camera_model2 = int(cameras["model1"]), int(cameras["model2"])
    for i in range(8):
        P.cam1[i] = float(cameras["cam1"][i])
        P.cam2[i] = float(cameras["cam2"][i])
    P.kb_precision = float(cameras.get("precision", 1e-6))
    for i, v in enumerate(np.asarray(cameras["R12"], np.float32).reshape(-1)):
        P.r12[i] = float(v)
    for i, v in enumerate(np.asarray(cameras["t12"], np.float32).reshape(-1)):
        P.t12[i] = float(v)
    for i, v in enumerate(np.asarray(cameras["levelSigma2_1"], np.float32).reshape(-1)):
        P.level_sigma2_1[i] = float(v)
    P.kf1_has_camera2 = int(cameras.get("kf1HasCamera2", 0))


class NewPointParams(C.Structure):
    """orbfe_newpoint_params: what "triangulate each match" of LocalMapping::CreateNewMapPoints reads for one key-frame pair."""
    _fields_ = [("struct_size", C.c_int), ("tcw1", C.c_float * 12), ("tcw2", C.c_float * 12), ("twc1", C.c_float * 3),
                ("twc2", C.c_float * 3), ("camera_model1", C.c_int), ("camera_model2", C.c_int), ("cam1", C.c_float * 8),
                ("cam2", C.c_float * 8), ("kb_precision", C.c_float), ("level_sigma2_1", C.c_float * 32),
                ("level_sigma2_2", C.c_float * 32), ("ratio_factor", C.c_float), ("inertial", C.c_int), ("far_points", C.c_int),
                ("th_far_points", C.c_float)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(NewPointParams)


# verdict bytes of orbfe_create_new_points_batch / orbfe_triangulate_pairs (ORBFE_NEWPT_*)
NEWPT_ACCEPTED, NEWPT_LOW_PARALLAX, NEWPT_AT_INFINITY, NEWPT_BEHIND_1, NEWPT_BEHIND_2 = 0, 1, 2, 3, 4
NEWPT_REPROJECTION_1, NEWPT_REPROJECTION_2, NEWPT_ZERO_DISTANCE, NEWPT_FAR, NEWPT_SCALE, NEWPT_NO_PARTNER = 5, 6, 7, 8, 9, 255


def newpoint_params(Tcw1, Tcw2, twc1, twc2, levelSigma2_1, levelSigma2_2, ratioFactor, model1=0, model2=0, cam1=None, cam2=None,
                    precision=1e-6, inertial=False, farPoints=False, thFarPoints=0.0):
    """orbfe_newpoint_params of one pair: Tcw = GetPose().matrix3x4() (3 x 4), twc = GetTranslationInverse(), cam = fx fy cx cy
    k1 k2 k3 k4, ratioFactor = 1.5f * mfScaleFactor"""
    P = NewPointParams()
    for dst, src, n in ((P.tcw1, Tcw1, 12), (P.tcw2, Tcw2, 12), (P.twc1, twc1, 3), (P.twc2, twc2, 3), (P.cam1, cam1, 8),
                        (P.cam2, cam2, 8), (P.level_sigma2_1, levelSigma2_1, None), (P.level_sigma2_2, levelSigma2_2, None)):
        if src is None:
            continue
        v = np.asarray(src, np.float32).reshape(-1)
        assert n is None or len(v) == n
        for i, x in enumerate(v):
            dst[i] = float(x)
    P.camera_model1, P.camera_model2 = int(model1), int(model2)
    P.kb_precision = float(precision)
    P.ratio_factor = float(np.float32(ratioFactor))
    P.inertial, P.far_points, P.th_far_points = int(inertial), int(farPoints), float(np.float32(thFarPoints))
    return P


class TwoViewParams(C.Structure):
    """orbfe_two_view_params: K, mSigma, mMaxIterations and the two constants of TwoViewReconstruction::Reconstruct."""
    _fields_ = [("struct_size", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("sigma", C.c_float), ("iterations", C.c_int), ("min_parallax_deg", C.c_float), ("min_triangulated", C.c_int)]

    def __init__(self, fx=0.0, fy=0.0, cx=0.0, cy=0.0, sigma=1.0, iterations=200, min_parallax_deg=1.0, min_triangulated=50):
        super().__init__(C.sizeof(TwoViewParams), fx, fy, cx, cy, sigma, iterations, min_parallax_deg, min_triangulated)


class TwoViewInfo(C.Structure):
    """orbfe_two_view_info: every intermediate of one orbfe_two_view_reconstruct call."""
    _fields_ = [("struct_size", C.c_int), ("n_matches", C.c_int), ("SH", C.c_float), ("SF", C.c_float), ("RH", C.c_float),
                ("model", C.c_int), ("exit_line", C.c_int), ("H21", C.c_float * 9), ("F21", C.c_float * 9),
                ("best_it_H", C.c_int), ("best_it_F", C.c_int), ("n_hypotheses", C.c_int), ("best_hypothesis", C.c_int),
                ("n_good", C.c_int * 8), ("cos_parallax", C.c_float * 8), ("hyp_R", C.c_float * 72), ("hyp_t", C.c_float * 24),
                ("scores", C.c_void_p), ("inliers_H", C.c_void_p), ("inliers_F", C.c_void_p), ("rt_flags", C.c_void_p),
                ("rt_x3d", C.c_void_p), ("rt_cos", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TwoViewInfo)


TWO_VIEW_MODEL_NONE, TWO_VIEW_MODEL_HOMOGRAPHY, TWO_VIEW_MODEL_FUNDAMENTAL = 0, 1, 2


class MlpnpParams(C.Structure):
    """orbfe_mlpnp_params: the frame's camera, the arguments of MLPnPsolver::SetRansacParameters and iterate's nIterations."""
    _fields_ = [("struct_size", C.c_int), ("camera_model", C.c_int), ("cam", C.c_float * 8), ("kb_precision", C.c_float),
                ("probability", C.c_double), ("min_inliers", C.c_int), ("max_iterations", C.c_int), ("min_set", C.c_int),
                ("epsilon", C.c_float), ("th2", C.c_float), ("n_iterations", C.c_int)]

    def __init__(self, cam=(0.0,) * 8, camera_model=0, kb_precision=1e-6, probability=0.95, min_inliers=50, max_iterations=300,
                 min_set=12, epsilon=0.5, th2=5.991, n_iterations=20):
        super().__init__(C.sizeof(MlpnpParams), int(camera_model), (C.c_float * 8)(*[float(x) for x in cam]), kb_precision, probability,
                         min_inliers, max_iterations, min_set, epsilon, th2, n_iterations)


class MlpnpInfo(C.Structure):
    """orbfe_mlpnp_info: every intermediate of one orbfe_mlpnp_ransac call."""
    _fields_ = [("struct_size", C.c_int), ("N", C.c_int), ("min_inliers", C.c_int), ("max_its", C.c_int), ("total_iterations", C.c_int),
                ("exit_kind", C.c_int), ("returning_iteration", C.c_int), ("n_candidates", C.c_int), ("hyp_Rt", C.c_void_p),
                ("hyp_inliers", C.c_void_p), ("hyp_planar", C.c_void_p), ("hyp_gn_evals", C.c_void_p), ("hyp_gn_exit", C.c_void_p),
                ("candidates", C.c_void_p), ("cand_Rt", C.c_void_p), ("cand_inliers", C.c_void_p), ("cand_planar", C.c_void_p),
                ("cand_mask", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(MlpnpInfo)


MLPNP_EXIT_ABORT, MLPNP_EXIT_REFINED, MLPNP_EXIT_BEST_UNREFINED, MLPNP_EXIT_FAILED = 0, 1, 2, 3


class PoseOptParams(C.Structure):
    """orbfe_pose_opt_params: the frame's camera and the constants of Optimizer::PoseOptimization (src/Optimizer.cc:765-1067)."""
    _fields_ = [("struct_size", C.c_int), ("camera_model", C.c_int), ("cam", C.c_float * 8), ("chi2_threshold", C.c_float),
                ("huber_delta2", C.c_double), ("iterations", C.c_int), ("rounds", C.c_int), ("stereo", C.c_int)]

    def __init__(self, cam=(0.0,) * 8, camera_model=0, chi2_threshold=5.991, huber_delta2=7.815, iterations=25, rounds=4, stereo=0):
        super().__init__(C.sizeof(PoseOptParams), int(camera_model), (C.c_float * 8)(*[float(x) for x in cam]), chi2_threshold,
                         huber_delta2, iterations, rounds, stereo)


class PoseOptInfo(C.Structure):
    """orbfe_pose_opt_info: every intermediate of one orbfe_pose_optimization call."""
    _fields_ = [("struct_size", C.c_int), ("N_e", C.c_int), ("rounds_run", C.c_int), ("iterations", C.c_int * 4), ("trials", C.c_int * 4),
                ("n_bad", C.c_int * 4), ("exit_kind", C.c_int * 4), ("pose", (C.c_double * 12) * 4), ("lambda_", C.c_double * 4),
                ("chi2", C.c_double * 4), ("outlier", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(PoseOptInfo)


POSE_OPT_EXIT_RAN_ALL, POSE_OPT_EXIT_TRIALS, POSE_OPT_EXIT_RHO_ZERO = 0, 1, 2


class PoseInertialParams(C.Structure):
    """orbfe_pose_inertial_params: the frame's camera and the constants of Optimizer::PoseInertialOptimizationLastKeyFrame
    (src/Optimizer.cc:3447-3844)."""
    _fields_ = [("struct_size", C.c_int), ("camera_model", C.c_int), ("cam", C.c_float * 8), ("chi2", C.c_float * 4),
                ("close_factor", C.c_double), ("close_depth", C.c_float), ("recover_chi2", C.c_float), ("recover_below", C.c_int),
                ("iterations", C.c_int), ("rounds", C.c_int), ("rec_init", C.c_int), ("huber_delta2", C.c_double), ("gravity", C.c_float),
                ("stereo", C.c_int)]

    def __init__(self, cam=(0.0,) * 8, camera_model=0, chi2=(12.0, 7.5, 5.991, 5.991), close_factor=1.5, close_depth=10.0,
                 recover_chi2=24.0, recover_below=30, iterations=15, rounds=4, rec_init=0, huber_delta2=5.991, gravity=9.81, stereo=0):
        super().__init__(C.sizeof(PoseInertialParams), int(camera_model), (C.c_float * 8)(*[float(x) for x in cam]),
                         (C.c_float * 4)(*[float(x) for x in chi2]), close_factor, close_depth, recover_chi2, int(recover_below),
                         int(iterations), int(rounds), int(rec_init), huber_delta2, gravity, int(stereo))


class ImuLink(C.Structure):
    """orbfe_imu_link: the fixed last key frame's state, the preintegrated constants and informations the caller computes with the
    reference's code, and the camera-body extrinsics.  Built from a dict of arrays named like the fields."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("Rwb1", C.c_float * 9), ("twb1", C.c_float * 3), ("v1", C.c_float * 3),
                ("bg1", C.c_float * 3), ("ba1", C.c_float * 3), ("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3),
                ("dt", C.c_float), ("Rcb", C.c_float * 9), ("tcb", C.c_float * 3), ("tbc", C.c_float * 3), ("info9", C.c_double * 81),
                ("infoG", C.c_double * 9), ("infoA", C.c_double * 9)]

    def __init__(self, link=None):
        super().__init__()
        self.struct_size = C.sizeof(ImuLink)
        if link is None:
            return
        for name, ctype in self._fields_[2:]:
            if name == "dt":
                self.dt = float(link[name])
            else:
                setattr(self, name, ctype(*[float(x) for x in np.asarray(link[name]).reshape(-1)]))


class PoseInertialInfo(C.Structure):
    """orbfe_pose_inertial_info: every intermediate of one orbfe_pose_inertial_optimization_last_keyframe call."""
    _fields_ = [("struct_size", C.c_int), ("N_e", C.c_int), ("rounds_run", C.c_int), ("recovered", C.c_int), ("iterations", C.c_int * 4),
                ("ok", C.c_int * 4), ("n_bad", C.c_int * 4), ("state", (C.c_double * 21) * 4), ("outlier", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(PoseInertialInfo)


class PoseInertialPrevParams(C.Structure):
    """orbfe_pose_inertial_prev_params: the frame's camera and the constants of Optimizer::PoseInertialOptimizationLastFrame
    (src/Optimizer.cc:3846-4275)."""
    _fields_ = [("struct_size", C.c_int), ("camera_model", C.c_int), ("cam", C.c_float * 8), ("chi2", C.c_float * 4),
                ("close_factor", C.c_double), ("close_depth", C.c_float), ("recover_chi2", C.c_float), ("recover_below", C.c_int),
                ("iterations", C.c_int), ("rounds", C.c_int), ("rec_init", C.c_int), ("huber_delta2", C.c_double),
                ("prior_huber_delta", C.c_double), ("inlier_threshold", C.c_int), ("gravity", C.c_float), ("stereo", C.c_int),
                ("reserved", C.c_int)]

    def __init__(self, cam=(0.0,) * 8, camera_model=0, chi2=(5.991, 5.991, 5.991, 5.991), close_factor=1.5, close_depth=10.0,
                 recover_chi2=24.0, recover_below=30, iterations=15, rounds=4, rec_init=0, huber_delta2=5.991, prior_huber_delta=5.0,
                 inlier_threshold=8, gravity=9.81, stereo=0):
        super().__init__(C.sizeof(PoseInertialPrevParams), int(camera_model), (C.c_float * 8)(*[float(x) for x in cam]),
                         (C.c_float * 4)(*[float(x) for x in chi2]), close_factor, close_depth, recover_chi2, int(recover_below),
                         int(iterations), int(rounds), int(rec_init), huber_delta2, prior_huber_delta, int(inlier_threshold), gravity,
                         int(stereo), 0)


class ImuLinkFree(C.Structure):
    """orbfe_imu_link_free: the previous frame's state, the preintegration at its own bias with its bias Jacobians, the informations
    and the camera-body extrinsics.  Built from a dict of arrays named like the fields."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("Rwb1", C.c_float * 9), ("twb1", C.c_float * 3), ("v1", C.c_float * 3),
                ("bg1", C.c_float * 3), ("ba1", C.c_float * 3), ("dR0", C.c_float * 9), ("dV0", C.c_float * 3), ("dP0", C.c_float * 3),
                ("bg0", C.c_float * 3), ("ba0", C.c_float * 3), ("JRg", C.c_float * 9), ("JVg", C.c_float * 9), ("JVa", C.c_float * 9),
                ("JPg", C.c_float * 9), ("JPa", C.c_float * 9), ("dt", C.c_float), ("Rcb", C.c_float * 9), ("tcb", C.c_float * 3),
                ("tbc", C.c_float * 3), ("reserved2", C.c_float), ("info9", C.c_double * 81), ("infoG", C.c_double * 9),
                ("infoA", C.c_double * 9)]

    def __init__(self, link=None):
        super().__init__()
        self.struct_size = C.sizeof(ImuLinkFree)
        if link is None:
            return
        for name, ctype in self._fields_[2:]:
            if name == "reserved2":
                continue
            if name == "dt":
                self.dt = float(link[name])
            else:
                setattr(self, name, ctype(*[float(x) for x in np.asarray(link[name]).reshape(-1)]))


class PoseImuPrior(C.Structure):
    """orbfe_pose_imu_prior: ConstraintPoseImu of the previous frame.  Built from a dict of arrays named like the fields."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("Rwb", C.c_double * 9), ("twb", C.c_double * 3), ("vwb", C.c_double * 3),
                ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("H", C.c_double * 225)]

    def __init__(self, prior=None):
        super().__init__()
        self.struct_size = C.sizeof(PoseImuPrior)
        if prior is None:
            return
        for name, ctype in self._fields_[2:]:
            setattr(self, name, ctype(*[float(x) for x in np.asarray(prior[name], np.float64).reshape(-1)]))


class PoseInertialPrevInfo(C.Structure):
    """orbfe_pose_inertial_prev_info: every intermediate of one orbfe_pose_inertial_optimization_last_frame call."""
    _fields_ = [("struct_size", C.c_int), ("N_e", C.c_int), ("rounds_run", C.c_int), ("recovered", C.c_int), ("iterations", C.c_int * 4),
                ("ok", C.c_int * 4), ("n_bad", C.c_int * 4), ("state", (C.c_double * 42) * 4), ("prior_chi2", C.c_double * 4),
                ("prior_weight", C.c_double * 4), ("outlier", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(PoseInertialPrevInfo)


class ImuNoise(C.Structure):
    """orbfe_imu_noise: the diagonals of Calib::Cov and Calib::CovWalk (gyro x 3, accelerometer x 3 each)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int), ("cov", C.c_float * 6), ("cov_walk", C.c_float * 6)]

    def __init__(self, cov=(0.0,) * 6, cov_walk=(0.0,) * 6):
        super().__init__(C.sizeof(ImuNoise), 0, (C.c_float * 6)(*[float(x) for x in cov]), (C.c_float * 6)(*[float(x) for x in cov_walk]))


IMU_SAMPLE_DTYPE = np.dtype([("t", "<f8"), ("a", "<f4", 3), ("w", "<f4", 3)])            # orbfe_imu_sample
IMU_STEP_DTYPE = np.dtype([("a", "<f4", 3), ("w", "<f4", 3), ("dt", "<f4"), ("reserved", "<f4")])  # orbfe_imu_step
IMU_FROM_KEYFRAME, IMU_FROM_FRAME = 0, 1


class ImuPreint(C.Structure):
    """orbfe_imu_preint: IMU::Preintegrated without its measurement list.  floats() / set_floats() move the 298 floats dT .. C."""
    _fields_ = [("struct_size", C.c_int), ("n_steps", C.c_int), ("dT", C.c_float), ("bg", C.c_float * 3), ("ba", C.c_float * 3),
                ("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3), ("JRg", C.c_float * 9), ("JVg", C.c_float * 9),
                ("JVa", C.c_float * 9), ("JPg", C.c_float * 9), ("JPa", C.c_float * 9), ("avgA", C.c_float * 3), ("avgW", C.c_float * 3),
                ("C", C.c_float * 225)]

    def __init__(self, floats=None, n_steps=0):
        super().__init__()
        self.struct_size = C.sizeof(ImuPreint)
        self.n_steps = int(n_steps)
        if floats is not None:
            self.set_floats(floats)

    def floats(self):
        return np.frombuffer(bytes(self), np.float32, 298, 8).copy()

    def set_floats(self, v):
        v = np.ascontiguousarray(v, np.float32).reshape(298)
        C.memmove(C.addressof(self) + 8, v.ctypes.data, v.nbytes)


class ImuPredictParams(C.Structure):
    """orbfe_imu_predict_params: which record the prediction and the link come from, gravity, the camera-body extrinsics."""
    _fields_ = [("struct_size", C.c_int), ("which", C.c_int), ("gravity", C.c_float), ("Rcb", C.c_float * 9), ("tcb", C.c_float * 3),
                ("tbc", C.c_float * 3)]

    def __init__(self, which=0, gravity=9.81, Rcb=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), tcb=(0.0,) * 3, tbc=(0.0,) * 3):
        super().__init__(C.sizeof(ImuPredictParams), int(which), float(gravity),
                         (C.c_float * 9)(*[float(x) for x in np.asarray(Rcb).reshape(-1)]), (C.c_float * 3)(*[float(x) for x in tcb]),
                         (C.c_float * 3)(*[float(x) for x in tbc]))


class InitialBAParams(C.Structure):
    """orbfe_initial_ba_params: the camera and the constants of Optimizer::GlobalBundleAdjustemnt(map, 20) (src/Optimizer.cc:60-369)."""
    _fields_ = [("struct_size", C.c_int), ("camera_model", C.c_int), ("cam", C.c_float * 8), ("huber_delta2", C.c_double),
                ("robust", C.c_int), ("iterations", C.c_int), ("stereo", C.c_int)]

    def __init__(self, cam=(0.0,) * 8, camera_model=0, huber_delta2=5.99, robust=1, iterations=20, stereo=0):
        super().__init__(C.sizeof(InitialBAParams), int(camera_model), (C.c_float * 8)(*[float(x) for x in cam]), huber_delta2, int(robust),
                         iterations, stereo)


class InitialBAInfo(C.Structure):
    """orbfe_initial_ba_info: every intermediate of one orbfe_initial_bundle_adjustment call."""
    _fields_ = [("struct_size", C.c_int), ("N", C.c_int), ("n_iterations", C.c_int), ("n_trials", C.c_int), ("exit_kind", C.c_int),
                ("trials", C.c_int * 64), ("cost", C.c_double * 64), ("lambda_", C.c_double * 64), ("pose", C.c_double * 12),
                ("chi2", C.c_void_p), ("depth_positive", C.c_void_p)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(InitialBAInfo)


class TrackParams(C.Structure):
    """orbfe_track_params: frame grid statics (src/Frame.cc:101-105) + the call parameters of SearchByProjection."""
    _fields_ = [("struct_size", C.c_int), ("grid_cols", C.c_int), ("grid_rows", C.c_int), ("min_x", C.c_float),
                ("min_y", C.c_float), ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float), ("th", C.c_float),
                ("nn_ratio", C.c_float), ("far_points", C.c_int), ("th_far_points", C.c_float)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TrackParams)


class TrackInertialParams(C.Structure):
    """orbfe_track_inertial_params: the one block of the inertial TrackLocalMap chain (SPEC DECISION S23) -- the grid and matcher
    parameters, the IMU noise, the prediction block (its `which` chooses the link kind and the optimisation), the frustum TEMPLATE
    (its pose fields are ignored) and the S19 / S20 blocks."""
    _fields_ = [("struct_size", C.c_int), ("inlier_threshold", C.c_int), ("track", TrackParams), ("noise", ImuNoise),
                ("predict", ImuPredictParams), ("frustum", Frustum), ("pose_keyframe", PoseInertialParams),
                ("pose_frame", PoseInertialPrevParams)]

    def __init__(self, track=None, noise=None, predict=None, frustum=None, pose_keyframe=None, pose_frame=None, inlier_threshold=8):
        super().__init__()
        self.struct_size = C.sizeof(TrackInertialParams)
        self.inlier_threshold = int(inlier_threshold)
        for name, v, t in (("track", track, TrackParams), ("noise", noise, ImuNoise), ("predict", predict, ImuPredictParams),
                           ("frustum", frustum, Frustum), ("pose_keyframe", pose_keyframe, PoseInertialParams),
                           ("pose_frame", pose_frame, PoseInertialPrevParams)):
            src = v if v is not None else t()
            C.memmove(C.addressof(self) + getattr(TrackInertialParams, name).offset, C.addressof(src), C.sizeof(t))


TRACK_INERTIAL_IO_FIELDS = ("d_samples", "sample_off", "d_t_prev", "d_t_cur", "d_frame_bias", "d_state1", "d_kf", "d_frame", "d_steps_out",
                            "d_kp", "d_desc", "d_n", "d_ids", "d_priors", "d_state_in", "d_info_ok", "d_mp_out", "d_match_out",
                            "d_n_matches", "d_state_out", "d_H_out", "d_Hprior_out", "d_outlier", "d_n_inliers", "d_accepted", "d_found",
                            "d_matches_inliers", "d_tracked", "d_Tcw_out")


class TrackInertialIO(C.Structure):
    """orbfe_track_inertial_io: the pointers of orbfe_track_inertial_batch_device (device pointers as ints; sample_off is HOST)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int)] + [(k, C.c_void_p) for k in TRACK_INERTIAL_IO_FIELDS]

    def __init__(self, **k):
        super().__init__(**k)
        self.struct_size = C.sizeof(TrackInertialIO)


class TrackInertialResult(C.Structure):
    """orbfe_track_inertial_result: what orbfe_track_frame_inertial hands back besides the frame's features."""
    _fields_ = [("struct_size", C.c_int), ("n_steps", C.c_int), ("steps_out", C.c_void_p), ("state_in", C.c_void_p), ("link_out", C.c_void_p),
                ("info_ok", C.c_int), ("n_matches", C.c_int), ("mp_out", C.c_void_p), ("match_out", C.c_void_p), ("state_out", C.c_void_p),
                ("H_out", C.c_void_p), ("Hprior_out", C.c_void_p), ("outlier", C.c_void_p), ("found", C.c_void_p), ("n_inliers", C.c_int),
                ("accepted", C.c_int), ("matches_inliers", C.c_int), ("tracked", C.c_int), ("Tcw", C.c_float * 12)]

    def __init__(self, **k):
        super().__init__(**k)
        self.struct_size = C.sizeof(TrackInertialResult)


# SPEC DECISION S24 (include/orbfe.h): the figures the tests need are mirrored here, and checked against the header by tests/test_local_map_abi.py
COVIS_MAX_COVISIBLE = 16
LOCAL_KF_MAX = 288
NO_POINT = 0x7fffffff
LOCAL_MAP_BLOCK = 1024       # threads of the points kernel's block: the chunk of the points walk
LOCAL_MAP_VOTE_TABLE = 512   # distinct voted key frames the LDS table holds before the call counts in HBM


class CovisKeyframe(C.Structure):
    """orbfe_covis_keyframe: one key frame as orbfe_covis_set_keyframes takes it (HOST pointers)."""
    _fields_ = [("struct_size", C.c_int), ("slot", C.c_int), ("mn_id", C.c_int), ("bad", C.c_int), ("parent", C.c_int), ("prev", C.c_int),
                ("n_features", C.c_int), ("n_covisible", C.c_int), ("n_children", C.c_int), ("reserved", C.c_int),
                ("point_ids", C.c_void_p), ("covisible", C.c_void_p), ("children", C.c_void_p)]

    def __init__(self, **k):
        super().__init__(**k)
        self.struct_size = C.sizeof(CovisKeyframe)


class LocalMapParams(C.Structure):
    """orbfe_local_map_params: mMaxLocalKFCount, mCovisibilityKeyFrameNd, mTemporalKeyFrameNd, the sensor kind and whether the voters are
    the current frame's own points (SPEC DECISION S24)."""
    _fields_ = [("struct_size", C.c_int), ("max_local_kf", C.c_int), ("n_covisible", C.c_int), ("n_temporal", C.c_int),
                ("inertial", C.c_int), ("mark_voters_seen", C.c_int)]

    def __init__(self, max_local_kf=10, n_covisible=5, n_temporal=10, inertial=1, mark_voters_seen=0):
        super().__init__(C.sizeof(LocalMapParams), int(max_local_kf), int(n_covisible), int(n_temporal), int(inertial), int(mark_voters_seen))


LOCAL_MAP_IO_FIELDS = ("d_vote_ids", "d_n_votes", "d_last_kf", "d_ids_out", "d_n_local_points", "d_local_kfs", "d_n_local_kfs",
                       "d_vote_ids_out")


class LocalMapIO(C.Structure):
    """orbfe_local_map_io: the device pointers of orbfe_update_local_map_batch_device (as ints)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int)] + [(k, C.c_void_p) for k in LOCAL_MAP_IO_FIELDS]

    def __init__(self, **k):
        super().__init__(**k)
        self.struct_size = C.sizeof(LocalMapIO)


# SPEC DECISION S25 (include/orbfe.h), checked against the header by tests/test_covis_update_abi.py
COVIS_MAX_CONN_STRIDE = 4096
COVIS_STATUS_OK, COVIS_STATUS_NO_COUNTS, COVIS_STATUS_REFUSED = 0, 1, 2


class CovisUpdateParams(C.Structure):
    """orbfe_covis_update_params: `th` of KeyFrame::UpdateConnections (KeyFrame.cc:500), 50 in this fork."""
    _fields_ = [("struct_size", C.c_int), ("min_weight", C.c_int)]

    def __init__(self, min_weight=50):
        super().__init__(C.sizeof(CovisUpdateParams), int(min_weight))


COVIS_UPDATE_IO_FIELDS = ("d_slots", "d_weights", "d_count", "d_status")


class CovisUpdateIO(C.Structure):
    """orbfe_covis_update_io: the device pointers of orbfe_covis_update_connections_device (as ints)."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int)] + [(k, C.c_void_p) for k in COVIS_UPDATE_IO_FIELDS]

    def __init__(self, **k):
        super().__init__(**k)
        self.struct_size = C.sizeof(CovisUpdateIO)


# SPEC DECISION S26 (include/orbfe.h), checked against the header by tests/test_point_refresh_abi.py
REFRESH_MAX_LEVELS = 32
REFRESH_DEPTH, REFRESH_DESCRIPTOR = 1, 2
REFRESH_IO_FIELDS = ("d_status", "d_min_distance", "d_max_distance", "d_best_slot", "d_best_index", "d_best_median")


class RefreshIO(C.Structure):
    """orbfe_refresh_io: the device pointers of orbfe_covis_refresh_points_device (as ints), any may be None."""
    _fields_ = [("struct_size", C.c_int), ("reserved", C.c_int)] + [(k, C.c_void_p) for k in REFRESH_IO_FIELDS]

    def __init__(self, **k):
        super().__init__(**k)
        self.struct_size = C.sizeof(RefreshIO)


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int), ("kp", C.c_void_p), ("desc", C.c_void_p), ("grid_cols", C.c_int),
                ("grid_rows", C.c_int), ("min_x", C.c_float), ("min_y", C.c_float),
                ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float), ("n_levels", C.c_int),
                ("scale_factors", C.c_void_p)]


# every symbol include/orbfe.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "orbfe_create", "orbfe_destroy", "orbfe_get_levels", "orbfe_get_scale_factor", "orbfe_get_scale_tables",
    "orbfe_get_level_info", "orbfe_max_keypoints", "orbfe_extract", "orbfe_extract_batch",
    "orbfe_extract_batch_device", "orbfe_get_pyramid_level", "orbfe_debug_get_candidates",
    "orbfe_set_stage_timing", "orbfe_get_stage_ms", "orbfe_stage_name", "orbfe_hamming",
    "orbfe_match_projection", "orbfe_match_projection_batch_device", "orbfe_match_bow", "orbfe_match_bow_rig", "orbfe_match_initialization", "orbfe_vocab_create", "orbfe_vocab_destroy", "orbfe_bow_transform",
    "orbfe_prep_create", "orbfe_prep_destroy", "orbfe_prepare_image", "orbfe_prepare_image_device", "orbfe_prepare_and_extract",
    "orbfe_project_map_points", "orbfe_project_map_points_device", "orbfe_fuse_search", "orbfe_fuse_search_right", "orbfe_fuse_search_sim3", "orbfe_search_by_sim3", "orbfe_match_projection_keyframe", "orbfe_match_triangulation", "orbfe_distinctive_descriptors", "orbfe_status_string", "orbfe_last_error", "orbfe_version",
    "orbfe_get_device_status", "orbfe_stream_create", "orbfe_stream_destroy", "orbfe_stream_submit", "orbfe_stream_collect",
    "orbfe_stream_collect_view", "orbfe_stream_in_flight", "orbfe_track_frame",
    "orbfe_keyframe_create", "orbfe_keyframe_destroy", "orbfe_keyframe_size", "orbfe_match_triangulation_batch",
    "orbfe_triangulation_select", "orbfe_create_new_points_batch", "orbfe_triangulate_pairs", "orbfe_map_create", "orbfe_map_destroy", "orbfe_map_update", "orbfe_stream_enable_track",
    "orbfe_stream_submit_track", "orbfe_stream_collect_track", "orbfe_track_frame_map", "orbfe_track_reference_keyframe", "orbfe_debug_graph_stats", "orbfe_set_graph_capture",
    "orbfe_debug_clock_probe", "orbfe_keyframe_set_grid", "orbfe_fuse_search_keyframe", "orbfe_fuse_search_keyframes", "orbfe_fuse_select",
    "orbfe_init_frame_create", "orbfe_init_frame_destroy", "orbfe_init_frame_size", "orbfe_track_initialization",
    "orbfe_set_stream_priority", "orbfe_two_view_reconstruct", "orbfe_mlpnp_plan", "orbfe_mlpnp_ransac",
    "orbfe_pose_optimization", "orbfe_pose_optimization_batch_device", "orbfe_initial_bundle_adjustment",
    "orbfe_pose_inertial_optimization_last_keyframe", "orbfe_pose_inertial_optimization_batch_device",
    "orbfe_pose_inertial_optimization_last_frame", "orbfe_pose_inertial_optimization_last_frame_batch_device",
    "orbfe_marginalize_pose_imu",
    "orbfe_imu_preintegrate_frame", "orbfe_imu_reintegrate", "orbfe_imu_predict", "orbfe_imu_frame_batch_device",
    "orbfe_imu_reintegrate_batch_device",
    "orbfe_track_inertial_batch_device", "orbfe_track_frame_inertial",
    "orbfe_covis_create", "orbfe_covis_destroy", "orbfe_covis_set_keyframes", "orbfe_covis_set_observations",
    "orbfe_update_local_map_batch_device", "orbfe_update_local_map", "orbfe_frame_points_batch_device",
    "orbfe_covis_enable_connections", "orbfe_covis_set_connections", "orbfe_covis_get_keyframe",
    "orbfe_covis_update_connections_device", "orbfe_covis_update_connections", "orbfe_covis_add_keyframe_device", "orbfe_covis_add_keyframe",
    "orbfe_covis_enable_refresh", "orbfe_covis_set_features", "orbfe_covis_set_features_device", "orbfe_covis_set_centres",
    "orbfe_covis_set_observations_indexed", "orbfe_covis_set_ref_keyframes", "orbfe_covis_get_point",
    "orbfe_covis_refresh_points_device", "orbfe_covis_refresh_points",
    "orbfe_shard_range", "orbfe_pool_create", "orbfe_pool_destroy", "orbfe_pool_size", "orbfe_pool_member",
    "orbfe_pool_member_frames", "orbfe_pool_last_error", "orbfe_pool_extract", "orbfe_pool_enable_track",
    "orbfe_pool_map_update", "orbfe_pool_track",
]

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (soname
    libamdhip64.so.7, looked up by file name through $ORIGIN); if liborbfe.so pulled in the system
    copy first, a later `import torch` would load a second HIP/HSA runtime that sees no GPU and
    whose streams are foreign to ours.  Loading torch's copy first makes liborbfe.so bind to it."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except OSError:
        pass


def lib():
    """Load liborbfe.so; fail loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("liborbfe.so not found at %s -- run __graft_entry__.build() (hipcc, gfx950); "
                           "there is no CPU fallback" % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    vp, ci, cf, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.orbfe_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.orbfe_destroy.argtypes = [vp]
    L.orbfe_destroy.restype = None
    L.orbfe_get_levels.argtypes = [vp]
    L.orbfe_get_scale_factor.argtypes = [vp]
    L.orbfe_get_scale_factor.restype = cf
    L.orbfe_get_scale_tables.argtypes = [vp, vp, vp, vp, vp]
    L.orbfe_get_level_info.argtypes = [vp, vp, vp, vp]
    L.orbfe_max_keypoints.argtypes = [vp]
    L.orbfe_extract.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    L.orbfe_extract_batch.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_get_device_status.argtypes = [vp, vp]
    L.orbfe_debug_graph_stats.argtypes = [vp, vp, vp]
    L.orbfe_set_graph_capture.argtypes = [vp, ci]
    L.orbfe_set_stream_priority.argtypes = [vp, ci]
    L.orbfe_debug_clock_probe.argtypes = [vp, ci, vp, vp]
    L.orbfe_stream_create.argtypes = [vp, ci, ci, C.POINTER(vp)]
    L.orbfe_stream_destroy.argtypes = [vp]
    L.orbfe_stream_destroy.restype = None
    L.orbfe_stream_submit.argtypes = [vp, vp, ci, ci]
    L.orbfe_stream_collect.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbfe_stream_collect_view.argtypes = [vp, vp, vp, vp, vp, vp]
    L.orbfe_stream_in_flight.argtypes = [vp]
    L.orbfe_map_create.argtypes = [vp, ci, C.POINTER(vp)]
    L.orbfe_map_destroy.argtypes = [vp]
    L.orbfe_map_destroy.restype = None
    L.orbfe_map_update.argtypes = [vp, vp, ci, vp, vp, vp]
    L.orbfe_stream_enable_track.argtypes = [vp, vp, ci]
    L.orbfe_stream_submit_track.argtypes = [vp, vp, ci, ci, C.POINTER(TrackParams), vp, ci, vp]
    L.orbfe_stream_collect_track.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_extract_batch_device.argtypes = [vp, vp, sz, ci, ci, vp, vp, vp, vp, vp]
    L.orbfe_get_pyramid_level.argtypes = [vp, ci, ci, ci, vp, ci]
    L.orbfe_debug_get_candidates.argtypes = [vp, ci, ci, vp, ci, vp, vp]
    L.orbfe_set_stage_timing.argtypes = [vp, ci]
    L.orbfe_get_stage_ms.argtypes = [vp, vp, vp]
    L.orbfe_stage_name.argtypes = [ci]
    L.orbfe_stage_name.restype = C.c_char_p
    L.orbfe_hamming.argtypes = [vp, vp]
    L.orbfe_match_projection.argtypes = [vp, C.POINTER(FrameView), ci, vp, vp, vp, cf, ci, cf, cf, vp, vp]
    L.orbfe_match_projection_batch_device.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, cf, cf, cf, cf, ci, vp, vp, vp,
                                                      cf, ci, cf, cf, vp, vp, vp]
    L.orbfe_match_bow.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, cf, ci, vp, vp]
    L.orbfe_match_bow_rig.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, ci, vp, vp, ci, cf, ci, vp, vp]
    L.orbfe_match_initialization.argtypes = [vp, C.POINTER(FrameView), C.POINTER(FrameView), ci, cf, ci, vp, vp]
    L.orbfe_track_frame.argtypes = [vp, vp, ci, C.POINTER(Frustum), C.POINTER(TrackParams), ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_track_frame_map.argtypes = [vp, vp, ci, C.POINTER(Frustum), C.POINTER(TrackParams), vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_track_reference_keyframe.argtypes = [vp, vp, ci, vp, ci, vp, vp, C.c_float, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbfe_init_frame_create.argtypes = [vp, ci, vp, vp, C.POINTER(vp)]
    L.orbfe_init_frame_destroy.argtypes = [vp]
    L.orbfe_init_frame_destroy.restype = None
    L.orbfe_init_frame_size.argtypes = [vp]
    L.orbfe_track_initialization.argtypes = [vp, vp, ci, vp, C.POINTER(TrackParams), ci, cf, ci, vp, vp, vp, vp, vp, vp]
    L.orbfe_project_map_points.argtypes = [vp, C.POINTER(Frustum), ci, vp, vp, vp]
    L.orbfe_project_map_points_device.argtypes = [vp, C.POINTER(Frustum), ci, vp, vp, vp, vp]
    L.orbfe_fuse_search.argtypes = [vp, C.POINTER(FrameView), vp, vp, C.POINTER(Frustum), cf, ci, vp, vp, vp, vp]
    L.orbfe_fuse_search_right.argtypes = [vp, C.POINTER(FrameView), ci, vp, vp, C.POINTER(Frustum), cf, ci, vp, vp, vp, vp]
    L.orbfe_prep_create.argtypes = [vp, ci, ci, vp, vp, ci, ci, C.POINTER(vp)]
    L.orbfe_prep_destroy.argtypes = [vp]
    L.orbfe_prep_destroy.restype = None
    L.orbfe_prepare_image.argtypes = [vp, vp, vp, ci, vp, ci]
    L.orbfe_prepare_image_device.argtypes = [vp, vp, vp, ci, vp, ci, vp]
    L.orbfe_prepare_and_extract.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, ci]
    L.orbfe_fuse_search_sim3.argtypes = [vp, C.POINTER(FrameView), C.POINTER(Frustum), cf, ci, vp, vp, vp, vp]
    L.orbfe_search_by_sim3.argtypes = [vp, C.POINTER(FrameView), C.POINTER(FrameView), C.POINTER(Sim3View),
                                       C.POINTER(Sim3View), vp, vp, vp, vp, cf, vp, C.POINTER(ci)]
    L.orbfe_match_projection_keyframe.argtypes = [vp, C.POINTER(FrameView), C.POINTER(Frustum), ci, vp, vp, vp, vp, cf,
                                                  ci, vp, C.POINTER(ci)]
    L.orbfe_match_triangulation.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci,
                                            C.POINTER(TriParams), vp, vp]
    L.orbfe_keyframe_create.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, C.POINTER(vp)]
    L.orbfe_keyframe_destroy.argtypes = [vp]
    L.orbfe_keyframe_destroy.restype = None
    L.orbfe_keyframe_size.argtypes = [vp]
    L.orbfe_keyframe_set_grid.argtypes = [vp, vp, ci, ci, cf, cf, cf, cf, vp, vp]
    L.orbfe_fuse_search_keyframe.argtypes = [vp, vp, vp, ci, vp, C.POINTER(Frustum), cf, vp, vp]
    L.orbfe_fuse_search_keyframes.argtypes = [vp, ci, vp, vp, vp, ci, vp, vp, cf, vp, vp, ci, vp, vp]
    L.orbfe_fuse_select.argtypes = [vp, ci, ci, vp, ci, vp, C.POINTER(ci), C.POINTER(ci)]
    L.orbfe_match_triangulation_batch.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.orbfe_triangulation_select.argtypes = [ci, vp, vp, vp, ci, vp, vp]
    if hasattr(L, "orbfe_create_new_points_batch"):  # an earlier build loaded for an A/B (bench.py --lib tools/ab/...) lacks the two
        L.orbfe_create_new_points_batch.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp]
        L.orbfe_triangulate_pairs.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp]
    if hasattr(L, "orbfe_two_view_reconstruct"):  # (as above: absent from an earlier build loaded for an A/B)
        L.orbfe_two_view_reconstruct.argtypes = [vp, C.POINTER(TwoViewParams), ci, vp, ci, vp, vp, vp, C.POINTER(ci), vp, vp, vp, vp,
                                                 C.POINTER(TwoViewInfo)]
    if hasattr(L, "orbfe_mlpnp_ransac"):  # (as above)
        L.orbfe_mlpnp_plan.argtypes = [C.POINTER(MlpnpParams), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.orbfe_mlpnp_ransac.argtypes = [vp, C.POINTER(MlpnpParams), ci, vp, vp, ci, vp, vp, ci, C.POINTER(ci), vp, vp, C.POINTER(ci),
                                         C.POINTER(ci), C.POINTER(MlpnpInfo)]
    if hasattr(L, "orbfe_pose_optimization"):  # (as above)
        L.orbfe_pose_optimization.argtypes = [vp, C.POINTER(PoseOptParams), ci, vp, vp, ci, vp, vp, vp, vp, vp, C.POINTER(ci),
                                              C.POINTER(PoseOptInfo)]
        L.orbfe_pose_optimization_batch_device.argtypes = [vp, C.POINTER(PoseOptParams), ci, vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    if hasattr(L, "orbfe_pose_inertial_optimization_last_keyframe"):  # (as above)
        L.orbfe_pose_inertial_optimization_last_keyframe.argtypes = [vp, C.POINTER(PoseInertialParams), C.POINTER(ImuLink), ci, vp, vp, ci] + \
            [vp] * 16 + [C.POINTER(ci), C.POINTER(PoseInertialInfo)]
        L.orbfe_pose_inertial_optimization_batch_device.argtypes = [vp, C.POINTER(PoseInertialParams), ci, vp, vp, vp, ci, vp, ci, vp, ci, vp,
                                                                    vp, vp, vp, vp, vp, vp]
    if hasattr(L, "orbfe_pose_inertial_optimization_last_frame"):  # (as above)
        L.orbfe_pose_inertial_optimization_last_frame.argtypes = [vp, C.POINTER(PoseInertialPrevParams), C.POINTER(ImuLinkFree),
                                                                  C.POINTER(PoseImuPrior), ci, vp, vp, ci] + [vp] * 17 + \
            [C.POINTER(ci), C.POINTER(ci), C.POINTER(PoseInertialPrevInfo)]
        L.orbfe_pose_inertial_optimization_last_frame_batch_device.argtypes = [vp, C.POINTER(PoseInertialPrevParams), ci, vp, vp, vp, vp, ci,
                                                                               vp, ci, vp, ci] + [vp] * 9
        L.orbfe_marginalize_pose_imu.argtypes = [vp, vp]
    if hasattr(L, "orbfe_imu_preintegrate_frame"):  # (as above)
        L.orbfe_imu_preintegrate_frame.argtypes = [vp, C.POINTER(ImuNoise), ci, vp, C.c_double, C.c_double, vp, C.POINTER(ImuPreint),
                                                   C.POINTER(ImuPreint), vp, C.POINTER(ci)]
        L.orbfe_imu_reintegrate.argtypes = [vp, C.POINTER(ImuNoise), vp, ci, vp, C.POINTER(ImuPreint)]
        L.orbfe_imu_predict.argtypes = [vp, C.POINTER(ImuPredictParams), vp, C.POINTER(ImuPreint), C.POINTER(ImuPreint), vp, vp, C.POINTER(ci)]
        L.orbfe_imu_frame_batch_device.argtypes = [vp, C.POINTER(ImuNoise), C.POINTER(ImuPredictParams), ci] + [vp] * 13
        L.orbfe_imu_reintegrate_batch_device.argtypes = [vp, C.POINTER(ImuNoise), ci, vp, vp, vp, vp, vp]
    if hasattr(L, "orbfe_track_inertial_batch_device"):  # (as above)
        L.orbfe_track_inertial_batch_device.argtypes = [vp, C.POINTER(TrackInertialParams), ci, ci, vp, ci, C.POINTER(TrackInertialIO), vp]
        L.orbfe_track_frame_inertial.argtypes = [vp, C.POINTER(TrackInertialParams), vp, ci, ci, vp, C.c_double, C.c_double, vp, vp,
                                                 C.POINTER(ImuPreint), C.POINTER(ImuPreint), vp, ci, vp, C.POINTER(PoseImuPrior), vp, vp,
                                                 C.POINTER(ci), vp, C.POINTER(TrackInertialResult)]
    if hasattr(L, "orbfe_update_local_map_batch_device"):  # (as above)
        L.orbfe_covis_create.argtypes = [vp, vp, ci, ci, ci, ci, C.POINTER(vp)]
        L.orbfe_covis_destroy.argtypes = [vp]
        L.orbfe_covis_destroy.restype = None
        L.orbfe_covis_set_keyframes.argtypes = [vp, vp, ci, vp]
        L.orbfe_covis_set_observations.argtypes = [vp, vp, ci, vp, vp, vp]
        L.orbfe_update_local_map_batch_device.argtypes = [vp, C.POINTER(LocalMapParams), ci, ci, vp, ci, C.POINTER(LocalMapIO), vp]
        L.orbfe_update_local_map.argtypes = [vp, C.POINTER(LocalMapParams), ci, vp, ci, vp, ci, vp, C.POINTER(ci), vp, C.POINTER(ci), vp]
        L.orbfe_frame_points_batch_device.argtypes = [vp, vp, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "orbfe_covis_update_connections_device"):  # (as above)
        L.orbfe_covis_enable_connections.argtypes = [vp, vp, ci]
        L.orbfe_covis_set_connections.argtypes = [vp, vp, ci, vp, vp, vp, vp]
        L.orbfe_covis_get_keyframe.argtypes = [vp, vp, ci, C.POINTER(CovisKeyframe), vp, vp, vp, vp, C.POINTER(ci)]
        L.orbfe_covis_update_connections_device.argtypes = [vp, C.POINTER(CovisUpdateParams), vp, ci, vp, vp, C.POINTER(CovisUpdateIO), vp]
        L.orbfe_covis_update_connections.argtypes = [vp, C.POINTER(CovisUpdateParams), vp, ci, ci, vp, vp, C.POINTER(ci), C.POINTER(ci)]
        L.orbfe_covis_add_keyframe_device.argtypes = [vp, vp, C.POINTER(CovisKeyframe), vp, ci, vp, vp, vp]
        L.orbfe_covis_add_keyframe.argtypes = [vp, vp, C.POINTER(CovisKeyframe), vp, C.POINTER(ci)]
    if hasattr(L, "orbfe_covis_refresh_points_device"):  # (as above)
        L.orbfe_covis_enable_refresh.argtypes = [vp, vp, ci, vp]
        L.orbfe_covis_set_features.argtypes = [vp, vp, ci, ci, vp, vp]
        L.orbfe_covis_set_features_device.argtypes = [vp, vp, ci, vp, vp, ci, vp]
        L.orbfe_covis_set_centres.argtypes = [vp, vp, ci, vp, vp]
        L.orbfe_covis_set_observations_indexed.argtypes = [vp, vp, ci, vp, vp, vp, vp]
        L.orbfe_covis_set_ref_keyframes.argtypes = [vp, vp, ci, vp, vp]
        L.orbfe_covis_get_point.argtypes = [vp, vp, ci, C.POINTER(ci), vp, vp, C.POINTER(ci), vp, vp]
        L.orbfe_covis_refresh_points_device.argtypes = [vp, vp, ci, vp, vp, ci, ci, C.POINTER(RefreshIO), vp]
        L.orbfe_covis_refresh_points.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "orbfe_initial_bundle_adjustment"):  # (as above)
        L.orbfe_initial_bundle_adjustment.argtypes = [vp, C.POINTER(InitialBAParams), ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                      C.POINTER(InitialBAInfo)]
    L.orbfe_distinctive_descriptors.argtypes = [vp, ci, vp, vp, vp, vp]
    L.orbfe_vocab_create.argtypes = [vp, ci, vp, vp, vp, vp, vp, ci, C.POINTER(vp)]
    L.orbfe_vocab_destroy.argtypes = [vp]
    L.orbfe_vocab_destroy.restype = None
    L.orbfe_bow_transform.argtypes = [vp, vp, vp, ci, ci, vp, vp, vp]
    L.orbfe_status_string.argtypes = [ci]
    L.orbfe_status_string.restype = C.c_char_p
    L.orbfe_last_error.argtypes = [vp]
    L.orbfe_last_error.restype = C.c_char_p
    L.orbfe_version.restype = C.c_char_p
    L.orbfe_shard_range.argtypes = [ci, ci, ci, vp, vp]
    L.orbfe_pool_create.argtypes = [C.POINTER(Params), vp, ci, ci, ci, C.POINTER(vp)]
    L.orbfe_pool_destroy.argtypes = [vp]
    L.orbfe_pool_destroy.restype = None
    L.orbfe_pool_size.argtypes = [vp]
    L.orbfe_pool_member.argtypes = [vp, ci]
    L.orbfe_pool_member.restype = vp
    L.orbfe_pool_member_frames.argtypes = [vp, ci]
    L.orbfe_pool_member_frames.restype = C.c_longlong
    L.orbfe_pool_last_error.argtypes = [vp]
    L.orbfe_pool_last_error.restype = C.c_char_p
    L.orbfe_pool_extract.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp]
    L.orbfe_pool_enable_track.argtypes = [vp, ci, ci]
    L.orbfe_pool_map_update.argtypes = [vp, ci, vp, vp, vp]
    L.orbfe_pool_track.argtypes = [vp, vp, ci, ci, C.POINTER(TrackParams), vp, ci, vp, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class ORBextractor:
    """ORB_SLAM3::ORBextractor (include/ORBextractor.h:52-130) on one MI355X."""

    def __init__(self, nFeatures, nFastFeatures, scaleFactor, nlevels, iniThFAST, minThFAST, imageWidth,
                 imageHeight, device=0, max_batch=1):
        self.L = lib()
        self.h = C.c_void_p()
        prm = Params(nFeatures, nFastFeatures, scaleFactor, nlevels, iniThFAST, minThFAST, imageWidth,
                     imageHeight, device, max_batch)
        rc = self.L.orbfe_create(C.byref(prm), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise OrbfeError(rc, "orbfe_create")
        self.nlevels, self.W, self.H, self.max_batch = nlevels, imageWidth, imageHeight, max_batch
        self.cap = self.L.orbfe_max_keypoints(self.h)
        n = nlevels
        self.mvScaleFactor = np.zeros(n, np.float32)
        self.mvInvScaleFactor = np.zeros(n, np.float32)
        self.mvLevelSigma2 = np.zeros(n, np.float32)
        self.mvInvLevelSigma2 = np.zeros(n, np.float32)
        self._chk(self.L.orbfe_get_scale_tables(self.h, _p(self.mvScaleFactor), _p(self.mvInvScaleFactor),
                                                _p(self.mvLevelSigma2), _p(self.mvInvLevelSigma2)), "scale_tables")
        self.mnFeaturesPerLevel = np.zeros(n, np.int32)
        self.levelW = np.zeros(n, np.int32)
        self.levelH = np.zeros(n, np.int32)
        self._chk(self.L.orbfe_get_level_info(self.h, _p(self.mnFeaturesPerLevel), _p(self.levelW), _p(self.levelH)),
                  "level_info")

    def _chk(self, rc, where):
        if rc != 0:
            raise OrbfeError(rc, where, self.L.orbfe_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_destroy(self.h)
            self.h = None

    __del__ = close

    # getters, include/ORBextractor.h:64-92
    def GetLevels(self):
        return self.L.orbfe_get_levels(self.h)

    def GetScaleFactor(self):
        return self.L.orbfe_get_scale_factor(self.h)

    def GetScaleFactors(self):
        return self.mvScaleFactor.copy()

    def GetInverseScaleFactors(self):
        return self.mvInvScaleFactor.copy()

    def GetScaleSigmaSquares(self):
        return self.mvLevelSigma2.copy()

    def GetInverseScaleSigmaSquares(self):
        return self.mvInvLevelSigma2.copy()

    def extractFeatures(self, im):
        """extractFeatures (include/ORBextractor.h:62): returns (keypoints, descriptors) or None."""
        im = np.asarray(im)
        assert im.dtype == np.uint8 and im.shape == (self.H, self.W) and im.strides[1] == 1
        kp = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = C.c_int()
        self.last_per_level = np.zeros(self.nlevels, np.int32)
        self._chk(self.L.orbfe_extract(self.h, _p(im), im.strides[0], _p(kp), _p(desc), C.byref(n),
                                       _p(self.last_per_level)), "orbfe_extract")
        if n.value == 0:
            return None
        return kp[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, ims):
        """Host-pointer batched mode: list/array of frames -> list of (kp, desc, per_level)."""
        ims = [np.ascontiguousarray(im, np.uint8) for im in ims]
        B = len(ims)
        assert 1 <= B <= self.max_batch
        ptrs = (C.c_void_p * B)(*[im.ctypes.data for im in ims])
        kp = np.zeros((B, self.cap), KP_DTYPE)
        desc = np.zeros((B, self.cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        per = np.zeros((B, self.nlevels), np.int32)
        self._chk(self.L.orbfe_extract_batch(self.h, ptrs, self.W, B, _p(kp), _p(desc), _p(n), _p(per)),
                  "orbfe_extract_batch")
        return [(kp[b, :n[b]].copy(), desc[b, :n[b]].copy(), per[b].copy()) for b in range(B)]

    def extract_batch_device(self, d_gray_ptr, frame_stride, pitch, batch, d_kp_ptr, d_desc_ptr, d_n_ptr,
                             d_per_ptr=None, stream=None):
        """Everything resident in HBM (raw device pointers as ints); asynchronous on `stream`."""
        self._chk(self.L.orbfe_extract_batch_device(self.h, d_gray_ptr, frame_stride, pitch, batch, d_kp_ptr,
                                                    d_desc_ptr, d_n_ptr, d_per_ptr, stream),
                  "orbfe_extract_batch_device")

    def device_status(self):
        """Guard flags of the last extract call on any stream (waits for it); raises when one is set."""
        flags = C.c_uint()
        self._chk(self.L.orbfe_get_device_status(self.h, C.byref(flags)), "orbfe_get_device_status")
        return flags.value

    def stream(self, slots=3, slot_frames=None):
        """Pipelined host-pointer extraction (orbfe_stream_*): see ExtractStream."""
        return ExtractStream(self, slots, slot_frames or self.max_batch)

    # mvImagePyramid / mvBlurredImagePyramid (include/ORBextractor.h:94-95)
    def pyramid_level(self, level, blurred=False, frame=0):
        w, h = int(self.levelW[level]), int(self.levelH[level])
        out = np.zeros((h, w), np.uint8)
        self._chk(self.L.orbfe_get_pyramid_level(self.h, frame, level, int(blurred), _p(out), w), "pyramid_level")
        return out

    def debug_candidates(self, level, frame=0):
        cap = ((int(self.levelW[level]) + 1) // 2) * ((int(self.levelH[level]) + 1) // 2)
        packed = np.zeros(cap, np.uint32)
        n = C.c_int()
        cnt = np.zeros(4, np.int32)
        self._chk(self.L.orbfe_debug_get_candidates(self.h, frame, level, _p(packed), cap, C.byref(n), _p(cnt)),
                  "debug_candidates")
        return packed[:n.value].copy(), cnt

    def set_graph_capture(self, on):
        self._chk(self.L.orbfe_set_graph_capture(self.h, int(bool(on))), "orbfe_set_graph_capture")

    def set_stream_priority(self, high):
        """orbfe_set_stream_priority: the handle's own stream at the device's highest (True) / lowest (False) priority"""
        self._chk(self.L.orbfe_set_stream_priority(self.h, int(bool(high))), "orbfe_set_stream_priority")

    def graph_stats(self):
        """(graphs captured, captures that failed and fell back to plain launches) of this handle"""
        a, b = C.c_int(), C.c_int()
        self._chk(self.L.orbfe_debug_graph_stats(self.h, C.byref(a), C.byref(b)), "orbfe_debug_graph_stats")
        return a.value, b.value

    def clock_probe(self, d_out_ptr, spin_us=20, stream=None):
        """orbfe_debug_clock_probe: asynchronous; d_out_ptr -> two device uint64 {shader cycles, 100 MHz ticks}"""
        self._chk(self.L.orbfe_debug_clock_probe(self.h, int(spin_us), d_out_ptr, stream), "orbfe_debug_clock_probe")

    def set_stage_timing(self, on):
        self._chk(self.L.orbfe_set_stage_timing(self.h, int(on)), "set_stage_timing")

    def stage_ms(self):
        ms = np.zeros(NUM_STAGES, np.float32)
        n = C.c_int()
        self._chk(self.L.orbfe_get_stage_ms(self.h, _p(ms), C.byref(n)), "get_stage_ms")
        names = [self.L.orbfe_stage_name(i).decode() for i in range(NUM_STAGES)]
        return dict(zip(names, ms.tolist())), n.value


def make_frame_view(kp, desc, gridCols, gridRows, minX, minY, maxX, maxY, scaleFactors):
    """Frame grid statics exactly as src/Frame.cc:101-105 derives them."""
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8)
    sf = np.ascontiguousarray(scaleFactors, np.float32)
    invw = np.float32(gridCols) / np.float32(np.float32(maxX) - np.float32(minX))
    invh = np.float32(gridRows) / np.float32(np.float32(maxY) - np.float32(minY))
    fv = FrameView(len(kp), kp.ctypes.data, desc.ctypes.data, gridCols, gridRows, minX, minY, float(invw),
                   float(invh), len(sf), sf.ctypes.data)
    fv._keep = (kp, desc, sf)
    return fv


class MapPoints:
    """orbfe_map: map points resident in HBM (world position, distance range, isBad, Observations, descriptor), indexed
    by a caller-chosen id in [0, capacity); frames name their local map points by id."""

    def __init__(self, extractor, capacity):
        self.e, self.L = extractor, extractor.L
        self.capacity = int(capacity)
        self.h = C.c_void_p()
        extractor._chk(self.L.orbfe_map_create(extractor.h, self.capacity, C.byref(self.h)), "orbfe_map_create")

    def update(self, ids, points, desc):
        ids = np.ascontiguousarray(ids, np.int32)
        points = np.ascontiguousarray(points, WP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        assert len(ids) == len(points) == len(desc)
        self.e._chk(self.L.orbfe_map_update(self.e.h, self.h, len(ids), _p(ids), _p(points), _p(desc)), "orbfe_map_update")

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_map_destroy(self.h)
            self.h = None

    __del__ = close


class Covisibility:
    """orbfe_covis: the graph Tracking::UpdateLocalMap walks, resident in HBM over the ids of one MapPoints (SPEC DECISION S24)."""

    def __init__(self, extractor, map_points, kf_capacity, kf_stride, obs_stride, child_stride):
        self.e, self.L, self.map = extractor, extractor.L, map_points
        self.kf_capacity, self.kf_stride, self.obs_stride, self.child_stride = int(kf_capacity), int(kf_stride), int(obs_stride), int(child_stride)
        self.h = C.c_void_p()
        extractor._chk(self.L.orbfe_covis_create(extractor.h, map_points.h, self.kf_capacity, self.kf_stride, self.obs_stride,
                                                 self.child_stride, C.byref(self.h)), "orbfe_covis_create")

    def set_keyframes(self, recs):
        """recs: dicts with slot, mn_id, bad, parent, prev, covisible, children and point_ids (None keeps the stored feature list)"""
        arr = (CovisKeyframe * max(len(recs), 1))()
        keep = []
        for r, k in zip(arr, recs):
            lists = {}
            for name in ("point_ids", "covisible", "children"):
                v = k.get(name)
                lists[name] = None if v is None else np.ascontiguousarray(v, np.int32)
            keep.append(lists)
            pts, cov, ch = lists["point_ids"], lists["covisible"], lists["children"]
            r.__init__(slot=int(k["slot"]), mn_id=int(k["mn_id"]), bad=int(k.get("bad", 0)), parent=int(k.get("parent", -1)),
                       prev=int(k.get("prev", -1)), n_features=0 if pts is None else len(pts), n_covisible=0 if cov is None else len(cov),
                       n_children=0 if ch is None else len(ch), point_ids=None if pts is None else pts.ctypes.data,
                       covisible=None if cov is None or not len(cov) else cov.ctypes.data,
                       children=None if ch is None or not len(ch) else ch.ctypes.data)
        self.e._chk(self.L.orbfe_covis_set_keyframes(self.e.h, self.h, len(recs), C.cast(arr, C.c_void_p)), "orbfe_covis_set_keyframes")

    def set_observations(self, ids, off, kf_slots):
        ids, off, kf_slots = (np.ascontiguousarray(a, np.int32) for a in (ids, off, kf_slots))
        assert len(off) == len(ids) + 1
        self.e._chk(self.L.orbfe_covis_set_observations(self.e.h, self.h, len(ids), _p(ids), _p(off), _p(kf_slots) if len(kf_slots) else None),
                    "orbfe_covis_set_observations")

    # ---- SPEC DECISION S25: the graph maintained on the device ----
    conn_stride = 0

    def enable_connections(self, conn_stride):
        """orbfe_covis_enable_connections: the full mConnectedKeyFrameWeights per key frame, up to conn_stride pairs"""
        self.e._chk(self.L.orbfe_covis_enable_connections(self.e.h, self.h, int(conn_stride)), "orbfe_covis_enable_connections")
        self.conn_stride = int(conn_stride)

    def set_connections(self, slots, off, conn_slots, weights):
        slots, off, conn_slots, weights = (np.ascontiguousarray(a, np.int32) for a in (slots, off, conn_slots, weights))
        assert len(off) == len(slots) + 1 and len(conn_slots) == len(weights)
        self.e._chk(self.L.orbfe_covis_set_connections(self.e.h, self.h, len(slots), _p(slots), _p(off), _p(conn_slots) if len(conn_slots) else None,
                                                       _p(weights) if len(weights) else None), "orbfe_covis_set_connections")

    def get_keyframe(self, slot):
        """orbfe_covis_get_keyframe -> dict(mn_id, bad, parent, prev, n_features, covisible, children, conn {slot: weight}); the row's
        order is not observable, so it comes back as a dict (None when connections are not enabled)"""
        rec = CovisKeyframe()
        cov, kids = np.zeros(COVIS_MAX_COVISIBLE, np.int32), np.zeros(self.child_stride, np.int32)
        cs, cw, nc = np.zeros(max(self.conn_stride, 1), np.int32), np.zeros(max(self.conn_stride, 1), np.int32), C.c_int(0)
        on = self.conn_stride > 0
        self.e._chk(self.L.orbfe_covis_get_keyframe(self.e.h, self.h, int(slot), C.byref(rec), _p(cov), _p(kids), _p(cs) if on else None,
                                                    _p(cw) if on else None, C.byref(nc) if on else None), "orbfe_covis_get_keyframe")
        conn = None
        if on:
            assert len(set(cs[:nc.value].tolist())) == nc.value, "a key frame is named twice in a connection row"
            conn = dict(zip(cs[:nc.value].tolist(), cw[:nc.value].tolist()))
        return dict(mn_id=rec.mn_id, bad=rec.bad, parent=rec.parent, prev=rec.prev, n_features=rec.n_features,
                    covisible=cov[:rec.n_covisible].tolist(), children=kids[:rec.n_children].tolist(), conn=conn)

    def update_connections(self, slot, flag=0, params=None):
        """orbfe_covis_update_connections: one key frame -> dict(slots, weights, count, status); raises on status 2 (OrbfeError)"""
        S = self.conn_stride
        sl, w, n, st = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32), C.c_int(0), C.c_int(0)
        params = params or CovisUpdateParams()
        self.e._chk(self.L.orbfe_covis_update_connections(self.e.h, C.byref(params), self.h, int(slot), int(flag), _p(sl), _p(w), C.byref(n),
                                                          C.byref(st)), "orbfe_covis_update_connections")
        return dict(slots=sl, weights=w, count=n.value, status=st.value)

    def update_connections_device(self, slots, flags, io, params=None, stream=None):
        """orbfe_covis_update_connections_device: slots / flags are HOST arrays, io a CovisUpdateIO of raw device pointers"""
        slots, flags = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(flags, np.int32)
        assert len(slots) == len(flags)
        params = params or CovisUpdateParams()
        self.e._chk(self.L.orbfe_covis_update_connections_device(self.e.h, C.byref(params), self.h, len(slots), _p(slots), _p(flags), C.byref(io),
                                                                 stream), "orbfe_covis_update_connections_device")

    def add_keyframe_device(self, slot, mn_id, d_point_ids_ptr, n_features, d_added_ptr, d_status_ptr, bad=0, parent=-1, prev=-1, stream=None):
        """orbfe_covis_add_keyframe_device: the graph part of LocalMapping::ProcessNewKeyFrame; raw device pointers"""
        rec = CovisKeyframe(slot=int(slot), mn_id=int(mn_id), bad=int(bad), parent=int(parent), prev=int(prev))
        self.e._chk(self.L.orbfe_covis_add_keyframe_device(self.e.h, self.h, C.byref(rec), d_point_ids_ptr, int(n_features), d_added_ptr,
                                                           d_status_ptr, stream), "orbfe_covis_add_keyframe_device")

    def add_keyframe(self, slot, mn_id, point_ids, bad=0, parent=-1, prev=-1):
        """orbfe_covis_add_keyframe: the same from a host array -> dict(added, status); raises on status 2 (OrbfeError)"""
        ids = np.ascontiguousarray(point_ids, np.int32)
        added, st = np.zeros(max(len(ids), 1), np.int32), C.c_int(0)
        rec = CovisKeyframe(slot=int(slot), mn_id=int(mn_id), bad=int(bad), parent=int(parent), prev=int(prev), n_features=len(ids),
                            point_ids=ids.ctypes.data if len(ids) else None)
        self.e._chk(self.L.orbfe_covis_add_keyframe(self.e.h, self.h, C.byref(rec), _p(added), C.byref(st)), "orbfe_covis_add_keyframe")
        return dict(added=added[:len(ids)], status=st.value)

    # ---- SPEC DECISION S26: map points refreshed from the graph ----
    n_levels = 0

    def enable_refresh(self, scale_factors):
        """orbfe_covis_enable_refresh: descriptors, octaves and centres per key frame, feature indices and mpRefKF per point"""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        self.e._chk(self.L.orbfe_covis_enable_refresh(self.e.h, self.h, len(sf), _p(sf)), "orbfe_covis_enable_refresh")
        self.n_levels = len(sf)

    def set_features(self, slot, kp, desc):
        kp, desc = np.ascontiguousarray(kp, KP_DTYPE), np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(kp) == len(desc)
        self.e._chk(self.L.orbfe_covis_set_features(self.e.h, self.h, int(slot), len(kp), _p(kp) if len(kp) else None,
                                                    _p(desc) if len(kp) else None), "orbfe_covis_set_features")

    def set_features_device(self, slot, d_kp_ptr, d_desc_ptr, n, stream=None):
        """orbfe_covis_set_features_device: the arrays an extraction left in HBM; raw device pointers"""
        self.e._chk(self.L.orbfe_covis_set_features_device(self.e.h, self.h, int(slot), d_kp_ptr, d_desc_ptr, int(n), stream),
                    "orbfe_covis_set_features_device")

    def set_centres(self, slots, twc):
        slots, twc = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(twc, np.float32).reshape(-1, 3)
        assert len(slots) == len(twc)
        self.e._chk(self.L.orbfe_covis_set_centres(self.e.h, self.h, len(slots), _p(slots), _p(twc)), "orbfe_covis_set_centres")

    def set_observations_indexed(self, ids, off, kf_slots, feat_idx):
        ids, off, kf_slots, feat_idx = (np.ascontiguousarray(a, np.int32) for a in (ids, off, kf_slots, feat_idx))
        assert len(off) == len(ids) + 1 and len(kf_slots) == len(feat_idx)
        self.e._chk(self.L.orbfe_covis_set_observations_indexed(self.e.h, self.h, len(ids), _p(ids), _p(off), _p(kf_slots) if len(kf_slots) else None,
                                                                _p(feat_idx) if len(feat_idx) else None), "orbfe_covis_set_observations_indexed")

    def set_ref_keyframes(self, ids, ref_slots):
        ids, ref_slots = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(ref_slots, np.int32)
        assert len(ids) == len(ref_slots)
        self.e._chk(self.L.orbfe_covis_set_ref_keyframes(self.e.h, self.h, len(ids), _p(ids), _p(ref_slots)), "orbfe_covis_set_ref_keyframes")

    def get_point(self, id_):
        """orbfe_covis_get_point -> dict(obs [(slot, index)], ref, record (WP_DTYPE scalar), desc (32 bytes))"""
        n, ref = C.c_int(0), C.c_int(0)
        sl, ix = np.zeros(self.obs_stride, np.int32), np.zeros(self.obs_stride, np.int32)
        rec, desc = np.zeros(1, WP_DTYPE), np.zeros(32, np.uint8)
        self.e._chk(self.L.orbfe_covis_get_point(self.e.h, self.h, int(id_), C.byref(n), _p(sl), _p(ix), C.byref(ref), _p(rec), _p(desc)),
                    "orbfe_covis_get_point")
        return dict(obs=list(zip(sl[:n.value].tolist(), ix[:n.value].tolist())), ref=ref.value, record=rec[0], desc=desc)

    def refresh_points_device(self, n, d_ids_ptr, what, io, d_select_ptr=None, select_value=0, stream=None):
        """orbfe_covis_refresh_points_device: raw device pointers, io a RefreshIO"""
        self.e._chk(self.L.orbfe_covis_refresh_points_device(self.e.h, self.h, int(n), d_ids_ptr, d_select_ptr, int(select_value), int(what),
                                                             C.byref(io), stream), "orbfe_covis_refresh_points_device")

    def refresh_points(self, ids, what=3):
        """orbfe_covis_refresh_points: a host list -> dict(status, min_distance, max_distance, best_slot, best_index, best_median)"""
        ids = np.ascontiguousarray(ids, np.int32)
        n = max(len(ids), 1)
        out = dict(status=np.zeros(n, np.int32), min_distance=np.zeros(n, np.float32), max_distance=np.zeros(n, np.float32),
                   best_slot=np.zeros(n, np.int32), best_index=np.zeros(n, np.int32), best_median=np.zeros(n, np.int32))
        self.e._chk(self.L.orbfe_covis_refresh_points(self.e.h, self.h, len(ids), _p(ids), int(what), *(_p(out[k]) for k in (
            "status", "min_distance", "max_distance", "best_slot", "best_index", "best_median"))), "orbfe_covis_refresh_points")
        return {k: v[:len(ids)] for k, v in out.items()}

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_covis_destroy(self.h)
            self.h = None

    __del__ = close


class ExtractStream:
    """orbfe_stream_*: a ring of pinned + device slots; submit() enqueues upload, kernels and download of up to
    `slot_frames` frames without waiting, collect() waits for the oldest submission only."""

    def __init__(self, ex, slots, slot_frames):
        self.ex, self.L = ex, ex.L
        self.slot_frames = slot_frames
        h = C.c_void_p()
        ex._chk(self.L.orbfe_stream_create(ex.h, slots, slot_frames, C.byref(h)), "orbfe_stream_create")
        self.h = h
        cap, nl = ex.cap, ex.nlevels
        self._kp = np.zeros((slot_frames, cap), KP_DTYPE)
        self._desc = np.zeros((slot_frames, cap, 32), np.uint8)
        self._n = np.zeros(slot_frames, np.int32)
        self._per = np.zeros((slot_frames, nl), np.int32)

    def close(self):
        if self.h:
            self.L.orbfe_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def in_flight(self):
        return self.L.orbfe_stream_in_flight(self.h)

    def submit_ptrs(self, ptrs, pitch, n):
        """ptrs: ctypes array of `n` host frame addresses; returns False when every slot is in flight."""
        rc = self.L.orbfe_stream_submit(self.h, ptrs, pitch, n)
        if rc == ERR_BUSY:
            return False
        self.ex._chk(rc, "orbfe_stream_submit")
        return True

    def submit(self, frames, pitch=None):
        """frames: [n][H][W] uint8 array (numpy, or anything exposing ctypes data) in host memory."""
        n = len(frames)
        base = frames.ctypes.data
        stride = frames.strides[0]
        ptrs = (C.c_void_p * n)(*[base + b * stride for b in range(n)])
        return self.submit_ptrs(ptrs, pitch or frames.strides[1], n)

    def collect_raw(self):
        """Results of the oldest submission in the stream's own arrays (overwritten by the next collect)."""
        nf = C.c_int()
        self.ex._chk(self.L.orbfe_stream_collect(self.h, _p(self._kp), _p(self._desc), _p(self._n), _p(self._per), C.byref(nf)),
                     "orbfe_stream_collect")
        return nf.value, self._kp, self._desc, self._n, self._per

    def collect(self):
        nf, kp, desc, n, per = self.collect_raw()
        return [(kp[b, :n[b]].copy(), desc[b, :n[b]].copy(), per[b].copy()) for b in range(nf)]

    # ---- extract-and-match submissions (orbfe_stream_enable_track / submit_track / collect_track) ----
    def enable_track(self, map_points, max_points, gridCols, gridRows, minX, minY, maxX, maxY):
        self.ex._chk(self.L.orbfe_stream_enable_track(self.h, map_points.h, int(max_points)), "orbfe_stream_enable_track")
        self._map = map_points
        self._grid = (int(gridCols), int(gridRows), float(minX), float(minY),
                      float(np.float32(gridCols) / np.float32(np.float32(maxX) - np.float32(minX))),
                      float(np.float32(gridRows) / np.float32(np.float32(maxY) - np.float32(minY))))
        self._match = np.full((self.slot_frames, self.ex.cap), -1, np.int32)
        self._nmatch = np.zeros(self.slot_frames, np.int32)

    def submit_track(self, frames, frusta, ids, th, nnRatio, bFarPoints=False, thFarPoints=0.0, pitch=None):
        """frames as submit(); frusta: ctypes array (Frustum * n) or list of Frustum; ids: [n][n_points] int32 (id >= 0:
        entry of the resident map, ~id: the entry with mnLastFrameSeen == current frame, i.e. skipped)."""
        n = len(frames)
        if not isinstance(frusta, C.Array):
            frusta = (Frustum * n)(*frusta)
        ids = np.ascontiguousarray(ids, np.int32)
        assert ids.ndim == 2 and ids.shape[0] == n
        tp = TrackParams()
        (tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y, tp.grid_inv_w, tp.grid_inv_h) = self._grid
        tp.th, tp.nn_ratio, tp.far_points, tp.th_far_points = th, nnRatio, int(bFarPoints), thFarPoints
        base, stride = frames.ctypes.data, frames.strides[0]
        ptrs = (C.c_void_p * n)(*[base + b * stride for b in range(n)])
        rc = self.L.orbfe_stream_submit_track(self.h, ptrs, pitch or frames.strides[1], n, C.byref(tp), frusta, ids.shape[1], _p(ids))
        if rc == ERR_BUSY:
            return False
        self.ex._chk(rc, "orbfe_stream_submit_track")
        return True

    def collect_track_raw(self):
        nf = C.c_int()
        self.ex._chk(self.L.orbfe_stream_collect_track(self.h, _p(self._kp), _p(self._desc), _p(self._n), _p(self._per), _p(self._match),
                                                       _p(self._nmatch), C.byref(nf)), "orbfe_stream_collect_track")
        return nf.value, self._kp, self._desc, self._n, self._per, self._match, self._nmatch

    def collect_track(self):
        nf, kp, desc, n, per, match, nm = self.collect_track_raw()
        return [(kp[b, :n[b]].copy(), desc[b, :n[b]].copy(), per[b].copy(), match[b, :n[b]].copy(), int(nm[b])) for b in range(nf)]

    def collect_view(self):
        """orbfe_stream_collect_view: the oldest submission's results as numpy VIEWS of the slot's pinned block (no
        copy); they stay valid until the submission that reuses the slot, `slots` submissions later.
        Returns (n_frames, kp[slot_frames][cap], desc[slot_frames][cap][32], n[slot_frames], per[slot_frames][levels])."""
        kp, desc, n, per = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        nf = C.c_int()
        self.ex._chk(self.L.orbfe_stream_collect_view(self.h, C.byref(kp), C.byref(desc), C.byref(n), C.byref(per), C.byref(nf)),
                     "orbfe_stream_collect_view")
        cap, nl, sf = self.ex.cap, self.ex.nlevels, self.slot_frames

        def view(ptr, nbytes, dtype, shape):
            return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr.value), dtype=dtype).reshape(shape)

        return (nf.value, view(kp, sf * cap * 24, KP_DTYPE, (sf, cap)), view(desc, sf * cap * 32, np.uint8, (sf, cap, 32)),
                view(n, sf * 4, np.int32, (sf,)), view(per, sf * nl * 4, np.int32, (sf, nl)))


def shard_range(n_frames, k, n_members):
    """orbfe_shard_range: the block [lo, hi) of n_frames that member k of n_members owns (host only)."""
    lo, hi = C.c_int(), C.c_int()
    rc = lib().orbfe_shard_range(int(n_frames), int(k), int(n_members), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise OrbfeError(rc, "orbfe_shard_range")
    return lo.value, hi.value


def _frame_ptrs(frames):
    """[n][H][W] host frames (numpy, or a list of [H][W] arrays) -> (ctypes array of n row-0 addresses, row pitch)"""
    if isinstance(frames, np.ndarray):
        base, stride = frames.ctypes.data, frames.strides[0]
        return (C.c_void_p * len(frames))(*[base + b * stride for b in range(len(frames))]), frames.strides[1]
    return (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames]), frames[0].strides[0]


class Pool:
    """orbfe_pool_*: the batched many-frame mode over several GPUs.  Member k is a handle on devices[k] (a device may repeat)
    with a ring of `slots` x `slot_frames`; the frames of a call are sharded over the members in contiguous blocks
    (shard_range) and every member runs its block through its own ring on a worker thread of its own.  Results are those of
    one ORBextractor's extract_batch / one FrameTracker's TrackFrameMap, frame by frame."""

    def __init__(self, args, devices, slots=3, slot_frames=None, max_batch=None):
        self.L = lib()
        self.h = None
        max_batch = int(max_batch or slot_frames or 64)
        self.slot_frames = int(slot_frames or max_batch)
        self.W, self.H = int(args[6]), int(args[7])
        prm = Params(*args, 0, max_batch)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.L.orbfe_pool_create(C.byref(prm), devs, len(devices), int(slots), self.slot_frames, C.byref(h))
        if rc != 0:
            raise OrbfeError(rc, "orbfe_pool_create")
        self.h = h
        self.size = self.L.orbfe_pool_size(self.h)
        m0 = self.L.orbfe_pool_member(self.h, 0)
        self.cap = self.L.orbfe_max_keypoints(m0)
        self.nlevels = self.L.orbfe_get_levels(m0)
        self._grid = None

    def _chk(self, rc, where):
        if rc != 0:
            raise OrbfeError(rc, where, self.L.orbfe_pool_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_pool_destroy(self.h)
            self.h = None

    __del__ = close

    def member_frames(self):
        return [self.L.orbfe_pool_member_frames(self.h, k) for k in range(self.size)]

    def extract_raw(self, frames, pitch=None, out=None):
        """orbfe_pool_extract into frame-major arrays (kp[n][cap], desc[n][cap][32], n[n], per[n][levels]); `out` reuses them"""
        ptrs, p = _frame_ptrs(frames)
        n = len(frames)
        kp, desc, cnt, per = out if out is not None else (np.zeros((n, self.cap), KP_DTYPE), np.zeros((n, self.cap, 32), np.uint8),
                                                          np.zeros(n, np.int32), np.zeros((n, self.nlevels), np.int32))
        self._chk(self.L.orbfe_pool_extract(self.h, ptrs, int(pitch or p), n, _p(kp), _p(desc), _p(cnt), _p(per)), "orbfe_pool_extract")
        return kp, desc, cnt, per

    def extract(self, frames, pitch=None):
        """per frame (kp, desc, per_level) as ORBextractor.extract_batch"""
        kp, desc, n, per = self.extract_raw(frames, pitch)
        return [(kp[b, :n[b]].copy(), desc[b, :n[b]].copy(), per[b].copy()) for b in range(len(n))]

    def enable_track(self, capacity, max_points, gridCols, gridRows, minX, minY, maxX, maxY):
        """one resident map of `capacity` entries per member; every ring takes up to max_points map points per frame"""
        self._chk(self.L.orbfe_pool_enable_track(self.h, int(capacity), int(max_points)), "orbfe_pool_enable_track")
        self._grid = (int(gridCols), int(gridRows), float(minX), float(minY),
                      float(np.float32(gridCols) / np.float32(np.float32(maxX) - np.float32(minX))),
                      float(np.float32(gridRows) / np.float32(np.float32(maxY) - np.float32(minY))))

    def map_update(self, ids, points, desc):
        ids = np.ascontiguousarray(ids, np.int32)
        points = np.ascontiguousarray(points, WP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        assert len(ids) == len(points) == len(desc)
        self._chk(self.L.orbfe_pool_map_update(self.h, len(ids), _p(ids), _p(points), _p(desc)), "orbfe_pool_map_update")

    def track_params(self, th, nnRatio, bFarPoints=False, thFarPoints=0.0):
        tp = TrackParams()
        if self._grid is not None:
            (tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y, tp.grid_inv_w, tp.grid_inv_h) = self._grid
        tp.th, tp.nn_ratio, tp.far_points, tp.th_far_points = th, nnRatio, int(bFarPoints), thFarPoints
        return tp

    def track_raw(self, frames, frusta, ids, tp, pitch=None, out=None):
        """orbfe_pool_track into frame-major arrays (kp, desc, n, per, match[n][cap], nmatch[n])"""
        ptrs, p = _frame_ptrs(frames)
        n = len(frames)
        if not isinstance(frusta, C.Array):
            frusta = (Frustum * n)(*frusta)
        ids = np.ascontiguousarray(ids, np.int32)
        assert ids.ndim == 2 and ids.shape[0] == n
        kp, desc, cnt, per, match, nm = out if out is not None else (
            np.zeros((n, self.cap), KP_DTYPE), np.zeros((n, self.cap, 32), np.uint8), np.zeros(n, np.int32),
            np.zeros((n, self.nlevels), np.int32), np.full((n, self.cap), -1, np.int32), np.zeros(n, np.int32))
        self._chk(self.L.orbfe_pool_track(self.h, ptrs, int(pitch or p), n, C.byref(tp), frusta, ids.shape[1], _p(ids), _p(kp), _p(desc),
                                          _p(cnt), _p(per), _p(match), _p(nm)), "orbfe_pool_track")
        return kp, desc, cnt, per, match, nm

    def track(self, frames, frusta, ids, th, nnRatio, bFarPoints=False, thFarPoints=0.0, pitch=None):
        """per frame (kp, desc, per_level, match, n_matches) as ExtractStream.collect_track; frusta: one Frustum per frame,
        ids: [n][n_points] int32 (id >= 0, ~id = skipped, outside the map = no point)"""
        kp, desc, n, per, match, nm = self.track_raw(frames, frusta, ids, self.track_params(th, nnRatio, bFarPoints, thFarPoints), pitch)
        return [(kp[b, :n[b]].copy(), desc[b, :n[b]].copy(), per[b].copy(), match[b, :n[b]].copy(), int(nm[b])) for b in range(len(n))]


class ORBmatcher:
    """ORB_SLAM3::ORBmatcher (include/ORBmatcher.h:36-84); statics bound to one extractor handle."""
    TH_LOW = 30
    TH_HIGH = 100
    HISTO_LENGTH = 30

    def __init__(self, extractor):
        self.e = extractor
        self.L = extractor.L

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().orbfe_hamming(_p(a), _p(b))

    def SearchByProjection(self, fv, mps, mpDesc, th, bFarPoints, thFarPoints, nnRatio, initObs=None):
        mps = np.ascontiguousarray(mps, MP_DTYPE)
        mpDesc = np.ascontiguousarray(mpDesc, np.uint8)
        io = None if initObs is None else np.ascontiguousarray(initObs, np.int32)
        out = np.full(max(1, fv.n), -1, np.int32)
        n = C.c_int()
        self.e._chk(self.L.orbfe_match_projection(self.e.h, C.byref(fv), len(mps), _p(mps), _p(mpDesc), _p(io), th,
                                                  int(bFarPoints), thFarPoints, nnRatio, _p(out), C.byref(n)),
                    "orbfe_match_projection")
        return n.value, out[:fv.n].copy()

    def SearchByProjection_batch_device(self, batch, d_kp, d_desc, d_n, kp_stride, gridCols, gridRows, minX, minY,
                                        maxX, maxY, M, d_mps, d_mp_desc, d_init_obs, th, nnRatio, d_match_out,
                                        d_n_matches, bFarPoints=False, thFarPoints=0.0, stream=None):
        """Batched HBM-resident SearchByProjection; all d_* are raw device pointers (ints)."""
        invw = float(np.float32(gridCols) / np.float32(np.float32(maxX) - np.float32(minX)))
        invh = float(np.float32(gridRows) / np.float32(np.float32(maxY) - np.float32(minY)))
        self.e._chk(self.L.orbfe_match_projection_batch_device(
            self.e.h, batch, d_kp, d_desc, d_n, kp_stride, gridCols, gridRows, minX, minY, invw, invh, M, d_mps,
            d_mp_desc, d_init_obs, th, int(bFarPoints), thFarPoints, nnRatio, d_match_out, d_n_matches, stream),
            "orbfe_match_projection_batch_device")

    def isInFrustum_batch(self, frustum, points):
        """The isInFrustum loop of Tracking::SearchLocalPoints (src/Tracking.cc:1059-1077) for all points at once:
        returns (map point records for SearchByProjection, mTrackProjXR)."""
        points = np.ascontiguousarray(points, WP_DTYPE)
        n = len(points)
        out = np.zeros(max(n, 1), MP_DTYPE)
        xr = np.zeros(max(n, 1), np.float32)
        self.e._chk(self.L.orbfe_project_map_points(self.e.h, C.byref(frustum), n, _p(points), _p(out), _p(xr)),
                    "orbfe_project_map_points")
        return out[:n], xr[:n]

    def SearchForTriangulation(self, off1, idx1, off2, idx2, kp1, desc1, hasMP1, stereo1, kp2, desc2, hasMP2, stereo2,
                               scaleFactors2, F12, ep, bOnlyStereo=False, bCoarse=False, checkOrientation=True, cameras=None):
        """ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:441-676): returns (nmatches, vMatches12).
        cameras (optional) = dict(model1, model2, cam1[8], cam2[8], precision, R12[3x3], t12[3], levelSigma2_1,
        kf1HasCamera2): the camera models of the two key frames; model1 == CAMERA_KANNALA_BRANDT8 selects
        KannalaBrandt8::epipolarConstrain (src/CameraModels/KannalaBrandt8.cpp:216-220)."""
        a32 = lambda v: np.ascontiguousarray(v, np.int32)
        u8 = lambda v: None if v is None else np.ascontiguousarray(v, np.uint8)
        off1, idx1, off2, idx2 = a32(off1), a32(idx1), a32(off2), a32(idx2)
        kp1, kp2 = np.ascontiguousarray(kp1, KP_DTYPE), np.ascontiguousarray(kp2, KP_DTYPE)
        desc1, desc2 = u8(desc1), u8(desc2)
        h1, h2, s1, s2 = u8(hasMP1), u8(hasMP2), u8(stereo1), u8(stereo2)
        sf = np.ascontiguousarray(scaleFactors2, np.float32)
        P = TriParams()
        for i, v in enumerate(np.asarray(F12, np.float32).reshape(-1)):
            P.f12[i] = float(v)
        P.ep_x, P.ep_y = float(ep[0]), float(ep[1])
        P.only_stereo, P.coarse, P.check_orientation = int(bOnlyStereo), int(bCoarse), int(checkOrientation)
        if cameras is not None:
            fill_tri_cameras(P, cameras)
        out = np.full(max(len(kp1), 1), -1, np.int32)
        n = C.c_int()
        self.e._chk(self.L.orbfe_match_triangulation(self.e.h, len(off1) - 1, _p(off1), _p(idx1), _p(off2), _p(idx2), len(kp1),
                                                     _p(kp1), _p(desc1), _p(h1), _p(s1), len(kp2), _p(kp2), _p(desc2), _p(h2),
                                                     _p(s2), _p(sf), len(sf), C.byref(P), _p(out), C.byref(n)),
                    "orbfe_match_triangulation")
        return n.value, out[:len(kp1)].copy()

    def ComputeDistinctiveDescriptors(self, setOff, desc):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:343-416) for a batch of descriptor sets (CSR):
        returns (index of the representative inside each set, its median distance)."""
        setOff = np.ascontiguousarray(setOff, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(setOff) - 1
        bi = np.zeros(max(n, 1), np.int32)
        bm = np.zeros(max(n, 1), np.int32)
        self.e._chk(self.L.orbfe_distinctive_descriptors(self.e.h, n, _p(setOff), _p(desc), _p(bi), _p(bm)),
                    "orbfe_distinctive_descriptors")
        return bi[:n], bm[:n]

    def Fuse_search(self, kf_view, invLevelSigma2, uRight, frustum, th, points, mpDesc):
        """The search part of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:678-836): (bestIdx, bestDist)
        per map point; the caller applies bestDist <= TH_LOW and the graph edits."""
        points = np.ascontiguousarray(points, WP_DTYPE)
        mpDesc = np.ascontiguousarray(mpDesc, np.uint8)
        is2 = np.ascontiguousarray(invLevelSigma2, np.float32)
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        M = len(points)
        bi = np.zeros(max(M, 1), np.int32)
        bd = np.zeros(max(M, 1), np.int32)
        self.e._chk(self.L.orbfe_fuse_search(self.e.h, C.byref(kf_view), _p(is2), _p(ur), C.byref(frustum), th, M,
                                             _p(points), _p(mpDesc), _p(bi), _p(bd)), "orbfe_fuse_search")
        return bi[:M], bd[:M]

    def Fuse_search_keyframe(self, kf, map_points, ids, frustum, th):
        """orbfe_fuse_search_keyframe: the search part of Fuse against a RESIDENT KeyFrame (set_grid done) with the map points
        named by id out of a resident MapPoints table (id >= 0; ~id = "!pMP || pMP->IsInKeyFrame(pKF)" for this call; outside
        the map = no point) -> (bestIdx, bestDist) per id."""
        ids = np.ascontiguousarray(ids, np.int32)
        M = len(ids)
        bi = np.zeros(max(M, 1), np.int32)
        bd = np.zeros(max(M, 1), np.int32)
        self.e._chk(self.L.orbfe_fuse_search_keyframe(self.e.h, kf.h, map_points.h, M, _p(ids), C.byref(frustum), th, _p(bi), _p(bd)),
                    "orbfe_fuse_search_keyframe")
        return bi[:M], bd[:M]

    def Fuse_search_keyframes(self, kfs, map_points, ids, frusta, th, skip=None, cand_cap=0):
        """orbfe_fuse_search_keyframes: Fuse_search_keyframe into all K targets of one SearchInNeighbors loop in ONE submission.
        kfs / frusta: K resident KeyFrames (set_grid done) and their Frustums; ids: M entries of the map; skip: (K, M) flags
        "!pMP || pMP->IsInKeyFrame(pKFk)" or None.  -> (bestIdx, bestDist) shaped (K, M); with cand_cap > 0 also
        (candIdx (K, M, cand_cap), candCount (K, M)): the features that passed every gate, in visit order, for fuse_select."""
        ids = np.ascontiguousarray(ids, np.int32)
        K, M = len(kfs), len(ids)
        assert len(frusta) == K
        fr = (Frustum * max(K, 1))()
        for k in range(K):
            C.memmove(C.byref(fr, k * C.sizeof(Frustum)), C.byref(frusta[k]), C.sizeof(Frustum))
        hs = (C.c_void_p * max(K, 1))(*[kf.h.value for kf in kfs])
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8)
            assert skip.shape == (K, M)
        n = max(K * M, 1)
        bi = np.zeros(n, np.int32)
        bd = np.zeros(n, np.int32)
        ci_ = np.zeros(n * max(cand_cap, 1), np.int32)
        cc = np.zeros(n, np.int32)
        self.e._chk(self.L.orbfe_fuse_search_keyframes(self.e.h, K, hs, fr, map_points.h, M, _p(ids), _p(skip), th, _p(bi), _p(bd),
                                                       cand_cap, _p(ci_), _p(cc)), "orbfe_fuse_search_keyframes")
        out = bi[:K * M].reshape(K, M), bd[:K * M].reshape(K, M)
        if cand_cap > 0:
            out += (ci_[:K * M * cand_cap].reshape(K, M, cand_cap), cc[:K * M].reshape(K, M))
        return out

    def Fuse_search_right(self, kf_left_view, nRight, invLevelSigma2, uRight, frustum, th, points, mpDesc):
        """Fuse(pKF, vpMapPoints, th, bRight = true) (src/ORBmatcher.cc:684-688,:820): kf_left_view describes the NLeft left
        features with desc = all NLeft + nRight rows of mDescriptors; frustum = right pose / mpCamera2; returned indices are
        idx + NLeft."""
        points = np.ascontiguousarray(points, WP_DTYPE)
        mpDesc = np.ascontiguousarray(mpDesc, np.uint8)
        is2 = np.ascontiguousarray(invLevelSigma2, np.float32)
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        M = len(points)
        bi = np.zeros(max(M, 1), np.int32)
        bd = np.zeros(max(M, 1), np.int32)
        self.e._chk(self.L.orbfe_fuse_search_right(self.e.h, C.byref(kf_left_view), int(nRight), _p(is2), _p(ur), C.byref(frustum),
                                                   th, M, _p(points), _p(mpDesc), _p(bi), _p(bd)), "orbfe_fuse_search_right")
        return bi[:M], bd[:M]

    def Fuse_search_sim3(self, kf_view, frustum, th, points, mpDesc):
        """The search part of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:864-975)."""
        points = np.ascontiguousarray(points, WP_DTYPE)
        mpDesc = np.ascontiguousarray(mpDesc, np.uint8)
        M = len(points)
        bi = np.zeros(max(M, 1), np.int32)
        bd = np.zeros(max(M, 1), np.int32)
        self.e._chk(self.L.orbfe_fuse_search_sim3(self.e.h, C.byref(kf_view), C.byref(frustum), th, M, _p(points),
                                                  _p(mpDesc), _p(bi), _p(bd)), "orbfe_fuse_search_sim3")
        return bi[:M], bd[:M]

    def SearchBySim3(self, kf1_view, kf2_view, dir12, dir21, mp1, mpDesc1, mp2, mpDesc2, th):
        """include/ORBmatcher.h:63 -> (nFound, match12) with match12[i1] = feature of key frame 2 or -1."""
        mp1 = np.ascontiguousarray(mp1, WP_DTYPE)
        mp2 = np.ascontiguousarray(mp2, WP_DTYPE)
        assert len(mp1) == kf1_view.n and len(mp2) == kf2_view.n
        mpDesc1 = np.ascontiguousarray(mpDesc1, np.uint8)
        mpDesc2 = np.ascontiguousarray(mpDesc2, np.uint8)
        out = np.full(max(1, kf1_view.n), -1, np.int32)
        n = C.c_int()
        self.e._chk(self.L.orbfe_search_by_sim3(self.e.h, C.byref(kf1_view), C.byref(kf2_view), C.byref(dir12),
                                                C.byref(dir21), _p(mp1), _p(mpDesc1), _p(mp2), _p(mpDesc2), th, _p(out),
                                                C.byref(n)), "orbfe_search_by_sim3")
        return n.value, out[:kf1_view.n]

    def SearchByProjection_keyframe(self, fv, frustum, points, mpDesc, kfAngle, frameHasMP, th, checkOrientation=True):
        """include/ORBmatcher.h:48 (relocalisation overload) -> (nmatches, match) with match[i2] = key-frame feature
        whose map point lands in CurrentFrame->mvpMapPoints[i2], or -1."""
        points = np.ascontiguousarray(points, WP_DTYPE)
        mpDesc = np.ascontiguousarray(mpDesc, np.uint8)
        ang = None if kfAngle is None else np.ascontiguousarray(kfAngle, np.float32)
        has = None if frameHasMP is None else np.ascontiguousarray(frameHasMP, np.uint8)
        out = np.full(max(1, fv.n), -1, np.int32)
        n = C.c_int()
        self.e._chk(self.L.orbfe_match_projection_keyframe(self.e.h, C.byref(fv), C.byref(frustum), len(points),
                                                           _p(points), _p(mpDesc), _p(ang), _p(has), th,
                                                           int(bool(checkOrientation)), _p(out), C.byref(n)),
                    "orbfe_match_projection_keyframe")
        return n.value, out[:fv.n]

    def isInFrustum_batch_device(self, frustum, n, d_points, d_out, d_proj_xr=None, stream=None):
        self.e._chk(self.L.orbfe_project_map_points_device(self.e.h, C.byref(frustum), n, d_points, d_out, d_proj_xr,
                                                           stream), "orbfe_project_map_points_device")

    def SearchForInitialization(self, fv1, fv2, windowSize, nnRatio, checkOrientation=True):
        """include/ORBmatcher.h:58 -> (nmatches, vnMatches12)."""
        out = np.full(max(1, fv1.n), -1, np.int32)
        n = C.c_int()
        self.e._chk(self.L.orbfe_match_initialization(self.e.h, C.byref(fv1), C.byref(fv2), int(windowSize), nnRatio,
                                                      int(checkOrientation), _p(out), C.byref(n)),
                    "orbfe_match_initialization")
        return n.value, out[:fv1.n].copy()

    def SearchByBoW(self, kfOff, kfIdx, fOff, fIdx, kfDesc, kfAngle, kfHasMP, fDesc, fAngle, nnRatio,
                    checkOrientation=True, nLeft=-1):
        a32 = lambda v: np.ascontiguousarray(v, np.int32)
        kfOff, kfIdx, fOff, fIdx = a32(kfOff), a32(kfIdx), a32(fOff), a32(fIdx)
        kfDesc = np.ascontiguousarray(kfDesc, np.uint8)
        fDesc = np.ascontiguousarray(fDesc, np.uint8)
        kfAngle = np.ascontiguousarray(kfAngle, np.float32)
        fAngle = np.ascontiguousarray(fAngle, np.float32)
        kfHasMP = np.ascontiguousarray(kfHasMP, np.uint8)
        out = np.full(max(1, len(fDesc)), -1, np.int32)
        n = C.c_int()
        self.e._chk(self.L.orbfe_match_bow_rig(self.e.h, len(kfOff) - 1, _p(kfOff), _p(kfIdx), _p(fOff), _p(fIdx),
                                               len(kfDesc), _p(kfDesc), _p(kfAngle), _p(kfHasMP), len(fDesc), _p(fDesc),
                                               _p(fAngle), int(nLeft), nnRatio, int(checkOrientation), _p(out), C.byref(n)),
                    "orbfe_match_bow_rig")
        return n.value, out[:len(fDesc)].copy()


def tri_params(F12, ep, bOnlyStereo=False, bCoarse=False, checkOrientation=True, cameras=None):
    """orbfe_tri_params of one key-frame pair (see ORBmatcher.SearchForTriangulation)"""
    P = TriParams()
    for i, v in enumerate(np.asarray(F12, np.float32).reshape(-1)):
        P.f12[i] = float(v)
    P.ep_x, P.ep_y = float(ep[0]), float(ep[1])
    P.only_stereo, P.coarse, P.check_orientation = int(bOnlyStereo), int(bCoarse), int(checkOrientation)
    if cameras is not None:
        fill_tri_cameras(P, cameras)
    return P


class KeyFrame:
    """A key frame resident in HBM (orbfe_keyframe_*): mvKeysUn, mDescriptors, mFeatVec (as the node of every feature, -1 =
    none), mvuRight >= 0, mvScaleFactors -- what the key-frame matchers read and what never changes after construction."""

    def __init__(self, extractor, kp, desc, nodeId, scaleFactors, stereo=None):
        self.e, self.L = extractor, extractor.L
        kp = np.ascontiguousarray(kp, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        node = np.ascontiguousarray(nodeId, np.int32)
        sf = np.ascontiguousarray(scaleFactors, np.float32)
        st = None if stereo is None else np.ascontiguousarray(stereo, np.uint8)
        assert len(desc) == len(kp) == len(node)
        self.n = len(kp)
        self.h = C.c_void_p()
        extractor._chk(self.L.orbfe_keyframe_create(extractor.h, self.n, _p(kp), _p(desc), _p(node), _p(st), _p(sf), len(sf),
                                                    C.byref(self.h)), "orbfe_keyframe_create")

    def set_grid(self, gridCols, gridRows, minX, minY, maxX, maxY, invLevelSigma2, uRight=None):
        """orbfe_keyframe_set_grid: mGrid's geometry (as make_frame_view derives it, src/Frame.cc:101-105), mvInvLevelSigma2 and
        mvuRight -- the per-level cell tables are built once and stay with the key frame (Fuse_search_keyframe)."""
        invw = float(np.float32(gridCols) / np.float32(np.float32(maxX) - np.float32(minX)))
        invh = float(np.float32(gridRows) / np.float32(np.float32(maxY) - np.float32(minY)))
        is2 = np.ascontiguousarray(invLevelSigma2, np.float32)
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        assert ur is None or len(ur) == self.n
        self.e._chk(self.L.orbfe_keyframe_set_grid(self.e.h, self.h, int(gridCols), int(gridRows), float(minX), float(minY), invw, invh,
                                                   _p(is2), _p(ur)), "orbfe_keyframe_set_grid")

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_keyframe_destroy(self.h)
            self.h = None

    __del__ = close


class InitialFrame:
    """mInitialFrame of Tracking::MonocularInitialization (src/Tracking.cc:569-586) resident in HBM (orbfe_init_frame_*): the
    keypoints and descriptors every following frame is matched against while the map is being initialised."""

    def __init__(self, extractor, kp, desc):
        self.e, self.L = extractor, extractor.L
        kp = np.ascontiguousarray(kp, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        assert len(kp) == len(desc)
        self.n = len(kp)
        self.h = C.c_void_p()
        extractor._chk(self.L.orbfe_init_frame_create(extractor.h, self.n, _p(kp), _p(desc), C.byref(self.h)), "orbfe_init_frame_create")

    def close(self):
        if getattr(self, "h", None):
            self.L.orbfe_init_frame_destroy(self.h)
            self.h = None

    __del__ = close


def SearchForTriangulation_batch(extractor, kf1, hasMP1, kf2s, hasMP2s, params):
    """orbfe_match_triangulation_batch: key frame kf1 against the neighbours kf2s in ONE launch -> (raw_match12 [K][n1],
    raw_bin [K][n1]); walk the neighbours in order with triangulation_select and the flags as they stand then."""
    K = len(kf2s)
    h1 = np.ascontiguousarray(hasMP1, np.uint8)
    h2 = [np.ascontiguousarray(v, np.uint8) for v in hasMP2s]
    kfp = (C.c_void_p * max(K, 1))(*[k.h.value for k in kf2s])
    h2p = (C.c_void_p * max(K, 1))(*[v.ctypes.data for v in h2])
    P = (TriParams * max(K, 1))(*params)
    raw = np.full((max(K, 1), max(kf1.n, 1)), -1, np.int32)
    rbin = np.zeros((max(K, 1), max(kf1.n, 1)), np.uint8)
    extractor._chk(extractor.L.orbfe_match_triangulation_batch(extractor.h, kf1.h, _p(h1), K, kfp, h2p, P, _p(raw), _p(rbin)),
                   "orbfe_match_triangulation_batch")
    return raw[:K, :kf1.n], rbin[:K, :kf1.n]


def CreateNewMapPoints_batch(extractor, kf1, hasMP1, kf2s, hasMP2s, params, np_params):
    """orbfe_create_new_points_batch: SearchForTriangulation_batch + the geometry of src/LocalMapping.cc:571-705 for every raw
    partner in the same submission -> (raw_match12 [K][n1], raw_bin [K][n1], x3d [K][n1][3], verdict [K][n1]); walk the
    neighbours in order with triangulation_select and create the points whose verdict is NEWPT_ACCEPTED."""
    K = len(kf2s)
    h1 = np.ascontiguousarray(hasMP1, np.uint8)
    h2 = [np.ascontiguousarray(v, np.uint8) for v in hasMP2s]
    kfp = (C.c_void_p * max(K, 1))(*[k.h.value for k in kf2s])
    h2p = (C.c_void_p * max(K, 1))(*[v.ctypes.data for v in h2])
    P = (TriParams * max(K, 1))(*params)
    Q = (NewPointParams * max(K, 1))(*np_params)
    raw = np.full((max(K, 1), max(kf1.n, 1)), -1, np.int32)
    rbin = np.zeros((max(K, 1), max(kf1.n, 1)), np.uint8)
    x3d = np.zeros((max(K, 1), max(kf1.n, 1), 3), np.float32)
    verdict = np.full((max(K, 1), max(kf1.n, 1)), NEWPT_NO_PARTNER, np.uint8)
    extractor._chk(extractor.L.orbfe_create_new_points_batch(extractor.h, kf1.h, _p(h1), K, kfp, h2p, P, Q, _p(raw), _p(rbin), _p(x3d),
                                                             _p(verdict)), "orbfe_create_new_points_batch")
    return raw[:K, :kf1.n], rbin[:K, :kf1.n], x3d[:K, :kf1.n], verdict[:K, :kf1.n]


def triangulate_pairs(extractor, kf1, kf2, np_params, idx1, idx2):
    """orbfe_triangulate_pairs: (x3d [n][3], verdict [n]) of the explicit pairs (idx1[p], idx2[p]) of two resident key frames"""
    i1 = np.ascontiguousarray(idx1, np.int32)
    i2 = np.ascontiguousarray(idx2, np.int32)
    assert len(i1) == len(i2)
    n = len(i1)
    x3d = np.zeros((max(n, 1), 3), np.float32)
    verdict = np.full(max(n, 1), NEWPT_NO_PARTNER, np.uint8)
    extractor._chk(extractor.L.orbfe_triangulate_pairs(extractor.h, kf1.h, kf2.h, C.byref(np_params), n, _p(i1), _p(i2), _p(x3d),
                                                       _p(verdict)), "orbfe_triangulate_pairs")
    return x3d[:n], verdict[:n]


def two_view_reconstruct(extractor, params, kp1, kp2, matches12, sets, want_info=True):
    """orbfe_two_view_reconstruct: TwoViewReconstruction::Reconstruct (src/TwoViewReconstruction.cc:40-127) for a pinhole K.
    kp1 / kp2: KP_DTYPE arrays (mvKeysUn), matches12 [n1] (index in frame 2 or -1), sets [iterations, 8] indices into the match
    list -> dict(reconstructed, R21 [3, 3], t21 [3], p3d [n1, 3], triangulated [n1]) plus, with want_info, every field of
    orbfe_two_view_info under its own name (the optional buffers included)."""
    kp1 = np.ascontiguousarray(kp1, KP_DTYPE)
    kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
    m12 = np.ascontiguousarray(matches12, np.int32)
    assert len(m12) == len(kp1)
    st = None if sets is None else np.ascontiguousarray(sets, np.int32)
    n1, n2 = len(kp1), len(kp2)
    N = int((m12 >= 0).sum())
    it = max(int(params.iterations), 1)
    R21, t21 = np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    p3d, tri = np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
    rec = C.c_int(0)
    info = None
    if want_info:
        info = TwoViewInfo()
        buf = dict(scores=np.zeros(2 * it, np.float32), inliers_H=np.zeros(max(N, 1), np.uint8), inliers_F=np.zeros(max(N, 1), np.uint8),
                   rt_flags=np.zeros((8, max(N, 1)), np.uint8), rt_x3d=np.zeros((8, max(N, 1), 3), np.float32),
                   rt_cos=np.zeros((8, max(N, 1)), np.float32))
        for k, v in buf.items():
            setattr(info, k, v.ctypes.data)
    extractor._chk(extractor.L.orbfe_two_view_reconstruct(extractor.h, C.byref(params), n1, _p(kp1), n2, _p(kp2), _p(m12), _p(st),
                                                          C.byref(rec), _p(R21), _p(t21), _p(p3d), _p(tri),
                                                          C.byref(info) if want_info else None), "orbfe_two_view_reconstruct")
    out = dict(reconstructed=bool(rec.value), R21=R21, t21=t21, p3d=p3d[:n1], triangulated=tri[:n1])
    if want_info:
        out.update(n_matches=info.n_matches, SH=np.float32(info.SH), SF=np.float32(info.SF), RH=np.float32(info.RH), model=info.model,
                   exit_line=info.exit_line, H21=np.array(info.H21, np.float32).reshape(3, 3), F21=np.array(info.F21, np.float32).reshape(3, 3),
                   best_it_H=info.best_it_H, best_it_F=info.best_it_F, n_hypotheses=info.n_hypotheses,
                   best_hypothesis=info.best_hypothesis, n_good=np.array(info.n_good, np.int32),
                   cos_parallax=np.array(info.cos_parallax, np.float32), hyp_R=np.array(info.hyp_R, np.float32).reshape(8, 3, 3),
                   hyp_t=np.array(info.hyp_t, np.float32).reshape(8, 3), scores=buf["scores"], inliers_H=buf["inliers_H"][:N],
                   inliers_F=buf["inliers_F"][:N], rt_flags=buf["rt_flags"].reshape(-1)[:8 * N].reshape(8, N),
                   rt_x3d=buf["rt_x3d"].reshape(-1)[:24 * N].reshape(8, N, 3), rt_cos=buf["rt_cos"].reshape(-1)[:8 * N].reshape(8, N))
    return out


def mlpnp_plan(params, N):
    """orbfe_mlpnp_plan (host-only): (mRansacMinInliers, mRansacMaxIts, passes of a first iterate(n_iterations)) for N correspondences"""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    rc = lib().orbfe_mlpnp_plan(C.byref(params), int(N), C.byref(a), C.byref(b), C.byref(c))
    if rc != 0:
        raise OrbfeError(rc, "orbfe_mlpnp_plan")
    return a.value, b.value, c.value


def mlpnp_ransac(extractor, params, kp, mp_index, points, sets, want_info=True):
    """orbfe_mlpnp_ransac: a fresh MLPnPsolver + SetRansacParameters + one iterate (src/MLPnPsolver.cpp).  kp: KP_DTYPE array
    (mvKeysUn), mp_index [n] (row of points or -1), points [m, 3] float32 world positions, sets [total_iterations, min_set] indices
    into the correspondence list (None when the plan says 0) -> dict(solved, Tcw [4, 4], inliers [n], n_inliers, no_more) plus, with
    want_info, every field of orbfe_mlpnp_info under its own name (the optional buffers included, cut to their used size)."""
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    mi = np.ascontiguousarray(mp_index, np.int32)
    assert len(mi) == len(kp)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    st = None if sets is None else np.ascontiguousarray(sets, np.int32)
    n_sets = 0 if st is None else (len(st) if st.ndim == 2 else st.size // max(int(params.min_set), 1))
    n = len(kp)
    N = int((mi >= 0).sum())
    Tcw, inl = np.zeros((4, 4), np.float32), np.zeros(max(n, 1), np.uint8)
    solved, n_inl, no_more = C.c_int(0), C.c_int(0), C.c_int(0)
    info = None
    if want_info:
        info = MlpnpInfo()
        T = max(n_sets, 1)
        buf = dict(hyp_Rt=np.zeros((T, 12), np.float64), hyp_inliers=np.zeros(T, np.int32), hyp_planar=np.zeros(T, np.uint8),
                   hyp_gn_evals=np.zeros(T, np.int32), hyp_gn_exit=np.zeros(T, np.int32), candidates=np.zeros(T, np.int32),
                   cand_Rt=np.zeros((T, 12), np.float64), cand_inliers=np.zeros(T, np.int32), cand_planar=np.zeros(T, np.uint8),
                   cand_mask=np.zeros(T * max(N, 1), np.uint8))
        for k, v in buf.items():
            setattr(info, k, v.ctypes.data)
    extractor._chk(extractor.L.orbfe_mlpnp_ransac(extractor.h, C.byref(params), n, _p(kp), _p(mi), len(pts), _p(pts), _p(st), n_sets,
                                                  C.byref(solved), _p(Tcw), _p(inl), C.byref(n_inl), C.byref(no_more),
                                                  C.byref(info) if want_info else None), "orbfe_mlpnp_ransac")
    out = dict(solved=bool(solved.value), Tcw=Tcw, inliers=inl[:n], n_inliers=n_inl.value, no_more=bool(no_more.value))
    if want_info:
        T, nc = info.total_iterations, info.n_candidates
        out.update(N=info.N, min_inliers=info.min_inliers, max_its=info.max_its, total_iterations=T, exit_kind=info.exit_kind,
                   returning_iteration=info.returning_iteration, n_candidates=nc, hyp_Rt=buf["hyp_Rt"][:T], hyp_inliers=buf["hyp_inliers"][:T],
                   hyp_planar=buf["hyp_planar"][:T], hyp_gn_evals=buf["hyp_gn_evals"][:T], hyp_gn_exit=buf["hyp_gn_exit"][:T],
                   candidates=buf["candidates"][:nc], cand_Rt=buf["cand_Rt"][:nc], cand_inliers=buf["cand_inliers"][:nc],
                   cand_planar=buf["cand_planar"][:nc], cand_mask=buf["cand_mask"][:nc * info.N].reshape(nc, info.N))
    return out


def pose_optimization(extractor, params, kp, mp_index, points, Rcw, tcw, want_info=True):
    """orbfe_pose_optimization: Optimizer::PoseOptimization (src/Optimizer.cc:765-1067), mono pinhole, SPEC DECISION S14.  kp: KP_DTYPE
    array (mvKeysUn), mp_index [n] (row of points or -1), points [m, 3] float32 world positions, Rcw [9] / tcw [3] float32 = the frame's
    pose -> dict(Tcw [4, 4], outlier [n], n_inliers) plus, with want_info, the fields of orbfe_pose_opt_info as N_e, rounds_run and
    round_pose / round_iterations / round_trials / round_lambda / round_chi2 / round_nbad / round_exit / round_outlier, cut to the
    rounds that ran."""
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    mi = np.ascontiguousarray(mp_index, np.int32)
    assert len(mi) == len(kp)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    R = np.ascontiguousarray(Rcw, np.float32).reshape(9)
    t = np.ascontiguousarray(tcw, np.float32).reshape(3)
    n = len(kp)
    Ne = int((mi >= 0).sum())
    Tcw, outl = np.zeros((4, 4), np.float32), np.zeros(max(n, 1), np.uint8)
    n_inl = C.c_int(0)
    info = None
    if want_info:
        info = PoseOptInfo()
        rbuf = np.zeros(4 * max(Ne, 1), np.uint8)
        info.outlier = rbuf.ctypes.data
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_pose_optimization(h, C.byref(params), n, _p(kp), _p(mi), len(pts), _p(pts), _p(R), _p(t), _p(Tcw), _p(outl),
                                       C.byref(n_inl), C.byref(info) if want_info else None)
    if rc != 0:
        raise OrbfeError(rc, "orbfe_pose_optimization", lib().orbfe_last_error(h).decode() if h else "")
    out = dict(Tcw=Tcw, outlier=outl[:n], n_inliers=n_inl.value)
    if want_info:
        nr, Ne = info.rounds_run, info.N_e
        out.update(N_e=Ne, rounds_run=nr, round_pose=np.array(info.pose, np.float64).reshape(4, 12)[:nr],
                   round_iterations=np.array(info.iterations, np.int32)[:nr], round_trials=np.array(info.trials, np.int32)[:nr],
                   round_lambda=np.array(info.lambda_, np.float64)[:nr], round_chi2=np.array(info.chi2, np.float64)[:nr],
                   round_nbad=np.array(info.n_bad, np.int32)[:nr], round_exit=np.array(info.exit_kind, np.int32)[:nr],
                   round_outlier=rbuf[:nr * Ne].reshape(nr, Ne))
    return out


def pose_optimization_batch_device(extractor, params, batch, d_kp_ptr, d_n_ptr, kp_stride, d_match_ptr, n_map_points, d_points_ptr,
                                   point_stride_frames, d_pose_in_ptr, d_pose_out_ptr, d_outlier_ptr, d_n_inliers_ptr, stream=None):
    """orbfe_pose_optimization_batch_device: one block per frame, everything resident in HBM (raw device pointers as ints: the
    keypoints / counts of extract_batch_device, the matches of match_projection_batch_device, orbfe_world_point records, 12-float
    poses); asynchronous on `stream`."""
    extractor._chk(extractor.L.orbfe_pose_optimization_batch_device(extractor.h, C.byref(params), int(batch), d_kp_ptr, d_n_ptr,
                                                                     int(kp_stride), d_match_ptr, int(n_map_points), d_points_ptr,
                                                                     int(point_stride_frames), d_pose_in_ptr, d_pose_out_ptr, d_outlier_ptr,
                                                                     d_n_inliers_ptr, stream), "orbfe_pose_optimization_batch_device")


def pose_inertial_optimization_last_keyframe(extractor, params, link, kp, mp_index, points, track_depth, Rcw, tcw, Rwb, twb, v, bg, ba,
                                             want_info=True):
    """orbfe_pose_inertial_optimization_last_keyframe: Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:3447-3844), mono
    pinhole, SPEC DECISION S19.  link: an ImuLink or a dict of its fields; kp: KP_DTYPE array (mvKeysUn), mp_index [n] (row of points /
    track_depth or -1), points [m, 3] and track_depth [m] float32; Rcw .. ba: the frame's state, float32 -> dict(Rwb [9], twb, v, bg,
    ba float32, H [15, 15] float64, outlier [n], n_inliers) plus, with want_info, the fields of orbfe_pose_inertial_info as N_e,
    rounds_run, recovered and round_iterations / round_ok / round_nbad / round_state / round_outlier, cut to the rounds that ran."""
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    mi = np.ascontiguousarray(mp_index, np.int32)
    assert len(mi) == len(kp)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    dep = np.ascontiguousarray(track_depth, np.float32).reshape(-1)
    assert len(dep) == len(pts)
    if link is not None and not isinstance(link, ImuLink):
        link = ImuLink(link)
    sin = [np.ascontiguousarray(a, np.float32).reshape(k) for a, k in ((Rcw, 9), (tcw, 3), (Rwb, 9), (twb, 3), (v, 3), (bg, 3), (ba, 3))]
    sout = [np.zeros(k, np.float32) for k in (9, 3, 3, 3, 3)]
    n = len(kp)
    Ne = int((mi >= 0).sum())
    H, outl = np.zeros((15, 15), np.float64), np.zeros(max(n, 1), np.uint8)
    n_inl = C.c_int(0)
    info = None
    if want_info:
        info = PoseInertialInfo()
        rbuf = np.zeros(4 * max(Ne, 1), np.uint8)
        info.outlier = rbuf.ctypes.data
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_pose_inertial_optimization_last_keyframe(h, C.byref(params), C.byref(link) if link is not None else None, n, _p(kp),
                                                              _p(mi), len(pts), _p(pts), _p(dep), *[_p(a) for a in sin],
                                                              *[_p(a) for a in sout], _p(H), _p(outl), C.byref(n_inl),
                                                              C.byref(info) if want_info else None)
    if rc != 0:
        raise OrbfeError(rc, "orbfe_pose_inertial_optimization_last_keyframe", lib().orbfe_last_error(h).decode() if h else "")
    out = dict(Rwb=sout[0], twb=sout[1], v=sout[2], bg=sout[3], ba=sout[4], H=H, outlier=outl[:n], n_inliers=n_inl.value)
    if want_info:
        nr, Ne = info.rounds_run, info.N_e
        out.update(N_e=Ne, rounds_run=nr, recovered=info.recovered, round_iterations=np.array(info.iterations, np.int32)[:nr],
                   round_ok=np.array(info.ok, np.int32)[:nr], round_nbad=np.array(info.n_bad, np.int32)[:nr],
                   round_state=np.array(info.state, np.float64).reshape(4, 21)[:nr], round_outlier=rbuf[:nr * Ne].reshape(nr, Ne))
    return out


def pose_inertial_optimization_batch_device(extractor, params, batch, d_links_ptr, d_kp_ptr, d_n_ptr, kp_stride, d_match_ptr, n_map_points,
                                            d_points_ptr, point_stride_frames, d_track_depth_ptr, d_state_in_ptr, d_state_out_ptr,
                                            d_H_out_ptr, d_outlier_ptr, d_n_inliers_ptr, stream=None):
    """orbfe_pose_inertial_optimization_batch_device: one block per frame, one orbfe_imu_link and one state per frame, everything
    resident in HBM (raw device pointers as ints); asynchronous on `stream`."""
    extractor._chk(extractor.L.orbfe_pose_inertial_optimization_batch_device(
        extractor.h, C.byref(params), int(batch), d_links_ptr, d_kp_ptr, d_n_ptr, int(kp_stride), d_match_ptr, int(n_map_points), d_points_ptr,
        int(point_stride_frames), d_track_depth_ptr, d_state_in_ptr, d_state_out_ptr, d_H_out_ptr, d_outlier_ptr, d_n_inliers_ptr, stream),
        "orbfe_pose_inertial_optimization_batch_device")


def pose_inertial_optimization_last_frame(extractor, params, link, prior, kp, mp_index, points, track_depth, Rcw, tcw, Rwb, twb, v, bg, ba,
                                          want_info=True, want_prior=True):
    """orbfe_pose_inertial_optimization_last_frame: Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:3846-4275), mono
    pinhole, SPEC DECISION S20.  link: an ImuLinkFree or a dict of its fields; prior: a PoseImuPrior or a dict; the other arguments as
    for pose_inertial_optimization_last_keyframe -> dict(Rwb [9], twb, v, bg, ba float32, H30 [30, 30] and Hprior [15, 15] float64
    (Hprior None without want_prior: the marginalisation is skipped), outlier [n], n_inliers, accepted) plus, with want_info, the
    fields of orbfe_pose_inertial_prev_info cut to the rounds that ran.  All outputs are written whatever `accepted` says."""
    kp = np.ascontiguousarray(kp, KP_DTYPE)
    mi = np.ascontiguousarray(mp_index, np.int32)
    assert len(mi) == len(kp)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    dep = np.ascontiguousarray(track_depth, np.float32).reshape(-1)
    assert len(dep) == len(pts)
    if link is not None and not isinstance(link, ImuLinkFree):
        link = ImuLinkFree(link)
    if prior is not None and not isinstance(prior, PoseImuPrior):
        prior = PoseImuPrior(prior)
    sin = [np.ascontiguousarray(a, np.float32).reshape(k) for a, k in ((Rcw, 9), (tcw, 3), (Rwb, 9), (twb, 3), (v, 3), (bg, 3), (ba, 3))]
    sout = [np.zeros(k, np.float32) for k in (9, 3, 3, 3, 3)]
    n = len(kp)
    Ne = int((mi >= 0).sum())
    H30, outl = np.zeros((30, 30), np.float64), np.zeros(max(n, 1), np.uint8)
    Hp = np.zeros((15, 15), np.float64) if want_prior else None
    n_inl, acc = C.c_int(0), C.c_int(0)
    info = None
    if want_info:
        info = PoseInertialPrevInfo()
        rbuf = np.zeros(4 * max(Ne, 1), np.uint8)
        info.outlier = rbuf.ctypes.data
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_pose_inertial_optimization_last_frame(h, C.byref(params), C.byref(link) if link is not None else None,
                                                           C.byref(prior) if prior is not None else None, n, _p(kp), _p(mi), len(pts),
                                                           _p(pts), _p(dep), *[_p(a) for a in sin], *[_p(a) for a in sout], _p(H30),
                                                           _p(Hp) if want_prior else None, _p(outl), C.byref(n_inl), C.byref(acc),
                                                           C.byref(info) if want_info else None)
    if rc != 0:
        raise OrbfeError(rc, "orbfe_pose_inertial_optimization_last_frame", lib().orbfe_last_error(h).decode() if h else "")
    out = dict(Rwb=sout[0], twb=sout[1], v=sout[2], bg=sout[3], ba=sout[4], H30=H30, Hprior=Hp, outlier=outl[:n], n_inliers=n_inl.value,
               accepted=acc.value)
    if want_info:
        nr, Ne = info.rounds_run, info.N_e
        out.update(N_e=Ne, rounds_run=nr, recovered=info.recovered, round_iterations=np.array(info.iterations, np.int32)[:nr],
                   round_ok=np.array(info.ok, np.int32)[:nr], round_nbad=np.array(info.n_bad, np.int32)[:nr],
                   round_state=np.array(info.state, np.float64).reshape(4, 42)[:nr],
                   round_prior_chi2=np.array(info.prior_chi2, np.float64)[:nr],
                   round_prior_weight=np.array(info.prior_weight, np.float64)[:nr], round_outlier=rbuf[:nr * Ne].reshape(nr, Ne))
    return out


def pose_inertial_optimization_last_frame_batch_device(extractor, params, batch, d_links_ptr, d_priors_ptr, d_kp_ptr, d_n_ptr, kp_stride,
                                                       d_match_ptr, n_map_points, d_points_ptr, point_stride_frames, d_track_depth_ptr,
                                                       d_state_in_ptr, d_state_out_ptr, d_H30_out_ptr, d_Hprior_out_ptr, d_outlier_ptr,
                                                       d_n_inliers_ptr, d_accepted_ptr, stream=None):
    """orbfe_pose_inertial_optimization_last_frame_batch_device: one block per frame, one orbfe_imu_link_free, one orbfe_pose_imu_prior
    and one state per frame, everything resident in HBM (raw device pointers as ints); asynchronous on `stream`."""
    extractor._chk(extractor.L.orbfe_pose_inertial_optimization_last_frame_batch_device(
        extractor.h, C.byref(params), int(batch), d_links_ptr, d_priors_ptr, d_kp_ptr, d_n_ptr, int(kp_stride), d_match_ptr,
        int(n_map_points), d_points_ptr, int(point_stride_frames), d_track_depth_ptr, d_state_in_ptr, d_state_out_ptr, d_H30_out_ptr,
        d_Hprior_out_ptr, d_outlier_ptr, d_n_inliers_ptr, d_accepted_ptr, stream), "orbfe_pose_inertial_optimization_last_frame_batch_device")


def marginalize_pose_imu(H):
    """orbfe_marginalize_pose_imu: Optimizer::Marginalize(H, 0, 14).block<15,15>(15,15) of a 30 x 30 H on the host (S20), the text of
    the kernel's epilogue -> [15, 15] float64"""
    H = np.ascontiguousarray(H, np.float64).reshape(900)
    Hp = np.zeros((15, 15), np.float64)
    rc = lib().orbfe_marginalize_pose_imu(_p(H), _p(Hp))
    if rc != 0:
        raise OrbfeError(rc, "orbfe_marginalize_pose_imu", "")
    return Hp


def _imu_fail(h, rc, where):
    raise OrbfeError(rc, where, lib().orbfe_last_error(h).decode() if h else "")


def imu_preintegrate_frame(extractor, noise, samples, t_prev, t_cur, frame_bias, kf, want_steps=True):
    """orbfe_imu_preintegrate_frame: Tracking::PreintegrateIMU (src/Tracking.cc:234-290) for a selected sample list, SPEC DECISION S22.
    samples: IMU_SAMPLE_DTYPE records; frame_bias: bwx bwy bwz bax bay baz; kf: the ImuPreint of the last key frame, integrated in
    place -> (frame ImuPreint, steps IMU_STEP_DTYPE records or None, n_steps).  Fewer than 2 samples: nothing changes, n_steps = 0."""
    smp = np.ascontiguousarray(samples, IMU_SAMPLE_DTYPE)
    fb = np.ascontiguousarray(frame_bias, np.float32).reshape(6)
    frame = ImuPreint()
    steps = np.zeros(max(len(smp) - 1, 1), IMU_STEP_DTYPE) if want_steps else None
    n = C.c_int(0)
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_imu_preintegrate_frame(h, C.byref(noise), len(smp), _p(smp), float(t_prev), float(t_cur), _p(fb), C.byref(kf),
                                            C.byref(frame), _p(steps), C.byref(n))
    if rc != 0:
        _imu_fail(h, rc, "orbfe_imu_preintegrate_frame")
    return frame, (steps[:n.value] if want_steps else None), n.value


def imu_reintegrate(extractor, noise, bias, steps):
    """orbfe_imu_reintegrate: Initialize(bias) and IntegrateNewMeasurement over `steps` (IMU_STEP_DTYPE records): Reintegrate(), and
    MergePrevious() with the two lists concatenated -> ImuPreint"""
    st = np.ascontiguousarray(steps, IMU_STEP_DTYPE)
    b = np.ascontiguousarray(bias, np.float32).reshape(6)
    out = ImuPreint()
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_imu_reintegrate(h, C.byref(noise), _p(b), len(st), _p(st) if len(st) else None, C.byref(out))
    if rc != 0:
        _imu_fail(h, rc, "orbfe_imu_reintegrate")
    return out


def imu_predict(extractor, params, state1, kf, frame=None):
    """orbfe_imu_predict: Tracking::PredictStateIMU with Frame::SetImuPoseVelocity and the inertial link.  state1: Rwb1 (9) twb1 v1 bg1
    ba1 -> (state [33] float32 = Rcw tcw Rwb twb v bg ba, link: an ImuLink (IMU_FROM_KEYFRAME) or an ImuLinkFree (IMU_FROM_FRAME),
    info_ok)"""
    s1 = np.ascontiguousarray(state1, np.float32).reshape(21)
    state = np.zeros(33, np.float32)
    link = ImuLinkFree() if params.which == IMU_FROM_FRAME else ImuLink()
    ok = C.c_int(0)
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_imu_predict(h, C.byref(params), _p(s1), C.byref(kf), C.byref(frame) if frame is not None else None, _p(state),
                                 C.addressof(link), C.byref(ok))
    if rc != 0:
        _imu_fail(h, rc, "orbfe_imu_predict")
    return state, link, ok.value


def imu_frame_batch_device(extractor, noise, params, batch, d_samples_ptr, sample_off, d_t_prev_ptr, d_t_cur_ptr, d_frame_bias_ptr,
                           d_state1_ptr, d_kf_ptr, d_frame_ptr, d_steps_out_ptr, d_state_in_ptr, d_links_ptr, d_info_ok_ptr, stream=None):
    """orbfe_imu_frame_batch_device: preintegration, prediction and link of a batch of frames in one launch; sample_off is a HOST array of
    batch + 1 ints, everything else resident in HBM (raw device pointers as ints); asynchronous on `stream`."""
    off = np.ascontiguousarray(sample_off, np.int32)
    assert len(off) == batch + 1
    extractor._chk(extractor.L.orbfe_imu_frame_batch_device(
        extractor.h, C.byref(noise), C.byref(params), int(batch), d_samples_ptr, _p(off), d_t_prev_ptr, d_t_cur_ptr, d_frame_bias_ptr,
        d_state1_ptr, d_kf_ptr, d_frame_ptr, d_steps_out_ptr, d_state_in_ptr, d_links_ptr, d_info_ok_ptr, stream),
        "orbfe_imu_frame_batch_device")


def imu_reintegrate_batch_device(extractor, noise, batch, d_steps_ptr, step_off, d_bias_ptr, d_out_ptr, stream=None):
    """orbfe_imu_reintegrate_batch_device: one record per step list (step_off: HOST array of batch + 1 ints) in one launch."""
    off = np.ascontiguousarray(step_off, np.int32)
    assert len(off) == batch + 1
    extractor._chk(extractor.L.orbfe_imu_reintegrate_batch_device(extractor.h, C.byref(noise), int(batch), d_steps_ptr, _p(off), d_bias_ptr,
                                                                  d_out_ptr, stream), "orbfe_imu_reintegrate_batch_device")


def track_inertial_batch_device(extractor, params, batch, kp_stride, map_points, n_points, io, stream=None):
    """orbfe_track_inertial_batch_device: Tracking::TrackLocalMap with the IMU for `batch` independent frames, resident in HBM (SPEC
    DECISION S23): preintegration + prediction, isInFrustum against the predicted pose, SearchByProjection, the inertial pose
    optimisation chosen by params.predict.which and the statistics of src/Tracking.cc:958-982, launched back to back on `stream`.
    io: a TrackInertialIO of raw device pointers (track_inertial_io() builds it and keeps the HOST offsets alive)."""
    extractor._chk(extractor.L.orbfe_track_inertial_batch_device(extractor.h, C.byref(params), int(batch), int(kp_stride),
                                                                 map_points.h if map_points is not None else None, int(n_points),
                                                                 C.byref(io), stream), "orbfe_track_inertial_batch_device")


def update_local_map_batch_device(extractor, params, batch, vote_stride, covis, n_points, io, stream=None):
    """orbfe_update_local_map_batch_device: Tracking::UpdateLocalMap for `batch` independent frames against the resident graph (SPEC
    DECISION S24); io: a LocalMapIO of raw device pointers.  d_ids_out is what the per-frame chains read as d_ids."""
    extractor._chk(extractor.L.orbfe_update_local_map_batch_device(extractor.h, C.byref(params), int(batch), int(vote_stride),
                                                                   covis.h if covis is not None else None, int(n_points), C.byref(io),
                                                                   stream), "orbfe_update_local_map_batch_device")


def update_local_map(extractor, params, vote_ids, last_kf, covis, n_points):
    """orbfe_update_local_map: one frame from host arrays -> dict(ids, n_local_points, local_kfs, n_local_kfs, vote_ids)"""
    votes = np.ascontiguousarray(vote_ids, np.int32)
    ids, kfs, votes_out = np.empty(int(n_points), np.int32), np.empty(LOCAL_KF_MAX, np.int32), np.empty(len(votes), np.int32)
    n_pts, n_kfs = C.c_int(), C.c_int()
    extractor._chk(extractor.L.orbfe_update_local_map(extractor.h, C.byref(params), len(votes), _p(votes) if len(votes) else None, int(last_kf),
                                                      covis.h, int(n_points), _p(ids), C.byref(n_pts), _p(kfs), C.byref(n_kfs),
                                                      _p(votes_out) if len(votes) else None), "orbfe_update_local_map")
    return dict(ids=ids, n_local_points=n_pts.value, local_kfs=kfs, n_local_kfs=n_kfs.value, vote_ids=votes_out)


def frame_points_batch_device(extractor, map_points, batch, kp_stride, n_points, d_ids_ptr, d_match_ptr, d_outlier_ptr, d_n_ptr, d_out_ptr,
                              stream=None):
    """orbfe_frame_points_batch_device: the frames' mvpMapPoints as Track() leaves them, from what the inertial chain left in HBM"""
    extractor._chk(extractor.L.orbfe_frame_points_batch_device(extractor.h, map_points.h, int(batch), int(kp_stride), int(n_points), d_ids_ptr,
                                                               d_match_ptr, d_outlier_ptr, d_n_ptr, d_out_ptr, stream),
                   "orbfe_frame_points_batch_device")


def track_inertial_io(sample_off, **ptrs):
    """-> (TrackInertialIO, the int32 offsets array that has to stay alive until the call has returned)"""
    off = np.ascontiguousarray(sample_off, np.int32)
    io = TrackInertialIO(sample_off=off.ctypes.data, **ptrs)
    return io, off


def track_frame_inertial(extractor, params, im, samples, t_prev, t_cur, frame_bias, state1, kf, frame, map_points, ids, prior=None,
                         want_hprior=True):
    """orbfe_track_frame_inertial: the chain of track_inertial_batch_device for ONE frame from host memory, image in, results out: one
    upload, extraction, the chain with batch == 1, one download, one synchronisation.  kf / frame: ImuPreint, updated in place.
    -> dict(kp, desc, per_level, steps, state_in, link, info_ok, mps, match, nmatches, state_out, H, Hprior, outlier, n_inliers,
    accepted, found, matches_inliers, tracked, Tcw)"""
    e = extractor
    im = np.asarray(im)
    assert im.dtype == np.uint8 and im.shape == (e.H, e.W) and im.strides[1] == 1
    smp = np.ascontiguousarray(samples, IMU_SAMPLE_DTYPE)
    fb = np.ascontiguousarray(frame_bias, np.float32).reshape(6)
    s1 = np.ascontiguousarray(state1, np.float32).reshape(21)
    ids = np.ascontiguousarray(ids, np.int32)
    M = len(ids)
    from_frame = params.predict.which == IMU_FROM_FRAME
    kp = np.zeros(e.cap, KP_DTYPE)
    desc = np.zeros((e.cap, 32), np.uint8)
    per = np.zeros(e.nlevels, np.int32)
    steps = np.zeros(max(len(smp) - 1, 1), IMU_STEP_DTYPE)
    state_in, state_out = np.zeros(33, np.float32), np.zeros(21, np.float32)
    link = ImuLinkFree() if from_frame else ImuLink()
    mps = np.zeros(max(M, 1), MP_DTYPE)
    match = np.full(e.cap, -1, np.int32)
    H = np.zeros(900 if from_frame else 225, np.float64)
    Hp = np.zeros(225, np.float64) if from_frame and want_hprior else None
    outlier = np.zeros(e.cap, np.uint8)
    found = np.zeros(max(M, 1), np.uint8)
    n = C.c_int()
    res = TrackInertialResult(steps_out=steps.ctypes.data, state_in=state_in.ctypes.data, link_out=C.addressof(link),
                              mp_out=mps.ctypes.data, match_out=match.ctypes.data, state_out=state_out.ctypes.data, H_out=H.ctypes.data,
                              Hprior_out=Hp.ctypes.data if Hp is not None else None, outlier=outlier.ctypes.data, found=found.ctypes.data)
    e._chk(e.L.orbfe_track_frame_inertial(e.h, C.byref(params), _p(im), im.strides[0], len(smp), _p(smp) if len(smp) else None, float(t_prev),
                                          float(t_cur), _p(fb), _p(s1), C.byref(kf), C.byref(frame), map_points.h, M, _p(ids) if M else None,
                                          C.byref(prior) if prior is not None else None, _p(kp), _p(desc), C.byref(n), _p(per), C.byref(res)),
           "orbfe_track_frame_inertial")
    k = n.value
    side = 30 if from_frame else 15
    return dict(kp=kp[:k], desc=desc[:k], per_level=per, steps=steps[:res.n_steps], state_in=state_in, link=link, info_ok=res.info_ok,
                mps=mps[:M], match=match[:k], nmatches=res.n_matches, state_out=state_out, H=H.reshape(side, side),
                Hprior=Hp.reshape(15, 15) if Hp is not None else None, outlier=outlier[:k], n_inliers=res.n_inliers, accepted=res.accepted,
                found=found[:M], matches_inliers=res.matches_inliers, tracked=res.tracked, Tcw=np.array(res.Tcw, np.float32))


def initial_bundle_adjustment(extractor, params, kp1, kp2, matches12, points, Rcw1, tcw1, Rcw2, tcw2, want_info=True):
    """orbfe_initial_bundle_adjustment: the bundle adjustment of the initial map (src/Tracking.cc:698 -> src/Optimizer.cc:60-369), two key
    frames with the first fixed, mono pinhole, SPEC DECISION S17.  kp1 / kp2: KP_DTYPE arrays (mvKeysUn), matches12 [n1] (an index into
    kp2 or negative), points [n1, 3] float32 (vIniP3D), Rcw* [9] / tcw* [3] float32 -> dict(Tcw2 [4, 4], points [n1, 3]) plus, with
    want_info, the fields of orbfe_initial_ba_info as N, iterations, trials, exit, it_cost / it_lambda / it_trials (cut to the
    iterations that ran), pose [12], chi2 [2, N] and depth_positive [2, N]."""
    kp1 = np.ascontiguousarray(kp1, KP_DTYPE)
    kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
    m12 = np.ascontiguousarray(matches12, np.int32)
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    assert len(m12) == len(kp1) and len(pts) == len(kp1)
    Ra, ta = np.ascontiguousarray(Rcw1, np.float32).reshape(9), np.ascontiguousarray(tcw1, np.float32).reshape(3)
    Rb, tb = np.ascontiguousarray(Rcw2, np.float32).reshape(9), np.ascontiguousarray(tcw2, np.float32).reshape(3)
    n1 = len(kp1)
    N = int((m12 >= 0).sum())
    Tcw, out_pts = np.zeros((4, 4), np.float32), np.zeros((max(n1, 1), 3), np.float32)
    info = None
    if want_info:
        info = InitialBAInfo()
        chi2, front = np.zeros((2, max(N, 1)), np.float64), np.zeros((2, max(N, 1)), np.uint8)
        info.chi2, info.depth_positive = chi2.ctypes.data, front.ctypes.data
    h = extractor.h if extractor is not None else None
    rc = lib().orbfe_initial_bundle_adjustment(h, C.byref(params), n1, _p(kp1), len(kp2), _p(kp2), _p(m12), _p(pts), _p(Ra), _p(ta), _p(Rb),
                                               _p(tb), _p(Tcw), _p(out_pts), C.byref(info) if want_info else None)
    if rc != 0:
        raise OrbfeError(rc, "orbfe_initial_bundle_adjustment", lib().orbfe_last_error(h).decode() if h else "")
    out = dict(Tcw2=Tcw, points=out_pts[:n1])
    if want_info:
        ni, N = info.n_iterations, info.N
        out.update(N=N, iterations=ni, trials=info.n_trials, exit=info.exit_kind, it_cost=np.array(info.cost, np.float64)[:ni],
                   it_lambda=np.array(info.lambda_, np.float64)[:ni], it_trials=np.array(info.trials, np.int32)[:ni],
                   pose=np.array(info.pose, np.float64), chi2=chi2.reshape(-1)[:2 * N].reshape(2, N),
                   depth_positive=front.reshape(-1)[:2 * N].reshape(2, N))
    return out


def triangulation_select(raw_match12, raw_bin, hasMP1_now, checkOrientation=True):
    """orbfe_triangulation_select (host-only): one neighbour's (nmatches, vMatches12) from its raw batch results and the
    CURRENT has-map-point flags of key frame 1."""
    raw = np.ascontiguousarray(raw_match12, np.int32)
    rb = np.ascontiguousarray(raw_bin, np.uint8)
    now = np.ascontiguousarray(hasMP1_now, np.uint8)
    out = np.full(max(len(raw), 1), -1, np.int32)
    n = C.c_int()
    rc = lib().orbfe_triangulation_select(len(raw), _p(raw), _p(rb), _p(now), int(checkOrientation), _p(out), C.byref(n))
    if rc != 0:
        raise OrbfeError(rc, "orbfe_triangulation_select")
    return n.value, out[:len(raw)]


def fuse_select(cand_idx, cand_count, cand_cap, kf_desc, mp_desc):
    """orbfe_fuse_select (host only): the strict "<" scan of src/ORBmatcher.cc:824-832 for one pair over a candidate list of
    ORBmatcher.Fuse_search_keyframes, with the descriptor the point has NOW -> (bestIdx, bestDist).  Raises OrbfeError
    (ORBFE_ERR_UNSUPPORTED) when the list is truncated (cand_count > cand_cap)."""
    cand_idx = np.ascontiguousarray(cand_idx, np.int32)
    kf_desc = np.ascontiguousarray(kf_desc, np.uint8)
    mp_desc = np.ascontiguousarray(mp_desc, np.uint8)
    bi, bd = C.c_int(-1), C.c_int(256)
    rc = lib().orbfe_fuse_select(_p(cand_idx), int(cand_count), int(cand_cap), _p(kf_desc), len(kf_desc), _p(mp_desc), C.byref(bi),
                                 C.byref(bd))
    if rc != 0:
        raise OrbfeError(rc, "orbfe_fuse_select")
    return bi.value, bd.value


class FrameTracker:
    """The tracking thread's per-frame chain of this fork once the IMU is initialised -- Frame::Frame -> ExtractORB
    (src/Tracking.cc:152-173, src/Frame.cc:178-189), the isInFrustum loop of Tracking::SearchLocalPoints (:1059-1077) and
    ORBmatcher::SearchByProjection(mCurrentFrame, mvpLocalMapPoints, ...) (:1108-1115) -- as ONE call / one captured
    hipGraph (orbfe_track_frame).  The grid statics are the frame's (src/Frame.cc:101-105)."""

    def __init__(self, extractor, gridCols, gridRows, minX, minY, maxX, maxY):
        self.e, self.L = extractor, extractor.L
        self.grid = (int(gridCols), int(gridRows), float(minX), float(minY),
                     float(np.float32(gridCols) / np.float32(np.float32(maxX) - np.float32(minX))),
                     float(np.float32(gridRows) / np.float32(np.float32(maxY) - np.float32(minY))))

    def TrackFrame(self, im, frustum, points, mpDesc, th, nnRatio, bFarPoints=False, thFarPoints=0.0):
        """-> dict(kp, desc, per_level, mps, proj_xr, match, nmatches); kp is empty when the frame has no keypoints
        (the reference returns early, src/Tracking.cc:158-159)."""
        e = self.e
        im = np.asarray(im)
        assert im.dtype == np.uint8 and im.shape == (e.H, e.W) and im.strides[1] == 1
        points = np.ascontiguousarray(points, WP_DTYPE)
        mpDesc = np.ascontiguousarray(mpDesc, np.uint8)
        M = len(points)
        assert mpDesc.shape == (M, 32) or M == 0
        tp = TrackParams()
        (tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y, tp.grid_inv_w, tp.grid_inv_h) = self.grid
        tp.th, tp.nn_ratio, tp.far_points, tp.th_far_points = th, nnRatio, int(bFarPoints), thFarPoints
        kp = np.zeros(e.cap, KP_DTYPE)
        desc = np.zeros((e.cap, 32), np.uint8)
        per = np.zeros(e.nlevels, np.int32)
        mps = np.zeros(max(M, 1), MP_DTYPE)
        xr = np.zeros(max(M, 1), np.float32)
        match = np.full(e.cap, -1, np.int32)
        n, nm = C.c_int(), C.c_int()
        e._chk(self.L.orbfe_track_frame(e.h, _p(im), im.strides[0], C.byref(frustum), C.byref(tp), M, _p(points), _p(mpDesc),
                                        _p(kp), _p(desc), C.byref(n), _p(per), _p(mps), _p(xr), _p(match), C.byref(nm)),
               "orbfe_track_frame")
        k = n.value
        return dict(kp=kp[:k], desc=desc[:k], per_level=per, mps=mps[:M], proj_xr=xr[:M], match=match[:k], nmatches=nm.value)

    def TrackFrameMap(self, im, frustum, map_points, ids, th, nnRatio, bFarPoints=False, thFarPoints=0.0):
        """orbfe_track_frame_map: the same chain with the local map points named by id out of a resident MapPoints table
        (id >= 0, ~id = skipped for this frame, outside the map = no point); match / mps / proj_xr index the id list."""
        e = self.e
        im = np.asarray(im)
        assert im.dtype == np.uint8 and im.shape == (e.H, e.W) and im.strides[1] == 1
        ids = np.ascontiguousarray(ids, np.int32)
        M = len(ids)
        tp = TrackParams()
        (tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y, tp.grid_inv_w, tp.grid_inv_h) = self.grid
        tp.th, tp.nn_ratio, tp.far_points, tp.th_far_points = th, nnRatio, int(bFarPoints), thFarPoints
        kp = np.zeros(e.cap, KP_DTYPE)
        desc = np.zeros((e.cap, 32), np.uint8)
        per = np.zeros(e.nlevels, np.int32)
        mps = np.zeros(max(M, 1), MP_DTYPE)
        xr = np.zeros(max(M, 1), np.float32)
        match = np.full(e.cap, -1, np.int32)
        n, nm = C.c_int(), C.c_int()
        e._chk(self.L.orbfe_track_frame_map(e.h, _p(im), im.strides[0], C.byref(frustum), C.byref(tp), map_points.h, M, _p(ids), _p(kp),
                                            _p(desc), C.byref(n), _p(per), _p(mps), _p(xr), _p(match), C.byref(nm)), "orbfe_track_frame_map")
        k = n.value
        return dict(kp=kp[:k], desc=desc[:k], per_level=per, mps=mps[:M], proj_xr=xr[:M], match=match[:k], nmatches=nm.value)

    def TrackInitialization(self, im, initial_frame, windowSize=40, nnRatio=0.45, checkOrientation=True):
        """orbfe_track_initialization: ExtractORB -> SearchForInitialization(mInitialFrame, mCurrentFrame, 40, 0.45, true)
        (Tracking::MonocularInitialization, src/Tracking.cc:566-607) as one call against a resident InitialFrame ->
        dict(kp, desc, per_level, matches12, nmatches); matches12[i1] = index in the current frame or -1."""
        e = self.e
        im = np.asarray(im)
        assert im.dtype == np.uint8 and im.shape == (e.H, e.W) and im.strides[1] == 1
        tp = TrackParams()
        (tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y, tp.grid_inv_w, tp.grid_inv_h) = self.grid
        kp = np.zeros(e.cap, KP_DTYPE)
        desc = np.zeros((e.cap, 32), np.uint8)
        per = np.zeros(e.nlevels, np.int32)
        m12 = np.full(max(initial_frame.n, 1), -1, np.int32)
        n, nm = C.c_int(), C.c_int()
        e._chk(self.L.orbfe_track_initialization(e.h, _p(im), im.strides[0], initial_frame.h, C.byref(tp), int(windowSize), nnRatio,
                                                 int(bool(checkOrientation)), _p(kp), _p(desc), C.byref(n), _p(per), _p(m12), C.byref(nm)),
               "orbfe_track_initialization")
        k = n.value
        return dict(kp=kp[:k], desc=desc[:k], per_level=per, matches12=m12[:initial_frame.n], nmatches=nm.value)

    def TrackReferenceKeyFrame(self, im, vocab, levelsup, kf, kfHasMP, nnRatio=0.75, checkOrientation=True):
        """orbfe_track_reference_keyframe: ExtractORB -> the per-feature part of ComputeBoW -> SearchByBoW(reference key frame,
        frame) (Tracking::TrackReferenceKeyFrame, src/Tracking.cc:825-835) as one call against a resident KeyFrame ->
        dict(kp, desc, per_level, word, node, weight, match, nmatches); match[i] = key-frame feature or -1."""
        e = self.e
        im = np.asarray(im)
        assert im.dtype == np.uint8 and im.shape == (e.H, e.W) and im.strides[1] == 1
        has = np.ascontiguousarray(kfHasMP, np.uint8)
        assert len(has) == kf.n
        kp = np.zeros(e.cap, KP_DTYPE)
        desc = np.zeros((e.cap, 32), np.uint8)
        per = np.zeros(e.nlevels, np.int32)
        word = np.zeros(e.cap, np.int32)
        node = np.zeros(e.cap, np.int32)
        weight = np.zeros(e.cap, np.float64)
        match = np.full(e.cap, -1, np.int32)
        n, nm = C.c_int(), C.c_int()
        e._chk(self.L.orbfe_track_reference_keyframe(e.h, _p(im), im.strides[0], vocab.v, int(levelsup), kf.h, _p(has), nnRatio,
                                                     int(checkOrientation), _p(kp), _p(desc), C.byref(n), _p(per), _p(word), _p(node),
                                                     _p(weight), _p(match), C.byref(nm)), "orbfe_track_reference_keyframe")
        k = n.value
        return dict(kp=kp[:k], desc=desc[:k], per_level=per, word=word[:k], node=node[:k], weight=weight[:k], match=match[:k],
                    nmatches=nm.value)


class ImagePreparer:
    """ImageGrabber::ConvertImageToGPU (ros2_ws/src/mono-inertial/include/image_grabber.hpp:96-110): fisheye remap
    (INTER_CUBIC) + resize (INTER_LINEAR) + BGR2GRAY as one kernel; `extract` chains ORBextractor::extractFeatures
    without the grey frame leaving the device."""

    def __init__(self, extractor, map1, map2, dst_w, dst_h):
        self.e = extractor
        self.L = extractor.L
        map1 = np.ascontiguousarray(map1, np.float32)
        map2 = np.ascontiguousarray(map2, np.float32)
        assert map1.ndim == 2 and map1.shape == map2.shape
        self.src_h, self.src_w = map1.shape
        self.dst_w, self.dst_h = int(dst_w), int(dst_h)
        self.p = C.c_void_p()
        extractor._chk(self.L.orbfe_prep_create(extractor.h, self.src_w, self.src_h, _p(map1), _p(map2), self.dst_w,
                                                self.dst_h, C.byref(self.p)), "orbfe_prep_create")

    def close(self):
        if self.p:
            self.L.orbfe_prep_destroy(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bgr(self, bgr):
        assert bgr.dtype == np.uint8 and bgr.ndim == 3 and bgr.shape == (self.src_h, self.src_w, 3) and bgr.strides[2] == 1 \
            and bgr.strides[1] == 3
        return bgr, bgr.strides[0]

    def prepare(self, bgr):
        bgr, pitch = self._bgr(bgr)
        out = np.zeros((self.dst_h, self.dst_w), np.uint8)
        self.e._chk(self.L.orbfe_prepare_image(self.e.h, self.p, bgr.ctypes.data, pitch, _p(out), self.dst_w),
                    "orbfe_prepare_image")
        return out

    def prepare_device(self, d_bgr, pitch, d_gray, gray_pitch, stream=None):
        self.e._chk(self.L.orbfe_prepare_image_device(self.e.h, self.p, d_bgr, pitch, d_gray, gray_pitch, stream),
                    "orbfe_prepare_image_device")

    def extract(self, bgr, want_gray=False):
        """-> (keypoints, descriptors[, grey]) or None when the frame has no keypoints (as extractFeatures)."""
        bgr, pitch = self._bgr(bgr)
        cap = self.e.cap
        kp = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        per = np.zeros(self.e.nlevels, np.int32)
        gray = np.zeros((self.dst_h, self.dst_w), np.uint8) if want_gray else None
        self.e._chk(self.L.orbfe_prepare_and_extract(self.e.h, self.p, bgr.ctypes.data, pitch, _p(kp), _p(desc), C.byref(n),
                                                     _p(per), _p(gray), self.dst_w), "orbfe_prepare_and_extract")
        if n.value == 0:
            return None
        return (kp[:n.value], desc[:n.value], gray) if want_gray else (kp[:n.value], desc[:n.value])


class ORBVocabulary:
    """Device copy of a DBoW2 vocabulary tree + the per-feature descent of Frame::ComputeBoW
    (src/Frame.cc:483-495 -> TemplatedVocabulary::transform)."""

    def __init__(self, extractor, childOff, childIdx, nodeDesc, wordId, weight, L):
        self.e, self.L_ = extractor, extractor.L
        a32 = lambda v: np.ascontiguousarray(v, np.int32)
        self._keep = (a32(childOff), a32(childIdx), np.ascontiguousarray(nodeDesc, np.uint8), a32(wordId),
                      np.ascontiguousarray(weight, np.float64))
        self.v = C.c_void_p()
        co, ci_, nd, wi, we = self._keep
        extractor._chk(self.L_.orbfe_vocab_create(extractor.h, len(wi), _p(co), _p(ci_), _p(nd), _p(wi), _p(we), int(L),
                                                  C.byref(self.v)), "orbfe_vocab_create")

    def close(self):
        if getattr(self, "v", None):
            self.L_.orbfe_vocab_destroy(self.v)
            self.v = None

    __del__ = close

    def transform(self, desc, levelsup):
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        word = np.zeros(max(n, 1), np.int32)
        node = np.zeros(max(n, 1), np.int32)
        weight = np.zeros(max(n, 1), np.float64)
        self.e._chk(self.L_.orbfe_bow_transform(self.e.h, self.v, _p(desc), n, levelsup, _p(word), _p(node), _p(weight)),
                    "orbfe_bow_transform")
        return word[:n], node[:n], weight[:n]

    # weighting / scoring enums of DBoW2 (TemplatedVocabulary.h:35-55)
    TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
    L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5

    def transform_bow(self, desc, levelsup, weighting=0, scoring=0):
        """TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
        (TemplatedVocabulary.h:1136-1204) as Frame::ComputeBoW calls it (src/Frame.cc:483-495, levelsup 4).
        The per-feature tree descent runs on the GPU; the map assembly (<= N inserts) stays on the host in the
        reference's order so the doubles come out bit-identical.  Returns (BowVector, FeatureVector) as dicts
        in ascending key order (std::map iteration order)."""
        word, node, w = self.transform(desc, levelsup)
        bow, fv = {}, {}
        tf = weighting in (self.TF_IDF, self.TF)
        for i in range(len(word)):
            wi = float(w[i])
            if wi > 0:
                k = int(word[i])
                if tf:
                    bow[k] = bow.get(k, 0.0) + wi      # BowVector::addWeight
                elif k not in bow:
                    bow[k] = wi                        # BowVector::addIfNotExist
                fv.setdefault(int(node[i]), []).append(i)  # FeatureVector::addFeature
        bow = dict(sorted(bow.items()))
        fv = dict(sorted(fv.items()))
        must = scoring != self.DOT_PRODUCT
        if tf and bow and not must:
            nd = float(len(bow))
            for k in bow:
                bow[k] /= nd
        if must:                                       # BowVector::normalize (src/DBoW2/BowVector.cpp:62-84)
            norm = 0.0
            if scoring == self.L2_NORM:
                for v in bow.values():
                    norm += v * v
                norm = float(np.sqrt(np.float64(norm)))
            else:
                for v in bow.values():
                    norm += abs(v)
            if norm > 0.0:
                for k in bow:
                    bow[k] /= norm
        return bow, fv


def load_vocabulary_text(path):
    """Parse the ORBvoc.txt format of TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1349-1436)
    into the CSR tree orbfe_vocab_create takes.  Returns a dict with k, L, scoring, weighting, childOff,
    childIdx, nodeDesc, wordId, weight.  Blank lines are skipped (the reference would read a node from
    them with an indeterminate parent)."""
    with open(path) as f:
        k, L, scoring, weighting = (int(t) for t in f.readline().split()[:4])
        if k < 0 or k > 20 or L < 1 or L > 10 or scoring < 0 or scoring > 5 or weighting < 0 or weighting > 3:
            raise ValueError("not a DBoW2 text vocabulary: %s" % path)
        parent, desc, weight, leaf = [0], [np.zeros(32, np.uint8)], [0.0], [0]
        for line in f:
            t = line.split()
            if not t:
                continue
            parent.append(int(t[0]))
            leaf.append(int(t[1]))
            desc.append(np.array([int(v) for v in t[2:34]], np.uint8))
            weight.append(float(t[34]))
    n = len(parent)
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[parent[i]].append(i)
    childOff = np.zeros(n + 1, np.int32)
    childOff[1:] = np.cumsum([len(c) for c in kids])
    childIdx = np.array([c for cs in kids for c in cs], np.int32)
    wordId = np.zeros(n, np.int32)  # Node::word_id defaults to 0 (TemplatedVocabulary.h:275)
    nw = 0
    for i in range(1, n):
        if leaf[i] > 0:
            wordId[i] = nw
            nw += 1
    return dict(k=k, L=L, scoring=scoring, weighting=weighting, childOff=childOff, childIdx=childIdx,
                nodeDesc=np.stack(desc), wordId=wordId, weight=np.array(weight, np.float64))

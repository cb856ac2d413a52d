"""What the host halves of the three pose solvers share (the staging of a host-pointer call and the call scope of the entry points),
at the shapes and on the paths the per-solver suites run seldom.

Staging shapes: for orbfe_pose_optimization, orbfe_pose_inertial_optimization_last_keyframe and
orbfe_pose_inertial_optimization_last_frame, keypoint subsets of one "general" scene with 65 edges -- no keypoint at all (the inertial
calls), 5 keypoints none of them matched, 3 keypoints all matched, and all 65 edges with 5 unmatched keypoints between them (one wave
and one edge) -- each without an info block, with an info block whose outlier pointer is null, and with the rows asked for; the last-frame
call also without Hprior_out.  Every output that is asked for is compared byte for byte with the restatement (*_ref.py), as the
per-solver suites compare; what is not asked for must stay untouched.

Error text: orbfe_last_error after a refusal that carries text (a wrong struct_size) and after one that carries none (a range
error), for a matcher, a solver's host call, a solver's batch call and an S22 call.  The matcher and the S22 call keep the older text
on a refusal without text, the solver calls replace it with the empty string."""
import ctypes as C

import numpy as np
import pytest

import pose_inertial_prev_scenarios as PS20
import pose_inertial_scenarios as PS19
import poseopt_scenarios as PS14
import test_pose_inertial_cpp as T19
import test_pose_inertial_prev_cpp as T20
import test_poseopt_cpp as T14

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
SHAPES = ("n0", "n5_unmatched", "n3_all_matched", "n70_Ne65")
INFO = ("no_info", "info_without_rows", "info_with_rows")
INFO_SCALARS = ("N_e", "rounds_run", "recovered")


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    assert e.mvInvLevelSigma2.tobytes() == (np.float32(1.0) / PS19.level_sigma2()).astype(np.float32).tobytes()
    yield e
    e.close()


def shaped(sc, shape):
    """the scene with a subset of its keypoints, in keypoint order; the points stay"""
    m = sc["mp_index"]
    edges, free = np.flatnonzero(m >= 0), np.flatnonzero(m < 0)
    assert len(edges) == 65
    if shape == "n0":
        keep = edges[:0]
    elif shape == "n5_unmatched":
        keep = free[:5]
    elif shape == "n3_all_matched":
        keep = edges[:3]
    else:
        keep = np.sort(np.concatenate([edges, free[(free > edges[0]) & (free < edges[-1])][:5]]))
        assert len(keep) == 70 and (m[keep] >= 0).sum() == 65
    out = dict(sc)
    out["kp_xy"], out["kp_octave"], out["mp_index"] = sc["kp_xy"][keep], sc["kp_octave"][keep], m[keep]
    return out


_scenes = {}


def scene_and_ref(mod, shape):
    """computed once per module and shape, shared by the info variants"""
    if (mod, shape) not in _scenes:
        sc = shaped(mod.make("general", 65, 0), shape)
        _scenes[(mod, shape)] = (sc, mod.ref(sc))
    return _scenes[(mod, shape)]


def keypoints(sc):
    import orbfe
    kp = np.zeros(len(sc["kp_xy"]), orbfe.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    kp["size"] = 31.0
    return kp


class Call:
    """the arguments every host-pointer pose call takes, and the info block in the three forms"""

    def __init__(self, sc, info_type, info_mode):
        import orbfe
        self.p = orbfe._p
        self.kp, self.mi = keypoints(sc), np.ascontiguousarray(sc["mp_index"], np.int32)
        self.pts = np.ascontiguousarray(sc["points"], np.float32).reshape(-1, 3)
        self.n, self.Ne = len(self.kp), int((self.mi >= 0).sum())
        self.outl = np.full(max(self.n, 1), 0xAB, np.uint8)
        self.n_inl = C.c_int(-3)
        self.info = info_type() if info_mode != "no_info" else None
        self.rows = np.full(4 * max(self.Ne, 1), 0xCD, np.uint8)
        if info_mode == "info_with_rows":
            self.info.outlier = self.rows.ctypes.data
        self.with_rows = info_mode == "info_with_rows"

    def info_ref(self):
        return C.byref(self.info) if self.info is not None else None

    def state(self, sc):
        sin = [np.ascontiguousarray(sc[k], np.float32).reshape(s) for k, s in (("Rcw", 9), ("tcw", 3), ("Rwb", 9), ("twb", 3), ("v", 3),
                                                                                ("bg", 3), ("ba", 3))]
        return sin, [np.zeros(s, np.float32) for s in (9, 3, 3, 3, 3)]

    def finish(self, rc, h, out, info_fields):
        import orbfe
        assert rc == 0, orbfe.lib().orbfe_last_error(h).decode()
        out.update(outlier=self.outl[:self.n], n_inliers=self.n_inl.value)
        assert (self.outl[self.n:] == 0xAB).all(), "flags beyond n written"
        if self.info is not None:
            nr, Ne = self.info.rounds_run, self.info.N_e
            out.update(N_e=Ne, rounds_run=nr)
            for name, field, dt, width in info_fields:
                out[name] = np.array(getattr(self.info, field), dt).reshape(4, width)[:nr].reshape(-1)
            if self.with_rows:
                out["round_outlier"] = self.rows[:nr * Ne].reshape(nr, Ne)
                assert (self.rows[4 * Ne:] == 0xCD).all() and (self.rows[nr * Ne:4 * Ne] == 0).all()
        if not self.with_rows:
            assert (self.rows == 0xCD).all(), "rows written without info->outlier"
        return out


def call_opt(ex, sc, info_mode):
    import orbfe
    c = Call(sc, orbfe.PoseOptInfo, info_mode)
    R, t = (np.ascontiguousarray(sc[k], np.float32).reshape(s) for k, s in (("Rcw", 9), ("tcw", 3)))
    Tcw = np.zeros((4, 4), np.float32)
    rc = orbfe.lib().orbfe_pose_optimization(ex.h, C.byref(orbfe.PoseOptParams(sc["cam"])), c.n, c.p(c.kp), c.p(c.mi), len(c.pts), c.p(c.pts),
                                             c.p(R), c.p(t), c.p(Tcw), c.p(c.outl), C.byref(c.n_inl), c.info_ref())
    return c.finish(rc, ex.h, dict(Tcw=Tcw), (("round_pose", "pose", np.float64, 12), ("round_iterations", "iterations", np.int32, 1),
                                             ("round_trials", "trials", np.int32, 1), ("round_lambda", "lambda_", np.float64, 1),
                                             ("round_chi2", "chi2", np.float64, 1), ("round_nbad", "n_bad", np.int32, 1),
                                             ("round_exit", "exit_kind", np.int32, 1)))


INERTIAL_INFO = (("round_iterations", "iterations", np.int32, 1), ("round_ok", "ok", np.int32, 1), ("round_nbad", "n_bad", np.int32, 1))


def call_imu(ex, sc, info_mode):
    import orbfe
    c = Call(sc, orbfe.PoseInertialInfo, info_mode)
    dep = np.ascontiguousarray(sc["track_depth"], np.float32)
    sin, sout = c.state(sc)
    H = np.zeros((15, 15), np.float64)
    link = orbfe.ImuLink(sc["link"])
    rc = orbfe.lib().orbfe_pose_inertial_optimization_last_keyframe(
        ex.h, C.byref(orbfe.PoseInertialParams(sc["cam"])), C.byref(link), c.n, c.p(c.kp), c.p(c.mi), len(c.pts), c.p(c.pts), c.p(dep),
        *[c.p(a) for a in sin], *[c.p(a) for a in sout], c.p(H), c.p(c.outl), C.byref(c.n_inl), c.info_ref())
    out = c.finish(rc, ex.h, dict(Rwb=sout[0], twb=sout[1], v=sout[2], bg=sout[3], ba=sout[4], H=H),
                   INERTIAL_INFO + (("round_state", "state", np.float64, 21),))
    if c.info is not None:
        out["recovered"] = c.info.recovered
    return out


def call_prev(ex, sc, info_mode, want_prior):
    import orbfe
    c = Call(sc, orbfe.PoseInertialPrevInfo, info_mode)
    dep = np.ascontiguousarray(sc["track_depth"], np.float32)
    sin, sout = c.state(sc)
    H30, Hp = np.zeros((30, 30), np.float64), np.full((15, 15), -7.0, np.float64)
    acc = C.c_int(-3)
    link, prior = orbfe.ImuLinkFree(sc["link"]), orbfe.PoseImuPrior(sc["prior"])
    rc = orbfe.lib().orbfe_pose_inertial_optimization_last_frame(
        ex.h, C.byref(orbfe.PoseInertialPrevParams(sc["cam"])), C.byref(link), C.byref(prior), c.n, c.p(c.kp), c.p(c.mi), len(c.pts),
        c.p(c.pts), c.p(dep), *[c.p(a) for a in sin], *[c.p(a) for a in sout], c.p(H30), c.p(Hp) if want_prior else None, c.p(c.outl),
        C.byref(c.n_inl), C.byref(acc), c.info_ref())
    out = c.finish(rc, ex.h, dict(Rwb=sout[0], twb=sout[1], v=sout[2], bg=sout[3], ba=sout[4], H30=H30, Hprior=Hp, accepted=acc.value),
                   INERTIAL_INFO + (("round_state", "state", np.float64, 42), ("round_prior_chi2", "prior_chi2", np.float64, 1),
                                    ("round_prior_weight", "prior_weight", np.float64, 1)))
    if c.info is not None:
        out["recovered"] = c.info.recovered
    if not want_prior:
        assert (Hp == -7.0).all(), "Hprior written without Hprior_out"
    return out


def same_asked(T, got, want, what, info_mode, skip=()):
    """T.same on what the call was asked for: bytes of every array, equality of every count"""
    if info_mode == "info_with_rows" and not skip:
        return T.same(got, want, what)
    info = info_mode != "no_info"
    for k in T.SCALARS:
        if info or k not in INFO_SCALARS:
            assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    for k, dt in T.FIELDS:
        if k in skip or (k.startswith("round_") and not info) or (k == "round_outlier" and info_mode != "info_with_rows"):
            continue
        g, w = np.ascontiguousarray(got[k], dt).reshape(-1), np.ascontiguousarray(want[k], dt).reshape(-1)
        assert g.shape == w.shape, "%s: %s has another size" % (what, k)
        assert g.tobytes() == w.tobytes(), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("info_mode", INFO)
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_pose_optimization_staging(ex, shape, info_mode):
    sc, want = scene_and_ref(PS14, shape)
    same_asked(T14, call_opt(ex, sc, info_mode), want, "%s, %s" % (shape, info_mode), info_mode)


@pytest.mark.parametrize("info_mode", INFO)
@pytest.mark.parametrize("shape", SHAPES)
def test_pose_inertial_last_keyframe_staging(ex, shape, info_mode):
    sc, want = scene_and_ref(PS19, shape)
    same_asked(T19, call_imu(ex, sc, info_mode), want, "%s, %s" % (shape, info_mode), info_mode)


@pytest.mark.parametrize("want_prior", [True, False], ids=["Hprior", "no_Hprior"])
@pytest.mark.parametrize("info_mode", INFO)
@pytest.mark.parametrize("shape", SHAPES)
def test_pose_inertial_last_frame_staging(ex, shape, info_mode, want_prior):
    sc, want = scene_and_ref(PS20, shape)
    same_asked(T20, call_prev(ex, sc, info_mode, want_prior), want, "%s, %s" % (shape, info_mode), info_mode,
               () if want_prior else ("Hprior",))


TRI_SIZE = "orbfe_tri_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)"
POSE_OPT_SIZE = "orbfe_pose_opt_params / orbfe_pose_opt_info struct_size does not match this library (rebuild the caller against include/orbfe.h)"
IMU_SIZE = ("orbfe_imu_noise / orbfe_imu_preint / orbfe_imu_predict_params struct_size does not match this library (rebuild the caller against "
            "include/orbfe.h)")


def test_last_error_after_refusals_with_and_without_text(ex):
    import orbfe
    L, h = orbfe.lib(), ex.h
    INVALID = 1   # ORBFE_ERR_INVALID_ARG

    def last():
        return L.orbfe_last_error(h).decode()

    # a matcher: the refusal without text comes back in front of the lock and leaves the text alone
    sf = np.ones(8, np.float32)
    nm = C.c_int(0)

    def tri(params, n1):
        return L.orbfe_match_triangulation(h, 0, None, None, None, None, n1, None, None, None, None, 0, None, None, None, None, orbfe._p(sf), 8,
                                           C.byref(params), None, C.byref(nm))
    bad = orbfe.TriParams()
    bad.struct_size += 4
    assert tri(bad, 0) == INVALID and last() == TRI_SIZE
    assert tri(orbfe.TriParams(), -1) == INVALID and last() == TRI_SIZE

    # a solver's host call: every refusal behind the check writes its text, the empty one too
    cam = PS14.make("general", 3, 0)["cam"]
    R, t, Tcw = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32), np.zeros(16, np.float32)
    ni = C.c_int(0)

    def opt(params):
        return L.orbfe_pose_optimization(h, C.byref(params), 0, None, None, 0, None, orbfe._p(R), orbfe._p(t), orbfe._p(Tcw), None, C.byref(ni),
                                         None)
    bad = orbfe.PoseOptParams(cam)
    bad.struct_size += 4
    assert opt(bad) == INVALID and last() == POSE_OPT_SIZE
    assert opt(orbfe.PoseOptParams(cam, rounds=5)) == INVALID and last() == ""

    # a solver's batch call: the same rule, from in front of the lock
    def opt_batch(params):
        return L.orbfe_pose_optimization_batch_device(h, C.byref(params), 1, None, None, 1, None, 0, None, 0, None, None, None, None, None)
    assert opt_batch(bad) == INVALID and last() == POSE_OPT_SIZE
    assert opt_batch(orbfe.PoseOptParams(cam, rounds=5)) == INVALID and last() == ""

    # an S22 call: a refusal without text keeps the older text
    s1, state, link, ok = np.zeros(21, np.float32), np.zeros(33, np.float32), orbfe.ImuLink(), C.c_int(0)
    kf = orbfe.ImuPreint()

    def predict(params):
        return L.orbfe_imu_predict(h, C.byref(params), orbfe._p(s1), C.byref(kf), None, orbfe._p(state), C.addressof(link), C.byref(ok))
    bad = orbfe.ImuPredictParams()
    bad.struct_size += 4
    assert predict(bad) == INVALID and last() == IMU_SIZE
    assert predict(orbfe.ImuPredictParams(which=7)) == INVALID and last() == IMU_SIZE


NO_GRID = "orbfe_fuse_search_keyframe: the key frame has no grid (orbfe_keyframe_set_grid)"


def test_last_error_after_a_refusal_from_inside_the_scope(ex):
    """a refusal that the run itself makes, behind the lock, the device and the scratch hand-over: its text becomes the last error, and a
    call that succeeds afterwards leaves it alone"""
    import orbfe
    import frustum_scenarios as FS
    from test_frustum import PN
    L, h = orbfe.lib(), ex.h
    fr = orbfe.Frustum()
    FS.fill_frustum(fr, PN, W=752.0, H=480.0, n_levels=8, seed=2)
    kf = orbfe.KeyFrame(ex, np.zeros(4, orbfe.KP_DTYPE), np.zeros((4, 32), np.uint8), np.full(4, -1, np.int32), ex.mvScaleFactor)
    mp = orbfe.MapPoints(ex, 4)
    assert L.orbfe_fuse_search_keyframe(h, kf.h, mp.h, 0, None, C.byref(fr), 3.0, None, None) == 1
    assert L.orbfe_last_error(h).decode() == NO_GRID
    sc, want = scene_and_ref(PS14, "n3_all_matched")
    same_asked(T14, call_opt(ex, sc, "info_with_rows"), want, "after the refusal", "info_with_rows")
    assert L.orbfe_last_error(h).decode() == NO_GRID

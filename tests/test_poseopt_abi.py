"""Argument refusals of orbfe_pose_optimization / orbfe_pose_optimization_batch_device.  What the parameter block alone decides --
struct sizes, the unsupported branches, the ranges -- is checked before the handle is looked at, so those refusals need no device
(the first three tests).  The octave check, mp_index against n_points, n > 65536 and the N_e < 3 return read the handle's level count;
the call decides them before it touches the device, but a handle cannot be created without one (orbfe_create, test_abi.py), so those
tests carry the gpu mark."""
import ctypes as C

import numpy as np
import pytest

import poseopt_scenarios as PS

INVALID, UNSUPPORTED = 1, 2


def _args(sc):
    import orbfe
    kp = np.zeros(len(sc["kp_xy"]), orbfe.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    return kp, sc["mp_index"], sc["points"], sc["Rcw"], sc["tcw"]


def _code(fn):
    import orbfe
    with pytest.raises(orbfe.OrbfeError) as ei:
        fn()
    return ei.value.code


def test_params_block_matches_the_header(built):
    import orbfe
    p = orbfe.PoseOptParams()
    assert p.struct_size == C.sizeof(orbfe.PoseOptParams) == 72 and orbfe.PoseOptInfo().struct_size == C.sizeof(orbfe.PoseOptInfo)
    assert (p.camera_model, p.iterations, p.rounds, p.stereo) == (0, 25, 4, 0)
    assert np.float32(p.chi2_threshold) == np.float32(5.991) and p.huber_delta2 == 7.815
    assert (orbfe.POSE_OPT_EXIT_RAN_ALL, orbfe.POSE_OPT_EXIT_TRIALS, orbfe.POSE_OPT_EXIT_RHO_ZERO) == (0, 1, 2)


def test_unsupported_branches_without_a_device(built):
    """KannalaBrandt8 and the stereo edges are refused as UNSUPPORTED before anything else is looked at: no handle, no device"""
    import orbfe
    a = _args(PS.make("general", 10, 0))
    cam = PS.make("general", 10, 0)["cam"]
    assert _code(lambda: orbfe.pose_optimization(None, orbfe.PoseOptParams(cam, camera_model=1), *a)) == UNSUPPORTED
    assert _code(lambda: orbfe.pose_optimization(None, orbfe.PoseOptParams(cam, stereo=1), *a)) == UNSUPPORTED
    L = orbfe.lib()
    for bad in (orbfe.PoseOptParams(cam, camera_model=1), orbfe.PoseOptParams(cam, stereo=1)):
        assert L.orbfe_pose_optimization_batch_device(None, C.byref(bad), 1, None, None, 1, None, 0, None, 0, None, None, None, None, None) == UNSUPPORTED


def test_struct_size_and_ranges_without_a_device(built):
    import orbfe
    sc = PS.make("general", 10, 0)
    a = _args(sc)
    for kw in (dict(iterations=0), dict(iterations=65), dict(rounds=0), dict(rounds=5), dict(huber_delta2=0.0), dict(huber_delta2=float("nan")),
               dict(chi2_threshold=-1.0), dict(camera_model=7)):
        assert _code(lambda: orbfe.pose_optimization(None, orbfe.PoseOptParams(sc["cam"], **kw), *a)) == INVALID, kw
    p = orbfe.PoseOptParams(sc["cam"])
    p.struct_size -= 4
    assert _code(lambda: orbfe.pose_optimization(None, p, *a)) == INVALID
    # a sound block and no handle is INVALID_ARG too; so is a NULL block
    assert _code(lambda: orbfe.pose_optimization(None, orbfe.PoseOptParams(sc["cam"]), *a)) == INVALID
    L = orbfe.lib()
    assert L.orbfe_pose_optimization(None, None, 0, None, None, 0, None, None, None, None, None, None, None) == INVALID
    assert L.orbfe_pose_optimization_batch_device(None, None, 1, None, None, 1, None, 0, None, 0, None, None, None, None, None) == INVALID


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.gpu
def test_refusals_that_need_the_handle(ex):
    import orbfe
    sc = PS.make("general", 10, 0)
    kp, mi, pts, Rcw, tcw = _args(sc)
    p = orbfe.PoseOptParams(sc["cam"])
    bad = mi.copy()
    bad[np.flatnonzero(mi >= 0)[0]] = len(pts)   # mp_index >= n_points
    assert _code(lambda: orbfe.pose_optimization(ex, p, kp, bad, pts, Rcw, tcw)) == INVALID
    for octave in (-1, 8):                       # an octave of a MATCHED keypoint outside the handle's levels
        k2 = kp.copy()
        k2["octave"][np.flatnonzero(mi >= 0)[0]] = octave
        assert _code(lambda: orbfe.pose_optimization(ex, p, k2, mi, pts, Rcw, tcw)) == INVALID
    k3 = kp.copy()
    k3["octave"][np.flatnonzero(mi < 0)[0]] = 99  # ... of an unmatched one is never read
    assert orbfe.pose_optimization(ex, p, k3, mi, pts, Rcw, tcw)["n_inliers"] == orbfe.pose_optimization(ex, p, kp, mi, pts, Rcw, tcw)["n_inliers"]
    big = np.zeros(65537, orbfe.KP_DTYPE)
    assert _code(lambda: orbfe.pose_optimization(ex, p, big, np.full(65537, -1, np.int32), pts, Rcw, tcw)) == INVALID
    info = orbfe.PoseOptInfo()
    info.struct_size += 8
    n_inl, Tcw, outl = C.c_int(), np.zeros(16, np.float32), np.zeros(len(kp), np.uint8)
    rc = ex.L.orbfe_pose_optimization(ex.h, C.byref(p), len(kp), kp.ctypes.data, mi.ctypes.data, len(pts), np.ascontiguousarray(pts).ctypes.data,
                                      Rcw.ctypes.data, tcw.ctypes.data, Tcw.ctypes.data, outl.ctypes.data, C.byref(n_inl), C.byref(info))
    assert rc == INVALID
    assert ex.L.orbfe_pose_optimization_batch_device(ex.h, C.byref(p), 1, 1, 1, 65537, 1, 0, None, 0, 1, 1, 1, 1, None) == INVALID


@pytest.mark.gpu
def test_fewer_than_three_edges_is_ok_and_leaves_the_pose(ex):
    """(:949): ORBFE_OK, 0 inliers, the input pose back, no flags -- and nothing is launched (the info block says 0 rounds)"""
    import orbfe
    for ne in (0, 2):
        sc = PS.make("general", 2, 0)
        kp, mi, pts, Rcw, tcw = _args(sc)
        if ne == 0:
            mi = np.full_like(mi, -1)
        o = orbfe.pose_optimization(ex, orbfe.PoseOptParams(sc["cam"]), kp, mi, pts, Rcw, tcw)
        assert o["n_inliers"] == 0 and o["N_e"] == ne and o["rounds_run"] == 0 and not o["outlier"].any()
        assert o["Tcw"][:3, :3].reshape(-1).tobytes() == Rcw.tobytes() and o["Tcw"][:3, 3].tobytes() == tcw.tobytes()
        assert o["Tcw"][3].tolist() == [0.0, 0.0, 0.0, 1.0]

"""The ABI of orbfe_pose_inertial_optimization_last_keyframe / orbfe_pose_inertial_optimization_batch_device (SPEC DECISION S19): the
symbols, the versioned blocks against the header's figures, and every refusal.  What the blocks alone decide -- struct sizes, the
unsupported branches, the ranges -- is checked before the handle is looked at, so those refusals need no device.  The octave check,
mp_index against n_points and n > 65536 read the handle's level count; the call decides them before it touches the device, but a handle
cannot be created without one, so that test carries the gpu mark."""
import ctypes as C

import numpy as np
import pytest

import pose_inertial_scenarios as PS

INVALID, UNSUPPORTED = 1, 2


def _args(sc):
    import orbfe
    kp = np.zeros(len(sc["kp_xy"]), orbfe.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    return [kp, sc["mp_index"], sc["points"], sc["track_depth"]] + [sc[k] for k in ("Rcw", "tcw", "Rwb", "twb", "v", "bg", "ba")]


def _code(fn):
    import orbfe
    with pytest.raises(orbfe.OrbfeError) as ei:
        fn()
    return ei.value.code


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in ("orbfe_pose_inertial_optimization_last_keyframe", "orbfe_pose_inertial_optimization_batch_device"):
        assert hasattr(L, name) and name in orbfe.SYMBOLS


def test_blocks_match_the_header(built):
    import orbfe
    p = orbfe.PoseInertialParams()
    assert p.struct_size == C.sizeof(orbfe.PoseInertialParams) == 104
    assert orbfe.ImuLink().struct_size == C.sizeof(orbfe.ImuLink) == 8 + 52 * 4 + 99 * 8
    assert orbfe.PoseInertialInfo().struct_size == C.sizeof(orbfe.PoseInertialInfo) == 16 + 48 + 4 * 21 * 8 + 8
    # the reference's constants (src/Optimizer.cc:3498, :3658-3661, :3686, :3701, :3765-3768; IMU::GRAVITY_VALUE)
    assert [np.float32(c) for c in p.chi2] == [np.float32(c) for c in (12, 7.5, 5.991, 5.991)]
    assert (p.camera_model, p.iterations, p.rounds, p.rec_init, p.recover_below, p.stereo) == (0, 15, 4, 0, 30, 0)
    assert p.close_factor == 1.5 and p.close_depth == 10.0 and p.recover_chi2 == 24.0 and p.huber_delta2 == 5.991
    assert np.float32(p.gravity) == np.float32(9.81)
    link = orbfe.ImuLink(PS.make("general", 7, 0)["link"])
    assert link.dt == 0.25 and len(link.info9) == 81 and link.info9[80] > 0 and link.reserved == 0


def test_unsupported_branches_without_a_device(built):
    """KannalaBrandt8 and the stereo edges are refused as UNSUPPORTED before anything else is looked at: no handle, no device"""
    import orbfe
    sc = PS.make("general", 7, 0)
    a = _args(sc)
    call = orbfe.pose_inertial_optimization_last_keyframe
    assert _code(lambda: call(None, orbfe.PoseInertialParams(sc["cam"], camera_model=1), sc["link"], *a)) == UNSUPPORTED
    assert _code(lambda: call(None, orbfe.PoseInertialParams(sc["cam"], stereo=1), sc["link"], *a)) == UNSUPPORTED
    L = orbfe.lib()
    for bad in (orbfe.PoseInertialParams(sc["cam"], camera_model=1), orbfe.PoseInertialParams(sc["cam"], stereo=1)):
        assert L.orbfe_pose_inertial_optimization_batch_device(None, C.byref(bad), 1, *([None] * 3), 1, None, 0, None, 0,
                                                               *([None] * 7)) == UNSUPPORTED


def test_struct_sizes_and_ranges_without_a_device(built):
    import orbfe
    sc = PS.make("general", 7, 0)
    a = _args(sc)
    call = orbfe.pose_inertial_optimization_last_keyframe
    for kw in (dict(iterations=0), dict(iterations=65), dict(rounds=0), dict(rounds=5), dict(huber_delta2=0.0), dict(huber_delta2=float("nan")),
               dict(chi2=(12.0, -1.0, 5.991, 5.991)), dict(chi2=(12.0, 7.5, 5.991, float("nan"))), dict(close_factor=-1.0),
               dict(recover_below=-1), dict(camera_model=7)):
        assert _code(lambda: call(None, orbfe.PoseInertialParams(sc["cam"], **kw), sc["link"], *a)) == INVALID, kw
    p = orbfe.PoseInertialParams(sc["cam"])
    p.struct_size -= 4
    assert _code(lambda: call(None, p, sc["link"], *a)) == INVALID
    link = orbfe.ImuLink(sc["link"])
    link.struct_size += 8
    assert _code(lambda: call(None, orbfe.PoseInertialParams(sc["cam"]), link, *a)) == INVALID
    # a sound block and no handle is INVALID_ARG too; so are a NULL block and a NULL link
    assert _code(lambda: call(None, orbfe.PoseInertialParams(sc["cam"]), sc["link"], *a)) == INVALID
    assert _code(lambda: call(None, orbfe.PoseInertialParams(sc["cam"]), None, *a)) == INVALID
    L = orbfe.lib()
    assert L.orbfe_pose_inertial_optimization_last_keyframe(None, None, None, 0, None, None, 0, *([None] * 16), None, None) == INVALID
    assert L.orbfe_pose_inertial_optimization_batch_device(None, None, 1, *([None] * 3), 1, None, 0, None, 0, *([None] * 7)) == INVALID
    ok = orbfe.PoseInertialParams(sc["cam"])
    assert L.orbfe_pose_inertial_optimization_batch_device(None, C.byref(ok), 1, *([None] * 3), 1, None, 0, None, 0, *([None] * 7)) == INVALID


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.gpu
def test_refusals_that_need_the_handle(ex):
    import orbfe
    sc = PS.make("general", 7, 0)
    a = _args(sc)
    kp, mi, pts = a[0], a[1], a[2]
    p = orbfe.PoseInertialParams(sc["cam"])
    call = orbfe.pose_inertial_optimization_last_keyframe
    bad = mi.copy()
    bad[np.flatnonzero(mi >= 0)[0]] = len(pts)   # mp_index >= n_points
    assert _code(lambda: call(ex, p, sc["link"], kp, bad, *a[2:])) == INVALID
    for octave in (-1, 8):                       # an octave of a MATCHED keypoint outside the handle's levels
        k2 = kp.copy()
        k2["octave"][np.flatnonzero(mi >= 0)[0]] = octave
        assert _code(lambda: call(ex, p, sc["link"], k2, *a[1:])) == INVALID
    k3 = kp.copy()
    k3["octave"][np.flatnonzero(mi < 0)[0]] = 99  # ... of an unmatched one is never read
    assert call(ex, p, sc["link"], k3, *a[1:])["Rwb"].tobytes() == call(ex, p, sc["link"], *a)["Rwb"].tobytes()
    big = np.zeros(65537, orbfe.KP_DTYPE)
    assert _code(lambda: call(ex, p, sc["link"], big, np.full(65537, -1, np.int32), *a[2:])) == INVALID
    info = orbfe.PoseInertialInfo()
    info.struct_size += 8
    link = orbfe.ImuLink(sc["link"])
    bufs = [np.ascontiguousarray(x, np.float32) for x in a[2:]] + [np.zeros(9, np.float32)] + [np.zeros(3, np.float32) for _ in range(4)] + \
        [np.zeros(225), np.zeros(len(kp), np.uint8)]
    n_inl = C.c_int()
    rc = ex.L.orbfe_pose_inertial_optimization_last_keyframe(ex.h, C.byref(p), C.byref(link), len(kp), kp.ctypes.data, mi.ctypes.data, len(pts),
                                                             *[b.ctypes.data for b in bufs], C.byref(n_inl), C.byref(info))
    assert rc == INVALID
    assert ex.L.orbfe_pose_inertial_optimization_batch_device(ex.h, C.byref(p), 1, 1, 1, 1, 65537, 1, 0, None, 0, None, 1, 1, 1, 1, 1,
                                                              None) == INVALID

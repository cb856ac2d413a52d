"""The ABI of orbfe_pose_inertial_optimization_last_frame / orbfe_pose_inertial_optimization_last_frame_batch_device /
orbfe_marginalize_pose_imu (SPEC DECISION S20): the symbols, the versioned blocks against the header's figures, and every refusal.  What
the blocks alone decide -- struct sizes, the unsupported branches, the ranges -- is checked before the handle is looked at, so those
refusals need no device.  The octave check, mp_index against n_points and n > 65536 read the handle's level count; the call decides them
before it touches the device, but a handle cannot be created without one, so that test carries the gpu mark."""
import ctypes as C

import numpy as np
import pytest

import pose_inertial_prev_scenarios as PS

INVALID, UNSUPPORTED = 1, 2
NAMES = ("orbfe_pose_inertial_optimization_last_frame", "orbfe_pose_inertial_optimization_last_frame_batch_device",
         "orbfe_marginalize_pose_imu")


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


def _batch(L, h, p, kp_stride=1):
    """the batch call with NULL / 1 device pointers: it is refused before any of them is read"""
    return L.orbfe_pose_inertial_optimization_last_frame_batch_device(h, p, 1, *([None] * 4), kp_stride, None, 0, None, 0, *([None] * 9))


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in orbfe.SYMBOLS


def test_blocks_match_the_header(built):
    import orbfe
    p = orbfe.PoseInertialPrevParams()
    assert p.struct_size == C.sizeof(orbfe.PoseInertialPrevParams) == 120
    assert orbfe.ImuLinkFree().struct_size == C.sizeof(orbfe.ImuLinkFree) == 8 + 104 * 4 + 99 * 8
    assert orbfe.PoseImuPrior().struct_size == C.sizeof(orbfe.PoseImuPrior) == 8 + 246 * 8
    assert orbfe.PoseInertialPrevInfo().struct_size == C.sizeof(orbfe.PoseInertialPrevInfo) == 16 + 48 + 4 * 42 * 8 + 64 + 8
    # the reference's constants (src/Optimizer.cc:3897, :4070, :4075-4077, :4100, :4107, :4175-4178; Tracking.cc:946; IMU::GRAVITY_VALUE)
    assert [np.float32(c) for c in p.chi2] == [np.float32(5.991)] * 4
    assert (p.camera_model, p.iterations, p.rounds, p.rec_init, p.recover_below, p.stereo, p.inlier_threshold) == (0, 15, 4, 0, 30, 0, 8)
    assert p.close_factor == 1.5 and p.close_depth == 10.0 and p.recover_chi2 == 24.0 and p.huber_delta2 == 5.991
    assert p.prior_huber_delta == 5.0 and np.float32(p.gravity) == np.float32(9.81)
    sc = PS.make("general", 5, 0)
    link = orbfe.ImuLinkFree(sc["link"])
    assert link.dt == 0.25 and len(link.info9) == 81 and link.info9[80] > 0 and link.reserved == 0 and link.reserved2 == 0.0
    assert link.JRg[0] < 0 and link.bg0[0] == link.bg1[0]
    prior = orbfe.PoseImuPrior(sc["prior"])
    assert prior.H[0] > 0 and prior.H[224] > 0 and prior.reserved == 0


def test_unsupported_branches_without_a_device(built):
    """KannalaBrandt8 and the stereo edges are refused as UNSUPPORTED before anything else is looked at: no handle, no device"""
    import orbfe
    sc = PS.make("general", 5, 0)
    a = _args(sc)
    call = orbfe.pose_inertial_optimization_last_frame
    P = orbfe.PoseInertialPrevParams
    assert _code(lambda: call(None, P(sc["cam"], camera_model=1), sc["link"], sc["prior"], *a)) == UNSUPPORTED
    assert _code(lambda: call(None, P(sc["cam"], stereo=1), sc["link"], sc["prior"], *a)) == UNSUPPORTED
    L = orbfe.lib()
    for bad in (P(sc["cam"], camera_model=1), P(sc["cam"], stereo=1)):
        assert _batch(L, None, C.byref(bad)) == UNSUPPORTED


def test_struct_sizes_and_ranges_without_a_device(built):
    import orbfe
    sc = PS.make("general", 5, 0)
    a = _args(sc)
    call = orbfe.pose_inertial_optimization_last_frame
    P = orbfe.PoseInertialPrevParams
    for kw in (dict(iterations=0), dict(iterations=65), dict(rounds=0), dict(rounds=5), dict(huber_delta2=0.0), dict(huber_delta2=float("nan")),
               dict(chi2=(5.991, -1.0, 5.991, 5.991)), dict(chi2=(5.991, 5.991, 5.991, float("nan"))), dict(close_factor=-1.0),
               dict(recover_below=-1), dict(camera_model=7), dict(prior_huber_delta=0.0), dict(prior_huber_delta=float("nan"))):
        assert _code(lambda: call(None, P(sc["cam"], **kw), sc["link"], sc["prior"], *a)) == INVALID, kw
    p = P(sc["cam"])
    p.struct_size -= 4
    assert _code(lambda: call(None, p, sc["link"], sc["prior"], *a)) == INVALID
    link = orbfe.ImuLinkFree(sc["link"])
    link.struct_size += 8
    assert _code(lambda: call(None, P(sc["cam"]), link, sc["prior"], *a)) == INVALID
    prior = orbfe.PoseImuPrior(sc["prior"])
    prior.struct_size -= 8
    assert _code(lambda: call(None, P(sc["cam"]), sc["link"], prior, *a)) == INVALID
    # a sound block and no handle is INVALID_ARG too; so are a NULL block, a NULL link and a NULL prior
    assert _code(lambda: call(None, P(sc["cam"]), sc["link"], sc["prior"], *a)) == INVALID
    assert _code(lambda: call(None, P(sc["cam"]), None, sc["prior"], *a)) == INVALID
    assert _code(lambda: call(None, P(sc["cam"]), sc["link"], None, *a)) == INVALID
    L = orbfe.lib()
    assert L.orbfe_pose_inertial_optimization_last_frame(None, None, None, None, 0, None, None, 0, *([None] * 17), None, None, None) == INVALID
    assert _batch(L, None, None) == INVALID
    assert _batch(L, None, C.byref(P(sc["cam"]))) == INVALID
    H = np.zeros(900)
    assert L.orbfe_marginalize_pose_imu(None, H.ctypes.data) == INVALID and L.orbfe_marginalize_pose_imu(H.ctypes.data, None) == INVALID


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.gpu
def test_refusals_that_need_the_handle(ex):
    import orbfe
    sc = PS.make("general", 5, 0)
    a = _args(sc)
    kp, mi, pts = a[0], a[1], a[2]
    p = orbfe.PoseInertialPrevParams(sc["cam"])
    call = orbfe.pose_inertial_optimization_last_frame
    lp = (sc["link"], sc["prior"])
    bad = mi.copy()
    bad[np.flatnonzero(mi >= 0)[0]] = len(pts)   # mp_index >= n_points
    assert _code(lambda: call(ex, p, *lp, kp, bad, *a[2:])) == INVALID
    for octave in (-1, 8):                       # an octave of a MATCHED keypoint outside the handle's levels
        k2 = kp.copy()
        k2["octave"][np.flatnonzero(mi >= 0)[0]] = octave
        assert _code(lambda: call(ex, p, *lp, k2, *a[1:])) == INVALID
    k3 = kp.copy()
    k3["octave"][np.flatnonzero(mi < 0)[0]] = 99  # ... of an unmatched one is never read
    assert call(ex, p, *lp, k3, *a[1:])["H30"].tobytes() == call(ex, p, *lp, *a)["H30"].tobytes()
    big = np.zeros(65537, orbfe.KP_DTYPE)
    assert _code(lambda: call(ex, p, *lp, big, np.full(65537, -1, np.int32), *a[2:])) == INVALID
    info = orbfe.PoseInertialPrevInfo()
    info.struct_size += 8
    link, prior = orbfe.ImuLinkFree(sc["link"]), orbfe.PoseImuPrior(sc["prior"])
    bufs = [np.ascontiguousarray(x, np.float32) for x in a[2:]] + [np.zeros(9, np.float32)] + [np.zeros(3, np.float32) for _ in range(4)] + \
        [np.zeros(900), np.zeros(225), np.zeros(len(kp), np.uint8)]
    n_inl, acc = C.c_int(), C.c_int()
    rc = ex.L.orbfe_pose_inertial_optimization_last_frame(ex.h, C.byref(p), C.byref(link), C.byref(prior), len(kp), kp.ctypes.data,
                                                          mi.ctypes.data, len(pts), *[b.ctypes.data for b in bufs], C.byref(n_inl),
                                                          C.byref(acc), C.byref(info))
    assert rc == INVALID
    assert ex.L.orbfe_pose_inertial_optimization_last_frame_batch_device(ex.h, C.byref(p), 1, 1, 1, 1, 1, 65537, 1, 0, None, 0, None, 1, 1, 1,
                                                                         1, 1, 1, 1, None) == INVALID

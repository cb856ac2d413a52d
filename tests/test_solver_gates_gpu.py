"""The solver calls on the GPU on the scenes of tests/solver_gates.py, which sit exactly on the solvers' gates: a call parameter equals,
bit for bit, the value a gate compares with it, or two hypotheses tie.  tests/test_solver_gates.py proves on the CPU that every
one-token mistake in a gate changes the restatement's result on one of these scenes; here every scene goes through its host-pointer
call, and the three pose solvers also through their *_batch_device call (a 256-thread block at every N_e).  Every output and every
info field is compared with the restatement byte for byte, with the helpers of the solvers' own GPU tests: no tolerance, no skipped
element; the scene with Xc == (0, 0, 0) compares its non-finite values by position and kind, as the zero_depth scenes do."""
import numpy as np
import pytest

import solver_gates as SG
import test_mlpnp_gpu as TM
import test_pose_inertial_gpu as T19
import test_pose_inertial_prev_gpu as T20
import test_poseopt_gpu as T14
import test_twoview_gpu as T12
from test_pose_inertial_cpp import link_bytes as link_bytes19
from test_pose_inertial_prev_cpp import link_bytes as link_bytes20
from test_pose_inertial_prev_cpp import prior_bytes

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    assert e.mvLevelSigma2.tobytes() == SG.PS.level_sigma2().tobytes()   # the scenes' table is the handle's
    assert e.mvInvLevelSigma2.tobytes() == (np.float32(1.0) / SG.PS.level_sigma2()).astype(np.float32).tobytes()
    yield e
    e.close()


def nonfinite(s):
    return any(gate == "depth_zero" for _, _, gate in s["ties"])


# ---- the host-pointer calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SG.names("poseopt"))
def test_pose_optimization(ex, name):
    s = SG.build("poseopt", name)
    T14.same(T14.call(ex, s["sc"], **s["kw"]), s["want"], name)


@pytest.mark.parametrize("name", SG.names("inertial"))
def test_pose_inertial_last_keyframe(ex, name):
    s = SG.build("inertial", name)
    T19.same(T19.call(ex, s["sc"], **s["kw"]), s["want"], name, nonfinite(s))


@pytest.mark.parametrize("name", SG.names("inertial_prev"))
def test_pose_inertial_last_frame(ex, name):
    s = SG.build("inertial_prev", name)
    T20.same(T20.call(ex, s["sc"], **s["kw"]), s["want"], name, nonfinite(s))


@pytest.mark.parametrize("name", SG.names("twoview"))
def test_two_view_reconstruct(ex, name):
    s = SG.build("twoview", name)
    T12.same(T12.call(ex, s["sc"]), s["want"], name)


@pytest.mark.parametrize("name", SG.names("mlpnp"))
def test_mlpnp_ransac(ex, name):
    s = SG.build("mlpnp", name)
    sc = dict(s["sc"], ransac=dict(s["sc"]["ransac"], **s["kw"]))
    TM.same(TM.call(ex, sc), s["want"], name)


# ---- the batch calls: one launch of mixed frames, the tied frame among them --------------------------------------------------
def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _pack(orbfe, scs, keypoints, with_depth):
    """the frames of a batch with per-frame point sets, as the solvers' own batch tests lay them out"""
    B = len(scs)
    stride = max(len(sc["kp_xy"]) for sc in scs) + 7
    M = max(len(sc["points"]) for sc in scs)
    kp = np.zeros((B, stride), orbfe.KP_DTYPE)
    match = np.full((B, stride), -1, np.int32)
    pts = np.zeros((B, M), orbfe.WP_DTYPE)
    depth = np.zeros((B, M), np.float32)
    n = np.zeros(B, np.int32)
    for b, sc in enumerate(scs):
        k = keypoints(sc)
        n[b] = len(k)
        kp[b, :len(k)] = k
        kp[b, len(k):]["octave"] = 99   # beyond d_n: never read
        for i, f in enumerate("xyz"):
            pts[b, :len(sc["points"])][f] = sc["points"][:, i]
        if with_depth:
            depth[b, :len(sc["points"])] = sc["track_depth"]
        match[b, :len(k)] = sc["mp_index"]
        match[b, len(k):] = 5           # beyond d_n: never read
    return B, stride, M, kp, match, pts, depth, n


def _check_flags(outl, ninl, n, wants, what):
    for b, want in enumerate(wants):
        assert outl[b, :n[b]].tobytes() == want["outlier"].tobytes(), "%s frame %d: flags" % (what, b)
        assert (outl[b, n[b]:] == 0xAB).all(), "%s frame %d: bytes beyond d_n written" % (what, b)
        assert int(ninl[b]) == want["n_inliers"], "%s frame %d: count" % (what, b)


def _pose_bytes(want):
    T = want["Tcw"]
    return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).tobytes()


POSEOPT_OTHERS = (("general", 2, 0), ("far", 65, 0))   # the frames that share the launch: N_e = 2 (nothing runs) and another size


@pytest.mark.parametrize("name", SG.names("poseopt"))
def test_pose_optimization_batch(ex, name):
    """the tied frame between two others in one launch, all under the scene's threshold: every frame against the restatement"""
    import torch
    import orbfe
    s = SG.build("poseopt", name)
    others = [SG.PS.make_case(c) for c in POSEOPT_OTHERS]
    scs = [others[0], s["sc"], others[1]]
    wants = [SG.PS.ref(others[0], **s["kw"]), s["want"], SG.PS.ref(others[1], **s["kw"])]
    B, stride, M, kp, match, pts, _, n = _pack(orbfe, scs, T14.keypoints, False)
    pose = np.stack([np.concatenate([sc["Rcw"], sc["tcw"]]) for sc in scs]).astype(np.float32)
    d_kp, d_match, d_pts, d_pose, d_n = (_dev(torch, a) for a in (kp, match, pts, pose, n))
    d_out = torch.full((B * 12,), -7.0, dtype=torch.float32, device="cuda")
    d_outl = torch.full((B * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ninl = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    orbfe.pose_optimization_batch_device(ex, orbfe.PoseOptParams(s["sc"]["cam"], **s["kw"]), B, d_kp.data_ptr(), d_n.data_ptr(), stride,
                                         d_match.data_ptr(), M, d_pts.data_ptr(), M, d_pose.data_ptr(), d_out.data_ptr(), d_outl.data_ptr(),
                                         d_ninl.data_ptr(), st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy().reshape(B, 12)
    for b, want in enumerate(wants):
        assert _pose_bytes(want) == out[b].tobytes(), "%s frame %d: pose" % (name, b)
    _check_flags(d_outl.cpu().numpy().reshape(B, stride), d_ninl.cpu().numpy(), n, wants, name)


def _state_same(out, want, what, by_kind):
    w = np.concatenate([want[k] for k in ("Rwb", "twb", "v", "bg", "ba")])
    _same_floats(out, w, what + ": state", by_kind)


def _same_floats(g, w, what, by_kind):
    g, w = np.ascontiguousarray(g).reshape(-1), np.ascontiguousarray(w).reshape(-1)
    assert g.shape == w.shape and g.dtype == w.dtype, what
    if by_kind:   # non-finite values by position and kind (NaN payloads differ between hosts and the GPU), everything finite by bytes
        fin = np.isfinite(w)
        assert np.array_equal(np.isfinite(g), fin) and np.array_equal(np.isnan(g), np.isnan(w)), what + " non-finite pattern"
        assert np.array_equal(np.sign(g[np.isinf(g)]), np.sign(w[np.isinf(w)])), what + " sign of infinity"
        g, w = g[fin], w[fin]
    assert g.tobytes() == w.tobytes(), what


IMU_OTHERS = (("few", 0, 0), ("general", 65, 0))   # the frames that share the launch: no match at all, and another size


@pytest.mark.parametrize("name", SG.names("inertial"))
def test_pose_inertial_last_keyframe_batch(ex, name):
    import torch
    import orbfe
    s = SG.build("inertial", name)
    others = [SG.S19.make_case(c) for c in IMU_OTHERS]
    scs = [others[0], s["sc"], others[1]]
    wants = [SG.S19.ref(others[0], **s["kw"]), s["want"], SG.S19.ref(others[1], **s["kw"])]
    B, stride, M, kp, match, pts, depth, n = _pack(orbfe, scs, T19.keypoints, True)
    state = np.stack([T19.state_in(sc) for sc in scs])
    links = b"".join(np.array([len(link_bytes19(sc["link"])) + 8, 0], np.int32).tobytes() + link_bytes19(sc["link"]) for sc in scs)
    d_kp, d_match, d_pts, d_depth, d_state, d_n = (_dev(torch, a) for a in (kp, match, pts, depth, state, n))
    d_links = _dev(torch, np.frombuffer(links, np.uint8))
    d_out = torch.full((B * 21,), -7.0, dtype=torch.float32, device="cuda")
    d_H = torch.full((B * 225,), -7.0, dtype=torch.float64, device="cuda")
    d_outl = torch.full((B * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ninl = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    orbfe.pose_inertial_optimization_batch_device(ex, orbfe.PoseInertialParams(s["sc"]["cam"], **s["kw"]), B, d_links.data_ptr(),
                                                  d_kp.data_ptr(), d_n.data_ptr(), stride, d_match.data_ptr(), M, d_pts.data_ptr(), M,
                                                  d_depth.data_ptr(), d_state.data_ptr(), d_out.data_ptr(), d_H.data_ptr(),
                                                  d_outl.data_ptr(), d_ninl.data_ptr(), st.cuda_stream)
    st.synchronize()
    out, Hs = d_out.cpu().numpy().reshape(B, 21), d_H.cpu().numpy().reshape(B, 15, 15)
    for b, want in enumerate(wants):
        by_kind = b == 1 and nonfinite(s)
        _state_same(out[b], want, "%s frame %d" % (name, b), by_kind)
        _same_floats(Hs[b], want["H"], "%s frame %d: Hessian" % (name, b), by_kind)
    _check_flags(d_outl.cpu().numpy().reshape(B, stride), d_ninl.cpu().numpy(), n, wants, name)


IMU_PREV_OTHERS = (("few", 0, 0), ("prior_far", 65, 0))


@pytest.mark.parametrize("name", SG.names("inertial_prev"))
def test_pose_inertial_last_frame_batch(ex, name):
    import torch
    import orbfe
    s = SG.build("inertial_prev", name)
    others = [SG.S20.make_case(c) for c in IMU_PREV_OTHERS]
    scs = [others[0], s["sc"], others[1]]
    wants = [SG.S20.ref(others[0], **s["kw"]), s["want"], SG.S20.ref(others[1], **s["kw"])]
    B, stride, M, kp, match, pts, depth, n = _pack(orbfe, scs, T20.keypoints, True)
    state = np.stack([T20.state_in(sc) for sc in scs])
    links = b"".join(np.array([len(link_bytes20(sc["link"])) + 8, 0], np.int32).tobytes() + link_bytes20(sc["link"]) for sc in scs)
    priors = b"".join(np.array([len(prior_bytes(sc["prior"])) + 8, 0], np.int32).tobytes() + prior_bytes(sc["prior"]) for sc in scs)
    d_kp, d_match, d_pts, d_depth, d_state, d_n = (_dev(torch, a) for a in (kp, match, pts, depth, state, n))
    d_links, d_priors = _dev(torch, np.frombuffer(links, np.uint8)), _dev(torch, np.frombuffer(priors, np.uint8))
    d_out = torch.full((B * 21,), -7.0, dtype=torch.float32, device="cuda")
    d_H = torch.full((B * 900,), -7.0, dtype=torch.float64, device="cuda")
    d_Hp = torch.full((B * 225,), -7.0, dtype=torch.float64, device="cuda")
    d_outl = torch.full((B * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ninl = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    d_acc = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    orbfe.pose_inertial_optimization_last_frame_batch_device(
        ex, orbfe.PoseInertialPrevParams(s["sc"]["cam"], **s["kw"]), B, d_links.data_ptr(), d_priors.data_ptr(), d_kp.data_ptr(),
        d_n.data_ptr(), stride, d_match.data_ptr(), M, d_pts.data_ptr(), M, d_depth.data_ptr(), d_state.data_ptr(), d_out.data_ptr(),
        d_H.data_ptr(), d_Hp.data_ptr(), d_outl.data_ptr(), d_ninl.data_ptr(), d_acc.data_ptr(), st.cuda_stream)
    st.synchronize()
    out, Hs, Hps = d_out.cpu().numpy().reshape(B, 21), d_H.cpu().numpy().reshape(B, 30, 30), d_Hp.cpu().numpy().reshape(B, 15, 15)
    acc = d_acc.cpu().numpy()
    for b, want in enumerate(wants):
        by_kind = b == 1 and nonfinite(s)
        _state_same(out[b], want, "%s frame %d" % (name, b), by_kind)
        _same_floats(Hs[b], want["H30"], "%s frame %d: Hessian" % (name, b), by_kind)
        _same_floats(Hps[b], want["Hprior"], "%s frame %d: marginalised Hessian" % (name, b), by_kind)
        assert int(acc[b]) == want["accepted"], "%s frame %d: accepted" % (name, b)
    _check_flags(d_outl.cpu().numpy().reshape(B, stride), d_ninl.cpu().numpy(), n, wants, name)

"""orbfe_pose_optimization / orbfe_pose_optimization_batch_device on the GPU against the restatement of SPEC DECISION S14
(poseopt_ref.pose_optimization, written from src/Optimizer.cc:765-1067) on the scenes of poseopt_scenarios (test_poseopt.py checks
which exits and branches they reach).  Every comparison is exact: the bytes of the pose, the flags, the count and every field of
orbfe_pose_opt_info.  No tolerance, no skipped element; the zero_depth scenes compare their non-finite values by position and kind
(NaN payloads differ between hosts and the GPU) and everything finite by bytes."""
import numpy as np
import pytest

import poseopt_scenarios as PS
from test_poseopt_cpp import same

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)


def keypoints(sc):
    import orbfe
    kp = np.zeros(len(sc["kp_xy"]), orbfe.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    kp["size"] = 31.0
    return kp


def call(ex, sc, want_info=True, **kw):
    import orbfe
    return orbfe.pose_optimization(ex, orbfe.PoseOptParams(sc["cam"], **kw), keypoints(sc), sc["mp_index"], sc["points"], sc["Rcw"], sc["tcw"],
                                   want_info)


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    assert e.mvLevelSigma2.tobytes() == PS.level_sigma2().tobytes()  # the scenes' table is the handle's
    assert e.mvInvLevelSigma2.tobytes() == (np.float32(1.0) / PS.level_sigma2()).astype(np.float32).tobytes()
    yield e
    e.close()


@pytest.mark.parametrize("case", PS.CASES, ids=PS.case_id)
def test_equals_restatement(ex, case):
    sc, want = PS.make_case(case), PS.ref_cached(case)
    same(call(ex, sc), want, PS.case_id(case), case[0] == "zero_depth")


def test_fewer_iterations_and_rounds(ex):
    """the parameters are the call's, not constants of the kernel"""
    case = ("far", 300, 0)
    sc = PS.make_case(case)
    want = PS.ref(sc, iterations=3, rounds=2, chi2_threshold=3.0, huber_delta2=4.0)
    assert want["rounds_run"] == 2 and (want["round_exit"] == 0).any()
    same(call(ex, sc, iterations=3, rounds=2, chi2_threshold=3.0, huber_delta2=4.0), want, "far, 3 iterations, 2 rounds")


def test_two_calls_give_equal_bytes(ex):
    sc = PS.make_case(("outliers", 1000, 1))
    a, b = call(ex, sc), call(ex, sc)
    same(a, b, "second call")
    c = call(ex, sc, want_info=False)
    assert c["Tcw"].tobytes() == a["Tcw"].tobytes() and c["outlier"].tobytes() == a["outlier"].tobytes() and c["n_inliers"] == a["n_inliers"]


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


BATCH = (("general", 300, 0), ("general", 2, 0), ("outliers", 1000, 1), None, ("far", 65, 0))   # None: a frame without matches


@pytest.mark.parametrize("shared", [False, True], ids=["per_frame_points", "shared_points"])
def test_batch_equals_single_calls(ex, shared):
    """5 frames of different N_e in one launch (one with N_e = 0, one with N_e = 2) against five host calls"""
    import torch
    import orbfe
    scs = []
    for c in BATCH:
        sc = dict(PS.make_case(c if c else ("general", 64, 0)))
        if c is None:
            sc["mp_index"] = np.full_like(sc["mp_index"], -1)
        scs.append(sc)
    B = len(scs)
    stride = max(len(sc["kp_xy"]) for sc in scs) + 7
    M = max(len(sc["points"]) for sc in scs)
    if shared:   # one point set for all frames: each frame's indices are shifted into it
        off = np.cumsum([0] + [len(sc["points"]) for sc in scs])
        M = int(off[-1])
    kp = np.zeros((B, stride), orbfe.KP_DTYPE)
    match = np.full((B, stride), -1, np.int32)
    pts = np.zeros((1 if shared else B, M), orbfe.WP_DTYPE)
    pose = np.zeros((B, 12), np.float32)
    n = np.zeros(B, np.int32)
    singles = []
    for b, sc in enumerate(scs):
        k = keypoints(sc)
        n[b] = len(k)
        kp[b, :len(k)] = k
        kp[b, len(k):]["octave"] = 99   # beyond d_n: never read
        mi = sc["mp_index"].copy()
        row, base = (0, int(off[b])) if shared else (b, 0)
        pts[row, base:base + len(sc["points"])]["x"] = sc["points"][:, 0]
        pts[row, base:base + len(sc["points"])]["y"] = sc["points"][:, 1]
        pts[row, base:base + len(sc["points"])]["z"] = sc["points"][:, 2]
        match[b, :len(k)] = np.where(mi >= 0, mi + base, -1)
        match[b, len(k):] = 5       # beyond d_n: never read
        pose[b, :9], pose[b, 9:] = sc["Rcw"], sc["tcw"]
        singles.append(call(ex, sc, want_info=False))
    d_kp, d_match, d_pts, d_pose, d_n = (_dev(torch, a) for a in (kp, match, pts, pose, n))
    d_out = torch.full((B * 12,), -7.0, dtype=torch.float32, device="cuda")
    d_outl = torch.full((B * stride,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ninl = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    orbfe.pose_optimization_batch_device(ex, orbfe.PoseOptParams(scs[0]["cam"]), B, d_kp.data_ptr(), d_n.data_ptr(), stride, d_match.data_ptr(),
                                         M, d_pts.data_ptr(), 0 if shared else M, d_pose.data_ptr(), d_out.data_ptr(), d_outl.data_ptr(),
                                         d_ninl.data_ptr(), st.cuda_stream)
    st.synchronize()
    out, outl, ninl = d_out.cpu().numpy().reshape(B, 12), d_outl.cpu().numpy().reshape(B, stride), d_ninl.cpu().numpy()
    for b, (sc, one) in enumerate(zip(scs, singles)):
        T = one["Tcw"]
        assert np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).tobytes() == out[b].tobytes(), "frame %d: pose" % b
        assert outl[b, :n[b]].tobytes() == one["outlier"].tobytes(), "frame %d: flags" % b
        assert (outl[b, n[b]:] == 0xAB).all(), "frame %d: bytes beyond d_n written" % b
        assert int(ninl[b]) == one["n_inliers"], "frame %d: count" % b
    assert singles[1]["n_inliers"] == 0 and singles[3]["n_inliers"] == 0 and singles[0]["n_inliers"] > 200


def test_fed_from_extract_and_match_on_device(built):
    """orbfe_extract_batch_device -> orbfe_project_map_points_device -> orbfe_match_projection_batch_device ->
    orbfe_pose_optimization_batch_device on two synthetic frames, nothing downloaded in between; the result must equal the host call
    on the downloaded keypoints and matches"""
    import torch
    import orbfe
    import frustum_scenarios as FS
    from orbfe import synth
    from test_frustum import PN
    W, H, B, M = 640, 480, 2, 900
    args = (1000, 20000, 1.2, 8, 20, 7, W, H)
    e = orbfe.ORBextractor(*args, device=0, max_batch=B)
    m = orbfe.ORBmatcher(e)
    cap = e.cap
    frames = np.stack([synth.frame(W, H, 21), synth.frame(W, H, 22)])
    got = e.extract_batch(list(frames))
    d_gray = torch.from_numpy(frames.reshape(B, -1)).cuda()
    d_kp = torch.zeros(B * cap * 24, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_mps = torch.zeros(B * M * orbfe.MP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_match = torch.full((B * cap,), -9, dtype=torch.int32, device="cuda")
    d_nm = torch.zeros(B, dtype=torch.int32, device="cuda")
    Fp = orbfe.Frustum()
    v = FS.fill_frustum(Fp, PN, W=float(W), H=float(H), seed=5, cx=W / 2.0, cy=H / 2.0)
    cam = (v["fx"], v["fy"], v["cx"], v["cy"], 0, 0, 0, 0)
    pts, mpd = [], []
    for b in range(B):   # map points that re-project onto the frame's keypoints under the frustum's pose
        p, d = FS.world_points_on_keypoints(got[b][0], got[b][1], v, M, np.random.default_rng(30 + b), 8, orbfe.WP_DTYPE)
        p["bad"], p["skip"] = 0, 0
        pts.append(p)
        mpd.append(d)
    d_pts, d_mpd = _dev(torch, np.stack(pts)), _dev(torch, np.stack(mpd))
    # the initial pose: the frustum's, moved by a centimetre
    pose = np.tile(np.concatenate([np.asarray(v["rcw"], np.float32), np.asarray(v["tcw"], np.float32) + np.float32(0.01)]), (B, 1))
    d_pose = _dev(torch, pose.astype(np.float32))
    d_out = torch.zeros(B * 12, dtype=torch.float32, device="cuda")
    d_outl = torch.zeros(B * cap, dtype=torch.uint8, device="cuda")
    d_ninl = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = st.cuda_stream
    e.extract_batch_device(d_gray.data_ptr(), W * H, W, B, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), None, s)
    wp = orbfe.WP_DTYPE.itemsize
    for b in range(B):
        m.isInFrustum_batch_device(Fp, M, d_pts.data_ptr() + b * M * wp, d_mps.data_ptr() + b * M * orbfe.MP_DTYPE.itemsize, None, s)
    m.SearchByProjection_batch_device(B, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, 64, 48, 0.0, 0.0, float(W), float(H), M,
                                      d_mps.data_ptr(), d_mpd.data_ptr(), None, 3.0, 0.8, d_match.data_ptr(), d_nm.data_ptr(), stream=s)
    prm = orbfe.PoseOptParams(cam)
    orbfe.pose_optimization_batch_device(e, prm, B, d_kp.data_ptr(), d_n.data_ptr(), cap, d_match.data_ptr(), M, d_pts.data_ptr(), M,
                                         d_pose.data_ptr(), d_out.data_ptr(), d_outl.data_ptr(), d_ninl.data_ptr(), s)
    st.synchronize()
    assert e.device_status() == 0
    n = d_n.cpu().numpy()
    kp = d_kp.cpu().numpy().view(orbfe.KP_DTYPE).reshape(B, cap)
    match = d_match.cpu().numpy().reshape(B, cap)
    out, outl, ninl = d_out.cpu().numpy().reshape(B, 12), d_outl.cpu().numpy().reshape(B, cap), d_ninl.cpu().numpy()
    for b in range(B):
        assert n[b] == len(got[b][0]) and (match[b, :n[b]] >= 0).sum() > 100, "frame %d: too few matches for the test to mean anything" % b
        xyz = np.stack([pts[b]["x"], pts[b]["y"], pts[b]["z"]], 1)
        one = orbfe.pose_optimization(e, prm, kp[b, :n[b]], match[b, :n[b]], xyz, pose[b, :9], pose[b, 9:], False)
        T = one["Tcw"]
        assert np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).tobytes() == out[b].tobytes(), "frame %d: pose" % b
        assert outl[b, :n[b]].tobytes() == one["outlier"].tobytes() and int(ninl[b]) == one["n_inliers"], "frame %d" % b
        assert one["n_inliers"] > 50
    e.close()

"""orbfe_pose_inertial_optimization_last_frame / orbfe_pose_inertial_optimization_last_frame_batch_device on the GPU against the
restatement of SPEC DECISION S20 (pose_inertial_prev_ref.pose_inertial_optimization_last_frame, written from src/Optimizer.cc:3846-4275,
:2882-2962, src/G2oTypes.cc and src/ImuTypes.cc) on the scenes of pose_inertial_prev_scenarios (test_pose_inertial_prev.py checks which
branches they reach).  Every comparison is exact: the bytes of the state, both Hessians, the flags, the count, `accepted` and every
field of orbfe_pose_inertial_prev_info.  No tolerance, no skipped element; the zero_depth scenes compare non-finite values by position
and kind and everything finite by bytes.  The sizes are those at which the tree shape (1, 63 / 64 / 65, 257), the wave-walked run
(1000, 4097), the N_e + 4 < 10 break (5 / 6) and the solve without any mono edge (0) can go wrong."""
import numpy as np
import pytest

import pose_inertial_prev_scenarios as PS
from test_pose_inertial_prev_cpp import link_bytes, prior_bytes, same, state_in

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)


def keypoints(sc):
    import orbfe
    kp = np.zeros(len(sc["kp_xy"]), orbfe.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    kp["size"] = 31.0
    return kp


def call(ex, sc, want_info=True, want_prior=True, **kw):
    import orbfe
    return orbfe.pose_inertial_optimization_last_frame(ex, orbfe.PoseInertialPrevParams(sc["cam"], **kw), sc["link"], sc["prior"],
                                                       keypoints(sc), sc["mp_index"], sc["points"], sc["track_depth"], sc["Rcw"], sc["tcw"],
                                                       sc["Rwb"], sc["twb"], sc["v"], sc["bg"], sc["ba"], want_info, want_prior)


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    assert e.mvInvLevelSigma2.tobytes() == (np.float32(1.0) / PS.PS19.level_sigma2()).astype(np.float32).tobytes()
    yield e
    e.close()


@pytest.mark.parametrize("case", PS.CASES, ids=PS.case_id)
def test_equals_restatement(ex, case):
    sc, want = PS.make_case(case), PS.ref_cached(case)
    same(call(ex, sc, **PS.case_kw(case)), want, PS.case_id(case), case[0] == "zero_depth")


def test_changed_parameters_are_honoured(ex):
    """the parameters are the call's, not constants of the kernel"""
    sc = PS.make_case(("prior_far", 65, 0))
    kw = dict(iterations=3, rounds=2, chi2=(9.0, 4.0, 5.991, 5.991), huber_delta2=4.0, close_factor=1.25, close_depth=6.0, gravity=9.8,
              prior_huber_delta=2.5, inlier_threshold=66)
    want = PS.ref(sc, **kw)
    assert want["rounds_run"] == 2 and list(want["round_iterations"]) == [3, 3] and want["accepted"] == 0
    assert want["round_prior_weight"][0] != PS.ref_cached(("prior_far", 65, 0))["round_prior_weight"][0]
    same(call(ex, sc, **kw), want, "prior_far, 3 iterations, 2 rounds, prior delta 2.5")


def test_two_calls_give_equal_bytes(ex):
    sc = PS.make_case(("outliers", 1000, 0))
    a, b = call(ex, sc), call(ex, sc)
    same(a, b, "second call")
    c = call(ex, sc, want_info=False)
    for k in ("Rwb", "twb", "v", "bg", "ba", "H30", "Hprior", "outlier"):
        assert c[k].tobytes() == a[k].tobytes(), k
    assert c["n_inliers"] == a["n_inliers"] and c["accepted"] == a["accepted"]
    d = call(ex, sc, want_prior=False)   # without the marginalisation: everything else is the same
    assert d["Hprior"] is None
    for k in ("Rwb", "twb", "v", "bg", "ba", "H30", "outlier", "round_state"):
        assert d[k].tobytes() == a[k].tobytes(), k


def test_host_marginalisation_equals_the_kernels_epilogue(ex):
    import orbfe
    for case in (("general", 257, 0), ("rank_deficient_prior", 64, 0)):
        got = call(ex, PS.make_case(case), want_info=False)
        assert orbfe.marginalize_pose_imu(got["H30"]).tobytes() == got["Hprior"].tobytes(), case


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


BATCH = (("outliers", 257, 0), ("few", 0, 0), ("prior_far", 65, 0))


@pytest.mark.parametrize("shared", [False, True], ids=["per_frame_points", "shared_points"])
def test_batch_equals_single_calls(ex, shared):
    """3 frames of different kinds and sizes (one without any match) in one launch, each with its own link, prior and state, against
    three host calls"""
    import torch
    import orbfe
    scs = [PS.make_case(c) for c in BATCH]
    B = len(scs)
    stride = max(len(sc["kp_xy"]) for sc in scs) + 7
    M = max(len(sc["points"]) for sc in scs)
    if shared:   # one point set for all frames: each frame's indices are shifted into it
        off = np.cumsum([0] + [len(sc["points"]) for sc in scs])
        M = int(off[-1])
    kp = np.zeros((B, stride), orbfe.KP_DTYPE)
    match = np.full((B, stride), -1, np.int32)
    pts = np.zeros((1 if shared else B, M), orbfe.WP_DTYPE)
    depth = np.zeros((1 if shared else B, M), np.float32)
    state = np.zeros((B, 33), np.float32)
    links, priors = b"", b""
    n = np.zeros(B, np.int32)
    singles = []
    for b, sc in enumerate(scs):
        k = keypoints(sc)
        n[b] = len(k)
        kp[b, :len(k)] = k
        kp[b, len(k):]["octave"] = 99   # beyond d_n: never read
        mi = sc["mp_index"].copy()
        row, base = (0, int(off[b])) if shared else (b, 0)
        for i, f in enumerate("xyz"):
            pts[row, base:base + len(sc["points"])][f] = sc["points"][:, i]
        depth[row, base:base + len(sc["points"])] = sc["track_depth"]
        match[b, :len(k)] = np.where(mi >= 0, mi + base, -1)
        match[b, len(k):] = 5       # beyond d_n: never read
        state[b] = state_in(sc)
        links += np.array([len(link_bytes(sc["link"])) + 8, 0], np.int32).tobytes() + link_bytes(sc["link"])
        priors += np.array([len(prior_bytes(sc["prior"])) + 8, 0], np.int32).tobytes() + prior_bytes(sc["prior"])
        singles.append(call(ex, sc, want_info=False))
    assert len(links) == B * 1216 and len(priors) == B * 1976
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
        ex, orbfe.PoseInertialPrevParams(scs[0]["cam"]), B, d_links.data_ptr(), d_priors.data_ptr(), d_kp.data_ptr(), d_n.data_ptr(), stride,
        d_match.data_ptr(), M, d_pts.data_ptr(), 0 if shared else M, d_depth.data_ptr(), d_state.data_ptr(), d_out.data_ptr(),
        d_H.data_ptr(), d_Hp.data_ptr(), d_outl.data_ptr(), d_ninl.data_ptr(), d_acc.data_ptr(), st.cuda_stream)
    st.synchronize()
    out, Hs, Hps = d_out.cpu().numpy().reshape(B, 21), d_H.cpu().numpy().reshape(B, 30, 30), d_Hp.cpu().numpy().reshape(B, 15, 15)
    outl, ninl, acc = d_outl.cpu().numpy().reshape(B, stride), d_ninl.cpu().numpy(), d_acc.cpu().numpy()
    for b, one in enumerate(singles):
        assert np.concatenate([one[k] for k in ("Rwb", "twb", "v", "bg", "ba")]).tobytes() == out[b].tobytes(), "frame %d: state" % b
        assert one["H30"].tobytes() == Hs[b].tobytes(), "frame %d: Hessian" % b
        assert one["Hprior"].tobytes() == Hps[b].tobytes(), "frame %d: marginalised Hessian" % b
        assert outl[b, :n[b]].tobytes() == one["outlier"].tobytes(), "frame %d: flags" % b
        assert (outl[b, n[b]:] == 0xAB).all(), "frame %d: bytes beyond d_n written" % b
        assert int(ninl[b]) == one["n_inliers"] and int(acc[b]) == one["accepted"], "frame %d: count" % b
    assert singles[1]["n_inliers"] == 0 and singles[1]["accepted"] == 0 and singles[0]["n_inliers"] > 120 and singles[2]["accepted"] == 1

"""orbfe_initial_bundle_adjustment on the GPU against the restatement of SPEC DECISION S17 (initial_ba_ref.initial_bundle_adjustment,
written from src/Optimizer.cc:60-369) on the scenes of initial_ba_scenarios (test_initial_ba.py checks which exits and branches they
reach).  Every comparison is exact: the bytes of the pose, the points and every field of orbfe_initial_ba_info.  No tolerance, no
skipped element; the zero_depth and nan_depth scenes compare their non-finite values by position and kind (NaN payloads differ between hosts and the
GPU) and everything finite by bytes.
The sizes are those where the mapping of points to threads changes, not the workload's: N = 1, 2 (the tree of one and of two), 63, 64,
65 (the 64 -> 256 thread switch), 257 (two points a thread, an odd count), 512, 513 (the last size whose points stay in registers and
the first parked in memory, walked by the waves), 1024, 1025, and one case at 4097 (32 chunks a wave)."""
import numpy as np
import pytest

import initial_ba_scenarios as BS
from test_initial_ba_cpp import keypoints, same

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
CASES = BS.CASES + [("general", 512, 0), ("general", 513, 0)]


def call(ex, sc, want_info=True, **kw):
    import orbfe
    kw.setdefault("robust", int(sc["robust"]))
    return orbfe.initial_bundle_adjustment(ex, orbfe.InitialBAParams(sc["cam"], **kw), keypoints(sc["kp1_xy"], sc["kp1_octave"], orbfe.KP_DTYPE),
                                           keypoints(sc["kp2_xy"], sc["kp2_octave"], orbfe.KP_DTYPE), sc["matches12"], sc["points"],
                                           sc["Rcw1"], sc["tcw1"], sc["Rcw2"], sc["tcw2"], want_info)


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    assert e.mvInvLevelSigma2.tobytes() == (np.float32(1.0) / BS.level_sigma2()).astype(np.float32).tobytes()  # the scenes' table is the handle's
    yield e
    e.close()


@pytest.mark.parametrize("case", CASES, ids=BS.case_id)
def test_equals_restatement(ex, case):
    sc, want = BS.make_case(case), BS.ref_cached(case)
    same(call(ex, sc), want, BS.case_id(case), case[0] in BS.NONFINITE)


def test_two_calls_give_equal_bytes_and_info_is_optional(ex):
    for case in (("outliers", 257, 0), ("far", 1025, 0)):
        sc = BS.make_case(case)
        a, b = call(ex, sc), call(ex, sc)
        same(a, b, "second call")
        c = call(ex, sc, want_info=False)
        assert c["Tcw2"].tobytes() == a["Tcw2"].tobytes() and c["points"].tobytes() == a["points"].tobytes()


def test_iterations_and_robust_are_the_calls_parameters(ex):
    """not constants of the kernel"""
    sc = BS.make_case(("outliers", 257, 0))
    want = BS.ref(sc, iterations=3, robust_kernel=False, huber_delta2=4.0)
    assert want["iterations"] == 3 and want["exit"] == 0
    same(call(ex, sc, iterations=3, robust=0, huber_delta2=4.0), want, "outliers, 3 iterations, no kernel")
    want = BS.ref(sc, iterations=3, huber_delta2=4.0)
    same(call(ex, sc, iterations=3, huber_delta2=4.0), want, "outliers, 3 iterations, delta^2 = 4")
    assert want["pose"].tobytes() != BS.ref_cached(("outliers", 257, 0))["pose"].tobytes()


def test_fed_from_two_view_reconstruction(ex):
    """the initialisation chain: orbfe_two_view_reconstruct's pose and points of a twoview_scenarios general scene go into the call;
    the result must equal the restatement on the same data"""
    import orbfe
    import initial_ba_ref as R
    import twoview_scenarios as TS
    sc = TS.make("general")
    fx, fy, cx, cy, sigma, iterations = sc["params"]
    kp1, kp2 = keypoints(sc["kp1"], 0, orbfe.KP_DTYPE), keypoints(sc["kp2"], 0, orbfe.KP_DTYPE)   # octave 0, as the two-view tests have it
    rec = orbfe.two_view_reconstruct(ex, orbfe.TwoViewParams(fx, fy, cx, cy, sigma, iterations), kp1, kp2, sc["matches12"], sc["sets"], False)
    assert rec["reconstructed"] and int(rec["triangulated"].sum()) > 50
    m12 = np.where(rec["triangulated"] != 0, sc["matches12"], -1).astype(np.int32)   # vIniMatches after Reconstruct (src/Tracking.cc:578-585)
    cam = np.array([fx, fy, cx, cy, 0, 0, 0, 0], np.float32)
    R1, t1 = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)
    got = orbfe.initial_bundle_adjustment(ex, orbfe.InitialBAParams(cam), kp1, kp2, m12, rec["p3d"], R1, t1, rec["R21"], rec["t21"])
    want = R.initial_bundle_adjustment(cam, BS.level_sigma2(), np.stack([kp1["x"], kp1["y"]], 1), kp1["octave"],
                                       np.stack([kp2["x"], kp2["y"]], 1), kp2["octave"], m12, rec["p3d"], R1, t1, rec["R21"], rec["t21"])
    same(got, want, "two-view chain")
    assert want["it_cost"][-1] < want["it_cost"][0] and want["N"] == int(rec["triangulated"].sum())

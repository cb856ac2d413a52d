"""SPEC DECISION S23 on the CPU: the three rules track_inertial_ref restates -- the camera centre from the predicted pose, the
statistics of src/Tracking.cc:958-982, the pose the frame is left with -- and the scenes of track_inertial_scenarios through the chain
of restatements, which must reach every planted verdict before the GPU tests gate on them.  No GPU."""
import numpy as np
import pytest

import imu_preint_ref as R22
import imu_preint_scenarios as PS
import track_inertial_ref as T
import track_inertial_scenarios as TS

f32, f64 = np.float32, np.float64


def test_twc_within_the_derived_bound():
    """twc_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2) in binary32 against -R^T t in binary64 on 1000 seeded poses.  Three rounded
    products and two rounded additions: every product carries at most (1 + u) and passes through at most two additions, so
    |error_k| <= gamma_3 sum_i |R_ik t_i| with gamma_3 = 3u / (1 - 3u) < 4u, u = 2^-24 (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1); the negation is exact.  The bound is derived, not measured."""
    rng = np.random.RandomState(2301)
    u = 2.0 ** -24
    worst = 0.0
    for _ in range(1000):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        R = q.astype(f32)
        t = (rng.uniform(-20, 20, 3) * 10.0 ** rng.uniform(-3, 1)).astype(f32)
        got = T.twc_from_state(R.reshape(9), t).astype(f64)
        Rd, td = R.astype(f64), t.astype(f64)
        want = -(Rd.T @ td)
        bound = 4.0 * u * (np.abs(Rd) * np.abs(td)[:, None]).sum(0)
        assert (np.abs(got - want) <= bound).all(), (got, want, bound)
        worst = max(worst, float((np.abs(got - want) / bound).max()))
    print("largest error / bound: %.3f" % worst)
    assert worst > 0.0   # the comparison is not vacuous: binary32 does round here


def test_statistics_of_a_planted_frame():
    """five keypoints, four id slots, counts written by hand:
      keypoint 0 -> slot 2, inlier, observations 3            found, counted
      keypoint 1 -> slot 0, inlier, observations 0            found, NOT counted (:969 Observations() > 0)
      keypoint 2 -> slot 3, flagged outlier, observations 2   not found, not counted
      keypoint 3 -> no match
      keypoint 4 -> beyond n: ignored although it carries a match
      slot 1: nobody matched it"""
    match = np.array([2, 0, 3, -1, 1], np.int32)
    outlier = np.array([0, 0, 1, 0, 0], np.uint8)
    obs = np.array([0, 4, 3, 2], np.int32)
    found, count, tracked = T.statistics(4, match, outlier, obs, 4, 8)
    assert found.tolist() == [1, 0, 1, 0] and count == 1 and tracked == 0
    assert T.statistics(4, match, outlier, obs, 4, 1)[2] == 1          # the threshold is >=
    empty = T.statistics(0, match, outlier, obs, 4, 0)                 # no keypoint: nothing found, 0 >= 0 is tracked
    assert empty[0].tolist() == [0, 0, 0, 0] and empty[1:] == (0, 1)


@pytest.mark.parametrize("case", [("moving", 3, 0), ("bias_changed", 10, 0), ("still", 3, 0)], ids=PS.case_id)
def test_tcw_out_is_set_imu_pose_velocity(case):
    """the pose behind the optimisation is SetImuPoseVelocity as imu_preint_ref.predict_state writes it: on the predicted Rwb / twb it
    gives the predicted Rcw / tcw, bytes"""
    sc = PS.make(*case)
    for which in (R22.FROM_KEYFRAME, R22.FROM_FRAME):
        s = PS.ref_cached(case, which)["state"]
        got = T.set_imu_pose(s[12:21], s[21:24], sc["Rcb"], sc["tcb"])
        assert got.tobytes() == s[0:12].tobytes()
        assert T.tcw_out(which, 1, s, s[12:33], sc["Rcb"], sc["tcb"]).tobytes() == s[0:12].tobytes()
    # a result that is not accepted leaves the predicted pose, whatever the optimiser wrote; the key-frame kind always applies
    s = PS.ref_cached(case, R22.FROM_FRAME)["state"]
    moved = s[12:33].copy()
    moved[9:12] += f32(0.25)
    assert T.tcw_out(R22.FROM_FRAME, 0, s, moved, sc["Rcb"], sc["tcb"]).tobytes() == s[0:12].tobytes()
    assert T.tcw_out(R22.FROM_FRAME, 1, s, moved, sc["Rcb"], sc["tcb"]).tobytes() != s[0:12].tobytes()
    assert T.tcw_out(R22.FROM_KEYFRAME, 0, s, moved, sc["Rcb"], sc["tcb"]).tobytes() == \
        T.tcw_out(R22.FROM_FRAME, 1, s, moved, sc["Rcb"], sc["tcb"]).tobytes()


def test_ids_resolve_as_the_gather_kernel_states():
    import orbfe
    pts = np.zeros(4, orbfe.WP_DTYPE)
    pts["x"] = [1, 2, 3, 4]
    pts["skip"] = 1            # the stored member is ignored: it is per frame
    desc = np.arange(128, dtype=np.uint8).reshape(4, 32)
    seen, d, rows = T.resolve_ids(np.array([2, ~1, 4, 2 ** 31 - 1], np.int32), 4, pts, desc)
    assert seen["x"].tolist() == [3, 2, 0, 0] and seen["skip"].tolist() == [0, 1, 1, 1] and seen["bad"].tolist() == [0, 0, 1, 1]
    assert d[0].tobytes() == desc[2].tobytes() and d[1].tobytes() == desc[1].tobytes() and not d[2:].any()
    assert rows[:2].tobytes() == pts[[2, 1]].tobytes() and rows[2:].tobytes() == bytes(64)


@pytest.fixture(scope="module")
def cpu_frames(built):
    import orbfe
    return {M: TS.make_batch(TS.KINDS, M, orbfe.WP_DTYPE, orbfe.KP_DTYPE) for M in (70, 300)}


@pytest.mark.parametrize("which", (R22.FROM_KEYFRAME, R22.FROM_FRAME), ids=("keyframe", "frame"))
def test_scene_reaches_every_planted_verdict(cpu_frames, which):
    """the ordinary frame of the M = 70 scene through the restatements alone: an outlier that the matcher matched, an inlier whose
    point has no observation, and every other planted slot.  A scene that does not produce them fails here; nothing skips."""
    frames, capacity, points, desc = cpu_frames[70]
    fr = frames[0]
    out = TS.chain(TS.CpuStages(), fr, which, capacity, points, desc, TS.prior_of(fr, 0) if which == R22.FROM_FRAME else None)
    v = TS.planted_verdicts(fr, out)
    print(v, "matches %d inliers %d counted %d" % (out["n_matches"], out["n_inliers"], out["matches_inliers"]))
    assert all(v.values()), v
    assert out["outlier"].sum() >= 1 and out["accepted"] == 1 and out["tracked"] == 1 and out["matches_inliers"] > 30
    assert out["Tcw"].tobytes() != out["state_in"][0:12].tobytes()     # the optimisation moved the pose


def test_matcher_and_projection_reach_the_planted_slots_at_both_sizes(cpu_frames):
    """the stages in front of the optimiser, both sizes, all three frames (cheap: the C oracle): M = 300 spans two blocks of the gather
    kernel, the standing frame predicts from the records as they stand, the empty frame matches nothing"""
    st = TS.CpuStages()
    for M, (frames, capacity, points, desc) in cpu_frames.items():
        for fr in frames:
            state_in, _link, ok = st.imu(fr, R22.FROM_KEYFRAME)
            seen, mpd, _rows = T.resolve_ids(fr["ids"], capacity, points, desc)
            mps = st.project(state_in, seen)
            assert ok and mps["inView"][TS.S_UNMATCHED] == 1 and mps["inView"][[TS.S_SKIP, TS.S_NOPOINT, TS.S_BEHIND, TS.S_OUTSIDE]].sum() == 0
            if fr["n"] == 0:
                continue
            nm, match = st.match(fr["kp"], fr["kp_desc"], mps, mpd)
            k = fr["kp_of_slot"]
            assert match[k[TS.S_FAR_KP]] == TS.S_FAR_KP and match[k[TS.S_NO_OBS]] == TS.S_NO_OBS and match[k[TS.S_SKIP]] == -1
            assert nm == len(k) - 1 == (match >= 0).sum(), (M, fr["kind"], nm, len(k))

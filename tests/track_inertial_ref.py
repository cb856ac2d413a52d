"""SPEC DECISION S23, normative: what orbfe_track_inertial_batch_device adds between the stages it chains --
the frustum built from the predicted state, the hand-over of point rows and depths to the inertial pose optimisation, the statistics
of Tracking::TrackLocalMap (src/Tracking.cc:958-982) and the pose the frame is left with (Frame::SetImuPoseVelocity,
src/Frame.cc:221-238).  Written from those lines and the text of S23, not from the kernels.

Rules as S8 / S22: binary32, one IEEE operation per operator, left to right, no contraction; a 3-term dot product is
(a0 b0 + a1 b1) + a2 b2.
"""
import numpy as np

import imu_preint_ref as R22

f32 = np.float32


def twc_from_state(rcw, tcw):
    """mTwc = mTcw.inverse() (src/Frame.cc:234) with R^T taken by index: twc_k = -((R_0k t_0 + R_1k t_1) + R_2k t_2).  Stated
    departure: no quaternion round trip."""
    R = np.asarray(rcw, f32).reshape(3, 3)
    t = np.asarray(tcw, f32).reshape(3)
    with np.errstate(all="ignore"):
        out = -((R[0, :] * t[0] + R[1, :] * t[1]) + R[2, :] * t[2])
    assert out.dtype == f32
    return out


def frustum_pose(state_in):
    """the pose fields of frame b's frustum from its 33-float predicted state -> (rcw [9], tcw [3], twc [3])"""
    s = np.asarray(state_in, f32).reshape(33)
    return s[0:9].copy(), s[9:12].copy(), twc_from_state(s[0:9], s[9:12])


def resolve_ids(ids, capacity, points, desc, wp_names=("bad", "skip")):
    """the id list of one frame against the resident map -> (the points isInFrustum sees, their descriptors, the rows the pose
    optimisation is handed).  id >= 0: the map's entry; ~id: the same entry, skipped for this frame; outside the map: a bad, skipped
    record with a zero descriptor and a zero row."""
    bad, skip = wp_names
    ids = np.asarray(ids, np.int32)
    M = len(ids)
    seen = np.zeros(M, points.dtype)
    rows = np.zeros(M, points.dtype)
    d = np.zeros((M, 32), np.uint8)
    for i, raw in enumerate(ids):
        k = int(~raw) if raw < 0 else int(raw)
        if k < capacity:
            seen[i] = points[k]
            rows[i] = points[k]
            seen[i][skip] = 1 if raw < 0 else 0
            d[i] = desc[k]
        else:
            seen[i][bad] = 1
            seen[i][skip] = 1
    return seen, d, rows


def statistics(n, match, outlier, observations, M, inlier_threshold):
    """the loop of src/Tracking.cc:958-982 (mbOnlyTracking == false, mono): for keypoint i < n with m = match[i] >= 0,
    found[m] = !outlier[i] (IncreaseFound, :967) and matches_inliers += !outlier[i] && Observations(m) > 0 (:969-976)
    -> (found [M] uint8, matches_inliers, tracked)"""
    found = np.zeros(M, np.uint8)
    count = 0
    for i in range(n):
        m = int(match[i])
        if m < 0:
            continue
        if not outlier[i]:
            found[m] = 1
            if observations[m] > 0:
                count += 1
    return found, count, int(count >= inlier_threshold)


def set_imu_pose(Rwb, twb, Rcb, tcb):
    """Frame::SetImuPoseVelocity (src/Frame.cc:221-238), the text of imu_preint_ref.predict_state: Rcw = Rcb Rwb^T,
    tcw = Rcb (-(Rwb^T twb)) + tcb -> 12 floats, Rcw then tcw"""
    Rwb = np.asarray(Rwb, f32).reshape(3, 3)
    twb = np.asarray(twb, f32).reshape(3)
    Rcb = np.asarray(Rcb, f32).reshape(3, 3)
    tcb = np.asarray(tcb, f32).reshape(3)
    with np.errstate(all="ignore"):
        Rbw = np.ascontiguousarray(Rwb.T)
        Rcw = R22.mul3(Rcb, Rbw)
        tcw = R22.mv(Rcb, -R22.mv(Rbw, twb)) + tcb
    out = np.concatenate([Rcw.reshape(9), tcw])
    assert out.dtype == f32
    return out


def tcw_out(which, accepted, state_in, state_out, Rcb, tcb):
    """the pose TrackLocalMap leaves the frame with: SetImuPoseVelocity on the optimised Rwb / twb; with the last-frame kind and a
    result that is not accepted, the reference does not apply it (src/Optimizer.cc:4208) and the predicted pose stands"""
    if which == R22.FROM_FRAME and not accepted:
        return np.asarray(state_in, f32).reshape(33)[0:12].copy()
    s = np.asarray(state_out, f32).reshape(21)
    return set_imu_pose(s[0:9], s[9:12], Rcb, tcb)

"""Seeded two-view scenes for the S17 tests (tests/test_initial_ba*.py), in the style of poseopt_scenarios.py: N points at depth 2 .. 10
seen from two key frames a baseline apart, projections with pixel noise scaled by the keypoint's octave, extra keypoints in both frames
(point index != keypoint index, n1 != n2), key frame 2's keypoints shuffled, and a start -- pose 2 and the points -- that is off by a
kind-dependent amount.  Pose 1 is the identity except in general_pose1.

kinds:
  general        pose 2 off by 2 degrees / 3 cm, points off by 2 %, 0.5 px noise
  general_pose1  the same under a non-identity fixed pose
  converged      the truth as floats, noise-free: dx -> 0, the small-theta branch of exp
  far            10 degrees / 0.2 m / 10 %: rejected trials and a growing lambda
  outliers       20 % gross mismatches in key frame 2: Huber's linear region
  robust_off     the outliers scene's data, run by the tests with robust = 0
  low_parallax   baseline 0.01: D is near-singular for small lambda
  zero_depth     one point on pose 2's plane z = 0 (identity rotations, exact floats): non-finite blocks and sums
  unmatched      half of matches12 negative
  behind         the general scene mirrored through key frame 1's centre (X -> -X, t2 -> -t2): the same projections, every depth
                 negative in both frames; the adjustment converges there and the adaptor's median depth is negative
  nan_depth      one matched input point is a NaN: non-finite sums, nothing is accepted, the point comes back as it went in and
                 its depth in key frame 1 is a NaN
"""
import numpy as np

import initial_ba_ref as R
from mlpnp_scenarios import H, N_LEVELS, PINHOLE, W, _rodrigues, level_sigma2

# kind: (rotation offset in degrees, translation offset in metres, relative point offset, noise in level-0 pixels, baseline)
KINDS = {"general": (2.0, 0.03, 0.02, 0.5, 0.3), "general_pose1": (2.0, 0.03, 0.02, 0.5, 0.3), "converged": (0.0, 0.0, 0.0, 0.0, 0.3),
         "far": (10.0, 0.2, 0.1, 0.5, 0.3), "outliers": (2.0, 0.03, 0.02, 0.5, 0.3), "robust_off": (2.0, 0.03, 0.02, 0.5, 0.3),
         "low_parallax": (0.2, 0.001, 0.02, 0.5, 0.01), "zero_depth": (0.0, 0.0, 0.02, 0.5, 0.3), "unmatched": (2.0, 0.03, 0.02, 0.5, 0.3),
         "behind": (2.0, 0.03, 0.02, 0.5, 0.3), "nan_depth": (2.0, 0.03, 0.02, 0.5, 0.3)}
N_LIST = [1, 2, 63, 64, 65, 257, 1024, 1025, 4097]
POSE1_OMEGA, POSE1_CENTRE = (0.10, -0.20, 0.05), (0.3, -0.2, 0.1)
REL_OMEGA = (0.02, -0.05, 0.01)   # key frame 2 against key frame 1


def make(kind, N=300, seed=0):
    """-> dict(cam, level_sigma2, kp1_xy [n1, 2] float32, kp1_octave, kp2_xy [n2, 2], kp2_octave, matches12 [n1], points [n1, 3] float32
    (the start; rows without a match hold other values that must come back untouched), Rcw1, tcw1, Rcw2, tcw2 (float32; pose 2 is the
    start), R2_true, t2_true, X_true [N, 3], robust, kind, N)"""
    rot_deg, shift, rel, noise, baseline = KINDS[kind]
    rng = np.random.RandomState(9000 * seed + 17 * N + len(kind))
    cam = np.array(PINHOLE, np.float32)
    fx, fy, cx, cy = (float(v) for v in cam[:4])
    s2 = level_sigma2()
    if kind == "general_pose1":
        R1 = _rodrigues(POSE1_OMEGA).astype(np.float32).astype(np.float64)
        t1 = (-R1 @ np.array(POSE1_CENTRE)).astype(np.float32).astype(np.float64)
    else:
        R1, t1 = np.eye(3), np.zeros(3)
    if kind == "zero_depth":   # identity rotation: Xc2.z = Z + tz exactly
        R21, t21 = np.eye(3), np.array([-0.25, 0.0, 0.5])
    else:
        R21 = _rodrigues(REL_OMEGA)
        d = np.array([-1.0, 0.1, 0.05])
        t21 = baseline * d / np.linalg.norm(d)
    R2, t2 = R21 @ R1, R21 @ t1 + t21
    if kind == "converged":   # the truth must be representable: the caller's pose is float
        R2, t2 = R2.astype(np.float32).astype(np.float64), t2.astype(np.float32).astype(np.float64)
    nAll = 2 * N if kind == "unmatched" else N   # unmatched: every second candidate loses its match below
    uv = np.stack([rng.uniform(60, W - 60, nAll), rng.uniform(60, H - 60, nAll)], 1)
    z = rng.uniform(2.0, 10.0, nAll)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(nAll)], 1)
    Xw = ((ray * z[:, None] - t1) @ R1).astype(np.float32).astype(np.float64)
    if kind == "zero_depth":
        Xw[nAll // 2] = (1.0, 0.5, -0.5)

    def view(Rc, tc, sigma):
        Xc = Xw @ Rc.T + tc
        with np.errstate(all="ignore"):
            p = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
        p[~np.isfinite(p)] = 100.0
        return p + rng.normal(size=(nAll, 2)) * (noise * sigma)[:, None]
    oc1, oc2 = rng.randint(0, N_LEVELS, nAll), rng.randint(0, N_LEVELS, nAll)
    uv1 = view(R1, t1, np.sqrt(s2[oc1].astype(np.float64)))
    uv2 = view(R2, t2, np.sqrt(s2[oc2].astype(np.float64)))
    if kind in ("outliers", "robust_off"):
        nOut = max(int(round(0.2 * nAll)), 1)
        idx = rng.permutation(nAll)[:nOut]
        uv2[idx] = np.stack([rng.uniform(20, W - 20, nOut), rng.uniform(20, H - 20, nOut)], 1)
    # key frame 1: the candidates interleaved with extra keypoints; key frame 2: shuffled, with another number of extras
    e1, e2 = nAll // 4 + 3, nAll // 3 + 5
    kp1 = np.concatenate([uv1, np.stack([rng.uniform(20, W - 20, e1), rng.uniform(20, H - 20, e1)], 1)])
    o1 = np.concatenate([oc1, rng.randint(0, N_LEVELS, e1)])
    kp2 = np.concatenate([uv2, np.stack([rng.uniform(20, W - 20, e2), rng.uniform(20, H - 20, e2)], 1)])
    o2 = np.concatenate([oc2, rng.randint(0, N_LEVELS, e2)])
    perm1, perm2 = rng.permutation(len(kp1)), rng.permutation(len(kp2))
    inv1, inv2 = np.argsort(perm1), np.argsort(perm2)
    matches = np.full(len(kp1), -1, np.int32)
    keep = np.arange(nAll)
    if kind == "unmatched":
        keep = np.sort(rng.permutation(nAll)[:N])
    matches[inv1[keep]] = inv2[keep]
    start = Xw * (1.0 + rel * rng.normal(size=(nAll, 1))) if rel else Xw
    if kind == "zero_depth":
        start[nAll // 2] = Xw[nAll // 2]
    points = rng.uniform(-3, 3, (len(kp1), 3)).astype(np.float32)
    points[inv1[:nAll]] = start.astype(np.float32)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    dirn = rng.normal(size=3)
    dirn /= np.linalg.norm(dirn)
    R20 = _rodrigues(np.deg2rad(rot_deg) * axis) @ R2
    t20 = t2 + shift * dirn
    if kind == "behind":   # pose 1 is the identity: R2 (-X) + (-t2) = -(R2 X + t2), and x / z does not see the sign
        points[inv1[:nAll]] = -points[inv1[:nAll]]
        t20 = -t20
    if kind == "nan_depth":
        points[inv1[nAll // 2], 2] = np.nan
    order = np.sort(inv1[keep])
    Xtrue = np.zeros((len(kp1), 3))
    Xtrue[inv1[:nAll]] = Xw
    return dict(cam=cam, level_sigma2=s2, kp1_xy=kp1[perm1].astype(np.float32), kp1_octave=o1[perm1].astype(np.int32),
                kp2_xy=kp2[perm2].astype(np.float32), kp2_octave=o2[perm2].astype(np.int32), matches12=matches, points=points,
                Rcw1=R1.astype(np.float32).reshape(9), tcw1=t1.astype(np.float32), Rcw2=R20.astype(np.float32).reshape(9),
                tcw2=t20.astype(np.float32), R2_true=R2, t2_true=t2, X_true=Xtrue[order], robust=kind != "robust_off", kind=kind, N=N)


def ref(sc, **kw):
    kw.setdefault("robust_kernel", sc["robust"])
    return R.initial_bundle_adjustment(sc["cam"], sc["level_sigma2"], sc["kp1_xy"], sc["kp1_octave"], sc["kp2_xy"], sc["kp2_octave"],
                                       sc["matches12"], sc["points"], sc["Rcw1"], sc["tcw1"], sc["Rcw2"], sc["tcw2"], **kw)


_cache = {}


def ref_cached(case):
    """the restatement's result of a case, computed once per session and shared"""
    if case not in _cache:
        _cache[case] = ref(make_case(case))
    return _cache[case]


# (kind, N, seed): the comparison set of tests/test_initial_ba_gpu.py; the sizes are where the mapping of points to threads changes
CASES = [("general", n, 0) for n in N_LIST] + [
    ("general_pose1", 65, 0), ("general_pose1", 257, 0), ("converged", 64, 0), ("converged", 257, 0), ("far", 65, 0), ("far", 1025, 0),
    ("outliers", 63, 0), ("outliers", 257, 0), ("robust_off", 257, 0), ("low_parallax", 65, 0), ("low_parallax", 1025, 0),
    ("zero_depth", 2, 0), ("zero_depth", 257, 0), ("unmatched", 64, 0), ("unmatched", 1025, 0), ("behind", 257, 0), ("nan_depth", 257, 0),
]
NONFINITE = ("zero_depth", "nan_depth")   # kinds whose results hold non-finite values
HOST_CASES = [("general", 65, 0), ("outliers", 63, 0), ("far", 65, 0), ("zero_depth", 257, 0), ("general", 1, 0), ("unmatched", 64, 0),
              ("behind", 257, 0), ("nan_depth", 257, 0)]


def case_id(c):
    return "%s-N%d-seed%d" % c


def make_case(c):
    return make(c[0], c[1], c[2])

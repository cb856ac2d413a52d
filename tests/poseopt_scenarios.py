"""Seeded scenes for the S14 tests (tests/test_poseopt*.py), in the style of mlpnp_scenarios.py: world points seen from a pose,
projections with pixel noise scaled by the keypoint's octave, unmatched keypoints interleaved (edge index != keypoint index), map points
stored shuffled (mp_index != edge index), and an initial pose that is off by a kind-dependent amount.

kinds:
  general     initial pose a few degrees / centimetres off
  converged   initial pose = the truth (as floats), noise-free projections of it: dx -> 0, the small-theta branch of exp
  far         20 degrees / 0.5 m off: rejected trials and a growing lambda
  outliers    30 % wrong matches plus a sixth of the rest displaced to chi2 near the gate; the flag of at least one edge changes
              twice over the rounds (seeds are searched for that)
  huber_off   25 % of the matches displaced one-sidedly by about two sigma: Huber's linear region is active on the way from the
              initial pose, so round 3 (no kernel) takes another path and ends at another pose than round 2.  Only in the last
              bits: an inlier of round 2 has chi2 <= 5.991 < delta^2 = 7.815, so no active edge is in the linear region at the optimum
  collapsed   all points at one world position: H has rank 2.  Under Levenberg's lambda > 0 the damped system keeps positive pivots,
              so the solve succeeds (test_poseopt.py asserts that; `!ok` is reached by zero_depth, the 10-trial exit by general-N63)
  behind      a fifth of the points behind the camera (z < 0)
  zero_depth  one point with Xc.z == 0 at the initial pose (identity rotation, exact floats): non-finite sums
"""
import numpy as np

import poseopt_ref as R
from mlpnp_scenarios import H, N_LEVELS, PINHOLE, W, _rodrigues, level_sigma2

TRUE_OMEGA, TRUE_CENTRE = (0.10, -0.20, 0.05), (0.3, -0.2, 0.1)
# kind: (rotation offset in degrees, translation offset in metres, noise in level-0 pixels)
KINDS = {"general": (3.0, 0.05, 0.5), "converged": (0.0, 0.0, 0.0), "far": (20.0, 0.5, 0.5), "outliers": (3.0, 0.05, 0.5),
         "huber_off": (3.0, 0.05, 0.5), "collapsed": (3.0, 0.05, 0.5), "behind": (3.0, 0.05, 0.5), "zero_depth": (0.0, 0.0, 0.5)}
NE_LIST = [2, 3, 9, 10, 63, 64, 65, 300, 1000, 1025, 4097]


def make(kind, Ne=300, seed=0, extra=0.25):
    """-> dict(cam, level_sigma2, kp_xy [n, 2] float32, kp_octave [n], mp_index [n], points [m, 3] float32, Rcw [9] float32, tcw [3]
    float32 (the initial pose), R_true, t_true, kind, Ne)"""
    rot_deg, shift, noise = KINDS[kind]
    rng = np.random.RandomState(7000 * seed + 13 * Ne + len(kind))
    cam = np.array(PINHOLE, np.float32)
    fx, fy, cx, cy = (float(v) for v in cam[:4])
    s2 = level_sigma2()
    if kind == "zero_depth":
        Rt, tt = np.eye(3), np.array([0.25, -0.125, 0.5])
    else:
        Rt = _rodrigues(TRUE_OMEGA)
        tt = -Rt @ np.array(TRUE_CENTRE, np.float64)
    if kind == "converged":  # the truth must be representable: the caller's pose is float
        Rt, tt = Rt.astype(np.float32).astype(np.float64), tt.astype(np.float32).astype(np.float64)
    uv = np.stack([rng.uniform(30, W - 30, Ne), rng.uniform(30, H - 30, Ne)], 1)
    z = rng.uniform(2.0, 10.0, Ne)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(Ne)], 1)
    Xw = ((ray * z[:, None] - tt) @ Rt).astype(np.float32).astype(np.float64)
    if kind == "collapsed":
        Xw[:] = Xw[0]
    if kind == "behind":
        idx = rng.permutation(Ne)[:max(Ne // 5, 1)]
        Xc = Xw[idx] @ Rt.T + tt
        Xc[:, 2] = -Xc[:, 2]
        Xw[idx] = ((Xc - tt) @ Rt).astype(np.float32)
    if kind == "zero_depth":  # identity rotation: Xc.z = Z + tz exactly; Z = -0.5 gives 0.0
        Xw[Ne // 2] = (1.0, 0.5, -0.5)
    Xc = Xw @ Rt.T + tt
    with np.errstate(all="ignore"):
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    uv[~np.isfinite(uv)] = 100.0
    octave = rng.randint(0, N_LEVELS, Ne)
    sig = np.sqrt(s2[octave].astype(np.float64))
    uv = uv + rng.normal(size=(Ne, 2)) * (noise * sig)[:, None]
    if kind == "outliers":
        nOut = int(round(0.3 * Ne))
        idx = rng.permutation(Ne)[:nOut]
        uv[idx] = np.stack([rng.uniform(20, W - 20, nOut), rng.uniform(20, H - 20, nOut)], 1)
        rest = np.setdiff1d(np.arange(Ne), idx)
        edge = rest[rng.permutation(len(rest))[:max(Ne // 6, 1)]]   # borderline matches: chi2 near the gate, so small pose changes flip them
        ang = rng.uniform(0, 2 * np.pi, len(edge))
        mag = rng.uniform(2.2, 2.7, len(edge)) * sig[edge]
        uv[edge] = uv[edge] + np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    if kind == "huber_off":
        nOff = max(int(round(0.25 * Ne)), 1)
        idx = rng.permutation(Ne)[:nOff]
        ang = rng.uniform(-0.4, 0.4, nOff)   # one-sided: a bias the Huber weight damps and the plain sum does not
        mag = rng.uniform(2.5, 3.5, nOff) * sig[idx] * 0.7
        uv[idx] = uv[idx] + np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    e = int(extra * Ne) + 3
    kp = np.concatenate([uv, np.stack([rng.uniform(20, W - 20, e), rng.uniform(20, H - 20, e)], 1)])
    oc = np.concatenate([octave, rng.randint(0, N_LEVELS, e)])
    perm = rng.permutation(len(kp))
    inv = np.argsort(perm)
    pperm = rng.permutation(Ne + 5)
    points = np.zeros((Ne + 5, 3), np.float32)
    points[pperm[:Ne]] = Xw
    points[pperm[Ne:]] = rng.uniform(-3, 3, (5, 3))
    mp_index = np.full(len(kp), -1, np.int32)
    mp_index[inv[:Ne]] = pperm[:Ne]
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    dirn = rng.normal(size=3)
    dirn /= np.linalg.norm(dirn)
    R0 = _rodrigues(np.deg2rad(rot_deg) * axis) @ Rt
    t0 = tt + shift * dirn
    return dict(cam=cam, level_sigma2=s2, kp_xy=kp[perm].astype(np.float32), kp_octave=oc[perm].astype(np.int32), mp_index=mp_index,
                points=points, Rcw=R0.astype(np.float32).reshape(9), tcw=t0.astype(np.float32), R_true=Rt, t_true=tt, kind=kind, Ne=Ne)


def ref(sc, **kw):
    return R.pose_optimization(sc["cam"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"], sc["Rcw"],
                               sc["tcw"], **kw)


_cache = {}


def ref_cached(case):
    """the restatement's result of a case, computed once per session and shared"""
    if case not in _cache:
        _cache[case] = ref(make_case(case))
    return _cache[case]


# (kind, N_e, seed): the comparison set of tests/test_poseopt.py and tests/test_poseopt_gpu.py
CASES = [("general", n, 0) for n in NE_LIST] + [
    ("converged", 64, 0), ("converged", 300, 0), ("far", 65, 0), ("far", 300, 0), ("far", 1025, 0),
    ("outliers", 63, 24), ("outliers", 300, 1), ("outliers", 1000, 1), ("huber_off", 300, 0), ("huber_off", 65, 0),
    ("collapsed", 10, 0), ("collapsed", 300, 0), ("behind", 64, 0), ("behind", 300, 0), ("zero_depth", 10, 0), ("zero_depth", 300, 0),
]


def case_id(c):
    return "%s-N%d-seed%d" % c


def make_case(c):
    return make(c[0], c[1], c[2])

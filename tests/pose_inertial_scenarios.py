"""Seeded scenes for the S19 tests (tests/test_pose_inertial*.py), in the style of poseopt_scenarios.py.  A consistent ground truth gives
the constants: the key frame's and the frame's body states are picked, the preintegrated dR, dV, dP are derived from them (plus
noise), the camera pose follows from the body pose and the extrinsics, the world points are seen from that camera.  Unmatched keypoints
are interleaved (edge index != keypoint index) and the map points are stored shuffled (mp_index != edge index).

kinds:
  general         a consistent scene with small noise; the start a degree and a few centimetres off
  converged       the start is the truth (as floats), noise-free projections and constants: the small-angle branches of LogSO3 /
                  InverseRightJacobianSO3 / ExpSO3
  far             start 5 degrees and 0.3 m off: the general branches
  outliers        30 % gross outliers, some close, some beyond 10 m, plus a sixth of the rest displaced to chi2 near the gates; at
                  N_e = 1000, seed 0, the flag of one edge changes twice over the rounds (seeds were looked through for that)
  close_boundary  a quarter of the edges displaced to chi2 between chi2Mono and 1.5 chi2Mono of the last rounds, on both sides of
                  track_depth = 10: the close ones stay, the others are flagged
  few             general with the N_e asked for (0, 1, 6, 7: the N_e + 3 < 10 break on either side)
  recover         25 edges, a third of them displaced to chi2 of about 16-22: flagged in every round, taken back by the recovery
                  (rec_init = 0) or not (rec_init = 1)
  behind          a fifth of the points behind the camera (z < 0)
  zero_depth      one point with Xc.z == 0 at the caller's camera pose (identity rotations, exact floats): non-finite sums, the
                  solve is not positive, the round ends with the state kept
  weak_imu / strong_imu   info9 scaled by 1e-6 / 1e6
  scaled_dR       dR = (1 + 1e-6) I and the frame's rotation = the key frame's: costheta > 1, LogSO3's early return
"""
import numpy as np

import pose_inertial_ref as R
from mlpnp_scenarios import H, N_LEVELS, PINHOLE, W, _rodrigues, level_sigma2

GRAVITY = np.float64(np.float32(9.81))
# kind: (rotation offset in degrees, translation offset in metres, noise in level-0 pixels)
KINDS = {"general": (1.0, 0.03, 0.5), "converged": (0.0, 0.0, 0.0), "far": (5.0, 0.3, 0.5), "outliers": (1.0, 0.03, 0.5),
         "close_boundary": (1.0, 0.03, 0.0), "few": (1.0, 0.03, 0.5), "recover": (1.0, 0.03, 0.3), "behind": (1.0, 0.03, 0.5),
         "zero_depth": (0.0, 0.0, 0.5), "weak_imu": (1.0, 0.03, 0.5), "strong_imu": (1.0, 0.03, 0.5), "scaled_dR": (0.0, 0.02, 0.5)}
NE_LIST = [0, 1, 6, 7, 63, 64, 65, 257, 300, 1000, 4097]


def _spd(rng, diag, mix):
    """a symmetric positive definite matrix with the given diagonal scale"""
    n = len(diag)
    A = rng.normal(size=(n, n))
    M = np.eye(n) + mix * (A + A.T) / (2.0 * np.sqrt(n))
    d = np.sqrt(np.asarray(diag, np.float64))
    M = M * d[:, None] * d[None, :]
    return (M + M.T) / 2.0


def make(kind, Ne=300, seed=0, extra=0.25):
    """-> dict(cam, level_sigma2, kp_xy [n, 2] float32, kp_octave [n], mp_index [n], points [m, 3] float32, track_depth [m] float32,
    link (the fields of orbfe_imu_link), Rcw, tcw, Rwb, twb, v, bg, ba (the frame's state at the start, float32), truth, kind, Ne)"""
    rot_deg, shift, noise = KINDS[kind]
    rng = np.random.RandomState(9000 * seed + 17 * Ne + len(kind))
    cam = np.array(PINHOLE, np.float32)
    fx, fy, cx, cy = (float(v) for v in cam[:4])
    s2 = level_sigma2()
    f32 = np.float32
    dt = float(f32(0.25))
    g = np.array([0.0, 0.0, -GRAVITY])
    if kind == "zero_depth":
        Rcb, tcb = np.eye(3), np.zeros(3)
        Rwb1, Rwb2 = np.eye(3), np.eye(3)
        twb2 = -np.array([0.25, -0.125, 0.5])   # tcw = -twb: exact
    else:
        Rcb = _rodrigues((0.02, -1.55, 0.03)) @ _rodrigues((0.0, 0.0, 1.57))
        tcb = np.array([0.05, -0.02, 0.01])
        Rwb1 = _rodrigues((0.3, -0.1, 0.8))
        Rwb2 = Rwb1 if kind == "scaled_dR" else Rwb1 @ _rodrigues((0.04, -0.03, 0.06))
        twb2 = np.array([0.6, -0.3, 0.2])
    Rcb, tcb = Rcb.astype(f32).astype(np.float64), tcb.astype(f32).astype(np.float64)
    Rwb1, Rwb2, twb2 = (a.astype(f32).astype(np.float64) for a in (Rwb1, Rwb2, twb2))
    tbc = (-Rcb.T @ tcb).astype(f32).astype(np.float64)
    v1 = np.array([0.4, -0.2, 0.1]).astype(f32).astype(np.float64)
    v2 = (v1 + np.array([0.05, 0.08, -0.03])).astype(f32).astype(np.float64)
    twb1 = (twb2 - v1 * dt - 0.5 * (v2 - v1) * dt).astype(f32).astype(np.float64)
    bg1 = np.array([0.001, -0.002, 0.0015]).astype(f32)
    ba1 = np.array([0.02, -0.01, 0.03]).astype(f32)
    # the preintegrated constants of the truth (EdgeInertial::computeError = 0), plus noise
    imu_noise = 0.0 if kind in ("converged", "zero_depth") else 1.0
    dR = Rwb1.T @ Rwb2 @ _rodrigues(imu_noise * 1e-3 * rng.normal(size=3))
    dV = Rwb1.T @ (v2 - v1 - g * dt) + imu_noise * 2e-3 * rng.normal(size=3)
    dP = Rwb1.T @ (twb2 - twb1 - v1 * dt - g * dt * dt / 2.0) + imu_noise * 1e-3 * rng.normal(size=3)
    if kind == "scaled_dR":
        dR = (1.0 + 1e-6) * np.eye(3)
    info9 = _spd(rng, [3e5] * 3 + [2e3] * 3 + [2e4] * 3, 0.2)
    if kind == "weak_imu":
        info9 = info9 * 1e-6
    if kind == "strong_imu":
        info9 = info9 * 1e6
    infoG, infoA = _spd(rng, [1e7] * 3, 0.1), _spd(rng, [1e4] * 3, 0.1)
    link = dict(Rwb1=Rwb1.astype(f32).reshape(9), twb1=twb1.astype(f32), v1=v1.astype(f32), bg1=bg1, ba1=ba1, dR=dR.astype(f32).reshape(9),
                dV=dV.astype(f32), dP=dP.astype(f32), dt=f32(dt), Rcb=Rcb.astype(f32).reshape(9), tcb=tcb.astype(f32), tbc=tbc.astype(f32),
                info9=info9.reshape(81), infoG=infoG.reshape(9), infoA=infoA.reshape(9))
    # the camera of the truth and the points it sees
    Rt = Rcb @ Rwb2.T
    tt = Rcb @ (-Rwb2.T @ twb2) + tcb
    uv = np.stack([rng.uniform(30, W - 30, Ne), rng.uniform(30, H - 30, Ne)], 1)
    z = rng.uniform(2.0, 18.0, Ne)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(Ne)], 1)
    Xw = ((ray * z[:, None] - tt) @ Rt).astype(f32).astype(np.float64)
    if kind == "behind" and Ne:
        idx = rng.permutation(Ne)[:max(Ne // 5, 1)]
        Xc = Xw[idx] @ Rt.T + tt
        Xc[:, 2] = -Xc[:, 2]
        Xw[idx] = ((Xc - tt) @ Rt).astype(f32)
    if kind == "zero_depth" and Ne:
        Xw[Ne // 2] = (1.0, 0.5, -0.5)   # identity rotation: Xc.z = Z + tz = 0.0 exactly
    Xc = Xw @ Rt.T + tt
    with np.errstate(all="ignore"):
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    uv[~np.isfinite(uv)] = 100.0
    octave = rng.randint(0, N_LEVELS, Ne)
    sig = np.sqrt(s2[octave].astype(np.float64))
    uv = uv + rng.normal(size=(Ne, 2)) * (noise * sig)[:, None]

    def displace(idx, lo, hi):
        ang = rng.uniform(0, 2 * np.pi, len(idx))
        mag = rng.uniform(lo, hi, len(idx)) * sig[idx]
        uv[idx] = uv[idx] + np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)

    if kind == "outliers":
        nOut = int(round(0.3 * Ne))
        idx = rng.permutation(Ne)[:nOut]
        uv[idx] = np.stack([rng.uniform(20, W - 20, nOut), rng.uniform(20, H - 20, nOut)], 1)
        rest = np.setdiff1d(np.arange(Ne), idx)
        displace(rest[rng.permutation(len(rest))[:max(Ne // 6, 1)]], 2.2, 3.6)
    if kind == "close_boundary":
        displace(rng.permutation(Ne)[:max(Ne // 4, 1)], 2.65, 2.75)   # chi2 in (7.0, 7.6): between 5.991 and 1.5 * 5.991
    if kind == "recover":
        displace(rng.permutation(Ne)[:max(Ne // 3, 1)], 4.1, 4.6)    # chi2 in (16.8, 21.2): above every gate, below 24
    e = int(extra * Ne) + 3
    kp = np.concatenate([uv, np.stack([rng.uniform(20, W - 20, e), rng.uniform(20, H - 20, e)], 1)])
    oc = np.concatenate([octave, rng.randint(0, N_LEVELS, e)])
    perm = rng.permutation(len(kp))
    inv = np.argsort(perm)
    pperm = rng.permutation(Ne + 5)
    points = np.zeros((Ne + 5, 3), f32)
    points[pperm[:Ne]] = Xw
    points[pperm[Ne:]] = rng.uniform(-3, 3, (5, 3))
    depth = np.full(Ne + 5, 5.0, f32)
    depth[pperm[:Ne]] = np.abs(Xc[:, 2]).astype(f32)   # mTrackDepth: the distance SearchLocalPoints saw
    mp_index = np.full(len(kp), -1, np.int32)
    mp_index[inv[:Ne]] = pperm[:Ne]
    # the start: the truth moved by the kind's offsets
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    dirn = rng.normal(size=3)
    dirn /= np.linalg.norm(dirn)
    off = 0.0 if kind in ("converged", "zero_depth") else 1.0
    Rwb0 = (Rwb2 @ _rodrigues(np.deg2rad(rot_deg) * axis)).astype(f32).astype(np.float64)
    twb0 = (twb2 + shift * dirn).astype(f32).astype(np.float64)
    v0 = (v2 + off * 0.05 * rng.normal(size=3)).astype(f32)
    bg0 = (bg1 + off * 1e-4 * rng.normal(size=3)).astype(f32)
    ba0 = (ba1 + off * 1e-3 * rng.normal(size=3)).astype(f32)
    Rcw0 = Rcb @ Rwb0.T
    tcw0 = Rcb @ (-Rwb0.T @ twb0) + tcb
    return dict(cam=cam, level_sigma2=s2, kp_xy=kp[perm].astype(f32), kp_octave=oc[perm].astype(np.int32), mp_index=mp_index, points=points,
                track_depth=depth, link=link, Rcw=Rcw0.astype(f32).reshape(9), tcw=tcw0.astype(f32), Rwb=Rwb0.astype(f32).reshape(9),
                twb=twb0.astype(f32), v=v0, bg=bg0, ba=ba0, truth=dict(Rwb=Rwb2, twb=twb2, v=v2), kind=kind, Ne=Ne)


def ref(sc, **kw):
    return R.pose_inertial_optimization(sc["cam"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"],
                                        sc["track_depth"], sc["link"], sc["Rcw"], sc["tcw"], sc["Rwb"], sc["twb"], sc["v"], sc["bg"],
                                        sc["ba"], **kw)


_cache = {}


def ref_cached(case):
    """the restatement's result of a case, computed once per session and shared"""
    if case not in _cache:
        _cache[case] = ref(make_case(case), **case_kw(case))
    return _cache[case]


# (kind, N_e, seed[, rec_init]): the comparison set of tests/test_pose_inertial_gpu.py; every kind, every listed size
CASES = [("few", 0, 0), ("few", 1, 0), ("few", 6, 0), ("few", 7, 0), ("general", 63, 0), ("general", 64, 0), ("general", 65, 0),
         ("general", 257, 0), ("general", 300, 0), ("general", 1000, 0), ("general", 4097, 0),
         ("converged", 64, 0), ("converged", 300, 0), ("far", 65, 0), ("far", 300, 0), ("outliers", 63, 0), ("outliers", 300, 0),
         ("outliers", 1000, 0), ("close_boundary", 257, 0), ("recover", 25, 0), ("recover", 25, 0, 1), ("behind", 64, 0),
         ("behind", 300, 0), ("zero_depth", 7, 0), ("zero_depth", 300, 0), ("weak_imu", 300, 0), ("strong_imu", 300, 0),
         ("scaled_dR", 65, 0), ("outliers", 4097, 0)]
# one case of every kind for the host loop under the sanitizers
HOST_CASES = [("few", 0, 0), ("few", 1, 0), ("few", 6, 0), ("few", 7, 0), ("general", 300, 0), ("converged", 64, 0), ("far", 65, 0),
              ("outliers", 300, 0), ("close_boundary", 257, 0), ("recover", 25, 0), ("recover", 25, 0, 1), ("behind", 64, 0),
              ("zero_depth", 7, 0), ("zero_depth", 300, 0), ("weak_imu", 300, 0), ("strong_imu", 300, 0), ("scaled_dR", 65, 0)]


def case_id(c):
    return "%s-N%d-seed%d" % c[:3] + ("-rec_init" if len(c) > 3 and c[3] else "")


def case_kw(c):
    return dict(rec_init=1) if len(c) > 3 and c[3] else {}


def make_case(c):
    return make(c[0], c[1], c[2])

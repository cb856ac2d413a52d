"""Seeded scenes for the S20 tests (tests/test_pose_inertial_prev*.py).  The geometry -- camera, points, keypoints, the frame's start,
the consistent inertial constants -- is pose_inertial_scenarios.make's; added here are the previous frame as a free state, a
preintegration with non-zero bias Jacobians, and the prior on the previous frame.

kinds:
  general, converged, far, outliers, few, zero_depth, weak_imu    as in pose_inertial_scenarios
  bias_step              the previous frame's bias differs from the preintegration's: dbg and dba are non-zero from iteration 0 (dR0,
                         dV0, dP0 are moved back so that the deltas at the previous bias are still the consistent ones)
  prior_far              the prior's position is 0.2 m from the previous frame's start: its chi2 > 25 and its Huber weight < 1 in
                         round 0 (tests/test_pose_inertial_prev.py asserts it)
  rank_deficient_prior   the prior's H has four zero eigenvalues, as after ConstraintPoseImu's clamp
  threshold              63 edges of which all but 7 (seed 0) or 8 (seed 1) are gross outliers: the return value lands on 7 and on 8,
                         on either side of inlier_threshold
"""
import numpy as np

import pose_inertial_prev_ref as R
import pose_inertial_scenarios as PS19
from mlpnp_scenarios import H, W, _rodrigues

BASE = {"general": "general", "converged": "converged", "far": "far", "outliers": "outliers", "few": "few", "zero_depth": "zero_depth",
        "weak_imu": "weak_imu", "bias_step": "general", "prior_far": "general", "rank_deficient_prior": "general", "threshold": "general"}
KINDS = sorted(BASE)
NE_LIST = [0, 1, 5, 6, 63, 64, 65, 257, 1000, 4097]
f32 = np.float32


def make(kind, Ne=257, seed=0):
    """-> pose_inertial_scenarios.make's dict with link = the fields of orbfe_imu_link_free and prior = those of orbfe_pose_imu_prior"""
    sc = PS19.make(BASE[kind], Ne, seed)
    rng = np.random.RandomState(77000 + 131 * seed + 7 * Ne + len(kind))
    old = sc["link"]
    exact = kind in ("converged", "zero_depth")
    dt = float(old["dt"])
    eye = np.eye(3)
    jit = 0.0 if exact else 1.0
    JRg = -dt * (eye + 0.05 * jit * rng.normal(size=(3, 3)))
    JVa = -dt * (eye + 0.05 * jit * rng.normal(size=(3, 3)))
    JVg = 0.3 * dt * (_rodrigues((0.3, 0.2, -0.1)) + 0.1 * jit * rng.normal(size=(3, 3)))
    JPa = -0.5 * dt * dt * (eye + 0.05 * jit * rng.normal(size=(3, 3)))
    JPg = 0.1 * dt * dt * (_rodrigues((-0.2, 0.1, 0.3)) + 0.1 * jit * rng.normal(size=(3, 3)))
    bg1, ba1 = np.asarray(old["bg1"], np.float64), np.asarray(old["ba1"], np.float64)
    dR0 = np.asarray(old["dR"], np.float64).reshape(3, 3)
    dV0, dP0 = np.asarray(old["dV"], np.float64), np.asarray(old["dP"], np.float64)
    bg0, ba0 = bg1.copy(), ba1.copy()
    if kind == "bias_step":
        dbg, dba = np.array([2e-3, -1e-3, 1.5e-3]), np.array([0.02, 0.01, -0.015])
        bg0, ba0 = bg1 - dbg, ba1 - dba
        dR0 = dR0 @ _rodrigues(-(JRg @ dbg))
        dV0 = dV0 - JVg @ dbg - JVa @ dba
        dP0 = dP0 - JPg @ dbg - JPa @ dba
    # the previous frame's start: the truth moved a little (it is free now)
    move = 0.0 if exact else 1.0
    Rwb1 = np.asarray(old["Rwb1"], np.float64).reshape(3, 3) @ _rodrigues(move * 2e-3 * rng.normal(size=3))
    twb1 = np.asarray(old["twb1"], np.float64) + move * 5e-3 * rng.normal(size=3)
    v1 = np.asarray(old["v1"], np.float64) + move * 1e-2 * rng.normal(size=3)
    link = dict(Rwb1=Rwb1.astype(f32).reshape(9), twb1=twb1.astype(f32), v1=v1.astype(f32), bg1=bg1.astype(f32), ba1=ba1.astype(f32),
                dR0=dR0.astype(f32).reshape(9), dV0=dV0.astype(f32), dP0=dP0.astype(f32), bg0=bg0.astype(f32), ba0=ba0.astype(f32),
                JRg=JRg.astype(f32).reshape(9), JVg=JVg.astype(f32).reshape(9), JVa=JVa.astype(f32).reshape(9),
                JPg=JPg.astype(f32).reshape(9), JPa=JPa.astype(f32).reshape(9), dt=old["dt"], Rcb=old["Rcb"], tcb=old["tcb"],
                tbc=old["tbc"], info9=old["info9"], infoG=old["infoG"], infoA=old["infoA"])
    # the prior: centred near the previous frame's true state
    Hp = PS19._spd(rng, [2e4] * 3 + [1e4] * 3 + [2e3] * 3 + [1e6] * 3 + [1e4] * 3, 0.2)
    if kind == "rank_deficient_prior":
        lam, Q = np.linalg.eigh(Hp)
        lam[:4] = 0.0
        Hp = (Q * lam[None, :]) @ Q.T
        Hp = (Hp + Hp.T) / 2.0
    pn = 0.0 if exact else 1.0
    pR = np.asarray(old["Rwb1"], np.float64).reshape(3, 3) @ _rodrigues(pn * 1e-3 * rng.normal(size=3))
    pt = np.asarray(old["twb1"], np.float64) + pn * 3e-3 * rng.normal(size=3)
    if kind == "prior_far":
        pt = pt + np.array([0.2, 0.0, 0.0])
    prior = dict(Rwb=pR.reshape(9), twb=pt, vwb=np.asarray(old["v1"], np.float64) + pn * 5e-3 * rng.normal(size=3),
                 bg=bg1 + pn * 1e-5 * rng.normal(size=3), ba=ba1 + pn * 1e-4 * rng.normal(size=3), H=Hp.reshape(225))
    sc = dict(sc)
    sc["link"], sc["prior"], sc["kind"] = link, prior, kind
    if kind == "threshold" and Ne:
        keep = 7 + seed
        edges = np.flatnonzero(sc["mp_index"] >= 0)
        gross = edges[rng.permutation(len(edges))[keep:]]
        xy = sc["kp_xy"].copy()
        xy[gross] = np.stack([rng.uniform(20, W - 20, len(gross)), rng.uniform(20, H - 20, len(gross))], 1).astype(f32)
        sc["kp_xy"] = xy
    return sc


def ref(sc, **kw):
    return R.pose_inertial_optimization_last_frame(sc["cam"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"],
                                                   sc["track_depth"], sc["link"], sc["prior"], sc["Rcw"], sc["tcw"], sc["Rwb"], sc["twb"],
                                                   sc["v"], sc["bg"], sc["ba"], **kw)


_cache = {}


def ref_cached(case):
    """the restatement's result of a case, computed once per session and shared"""
    if case not in _cache:
        _cache[case] = ref(make_case(case), **case_kw(case))
    return _cache[case]


# (kind, N_e, seed[, rec_init]): the comparison set of tests/test_pose_inertial_prev_gpu.py; every kind, every listed size
CASES = [("few", 0, 0), ("few", 1, 0), ("few", 5, 0), ("few", 6, 0), ("general", 63, 0), ("general", 64, 0), ("general", 65, 0),
         ("general", 257, 0), ("general", 1000, 0), ("general", 4097, 0), ("converged", 64, 0), ("far", 65, 0), ("outliers", 257, 0),
         ("outliers", 1000, 0), ("zero_depth", 6, 0), ("zero_depth", 257, 0), ("bias_step", 257, 0), ("prior_far", 65, 0),
         ("prior_far", 65, 0, 1), ("rank_deficient_prior", 64, 0), ("weak_imu", 257, 0), ("threshold", 63, 0), ("threshold", 63, 1)]
# one case of every kind for the host loop under the sanitizers
HOST_CASES = [("few", 0, 0), ("few", 1, 0), ("few", 5, 0), ("few", 6, 0), ("general", 257, 0), ("converged", 64, 0), ("far", 65, 0),
              ("outliers", 257, 0), ("zero_depth", 6, 0), ("zero_depth", 257, 0), ("bias_step", 257, 0), ("prior_far", 65, 0),
              ("rank_deficient_prior", 64, 0), ("weak_imu", 257, 0), ("threshold", 63, 0), ("threshold", 63, 1)]


def case_id(c):
    return "%s-N%d-seed%d" % c[:3] + ("-rec_init" if len(c) > 3 and c[3] else "")


def case_kw(c):
    return dict(rec_init=1) if len(c) > 3 and c[3] else {}


def make_case(c):
    return make(c[0], c[1], c[2])

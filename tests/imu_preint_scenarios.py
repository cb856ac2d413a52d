"""Seeded scenes for the S22 tests (tests/test_imu_preint*.py): a smooth body trajectory, an IMU with EuRoC-like noise
(ng = 1.7e-4 sqrt(f), na = 2e-3 sqrt(f), ngw = 1.9393e-5 / sqrt(f), naw = 3e-3 / sqrt(f), f = 200, as src/Tracking.cc:116-123 scales
them) sampled every 5 ms, and frame stamps that fall between samples.  The key frame lies `pre` steps before the previous frame, so
the key-frame record already holds those steps when the frame's window is integrated.

kinds:
  moving         rotation up to 0.4 rad/s, accelerations of about 1 m/s^2: IntegratedRotation's general branch
  still          no motion: |w - b| dt < 1e-4 on every step, the small-angle branch
  bias_changed   the key-frame record stands at a bias that differs from the key frame's b1 (as after SetNewBias without a
                 reintegration): GetDelta* and the bias Jacobians matter
  long_kf        the key-frame record already holds 400 steps: the drift NormalizeRotation bounds
  clamped        a constructed key-frame record: C(8,8) raised by 2e12, so the information has an eigenvalue below 1e-12
  not_positive   a constructed key-frame record: C.block<3,3>(0,0) = -1e-6 I, so the first pivot is negative and info_ok = 0
"""
import numpy as np

import imu_preint_ref as R
from mlpnp_scenarios import H, N_LEVELS, PINHOLE, W, _rodrigues, level_sigma2

f32, f64 = np.float32, np.float64
DT = 0.005
T0 = 1403636580.0
GRAVITY = f32(9.81)
NATURAL = ("moving", "still", "bias_changed", "long_kf")
KINDS = NATURAL + ("clamped", "not_positive")
STEPS = (1, 2, 3, 10, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1)
# (kind, steps, seed): every step count for `moving`, the other kinds at the counts that reach their branch
CASES = [("moving", n, 0) for n in STEPS] + [("still", 3, 0), ("still", 10, 0), ("bias_changed", 2, 0), ("bias_changed", 10, 0),
                                              ("long_kf", 10, 0), ("clamped", 3, 0), ("not_positive", 3, 0), ("moving", 10, 1)]
HOST_CASES = [("moving", 1, 0), ("moving", 3, 0), ("moving", R.CHUNK + 1, 0), ("still", 3, 0), ("bias_changed", 10, 0), ("long_kf", 10, 0),
              ("clamped", 3, 0), ("not_positive", 3, 0)]


def case_id(c):
    return "%s-n%d-seed%d" % c


class Trajectory:
    """R(t) = Exp(theta(t) axis) about a fixed axis, p(t) a sum of sines: velocity, acceleration and body rate in closed form"""

    def __init__(self, rng, still):
        self.still = still
        ax = rng.normal(size=3)
        self.axis = ax / np.linalg.norm(ax)
        self.R0 = _rodrigues((0.3, -0.1, 0.8))
        self.ph = rng.uniform(0, 2 * np.pi, 4)
        self.amp = np.array([1.0, 0.8, 0.3])
        self.om = np.array([0.7, 0.5, 0.9])

    def theta(self, t):
        return 0.0 if self.still else 0.3 * np.sin(1.3 * t + self.ph[3])

    def rate(self, t):
        return np.zeros(3) if self.still else 0.39 * np.cos(1.3 * t + self.ph[3]) * self.axis

    def Rwb(self, t):
        return self.R0 @ _rodrigues(self.theta(t) * self.axis)

    def p(self, t):
        return np.array([0.6, -0.3, 0.2]) if self.still else self.amp * np.sin(self.om * t + self.ph[:3])

    def v(self, t):
        return np.zeros(3) if self.still else self.amp * self.om * np.cos(self.om * t + self.ph[:3])

    def acc(self, t):
        return np.zeros(3) if self.still else -self.amp * self.om * self.om * np.sin(self.om * t + self.ph[:3])

    def state(self, t, bias):
        """Rwb (9) twb v bg ba as floats"""
        return np.concatenate([self.Rwb(t).reshape(9), self.p(t), self.v(t), bias]).astype(f32)


def _window(rng, traj, k0, n, b_true, noisy=True):
    """n steps == n + 1 samples k0 .. k0 + n of the 5 ms grid; the stamps 2 ms before the first and 3 ms before the last sample"""
    ks = np.arange(k0, k0 + n + 1)
    rel = ks * DT
    g = np.array([0.0, 0.0, -float(GRAVITY)])
    sf = np.sqrt(200.0)
    w = np.stack([traj.rate(t) for t in rel]) + b_true[:3] + noisy * 1.7e-4 * sf * rng.normal(size=(n + 1, 3))
    a = np.stack([traj.Rwb(t).T @ (traj.acc(t) - g) for t in rel]) + b_true[3:] + noisy * 2e-3 * sf * rng.normal(size=(n + 1, 3))
    return dict(t=(T0 + rel).astype(f64), a=a.astype(f32), w=w.astype(f32), t_prev=T0 + rel[0] - 0.002, t_cur=T0 + rel[-1] - 0.003,
                rel_prev=rel[0] - 0.002, rel_cur=rel[-1] - 0.003)


_kf_cache = {}


def make(kind, n, seed, F=f32, noisy=True):
    """-> dict(noise, t, a, w, t_prev, t_cur (the frame's window), frame_bias [6], kf (the key-frame record before the window), state_kf /
    state_frame (the start states of either branch), gravity, Rcb, tcb, tbc, traj, rel_kf / rel_prev / rel_cur, kind, n, seed)"""
    key = (kind, n, seed, F, noisy)
    rng = np.random.RandomState(2200 + 97 * seed + len(kind))
    traj = Trajectory(rng, kind == "still")
    b_true = np.concatenate([0.01 * rng.normal(size=3), 0.05 * rng.normal(size=3)])
    b1 = b_true.astype(f32)                                  # the key frame's and the last frame's bias
    b_kf = b1.copy()
    if kind == "bias_changed":
        b_kf = (b_true + np.array([2e-3, -1e-3, 1.5e-3, 0.02, 0.01, -0.015])).astype(f32)
    pre = 400 if kind == "long_kf" else 5
    noise = R.Noise(F=F)
    k0 = 40
    pre_w = _window(rng, traj, k0, pre, b_true, noisy)
    win = _window(rng, traj, k0 + pre, n, b_true, noisy)
    ckey = (kind, seed, F, noisy)                             # the record before the window does not depend on n
    if ckey not in _kf_cache:
        kf, _, _ = R.preintegrate_frame(noise, pre_w["t"], pre_w["a"], pre_w["w"], pre_w["t_prev"], pre_w["t_cur"], b_kf, R.Record(b_kf, F),
                                        counts=R.collections.Counter())
        _kf_cache[ckey] = kf
    kf = _kf_cache[ckey].copy()
    if kind == "clamped":
        kf.C[8, 8] = kf.C[8, 8] + F(2e12)
    if kind == "not_positive":
        kf.C[0:3, 0:3] = -F(1e-6) * np.eye(3, dtype=F)
    Rcb = (_rodrigues((0.02, -1.55, 0.03)) @ _rodrigues((0.0, 0.0, 1.57))).astype(f32)
    tcb = np.array([0.05, -0.02, 0.01], f32)
    tbc = (-Rcb.astype(f64).T @ tcb.astype(f64)).astype(f32)
    sc = dict(win)
    sc.update(noise=noise, frame_bias=b1, kf=kf, state_kf=traj.state(pre_w["rel_prev"], b1), state_frame=traj.state(win["rel_prev"], b1),
              gravity=GRAVITY, Rcb=Rcb, tcb=tcb, tbc=tbc, traj=traj, rel_kf=pre_w["rel_prev"], kind=kind, n=n, seed=seed, key=key)
    return sc


_cache = {}


def ref_cached(case, which):
    """the restatement's outputs for a case, computed once per session and shared: dict(kf, frame, steps, state, link, ok)"""
    k = (case, which)
    if k not in _cache:
        sc = make(*case)
        kf, fr, steps = R.preintegrate_frame(sc["noise"], sc["t"], sc["a"], sc["w"], sc["t_prev"], sc["t_cur"], sc["frame_bias"], sc["kf"])
        s1 = sc["state_frame"] if which == R.FROM_FRAME else sc["state_kf"]
        state, link, ok = R.predict(which, s1, kf, fr, sc["gravity"], sc["Rcb"], sc["tcb"], sc["tbc"])
        _cache[k] = dict(kf=kf, frame=fr, steps=steps, state=state, link=link, ok=ok, state1=s1)
    return _cache[k]


def visual_edges(sc, Ne, seed, noise_px=0.5):
    """keypoints and map points seen from the true camera at the frame's stamp, every keypoint matched, in the argument layout of
    pose_inertial_ref / pose_inertial_prev_ref -> dict(cam, level_sigma2, kp_xy, kp_octave, mp_index, points, track_depth, truth)"""
    rng = np.random.RandomState(5100 + seed)
    traj = sc["traj"]
    t = sc["rel_cur"]
    Rwb, twb = traj.Rwb(t), traj.p(t)
    Rcb, tcb = sc["Rcb"].astype(f64), sc["tcb"].astype(f64)
    Rt = Rcb @ Rwb.T
    tt = Rcb @ (-Rwb.T @ twb) + tcb
    cam = np.array(PINHOLE, f32)
    fx, fy, cx, cy = (float(v) for v in cam[:4])
    uv = np.stack([rng.uniform(30, W - 30, Ne), rng.uniform(30, H - 30, Ne)], 1)
    z = rng.uniform(2.0, 18.0, Ne)
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(Ne)], 1)
    Xw = ((ray * z[:, None] - tt) @ Rt).astype(f32)
    Xc = Xw.astype(f64) @ Rt.T + tt
    uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    s2 = level_sigma2()
    octave = rng.randint(0, N_LEVELS, Ne)
    uv = uv + rng.normal(size=(Ne, 2)) * (noise_px * np.sqrt(s2[octave].astype(f64)))[:, None]
    return dict(cam=cam, level_sigma2=s2, kp_xy=uv.astype(f32), kp_octave=octave.astype(np.int32), mp_index=np.arange(Ne, dtype=np.int32),
                points=Xw, track_depth=np.abs(Xc[:, 2]).astype(f32), truth=dict(Rwb=Rwb, twb=twb, v=traj.v(t)))

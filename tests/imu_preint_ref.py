"""SPEC DECISION S22, normative: Tracking::PreintegrateIMU (src/Tracking.cc:234-290), IMU::Preintegrated
(src/ImuTypes.cc:36-39, 86-107, 149-237, 285-312), Tracking::PredictStateIMU (src/Tracking.cc:293-350), Frame::SetImuPoseVelocity
(src/Frame.cc:221-238) and the informations of the inertial links (src/G2oTypes.cc:500-508; src/Optimizer.cc:3645, 3652, 4046, 4053),
written from those lines and the text of S22, not from the kernel.

Rules as S14 / S19: the working type F (binary32 in the spec) where the C++ is float, binary64 where it is double; one IEEE operation
per operator, left to right; a 3-term dot product is (a0 b0 + a1 b1) + a2 b2; a structural zero block is never multiplied.  Matrices
are [3, 3] / [9, 9] / [15, 15] arrays here and row-major in the C structs.

Stated departures from the reference: NormalizeRotation is the polar factor through jacobi3 on A^T A in binary64; sin / cos of
IntegratedRotation are (F) of S13's binary64 sequences; the rotation at a new bias is S20's dR ExpSO3(JRg dbg) in binary64, rounded,
normalised; the covariance is inverted by L D L^T without pivoting of its upper triangle; the eigen-decomposition is S12's n = 9
Jacobi sequence.

The `literal_*` functions are the INDEPENDENT form: a plain numpy rendering of the same reference lines with numpy.linalg.svd,
numpy.linalg.inv, numpy.linalg.eigh, libm sin / cos and numpy's own matrix products.
"""
import collections

import numpy as np

import pose_inertial_ref as R19
import twoview_ref as R12
from initial_ba_ref import inv3_sym
from mlpnp_ref import sincos64

f64 = np.float64
f32 = np.float32
COUNTS = collections.Counter()   # which branches ran (tests/test_imu_preint.py asserts that the scenes reach them); no effect on results
CHUNK = 32                       # the kernel's staging chunk (csrc/imu_preint_math.h kPreintChunk): the scenes straddle it
FROM_KEYFRAME, FROM_FRAME = 0, 1
EPS = f32(1e-4)                  # ImuTypes.cc:34: const float eps = 1e-4
CLAMP = 1e-12                    # G2oTypes.cc:505
REC_FIELDS = (("dT", 1), ("bg", 3), ("ba", 3), ("dR", 9), ("dV", 3), ("dP", 3), ("JRg", 9), ("JVg", 9), ("JVa", 9), ("JPg", 9),
              ("JPa", 9), ("avgA", 3), ("avgW", 3), ("C", 225))


class Record:
    """IMU::Preintegrated without its measurement list"""

    def __init__(self, bias, F=f32):
        """Initialize(b) (ImuTypes.cc:149-168); bias = bwx bwy bwz bax bay baz"""
        bias = np.asarray(bias, F).reshape(6)
        self.F = F
        self.n_steps = 0
        self.dT = F(0)
        self.bg, self.ba = bias[:3].copy(), bias[3:].copy()
        self.dR = np.eye(3, dtype=F)
        self.dV, self.dP = np.zeros(3, F), np.zeros(3, F)
        self.JRg, self.JVg, self.JVa, self.JPg, self.JPa = (np.zeros((3, 3), F) for _ in range(5))
        self.avgA, self.avgW = np.zeros(3, F), np.zeros(3, F)
        self.C = np.zeros((15, 15), F)

    def copy(self):
        o = Record(np.zeros(6), self.F)
        o.n_steps = self.n_steps
        o.dT = self.dT
        for k, n in REC_FIELDS[1:]:
            setattr(o, k, getattr(self, k).copy())
        return o

    def floats(self):
        """the 298 floats of orbfe_imu_preint from dT to C"""
        return np.concatenate([np.asarray(getattr(self, k), self.F).reshape(-1) for k, _ in REC_FIELDS])

    @staticmethod
    def from_floats(v, n_steps, F=f32):
        v = np.asarray(v, F).reshape(298)
        o = Record(np.zeros(6), F)
        o.n_steps = int(n_steps)
        at = 0
        for k, n in REC_FIELDS:
            x = v[at:at + n].copy()
            at += n
            setattr(o, k, x[0] if k == "dT" else (x.reshape(3, 3) if n == 9 else (x.reshape(15, 15) if n == 225 else x)))
        return o


class Noise:
    """the diagonals of Calib::Cov and Calib::CovWalk, scaled as Tracking.cc:116-123 does"""

    def __init__(self, ng=1.7e-4, na=2e-3, ngw=1.9393e-5, naw=3e-3, freq=200.0, F=f32):
        sf = np.sqrt(f32(freq))   # const float sf = sqrt(mImuFreq)
        ng, na, ngw, naw = f32(f32(ng) * sf), f32(f32(na) * sf), f32(f32(ngw) / sf), f32(f32(naw) / sf)
        self.cov = np.array([ng * ng] * 3 + [na * na] * 3, f32).astype(F)
        self.walk = np.array([ngw * ngw] * 3 + [naw * naw] * 3, f32).astype(F)


def hat(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], v.dtype)


def mv(M, x):
    """(m_i0 x_0 + m_i1 x_1) + m_i2 x_2"""
    with np.errstate(all="ignore"):
        return (M[:, 0] * x[0] + M[:, 1] * x[1]) + M[:, 2] * x[2]


def mul3(A, B):
    with np.errstate(all="ignore"):
        return R12.mul3(A, B)


def normalize_rotation(A):
    """NormalizeRotation (ImuTypes.cc:36-39) as the polar factor: G = A^T A in binary64, (V, lambda) = jacobi3(G), P = V diag(1 /
    sqrt(lambda)) V^T as (v_ik s_k) v_jk summed as a 3-term dot product, R = (F)(A P)"""
    F = A.dtype.type
    Ad = A.astype(f64)
    with np.errstate(all="ignore"):
        G = np.zeros((3, 3), f64)
        for i in range(3):
            for j in range(3):
                G[i, j] = (Ad[0, i] * Ad[0, j] + Ad[1, i] * Ad[1, j]) + Ad[2, i] * Ad[2, j]
        M, V = R12.jacobi_cyclic(G[None], R12.SWEEPS)
        M, V = M[0], V[0]
        s = np.array([1.0 / np.sqrt(M[k, k]) for k in range(3)], f64)
        P = np.zeros((3, 3), f64)
        for i in range(3):
            for j in range(3):
                P[i, j] = ((V[i, 0] * s[0]) * V[j, 0] + (V[i, 1] * s[1]) * V[j, 1]) + (V[i, 2] * s[2]) * V[j, 2]
        return mul3(Ad, P).astype(F)


def integrated_rotation(v, counts=COUNTS):
    """IntegratedRotation (ImuTypes.cc:86-107) of v = (w - bg) dt -> (deltaR, rightJ)"""
    F = v.dtype.type
    I = np.eye(3, dtype=F)
    with np.errstate(all="ignore"):
        d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        d = np.sqrt(d2)
        W = hat(v)
        if d < F(EPS):
            counts["rot_small"] += 1
            return I + W, I.copy()
        counts["rot_general"] += 1
        W2 = mul3(W, W)
        s64, c64 = sincos64(f64(d))
        s, c = F(s64), F(c64)
        one = F(1)
        dR = (I + W * s / d) + W2 * (one - c) / d2
        rJ = (I - W * (one - c) / d2) + W2 * (d - s) / (d2 * d)
    assert dR.dtype == F and rJ.dtype == F
    return dR, rJ


def steps_from_samples(t, a, w, t_prev, t_cur, F=f32, counts=COUNTS):
    """the loop head of PreintegrateIMU (Tracking.cc:242-277): samples (t [n + 1] binary64, a / w [n + 1, 3]) -> steps [n, 8]
    (a, w, dt, 0).  Time differences are taken in binary64 and rounded to F."""
    t = np.asarray(t, f64)
    a, w = np.asarray(a, F), np.asarray(w, F)
    n = len(t) - 1
    out = np.zeros((max(n, 0), 8), F)
    half = F(0.5)
    with np.errstate(all="ignore"):
        for i in range(n):
            if i == 0 and i < n - 1:
                counts["step_first"] += 1
                tab, tini = F(t[i + 1] - t[i]), F(t[i] - f64(t_prev))
                r = tini / tab
                acc = ((a[i] + a[i + 1]) - (a[i + 1] - a[i]) * r) * half
                ang = ((w[i] + w[i + 1]) - (w[i + 1] - w[i]) * r) * half
                dt = F(t[i + 1] - f64(t_prev))
            elif i < n - 1:
                counts["step_middle"] += 1
                acc = (a[i] + a[i + 1]) * half
                ang = (w[i] + w[i + 1]) * half
                dt = F(t[i + 1] - t[i])
            elif i > 0 and i == n - 1:
                counts["step_last"] += 1
                tab, tend = F(t[i + 1] - t[i]), F(t[i + 1] - f64(t_cur))
                r = tend / tab
                acc = ((a[i] + a[i + 1]) - (a[i + 1] - a[i]) * r) * half
                ang = ((w[i] + w[i + 1]) - (w[i + 1] - w[i]) * r) * half
                dt = F(f64(t_cur) - t[i])
            else:
                counts["step_single"] += 1
                acc, ang = a[i], w[i]
                dt = F(f64(t_cur) - f64(t_prev))
            out[i, 0:3], out[i, 3:6], out[i, 6] = acc, ang, dt
    return out


def covariance_step(C9, A, B, cov):
    """A C A^T + B Nga B^T by 3 x 3 blocks.  A is block lower triangular (blocks bk <= bi), B has the blocks (0,0), (1,1), (2,1).
    T = A C: for a row block bi the block columns bk = 0 .. bi in turn, each a 3-term dot product, added left to right.  U = T A^T: for
    a column block bj the blocks bk = 0 .. bj the same way.  B Nga B^T exists where both rows share a block column of B (bk = 0 for rows
    0-2, bk = 1 for rows 3-8): ((B_ik n_k) B_jk) as a 3-term dot product, added to U last."""
    F = C9.dtype.type
    with np.errstate(all="ignore"):
        T = np.zeros((9, 9), F)
        for bi in range(3):
            rows = slice(3 * bi, 3 * bi + 3)
            acc = None
            for bk in range(bi + 1):
                k = 3 * bk
                term = (A[rows, k:k + 1] * C9[k:k + 1, :] + A[rows, k + 1:k + 2] * C9[k + 1:k + 2, :]) + A[rows, k + 2:k + 3] * C9[k + 2:k + 3, :]
                acc = term if acc is None else acc + term
            T[rows, :] = acc
        U = np.zeros((9, 9), F)
        for bj in range(3):
            cols = slice(3 * bj, 3 * bj + 3)
            acc = None
            for bk in range(bj + 1):
                k = 3 * bk
                term = (T[:, k:k + 1] * A[cols, k][None, :] + T[:, k + 1:k + 2] * A[cols, k + 1][None, :]) + T[:, k + 2:k + 3] * A[cols, k + 2][None, :]
                acc = term if acc is None else acc + term
            U[:, cols] = acc
        for rows, k in ((slice(0, 3), 0), (slice(3, 9), 3)):
            Bn = B[rows, k:k + 3] * cov[None, k:k + 3]
            Q = (Bn[:, 0:1] * B[rows, k][None, :] + Bn[:, 1:2] * B[rows, k + 1][None, :]) + Bn[:, 2:3] * B[rows, k + 2][None, :]
            U[rows, rows] = U[rows, rows] + Q
    assert T.dtype == F and U.dtype == F
    return U


def integrate(R, step, noise, counts=COUNTS):
    """IntegrateNewMeasurement (ImuTypes.cc:179-237), in place, in the reference's order"""
    F = R.F
    half, one = F(0.5), F(1)
    step = np.asarray(step, F)
    dt = step[6]
    with np.errstate(all="ignore"):
        acc = step[0:3] - R.ba
        accW = step[3:6] - R.bg
        dR = R.dR.copy()
        Ra = mv(dR, acc)
        dTn = R.dT + dt
        R.avgA = (R.dT * R.avgA + Ra * dt) / dTn
        R.avgW = (R.dT * R.avgW + accW * dt) / dTn
        hdR = half * dR
        R.dP = (R.dP + R.dV * dt) + mv(hdR, acc) * dt * dt
        R.dV = R.dV + Ra * dt
        Wacc = hat(acc)
        dRdt = dR * dt
        hh = hdR * dt * dt
        A = np.eye(9, dtype=F)
        B = np.zeros((9, 6), F)
        A[3:6, 0:3] = mul3(-dR * dt, Wacc)
        A[6:9, 0:3] = mul3(-half * dR * dt * dt, Wacc)
        A[6:9, 3:6] = np.diag(np.array([dt, dt, dt], F))
        B[3:6, 3:6] = dRdt
        B[6:9, 3:6] = hh
        JRg = R.JRg.copy()
        R.JPa = (R.JPa + R.JVa * dt) - hh
        R.JPg = (R.JPg + R.JVg * dt) - mul3(mul3(hh, Wacc), JRg)
        R.JVa = R.JVa - dRdt
        R.JVg = R.JVg - mul3(mul3(dRdt, Wacc), JRg)
        dRi, rJ = integrated_rotation(accW * dt, counts)
        R.dR = normalize_rotation(mul3(dR, dRi))
        A[0:3, 0:3] = dRi.T
        B[0:3, 0:3] = rJ * dt
        R.C[0:9, 0:9] = covariance_step(R.C[0:9, 0:9].copy(), A, B, noise.cov)
        for k in range(6):
            R.C[9 + k, 9 + k] = R.C[9 + k, 9 + k] + noise.walk[k]
        R.JRg = mul3(np.ascontiguousarray(dRi.T), JRg) - rJ * dt
        R.dT = dTn
    R.n_steps += 1
    for k, _ in REC_FIELDS:
        assert np.asarray(getattr(R, k)).dtype == F, k
    assert one.dtype == F


def reintegrate(noise, bias, steps, F=f32, counts=COUNTS):
    """Initialize(bias) and the loop over a step list: Reintegrate (ImuTypes.cc:170-177), MergePrevious (:239-264) with the two lists
    concatenated"""
    R = Record(bias, F)
    for s in np.asarray(steps, F).reshape(-1, 8):
        integrate(R, s, noise, counts)
    return R


def preintegrate_frame(noise, t, a, w, t_prev, t_cur, frame_bias, kf, counts=COUNTS):
    """PreintegrateIMU for a selected sample list -> (kf record, frame record or None, steps).  Fewer than 2 samples: nothing changes
    (Tracking.cc:235-238)."""
    F = kf.F
    if len(t) < 2:
        return kf, None, np.zeros((0, 8), F)
    steps = steps_from_samples(t, a, w, t_prev, t_cur, F, counts)
    kf = kf.copy()
    fr = Record(frame_bias, F)
    for s in steps:
        integrate(kf, s, noise, counts)
        integrate(fr, s, noise, counts)
    return kf, fr, steps


def deltas(R, bg, ba, counts=COUNTS):
    """GetDeltaRotation / Velocity / Position (ImuTypes.cc:285-312) at the bias (bg, ba)"""
    F = R.F
    with np.errstate(all="ignore"):
        dbg = np.asarray(bg, F) - R.bg
        dba = np.asarray(ba, F) - R.ba
        dV = (R.dV + mv(R.JVg, dbg)) + mv(R.JVa, dba)
        dP = (R.dP + mv(R.JPg, dbg)) + mv(R.JPa, dba)
        rot = mv(R.JRg, dbg)
        E = R19.exp_so3(rot.astype(f64), counts).reshape(3, 3)
        dR = normalize_rotation(mul3(R.dR.astype(f64), E).astype(F))
    assert dV.dtype == F and dP.dtype == F and rot.dtype == F
    return dR, dV, dP


def predict_state(s1, dRb, dVb, dPb, t12, gravity, Rcb, tcb):
    """PredictStateIMU (Tracking.cc:303-316 == :328-340) and SetImuPoseVelocity (Frame.cc:221-238): s1 = Rwb1 (9) twb1 v1 bg1 ba1 ->
    the 33 floats Rcw tcw Rwb twb v bg ba"""
    F = dRb.dtype.type
    s1 = np.asarray(s1, F).reshape(21)
    Rwb1, twb1, v1 = s1[0:9].reshape(3, 3), s1[9:12], s1[12:15]
    half = F(0.5)
    g = np.array([0, 0, -F(gravity)], F)
    with np.errstate(all="ignore"):
        Rwb2 = normalize_rotation(mul3(Rwb1, dRb))
        twb2 = ((twb1 + v1 * t12) + half * t12 * t12 * g) + mv(Rwb1, dPb)
        v2 = (v1 + t12 * g) + mv(Rwb1, dVb)
        Rbw2 = np.ascontiguousarray(Rwb2.T)
        Rcw = mul3(Rcb, Rbw2)
        tcw = mv(Rcb, -mv(Rbw2, twb2)) + tcb
    out = np.concatenate([Rcw.reshape(9), tcw, Rwb2.reshape(9), twb2, v2, s1[15:18], s1[18:21]])
    assert out.dtype == F
    return out


def ldlt_inverse9(M):
    """the inverse of the symmetric 9 x 9 given by M's upper triangle: L D L^T without pivoting, then the nine unit vectors.
    -> (X [9, 9], every pivot > 0)"""
    N = 9
    A = np.zeros((N, N), f64)
    for i in range(N):
        for j in range(N):
            A[i, j] = M[min(i, j), max(i, j)]
    L = np.zeros((N, N), f64)
    with np.errstate(all="ignore"):
        for k in range(N - 1):
            dk = A[k, k]
            col = A[:, k].copy()
            for i in range(k + 1, N):
                li = f64(0.0) if dk == 0.0 else col[i] / dk
                L[i, k] = li
                for j in range(k + 1, i + 1):
                    A[i, j] = A[i, j] - li * col[j]
        d = np.array([A[k, k] for k in range(N)], f64)
        X = np.zeros((N, N), f64)
        for c in range(N):
            z = np.zeros(N, f64)
            for i in range(N):
                acc = f64(1.0 if i == c else 0.0)
                for j in range(i):
                    acc = acc - L[i, j] * z[j]
                z[i] = acc
            for i in range(N):
                z[i] = f64(0.0) if d[i] == 0.0 else z[i] / d[i]
            for i in range(N - 1, -1, -1):
                acc = z[i]
                for j in range(i + 1, N):
                    acc = acc - L[j, i] * z[j]
                z[i] = acc
            X[:, c] = z
    return X, bool(np.all(d > 0.0))


def info9(C, counts=COUNTS):
    """EdgeInertial's information (G2oTypes.cc:500-508) of C.block<9,9>(0,0) -> (info [81] binary64, info_ok)"""
    X, ok = ldlt_inverse9(np.asarray(C)[0:9, 0:9].astype(f64))
    if not ok:
        counts["not_positive"] += 1
    with np.errstate(all="ignore"):
        S = (X + X.T) / 2.0
        M, V = R12.jacobi_rounds9(S[None])
        M, V = M[0], V[0]
        lam = np.array([M[k, k] for k in range(9)], f64)
        counts["clamped"] += int((lam < CLAMP).sum())
        lam = np.where(lam < CLAMP, 0.0, lam)
        out = np.zeros((9, 9), f64)
        for k in range(9):
            term = (V[:, k:k + 1] * lam[k]) * V[:, k][None, :]
            out = term if k == 0 else out + term
    return out.reshape(81), ok


def info3(C, at):
    """C.block<3,3>(at, at).cast<double>().inverse() (Optimizer.cc:3645, 3652, 4046, 4053): S17's inv3_sym of the upper triangle"""
    b = np.asarray(C)[at:at + 3, at:at + 3].astype(f64)
    with np.errstate(all="ignore"):
        s = inv3_sym(np.array([b[0, 0], b[0, 1], b[0, 2], b[1, 1], b[1, 2], b[2, 2]], f64))
    return np.array([s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]], f64)


def predict(which, s1, kf, frame, gravity, Rcb, tcb, tbc, counts=COUNTS):
    """-> (state [33], link dict, info_ok).  FROM_KEYFRAME: prediction and link from the key-frame record, the link an orbfe_imu_link
    with GetDelta*(b1).  FROM_FRAME: from the frame record, an orbfe_imu_link_free with the raw deltas; infoG / infoA are the
    key-frame record's either way (Optimizer.cc:4046)."""
    R = frame if which == FROM_FRAME else kf
    F = R.F
    s1 = np.asarray(s1, F).reshape(21)
    Rcb, tcb, tbc = np.asarray(Rcb, F).reshape(3, 3), np.asarray(tcb, F).reshape(3), np.asarray(tbc, F).reshape(3)
    info, ok = info9(R.C, counts)
    dRb, dVb, dPb = deltas(R, s1[15:18], s1[18:21], counts)
    state = predict_state(s1, dRb, dVb, dPb, R.dT, gravity, Rcb, tcb)
    link = dict(Rwb1=s1[0:9], twb1=s1[9:12], v1=s1[12:15], bg1=s1[15:18], ba1=s1[18:21], dt=R.dT, Rcb=Rcb.reshape(9), tcb=tcb, tbc=tbc,
                info9=info, infoG=info3(kf.C, 9), infoA=info3(kf.C, 12))
    if which == FROM_FRAME:
        link.update(dR0=R.dR.reshape(9), dV0=R.dV, dP0=R.dP, bg0=R.bg, ba0=R.ba, JRg=R.JRg.reshape(9), JVg=R.JVg.reshape(9),
                    JVa=R.JVa.reshape(9), JPg=R.JPg.reshape(9), JPa=R.JPa.reshape(9))
    else:
        link.update(dR=dRb.reshape(9), dV=dVb, dP=dPb)
    return state, link, ok


# ---------------------------------------------------------------------------------------------------------------------
# the INDEPENDENT form
# ---------------------------------------------------------------------------------------------------------------------
def literal_normalize(R):
    U, _, Vt = np.linalg.svd(R)
    return (U @ Vt).astype(R.dtype)


def literal_integrated_rotation(v):
    F = v.dtype.type
    d2 = F(v @ v)
    d = F(np.sqrt(d2))
    W = hat(v)
    I = np.eye(3, dtype=F)
    if d < F(EPS):
        return I + W, I
    s, c = F(np.sin(d)), F(np.cos(d))
    return (I + W * s / d + (W @ W) * (F(1) - c) / d2).astype(F), (I - W * (F(1) - c) / d2 + (W @ W) * (d - s) / (d2 * d)).astype(F)


def literal_integrate(R, step, noise):
    F = R.F
    step = np.asarray(step, F)
    a, w, dt = step[0:3], step[3:6], step[6]
    acc, accW = a - R.ba, w - R.bg
    dR, dT = R.dR, R.dT
    A, B = np.eye(9, dtype=F), np.zeros((9, 6), F)
    R.avgA = (dT * R.avgA + dR @ acc * dt) / (dT + dt)
    R.avgW = (dT * R.avgW + accW * dt) / (dT + dt)
    R.dP = R.dP + R.dV * dt + F(0.5) * (dR @ acc) * dt * dt
    R.dV = R.dV + dR @ acc * dt
    Wacc = hat(acc)
    A[3:6, 0:3] = -dR * dt @ Wacc
    A[6:9, 0:3] = -F(0.5) * dR * dt * dt @ Wacc
    A[6:9, 3:6] = np.eye(3, dtype=F) * dt
    B[3:6, 3:6] = dR * dt
    B[6:9, 3:6] = F(0.5) * dR * dt * dt
    R.JPa = R.JPa + R.JVa * dt - F(0.5) * dR * dt * dt
    R.JPg = R.JPg + R.JVg * dt - F(0.5) * dR * dt * dt @ Wacc @ R.JRg
    R.JVa = R.JVa - dR * dt
    R.JVg = R.JVg - dR * dt @ Wacc @ R.JRg
    dRi, rJ = literal_integrated_rotation(accW * dt)
    R.dR = literal_normalize(dR @ dRi)
    A[0:3, 0:3] = dRi.T
    B[0:3, 0:3] = rJ * dt
    R.C[0:9, 0:9] = A @ R.C[0:9, 0:9] @ A.T + B @ np.diag(noise.cov.astype(F)) @ B.T
    R.C[9:15, 9:15] += np.diag(noise.walk.astype(F))
    R.JRg = dRi.T @ R.JRg - rJ * dt
    R.dT = F(dT + dt)
    R.n_steps += 1
    for k, _ in REC_FIELDS:
        setattr(R, k, np.asarray(getattr(R, k), F) if k != "dT" else F(R.dT))


def literal_reintegrate(noise, bias, steps, F=f32):
    R = Record(bias, F)
    for s in np.asarray(steps, F).reshape(-1, 8):
        literal_integrate(R, s, noise)
    return R


def literal_exp(w):
    F = w.dtype.type
    th = F(np.sqrt(w @ w))
    W = hat(w)
    I = np.eye(3, dtype=F)
    if th < 1e-10:
        return I + W
    return (I + F(np.sin(th) / th) * W + F((1 - np.cos(th)) / (th * th)) * (W @ W)).astype(F)


def literal_deltas(R, bg, ba):
    F = R.F
    dbg, dba = np.asarray(bg, F) - R.bg, np.asarray(ba, F) - R.ba
    return (literal_normalize(R.dR @ literal_exp(R.JRg @ dbg)), R.dV + R.JVg @ dbg + R.JVa @ dba, R.dP + R.JPg @ dbg + R.JPa @ dba)


def literal_predict(which, s1, kf, frame, gravity, Rcb, tcb):
    R = frame if which == FROM_FRAME else kf
    F = R.F
    s1 = np.asarray(s1, F).reshape(21)
    Rcb, tcb = np.asarray(Rcb, F).reshape(3, 3), np.asarray(tcb, F).reshape(3)
    Rwb1, twb1, v1 = s1[0:9].reshape(3, 3), s1[9:12], s1[12:15]
    dRb, dVb, dPb = literal_deltas(R, s1[15:18], s1[18:21])
    g = np.array([0, 0, -gravity], F)
    t12 = R.dT
    Rwb2 = literal_normalize(Rwb1 @ dRb)
    twb2 = twb1 + v1 * t12 + F(0.5) * t12 * t12 * g + Rwb1 @ dPb
    v2 = v1 + t12 * g + Rwb1 @ dVb
    Rcw = Rcb @ Rwb2.T
    tcw = Rcb @ (-(Rwb2.T @ twb2)) + tcb
    return np.concatenate([Rcw.reshape(9), tcw, Rwb2.reshape(9), twb2, v2, s1[15:21]]).astype(F)


def literal_info9(C):
    Info = np.linalg.inv(np.asarray(C)[0:9, 0:9].astype(f64))
    Info = (Info + Info.T) / 2
    lam, V = np.linalg.eigh(Info)
    lam = np.where(lam < CLAMP, 0.0, lam)
    return (V * lam[None, :]) @ V.T

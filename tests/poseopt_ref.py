"""SPEC DECISION S14, normative: Optimizer::PoseOptimization (src/Optimizer.cc:765-1067) for the branch this fork
takes -- !mpCamera2, mvuRight[i] < 0, EdgeSE3ProjectXYZOnlyPose (include/OptimizableTypes.h:31-57, src/OptimizableTypes.cpp:49-63), pinhole
camera (src/CameraModels/Pinhole.cpp:33-39,69-79) -- written from those lines and the text of S14, not from the kernel.  binary64 where
the C++ is double, binary32 where it is float, one rounding per operator (numpy's elementwise operations do not contract), C++ precedence
as parenthesisation.  The Levenberg loop and SE3Quat::exp are g2o's, which is not in the tree: they are restated from the published
algorithm and adopted as this project's definition (parity with g2o is unpinned).

Every sum over edges is the fixed pairwise tree `tree_sum`; everything else is sequential as written.
"""
import collections
import math

import numpy as np

from mlpnp_ref import sincos64

f64 = np.float64
DBL_MAX = float(np.finfo(f64).max)
EXIT_RAN_ALL, EXIT_TRIALS, EXIT_RHO_ZERO = 0, 1, 2
MAX_TRIALS = 10
MIN_EDGES, MIN_EDGES_ROUNDS = 3, 10   # (:949), (:1055)
THIRD, TWO_THIRDS = 1.0 / 3.0, 2.0 / 3.0
COUNTS = collections.Counter()   # which branches ran (tests/test_poseopt.py asserts that the scenes reach them); no effect on results
TRI = [(j, k) for j in range(6) for k in range(j, 6)]   # the 21 upper-triangle entries of H, row by row


def pow2_at_least(n):
    p = 1
    while p < max(n, 1):
        p *= 2
    return p


def tree_sum(v, P=None):
    """T(v): v padded with +0.0 to the power of two P, then halves added pairwise: T(first half) + T(second half).  v may carry
    leading axes; the tree runs along the last one."""
    v = np.asarray(v, f64)
    P = pow2_at_least(v.shape[-1]) if P is None else P
    pad = np.zeros(v.shape[:-1] + (P,), f64)
    pad[..., :v.shape[-1]] = v
    v = pad
    with np.errstate(all="ignore"):
        while v.shape[-1] > 1:
            v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def camera_point(R, t, Xw):
    """Xc_k = ((R_k0 X + R_k1 Y) + R_k2 Z) + t_k"""
    X, Y, Z = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    return [((R[3 * k] * X + R[3 * k + 1] * Y) + R[3 * k + 2] * Z) + t[k] for k in range(3)]


def residual(R, t, cam, obs, Xw):
    """e = obs - project(Xc) (Pinhole.cpp:33-39) -> (e0, e1, x, y, z)"""
    fx, fy, cx, cy = (f64(c) for c in cam[:4])
    with np.errstate(all="ignore"):
        x, y, z = camera_point(R, t, Xw)
        u = fx * x / z + cx
        v = fy * y / z + cy
        return obs[:, 0] - u, obs[:, 1] - v, x, y, z


def chi2_of(e0, e1, w):
    with np.errstate(all="ignore"):
        return e0 * (w * e0) + e1 * (w * e1)


def robust(chi2, delta, huber):
    """(rho0, rho1): Huber with delta when `huber`, else (chi2, 1)"""
    if not huber:
        return chi2.copy(), np.ones_like(chi2)
    d2 = delta * delta
    with np.errstate(all="ignore"):
        s = np.sqrt(chi2)
        small = chi2 <= d2
        return np.where(small, chi2, 2.0 * s * delta - d2), np.where(small, 1.0, delta / s)


def jacobian(cam, x, y, z):
    """J = -projectJac(Xc) SE3deriv (OptimizableTypes.cpp:57-62, Pinhole.cpp:69-79), 2 x 6 as J[r][c]; columns 0..2 rotation, 3..5
    translation.  The structural zeros of the two factors are not multiplied: J[0][4] = J[1][3] = +0.0."""
    fx, fy = f64(cam[0]), f64(cam[1])
    with np.errstate(all="ignore"):
        zz = z * z
        a = fx / z
        b = -fx * x / zz
        c = fy / z
        d = -fy * y / zz
        zero = np.zeros_like(z)
        J0 = [-(b * y), -(a * z - b * x), a * y, -a, zero, -b]
        J1 = [-(d * y - c * z), d * x, -(c * x), zero, -c, -d]
    return J0, J1


def build(R, t, cam, obs, w, Xw, active, delta, huber, P):
    """-> H [21] (upper triangle, row by row), b [6], cur = sum rho0; inactive edges contribute +0.0"""
    e0, e1, x, y, z = residual(R, t, cam, obs, Xw)
    chi2 = chi2_of(e0, e1, w)
    rho0, rho1 = robust(chi2, delta, huber)
    if huber and bool(np.any(active & (chi2 > delta * delta))):
        COUNTS["huber_linear_region"] += 1
    J0, J1 = jacobian(cam, x, y, z)
    with np.errstate(all="ignore"):
        ww = rho1 * w
        we0, we1 = ww * e0, ww * e1
        terms = [(J0[j] * ww) * J0[k] + (J1[j] * ww) * J1[k] for j, k in TRI]
        terms += [-(J0[j] * we0 + J1[j] * we1) for j in range(6)]
        terms.append(rho0)
    v = np.where(active[None, :], np.array(terms, f64), 0.0)
    s = tree_sum(v, P)
    return s[:21], s[21:27], float(s[27])


def sum_rho0(R, t, cam, obs, w, Xw, active, delta, huber, P):
    e0, e1, _, _, _ = residual(R, t, cam, obs, Xw)
    rho0, _ = robust(chi2_of(e0, e1, w), delta, huber)
    return float(tree_sum(np.where(active, rho0, 0.0), P))


def ldlt_solve6(A, b):
    """S13's L D L^T with diagonal pivoting (csrc/ldlt.h; tests/mlpnp_ref.py ldlt_solve is the same sequence, batched) -> (x, every
    pivot > 0)"""
    A = [[float(v) for v in row] for row in A]
    n = 6
    L = [[0.0] * n for _ in range(n)]
    d = [0.0] * n
    perm = list(range(n))
    with np.errstate(all="ignore"):
        for k in range(n):
            best = k
            for i in range(k + 1, n):
                if abs(A[i][i]) > abs(A[best][best]):
                    best = i
            A[k], A[best] = A[best], A[k]
            for i in range(n):
                A[i][k], A[i][best] = A[i][best], A[i][k]
            L[k], L[best] = L[best], L[k]
            perm[k], perm[best] = perm[best], perm[k]
            dk = A[k][k]
            d[k] = dk
            col = [A[i][k] for i in range(n)]
            for i in range(k + 1, n):
                li = 0.0 if dk == 0.0 else float(f64(col[i]) / f64(dk))
                L[i][k] = li
                for j in range(k + 1, i + 1):
                    val = float(f64(A[i][j]) - f64(li) * f64(col[j]))
                    A[i][j] = val
                    A[j][i] = val
        z = [0.0] * n
        for i in range(n):
            acc = f64(b[perm[i]])
            for j in range(i):
                acc = acc - f64(L[i][j]) * f64(z[j])
            z[i] = float(acc)
        wv = [0.0 if d[i] == 0.0 else float(f64(z[i]) / f64(d[i])) for i in range(n)]
        xs = [0.0] * n
        for i in range(n - 1, -1, -1):
            acc = f64(wv[i])
            for j in range(i + 1, n):
                acc = acc - f64(L[j][i]) * f64(xs[j])
            xs[i] = float(acc)
    x = [0.0] * n
    for i in range(n):
        x[perm[i]] = xs[i]
    return np.array(x, f64), all(dk > 0.0 for dk in d)


def mul3(A, B):
    with np.errstate(all="ignore"):
        return np.array([(A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)], f64)


def matvec3(A, v):
    with np.errstate(all="ignore"):
        return np.array([(A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2] for i in range(3)], f64)


EYE = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], f64)


def se3_exp(dx):
    """SE3Quat::exp as published, kept as matrices: omega = dx[0..3), upsilon = dx[3..6) -> (R [9], V upsilon [3])"""
    dx = np.asarray(dx, f64)
    om, up = dx[:3], dx[3:]
    with np.errstate(all="ignore"):
        theta = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
        Om = np.array([0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0], f64)
        Om2 = mul3(Om, Om)
        COUNTS["small_theta" if theta < 1e-5 else "large_theta"] += 1
        if theta < 1e-5:
            R = (EYE + Om) + 0.5 * Om2
            V = (EYE + 0.5 * Om) + Om2 / 6.0
        else:
            s, c = sincos64(theta)
            s, c = f64(s), f64(c)
            A = s / theta
            B = (1.0 - c) / (theta * theta)
            Cc = (theta - s) / (theta * theta * theta)
            R = (EYE + A * Om) + B * Om2
            V = (EYE + B * Om) + Cc * Om2
        return R, matvec3(V, up)


def apply_update(dx, R, t):
    """exp(dx) . (R, t) = (Re R, Re t + V upsilon)"""
    Re, Vu = se3_exp(dx)
    with np.errstate(all="ignore"):
        return mul3(Re, R), matvec3(Re, t) + Vu


def delta_of(huber_delta2):
    """deltaMono = (float) sqrt(7.815) (:805), setDelta takes it as a double (:837)"""
    return float(f64(np.float32(math.sqrt(float(huber_delta2)))))


def edges_of(level_sigma2, kp_xy, kp_octave, mp_index, points):
    first = np.flatnonzero(np.asarray(mp_index) >= 0)
    obs = np.asarray(kp_xy, np.float32)[first].astype(f64)
    inv = (np.float32(1.0) / np.asarray(level_sigma2, np.float32)).astype(np.float32)   # mvInvLevelSigma2 (ORBextractor.cc:99)
    w = inv[np.asarray(kp_octave)[first]].astype(f64)
    Xw = np.asarray(points, np.float32).reshape(-1, 3)[np.asarray(mp_index)[first]].astype(f64)
    return first, obs, w, Xw


def one_round(R0, t0, cam, obs, w, Xw, active, delta, huber, iterations, P, trace=None):
    """one optimizer.optimize(its) from the initial pose -> dict(R, t, iterations, trials, lam, chi2, exit)"""
    R, t = R0.copy(), t0.copy()
    lam, ni, cur = 0.0, 2.0, 0.0
    n_it, n_trials, exit_kind = 0, 0, EXIT_RAN_ALL
    with np.errstate(all="ignore"):
        for k in range(iterations):
            n_it += 1
            H, b, cur = build(R, t, cam, obs, w, Xw, active, delta, huber, P)
            diag = [H[TRI.index((j, j))] for j in range(6)]
            if k == 0:
                m = 0.0
                for j in range(6):
                    if abs(diag[j]) > m:
                        m = abs(float(diag[j]))
                lam = float(f64(1e-5) * f64(m))
                ni = 2.0
            rho, q = 0.0, 0
            while True:
                A = np.zeros((6, 6), f64)
                for (j, kk), h in zip(TRI, H):
                    A[j, kk] = h
                    A[kk, j] = h
                for j in range(6):
                    A[j, j] = f64(diag[j]) + f64(lam)
                dx, ok = ldlt_solve6(A, b)
                Rn, tn = apply_update(dx, R, t)
                tmp = sum_rho0(Rn, tn, cam, obs, w, Xw, active, delta, huber, P)
                if not ok:
                    COUNTS["not_ok"] += 1
                    tmp = DBL_MAX
                scale = f64(0.0)
                for j in range(6):
                    scale = scale + dx[j] * (f64(lam) * dx[j] + b[j])
                scale = scale + f64(1e-3)
                rho = float((f64(cur) - f64(tmp)) / scale)
                n_trials += 1
                q += 1
                if rho > 0 and math.isfinite(tmp):
                    R, t = Rn, tn
                    tt = f64(2.0) * f64(rho) - f64(1.0)
                    alpha = float(f64(1.0) - (tt * tt) * tt)
                    sf = TWO_THIRDS if TWO_THIRDS < alpha else alpha     # std::min(alpha, 2/3)
                    sf = sf if THIRD < sf else THIRD                     # std::max(1/3, .)
                    lam = float(f64(lam) * f64(sf))
                    ni = 2.0
                    cur = tmp
                    COUNTS["accepted"] += 1
                    if trace is not None:
                        trace.append(cur)
                else:
                    COUNTS["rejected"] += 1
                    lam = float(f64(lam) * f64(ni))
                    ni = float(f64(ni) * f64(2.0))
                if not (rho < 0 and q < MAX_TRIALS):
                    break
            if q == MAX_TRIALS:
                exit_kind = EXIT_TRIALS
                break
            if rho == 0:
                exit_kind = EXIT_RHO_ZERO
                break
    return dict(R=R, t=t, iterations=n_it, trials=n_trials, lam=lam, chi2=cur, exit=exit_kind)


def pose_optimization(cam, level_sigma2, kp_xy, kp_octave, mp_index, points, Rcw, tcw, chi2_threshold=5.991, huber_delta2=7.815,
                      iterations=25, rounds=4, traces=None):
    """-> dict(Tcw [4, 4] float32, outlier [n] uint8, n_inliers, N_e, rounds_run, round_pose [rounds_run, 12] float64, round_iterations,
    round_trials, round_lambda, round_chi2, round_nbad, round_exit, round_outlier [rounds_run, N_e] uint8)"""
    n = len(mp_index)
    first, obs, w, Xw = edges_of(level_sigma2, kp_xy, kp_octave, mp_index, points)
    Ne = len(first)
    R0 = np.asarray(Rcw, np.float32).reshape(9).astype(f64)
    t0 = np.asarray(tcw, np.float32).reshape(3).astype(f64)
    out = dict(N_e=Ne, rounds_run=0, outlier=np.zeros(n, np.uint8), n_inliers=0, round_pose=np.zeros((0, 12), f64),
               round_iterations=np.zeros(0, np.int32), round_trials=np.zeros(0, np.int32), round_lambda=np.zeros(0, f64),
               round_chi2=np.zeros(0, f64), round_nbad=np.zeros(0, np.int32), round_exit=np.zeros(0, np.int32),
               round_outlier=np.zeros((0, Ne), np.uint8))
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3] = np.asarray(Rcw, np.float32).reshape(3, 3)
    Tcw[:3, 3] = np.asarray(tcw, np.float32).reshape(3)
    out["Tcw"] = Tcw
    if Ne < MIN_EDGES:
        return out
    delta = delta_of(huber_delta2)
    thr = np.float32(chi2_threshold)
    P = pow2_at_least(Ne)
    active = np.ones(Ne, bool)
    rec = {k: [] for k in ("pose", "iterations", "trials", "lambda", "chi2", "nbad", "exit", "outlier")}
    for rnd in range(rounds):
        tr = [] if traces is not None else None
        r = one_round(R0, t0, cam, obs, w, Xw, active, delta, rnd <= 2, iterations, P, tr)
        if traces is not None:
            traces.append(tr)
        e0, e1, _, _, _ = residual(r["R"], r["t"], cam, obs, Xw)
        with np.errstate(all="ignore"):
            bad = chi2_of(e0, e1, w).astype(np.float32) > thr
        active = ~bad
        rec["pose"].append(np.concatenate([r["R"], r["t"]]))
        for k, key in (("iterations", "iterations"), ("trials", "trials"), ("lambda", "lam"), ("chi2", "chi2"), ("exit", "exit")):
            rec[k].append(r[key])
        rec["nbad"].append(int(bad.sum()))
        rec["outlier"].append(bad.astype(np.uint8))
        if Ne < MIN_EDGES_ROUNDS:
            break
    nr = len(rec["pose"])
    out.update(rounds_run=nr, round_pose=np.array(rec["pose"], f64), round_iterations=np.array(rec["iterations"], np.int32),
               round_trials=np.array(rec["trials"], np.int32), round_lambda=np.array(rec["lambda"], f64),
               round_chi2=np.array(rec["chi2"], f64), round_nbad=np.array(rec["nbad"], np.int32),
               round_exit=np.array(rec["exit"], np.int32), round_outlier=np.array(rec["outlier"], np.uint8).reshape(nr, Ne))
    last = out["round_pose"][-1]
    with np.errstate(all="ignore"):
        Tcw[:3, :3] = last[:9].reshape(3, 3).astype(np.float32)
        Tcw[:3, 3] = last[9:].astype(np.float32)
    out["outlier"][first] = rec["outlier"][-1]
    out["n_inliers"] = Ne - rec["nbad"][-1]
    return out

"""SPEC DECISION S19, normative: Optimizer::PoseInertialOptimizationLastKeyFrame (src/Optimizer.cc:3447-3844) for
the branch this fork takes -- one pinhole camera, mono edges only -- written from those lines, src/G2oTypes.cc:73-119, 170-220, 375-395,
492-594, 777-861, include/G2oTypes.h:390-423, 634-700, src/CameraModels/Pinhole.cpp and the text of S19, not from the kernel.  binary64
where the C++ is double, binary32 where it is float, one rounding per operator (numpy's elementwise operations do not contract), C++ /
Eigen coefficient-wise precedence as parenthesisation; sin, cos, acos are the sequences of csrc/spec_math.h (mlpnp_ref.sincos64 /
acos64).  The Gauss-Newton loop (OptimizationAlgorithmGaussNewton + LinearSolverDense) is g2o's, which is not in the tree: it is
restated from the published algorithm and adopted as this project's definition (parity with g2o is unpinned, as in S14 and S17).

Every sum over mono edges is S14's fixed pairwise tree (poseopt_ref.tree_sum); everything else is sequential as written.
"""
import collections

import numpy as np

from mlpnp_ref import acos64, sincos64
from poseopt_ref import chi2_of, delta_of, edges_of, matvec3, mul3, pow2_at_least, residual, robust, tree_sum

f64 = np.float64
f32 = np.float32
N = 15
COUNTS = collections.Counter()   # which branches ran (tests/test_pose_inertial.py asserts that the scenes reach them); no effect on results
TRI6 = [(j, k) for j in range(6) for k in range(j, 6)]
EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
ROW_OF_BLOCK = (0, 6, 3)          # the rows of J9's block for the column blocks rotation, translation, velocity

PARAMS = dict(chi2=(12.0, 7.5, 5.991, 5.991), close_factor=1.5, close_depth=10.0, recover_chi2=24.0, recover_below=30,
              huber_delta2=5.991, iterations=15, rounds=4, rec_init=0, gravity=9.81)


def d64(a, n):
    """the caller's floats as binary64"""
    return np.asarray(a, f32).reshape(n).astype(f64)


def hat(w):
    x, y, z = w
    return np.array([0.0, -z, y, z, 0.0, -x, -y, x, 0.0], f64)


def transpose3(A):
    return np.array([A[3 * j + i] for i in range(3) for j in range(3)], f64)


def norm2(w):
    with np.errstate(all="ignore"):
        return (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]


def exp_so3(w, counts=COUNTS):
    """ExpSO3 (G2oTypes.cc:782-798) without NormalizeRotation (departure 1)"""
    w = np.asarray(w, f64)
    with np.errstate(all="ignore"):
        d2 = norm2(w)
        d = np.sqrt(d2)
        W = hat(w)
        W2 = mul3(W, W)
        if d < 1e-5:
            counts["exp_small"] += 1
            return np.array([(f64(EYE[i]) + W[i]) + 0.5 * W2[i] for i in range(9)], f64)
        counts["exp_general"] += 1
        s, c = (f64(v) for v in sincos64(d))
        return np.array([(f64(EYE[i]) + W[i] * s / d) + W2[i] * (1.0 - c) / d2 for i in range(9)], f64)


def log_so3(R, counts=COUNTS):
    """LogSO3 (:800-814)"""
    with np.errstate(all="ignore"):
        tr = (R[0] + R[4]) + R[8]
        w = np.array([(R[7] - R[5]) / 2.0, (R[2] - R[6]) / 2.0, (R[3] - R[1]) / 2.0], f64)
        costheta = (tr - 1.0) * 0.5
        if costheta > 1.0 or costheta < -1.0:
            counts["log_outside"] += 1
            return w
        theta = f64(acos64(costheta))
        s = f64(sincos64(theta)[0])
        if abs(s) < 1e-5:
            counts["log_small"] += 1
            return w
        counts["log_general"] += 1
        return np.array([theta * w[i] / s for i in range(3)], f64)


def inverse_right_jacobian_so3(v, counts=COUNTS):
    """InverseRightJacobianSO3 (:821-832)"""
    v = np.asarray(v, f64)
    with np.errstate(all="ignore"):
        d2 = norm2(v)
        d = np.sqrt(d2)
        if d < 1e-5:
            counts["invjr_small"] += 1
            return np.array(EYE, f64)
        counts["invjr_general"] += 1
        W = hat(v)
        W2 = mul3(W, W)
        s, c = (f64(x) for x in sincos64(d))
        k = 1.0 / d2 - (1.0 + c) / (2.0 * d * s)
        return np.array([(f64(EYE[i]) + W[i] / 2.0) + W2[i] * k for i in range(9)], f64)


def right_jacobian_so3(v, counts=COUNTS):
    """RightJacobianSO3 (:839-854): pinned with the other three; the solver does not call it (only a fixed vertex's column does)"""
    v = np.asarray(v, f64)
    with np.errstate(all="ignore"):
        d2 = norm2(v)
        d = np.sqrt(d2)
        if d < 1e-5:
            counts["jr_small"] += 1
            return np.array(EYE, f64)
        counts["jr_general"] += 1
        W = hat(v)
        W2 = mul3(W, W)
        s, c = (f64(x) for x in sincos64(d))
        return np.array([(f64(EYE[i]) - W[i] * (1.0 - c) / d2) + W2[i] * (d - s) / (d2 * d) for i in range(9)], f64)


def ldlt_solve(A, b):
    """csrc/ldlt.h ldlt_solve_n: L D L^T with diagonal pivoting (largest |diagonal| of the trailing block, first of equals, found with
    '>'), any n -> (x, every pivot > 0)"""
    n = len(b)
    A = [[f64(v) for v in row] for row in A]
    L = [[f64(0.0)] * n for _ in range(n)]
    d = [f64(0.0)] * n
    perm = list(range(n))
    with np.errstate(all="ignore"):
        for k in range(n):
            best, best_abs = k, abs(A[k][k])
            for i in range(k + 1, n):
                if abs(A[i][i]) > best_abs:
                    best, best_abs = i, abs(A[i][i])
            A[k], A[best] = A[best], A[k]
            for i in range(n):
                A[i][k], A[i][best] = A[i][best], A[i][k]
            L[k], L[best] = L[best], L[k]
            perm[k], perm[best] = perm[best], perm[k]
            dk = A[k][k]
            d[k] = dk
            col = [A[i][k] for i in range(n)]
            for i in range(k + 1, n):
                li = f64(0.0) if dk == 0.0 else col[i] / dk
                L[i][k] = li
                for j in range(k + 1, i + 1):
                    val = A[i][j] - li * col[j]
                    A[i][j] = val
                    A[j][i] = val
        z = [f64(0.0)] * n
        for i in range(n):
            acc = f64(b[perm[i]])
            for j in range(i):
                acc = acc - L[i][j] * z[j]
            z[i] = acc
        wv = [f64(0.0) if d[i] == 0.0 else z[i] / d[i] for i in range(n)]
        xs = [f64(0.0)] * n
        for i in range(n - 1, -1, -1):
            acc = wv[i]
            for j in range(i + 1, n):
                acc = acc - L[j][i] * xs[j]
            xs[i] = acc
    x = [f64(0.0)] * n
    for i in range(n):
        x[perm[i]] = xs[i]
    return np.array(x, f64), all(dk > 0.0 for dk in d)


class Link:
    """orbfe_imu_link as binary64: the fixed key frame's state, the preintegrated constants, the extrinsics"""

    def __init__(self, link):
        self.Rwb1, self.twb1, self.v1 = d64(link["Rwb1"], 9), d64(link["twb1"], 3), d64(link["v1"], 3)
        self.bg1, self.ba1 = d64(link["bg1"], 3), d64(link["ba1"], 3)
        self.dR, self.dV, self.dP = d64(link["dR"], 9), d64(link["dV"], 3), d64(link["dP"], 3)
        self.dt = f64(f32(link["dt"]))
        self.Rcb, self.tcb, self.tbc = d64(link["Rcb"], 9), d64(link["tcb"], 3), d64(link["tbc"], 3)
        self.info9 = np.asarray(link["info9"], f64).reshape(81)
        self.infoG, self.infoA = np.asarray(link["infoG"], f64).reshape(9), np.asarray(link["infoA"], f64).reshape(9)


class State:
    def __init__(self, Rcw, tcw, Rwb, twb, v, bg, ba):
        self.Rcw, self.tcw = d64(Rcw, 9), d64(tcw, 3)
        self.Rwb, self.twb, self.v, self.bg, self.ba = d64(Rwb, 9), d64(twb, 3), d64(v, 3), d64(bg, 3), d64(ba, 3)

    def vector(self):
        return np.concatenate([self.Rwb, self.twb, self.v, self.bg, self.ba])


def update(K, dx, S):
    """ImuCamPose::Update (:192-220) and the three additive vertices; no NormalizeRotation"""
    ur, ut = dx[0:3], dx[3:6]
    with np.errstate(all="ignore"):
        S.twb = S.twb + matvec3(S.Rwb, ut)
        S.Rwb = mul3(S.Rwb, exp_so3(ur))
        S.v = S.v + dx[6:9]
        S.bg = S.bg + dx[9:12]
        S.ba = S.ba + dx[12:15]
        Rbw = transpose3(S.Rwb)
        tbw = -matvec3(Rbw, S.twb)
        S.Rcw = mul3(K.Rcb, Rbw)
        S.tcw = matvec3(K.Rcb, tbw) + K.tcb


def mono_jacobian(cam, K, x, y, z):
    """projectJac(Xc) Rcb [-[Xb]x | I] (:375-395), 2 x 6 as J[r][c]; the structural zeros of both factors are not multiplied"""
    fx, fy = f64(cam[0]), f64(cam[1])
    R = K.Rcb
    with np.errstate(all="ignore"):
        xb = ((R[0] * x + R[3] * y) + R[6] * z) + K.tbc[0]
        yb = ((R[1] * x + R[4] * y) + R[7] * z) + K.tbc[1]
        zb = ((R[2] * x + R[5] * y) + R[8] * z) + K.tbc[2]
        zz = z * z
        a = fx / z
        b = -fx * x / zz
        c = fy / z
        d = -fy * y / zz
        P0 = [a * R[j] + b * R[6 + j] for j in range(3)]
        P1 = [c * R[3 + j] + d * R[6 + j] for j in range(3)]
        rows = []
        for P in (P0, P1):
            rows.append([P[1] * -zb + P[2] * yb, P[0] * zb + P[2] * -xb, P[0] * -yb + P[1] * xb, P[0], P[1], P[2]])
    return rows


def mono_sums(S, K, cam, obs, w, Xw, active, delta, huber, P):
    """-> the 28 tree sums: H [21] (upper triangle of the pose block, row by row), b [6], sum rho0; inactive edges contribute +0.0"""
    e0, e1, x, y, z = residual(S.Rcw, S.tcw, cam, obs, Xw)
    chi2 = chi2_of(e0, e1, w)
    rho0, rho1 = robust(chi2, delta, huber)
    if huber and bool(np.any(active & (chi2 > delta * delta))):
        COUNTS["huber_linear_region"] += 1
    J0, J1 = mono_jacobian(cam, K, x, y, z)
    with np.errstate(all="ignore"):
        ww = rho1 * w
        we0, we1 = ww * e0, ww * e1
        terms = [(J0[j] * ww) * J0[k] + (J1[j] * ww) * J1[k] for j, k in TRI6]
        terms += [-(J0[j] * we0 + J1[j] * we1) for j in range(6)]
        terms.append(rho0)
    v = np.where(active[None, :], np.array(terms, f64).reshape(28, len(w)), 0.0)
    return tree_sum(v, P)


def inertial_edge(K, gravity, S):
    """-> (H9 [9, 9], b9 [9], e9 [9]): J9^T info9 J9 and -J9^T (info9 e9) over the columns of the free pose and velocity (:514-594).
    Block (p, q), p <= q, is B_p^T (info9[rows of p][rows of q] B_q); the lower triangle is the mirror of the upper."""
    with np.errstate(all="ignore"):
        Rbw1 = transpose3(K.Rwb1)
        eR = mul3(mul3(transpose3(K.dR), Rbw1), S.Rwb)
        er = log_so3(eR)
        g = np.array([0.0, 0.0, -gravity], f64)
        a = (S.v - K.v1) - g * K.dt
        c = ((S.twb - K.twb1) - K.v1 * K.dt) - g * K.dt * K.dt / 2.0
        e9 = np.concatenate([er, matvec3(Rbw1, a) - K.dV, matvec3(Rbw1, c) - K.dP])
        B = [inverse_right_jacobian_so3(er), mul3(Rbw1, S.Rwb), Rbw1]
        Om = K.info9
        Or = np.zeros(9, f64)
        for r in range(9):
            acc = Om[9 * r] * e9[0]
            for q in range(1, 9):
                acc = acc + Om[9 * r + q] * e9[q]
            Or[r] = -acc
        H9, b9 = np.zeros((9, 9), f64), np.zeros(9, f64)
        for p in range(3):
            rp = ROW_OF_BLOCK[p]
            Bt = transpose3(B[p])
            b9[3 * p:3 * p + 3] = matvec3(Bt, Or[rp:rp + 3])
            for q in range(p, 3):
                rq = ROW_OF_BLOCK[q]
                W = np.array([Om[9 * (rp + i) + (rq + j)] for i in range(3) for j in range(3)], f64)
                Hb = mul3(Bt, mul3(W, B[q]))
                for i in range(3):
                    for j in range(3):
                        if q > p or j >= i:
                            H9[3 * p + i, 3 * q + j] = Hb[3 * i + j]
                            H9[3 * q + j, 3 * p + i] = Hb[3 * i + j]
    return H9, b9, e9


def sym_upper(M):
    """the upper triangle of a 3 x 3 (row-major 9), mirrored"""
    return np.array([[M[3 * min(i, j) + max(i, j)] for j in range(3)] for i in range(3)], f64)


def system(K, gravity, S, sums):
    """the 15 x 15 system of one iteration; order of the additions: the mono tree sum first, the inertial term added to it"""
    H9, b9, _ = inertial_edge(K, gravity, S)
    H, b = np.zeros((N, N), f64), np.zeros(N, f64)
    with np.errstate(all="ignore"):
        H[:9, :9] = H9
        for (j, k), s in zip(TRI6, sums[:21]):
            H[j, k] = s + H9[j, k]
            H[k, j] = H[j, k]
        b[:6] = sums[21:27] + b9[:6]
        b[6:9] = b9[6:9]
        H[9:12, 9:12] = sym_upper(K.infoG)
        H[12:15, 12:15] = sym_upper(K.infoA)
        b[9:12] = -matvec3(K.infoG, S.bg - K.bg1)
        b[12:15] = -matvec3(K.infoA, S.ba - K.ba1)
    return H, b


def score(S, cam, obs, w, Xw):
    """fresh (float) chi2 and Xc.z > 0 of every edge at the state (departure 2)"""
    e0, e1, _, _, z = residual(S.Rcw, S.tcw, cam, obs, Xw)
    with np.errstate(all="ignore"):
        return chi2_of(e0, e1, w).astype(f32), z > 0.0


def pose_inertial_optimization(cam, level_sigma2, kp_xy, kp_octave, mp_index, points, track_depth, link, Rcw, tcw, Rwb, twb, v, bg, ba,
                               **kw):
    """-> dict(Rwb [9], twb, v, bg, ba float32; H [15, 15] float64; outlier [n] uint8; n_inliers; N_e; rounds_run; recovered;
    round_iterations, round_ok, round_nbad [rounds_run]; round_state [rounds_run, 21] float64 (Rwb, twb, v, bg, ba);
    round_outlier [rounds_run, N_e] uint8)"""
    prm = dict(PARAMS)
    prm.update(kw)
    n = len(mp_index)
    first, obs, w, Xw = edges_of(level_sigma2, kp_xy, kp_octave, mp_index, points)
    Ne = len(first)
    P = pow2_at_least(Ne)
    K = Link(link)
    S = State(Rcw, tcw, Rwb, twb, v, bg, ba)
    gravity = f64(f32(prm["gravity"]))
    delta = delta_of(prm["huber_delta2"])
    close = np.asarray(track_depth, f32)[np.asarray(mp_index)[first]] < f32(prm["close_depth"])
    active = np.ones(Ne, bool)
    bad = np.zeros(Ne, bool)
    rec = {k: [] for k in ("iterations", "ok", "nbad", "state", "outlier")}
    n_bad = 0
    for rnd in range(prm["rounds"]):
        huber = rnd <= 2   # the kernel is dropped after round index 2 (:3717-3718)
        n_it, ok = 0, True
        for _ in range(prm["iterations"]):
            n_it += 1
            sums = mono_sums(S, K, cam, obs, w, Xw, active, delta, huber, P)
            H, b = system(K, gravity, S, sums)
            dx, ok = ldlt_solve(H, b)
            if not ok:
                COUNTS["not_ok"] += 1
                break
            update(K, dx, S)
        thr = f32(prm["chi2"][rnd])
        thr_close = f32(f64(prm["close_factor"]) * f64(thr))
        chi2, front = score(S, cam, obs, w, Xw)
        with np.errstate(all="ignore"):
            bad = ((chi2 > thr) & ~close) | (close & (chi2 > thr_close)) | ~front
        if bool(np.any(bad & ~front)):
            COUNTS["depth_not_positive"] += 1
        active = ~bad
        n_bad = int(bad.sum())
        rec["iterations"].append(n_it)
        rec["ok"].append(int(ok))
        rec["nbad"].append(n_bad)
        rec["state"].append(S.vector())
        rec["outlier"].append(bad.astype(np.uint8))
        if Ne + 3 < 10:   # optimizer.edges().size() < 10 (:3757)
            COUNTS["few_edges_break"] += 1
            break
    recovered = 0
    if Ne - n_bad < prm["recover_below"] and not prm["rec_init"]:
        COUNTS["recovery"] += 1
        recovered = 1
        chi2, _ = score(S, cam, obs, w, Xw)
        with np.errstate(all="ignore"):
            good = chi2 < f32(prm["recover_chi2"])
        bad = bad & ~good
        n_bad = int((~good).sum())
    # the Hessian at the final state (:3800-3837): no robust weight on the mono edges
    sums = mono_sums(S, K, cam, obs, w, Xw, ~bad, delta, False, P)
    H9, _, _ = inertial_edge(K, gravity, S)
    Hout = np.zeros((N, N), f64)
    with np.errstate(all="ignore"):
        Hout[:9, :9] = H9
        for (j, k), s in zip(TRI6, sums[:21]):
            Hout[j, k] = H9[j, k] + s
            Hout[k, j] = Hout[j, k]
    Hout[9:12, 9:12] = K.infoG.reshape(3, 3)
    Hout[12:15, 12:15] = K.infoA.reshape(3, 3)
    nr = len(rec["iterations"])
    outlier = np.zeros(n, np.uint8)
    outlier[first] = bad.astype(np.uint8)
    with np.errstate(all="ignore"):
        out = dict(Rwb=S.Rwb.astype(f32), twb=S.twb.astype(f32), v=S.v.astype(f32), bg=S.bg.astype(f32), ba=S.ba.astype(f32), H=Hout,
                   outlier=outlier, n_inliers=Ne - n_bad, N_e=Ne, rounds_run=nr, recovered=recovered,
                   round_iterations=np.array(rec["iterations"], np.int32), round_ok=np.array(rec["ok"], np.int32),
                   round_nbad=np.array(rec["nbad"], np.int32), round_state=np.array(rec["state"], f64).reshape(nr, 21),
                   round_outlier=np.array(rec["outlier"], np.uint8).reshape(nr, Ne))
    out["state64"] = S.vector()
    return out

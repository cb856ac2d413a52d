"""SPEC DECISION S17, normative: the bundle adjustment of the initial map -- Optimizer::GlobalBundleAdjustemnt(map, 20)
as CreateInitialMapMonocular calls it (src/Tracking.cc:698 -> src/Optimizer.cc:60-369) -- for the only shape that call has: two key
frames of which the first is fixed (:133), N map points each observed once in either frame, EdgeSE3ProjectXYZ
(include/OptimizableTypes.h:99-110, src/OptimizableTypes.cpp:139-160), pinhole camera (src/CameraModels/Pinhole.cpp:33-39,69-79), one
Levenberg run with a Huber kernel of delta = (float) sqrt(5.99) (:139) and no outlier rounds.  Written from those lines and the text of
S17, not from the kernel.

binary64 where the C++ is double, binary32 where it is float, one rounding per operator (numpy's elementwise operations do not
contract), C++ precedence as parenthesisation.  g2o is an empty submodule of the reference tree: the Levenberg loop
(OptimizationAlgorithmLevenberg), the block solver's Schur complement over the marginalised points (BlockSolver_6_3) and SE3Quat::exp
are restated from the published algorithm and adopted as this project's definition; parity with a g2o build is unpinned, as in S14.
What S14 pinned is imported from poseopt_ref.py word for word: the residual, chi2, Huber, the pose Jacobian, exp, the 6 x 6 solve, the
tree.

Point p is the p-th i, ascending, with matches12[i] >= 0.  Its edge 0 observes kp1[i] from pose 1 (fixed: a fixed vertex gets no
Jacobian), its edge 1 observes kp2[matches12[i]] from pose 2 (free).  The reference walks a std::map keyed by pointer, so its edge
order is unpinned; here edge 0 comes first.

Every sum over points is the fixed pairwise tree `tree_sum` over P = the smallest power of two >= N (+0.0 padding); everything else is
sequential as written.  The one reduction that is no sum -- the maximum behind lambda_0 -- is taken with `>` from 0.0 over values of
which none that is kept is a NaN (a NaN never wins a `>`), and a maximum of non-NaN values does not depend on the order they are
visited in: any reduction order gives the same bits.
"""
import collections
import math

import numpy as np

import poseopt_ref as P14
from poseopt_ref import (DBL_MAX, EXIT_RAN_ALL, EXIT_RHO_ZERO, EXIT_TRIALS, MAX_TRIALS, THIRD, TRI, TWO_THIRDS, apply_update, chi2_of,
                         delta_of, jacobian, ldlt_solve6, pow2_at_least, residual, robust, tree_sum)

f64 = np.float64
COUNTS = collections.Counter()   # which branches ran (tests/test_initial_ba.py asserts that the scenes reach them); no effect on results
SYM = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]   # the six distinct entries of a symmetric 3 x 3, row by row
MAX_ITERATIONS = 64


def point_rows(cam, R, x, y, z):
    """-projectJac(Xc) R (OptimizableTypes.cpp:150-152), 2 x 3 as P[r][k]; the structural zeros of projectJac are not multiplied"""
    fx, fy = f64(cam[0]), f64(cam[1])
    with np.errstate(all="ignore"):
        zz = z * z
        a = fx / z
        b = -fx * x / zz
        c = fy / z
        d = -fy * y / zz
        P0 = [((-a) * R[k]) + ((-b) * R[6 + k]) for k in range(3)]
        P1 = [((-c) * R[3 + k]) + ((-d) * R[6 + k]) for k in range(3)]
    return P0, P1


def linearise(Ra, ta, Rb, tb, cam, obs1, w1, obs2, w2, X, delta, huber):
    """per point: Hpp [6] (SYM order), bp [3], Hxp [6][3], the 21 + 6 pose terms and the cost; edge 0's terms first, edge 1's added"""
    with np.errstate(all="ignore"):
        e0, e1, x, y, z = residual(Ra, ta, cam, obs1, X)
        chi = chi2_of(e0, e1, w1)
        rho0a, rho1 = robust(chi, delta, huber)
        lin = chi > delta * delta
        P0, P1 = point_rows(cam, Ra, x, y, z)
        ww = rho1 * w1
        we0, we1 = ww * e0, ww * e1
        Hpp = [((P0[j] * ww) * P0[k]) + ((P1[j] * ww) * P1[k]) for j, k in SYM]
        bp = [-((P0[j] * we0) + (P1[j] * we1)) for j in range(3)]

        e0, e1, x, y, z = residual(Rb, tb, cam, obs2, X)
        chi = chi2_of(e0, e1, w2)
        rho0b, rho1 = robust(chi, delta, huber)
        if huber and bool(np.any(lin | (chi > delta * delta))):
            COUNTS["huber_linear_region"] += 1
        J0, J1 = jacobian(cam, x, y, z)
        P0, P1 = point_rows(cam, Rb, x, y, z)
        ww = rho1 * w2
        we0, we1 = ww * e0, ww * e1
        Hpp = [h + (((P0[j] * ww) * P0[k]) + ((P1[j] * ww) * P1[k])) for h, (j, k) in zip(Hpp, SYM)]
        bp = [bp[j] + (-((P0[j] * we0) + (P1[j] * we1))) for j in range(3)]
        Hxp = [[((J0[j] * ww) * P0[k]) + ((J1[j] * ww) * P1[k]) for k in range(3)] for j in range(6)]
        pose = [(J0[j] * ww) * J0[k] + (J1[j] * ww) * J1[k] for j, k in TRI]
        pose += [-(J0[j] * we0 + J1[j] * we1) for j in range(6)]
        pose.append(rho0a + rho0b)
    return Hpp, bp, Hxp, np.array(pose, f64)


def cost_of(Ra, ta, Rb, tb, cam, obs1, w1, obs2, w2, X, delta, huber):
    """per point: rho0(edge 0) + rho0(edge 1)"""
    with np.errstate(all="ignore"):
        e0, e1, _, _, _ = residual(Ra, ta, cam, obs1, X)
        ra, _ = robust(chi2_of(e0, e1, w1), delta, huber)
        e0, e1, _, _, _ = residual(Rb, tb, cam, obs2, X)
        rb, _ = robust(chi2_of(e0, e1, w2), delta, huber)
        return ra + rb


def inv3_sym(a):
    """the inverse of a symmetric 3 x 3 given as its six distinct entries (SYM order): the six distinct cofactors in the order of
    S12's adjugate (csrc/jacobi.h inv3), det by its first row, one reciprocal"""
    a00, a01, a02, a11, a12, a22 = a
    with np.errstate(all="ignore"):
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a02 * a01 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        inv = 1.0 / det
        return [c00 * inv, c01 * inv, c02 * inv, c11 * inv, c12 * inv, c22 * inv]


def sym_at(S, j, k):
    return S[SYM.index((min(j, k), max(j, k)))]


def points_of(level_sigma2, kp1_xy, kp1_octave, kp2_xy, kp2_octave, matches12, points):
    m = np.asarray(matches12)
    idx = np.flatnonzero(m >= 0)
    inv = (np.float32(1.0) / np.asarray(level_sigma2, np.float32)).astype(np.float32)   # mvInvLevelSigma2 (ORBextractor.cc:99)
    obs1 = np.asarray(kp1_xy, np.float32)[idx].astype(f64)
    obs2 = np.asarray(kp2_xy, np.float32)[m[idx]].astype(f64)
    w1 = inv[np.asarray(kp1_octave)[idx]].astype(f64)
    w2 = inv[np.asarray(kp2_octave)[m[idx]]].astype(f64)
    X = np.asarray(points, np.float32).reshape(-1, 3)[idx].astype(f64)
    return idx, obs1, w1, obs2, w2, X


def initial_bundle_adjustment(cam, level_sigma2, kp1_xy, kp1_octave, kp2_xy, kp2_octave, matches12, points, Rcw1, tcw1, Rcw2, tcw2,
                              huber_delta2=5.99, robust_kernel=True, iterations=20, trace=None):
    """-> dict(Tcw2 [4, 4] float32, points [n1, 3] float32, N, iterations, trials, exit, it_cost / it_lambda / it_trials [iterations],
    pose [12] float64, chi2 [2, N] float64, depth_positive [2, N] uint8)"""
    pts_in = np.asarray(points, np.float32).reshape(-1, 3)
    idx, obs1, w1, obs2, w2, X = points_of(level_sigma2, kp1_xy, kp1_octave, kp2_xy, kp2_octave, matches12, pts_in)
    N = len(idx)
    Ra = np.asarray(Rcw1, np.float32).reshape(9).astype(f64)
    ta = np.asarray(tcw1, np.float32).reshape(3).astype(f64)
    R = np.asarray(Rcw2, np.float32).reshape(9).astype(f64)
    t = np.asarray(tcw2, np.float32).reshape(3).astype(f64)
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3] = np.asarray(Rcw2, np.float32).reshape(3, 3)
    Tcw[:3, 3] = np.asarray(tcw2, np.float32).reshape(3)
    out = dict(Tcw2=Tcw, points=pts_in.copy(), N=N, iterations=0, trials=0, exit=EXIT_RAN_ALL, it_cost=np.zeros(0, f64),
               it_lambda=np.zeros(0, f64), it_trials=np.zeros(0, np.int32), pose=np.concatenate([R, t]), chi2=np.zeros((2, N), f64),
               depth_positive=np.zeros((2, N), np.uint8))
    if N == 0:
        return out
    assert 1 <= iterations <= MAX_ITERATIONS
    delta = delta_of(huber_delta2)
    huber = bool(robust_kernel)
    Pw = pow2_at_least(N)
    x = X[:, 0].copy(), X[:, 1].copy(), X[:, 2].copy()
    lam, ni, cur = 0.0, 2.0, 0.0
    n_it, n_trials, exit_kind = 0, 0, EXIT_RAN_ALL
    it_cost, it_lambda, it_trials = [], [], []
    args = (cam, obs1, w1, obs2, w2)
    with np.errstate(all="ignore"):
        for k in range(iterations):
            n_it += 1
            Xn = np.stack(x, 1)
            Hpp, bp, Hxp, pose = linearise(Ra, ta, R, t, *args, Xn, delta, huber)
            s = tree_sum(pose, Pw)
            H, b, cur = s[:21], s[21:27], float(s[27])
            diag = [H[TRI.index((j, j))] for j in range(6)]
            if k == 0:
                m = 0.0
                for j in range(6):
                    if diag[j] > m:
                        m = float(diag[j])
                for kk in (0, 3, 5):
                    v = Hpp[kk][np.greater(Hpp[kk], 0.0)]   # a NaN fails `>` and is never kept
                    if len(v) and float(v.max()) > m:
                        m = float(v.max())
                lam = float(f64(1e-5) * f64(m))
                ni = 2.0
            rho, q = 0.0, 0
            while True:
                fl = f64(lam)
                D = list(Hpp)
                for kk in (0, 3, 5):
                    D[kk] = Hpp[kk] + fl
                Dinv = inv3_sym(D)
                if not bool(np.all(np.isfinite(np.array(Dinv)))):
                    COUNTS["nonfinite_block"] += 1
                B = [[(Hxp[j][0] * sym_at(Dinv, 0, kk) + Hxp[j][1] * sym_at(Dinv, 1, kk)) + Hxp[j][2] * sym_at(Dinv, 2, kk) for kk in range(3)]
                     for j in range(6)]
                terms = [(B[j][0] * Hxp[kk][0] + B[j][1] * Hxp[kk][1]) + B[j][2] * Hxp[kk][2] for j, kk in TRI]
                terms += [(B[j][0] * bp[0] + B[j][1] * bp[1]) + B[j][2] * bp[2] for j in range(6)]
                Ts = tree_sum(np.array(terms, f64), Pw)
                S = np.zeros((6, 6), f64)
                for (j, kk), h, sv in zip(TRI, H, Ts[:21]):
                    val = (h + fl) - sv if j == kk else h - sv
                    S[j, kk] = val
                    S[kk, j] = val
                g = np.array([b[j] - Ts[21 + j] for j in range(6)], f64)
                dx, ok = ldlt_solve6(S, g)
                c = []
                for kk in range(3):
                    acc = np.zeros(N, f64)
                    for j in range(6):
                        acc = acc + Hxp[j][kk] * dx[j]
                    c.append(bp[kk] - acc)
                dp = [(sym_at(Dinv, kk, 0) * c[0] + sym_at(Dinv, kk, 1) * c[1]) + sym_at(Dinv, kk, 2) * c[2] for kk in range(3)]
                Rn, tn = apply_update(dx, R, t)
                xn = [x[kk] + dp[kk] for kk in range(3)]
                tc = cost_of(Ra, ta, Rn, tn, *args, np.stack(xn, 1), delta, huber)
                ps = ((dp[0] * ((fl * dp[0]) + bp[0])) + (dp[1] * ((fl * dp[1]) + bp[1]))) + (dp[2] * ((fl * dp[2]) + bp[2]))
                T2 = tree_sum(np.array([tc, ps], f64), Pw)
                tmp = float(T2[0])
                if not ok:
                    COUNTS["not_ok"] += 1
                    tmp = DBL_MAX
                scale = f64(0.0)
                for j in range(6):
                    scale = scale + dx[j] * ((fl * dx[j]) + b[j])
                scale = (scale + T2[1]) + f64(1e-3)
                rho = float((f64(cur) - f64(tmp)) / scale)
                n_trials += 1
                q += 1
                if rho > 0 and math.isfinite(tmp):
                    R, t, x = Rn, tn, xn
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
            it_cost.append(cur)
            it_lambda.append(lam)
            it_trials.append(q)
            if q == MAX_TRIALS:
                exit_kind = EXIT_TRIALS
                break
            if rho == 0:
                exit_kind = EXIT_RHO_ZERO
                break
        Xf = np.stack(x, 1)
        chi, dep = np.zeros((2, N), f64), np.zeros((2, N), np.uint8)
        for e, (Re, te, ob, w) in enumerate(((Ra, ta, obs1, w1), (R, t, obs2, w2))):
            e0, e1, _, _, z = residual(Re, te, cam, ob, Xf)
            chi[e] = chi2_of(e0, e1, w)
            dep[e] = z > 0.0
        Tcw[:3, :3] = R.reshape(3, 3).astype(np.float32)
        Tcw[:3, 3] = t.astype(np.float32)
        out["points"][idx] = Xf.astype(np.float32)
    out.update(iterations=n_it, trials=n_trials, exit=exit_kind, it_cost=np.array(it_cost, f64), it_lambda=np.array(it_lambda, f64),
               it_trials=np.array(it_trials, np.int32), pose=np.concatenate([R, t]), chi2=chi, depth_positive=dep)
    return out


def median_depth_scale(out, Rcw1, tcw1, matches12, inertial=False, min_points=50):
    """the adaptor's host step in binary32: KeyFrame::ComputeSceneMedianDepth(2) (src/KeyFrame.cc:859-892) with pose 1 on the returned
    points, then the rescale of src/Tracking.cc:700-729 -> (ok, tcw2 [3] float32, points [n1, 3] float32, median)"""
    f32 = np.float32
    idx = np.flatnonzero(np.asarray(matches12) >= 0)
    pts = np.asarray(out["points"], f32).reshape(-1, 3)
    R = np.asarray(Rcw1, f32).reshape(9)
    tz = f32(np.asarray(tcw1, f32).reshape(3)[2])
    t2 = out["Tcw2"][:3, 3].astype(f32)
    if len(idx) == 0:
        return False, t2, pts, f32(0)
    with np.errstate(all="ignore"):
        z = ((R[6] * pts[idx, 0] + R[7] * pts[idx, 1]) + R[8] * pts[idx, 2]) + tz
    if bool(np.isnan(z).any()):
        return False, t2, pts, f32(np.nan)
    med = f32(np.sort(z)[(len(z) - 1) // 2])
    if med < 0 or len(idx) < min_points:
        return False, t2, pts, med
    with np.errstate(all="ignore"):
        inv = (f32(4.0) if inertial else f32(1.0)) / med
        sp = pts.copy()
        sp[idx] = pts[idx] * inv
        return True, (t2 * inv).astype(f32), sp, med

"""SPEC DECISION S20, normative: Optimizer::PoseInertialOptimizationLastFrame (src/Optimizer.cc:3846-4275) for the
branch this fork takes -- one pinhole camera, mono edges, one EdgeInertial with all six vertices free, EdgeGyroRW, EdgeAccRW,
EdgePriorPoseImu -- and Optimizer::Marginalize (:2882-2962), written from those lines, src/G2oTypes.cc:514-594 and :720-760,
include/G2oTypes.h:508-518, 634-751, src/ImuTypes.cc:278-312 and the text of S20, not from the kernel.  The rules are S14's and S19's
(see pose_inertial_ref.py, whose SO(3) functions, mono edge, update and scoring are used as they stand); g2o and Sophus are empty
submodules of the reference, so parity with a g2o build is unpinned.

marginalize_svd is the INDEPENDENT form of the marginalisation: a literal numpy rendering of :2882-2962 with numpy.linalg.svd.
"""
import collections

import numpy as np

import pose_inertial_ref as R19
from poseopt_ref import delta_of, edges_of, matvec3, mul3, pow2_at_least, robust

f64 = np.float64
f32 = np.float32
N = 30
COUNTS = collections.Counter()
TRI6 = R19.TRI6
EYE = np.array(R19.EYE, f64)
MARG_SWEEPS = 9
MARG_THRESHOLD = 1e-6

PARAMS = dict(chi2=(5.991, 5.991, 5.991, 5.991), close_factor=1.5, close_depth=10.0, recover_chi2=24.0, recover_below=30,
              huber_delta2=5.991, prior_huber_delta=5.0, inlier_threshold=8, iterations=15, rounds=4, rec_init=0, gravity=9.81)

# EdgeInertial's column blocks in the reference's order: pose 1 rotation, pose 1 translation, v1, bg1, ba1, pose 2 rotation, pose 2
# translation, v2; and where each starts in the solver's order (the frame 0-14, the previous frame 15-29)
SOLVER_OF_REF = np.concatenate([np.arange(15, 30), np.arange(0, 9)])   # reference index 0..23 -> solver index
REF24_OF_SOLVER = {int(s): r for r, s in enumerate(SOLVER_OF_REF)}


def d32(a, n):
    return np.asarray(a, f32).reshape(n)


class Link:
    """orbfe_imu_link_free: floats stay binary32 where ImuTypes.cc computes in binary32"""

    def __init__(self, link):
        g = lambda k, n: d32(link[k], n)
        self.dR0, self.dV0, self.dP0 = g("dR0", 9), g("dV0", 3), g("dP0", 3)
        self.bg0, self.ba0 = g("bg0", 3), g("ba0", 3)
        self.JRg, self.JVg, self.JVa, self.JPg, self.JPa = (g(k, 9) for k in ("JRg", "JVg", "JVa", "JPg", "JPa"))
        self.dt = f64(f32(link["dt"]))
        self.Rcb, self.tcb, self.tbc = g("Rcb", 9).astype(f64), g("tcb", 3).astype(f64), g("tbc", 3).astype(f64)
        self.info9 = np.asarray(link["info9"], f64).reshape(81)
        self.infoG, self.infoA = np.asarray(link["infoG"], f64).reshape(9), np.asarray(link["infoA"], f64).reshape(9)


class Prior:
    def __init__(self, prior):
        g = lambda k, n: np.asarray(prior[k], f64).reshape(n)
        self.Rwb, self.twb, self.vwb, self.bg, self.ba, self.H = g("Rwb", 9), g("twb", 3), g("vwb", 3), g("bg", 3), g("ba", 3), g("H", 225)


def state_vector(S1, S2):
    return np.concatenate([S2.vector(), S1.vector()])


def mv32(M, x):
    with np.errstate(all="ignore"):
        return np.array([(M[3 * i] * x[0] + M[3 * i + 1] * x[1]) + M[3 * i + 2] * x[2] for i in range(3)], f32)


def deltas(K, bg1, ba1):
    """GetDeltaRotation / Velocity / Position at the bias (bg1, ba1) (ImuTypes.cc:285-312) -> dR [9], dV, dP binary64, dbg binary64.
    Stated departure: dR = (double) dR0 . ExpSO3((double) rot_lie) in binary64 without NormalizeRotation."""
    with np.errstate(all="ignore"):
        dbg = np.asarray(bg1, f64).astype(f32) - K.bg0
        dba = np.asarray(ba1, f64).astype(f32) - K.ba0
        dV = (K.dV0 + mv32(K.JVg, dbg)) + mv32(K.JVa, dba)
        dP = (K.dP0 + mv32(K.JPg, dbg)) + mv32(K.JPa, dba)
        rot = mv32(K.JRg, dbg)
        dR = mul3(K.dR0.astype(f64), R19.exp_so3(rot.astype(f64)))
    assert dV.dtype == f32 and dP.dtype == f32 and rot.dtype == f32
    return dR, dV.astype(f64), dP.astype(f64), dbg.astype(f64)


def delta_rotation_f32(K, bg1):
    """the reference's own line, NormalizeRotation(dR * SO3f::exp(rot_lie)), in plain binary32 numpy: Rodrigues and an SVD.  Only to
    measure how far the stated departure is from it (tests/test_pose_inertial_prev.py)."""
    dbg = np.asarray(bg1, f64).astype(f32) - K.bg0
    rot = mv32(K.JRg, dbg)
    th = f32(np.sqrt(f32(rot @ rot)))
    W = np.array([[0, -rot[2], rot[1]], [rot[2], 0, -rot[0]], [-rot[1], rot[0], 0]], f32)
    if th < f32(1e-10):
        E = np.eye(3, dtype=f32) + W
    else:
        E = np.eye(3, dtype=f32) + f32(np.sin(th) / th) * W + f32((f32(1) - np.cos(th)) / (th * th)) * (W @ W)
    M = K.dR0.reshape(3, 3) @ E.astype(f32)
    U, _, Vt = np.linalg.svd(M.astype(f32))
    return (U @ Vt).astype(f32).reshape(9)


def hat(v):
    return R19.hat(v)


PRESENT = {0: (0, 1, 2), 1: (2,), 2: (1, 2), 3: (0, 1, 2), 4: (1, 2), 5: (0,), 6: (2,), 7: (1,)}   # column block -> row blocks


def inertial_edge(K, gravity, S1, S2):
    """-> (H24 [24, 24], b24 [24], e9): J^T info9 J and -J^T (info9 e9) in the reference's order.  Errors :528-531, Jacobian blocks
    :558-593.  Block pair (p, q), p <= q: the present row blocks in ascending order (rp, then rq), each J[rp][p]^T (info9[rp][rq]
    J[rq][q]); the diagonal pairs' upper triangle, everything mirrored."""
    with np.errstate(all="ignore"):
        dR, dV, dP, dbg = deltas(K, S1.bg, S1.ba)
        Rwb1, Rwb2 = S1.Rwb, S2.Rwb
        Rbw1 = R19.transpose3(Rwb1)
        eR = mul3(mul3(R19.transpose3(dR), Rbw1), Rwb2)
        er = R19.log_so3(eR)
        dt = K.dt
        g = np.array([0.0, 0.0, -gravity], f64)
        a = (S2.v - S1.v) - g * dt
        base = (S2.twb - S1.twb) - S1.v * dt
        c = base - g * dt * dt / 2.0
        c2 = base - 0.5 * g * dt * dt
        ra, rc, rc2 = matvec3(Rbw1, a), matvec3(Rbw1, c), matvec3(Rbw1, c2)
        e9 = np.concatenate([er, ra - dV, rc - dP])
        Om = K.info9
        Or = np.zeros(9, f64)
        for r in range(9):
            acc = Om[9 * r] * e9[0]
            for q in range(1, 9):
                acc = acc + Om[9 * r + q] * e9[q]
            Or[r] = -acc
        invJr = R19.inverse_right_jacobian_so3(er)
        JRg = K.JRg.astype(f64)
        J = {}
        J[0, 0] = mul3(mul3(-invJr, R19.transpose3(Rwb2)), Rwb1)
        J[1, 0] = hat(ra)
        J[2, 0] = hat(rc2)
        J[2, 1] = -EYE
        J[1, 2] = -Rbw1
        J[2, 2] = -Rbw1 * dt
        J[0, 3] = mul3(mul3(mul3(-invJr, R19.transpose3(eR)), R19.right_jacobian_so3(matvec3(JRg, dbg))), JRg)
        J[1, 3] = -K.JVg.astype(f64)
        J[2, 3] = -K.JPg.astype(f64)
        J[1, 4] = -K.JVa.astype(f64)
        J[2, 4] = -K.JPa.astype(f64)
        J[0, 5] = invJr
        J[2, 6] = mul3(Rbw1, Rwb2)
        J[1, 7] = Rbw1
        assert sorted(J) == sorted((r, c) for c, rs in PRESENT.items() for r in rs)
        H, b = np.zeros((24, 24), f64), np.zeros(24, f64)
        for p in range(8):
            acc = None
            for rp in PRESENT[p]:
                t = matvec3(R19.transpose3(J[rp, p]), Or[3 * rp:3 * rp + 3])
                acc = t if acc is None else acc + t
            b[3 * p:3 * p + 3] = acc
            for q in range(p, 8):
                Hb = None
                for rp in PRESENT[p]:
                    Jt = R19.transpose3(J[rp, p])
                    for rq in PRESENT[q]:
                        W = np.array([Om[9 * (3 * rp + i) + (3 * rq + j)] for i in range(3) for j in range(3)], f64)
                        M = mul3(Jt, mul3(W, J[rq, q]))
                        Hb = M if Hb is None else Hb + M
                for i in range(3):
                    for j in range(3):
                        if q > p or j >= i:
                            H[3 * p + i, 3 * q + j] = Hb[3 * i + j]
                            H[3 * q + j, 3 * p + i] = Hb[3 * i + j]
    return H, b, e9


def prior_edge(Pr, delta, S1, unit=False):
    """EdgePriorPoseImu (:731-760) -> (Hp [15, 15], bp [15], chi2, Huber weight).  chi2 = e^T (H e), sums in column order; S14's robust
    with delta; the weight multiplies H entry by entry (1 with `unit`: GetHessian carries none); the identity blocks are not multiplied."""
    with np.errstate(all="ignore"):
        Rpt = R19.transpose3(Pr.Rwb)
        Rr = mul3(Rpt, S1.Rwb)
        er = R19.log_so3(Rr)
        e = np.concatenate([er, matvec3(Rpt, S1.twb - Pr.twb), S1.v - Pr.vwb, S1.bg - Pr.bg, S1.ba - Pr.ba])
        He = np.zeros(15, f64)
        for r in range(15):
            acc = Pr.H[15 * r] * e[0]
            for q in range(1, 15):
                acc = acc + Pr.H[15 * r + q] * e[q]
            He[r] = acc
        chi2 = e[0] * He[0]
        for r in range(1, 15):
            chi2 = chi2 + e[r] * He[r]
        _, rho1 = robust(np.array([chi2], f64), delta, True)
        rho1 = f64(rho1[0])
        w = f64(1.0) if unit else rho1
        Orw = w * -He
        Jb = [R19.inverse_right_jacobian_so3(er), Rr]
        Hp, bp = np.zeros((15, 15), f64), np.zeros(15, f64)
        for p in range(5):
            o = Orw[3 * p:3 * p + 3]
            bp[3 * p:3 * p + 3] = matvec3(R19.transpose3(Jb[p]), o) if p < 2 else o
            for q in range(p, 5):
                M = np.array([w * Pr.H[15 * (3 * p + i) + (3 * q + j)] for i in range(3) for j in range(3)], f64)
                if q < 2:
                    M = mul3(M, Jb[q])
                if p < 2:
                    M = mul3(R19.transpose3(Jb[p]), M)
                for i in range(3):
                    for j in range(3):
                        if q > p or j >= i:
                            Hp[3 * p + i, 3 * q + j] = M[3 * i + j]
                            Hp[3 * q + j, 3 * p + i] = M[3 * i + j]
    return Hp, bp, f64(chi2), rho1


def sym_upper(M):
    return R19.sym_upper(M)


def system(K, Pr, prm, gravity, S1, S2, sums):
    """the 30 x 30 system in the solver's order.  Per entry, the reference's edge insertion order: the mono tree sum, the inertial edge,
    the gyro random walk, the accelerometer random walk, the prior; entries no edge touches are +0.0."""
    H24, b24, _ = inertial_edge(K, gravity, S1, S2)
    Hp, bp, _, _ = prior_edge(Pr, prm["prior_huber_delta"], S1)
    with np.errstate(all="ignore"):
        G, A = sym_upper(K.infoG), sym_upper(K.infoA)
        rwG, rwA = matvec3(K.infoG, S2.bg - S1.bg), matvec3(K.infoA, S2.ba - S1.ba)
        terms = [[[] for _ in range(N)] for _ in range(N)]
        rhs = [[] for _ in range(N)]
        for (j, k), s in zip(TRI6, sums[:21]):
            terms[j][k].append(s)
        for j in range(6):
            rhs[j].append(sums[21 + j])
        for r in range(24):
            i = int(SOLVER_OF_REF[r])
            rhs[i].append(b24[r])
            for c in range(24):
                j = int(SOLVER_OF_REF[c])
                if i <= j:
                    terms[i][j].append(H24[r, c])
        for info, vec, cur, prv in ((G, rwG, 9, 24), (A, rwA, 12, 27)):
            for a in range(3):
                rhs[cur + a].append(-vec[a])
                rhs[prv + a].append(vec[a])
                for b in range(3):
                    if a <= b:
                        terms[cur + a][cur + b].append(info[a, b])
                        terms[prv + a][prv + b].append(info[a, b])
                    terms[cur + a][prv + b].append(-info[a, b])
        for a in range(15):
            rhs[15 + a].append(bp[a])
            for b in range(a, 15):
                terms[15 + a][15 + b].append(Hp[a, b])
        H, b = np.zeros((N, N), f64), np.zeros(N, f64)
        for i in range(N):
            acc = None
            for t in rhs[i]:
                acc = t if acc is None else acc + t
            b[i] = acc
            for j in range(i, N):
                acc = None
                for t in terms[i][j]:
                    acc = t if acc is None else acc + t
                H[i, j] = H[j, i] = f64(0.0) if acc is None else acc
    return H, b


def ldlt_solve(A, b):
    """csrc/ldlt.h ldlt_solve_n (pose_inertial_ref.ldlt_solve), the trailing update of a row taken elementwise by numpy: the same
    operations in the same order"""
    n = len(b)
    A = np.array(A, f64)
    L, d, perm = np.zeros((n, n), f64), np.zeros(n, f64), list(range(n))
    with np.errstate(all="ignore"):
        for k in range(n):
            best, best_abs = k, abs(A[k, k])
            for i in range(k + 1, n):
                if abs(A[i, i]) > best_abs:
                    best, best_abs = i, abs(A[i, i])
            if best != k:
                A[[k, best], :] = A[[best, k], :]
                L[[k, best], :] = L[[best, k], :]
                perm[k], perm[best] = perm[best], perm[k]
                A[:, [k, best]] = A[:, [best, k]]
            dk = A[k, k]
            d[k] = dk
            col = A[:, k].copy()
            for i in range(k + 1, n):
                li = f64(0.0) if dk == 0.0 else col[i] / dk
                L[i, k] = li
                val = A[i, k + 1:i + 1] - li * col[k + 1:i + 1]
                A[i, k + 1:i + 1] = val
                A[k + 1:i + 1, i] = val
        z = np.zeros(n, f64)
        for i in range(n):
            acc = f64(b[perm[i]])
            for j in range(i):
                acc = acc - L[i, j] * z[j]
            z[i] = acc
        xs = np.zeros(n, f64)
        for i in range(n - 1, -1, -1):
            acc = f64(0.0) if d[i] == 0.0 else z[i] / d[i]
            for j in range(i + 1, n):
                acc = acc - L[j, i] * xs[j]
            xs[i] = acc
    x = np.zeros(n, f64)
    for i in range(n):
        x[perm[i]] = xs[i]
    return x, bool(np.all(d > 0.0))


def hessian30(K, Pr, gravity, S1, S2, sums):
    """the Hessian handed out (:4216-4264), reference order, in the reference's addition order: ((0 + inertial) + random walk) + prior)
    + T.  The random-walk blocks are the informations as handed in; the prior carries no robust weight; T is the mono tree sum."""
    H24, _, _ = inertial_edge(K, gravity, S1, S2)
    Hp, _, _, _ = prior_edge(Pr, 1.0, S1, unit=True)
    with np.errstate(all="ignore"):
        H = np.zeros((N, N), f64)
        H[:24, :24] = H[:24, :24] + H24
        for info, a, b in ((K.infoG.reshape(3, 3), 9, 24), (K.infoA.reshape(3, 3), 12, 27)):
            H[a:a + 3, a:a + 3] = H[a:a + 3, a:a + 3] + info
            H[a:a + 3, b:b + 3] = H[a:a + 3, b:b + 3] + -info
            H[b:b + 3, a:a + 3] = H[b:b + 3, a:a + 3] + -info
            H[b:b + 3, b:b + 3] = H[b:b + 3, b:b + 3] + info
        H[:15, :15] = H[:15, :15] + Hp
        T = np.zeros((6, 6), f64)
        for (j, k), s in zip(TRI6, sums[:21]):
            T[j, k] = T[k, j] = s
        H[15:21, 15:21] = H[15:21, 15:21] + T
    return H


def jacobi_eig(Hbb, sweeps=MARG_SWEEPS):
    """the pinned symmetric eigen-decomposition: Hbb's upper triangle mirrored, `sweeps` cyclic sweeps over (0,1) (0,2) .. (13,14),
    jacobi.h's angle, apq == 0.0 skipped, no data-dependent exit -> (diagonal, V)"""
    n = Hbb.shape[0]
    M = np.array([[Hbb[min(i, j), max(i, j)] for j in range(n)] for i in range(n)], f64)
    V = np.eye(n, dtype=f64)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = M[p, q]
                    if apq == 0.0:
                        continue
                    theta = (M[q, q] - M[p, p]) / (2.0 * apq)
                    t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    sn = t * c
                    a, b = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * a - sn * b
                    M[:, q] = sn * a + c * b
                    a, b = M[p, :].copy(), M[q, :].copy()
                    M[p, :] = c * a - sn * b
                    M[q, :] = sn * a + c * b
                    a, b = V[:, p].copy(), V[:, q].copy()
                    V[:, p] = c * a - sn * b
                    V[:, q] = sn * a + c * b
    return np.diagonal(M).copy(), V


def marginalize(H, sweeps=MARG_SWEEPS):
    """S20: Hp = Hcc - (Hcb pinv(Hbb)) Hbc, b = rows 0-14, c = rows 15-29; pinv = (V L^+) V^T with lambda inverted when
    |lambda| > 1e-6, else 0; every product a sequential sum in column order"""
    H = np.asarray(H, f64).reshape(N, N)
    lam, V = jacobi_eig(H[:15, :15], sweeps)
    with np.errstate(all="ignore"):
        inv = np.array([1.0 / l if abs(l) > MARG_THRESHOLD else 0.0 for l in lam], f64)
        if np.any(~(np.abs(lam) > MARG_THRESHOLD)):
            COUNTS["marg_below_threshold"] += 1

        def seq(A, B):
            acc = A[:, 0][:, None] * B[0, :][None, :]
            for k in range(1, A.shape[1]):
                acc = acc + A[:, k][:, None] * B[k, :][None, :]
            return acc
        P = seq(V * inv[None, :], V.T.copy())
        T = seq(H[15:, :15], P)
        return H[15:, 15:] - seq(T, H[:15, 15:])


def marginalize_svd(H, start=0, end=14):
    """a literal rendering of Optimizer::Marginalize (:2882-2962) with numpy.linalg.svd -> the full matrix it returns"""
    H = np.asarray(H, f64)
    a, b, c = start, end - start + 1, H.shape[1] - (end + 1)
    Hn = np.zeros_like(H)
    if a > 0:
        Hn[0:a, 0:a] = H[0:a, 0:a]
        Hn[0:a, a + c:a + c + b] = H[0:a, a:a + b]
        Hn[a + c:a + c + b, 0:a] = H[a:a + b, 0:a]
    if a > 0 and c > 0:
        Hn[0:a, a:a + c] = H[0:a, a + b:a + b + c]
        Hn[a:a + c, 0:a] = H[a + b:a + b + c, 0:a]
    if c > 0:
        Hn[a:a + c, a:a + c] = H[a + b:, a + b:]
        Hn[a:a + c, a + c:] = H[a + b:, a:a + b]
        Hn[a + c:, a:a + c] = H[a:a + b, a + b:]
    Hn[a + c:, a + c:] = H[a:a + b, a:a + b]
    U, s, Vt = np.linalg.svd(Hn[a + c:, a + c:])
    s_inv = np.where(s > 1e-6, 1.0 / np.where(s > 1e-6, s, 1.0), 0.0)
    inv_hb = Vt.T @ np.diag(s_inv) @ U.T
    Hn[0:a + c, 0:a + c] = Hn[0:a + c, 0:a + c] - Hn[0:a + c, a + c:] @ inv_hb @ Hn[a + c:, 0:a + c]
    Hn[a + c:, a + c:] = 0.0
    Hn[0:a + c, a + c:] = 0.0
    Hn[a + c:, 0:a + c] = 0.0
    res = np.zeros_like(H)
    if a > 0:
        res[0:a, 0:a] = Hn[0:a, 0:a]
        res[0:a, a:a + b] = Hn[0:a, a + c:]
        res[a:a + b, 0:a] = Hn[a + c:, 0:a]
    if a > 0 and c > 0:
        res[0:a, a + b:] = Hn[0:a, a:a + c]
        res[a + b:, 0:a] = Hn[a:a + c, 0:a]
    if c > 0:
        res[a + b:, a + b:] = Hn[a:a + c, a:a + c]
        res[a + b:, a:a + b] = Hn[a:a + c, a + c:]
        res[a:a + b, a + b:] = Hn[a + c:, a:a + c]
    res[a:a + b, a:a + b] = Hn[a + c:, a + c:]
    return res


def prev_state(link):
    """the previous frame's four vertices at the start: the link's floats as binary64 (Rcw / tcw are not its own: never read)"""
    return R19.State(np.zeros(9), np.zeros(3), link["Rwb1"], link["twb1"], link["v1"], link["bg1"], link["ba1"])


def pose_inertial_optimization_last_frame(cam, level_sigma2, kp_xy, kp_octave, mp_index, points, track_depth, link, prior, Rcw, tcw, Rwb,
                                          twb, v, bg, ba, **kw):
    """-> dict(Rwb [9], twb, v, bg, ba float32 (the frame); H30 [30, 30], Hprior [15, 15] float64; outlier [n] uint8; n_inliers;
    accepted; N_e; rounds_run; recovered; round_iterations, round_ok, round_nbad [rounds_run]; round_state [rounds_run, 42] float64;
    round_prior_chi2, round_prior_weight [rounds_run]; round_outlier [rounds_run, N_e] uint8)"""
    prm = dict(PARAMS)
    prm.update(kw)
    n = len(mp_index)
    first, obs, w, Xw = edges_of(level_sigma2, kp_xy, kp_octave, mp_index, points)
    Ne = len(first)
    P = pow2_at_least(Ne)
    K, Pr = Link(link), Prior(prior)
    S2 = R19.State(Rcw, tcw, Rwb, twb, v, bg, ba)
    S1 = prev_state(link)
    gravity = f64(f32(prm["gravity"]))
    delta = delta_of(prm["huber_delta2"])
    pdelta = f64(prm["prior_huber_delta"])
    prm["prior_huber_delta"] = pdelta
    close = np.asarray(track_depth, f32)[np.asarray(mp_index)[first]] < f32(prm["close_depth"])
    active = np.ones(Ne, bool)
    bad = np.zeros(Ne, bool)
    rec = {k: [] for k in ("iterations", "ok", "nbad", "state", "outlier", "pchi2", "pw")}
    n_bad = 0
    for rnd in range(prm["rounds"]):
        huber = rnd <= 2   # setRobustKernel(0) after round index 2 touches the mono edges only (:4130)
        n_it, ok = 0, True
        for _ in range(prm["iterations"]):
            n_it += 1
            sums = R19.mono_sums(S2, K, cam, obs, w, Xw, active, delta, huber, P)
            H, b = system(K, Pr, prm, gravity, S1, S2, sums)
            dx, ok = ldlt_solve(H, b)
            if not ok:
                COUNTS["not_ok"] += 1
                break
            R19.update(K, dx[:15], S2)
            R19.update(K, dx[15:], S1)
        thr = f32(prm["chi2"][rnd])
        thr_close = f32(f64(prm["close_factor"]) * f64(thr))
        chi2, front = R19.score(S2, cam, obs, w, Xw)
        with np.errstate(all="ignore"):
            bad = ((chi2 > thr) & ~close) | (close & (chi2 > thr_close)) | ~front
        active = ~bad
        n_bad = int(bad.sum())
        _, _, pchi2, pw = prior_edge(Pr, pdelta, S1)
        if pw < 1.0:
            COUNTS["prior_huber_active"] += 1
        rec["iterations"].append(n_it)
        rec["ok"].append(int(ok))
        rec["nbad"].append(n_bad)
        rec["state"].append(state_vector(S1, S2))
        rec["outlier"].append(bad.astype(np.uint8))
        rec["pchi2"].append(pchi2)
        rec["pw"].append(pw)
        if Ne + 4 < 10:   # optimizer.edges().size() < 10 (:4168): the mono edges and the four others
            COUNTS["few_edges_break"] += 1
            break
    recovered = 0
    if Ne - n_bad < prm["recover_below"] and not prm["rec_init"]:   # (:4175-4203)
        COUNTS["recovery"] += 1
        recovered = 1
        chi2, _ = R19.score(S2, cam, obs, w, Xw)
        with np.errstate(all="ignore"):
            good = chi2 < f32(prm["recover_chi2"])
        bad = bad & ~good
        n_bad = int((~good).sum())
    valid = Ne - n_bad
    accepted = int(valid >= prm["inlier_threshold"])
    COUNTS["accepted" if accepted else "rejected"] += 1
    sums = R19.mono_sums(S2, K, cam, obs, w, Xw, ~bad, delta, False, P)
    H30 = hessian30(K, Pr, gravity, S1, S2, sums)
    Hprior = marginalize(H30)
    nr = len(rec["iterations"])
    outlier = np.zeros(n, np.uint8)
    outlier[first] = bad.astype(np.uint8)
    with np.errstate(all="ignore"):
        out = dict(Rwb=S2.Rwb.astype(f32), twb=S2.twb.astype(f32), v=S2.v.astype(f32), bg=S2.bg.astype(f32), ba=S2.ba.astype(f32),
                   H30=H30, Hprior=Hprior, outlier=outlier, n_inliers=valid, accepted=accepted, N_e=Ne, rounds_run=nr,
                   recovered=recovered, round_iterations=np.array(rec["iterations"], np.int32), round_ok=np.array(rec["ok"], np.int32),
                   round_nbad=np.array(rec["nbad"], np.int32), round_state=np.array(rec["state"], f64).reshape(nr, 42),
                   round_prior_chi2=np.array(rec["pchi2"], f64), round_prior_weight=np.array(rec["pw"], f64),
                   round_outlier=np.array(rec["outlier"], np.uint8).reshape(nr, Ne))
    out["state64"] = state_vector(S1, S2)
    return out

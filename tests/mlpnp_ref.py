"""SPEC DECISION S13 restated for the tests: a fresh MLPnPsolver(F, vpMapPointMatches) + SetRansacParameters
+ one iterate(nIterations) (src/MLPnPsolver.cpp; the call: src/Tracking.cc:838-845), written from that file.

`ransac` is the pinned sequence and the NORMATIVE definition: numpy binary64 / binary32 where the C++ is double / float, ONE IEEE
operation per operator (numpy evaluates every operator on its own, so nothing is contracted; element-wise array operations round
exactly like scalars, the arrays only run all hypotheses at once), every sum sequential from 0.0 in ascending order, the
decompositions by fixed Jacobi sequences, sin / cos / acos / cbrt by the sequences below (+ - x / sqrt and the exact floor / frexp /
ldexp only).  `ransac_f64` is the same function on numpy.linalg.svd / eigh / solve and numpy's sin / cos / arccos / cbrt: what S13 is
measured against (the reference's Eigen decompositions cannot be built here).

The S5 / S10 camera pieces (unproject, project) are those of newpoints_ref (the oracle's exported functions for KannalaBrandt8)."""
import math

import numpy as np

import newpoints_ref as NR
import twoview_ref as T

f32 = np.float32
f64 = np.float64
EPS = float(np.finfo(f64).eps)
SWEEPS12 = 12        # S13: fixed (results stop changing at 7 on the test scenes)
SWEEPS9 = T.SWEEPS   # the planar branch's 9 x 9 null vector is S12's sequence as it stands
EXIT_ABORT, EXIT_REFINED, EXIT_BEST, EXIT_FAILED = 0, 1, 2, 3
GN_MAXIT, GN_SPURIOUS, GN_CONVERGED = 0, 1, 2   # how mlpnp_gn left its loop: it_cnt == maxIt, :743, :747
RANK_TOL = 3.0 * EPS  # Eigen's FullPivHouseholderQR threshold for a 3 x 3: pivot > 3 eps * largest pivot

# round r of the 12 x 12 sequence (r = 0 .. 10): {r, 11} and {(r + k) mod 11, (r - k) mod 11} for k = 1 .. 5 -- the circle
# method: 6 disjoint pairs per round, every pair of 0 .. 11 exactly once per sweep
ROUNDS12 = [[(r, 11)] + [tuple(sorted(((r + k) % 11, (r - k) % 11))) for k in range(1, 6)] for r in range(11)]
assert len({p for r in ROUNDS12 for p in r}) == 66 and all(len({x for p in r for x in p}) == 12 for r in ROUNDS12)

# ---------------------------------------------------------------------------------------------------------------------
# binary64 sin / cos / acos / cbrt (the same constants as csrc/spec_math.h: test_mlpnp.py compares the two tables)
# ---------------------------------------------------------------------------------------------------------------------
_h = float.fromhex
TWO_OVER_PI = _h("0x1.45f306dc9c883p-1")
PIO2_1, PIO2_2, PIO2_3 = _h("0x1.921fb54400000p+0"), _h("0x1.0b4611a600000p-34"), _h("0x1.3198a2e037073p-69")  # pi / 2 in three parts
PIO2_HI, PIO2_LO = _h("0x1.921fb54442d18p+0"), _h("0x1.1a62633145c07p-54")
PI_HI, PI_LO = _h("0x1.921fb54442d18p+1"), _h("0x1.1a62633145c07p-53")
SIN_C = [_h(s) for s in ("-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19",
                         "-0x1.ae64567f544e4p-26", "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41", "0x1.952c77030ad4ap-49",
                         "-0x1.2f49b46814157p-57")]  # (-1)^k / (2k + 1)!, k = 1 .. 9
COS_C = [_h(s) for s in ("-0x1.0000000000000p-1", "0x1.5555555555555p-5", "-0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-16",
                         "-0x1.27e4fb7789f5cp-22", "0x1.1eed8eff8d898p-29", "-0x1.93974a8c07c9dp-37", "0x1.ae7f3e733b81fp-45",
                         "-0x1.6827863b97d97p-53", "0x1.e542ba4020225p-62")]  # (-1)^k / (2k)!, k = 1 .. 10
ASIN_C = [_h(s) for s in (
    "0x1.5555555555555p-3", "0x1.3333333333333p-4", "0x1.6db6db6db6db7p-5", "0x1.f1c71c71c71c7p-6", "0x1.6e8ba2e8ba2e9p-6",
    "0x1.1c4ec4ec4ec4fp-6", "0x1.c99999999999ap-7", "0x1.7a87878787878p-7", "0x1.3fde50d79435ep-7", "0x1.12ef3cf3cf3cfp-7",
    "0x1.df3bd37a6f4dfp-8", "0x1.a6863d70a3d71p-8", "0x1.782dda12f684cp-8", "0x1.51ba308d3dcb1p-8", "0x1.31683bdef7bdfp-8",
    "0x1.15ee9d45d1746p-8", "0x1.fcaf8fb6db6dbp-9", "0x1.d3d2a8e0dd67dp-9", "0x1.b026f57b13b14p-9", "0x1.90cb77f60c7cep-9",
    "0x1.750de64d7d05fp-9", "0x1.5c5f56efaaaabp-9", "0x1.464c0950f7d47p-9", "0x1.3275586c5f2f0p-9", "0x1.208d3570ae5a6p-9",
    "0x1.1052bc5fa960ap-9", "0x1.018f963c229bfp-9", "0x1.e82be60d9127ep-10")]  # (2k)! / (4^k k!^2 (2k + 1)), k = 1 .. 28
CBRT_A, CBRT_B, CBRT_NEWTON = 0.75, 0.22, 6


def _horner(z, coef):
    p = np.full_like(z, coef[-1])
    for c in coef[-2::-1]:
        p = p * z + c
    return p


def sincos64(x):
    """(sin x, cos x) for 0 <= x < 2^20 (NaN elsewhere): k = floor(x * 2/pi + 0.5); r = ((x - k P1) - k P2) - k P3; Taylor
    polynomials of r by Horner in z = r * r; the quadrant k mod 4 picks and signs them"""
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        ok = (x >= 0.0) & (x < 1048576.0)
        xs = np.where(ok, x, 0.0)
        k = np.floor(xs * TWO_OVER_PI + 0.5)
        r = ((xs - k * PIO2_1) - k * PIO2_2) - k * PIO2_3
        z = r * r
        sn = r + (r * z) * _horner(z, SIN_C)
        cs = 1.0 + z * _horner(z, COS_C)
        q = k - 4.0 * np.floor(k * 0.25)
        s = np.where(q == 0.0, sn, np.where(q == 1.0, cs, np.where(q == 2.0, -sn, -cs)))
        c = np.where(q == 0.0, cs, np.where(q == 1.0, -sn, np.where(q == 2.0, -cs, sn)))
    return np.where(ok, s, np.nan), np.where(ok, c, np.nan)


def acos64(x):
    """acos on [-1, 1] (NaN outside): |x| <= 0.5: pi/2 - asin(x); else 2 asin(sqrt((1 - |x|) / 2)), reflected about pi for x < 0;
    asin(t) = t + t z P(z), z = t * t, P the Taylor series to z^28"""
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        small = ax <= 0.5
        zs = x * x
        a_small = x + (x * zs) * _horner(zs, ASIN_C)
        r_small = (PIO2_HI - a_small) + PIO2_LO
        zb = (1.0 - ax) * 0.5
        sb = np.sqrt(zb)
        a_big = sb + (sb * zb) * _horner(zb, ASIN_C)
        r_big = 2.0 * a_big
        r_big = np.where(x < 0.0, (PI_HI - r_big) + PI_LO, r_big)
    return np.where(small, r_small, r_big)


def cbrt64(x):
    """cube root of x > 0 (0, inf and NaN are returned as they are): x = m 2^e (frexp), e + 3000 = 3 q + r, a = m 2^r in [0.5, 4),
    y = 0.75 + 0.22 a, six Newton steps y = y - ((y y) y - a) / (3 (y y)), result y 2^(q - 1000)"""
    x = np.asarray(x, f64)
    with np.errstate(all="ignore"):
        ok = (x > 0.0) & (x < np.inf)
        xs = np.where(ok, x, 1.0)
        m, e = np.frexp(xs)
        e3 = e.astype(np.int64) + 3000
        q = e3 // 3
        r = e3 - 3 * q
        a = np.ldexp(m, r.astype(np.int32))
        y = CBRT_A + CBRT_B * a
        for _ in range(CBRT_NEWTON):
            y = y - ((y * y) * y - a) / (3.0 * (y * y))
        y = np.ldexp(y, (q - 1000).astype(np.int32))
    return np.where(ok, y, x)


# ---------------------------------------------------------------------------------------------------------------------
# small binary64 helpers; leading axes are batch axes
# ---------------------------------------------------------------------------------------------------------------------
def seqsum(terms, axis):
    """sum along `axis` in ascending order from 0.0"""
    terms = np.moveaxis(terms, axis, 0)
    acc = np.zeros(terms.shape[1:], terms.dtype)
    for k in range(terms.shape[0]):
        acc = acc + terms[k]
    return acc


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm3(a):
    return np.sqrt(dot3(a, a))


def matvec3(R, x):
    """(R[i][0] x0 + R[i][1] x1) + R[i][2] x2; R [..., 3, 3], x [..., 3]"""
    return (R[..., :, 0] * x[..., None, 0] + R[..., :, 1] * x[..., None, 1]) + R[..., :, 2] * x[..., None, 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def tr(A):
    return np.swapaxes(A, -1, -2).copy()


def null_space(f):
    """:370-372, S13: columns 1 and 2 of the Householder reflector H = I - beta v v^T of f (H f = alpha e0):
    alpha = -|f| for f0 >= 0, +|f| otherwise; v = (f0 - alpha, f1, f2); beta = 2 / (v . v); w = beta v;
    r_k = [k == 1] - w_k v_1, s_k = [k == 2] - w_k v_2"""
    f = np.asarray(f, f64)
    nrm = norm3(f)
    alpha = np.where(f[..., 0] >= 0.0, -nrm, nrm)
    v = f.copy()
    v[..., 0] = f[..., 0] - alpha
    with np.errstate(all="ignore"):
        beta = 2.0 / dot3(v, v)
    w = beta[..., None] * v
    r = np.array([0.0, 1.0, 0.0]) - w * v[..., 1, None]
    s = np.array([0.0, 0.0, 1.0]) - w * v[..., 2, None]
    return r, s


def null_space_svd(f):
    f = np.asarray(f, f64)
    V = np.linalg.svd(f[..., None, :])[2]  # rows of Vt
    return V[..., 1, :].copy(), V[..., 2, :].copy()


def jacobi_rounds(M, rounds, sweeps):
    """per round the angles from M at the start of the round, then the column phase of all pairs, the row phase of all, V's columns"""
    M = np.array(M, f64)
    B, n, _ = M.shape
    V = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    for _ in range(sweeps):
        for pairs in rounds:
            rot = []
            for p, q in pairs:
                apq = M[:, p, q].copy()
                c, s = T._angle(M[:, p, p].copy(), M[:, q, q].copy(), apq)
                rot.append((p, q, c, s, apq == 0.0))
            for p, q, c, s, skip in rot:
                T._rot_cols(M, p, q, c, s, skip)
            for p, q, c, s, skip in rot:
                T._rot_rows(M, p, q, c, s, skip)
            for p, q, c, s, skip in rot:
                T._rot_cols(V, p, q, c, s, skip)
    return M, V


def eig3_sorted(G, descending):
    """eigenvalues / eigenvectors (columns) of the symmetric [B, 3, 3] G from the n = 3 sequence (S12), stably sorted"""
    M, E = T.jacobi_cyclic(G, T.SWEEPS)
    lam = np.stack([M[:, i, i] for i in range(3)], 1)
    order = np.argsort(-lam if descending else lam, axis=1, kind="stable")
    lam = np.take_along_axis(lam, order, 1)
    E = np.take_along_axis(E, order[:, None, :], 2)
    return lam, E


def gram3(P):
    """P^T P, k ascending from 0.0"""
    G = np.zeros(P.shape[:-2] + (3, 3), f64)
    for k in range(3):
        G = G + P[..., k, :, None] * P[..., k, None, :]
    return G


def mul3d(A, B):
    """A B, k ascending: (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j"""
    return (A[..., :, None, 0] * B[..., None, 0, :] + A[..., :, None, 1] * B[..., None, 1, :]) + A[..., :, None, 2] * B[..., None, 2, :]


def polar3(A, exact):
    """U V^T of A's singular value decomposition, negated when its determinant is negative (:545-549, :604-608).  S13: V and the
    order from the n = 3 sequence on A^T A by descending eigenvalue; u_i = A v_i / |A v_i| for i = 0, 1; u_2 = u_0 x u_1, negated
    when it points against A v_2 (so that A = U diag(w) V^T holds with w >= 0, as with any true SVD: S12's lesson)"""
    A = np.asarray(A, f64)
    with np.errstate(all="ignore"):
        if exact:
            U, _, Vt = np.linalg.svd(A)
            R = U @ Vt
        else:
            _, E = eig3_sorted(gram3(A), True)
            v = [E[:, :, i] for i in range(3)]
            av = [matvec3(A, v[i]) for i in range(3)]
            u = [av[i] / norm3(av[i])[:, None] for i in range(2)]
            u2 = cross3(u[0], u[1])
            u.append(np.where((dot3(av[2], u2) < 0.0)[:, None], -u2, u2))
            R = (u[0][:, :, None] * v[0][:, None, :] + u[1][:, :, None] * v[1][:, None, :]) + u[2][:, :, None] * v[2][:, None, :]
        det = np.linalg.det(R) if exact else T.det3(R)
    return np.where((det < 0.0)[:, None, None], -R, R)


SKEW = np.zeros((3, 3, 3), f64)  # SKEW[k] = [e_k]x
SKEW[0, 1, 2], SKEW[0, 2, 1] = -1.0, 1.0
SKEW[1, 0, 2], SKEW[1, 2, 0] = 1.0, -1.0
SKEW[2, 0, 1], SKEW[2, 1, 0] = -1.0, 1.0


def skew(w):
    K = np.zeros(w.shape[:-1] + (3, 3), f64)
    K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
    K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
    return K


def rodrigues2rot(w, exact=False, derivatives=False):
    """:659-674 -> R [B, 3, 3]; with derivatives also D [B, 3, 3, 3], D[:, k] = dR / dw_k from the closed form
    R = I + a K + b K^2, a = sin n / n, b = (1 - cos n) / n^2:  dR/dw_k = (a' w_k / n) K + a G_k + (b' w_k / n) K^2 + b (G_k K + K G_k),
    a' = (n cos n - sin n) / n^2, b' = (n sin n - 2 (1 - cos n)) / n^3.  For n <= eps (where R = I, :669) S13 takes the limit
    dR/dw_k = G_k; the reference's generated expression divides by zero there."""
    w = np.asarray(w, f64)
    B = len(w)
    K = skew(w)
    K2 = mul3d(K, K)
    n = norm3(w)
    big = n > EPS
    I = np.broadcast_to(np.eye(3), (B, 3, 3))
    with np.errstate(all="ignore"):
        sn, cs = (np.sin(n), np.cos(n)) if exact else sincos64(n)
        a = sn / n
        nn = n * n
        b = (1.0 - cs) / nn
        R = (I + a[:, None, None] * K) + b[:, None, None] * K2
        R = np.where(big[:, None, None], R, I)
        if not derivatives:
            return R
        da = (n * cs - sn) / nn
        db = (n * sn - 2.0 * (1.0 - cs)) / (nn * n)
        D = np.zeros((B, 3, 3, 3), f64)
        for k in range(3):
            G = np.broadcast_to(SKEW[k], (B, 3, 3))
            wk = w[:, k] / n
            ca, cb = (da * wk)[:, None, None], (db * wk)[:, None, None]
            S = mul3d(G, K) + mul3d(K, G)
            Dk = ((ca * K + a[:, None, None] * G) + cb * K2) + b[:, None, None] * S
            D[:, k] = np.where(big[:, None, None], Dk, G)
    return R, D


def rot2rodrigues(R, exact=False):
    """:676-691"""
    with np.errstate(all="ignore"):
        trace = ((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - 1.0
        wn = np.arccos(trace / 2.0) if exact else acos64(trace / 2.0)
        sn = np.sin(wn) if exact else sincos64(wn)[0]
        sc = wn / (2.0 * sn)
        om = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1) * sc[:, None]
    return np.where((wn > EPS)[:, None], om, 0.0)


def residuals_and_jacs(x, X, nr, ns, exact=False):
    """:759-805 with the Jacobian by the chain rule (S13).  x [B, 6], X / nr / ns [B, n, 3] -> r [B, 2n], J [B, 2n, 6]; row 2p is
    point p's nullspace_r, row 2p + 1 its nullspace_s"""
    B, n, _ = X.shape
    R, D = rodrigues2rot(x[:, :3], exact, True)
    with np.errstate(all="ignore"):
        q = matvec3(R[:, None], X) + x[:, None, 3:]
        nq = norm3(q)
        v = q / nq[..., None]
        DX = [matvec3(D[:, None, k], X) for k in range(3)]
        r = np.zeros((B, 2 * n), f64)
        J = np.zeros((B, 2 * n, 6), f64)
        for h, nv in enumerate((nr, ns)):
            d = dot3(nv, v)
            g = (nv - d[..., None] * v) / nq[..., None]
            r[:, h::2] = d
            for k in range(3):
                J[:, h::2, k] = dot3(g, DX[k])
            J[:, h::2, 3:] = g
    return r, J


def ldlt_solve(A, b):
    """A x = b for symmetric 6 x 6 A by L D L^T with diagonal pivoting (S13): at step k the largest |diagonal| of the trailing block
    (first of equals, found with '>') is swapped to k; l_i = A_ik / d; A_ij = A_ij - l_i A_jk for k < j <= i; a zero pivot zeroes its
    column of L and its component of the solution.  Then forward, diagonal and backward substitution, j ascending."""
    A = np.array(A, f64)
    B = len(A)
    n = A.shape[1]
    ar = np.arange(B)
    perm = np.broadcast_to(np.arange(n), (B, n)).copy()
    L = np.zeros_like(A)
    d = np.zeros((B, n), f64)
    with np.errstate(all="ignore"):
        for k in range(n):
            best = np.full(B, k)
            for i in range(k + 1, n):
                better = np.abs(A[ar, i, i]) > np.abs(A[ar, best, best])
                best = np.where(better, i, best)
            rk, rb = A[ar, k, :].copy(), A[ar, best, :].copy()
            A[ar, k, :], A[ar, best, :] = rb, rk
            ck, cb = A[ar, :, k].copy(), A[ar, :, best].copy()
            A[ar, :, k], A[ar, :, best] = cb, ck
            lk, lb = L[ar, k, :].copy(), L[ar, best, :].copy()
            L[ar, k, :], L[ar, best, :] = lb, lk
            pk, pb = perm[ar, k].copy(), perm[ar, best].copy()
            perm[ar, k], perm[ar, best] = pb, pk
            dk = A[:, k, k].copy()
            d[:, k] = dk
            zero = dk == 0.0
            col = A[:, :, k].copy()
            for i in range(k + 1, n):
                li = np.where(zero, 0.0, col[:, i] / dk)
                L[:, i, k] = li
                for j in range(k + 1, i + 1):
                    val = A[:, i, j] - li * col[:, j]
                    A[:, i, j] = val
                    A[:, j, i] = val
        y = np.take_along_axis(np.asarray(b, f64), perm, 1)
        z = np.zeros((B, n), f64)
        for i in range(n):
            acc = y[:, i].copy()
            for j in range(i):
                acc = acc - L[:, i, j] * z[:, j]
            z[:, i] = acc
        wv = np.where(d == 0.0, 0.0, z / d)
        xs = np.zeros((B, n), f64)
        for i in range(n - 1, -1, -1):
            acc = wv[:, i].copy()
            for j in range(i + 1, n):
                acc = acc - L[:, j, i] * xs[:, j]
            xs[:, i] = acc
        out = np.zeros((B, n), f64)
        np.put_along_axis(out, perm, xs, 1)
    return out


def first_max_abs(a, axis=-1):
    """max |a| found with '>' from the first element (a NaN first element stays)"""
    a = np.moveaxis(np.abs(a), axis, 0)
    m = a[0].copy()
    for k in range(1, len(a)):
        m = np.where(a[k] > m, a[k], m)
    return m


def first_min_abs(a):
    a = np.moveaxis(np.abs(a), -1, 0)
    m = a[0].copy()
    for k in range(1, len(a)):
        m = np.where(a[k] < m, a[k], m)
    return m


def gauss_newton(x, X, nr, ns, exact=False):
    """mlpnp_gn (:693-757) -> x, evaluations made [B], exit kind [B]"""
    x = np.array(x, f64)
    B = len(x)
    active = np.ones(B, bool)
    evals = np.zeros(B, np.int32)
    kind = np.full(B, GN_MAXIT, np.int32)
    for _ in range(5):
        if not active.any():
            break
        r, J = residuals_and_jacs(x, X, nr, ns, exact)
        with np.errstate(all="ignore"):
            A = seqsum(J[:, :, :, None] * J[:, :, None, :], 1)
            g = seqsum(J * r[:, :, None], 1)
            if exact:
                dx = np.zeros((B, 6))
                for b in range(B):
                    try:
                        dx[b] = np.linalg.solve(A[b], g[b])
                    except np.linalg.LinAlgError:
                        dx[b] = np.nan
            else:
                dx = ldlt_solve(A, g)
            evals = evals + active
            spurious = (first_max_abs(dx) > 5.0) | (first_min_abs(dx) > 1.0)
            dl = ((((J[:, :, 0] * dx[:, None, 0] + J[:, :, 1] * dx[:, None, 1]) + J[:, :, 2] * dx[:, None, 2]) + J[:, :, 3] * dx[:, None, 3])
                  + J[:, :, 4] * dx[:, None, 4]) + J[:, :, 5] * dx[:, None, 5]
            converged = first_max_abs(dl) < 1e-5
        kind = np.where(active & spurious, GN_SPURIOUS, np.where(active & ~spurious & converged, GN_CONVERGED, kind))
        update = active & ~spurious
        x = np.where(update[:, None], x - dx, x)
        active = active & ~spurious & ~converged
    return x, evals, kind


# ---------------------------------------------------------------------------------------------------------------------
# computePose (:355-657) for B point sets of n points each
# ---------------------------------------------------------------------------------------------------------------------
def null_vector(A, n, exact, sweeps):
    if exact:
        return np.linalg.svd(T.gram64(A))[2][:, -1, :]
    M = T.gram64(A)
    M, V = jacobi_rounds(M, ROUNDS12, sweeps) if n == 12 else T.jacobi_rounds9(M, SWEEPS9)
    return T.min_column(M, V)


def planarity(X, exact):
    """:380-388 -> planar [B], eigenRot [B, 3, 3] (rows: eigenvectors by ascending eigenvalue).  S13: rank = the number of
    eigenvalues of the n = 3 sequence with |lambda| > 3 eps max |lambda|"""
    G = seqsum(X[:, :, :, None] * X[:, :, None, :], 1)
    if exact:
        lam, E = np.linalg.eigh(G)
    else:
        lam, E = eig3_sorted(G, False)
    al = np.abs(lam)
    rank = (al > RANK_TOL * al.max(1)[:, None]).sum(1)
    return rank == 2, tr(E)


def pose_general(X, nr, ns, f, exact, sweeps):
    B, n, _ = X.shape
    A = np.zeros((B, 2 * n, 12), f64)
    for h, nv in enumerate((nr, ns)):
        for i in range(3):
            for j in range(3):
                A[:, h::2, 3 * i + j] = nv[:, :, i] * X[:, :, j]
            A[:, h::2, 9 + i] = nv[:, :, i]
    res = null_vector(A, 12, exact, sweeps)
    with np.errstate(all="ignore"):
        tmp = tr(res[:, :9].reshape(B, 3, 3))  # (:596-598)
        cn = [np.sqrt((tmp[:, 0, j] * tmp[:, 0, j] + tmp[:, 1, j] * tmp[:, 1, j]) + tmp[:, 2, j] * tmp[:, 2, j]) for j in range(3)]
        prod = np.abs((cn[0] * cn[1]) * cn[2])
        scale = 1.0 / (np.cbrt(prod) if exact else cbrt64(prod))
        Rout = polar3(tmp, exact)
        tout = matvec3(Rout, scale[:, None] * res[:, 9:12])
        # the direction test (:613-634).  S13: the inverse of [Rout | +-tout] is taken as [Rout^T | -+Rout^T tout]
        Rinv = tr(Rout)
        tinv = -matvec3(Rinv, tout)
        err = []
        for t in (tinv, -tinv):
            v = matvec3(Rinv[:, None], X[:, :6]) + t[:, None, :]
            v = v / norm3(v)[..., None]
            err.append(seqsum(1.0 - dot3(v, f[:, :6]), 1))
        t0 = np.where((err[0] < err[1])[:, None], tinv, -tinv)
    return Rinv, t0


def pose_planar(X, nr, ns, f, eigenRot, exact):
    B, n, _ = X.shape
    P3 = matvec3(eigenRot[:, None], X)  # (:396-397)
    A = np.zeros((B, 2 * n, 9), f64)
    for h, nv in enumerate((nr, ns)):
        for i in range(3):
            A[:, h::2, 2 * i] = nv[:, :, i] * P3[:, :, 1]
            A[:, h::2, 2 * i + 1] = nv[:, :, i] * P3[:, :, 2]
            A[:, h::2, 6 + i] = nv[:, :, i]
    res = null_vector(A, 9, exact, None)
    with np.errstate(all="ignore"):
        c1 = np.stack([res[:, 0], res[:, 2], res[:, 4]], 1)
        c2 = np.stack([res[:, 1], res[:, 3], res[:, 5]], 1)
        tmp = np.stack([cross3(c1, c2), c1, c2], 1)  # after transposeInPlace: rows (:536-541)
        n1 = np.sqrt((tmp[:, 0, 1] * tmp[:, 0, 1] + tmp[:, 1, 1] * tmp[:, 1, 1]) + tmp[:, 2, 1] * tmp[:, 2, 1])
        n2 = np.sqrt((tmp[:, 0, 2] * tmp[:, 0, 2] + tmp[:, 1, 2] * tmp[:, 1, 2]) + tmp[:, 2, 2] * tmp[:, 2, 2])
        scale = 1.0 / np.sqrt(np.abs(n1 * n2))
        Rout1 = polar3(tmp, exact)
        Rout1 = mul3d(tr(eigenRot), Rout1)
        t = scale[:, None] * res[:, 6:9]
        Rout1 = -tr(Rout1)
        det = np.linalg.det(Rout1) if exact else T.det3(Rout1)
        Rout1[:, :, 2] = np.where((det < 0.0)[:, None], -Rout1[:, :, 2], Rout1[:, :, 2])
        R2 = Rout1.copy()
        R2[:, :, 0], R2[:, :, 1] = -Rout1[:, :, 0], -Rout1[:, :, 1]
        Ts = [(Rout1, t), (Rout1, -t), (R2, t), (R2, -t)]
        best = None
        for Rc, tc in Ts:  # (:577-590): std::min_element keeps the first minimum
            p = matvec3(Rc[:, None], X[:, :6]) + tc[:, None, :]
            p = p / norm3(p)[..., None]
            val = seqsum(1.0 - dot3(p, f[:, :6]), 1)
            if best is None:
                best, Rb, tb = val, Rc.copy(), tc.copy()
            else:
                less = val < best
                best = np.where(less, val, best)
                Rb = np.where(less[:, None, None], Rc, Rb)
                tb = np.where(less[:, None], tc, tb)
    return Rb, tb


def compute_pose(X, f, exact=False, sweeps=SWEEPS12):
    """X, f [B, n, 3] world points and bearings -> R [B, 3, 3], t [B, 3], planar [B], GN evaluations [B], GN exit [B]"""
    X, f = np.asarray(X, f64), np.asarray(f, f64)
    B = len(X)
    nr, ns = null_space_svd(f) if exact else null_space(f)
    planar, eigenRot = planarity(X, exact)
    R0 = np.zeros((B, 3, 3), f64)
    t0 = np.zeros((B, 3), f64)
    ig, ip = np.flatnonzero(~planar), np.flatnonzero(planar)
    if len(ig):
        R0[ig], t0[ig] = pose_general(X[ig], nr[ig], ns[ig], f[ig], exact, sweeps)
    if len(ip):
        R0[ip], t0[ip] = pose_planar(X[ip], nr[ip], ns[ip], f[ip], eigenRot[ip], exact)
    x0 = np.concatenate([rot2rodrigues(R0, exact), t0], 1)
    x, evals, kind = gauss_newton(x0, X, nr, ns, exact)
    return rodrigues2rot(x[:, :3], exact), x[:, 3:].copy(), planar, evals, kind


# ---------------------------------------------------------------------------------------------------------------------
# the solver
# ---------------------------------------------------------------------------------------------------------------------
def plan(N, probability=0.95, min_inliers=50, max_iterations=300, min_set=12, epsilon=0.5, n_iterations=20):
    """SetRansacParameters (:224-259) -> (mRansacMinInliers, mRansacMaxIts, passes of the first iterate(n_iterations));
    (min_inliers, 0, 0) when N < mRansacMinInliers (:106-111)"""
    eps = f32(epsilon)
    nMin = int(f32(N) * eps)
    nMin = max(nMin, min_inliers, min_set)
    if N < nMin:
        return nMin, 0, 0
    if eps < f32(nMin) / f32(N):
        eps = f32(nMin) / f32(N)
    if nMin == N:
        nIt = 1.0
    else:
        den = math.log(1.0 - math.pow(float(eps), 3.0))
        num = math.log(1.0 - probability)
        nIt = math.ceil(num / den) if den != 0.0 else math.inf
    its = max_iterations if not (nIt < max_iterations) else int(nIt)
    its = max(1, its)
    return nMin, its, max(its, n_iterations)


def draw_sets(N, iterations, min_set, rand):
    """the min-sets as :121-141 draws them (DUtils::Random::RandomInt, swap with the back)"""
    RAND_MAX = 2147483647
    sets = np.zeros((iterations, min_set), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(min_set):
            d = len(avail)
            randi = int((rand() / (RAND_MAX + 1.0)) * d)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def check_inliers(R, t, cam, model, P2D, X32, max_err):
    """:261-292 for poses [B]: -> inlier flags [B, N]"""
    B = len(R)
    N = len(X32)
    Xd = X32.astype(f64)
    with np.errstate(all="ignore"):
        pc = []
        for i in range(3):
            v = ((R[:, None, i, 0] * Xd[None, :, 0] + R[:, None, i, 1] * Xd[None, :, 1]) + R[:, None, i, 2] * Xd[None, :, 2]) + t[:, None, i]
            pc.append(v.astype(f32).reshape(-1))
        u, v = NR.project(cam, model, pc[0], pc[1], pc[2])
        dX = np.tile(P2D[:, 0], B) - u
        dY = np.tile(P2D[:, 1], B) - v
        e2 = dX * dX + dY * dY
        return (e2 < np.tile(max_err, B)).reshape(B, N)


def _ransac(exact, cam, model, precision, level_sigma2, kp_xy, kp_octave, mp_index, points, sets, probability, min_inliers,
            max_iterations, min_set, epsilon, th2, n_iterations, sweeps):
    kp_xy = np.asarray(kp_xy, f32).reshape(-1, 2)
    mp_index = np.asarray(mp_index, np.int64)
    points = np.asarray(points, f32).reshape(-1, 3)
    cam = np.asarray(cam, f32)
    n = len(kp_xy)
    idx = np.flatnonzero(mp_index >= 0)
    N = len(idx)
    nMin, maxIts, total = plan(N, probability, min_inliers, max_iterations, min_set, epsilon, n_iterations)
    out = dict(solved=False, Tcw=np.eye(4, dtype=f32), inliers=np.zeros(n, np.uint8), n_inliers=0, no_more=True, N=N,
               min_inliers=nMin, max_its=maxIts, total_iterations=total, exit_kind=EXIT_ABORT, returning_iteration=-1,
               hyp_Rt=np.zeros((total, 12), f64), hyp_inliers=np.zeros(total, np.int32), hyp_planar=np.zeros(total, np.uint8),
               hyp_gn_evals=np.zeros(total, np.int32), hyp_gn_exit=np.zeros(total, np.int32), n_candidates=0,
               candidates=np.zeros(0, np.int32), cand_Rt=np.zeros((0, 12), f64), cand_inliers=np.zeros(0, np.int32),
               cand_planar=np.zeros(0, np.uint8), cand_mask=np.zeros((0, N), np.uint8), first=idx)
    if total == 0:
        return out
    sets = np.asarray(sets, np.int64).reshape(total, min_set)
    P2D = kp_xy[idx]
    X32 = points[mp_index[idx]]
    rx, ry = NR.unproject(cam, model, f32(precision), P2D[:, 0].copy(), P2D[:, 1].copy())
    f = np.stack([np.asarray(rx, f32).astype(f64), np.asarray(ry, f32).astype(f64), np.ones(N)], 1)
    X = X32.astype(f64)
    max_err = (np.asarray(level_sigma2, f32)[np.asarray(kp_octave, np.int64)[idx]] * f32(th2)).astype(f32)

    R, t, planar, evals, kind = compute_pose(X[sets], f[sets], exact, sweeps)
    inl = check_inliers(R, t, cam, model, P2D, X32, max_err)
    cnt = inl.sum(1).astype(np.int32)
    out.update(hyp_Rt=np.concatenate([R.reshape(total, 9), t], 1), hyp_inliers=cnt, hyp_planar=planar.astype(np.uint8),
               hyp_gn_evals=evals, hyp_gn_exit=kind)
    cands, best = [], 0
    for i in range(total):
        if cnt[i] >= nMin and cnt[i] > best:
            best = int(cnt[i])
            cands.append(i)
    out.update(no_more=True, n_candidates=len(cands), candidates=np.array(cands, np.int32), cand_Rt=np.zeros((len(cands), 12), f64),
               cand_inliers=np.zeros(len(cands), np.int32), cand_planar=np.zeros(len(cands), np.uint8),
               cand_mask=np.zeros((len(cands), N), np.uint8), exit_kind=EXIT_FAILED)
    winner = -1
    # every candidate is refined (the GPU does so speculatively); the first success returns.  S13 adopts the refined pose before
    # CheckInliers; the reference never copies it into mRi / mti (:323-335) and re-scores the hypothesis: DESIGN.md S13, stated departure
    for c, i in enumerate(cands):
        sel = np.flatnonzero(inl[i])
        Rr, tr_, pl, _, _ = compute_pose(X[sel][None], f[sel][None], exact, sweeps)
        m = check_inliers(Rr, tr_, cam, model, P2D, X32, max_err)[0]
        out["cand_Rt"][c] = np.concatenate([Rr.reshape(9), tr_.reshape(3)])
        out["cand_inliers"][c] = int(m.sum())
        out["cand_planar"][c] = int(pl[0])
        out["cand_mask"][c] = m
        if winner < 0 and int(m.sum()) > nMin:
            winner = c
    if winner >= 0:
        Rt, mask, kindx, it = out["cand_Rt"][winner], out["cand_mask"][winner].astype(bool), EXIT_REFINED, cands[winner]
        out["no_more"] = False
    elif cands:
        Rt, mask, kindx, it = out["hyp_Rt"][cands[-1]], inl[cands[-1]], EXIT_BEST, cands[-1]
    else:
        return out
    Tcw = np.eye(4, dtype=f32)
    Tcw[:3, :3] = Rt[:9].reshape(3, 3).astype(f32)
    Tcw[:3, 3] = Rt[9:].astype(f32)
    inliers = np.zeros(n, np.uint8)
    inliers[idx[mask]] = 1
    out.update(solved=True, Tcw=Tcw, inliers=inliers, n_inliers=int(mask.sum()), exit_kind=kindx, returning_iteration=int(it))
    return out


def ransac(cam, model, precision, level_sigma2, kp_xy, kp_octave, mp_index, points, sets, probability=0.95, min_inliers=50,
           max_iterations=300, min_set=12, epsilon=0.5, th2=5.991, n_iterations=20, sweeps=SWEEPS12):
    """S13.  cam: fx fy cx cy k1 k2 k3 k4; kp_xy [n, 2] / kp_octave [n]: mvKeysUn; mp_index [n]: row of `points` or -1; points
    [m, 3] float world positions; sets [total_iterations, min_set] indices into the correspondence list.  Returns every field
    orbfe_mlpnp_info exposes (same names)."""
    return _ransac(False, cam, model, precision, level_sigma2, kp_xy, kp_octave, mp_index, points, sets, probability, min_inliers,
                   max_iterations, min_set, epsilon, th2, n_iterations, sweeps)


def ransac_f64(cam, model, precision, level_sigma2, kp_xy, kp_octave, mp_index, points, sets, probability=0.95, min_inliers=50,
               max_iterations=300, min_set=12, epsilon=0.5, th2=5.991, n_iterations=20):
    """the same function on numpy.linalg and numpy's sin / cos / arccos / cbrt"""
    return _ransac(True, cam, model, precision, level_sigma2, kp_xy, kp_octave, mp_index, points, sets, probability, min_inliers,
                   max_iterations, min_set, epsilon, th2, n_iterations, SWEEPS12)

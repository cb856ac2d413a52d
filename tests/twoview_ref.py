"""SPEC DECISION S12 restated for the tests: TwoViewReconstruction::Reconstruct
(src/TwoViewReconstruction.cc:40-127) for a pinhole K, written from that file.

`reconstruct` is the pinned sequence and the NORMATIVE definition: numpy binary32 where the C++ is float, ONE IEEE operation
per operator (numpy evaluates every operator on its own, so nothing is contracted; element-wise array operations round
exactly like scalars, the arrays only run all hypotheses / matches at once), the C++'s own promotions kept (1.0 / x is a
binary64 divide rounded to float, comparisons against double literals are made in binary64), sequential sums as
numpy.add.accumulate, and the four decompositions by fixed Jacobi sequences on A^T A in binary64.
`reconstruct_f64` is the same function with every step in binary64 and numpy.linalg.svd for all four decompositions: what
S12 is measured against (the reference's Eigen JacobiSVD cannot be built here).

Every match is carried through ALL steps of a gate chain (a rejected one computes garbage that is never looked at)."""
import numpy as np

f32 = np.float32
f64 = np.float64
MODEL_NONE, MODEL_H, MODEL_F = 0, 1, 2
SWEEPS = 10          # S12: fixed
SWEEPS_SYM4 = 8      # S10
COS_ONE_DEGREE = float.fromhex("0x1.ffec097f5af8ap-1")  # cos(1 deg) in binary64

# round r of the 9 x 9 sequence: the pairs {i, j}, i < j, i + j == r (mod 9), in ascending i
ROUNDS9 = [[(i, (r - i) % 9) for i in range(9) if i < (r - i) % 9] for r in range(9)]
assert all(len(r) == 4 and len({x for p in r for x in p}) == 8 for r in ROUNDS9)


# ---------------------------------------------------------------------------------------------------------------------
# Jacobi sequences (binary64).  M: [B, n, n] symmetric, returns (diagonalised M, V)
# ---------------------------------------------------------------------------------------------------------------------
def _angle(app, aqq, apq):
    """c, s of one rotation (kernels: jacobi_angle); entries with apq == 0 are skipped by the caller"""
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
    return c, s


def _rot_cols(X, p, q, c, s, skip):
    a = X[:, :, p].copy()
    b = X[:, :, q].copy()
    with np.errstate(all="ignore"):
        X[:, :, p] = np.where(skip[:, None], a, c[:, None] * a - s[:, None] * b)
        X[:, :, q] = np.where(skip[:, None], b, s[:, None] * a + c[:, None] * b)


def _rot_rows(X, p, q, c, s, skip):
    a = X[:, p, :].copy()
    b = X[:, q, :].copy()
    with np.errstate(all="ignore"):
        X[:, p, :] = np.where(skip[:, None], a, c[:, None] * a - s[:, None] * b)
        X[:, q, :] = np.where(skip[:, None], b, s[:, None] * a + c[:, None] * b)


def jacobi_cyclic(M, sweeps):
    """the S10 sequence for any n: pairs (p, q), p < q, in lexicographic order, each angle from M as it stands"""
    M = np.array(M, f64)
    B, n, _ = M.shape
    V = np.broadcast_to(np.eye(n), (B, n, n)).copy()
    for _ in range(sweeps):
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = M[:, p, q].copy()
                skip = apq == 0.0
                c, s = _angle(M[:, p, p].copy(), M[:, q, q].copy(), apq)
                _rot_cols(M, p, q, c, s, skip)
                _rot_rows(M, p, q, c, s, skip)
                _rot_cols(V, p, q, c, s, skip)
    return M, V


def jacobi_rounds9(M, sweeps=SWEEPS):
    """the S12 sequence at n = 9: per round the four angles from M at the start of the round, then the column phase of all
    four pairs, then the row phase of all four, then V's column phase"""
    M = np.array(M, f64)
    B = M.shape[0]
    V = np.broadcast_to(np.eye(9), (B, 9, 9)).copy()
    for _ in range(sweeps):
        for pairs in ROUNDS9:
            rot = []
            for p, q in pairs:
                apq = M[:, p, q].copy()
                c, s = _angle(M[:, p, p].copy(), M[:, q, q].copy(), apq)
                rot.append((p, q, c, s, apq == 0.0))
            for p, q, c, s, skip in rot:
                _rot_cols(M, p, q, c, s, skip)
            for p, q, c, s, skip in rot:
                _rot_rows(M, p, q, c, s, skip)
            for p, q, c, s, skip in rot:
                _rot_cols(V, p, q, c, s, skip)
    return M, V


def min_column(M, V):
    """column of V at the smallest diagonal entry, lowest index on ties"""
    B, n, _ = M.shape
    best = M[:, 0, 0].copy()
    out = V[:, :, 0].copy()
    for i in range(1, n):
        less = M[:, i, i] < best
        best = np.where(less, M[:, i, i], best)
        out = np.where(less[:, None], V[:, :, i], out)
    return out


def gram64(A):
    """A^T A in binary64: each entry a sum over the rows in ascending row order, from 0.0"""
    A = np.asarray(A).astype(f64)
    B, rows, n = A.shape
    M = np.zeros((B, n, n), f64)
    for k in range(rows):
        M = M + A[:, k, :, None] * A[:, k, None, :]
    return M


# ---------------------------------------------------------------------------------------------------------------------
# 3 x 3 helpers in the working type F (binary32 in the spec), batch-free
# ---------------------------------------------------------------------------------------------------------------------
def mul3(A, B):
    """k ascending: (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j"""
    C = np.zeros(A.shape[:-2] + (3, 3), A.dtype)
    for i in range(3):
        for j in range(3):
            C[..., i, j] = (A[..., i, 0] * B[..., 0, j] + A[..., i, 1] * B[..., 1, j]) + A[..., i, 2] * B[..., 2, j]
    return C


def cof3(a):
    c = np.zeros_like(a)
    c[..., 0, 0] = a[..., 1, 1] * a[..., 2, 2] - a[..., 1, 2] * a[..., 2, 1]
    c[..., 0, 1] = a[..., 0, 2] * a[..., 2, 1] - a[..., 0, 1] * a[..., 2, 2]
    c[..., 0, 2] = a[..., 0, 1] * a[..., 1, 2] - a[..., 0, 2] * a[..., 1, 1]
    c[..., 1, 0] = a[..., 1, 2] * a[..., 2, 0] - a[..., 1, 0] * a[..., 2, 2]
    c[..., 1, 1] = a[..., 0, 0] * a[..., 2, 2] - a[..., 0, 2] * a[..., 2, 0]
    c[..., 1, 2] = a[..., 0, 2] * a[..., 1, 0] - a[..., 0, 0] * a[..., 1, 2]
    c[..., 2, 0] = a[..., 1, 0] * a[..., 2, 1] - a[..., 1, 1] * a[..., 2, 0]
    c[..., 2, 1] = a[..., 0, 1] * a[..., 2, 0] - a[..., 0, 0] * a[..., 2, 1]
    c[..., 2, 2] = a[..., 0, 0] * a[..., 1, 1] - a[..., 0, 1] * a[..., 1, 0]
    return c


def det3(a):
    c = cof3(a)
    return (a[..., 0, 0] * c[..., 0, 0] + a[..., 0, 1] * c[..., 1, 0]) + a[..., 0, 2] * c[..., 2, 0]


def inv3(a):
    """adjugate / determinant"""
    F = a.dtype.type
    c = cof3(a)
    det = (a[..., 0, 0] * c[..., 0, 0] + a[..., 0, 1] * c[..., 1, 0]) + a[..., 0, 2] * c[..., 2, 0]
    with np.errstate(all="ignore"):
        inv = F(1.0) / det
        return c * inv[..., None, None]


def inv_via64(x, F):
    """`1.0 / x` of the C++ with float x: a binary64 divide rounded to float"""
    with np.errstate(all="ignore"):
        return (f64(1.0) / np.asarray(x).astype(f64)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# Normalize (:750-797)
# ---------------------------------------------------------------------------------------------------------------------
def normalize(xy, F):
    xy = np.asarray(xy, F)
    n = len(xy)
    meanX = np.add.accumulate(xy[:, 0], dtype=F)[-1]
    meanY = np.add.accumulate(xy[:, 1], dtype=F)[-1]
    meanX = meanX / F(n)
    meanY = meanY / F(n)
    px = xy[:, 0] - meanX
    py = xy[:, 1] - meanY
    meanDevX = np.add.accumulate(np.abs(px), dtype=F)[-1]
    meanDevY = np.add.accumulate(np.abs(py), dtype=F)[-1]
    meanDevX = meanDevX / F(n)
    meanDevY = meanDevY / F(n)
    sX = inv_via64(meanDevX, F)
    sY = inv_via64(meanDevY, F)
    px = px * sX
    py = py * sY
    T = np.zeros((3, 3), F)
    T[0, 0] = sX
    T[1, 1] = sY
    T[0, 2] = -meanX * sX
    T[1, 2] = -meanY * sY
    T[2, 2] = F(1.0)
    return np.stack([px, py], 1), T


# ---------------------------------------------------------------------------------------------------------------------
# ComputeH21 / ComputeF21 (:230-306) for all iterations at once
# ---------------------------------------------------------------------------------------------------------------------
def null_vector(A, F, exact, sweeps):
    if exact:
        return np.linalg.svd(A.astype(f64))[2][:, -1, :]
    M, V = jacobi_rounds9(gram64(A), sweeps)
    return min_column(M, V).astype(F)


def compute_h21(p1, p2, F, exact, sweeps):
    """p1, p2: [B, 8, 2] normalised points -> Hn [B, 3, 3]"""
    B = len(p1)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A = np.zeros((B, 16, 9), F)
    A[:, 0::2, 3] = -u1
    A[:, 0::2, 4] = -v1
    A[:, 0::2, 5] = F(-1.0)
    A[:, 0::2, 6] = v2 * u1
    A[:, 0::2, 7] = v2 * v1
    A[:, 0::2, 8] = v2
    A[:, 1::2, 0] = u1
    A[:, 1::2, 1] = v1
    A[:, 1::2, 2] = F(1.0)
    A[:, 1::2, 6] = -u2 * u1
    A[:, 1::2, 7] = -u2 * v1
    A[:, 1::2, 8] = -u2
    return null_vector(A, F, exact, sweeps).reshape(B, 3, 3)


def rank2(Fpre, F, exact):
    """:300-305.  S12: Fpre - (Fpre v) v^T, v = eigenvector of the smallest eigenvalue of Fpre^T Fpre (n = 3 sequence)"""
    if exact:
        U, w, Vt = np.linalg.svd(Fpre.astype(f64))
        w[:, 2] = 0.0
        return (U * w[:, None, :]) @ Vt
    P = Fpre.astype(f64)
    G = np.zeros_like(P)
    for k in range(3):
        G = G + P[:, k, :, None] * P[:, k, None, :]
    M, V = jacobi_cyclic(G, SWEEPS)
    v = min_column(M, V)
    w = (P[:, :, 0] * v[:, None, 0] + P[:, :, 1] * v[:, None, 1]) + P[:, :, 2] * v[:, None, 2]
    return (P - w[:, :, None] * v[:, None, :]).astype(F)


def compute_f21(p1, p2, F, exact, sweeps):
    B = len(p1)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A = np.zeros((B, 8, 9), F)
    A[:, :, 0] = u2 * u1
    A[:, :, 1] = u2 * v1
    A[:, :, 2] = u2
    A[:, :, 3] = v2 * u1
    A[:, :, 4] = v2 * v1
    A[:, :, 5] = v2
    A[:, :, 6] = u1
    A[:, :, 7] = v1
    A[:, :, 8] = F(1.0)
    Fpre = null_vector(A, F, exact, sweeps).reshape(B, 3, 3)
    return rank2(Fpre, F, exact)


# ---------------------------------------------------------------------------------------------------------------------
# CheckHomography / CheckFundamental (:308-471) for all iterations x all matches
# ---------------------------------------------------------------------------------------------------------------------
def _score(term1, term2, F):
    """sequential sum in match order, first-image term first; a rejected term (already 0) adds nothing"""
    B, N = term1.shape
    terms = np.empty((B, 2 * N), F)
    terms[:, 0::2] = term1
    terms[:, 1::2] = term2
    return np.add.accumulate(terms, axis=1, dtype=F)[:, -1]


def check_homography(H21, H12, pts, sigma, F):
    th = F(5.991)
    invSigmaSquare = inv_via64(sigma * sigma, F)
    u1, v1, u2, v2 = (pts[None, :, k] for k in range(4))
    h = lambda M, i, j: M[:, i, j][:, None]
    with np.errstate(all="ignore"):
        w2in1inv = inv_via64((h(H12, 2, 0) * u2 + h(H12, 2, 1) * v2) + h(H12, 2, 2), F)
        u2in1 = ((h(H12, 0, 0) * u2 + h(H12, 0, 1) * v2) + h(H12, 0, 2)) * w2in1inv
        v2in1 = ((h(H12, 1, 0) * u2 + h(H12, 1, 1) * v2) + h(H12, 1, 2)) * w2in1inv
        du, dv = u1 - u2in1, v1 - v2in1
        chi1 = (du * du + dv * dv) * invSigmaSquare
        w1in2inv = inv_via64((h(H21, 2, 0) * u1 + h(H21, 2, 1) * v1) + h(H21, 2, 2), F)
        u1in2 = ((h(H21, 0, 0) * u1 + h(H21, 0, 1) * v1) + h(H21, 0, 2)) * w1in2inv
        v1in2 = ((h(H21, 1, 0) * u1 + h(H21, 1, 1) * v1) + h(H21, 1, 2)) * w1in2inv
        du, dv = u2 - u1in2, v2 - v1in2
        chi2 = (du * du + dv * dv) * invSigmaSquare
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, F(0.0), th - chi1)
        t2 = np.where(out2, F(0.0), th - chi2)
    return _score(t1, t2, F), ~(out1 | out2), (chi1, chi2)


def check_fundamental(F21, pts, sigma, F):
    th, thScore = F(3.841), F(5.991)
    invSigmaSquare = inv_via64(sigma * sigma, F)
    u1, v1, u2, v2 = (pts[None, :, k] for k in range(4))
    f = lambda i, j: F21[:, i, j][:, None]
    with np.errstate(all="ignore"):
        a2 = (f(0, 0) * u1 + f(0, 1) * v1) + f(0, 2)
        b2 = (f(1, 0) * u1 + f(1, 1) * v1) + f(1, 2)
        c2 = (f(2, 0) * u1 + f(2, 1) * v1) + f(2, 2)
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invSigmaSquare
        a1 = (f(0, 0) * u2 + f(1, 0) * v2) + f(2, 0)
        b1 = (f(0, 1) * u2 + f(1, 1) * v2) + f(2, 1)
        c1 = (f(0, 2) * u2 + f(1, 2) * v2) + f(2, 2)
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invSigmaSquare
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, F(0.0), thScore - chi1)
        t2 = np.where(out2, F(0.0), thScore - chi2)
    return _score(t1, t2, F), ~(out1 | out2), (chi1, chi2)


def first_max(scores):
    """`if(currentScore>score)` from score = 0 over the iterations in order -> (index or -1, score)"""
    best, idx = scores.dtype.type(0.0), -1
    for i, s in enumerate(scores):
        if s > best:
            best, idx = s, i
    return idx, best


# ---------------------------------------------------------------------------------------------------------------------
# the 3 x 3 SVDs (:597, :919) and the motion hypotheses
# ---------------------------------------------------------------------------------------------------------------------
def svd3(A, F, exact, full_rank=False):
    """-> U, w, V in F.  S12: V and w^2 from the n = 3 sequence on A^T A (binary64) by descending eigenvalue (lower index first
    among equals); u_i = A v_i / |A v_i| for i = 0, 1 and u_2 = u_0 x u_1; w_i = sqrt(max(eigenvalue_i, 0)); rounded per entry.
    full_rank (:597): u_2 is negated when it points against A v_2 (binary64 dot product), so that A = U diag(w) V^T holds with
    w >= 0 and s = det(U) det(V^T) of :603 carries the sign of det(A), as it does with any true SVD."""
    if exact:
        U, w, Vt = np.linalg.svd(A.astype(f64))
        return U, w, Vt.T.copy()
    P = A.astype(f64)
    G = np.zeros((3, 3), f64)
    for k in range(3):
        G = G + P[k, :, None] * P[k, None, :]
    M, E = jacobi_cyclic(G[None], SWEEPS)
    lam = np.array([M[0, i, i] for i in range(3)])
    order = sorted(range(3), key=lambda i: (-lam[i], i))
    v = [E[0, :, c].copy() for c in order]
    w = np.array([np.sqrt(lam[c] if lam[c] > 0.0 else f64(0.0)) for c in order], f64)
    u = []
    with np.errstate(all="ignore"):
        for i in range(2):
            av = (P[:, 0] * v[i][0] + P[:, 1] * v[i][1]) + P[:, 2] * v[i][2]
            nrm = np.sqrt((av[0] * av[0] + av[1] * av[1]) + av[2] * av[2])
            u.append(av / nrm)
    u.append(np.array([u[0][1] * u[1][2] - u[0][2] * u[1][1], u[0][2] * u[1][0] - u[0][0] * u[1][2],
                       u[0][0] * u[1][1] - u[0][1] * u[1][0]], f64))
    if full_rank:
        av = (P[:, 0] * v[2][0] + P[:, 1] * v[2][1]) + P[:, 2] * v[2][2]
        if (av[0] * u[2][0] + av[1] * u[2][1]) + av[2] * u[2][2] < 0.0:
            u[2] = -u[2]
    return np.stack(u, 1).astype(F), w.astype(F), np.stack(v, 1).astype(F)


def _unit(t):
    with np.errstate(all="ignore"):
        nrm = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
        return t / nrm


def hypotheses_f(F21, K, F, exact):
    """DecomposeE (:916-940) in the order of :498-501: (R1, t) (R2, t) (R1, -t) (R2, -t)"""
    E = mul3(mul3(K.T.copy(), F21), K)
    U, w, V = svd3(E, F, exact)
    Vt = V.T.copy()
    t = _unit(U[:, 2].copy())
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
    R1 = mul3(mul3(U, W), Vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = mul3(mul3(U, W.T.copy()), Vt)
    if det3(R2) < 0:
        R2 = -R2
    return [R1, R2, R1, R2], [t, t, -t, -t]


def hypotheses_h(H21, K, F, exact):
    """:594-702 -> (Rs, ts) or None when the singular values are too close (:609)"""
    A = mul3(mul3(inv3(K), H21), K)
    U, w, V = svd3(A, F, exact, full_rank=True)
    Vt = V.T.copy()
    s = det3(U) * det3(Vt)
    d1, d2, d3 = w[0], w[1], w[2]
    with np.errstate(all="ignore"):
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
        aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
        sU = s * U
        Rs, ts = [], []
        z, one = F(0.0), F(1.0)
        for i in range(4):
            Rp = np.array([[ctheta, z, -stheta[i]], [z, one, z], [stheta[i], z, ctheta]], F)
            Rs.append(mul3(mul3(sU, Rp), Vt))
            k = d1 - d3
            tp = np.array([x1[i] * k, z * k, -x3[i] * k], F)
            ts.append(_unit((U[:, 0] * tp[0] + U[:, 1] * tp[1]) + U[:, 2] * tp[2]))
        for i in range(4):
            Rp = np.array([[cphi, z, sphi[i]], [z, -one, z], [sphi[i], z, -cphi]], F)
            Rs.append(mul3(mul3(sU, Rp), Vt))
            k = d1 + d3
            tp = np.array([x1[i] * k, z * k, x3[i] * k], F)
            ts.append(_unit((U[:, 0] * tp[0] + U[:, 1] * tp[1]) + U[:, 2] * tp[2]))
    return Rs, ts


# ---------------------------------------------------------------------------------------------------------------------
# CheckRT (:799-914) for one motion hypothesis over all matches
# ---------------------------------------------------------------------------------------------------------------------
def ordered_key(c):
    u = np.asarray(c, f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def check_rt(R, t, K, pts, inlier, th2, F, exact):
    """-> flags [N] (bit 0 counted in nGood, bit 1 vbGood), x3d [N, 3], cos [N], nGood, cosine at rank min(50, nGood - 1)"""
    N = len(pts)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    u1, v1, u2, v2 = (pts[:, k] for k in range(4))
    z = F(0.0)
    P1 = np.array([[fx, z, cx, z], [z, fy, cy, z], [z, z, F(1.0), z]], F)
    Rt = np.concatenate([R, t[:, None]], 1)
    P2 = np.zeros((3, 4), F)
    for i in range(3):
        for j in range(4):
            P2[i, j] = (K[i, 0] * Rt[0, j] + K[i, 1] * Rt[1, j]) + K[i, 2] * Rt[2, j]
    O2 = np.array([((-R[0, i]) * t[0] + (-R[1, i]) * t[1]) + (-R[2, i]) * t[2] for i in range(3)], F)
    with np.errstate(all="ignore"):
        A = np.zeros((N, 4, 4), F)
        for j in range(4):  # GeometricTools::Triangulate rows (S11)
            A[:, 0, j] = u1 * P1[2, j] - P1[0, j]
            A[:, 1, j] = v1 * P1[2, j] - P1[1, j]
            A[:, 2, j] = u2 * P2[2, j] - P2[0, j]
            A[:, 3, j] = v2 * P2[2, j] - P2[1, j]
        if exact:
            vv = np.linalg.svd(A.astype(f64))[2][:, -1, :]
        else:
            M, V = jacobi_cyclic(gram64(A), SWEEPS_SYM4)
            vv = min_column(M, V)
        X = (vv[:, 0] / vv[:, 3]).astype(F)
        Y = (vv[:, 1] / vv[:, 3]).astype(F)
        Z = (vv[:, 2] / vv[:, 3]).astype(F)
        finite = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
        dist1 = np.sqrt((X * X + Y * Y) + Z * Z)
        n2x, n2y, n2z = X - O2[0], Y - O2[1], Z - O2[2]
        dist2 = np.sqrt((n2x * n2x + n2y * n2y) + n2z * n2z)
        cosP = ((X * n2x + Y * n2y) + Z * n2z) / (dist1 * dist2)
        low = ~(cosP.astype(f64) < 0.99998)
        X2 = ((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]
        Y2 = ((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]
        Z2 = ((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2]
        invZ1 = inv_via64(Z, F)
        e1x = ((fx * X) * invZ1 + cx) - u1
        e1y = ((fy * Y) * invZ1 + cy) - v1
        err1 = e1x * e1x + e1y * e1y
        invZ2 = inv_via64(Z2, F)
        e2x = ((fx * X2) * invZ2 + cx) - u2
        e2y = ((fy * Y2) * invZ2 + cy) - v2
        err2 = e2x * e2x + e2y * e2y
        good = inlier.astype(bool) & finite & ~((Z <= 0) & ~low) & ~((Z2 <= 0) & ~low) & ~(err1 > th2) & ~(err2 > th2)
    flags = (good.astype(np.uint8) | ((good & ~low).astype(np.uint8) << 1)).astype(np.uint8)
    x3d = np.where(good[:, None], np.stack([X, Y, Z], 1), F(0.0)).astype(F)
    cosv = np.where(good, cosP, F(0.0)).astype(F)
    nGood = int(good.sum())
    if nGood == 0:
        cosSel = F(1.0)
    else:
        c = cosP[good]
        rank = min(50, nGood - 1)
        cosSel = c[np.argsort(ordered_key(c), kind="stable")][rank] if F is f32 else np.sort(c)[rank]
    detail = dict(Z=Z, Z2=Z2, err1=err1, err2=err2, cos=cosP, finite=finite)
    return flags, x3d, cosv, nGood, cosSel, detail


# ---------------------------------------------------------------------------------------------------------------------
# Reconstruct (:40-127)
# ---------------------------------------------------------------------------------------------------------------------
def _reconstruct(F, exact, fx, fy, cx, cy, sigma, iterations, kp1_xy, kp2_xy, matches12, sets, min_triangulated, sweeps):
    kp1_xy, kp2_xy = np.asarray(kp1_xy, F).reshape(-1, 2), np.asarray(kp2_xy, F).reshape(-1, 2)
    matches12 = np.asarray(matches12, np.int64)
    n1 = len(kp1_xy)
    first = np.nonzero(matches12 >= 0)[0]
    second = matches12[first]
    N = len(first)
    out = dict(reconstructed=False, R21=np.zeros((3, 3), F), t21=np.zeros(3, F), p3d=np.zeros((n1, 3), F),
               triangulated=np.zeros(n1, np.uint8), n_matches=N, SH=F(0), SF=F(0), RH=F(0), model=MODEL_NONE, exit_line=62,
               H21=np.zeros((3, 3), F), F21=np.zeros((3, 3), F), best_it_H=-1, best_it_F=-1, n_hypotheses=0, best_hypothesis=-1,
               n_good=np.zeros(8, np.int32), cos_parallax=np.ones(8, F), hyp_R=np.zeros((8, 3, 3), F), hyp_t=np.zeros((8, 3), F),
               scores=np.zeros(2 * iterations, F), inliers_H=np.zeros(N, np.uint8), inliers_F=np.zeros(N, np.uint8),
               rt_flags=np.zeros((8, N), np.uint8), rt_x3d=np.zeros((8, N, 3), F), rt_cos=np.zeros((8, N), F), first=first,
               details=[])
    if N < 8:
        return out
    sets = np.asarray(sets, np.int64).reshape(iterations, 8)
    sigma = F(sigma)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
    pn1, T1 = normalize(kp1_xy, F)
    pn2, T2 = normalize(kp2_xy, F)
    T2inv = inv3(T2)
    T2t = T2.T.copy()
    pts = np.concatenate([kp1_xy[first], kp2_xy[second]], 1)      # [N, 4] u1 v1 u2 v2
    p1 = pn1[first][sets]                                         # [B, 8, 2]
    p2 = pn2[second][sets]

    Hn = compute_h21(p1, p2, F, exact, sweeps)
    H21 = mul3(mul3(np.broadcast_to(T2inv, Hn.shape), Hn), np.broadcast_to(T1, Hn.shape))
    H12 = inv3(H21)
    scH, inH, chiH = check_homography(H21, H12, pts, sigma, F)
    Fn = compute_f21(p1, p2, F, exact, sweeps)
    F21 = mul3(mul3(np.broadcast_to(T2t, Fn.shape), Fn), np.broadcast_to(T1, Fn.shape))
    scF, inF, chiF = check_fundamental(F21, pts, sigma, F)
    out["scores"] = np.concatenate([scH, scF])
    iH, SH = first_max(scH)
    iF, SF = first_max(scF)
    out.update(SH=SH, SF=SF, best_it_H=iH, best_it_F=iF)
    if iH >= 0:
        out.update(H21=H21[iH], inliers_H=inH[iH].astype(np.uint8), chi_H=(chiH[0][iH], chiH[1][iH]))
    if iF >= 0:
        out.update(F21=F21[iF], inliers_F=inF[iF].astype(np.uint8), chi_F=(chiF[0][iF], chiF[1][iF]))

    if SH + SF == 0:
        out["exit_line"] = 110
        return out
    RH = SH / (SH + SF)
    useH = f64(RH) > 0.40
    out.update(RH=RH, model=MODEL_H if useH else MODEL_F)
    inl = out["inliers_H"] if useH else out["inliers_F"]
    nInliers = int(inl.sum())
    hyp = hypotheses_h(out["H21"], K, F, exact) if useH else hypotheses_f(out["F21"], K, F, exact)
    if hyp is None:
        out["exit_line"] = 609
        return out
    Rs, ts = hyp
    nh = len(Rs)
    out["n_hypotheses"] = nh
    sigma2 = sigma * sigma
    th2 = (f64(4.0) * f64(sigma2)).astype(F)
    for h in range(nh):
        out["hyp_R"][h], out["hyp_t"][h] = Rs[h], ts[h]
        fl, x3, cs, ng, csel, det = check_rt(Rs[h], ts[h], K, pts, inl, th2, F, exact)
        out["rt_flags"][h], out["rt_x3d"][h], out["rt_cos"][h], out["n_good"][h], out["cos_parallax"][h] = fl, x3, cs, ng, csel
        out["details"].append(det)
    nGood, cosSel = out["n_good"], out["cos_parallax"]
    best = -1
    if not useH:  # :503-580
        maxGood = int(max(nGood[:4]))
        nMinGood = max(int(0.9 * nInliers), min_triangulated)
        nsimilar = sum(1 for h in range(4) if nGood[h] > 0.7 * maxGood)
        if maxGood < nMinGood or nsimilar > 1:
            out["exit_line"] = 528
            return out
        pick = [h for h in range(4) if nGood[h] == maxGood][0]
        if nGood[pick] > 0 and f64(cosSel[pick]) < COS_ONE_DEGREE:
            best = pick
        if best < 0:
            out["exit_line"] = 580
            return out
    else:  # :705-746
        bestGood, secondBestGood, bestIdx = 0, 0, -1
        for h in range(8):
            if nGood[h] > bestGood:
                secondBestGood, bestGood, bestIdx = bestGood, int(nGood[h]), h
            elif nGood[h] > secondBestGood:
                secondBestGood = int(nGood[h])
        ok = bestIdx >= 0 and f64(cosSel[bestIdx]) <= COS_ONE_DEGREE
        if secondBestGood < 0.75 * bestGood and ok and bestGood > min_triangulated and bestGood > 0.9 * nInliers:
            best = bestIdx
        if best < 0:
            out["exit_line"] = 746
            return out
    out.update(reconstructed=True, exit_line=0, best_hypothesis=best, R21=Rs[best].copy(), t21=ts[best].copy())
    fl = out["rt_flags"][best]
    out["p3d"][first] = out["rt_x3d"][best]
    out["triangulated"][first] = (fl >> 1) & 1
    return out


def reconstruct(fx, fy, cx, cy, sigma, iterations, kp1_xy, kp2_xy, matches12, sets, min_triangulated=50, sweeps=SWEEPS):
    """S12.  kp*_xy: [n, 2] mvKeysUn[i].pt; matches12: [n1] index in frame 2 or -1; sets: [iterations, 8] indices into the match
    list.  Returns every intermediate orbfe_two_view_info exposes (same names)."""
    return _reconstruct(f32, False, f32(fx), f32(fy), f32(cx), f32(cy), sigma, iterations, kp1_xy, kp2_xy, matches12, sets,
                        min_triangulated, sweeps)


def reconstruct_f64(fx, fy, cx, cy, sigma, iterations, kp1_xy, kp2_xy, matches12, sets, min_triangulated=50):
    """the same function, every step in binary64, numpy.linalg.svd for all four decompositions"""
    return _reconstruct(f64, True, f64(f32(fx)), f64(f32(fy)), f64(f32(cx)), f64(f32(cy)), sigma, iterations, kp1_xy, kp2_xy,
                        matches12, sets, min_triangulated, SWEEPS)


def draw_sets(N, iterations, rand):
    """mvSets as :75-94 draws them; rand() -> the next value of the process's rand() stream in [0, RAND_MAX];
    DUtils::Random::RandomInt (Thirdparty/DBoW2/src/DUtils/Random.cpp:47-50): d = max - min + 1; int(rand() / (RAND_MAX + 1.0) * d) + min"""
    RAND_MAX = 2147483647
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(8):
            d = len(avail)
            randi = int((rand() / (RAND_MAX + 1.0)) * d)
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets

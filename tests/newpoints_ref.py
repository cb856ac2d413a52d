"""SPEC DECISION S11 restated for the tests: "triangulate each match" of
LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:571-705) with GeometricTools::Triangulate
(src/GeometricTools.cc:47-66) for monocular key frames, written from those two files.

`triangulate` is the pinned sequence: numpy binary32, ONE IEEE operation per line, left to right (numpy evaluates every
operator on its own, so nothing is contracted; element-wise array operations round exactly like scalars, the arrays only
run all pairs at once), binary64 for the comparisons against the reference's double literals and for the null vector
(A^T A, eight cyclic Jacobi sweeps, the S10 sequence).  The S5 pieces (KannalaBrandt8 unproject, atan2, cos / sin) are the
oracle's exported functions.  `triangulate_f64` is the same function with every step in binary64 and numpy.linalg.svd for
the null vector: what S11 is measured against (the reference's Eigen JacobiSVD cannot be built here).

Every pair is carried through ALL steps (a pair rejected early computes garbage that is never looked at) and the verdict is
the FIRST gate that fails, in the reference's order -- the same result as the reference's chain of `continue`s."""
import numpy as np

import oracle_py as O

f32 = np.float32
f64 = np.float64
ACCEPTED, LOW_PARALLAX, AT_INFINITY, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, FAR, SCALE, NO_PARTNER = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 255
RAD2DEG = f32(float.fromhex("0x1.ca5dc2p+5"))


def params(Tcw1, Tcw2, twc1, twc2, sigma2_1, sigma2_2, ratioFactor, model1=0, model2=0, cam1=None, cam2=None, precision=1e-6,
           inertial=False, farPoints=False, thFarPoints=0.0):
    """the per-pair-of-key-frames inputs (the fields of orbfe_newpoint_params), rounded to binary32 once"""
    return dict(Tcw1=np.asarray(Tcw1, f32).reshape(3, 4), Tcw2=np.asarray(Tcw2, f32).reshape(3, 4), twc1=np.asarray(twc1, f32),
                twc2=np.asarray(twc2, f32), sigma2_1=np.asarray(sigma2_1, f32), sigma2_2=np.asarray(sigma2_2, f32),
                ratioFactor=f32(ratioFactor), model1=int(model1), model2=int(model2), cam1=np.asarray(cam1, f32),
                cam2=np.asarray(cam2, f32), precision=f32(precision), inertial=bool(inertial), farPoints=bool(farPoints),
                thFarPoints=f32(thFarPoints))


# ---------------------------------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------------------------------
def unproject(cam, model, precision, u, v):
    """GeometricCamera::unprojectEig -> (x, y) of the ray (x, y, 1): Pinhole.cpp:57-60 / KannalaBrandt8.cpp:115-142 (S10)"""
    if model == 0:
        x = (u - cam[2]) / cam[0]
        y = (v - cam[3]) / cam[1]
        return x, y
    x = np.zeros(len(u), f32)
    y = np.zeros(len(u), f32)
    for i in range(len(u)):
        x[i], y[i] = O.kb8_unproject(cam, 1, precision, u[i], v[i])
    return x, y


def project(cam, model, x, y, z, live=None):
    """GeometricCamera::project (S8): Pinhole.cpp:41-47 / KannalaBrandt8.cpp:66-83 on the oracle's S5 atan2 and cos / sin.
    `live`: the pairs whose result is looked at (the others get NaN; spares the per-pair oracle calls)"""
    fx, fy, cx, cy = cam[0], cam[1], cam[2], cam[3]
    if model == 0:
        a = fx * x
        a = a / z
        u = a + cx
        b = fy * y
        b = b / z
        v = b + cy
        return u, v
    u = np.full(len(x), np.nan, f32)
    v = np.full(len(x), np.nan, f32)
    for i in (range(len(x)) if live is None else np.flatnonzero(live)):
        u[i], v[i] = kb8_project_one(cam, x[i], y[i], z[i])
    return u, v


def kb8_project_one(cam, x, y, z):
    fx, fy, cx, cy, k1, k2, k3, k4 = (f32(c) for c in cam)
    x, y, z = f32(x), f32(y), f32(z)
    xx = x * x
    yy = y * y
    x2_plus_y2 = xx + yy
    theta = f32(O.spec_atan2f(np.sqrt(x2_plus_y2), z))
    psi = f32(O.spec_atan2f(y, x))
    theta2 = theta * theta
    theta3 = theta * theta2
    theta5 = theta3 * theta2
    theta7 = theta5 * theta2
    theta9 = theta7 * theta2
    r = k1 * theta3
    r = theta + r
    t = k2 * theta5
    r = r + t
    t = k3 * theta7
    r = r + t
    t = k4 * theta9
    r = r + t
    deg = psi * RAD2DEG
    if deg < 0:
        deg = deg + f32(360.0)
    c, s = O.cos_sin_deg(deg)
    c, s = f32(c), f32(s)
    u = fx * r
    u = u * c
    u = u + cx
    v = fy * r
    v = v * s
    v = v + cy
    return u, v


# ---------------------------------------------------------------------------------------------------------------------
# the null vector of A (S10 sequence): A^T A in binary64, eight cyclic Jacobi sweeps, pair order (0,1) ... (2,3)
# ---------------------------------------------------------------------------------------------------------------------
def min_eigenvector(A):
    """A: 4 x 4 lists of binary32 arrays -> the four components (binary64 arrays) of the eigenvector of A^T A's smallest
    eigenvalue, lowest index on ties"""
    n = len(A[0][0])
    A64 = [[A[i][j].astype(f64) for j in range(4)] for i in range(4)]
    M = [[None] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            acc = np.zeros(n, f64)
            for k in range(4):
                prod = A64[k][i] * A64[k][j]
                acc = acc + prod
            M[i][j] = acc
    V = [[np.full(n, 1.0 if i == j else 0.0, f64) for j in range(4)] for i in range(4)]
    for _ in range(8):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = M[p][q]
                on = apq != 0.0                       # "if (apq == 0.0) continue"
                den = np.where(on, 2.0 * apq, 1.0)
                theta = M[q][q] - M[p][p]
                theta = theta / den
                sq = theta * theta
                sq = sq + 1.0
                sq = np.sqrt(sq)
                sq = np.abs(theta) + sq
                t = np.where(theta >= 0.0, 1.0, -1.0) / sq
                c = t * t
                c = c + 1.0
                c = np.sqrt(c)
                c = 1.0 / c
                sn = t * c

                def rot(a, b):
                    lo = c * a
                    lo = lo - sn * b
                    hi = sn * a
                    hi = hi + c * b
                    return np.where(on, lo, a), np.where(on, hi, b)

                for k in range(4):
                    M[k][p], M[k][q] = rot(M[k][p], M[k][q])
                for k in range(4):
                    M[p][k], M[q][k] = rot(M[p][k], M[q][k])
                for k in range(4):
                    V[k][p], V[k][q] = rot(V[k][p], V[k][q])
    best = M[0][0]
    out = [V[k][0] for k in range(4)]
    for i in range(1, 4):
        less = M[i][i] < best
        best = np.where(less, M[i][i], best)
        out = [np.where(less, V[k][i], out[k]) for k in range(4)]
    return out


def row_dot(T, r, X, Y, Z):
    """((T[r][0] X + T[r][1] Y) + T[r][2] Z) + T[r][3]"""
    a = T[r, 0] * X
    b = T[r, 1] * Y
    a = a + b
    b = T[r, 2] * Z
    a = a + b
    return a + T[r, 3]


def norm3(x, y, z):
    a = x * x
    b = y * y
    a = a + b
    b = z * z
    a = a + b
    return np.sqrt(a)


def triangulate(P, kp1, kp2, sf1, sf2, idx1, idx2):
    """S11 for the pairs (kp1[idx1[p]], kp2[idx2[p]]) of two key frames with scale factors sf1 / sf2 ->
    (verdict uint8 [n], x3D float32 [n][3]; three zeros for verdicts 1 and 2)"""
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    n = len(idx1)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros((0, 3), f32)
    T1, T2 = P["Tcw1"], P["Tcw2"]
    u1, v1, o1 = kp1["x"][idx1].astype(f32), kp1["y"][idx1].astype(f32), kp1["octave"][idx1]
    u2, v2, o2 = kp2["x"][idx2].astype(f32), kp2["y"][idx2].astype(f32), kp2["octave"][idx2]
    one = np.ones(n, f32)
    with np.errstate(all="ignore"):
        x1, y1 = unproject(P["cam1"], P["model1"], P["precision"], u1, v1)   # :572-573
        x2, y2 = unproject(P["cam2"], P["model2"], P["precision"], u2, v2)

        def ray(T, x, y, i):   # (Rwc xn)_i with Rwc = Rcw^T: (r0 x + r1 y) + r2 z, z = 1 (:575-576)
            a = T[0, i] * x
            b = T[1, i] * y
            a = a + b
            b = T[2, i] * one
            return a + b

        r1 = [ray(T1, x1, y1, i) for i in range(3)]
        r2 = [ray(T2, x2, y2, i) for i in range(3)]
        dot = r1[0] * r2[0]
        t = r1[1] * r2[1]
        dot = dot + t
        t = r1[2] * r2[2]
        dot = dot + t
        n1 = norm3(*r1)
        n2 = norm3(*r2)
        nn = n1 * n2
        cosp = dot / nn                                                      # :577
        limit = 0.9996 if P["inertial"] else 0.9998
        parallax_ok = (cosp > 0) & (cosp.astype(f64) < limit)                # :596-597 without stereo
        # GeometricTools::Triangulate :50-53
        A = [[None] * 4 for _ in range(4)]
        for j in range(4):
            for r, (c, T, base) in enumerate(((x1, T1, 0), (y1, T1, 1), (x2, T2, 0), (y2, T2, 1))):
                a = c * T[2, j]
                A[r][j] = a - T[base, j]
        vv = min_eigenvector(A)
        w_zero = vv[3] == 0.0                                                # :59
        X = (vv[0] / vv[3]).astype(f32)                                      # :63
        Y = (vv[1] / vv[3]).astype(f32)
        Z = (vv[2] / vv[3]).astype(f32)
        z1 = row_dot(T1, 2, X, Y, Z)                                         # :627
        z2 = row_dot(T2, 2, X, Y, Z)                                         # :631
        front1 = z1 > 0
        front2 = z2 > 0
        live = parallax_ok & ~w_zero & front1 & front2
        xc1 = row_dot(T1, 0, X, Y, Z)                                        # :637-638
        yc1 = row_dot(T1, 1, X, Y, Z)
        pu, pv = project(P["cam1"], P["model1"], xc1, yc1, z1, live)         # :643
        ex = pu - u1
        ey = pv - v1
        ex = ex * ex
        ey = ey * ey
        e1 = ex + ey
        bad1 = e1.astype(f64) > 5.991 * P["sigma2_1"][o1].astype(f64)        # :647
        xc2 = row_dot(T2, 0, X, Y, Z)                                        # :665-666
        yc2 = row_dot(T2, 1, X, Y, Z)
        pu, pv = project(P["cam2"], P["model2"], xc2, yc2, z2, live & ~bad1)  # :670
        ex = pu - u2
        ey = pv - v2
        ex = ex * ex
        ey = ey * ey
        e2 = ex + ey
        bad2 = e2.astype(f64) > 5.991 * P["sigma2_2"][o2].astype(f64)        # :673
        dist1 = norm3(X - P["twc1"][0], Y - P["twc1"][1], Z - P["twc1"][2])  # :689-693
        dist2 = norm3(X - P["twc2"][0], Y - P["twc2"][1], Z - P["twc2"][2])
        zero = (dist1 == 0) | (dist2 == 0)                                   # :695
        far = (dist1 >= P["thFarPoints"]) | (dist2 >= P["thFarPoints"]) if P["farPoints"] else np.zeros(n, bool)  # :698
        ratioDist = dist2 / dist1                                            # :701-704
        ratioOctave = np.asarray(sf1, f32)[o1] / np.asarray(sf2, f32)[o2]
        lo = ratioDist * P["ratioFactor"]
        hi = ratioOctave * P["ratioFactor"]
        scale_bad = (lo < ratioOctave) | (ratioDist > hi)
    verdict = np.full(n, ACCEPTED, np.uint8)
    for code, fails in ((SCALE, scale_bad), (FAR, far), (ZERO_DIST, zero), (REPROJ_2, bad2), (REPROJ_1, bad1), (BEHIND_2, ~front2),
                        (BEHIND_1, ~front1), (AT_INFINITY, w_zero), (LOW_PARALLAX, ~parallax_ok)):
        verdict[fails] = code   # later entries are earlier gates: the first failing gate wins
    x3d = np.stack([X, Y, Z], 1).astype(f32)
    x3d[(verdict == LOW_PARALLAX) | (verdict == AT_INFINITY)] = 0
    return verdict, x3d


# ---------------------------------------------------------------------------------------------------------------------
# the same function in binary64 with an SVD
# ---------------------------------------------------------------------------------------------------------------------
def unproject64(cam, model, u, v):
    cam = np.asarray(cam, f64)
    x, y = (u - cam[2]) / cam[0], (v - cam[3]) / cam[1]
    if model == 0:
        return x, y
    td = np.clip(np.hypot(x, y), -np.pi / 2, np.pi / 2)
    th = td.copy()
    for _ in range(50):
        t2 = th * th
        num = th * (1 + cam[4] * t2 + cam[5] * t2**2 + cam[6] * t2**3 + cam[7] * t2**4) - td
        den = 1 + 3 * cam[4] * t2 + 5 * cam[5] * t2**2 + 7 * cam[6] * t2**3 + 9 * cam[7] * t2**4
        th = th - num / den
    s = np.where(td > 1e-8, np.tan(th) / np.where(td > 1e-8, td, 1.0), 1.0)
    return x * s, y * s


def project64(cam, model, x, y, z):
    cam = np.asarray(cam, f64)
    if model == 0:
        return cam[0] * x / z + cam[2], cam[1] * y / z + cam[3]
    th = np.arctan2(np.hypot(x, y), z)
    psi = np.arctan2(y, x)
    r = th + cam[4] * th**3 + cam[5] * th**5 + cam[6] * th**7 + cam[7] * th**9
    return cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]


def triangulate_f64(P, kp1, kp2, sf1, sf2, idx1, idx2):
    """-> (verdict [n], x3D float64 [n][3], margin [n][10]): margin[p][g] = relative distance of the quantity gate g tests
    to its threshold (gates against zero: |z| / (|z| + 1) and the like), for judging verdict flips of the binary32 sequence"""
    idx1, idx2 = np.asarray(idx1, np.int64), np.asarray(idx2, np.int64)
    n = len(idx1)
    T1, T2 = P["Tcw1"].astype(f64), P["Tcw2"].astype(f64)
    u1, v1, o1 = kp1["x"][idx1].astype(f64), kp1["y"][idx1].astype(f64), kp1["octave"][idx1]
    u2, v2, o2 = kp2["x"][idx2].astype(f64), kp2["y"][idx2].astype(f64), kp2["octave"][idx2]
    margin = np.full((n, 10), np.inf)
    with np.errstate(all="ignore"):
        x1, y1 = unproject64(P["cam1"], P["model1"], u1, v1)
        x2, y2 = unproject64(P["cam2"], P["model2"], u2, v2)
        xn1 = np.stack([x1, y1, np.ones(n)], 1)
        xn2 = np.stack([x2, y2, np.ones(n)], 1)
        ray1 = xn1 @ T1[:, :3]   # rows: Rcw^T xn
        ray2 = xn2 @ T2[:, :3]
        cosp = (ray1 * ray2).sum(1) / (np.linalg.norm(ray1, axis=1) * np.linalg.norm(ray2, axis=1))
        limit = 0.9996 if P["inertial"] else 0.9998
        parallax_ok = (cosp > 0) & (cosp < limit)
        margin[:, LOW_PARALLAX] = np.minimum(np.abs(cosp - limit) / limit, np.abs(cosp))
        A = np.stack([x1[:, None] * T1[2] - T1[0], y1[:, None] * T1[2] - T1[1], x2[:, None] * T2[2] - T2[0],
                      y2[:, None] * T2[2] - T2[1]], 1)
        A = np.where(np.isfinite(A), A, 0.0)
        Vt = np.linalg.svd(A)[2]
        vh = Vt[:, 3, :]
        w_zero = vh[:, 3] == 0.0
        margin[:, AT_INFINITY] = np.abs(vh[:, 3])
        X = vh[:, :3] / vh[:, 3:4]
        Xh = np.concatenate([X, np.ones((n, 1))], 1)
        c1 = Xh @ T1.T
        c2 = Xh @ T2.T
        z1, z2 = c1[:, 2], c2[:, 2]
        margin[:, BEHIND_1] = np.abs(z1) / (np.abs(z1) + 1)
        margin[:, BEHIND_2] = np.abs(z2) / (np.abs(z2) + 1)
        pu, pv = project64(P["cam1"], P["model1"], c1[:, 0], c1[:, 1], z1)
        e1 = (pu - u1) ** 2 + (pv - v1) ** 2
        th1 = 5.991 * P["sigma2_1"][o1].astype(f64)
        margin[:, REPROJ_1] = np.abs(e1 - th1) / th1
        pu, pv = project64(P["cam2"], P["model2"], c2[:, 0], c2[:, 1], z2)
        e2 = (pu - u2) ** 2 + (pv - v2) ** 2
        th2 = 5.991 * P["sigma2_2"][o2].astype(f64)
        margin[:, REPROJ_2] = np.abs(e2 - th2) / th2
        dist1 = np.linalg.norm(X - P["twc1"].astype(f64), axis=1)
        dist2 = np.linalg.norm(X - P["twc2"].astype(f64), axis=1)
        zero = (dist1 == 0) | (dist2 == 0)
        margin[:, ZERO_DIST] = np.minimum(dist1, dist2)
        thf = float(P["thFarPoints"])
        far = ((dist1 >= thf) | (dist2 >= thf)) if P["farPoints"] else np.zeros(n, bool)
        if P["farPoints"]:
            margin[:, FAR] = np.minimum(np.abs(dist1 - thf), np.abs(dist2 - thf)) / thf
        ratioDist = dist2 / dist1
        ratioOctave = np.asarray(sf1, f64)[o1] / np.asarray(sf2, f64)[o2]
        rf = float(P["ratioFactor"])
        scale_bad = (ratioDist * rf < ratioOctave) | (ratioDist > ratioOctave * rf)
        margin[:, SCALE] = np.minimum(np.abs(ratioDist * rf - ratioOctave) / ratioOctave,
                                      np.abs(ratioDist - ratioOctave * rf) / (ratioOctave * rf))
    verdict = np.full(n, ACCEPTED, np.uint8)
    for code, fails in ((SCALE, scale_bad), (FAR, far), (ZERO_DIST, zero), (REPROJ_2, e2 > th2), (REPROJ_1, e1 > th1),
                        (BEHIND_2, ~(z2 > 0)), (BEHIND_1, ~(z1 > 0)), (AT_INFINITY, w_zero), (LOW_PARALLAX, ~parallax_ok)):
        verdict[fails] = code
    return verdict, X, margin

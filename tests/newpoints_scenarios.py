"""Scenes with real geometry for "triangulate each match" of LocalMapping::CreateNewMapPoints: a cloud of 3-D points, key
frame 1 at the origin and K neighbours along a path, keypoints = projections + pixel noise at an octave that follows the
depth.  Every gate of src/LocalMapping.cc:571-705 is hit on purpose:

* baselines cycle through 0 ... 4 units (low parallax for the short ones),
* two neighbours are turned by 2.6 rad and three by +-1.2 rad (points behind a camera, negative parallax),
  one is moved 6 units forward (points behind camera 2 only),
* 15 % of the pairs have a wrong partner (the projection of another point): reprojection errors, negative depths,
* pixel noise sigma = 0.5 * scale factor of the octave, x 6 for 10 % of the second keypoints: reprojection gates,
* the octave of the second keypoint is raised by 4 for 8 % and lowered by 4 for another 8 %: scale consistency,
* the far-point gate (30 units) on every other neighbour, inertial parallax limit on two neighbours of three.

A neighbour's feature j IS pair j: it carries the descriptor (a few bits flipped) and the vocabulary node of its key-frame-1
feature, so SearchForTriangulation finds (idx1[j], j) when its own gates let it."""
import numpy as np

import match_scenarios as S
import newpoints_ref as R

PIN_CAM = np.array([458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0])                       # 752 x 480, match_scenarios' camera
KB_CAM = np.array([190.978, 190.973, 254.932, 256.897, 0.00348, 0.000715, -0.00205, 0.000203])  # 512 x 512, TUM-VI like
BASELINES = [0.0, 0.002, 0.02, 0.1, 0.3, 0.6, 1.0, 1.5, 2.5, 4.0]


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def nodes_of(kp, height):
    """vocabulary nodes as test_triangulation_batch.nodes_of: 40-px rows x octave (rows clipped to the image)"""
    row = np.clip(kp["y"] // 40, 0, height // 40).astype(np.int32)
    return (row * 8 + kp["octave"]).astype(np.int32)


def make_kp(uv, octave, angle, kp_dtype):
    kp = np.zeros(len(uv), kp_dtype)
    kp["x"], kp["y"] = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    kp["octave"] = octave
    kp["angle"] = angle.astype(np.float32)
    kp["size"] = 31.0
    kp["response"] = 50
    return kp


def scene(seed, K=20, n_points=1000, model1=0, model2=0, n_levels=8, scale=1.2, cam1=None, cam2=None, height=480,
          pair_frac=0.25, kp_dtype=None, extent=(6.0, 4.0, 2.0, 40.0)):
    """-> dict(kp1, desc1, node1, sf, sigma2, X (the cloud), nbs=[dict(kp, desc, node, has, Tcw, twc, np (newpoints_ref.params),
    idx1, idx2 (pair j = (idx1[j], idx2[j] = position of neighbour feature j)), intended, noise_free, baseline, turned, F12, ep,
    cameras)])"""
    import oracle_py as O
    kp_dtype = kp_dtype or O.KP_DTYPE
    rng = np.random.default_rng(seed)
    cam1 = np.asarray(PIN_CAM if cam1 is None else cam1, np.float64)
    cam2 = np.asarray(cam1 if cam2 is None else cam2, np.float64)
    sf = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(n_levels - 1, np.float32(scale), np.float32)])).astype(np.float32)
    sigma2 = (sf * sf).astype(np.float32)
    ex, ey, z0, z1 = extent
    X = np.stack([rng.uniform(-ex, ex, n_points), rng.uniform(-ey, ey, n_points), rng.uniform(z0, z1, n_points)], 1)
    d1 = np.linalg.norm(X, axis=1)
    oct1 = rng.integers(0, n_levels, n_points)
    size = d1 * scale ** oct1.astype(np.float64)          # the feature is seen at octave log(size / distance)
    uv1 = np.stack(R.project64(cam1, model1, X[:, 0], X[:, 1], X[:, 2]), 1)
    clean1 = rng.random(n_points) < 0.2                    # a share without pixel noise (see noise_free)
    uv1 = uv1 + rng.normal(0, 0.5, (n_points, 2)) * (sf[oct1] * ~clean1)[:, None]
    ang1 = rng.uniform(0, 360, n_points)
    kp1 = make_kp(uv1, oct1, ang1, kp_dtype)
    desc1 = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    node1 = nodes_of(kp1, height)
    T1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    turned_by = {5: 2.6, 13: 2.6, 3: 1.2, 9: -1.2, 16: 1.2}
    nbs = []
    for k in range(K):
        b = BASELINES[k % len(BASELINES)]
        d = rng.normal(0, 0.15, 3) + np.array([1.0, 0.0, 0.0])
        twc = b * d / np.linalg.norm(d)
        ang = rng.normal(0, 0.02, 3)
        turn = turned_by.get(k, 0.0)
        ang[1] += turn
        if k == 7:
            twc = twc + np.array([0.0, 0.0, 6.0])
        Rwc = rot(*ang)
        Rcw = Rwc.T
        Tcw = np.hstack([Rcw, (-Rcw @ twc)[:, None]])
        src = np.sort(rng.choice(n_points, max(1, int(n_points * pair_frac)), replace=False))
        m = len(src)
        wrong = rng.random(m) < 0.15
        seen = np.where(wrong, rng.integers(0, n_points, m), src)   # the point the neighbour's keypoint really shows
        Xc = X[seen] @ Rcw.T + Tcw[:, 3]
        d2 = np.linalg.norm(X[seen] - twc, axis=1)
        o2 = np.clip(np.rint(np.log(size[seen] / d2) / np.log(scale)), 0, n_levels - 1).astype(np.int64)
        u = rng.random(m)
        o2 = np.where(u < 0.08, np.minimum(o2 + 4, n_levels - 1), np.where(u < 0.16, np.maximum(o2 - 4, 0), o2))
        octave_off = u < 0.16
        uv2 = np.stack(R.project64(cam2, model2, Xc[:, 0], Xc[:, 1], Xc[:, 2]), 1)
        noisy = rng.random(m) < 0.10
        clean = rng.random(m) < 0.20                                 # a share without any pixel noise in the second view
        sig = 0.5 * sf[o2] * np.where(noisy, 6.0, 1.0) * np.where(clean & ~noisy, 0.0, 1.0)
        uv2 = uv2 + rng.normal(0, 1.0, (m, 2)) * sig[:, None]
        uv2 = np.where(np.isfinite(uv2), uv2, 0.0)
        a2 = (ang1[src] + rng.normal(0, 2, m)) % 360
        perm = rng.permutation(m)                                    # neighbour feature perm[j] ... shuffled storage order
        inv = np.argsort(perm)
        kp2 = make_kp(uv2, o2, a2, kp_dtype)[perm]
        desc2 = np.stack([S.flip_bits(desc1[s], int(rng.integers(0, 12)), rng) for s in src])[perm]
        node2 = node1[src][perm]
        c = np.float32
        npar = R.params(Tcw1=T1, Tcw2=Tcw, twc1=np.zeros(3), twc2=twc, sigma2_1=sigma2, sigma2_2=sigma2, ratioFactor=c(1.5) * c(scale),
                        model1=model1, model2=model2, cam1=cam1, cam2=cam2, inertial=(k % 3 != 2), farPoints=(k % 2 == 1),
                        thFarPoints=30.0)
        # SearchForTriangulation's own inputs (src/ORBmatcher.cc:448-468): T12 = T1w Tw2, F12, the epipole in key frame 2
        R12, t12 = Rwc, twc
        K1 = np.array([[cam1[0], 0, cam1[2]], [0, cam1[1], cam1[3]], [0, 0, 1]])
        K2 = np.array([[cam2[0], 0, cam2[2]], [0, cam2[1], cam2[3]], [0, 0, 1]])
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
        F12 = (np.linalg.inv(K1).T @ tx @ R12 @ np.linalg.inv(K2)).astype(np.float32)
        C2 = Tcw[:, 3]                                               # camera 1's centre (the origin) in camera 2
        with np.errstate(all="ignore"):
            ep = R.project64(cam2, model2, C2[0], C2[1], C2[2])
        ep = tuple(float(e) if np.isfinite(e) else 1.0e6 for e in ep)
        cameras = dict(model1=model1, model2=model2, cam1=cam1, cam2=cam2, precision=1e-6, R12=R12.astype(np.float32),
                       t12=t12.astype(np.float32), levelSigma2_1=sigma2, kf1HasCamera2=0)
        nbs.append(dict(kp=kp2, desc=desc2, node=node2, has=np.zeros(m, np.uint8), Tcw=Tcw, twc=twc, np=npar, idx1=src.copy(),
                        idx2=inv.copy(), intended=~wrong, noise_free=(clean1[src] & clean & ~noisy & ~wrong & ~octave_off), baseline=b,
                        turned=(turn != 0.0), F12=F12, ep=ep, cameras=cameras))
    return dict(kp1=kp1, desc1=desc1, node1=node1, sf=sf, sigma2=sigma2, X=X, nbs=nbs, cam1=cam1, cam2=cam2, model1=model1,
                model2=model2)


def all_pairs(sc):
    """[(k, verdict, x3D)] of newpoints_ref over the scene's own pair lists"""
    out = []
    for k, nb in enumerate(sc["nbs"]):
        v, x = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], nb["idx1"], nb["idx2"])
        out.append((k, v, x))
    return out


def infinity_case(kp_dtype=None):
    """a pose pair whose null vector has w == 0 exactly (verdict 2): key frame 1 = [I | 0] looking along its optical axis,
    "Tcw2" with a zero first rotation row, so that the fourth column of A is orthogonal to the other three and A^T A splits
    into a 3 x 3 block (which holds the smallest eigenvalue, 0.117) and the entry 1 of the fourth coordinate: the Jacobi
    sequence never mixes the two, the eigenvector is (x, y, z, 0).  The rays still make cos = 0.894."""
    import oracle_py as O
    kp_dtype = kp_dtype or O.KP_DTYPE
    cam = np.array([100.0, 100.0, 0.0, 0.0, 0, 0, 0, 0])
    kp1 = make_kp(np.array([[0.0, 0.0]]), np.array([0]), np.array([0.0]), kp_dtype)
    kp2 = make_kp(np.array([[0.0, 50.0]]), np.array([0]), np.array([0.0]), kp_dtype)
    T1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    T2 = np.array([[0.0, 0, 0, -1.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    sf = np.ones(8, np.float32)
    P = R.params(T1, T2, np.zeros(3), np.array([1.0, 0, 0]), sf, sf, 1.8, cam1=cam, cam2=cam)
    return P, kp1, kp2, sf


def centre_case(kp_dtype=None):
    """a point at a camera centre (verdict 7): an ordinary pair, and GetTranslationInverse() of key frame 2 handed over as the
    very point the pair triangulates to (twc is taken from the caller, S11) -> dist2 == 0"""
    sc = scene(3, K=7, n_points=200, kp_dtype=kp_dtype)
    nb = sc["nbs"][6]
    v, x = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], nb["idx1"], nb["idx2"])
    p = int(np.flatnonzero(v == R.ACCEPTED)[0])
    P = dict(nb["np"], twc2=x[p].copy())
    return P, sc["kp1"], nb["kp"], sc["sf"], nb["idx1"][p:p + 1], nb["idx2"][p:p + 1]

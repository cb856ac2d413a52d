"""Seeded PnP scenes for the S13 tests (tests/test_mlpnp*.py): world points seen from a pose, projections with pixel noise scaled
by the keypoint's octave (0 .. 7), a share of outliers, unmatched keypoints interleaved (correspondence index != keypoint index) and
map points stored in shuffled order (mp_index != correspondence index).

kinds:
  general    points at depth 2 .. 10 in front of a camera that is rotated and shifted against the world frame
  plane      points with world z = 0 exactly (a plane through the world origin: the planar branch, :388)
  identity   pose = identity and noise-free projections: the linear estimate is the identity, omega = 0 (S13 takes the limit of
             the Jacobian there)
  near       a rotation of 1e-3 rad
  pi         a rotation of pi - 1e-3 rad about a tilted axis
  kb8        the general scene seen through a KannalaBrandt8 camera
  junk       random keypoints: no hypothesis qualifies
  two        the general scene, but exactly min_inliers of the keypoints are noise-free projections under a second pose: a min-set
             drawn from them qualifies with exactly min_inliers inliers, becomes a candidate and fails Refine's strict '>' (:335);
             a later min-set from the other points sets a new best and returns (seeds are searched for this order)
"""
import numpy as np

import mlpnp_ref as R

W, H = 752, 480
PINHOLE = (458.654, 457.296, 367.215, 248.375, 0.0, 0.0, 0.0, 0.0)
KB8 = (190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0034823894022493434, 0.0007150348452162257,
       -0.0020532361418706202, 0.00020293673591811182)
N_LEVELS, SCALE = 8, 1.2


def level_sigma2():
    """mvLevelSigma2 as the extractor builds it (src/ORBextractor.cc:92-100)"""
    sf = [np.float32(1.0)]
    for _ in range(1, N_LEVELS):
        sf.append(np.float32(np.float64(sf[-1]) * np.float64(np.float32(SCALE))))
    sf = np.array(sf, np.float32)
    return sf * sf


def _rodrigues(w):
    w = np.asarray(w, np.float64)
    n = np.linalg.norm(w)
    if n == 0:
        return np.eye(3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / n
    return np.eye(3) + np.sin(n) * K + (1 - np.cos(n)) * K @ K


def _project(cam, model, Xc):
    fx, fy, cx, cy, k1, k2, k3, k4 = cam
    if model == 0:
        return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    r = np.hypot(Xc[:, 0], Xc[:, 1])
    th = np.arctan2(r, Xc[:, 2])
    psi = np.arctan2(Xc[:, 1], Xc[:, 0])
    rd = th + k1 * th ** 3 + k2 * th ** 5 + k3 * th ** 7 + k4 * th ** 9
    return np.stack([fx * rd * np.cos(psi) + cx, fy * rd * np.sin(psi) + cy], 1)


def _unproject_rays(cam, model, uv):
    fx, fy, cx, cy = cam[:4]
    x, y = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    if model == 1:  # rays of an (approximately) equidistant lens: good enough to place points inside the image
        rd = np.hypot(x, y)
        s = np.where(rd > 1e-9, np.tan(np.minimum(rd, 1.3)) / np.maximum(rd, 1e-9), 1.0)
        x, y = x * s, y * s
    return np.stack([x, y, np.ones(len(x))], 1)


KINDS = {
    # kind: (structure, omega, camera centre in the world, model, noise in level-0 pixels)
    "general": ("volume", (0.10, -0.20, 0.05), (0.3, -0.2, 0.1), 0, 0.5),
    "plane": ("plane", (0.25, -0.15, 0.05), (0.3, -0.2, -4.0), 0, 0.5),
    "identity": ("volume", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0, 0.0),
    "near": ("volume", (6e-4, -7e-4, 4e-4), (0.02, -0.01, 0.03), 0, 0.5),
    "pi": ("volume", tuple((np.pi - 1e-3) * np.array([0.6, 0.0, 0.8])), (0.3, -0.2, 0.1), 0, 0.5),
    "kb8": ("volume", (0.10, -0.20, 0.05), (0.3, -0.2, 0.1), 1, 0.5),
    "junk": ("volume", (0.10, -0.20, 0.05), (0.3, -0.2, 0.1), 0, 0.5),
    "two": ("volume", (0.10, -0.20, 0.05), (0.3, -0.2, 0.1), 0, 0.5),
}
SECOND_POSE = ((0.14, -0.16, 0.02), (0.1, 0.0, 0.3))  # of kind "two": omega, camera centre


def make(kind, N=300, seed=0, outliers=0.0, min_set=12, epsilon=0.5, n_iterations=20, extra=0.25, min_inliers=50, max_iterations=300):
    """-> dict(cam, model, precision, level_sigma2, kp_xy [n, 2] float32, kp_octave [n], mp_index [n], points [m, 3] float32, sets,
    ransac = dict of the RANSAC parameters, Rcw, tcw)"""
    structure, om, centre, model, noise = KINDS[kind]
    cam = KB8 if model else PINHOLE
    Wd, Hd = (512, 512) if model else (W, H)
    rng = np.random.RandomState(1000 * seed + 17 * N + len(kind) + 131 * min_set)
    Rcw = _rodrigues(om)
    tcw = -Rcw @ np.array(centre, np.float64)
    s2 = level_sigma2()
    uv_all = np.zeros((0, 2))
    Xw_all = np.zeros((0, 3))
    while len(uv_all) < N:
        n = 4 * N
        uv = np.stack([rng.uniform(30, Wd - 30, n), rng.uniform(30, Hd - 30, n)], 1)
        ray = _unproject_rays(cam, model, uv)
        if structure == "plane":  # intersect the viewing ray with the world plane z = 0
            d = ray @ Rcw  # ray direction in the world (Rwc ray)
            o = np.array(centre, np.float64)
            lam = -o[2] / d[:, 2]
            Xw = o + lam[:, None] * d
            Xw[:, 2] = 0.0
            ok = lam > 0.5
        else:
            z = rng.uniform(2.0, 10.0, n)
            Xw = (ray * z[:, None] - tcw) @ Rcw  # Rwc (Xc - tcw)
            ok = np.ones(n, bool)
        Xw = Xw.astype(np.float32).astype(np.float64)  # map points are stored as float
        Xc = Xw @ Rcw.T + tcw
        p = _project(cam, model, Xc)
        ok &= (Xc[:, 2] > 0.2) & (p[:, 0] >= 20) & (p[:, 0] < Wd - 20) & (p[:, 1] >= 20) & (p[:, 1] < Hd - 20)
        uv_all, Xw_all = np.concatenate([uv_all, p[ok]]), np.concatenate([Xw_all, Xw[ok]])
    uv, Xw = uv_all[:N].copy(), Xw_all[:N].copy()
    octave = rng.randint(0, N_LEVELS, N)
    uv = uv + rng.normal(size=(N, 2)) * (noise * np.sqrt(s2[octave].astype(np.float64)))[:, None]
    if kind == "junk":
        outliers = 1.0
    if kind == "two":
        Rb = _rodrigues(SECOND_POSE[0])
        tb = -Rb @ np.array(SECOND_POSE[1], np.float64)
        uv[:min_inliers] = _project(cam, model, Xw[:min_inliers] @ Rb.T + tb)
    nOut = int(round(outliers * N))
    if nOut:
        idx = rng.permutation(N)[:nOut]
        uv[idx] = np.stack([rng.uniform(20, Wd - 20, nOut), rng.uniform(20, Hd - 20, nOut)], 1)
    e = int(extra * N) + 3
    kp = np.concatenate([uv, np.stack([rng.uniform(20, Wd - 20, e), rng.uniform(20, Hd - 20, e)], 1)])
    oc = np.concatenate([octave, rng.randint(0, N_LEVELS, e)])
    perm = rng.permutation(len(kp))
    inv = np.argsort(perm)
    pperm = rng.permutation(N + 5)  # five map points nobody matched
    points = np.zeros((N + 5, 3), np.float32)
    points[pperm[:N]] = Xw
    points[pperm[N:]] = rng.uniform(-3, 3, (5, 3))
    mp_index = np.full(len(kp), -1, np.int32)
    mp_index[inv[:N]] = pperm[:N]
    rp = dict(probability=0.95, min_inliers=min_inliers, max_iterations=max_iterations, min_set=min_set, epsilon=epsilon, th2=5.991,
              n_iterations=n_iterations)
    total = R.plan(N, 0.95, min_inliers, max_iterations, min_set, epsilon, n_iterations)[2]
    sets = R.draw_sets(N, total, min_set, lambda: int(rng.randint(0, 2 ** 31 - 1))) if total else np.zeros((0, min_set), np.int32)
    return dict(cam=np.array(cam, np.float32), model=model, precision=1e-6, level_sigma2=s2, kp_xy=kp[perm].astype(np.float32),
                kp_octave=oc[perm].astype(np.int32), mp_index=mp_index, points=points, sets=sets, ransac=rp, Rcw=Rcw, tcw=tcw, kind=kind,
                N=N)


def ref(sc, exact=False, **kw):
    fn = R.ransac_f64 if exact else R.ransac
    return fn(sc["cam"], sc["model"], sc["precision"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"],
              sc["sets"], **sc["ransac"], **kw)


REFINE_BLOCK = 256  # threads of mlpnp_refine_kernel (csrc/kernels_mlpnp.hip kMlpnpRefineThreads)

# (kind, N, outliers, min_set, epsilon, seed): the comparison set of tests/test_mlpnp.py and tests/test_mlpnp_gpu.py
CASES = [
    ("general", 300, 0.3, 12, 0.5, 0), ("general", 300, 0.0, 12, 0.5, 0), ("plane", 300, 0.3, 12, 0.5, 0), ("identity", 100, 0.0, 12, 0.5, 0),
    ("near", 130, 0.1, 12, 0.5, 0), ("pi", 300, 0.1, 12, 0.5, 0), ("kb8", 100, 0.1, 12, 0.5, 0), ("general", 300, 0.6, 12, 0.5, 0),
    ("junk", 100, 1.0, 12, 0.5, 0),
    ("general", 49, 0.0, 12, 0.5, 0), ("general", 50, 0.0, 12, 0.5, 0), ("general", 64, 0.1, 12, 0.5, 0), ("general", 65, 0.1, 12, 0.5, 0),
    ("general", 130, 0.1, 6, 0.5, 0), ("general", 130, 0.1, 13, 0.5, 0), ("general", REFINE_BLOCK + 1, 0.2, 12, 0.5, 0),
    ("general", 300, 0.3, 12, 0.2, 0), ("two", 102, 0.0, 6, 0.2, 68),
]


def case_id(c):
    return "%s-N%d-o%d-s%d-e%d-seed%d" % (c[0], c[1], int(100 * c[2]), c[3], int(100 * c[4]), c[5])


def make_case(c):
    return make(c[0], c[1], c[5], c[2], c[3], c[4])

"""Seeded scenes for the S23 tests: one frame = an imu_preint_scenarios window, a slice of the resident map seen from the true camera
at the frame's stamp, and keypoints with descriptors on most of those points.  The id list carries the slots the gather kernel and the
statistics have to get right:

  slot 0   ~id            a visible point with a keypoint on it, skipped for this frame (mnLastFrameSeen == current frame)
  slot 1   id >= capacity  no point
  slot 2   behind the camera
  slot 3   outside the image bounds
  slot 4   its keypoint sits 50 px off but carries its descriptor: matched inside the th = 40 radius, rejected by chi^2
  slot 5   observations == 0 with a good keypoint: found, but not counted in mnMatchesInliers
  slot 6   a visible point nobody matches (no keypoint, a descriptor of its own)
  7 ..     ordinary points; the first `n_on` of them have a keypoint

Keypoints are in the coordinates the matcher and the optimiser both compare (S6); a point's distance range is chosen so that
PredictScale gives its keypoint's octave.
"""
import numpy as np

import imu_preint_ref as R22
import imu_preint_scenarios as PS
import track_inertial_ref as T
from match_scenarios import flip_bits
from mlpnp_scenarios import H, N_LEVELS, PINHOLE, SCALE, W

f32, f64 = np.float32, np.float64
GRID = (64, 48)
TH, NN_RATIO = 40.0, 0.75        # src/Tracking.cc:1108-1113 once the IMU is initialised; nnratio of the ORBmatcher built at :1105
N_PLANTED = 7
S_SKIP, S_NOPOINT, S_BEHIND, S_OUTSIDE, S_FAR_KP, S_NO_OBS, S_UNMATCHED = range(N_PLANTED)
KINDS = ("ordinary", "standing", "empty")
# (window of the IMU, what is special): the ordinary frame; fewer than 2 samples -- the records stand; no keypoint at all
ARCHETYPES = {"ordinary": ("moving", 10, 0), "standing": ("bias_changed", 10, 0), "empty": ("moving", 3, 0)}


def _camera_pose(sc):
    traj, t = sc["traj"], sc["rel_cur"]
    Rwb, twb = traj.Rwb(t), traj.p(t)
    Rcb, tcb = sc["Rcb"].astype(f64), sc["tcb"].astype(f64)
    return Rcb @ Rwb.T, Rcb @ (-Rwb.T @ twb) + tcb


def make_frame(kind, M, seed, id_base, capacity, wp_dtype, kp_dtype, n_kp=150, case=None, sc=None):
    """-> dict(sc, which-independent IMU inputs, ids [M], points / desc: the map entries id_base .. id_base + M - 1, kp, kp_desc, n).
    `sc`: a window of the caller's own (track_inertial_sequence) instead of the archetype's"""
    assert M == 0 or M >= N_PLANTED + 8
    case = case or ARCHETYPES[kind]
    sc = sc if sc is not None else PS.make(*case)
    rng = np.random.RandomState(2300 + 31 * seed + M)
    Rt, tt = _camera_pose(sc)
    fx, fy, cx, cy = (float(v) for v in PINHOLE[:4])
    sf = np.float32(SCALE)

    uv = np.stack([rng.uniform(40, W - 40, M), rng.uniform(40, H - 40, M)], 1) if M else np.zeros((0, 2))
    z = rng.uniform(2.0, 18.0, M)
    if M:
        uv[S_OUTSIDE, 0] = W + 60.0
        z[S_BEHIND] = -4.0
    ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(M)], 1)
    Xw = ((ray * z[:, None] - tt) @ Rt).astype(f32)
    Xc = Xw.astype(f64) @ Rt.T + tt
    twc = -Rt.T @ tt
    dist = np.linalg.norm(Xw.astype(f64) - twc, axis=1)
    octave = rng.randint(0, N_LEVELS, M)
    pts = np.zeros(M, wp_dtype)
    lo, hi = wp_dtype.names[3], wp_dtype.names[4]
    pts["x"], pts["y"], pts["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    pts[hi] = dist * float(sf) ** (octave - 0.3)           # ceil(log(max / dist) / log(scale)) == octave
    pts[lo] = pts[hi] / float(sf) ** (N_LEVELS - 1)
    pts["observations"] = rng.randint(1, 5, M)
    desc = rng.randint(0, 256, (M, 32)).astype(np.uint8)
    ids = (id_base + np.arange(M)).astype(np.int32)
    if M:
        pts["observations"][S_NO_OBS] = 0
        ids[S_SKIP] = ~ids[S_SKIP]
        ids[S_NOPOINT] = capacity + 5

    n_on = 0 if kind == "empty" or M == 0 else min(M - N_PLANTED, n_kp - 12)
    on = [S_SKIP, S_FAR_KP, S_NO_OBS] + list(range(N_PLANTED, N_PLANTED + n_on)) if n_on else []
    n = 0 if kind == "empty" else (n_kp if M else 40)
    kp = np.zeros(n, kp_dtype)
    kdesc = rng.randint(0, 256, (n, 32)).astype(np.uint8)   # the keypoints without a point: a random descriptor matches nothing
    if n:
        kp["x"], kp["y"] = rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)
        kp["octave"] = rng.randint(0, N_LEVELS, n)
        kp["size"], kp["angle"], kp["response"] = 31.0, rng.uniform(0, 360, n), 50
    where = rng.permutation(n)[:len(on)]
    for slot, i in zip(on, where):
        u = fx * Xc[slot, 0] / Xc[slot, 2] + cx
        v = fy * Xc[slot, 1] / Xc[slot, 2] + cy
        s = float(sf) ** octave[slot]
        kp["x"][i], kp["y"][i] = u + 0.5 * s * rng.normal(), v + 0.5 * s * rng.normal()
        if slot == S_FAR_KP:
            kp["x"][i] = u + (50.0 if u < W / 2 else -50.0)
        kp["octave"][i] = octave[slot]
        kdesc[i] = flip_bits(desc[slot], int(rng.randint(0, 12)), rng)
    smp = np.zeros(len(sc["t"]), [("t", "<f8"), ("a", "<f4", 3), ("w", "<f4", 3)])
    smp["t"], smp["a"], smp["w"] = sc["t"], sc["a"], sc["w"]
    return dict(kind=kind, case=case, sc=sc, M=M, ids=ids, points=pts, desc=desc, id_base=id_base, kp=kp, kp_desc=kdesc, n=n,
                samples=smp[:1] if kind == "standing" else smp, kp_of_slot=dict(zip(on, (int(i) for i in where))))


def records_in(fr, which):
    """the two records as the call finds them -> (kf Record, frame Record or None): the standing frame has the records the window's
    integration left (the restatement's), every other frame the scene's key-frame record and no frame record yet.  A frame of a
    sequence (track_inertial_sequence) carries the records the frame before left, as fr["records"]"""
    if "records" in fr:
        return fr["records"]
    if fr["kind"] == "standing":
        r = PS.ref_cached(fr["case"], which)
        return r["kf"], r["frame"]
    return fr["sc"]["kf"], None


def start_state(fr, which):
    return fr["sc"]["state_frame"] if which == R22.FROM_FRAME else fr["sc"]["state_kf"]


def prior_of(fr, seed):
    """a ConstraintPoseImu on the previous frame's state, as tests/test_imu_preint_gpu.py builds it"""
    from pose_inertial_scenarios import _spd
    s = fr["sc"]["state_frame"].astype(f64)
    Hp = _spd(np.random.RandomState(40 + seed), [2e4] * 3 + [1e4] * 3 + [2e3] * 3 + [1e6] * 3 + [1e4] * 3, 0.2)
    return dict(Rwb=s[0:9], twb=s[9:12], vwb=s[12:15], bg=s[15:18], ba=s[18:21], H=Hp.reshape(225))


def make_batch(kinds, M, wp_dtype, kp_dtype, seed0=0, cases=None):
    """frames that share one resident map: frame b owns the entries b * M .. (b + 1) * M - 1 -> (frames, capacity, points, desc)"""
    B = len(kinds)
    capacity = max(B * M, 1)
    frames = [make_frame(k, M, seed0 + b, b * M, capacity, wp_dtype, kp_dtype, case=cases[b] if cases else None) for b, k in enumerate(kinds)]
    points = np.concatenate([f["points"] for f in frames]) if M else np.zeros(0, wp_dtype)
    desc = np.concatenate([f["desc"] for f in frames]) if M else np.zeros((0, 32), np.uint8)
    return frames, capacity, points, desc


def frustum_template(F):
    """the fields of an orbfe_frustum / oracle Frustum the chain takes from the template; the pose fields are poisoned"""
    names = {n for n, _ in F._fields_}
    snake = "min_x" in names
    g = (lambda a, b: a) if snake else (lambda a, b: b)
    for k, v in ((g("min_x", "minX"), 0.0), (g("max_x", "maxX"), float(W)), (g("min_y", "minY"), 0.0), (g("max_y", "maxY"), float(H)),
                 ("fx", PINHOLE[0]), ("fy", PINHOLE[1]), ("cx", PINHOLE[2]), ("cy", PINHOLE[3]), ("mbf", 47.9),
                 (g("log_scale_factor", "logScaleFactor"), float(np.log(np.float32(SCALE)))), (g("n_levels", "nLevels"), N_LEVELS),
                 (g("camera_model", "cameraModel"), 0)):
        setattr(F, k, v)
    for name in ("rcw", "tcw", "twc"):
        a = getattr(F, name)
        for i in range(len(a)):
            a[i] = 1e9
    return F


def set_frustum_pose(F, state_in):
    rcw, tcw, twc = T.frustum_pose(state_in)
    for name, v in (("rcw", rcw), ("tcw", tcw), ("twc", twc)):
        a = getattr(F, name)
        for i, x in enumerate(v):
            a[i] = float(x)
    return F


def scale_factors():
    """mvScaleFactor as the extractor builds it (src/ORBextractor.cc:92-100)"""
    sf = [np.float32(1.0)]
    for _ in range(1, N_LEVELS):
        sf.append(np.float32(np.float64(sf[-1]) * np.float64(np.float32(SCALE))))
    return np.array(sf, np.float32)


class CpuStages:
    """the stages of the chain from the restatements (imu_preint_ref, pose_inertial_ref, pose_inertial_prev_ref) and the C oracle
    (isInFrustum, SearchByProjection): no GPU"""

    def imu(self, fr, which):
        """-> (state_in [33], link dict, info_ok)"""
        sc = fr["sc"]
        kf, frame = records_in(fr, which)
        if fr["kind"] != "standing":
            kf, frame, steps = R22.preintegrate_frame(sc["noise"], sc["t"], sc["a"], sc["w"], sc["t_prev"], sc["t_cur"], sc["frame_bias"], kf)
        else:
            steps = np.zeros((0, 8), f32)
        self.last = dict(kf=kf, frame=frame, steps=steps)    # what the IMU stage left in the records, as HostStages keeps it
        return R22.predict(which, start_state(fr, which), kf, frame, sc["gravity"], sc["Rcb"], sc["tcb"], sc["tbc"])

    def project(self, state_in, seen):
        import oracle_py as O
        F = set_frustum_pose(frustum_template(O.Frustum()), state_in)
        return O.is_in_frustum(F, seen.view(O.WP_DTYPE))[0]

    def match(self, kp, kdesc, mps, mpd):
        import oracle_py as O
        fv = O.make_frame_view(kp.view(O.KP_DTYPE), kdesc, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), scale_factors())
        nm, out = O.search_by_projection(fv, mps.view(O.MP_DTYPE), mpd, None, TH, NN_RATIO)
        return nm, out

    def pose(self, which, link, prior, kp, match, rows_xyz, depth, s):
        import pose_inertial_prev_ref as R20
        import pose_inertial_ref as R19
        from mlpnp_scenarios import level_sigma2
        a = (np.array(PINHOLE, f32), level_sigma2(), np.stack([kp["x"], kp["y"]], 1).astype(f32).reshape(-1, 2), kp["octave"].astype(np.int32),
             match, rows_xyz, depth, link)
        tail = (s[0:9], s[9:12], s[12:21], s[21:24], s[24:27], s[27:30], s[30:33])
        r = R20.pose_inertial_optimization_last_frame(*a, prior, *tail) if which == R22.FROM_FRAME else R19.pose_inertial_optimization(*a, *tail)
        # the problem and the restatement's whole result, for the tests that solve it again independently
        self.last_pose = dict(zip(("cam", "level_sigma2", "kp_xy", "kp_octave", "mp_index", "points", "track_depth", "link"), a), prior=prior,
                              Rwb=s[12:21], twb=s[21:24], v=s[24:27], bg=s[27:30], ba=s[30:33], ref=r)
        if which == R22.FROM_FRAME:
            return r, r["H30"], r["accepted"]
        return r, r["H"], 1


def chain(stages, fr, which, capacity, points, desc, prior=None, inlier_threshold=8):
    """S23's chain for one frame through `stages`, taken through the host -> dict of every output of the device call"""
    sc = fr["sc"]
    state_in, link, ok = stages.imu(fr, which)
    M, n = fr["M"], fr["n"]
    seen, mpd, rows = T.resolve_ids(fr["ids"], capacity, points, desc)
    mps = stages.project(state_in, seen) if M else np.zeros(0, seen.dtype)
    nm, match = stages.match(fr["kp"], fr["kp_desc"], mps, mpd) if M and n else (0, np.full(n, -1, np.int32))
    depth = np.ascontiguousarray(mps[mps.dtype.names[3]], f32)
    xyz = np.stack([rows["x"], rows["y"], rows["z"]], 1).astype(f32).reshape(-1, 3)
    r, Hm, accepted = stages.pose(which, link, prior, fr["kp"], np.asarray(match, np.int32), xyz, depth, state_in)
    state_out = np.concatenate([r[k] for k in ("Rwb", "twb", "v", "bg", "ba")]).astype(f32)
    found, mi, tracked = T.statistics(n, match, r["outlier"], mps[mps.dtype.names[7]] if M else [], M, inlier_threshold)
    return dict(state_in=state_in, link=link, info_ok=int(ok), mps=mps, match=np.asarray(match, np.int32), n_matches=int(nm), state_out=state_out,
                H=np.ascontiguousarray(Hm, f64), Hprior=r.get("Hprior"), outlier=np.asarray(r["outlier"], np.uint8), n_inliers=int(r["n_inliers"]),
                accepted=int(accepted), found=found, matches_inliers=mi, tracked=tracked,
                Tcw=T.tcw_out(which, accepted, state_in, state_out, sc["Rcb"], sc["tcb"]), rows=rows, depth=depth)


def planted_verdicts(fr, out):
    """what the planted slots must have led to, read off a chain's outputs -> dict of booleans; a test asserts every one"""
    k = fr["kp_of_slot"]
    mps, match, outl = out["mps"], out["match"], out["outlier"]
    inv, px = mps.dtype.names[5], mps.dtype.names[0]
    return dict(
        skipped_not_in_view=mps[inv][S_SKIP] == 0 and match[k[S_SKIP]] == -1,
        no_point_is_bad=mps["bad"][S_NOPOINT] == 1 and mps[inv][S_NOPOINT] == 0,
        behind_not_in_view=mps[inv][S_BEHIND] == 0 and mps[px][S_BEHIND] == -1.0,
        outside_not_in_view=mps[inv][S_OUTSIDE] == 0 and mps[px][S_OUTSIDE] == -1.0,
        far_keypoint_matched=match[k[S_FAR_KP]] == S_FAR_KP,
        far_keypoint_is_an_outlier=outl[k[S_FAR_KP]] == 1 and out["found"][S_FAR_KP] == 0,
        no_obs_point_is_an_inlier=match[k[S_NO_OBS]] == S_NO_OBS and outl[k[S_NO_OBS]] == 0 and out["found"][S_NO_OBS] == 1,
        no_obs_point_not_counted=out["matches_inliers"] == int(out["found"].sum()) - 1,
        unmatched_slot=mps[inv][S_UNMATCHED] == 1 and not (match == S_UNMATCHED).any() and out["found"][S_UNMATCHED] == 0)

"""Consecutive frames for the S23 tests: what the caller of orbfe_track_frame_inertial / orbfe_track_inertial_batch_device carries from
one frame to the next, restated from the reference lines, and sequences of K frames on ONE imu_preint_scenarios.Trajectory to carry it
over.  No GPU, and no orbfe import at module level.

The between-frames rules (run_sequence):

  branch       against the last frame iff !mbMapUpdated and the PREVIOUS frame left a prior (src/Tracking.cc:940-953: mpcpiExists is read
               from mCurrentFrame->mpPrevFrame); otherwise against the last key frame.
  prior        a key-frame kind always leaves one: its state_out and its H (src/Optimizer.cc:3839).  A last-frame kind leaves one only
               when it is accepted: its state_out and Hprior (:4268 stands inside `if(validPoints >= inlierThreshold)`, :4208).  A rejected
               frame leaves none -- a new Frame starts with mpcpi(nullptr) (src/Frame.cc:59) -- so the frame after it is a key-frame kind.
               The 225 doubles go on "raw", or "clamped": the constructor of ConstraintPoseImu (include/G2oTypes.h:710-721), (H + H) / 2,
               the symmetric eigen-decomposition, eigenvalues below 1e-12 set to 0, recomposed -- applied ONCE, here, in numpy, so that
               every side of a comparison reads the same bytes.  The state of the prior is state_out's floats as doubles.
  start state  after an accepted frame (and after every key-frame kind) the last frame's state is state_out, biases included
               (:4210-4213, :3790-3796); after a rejected frame it is the predicted state_in[12:33] -- :4208-4213 did not run, the pose
               of PredictStateIMU and the bias it copied from the last frame stand.  A key-frame kind starts from the key frame's
               state, which is fixed until there is a new key frame.
  records      the key-frame record a frame leaves is the next frame's input; the frame record is made per frame at the last frame's
               bias; a frame with fewer than two samples predicts from both records as they stand (src/Tracking.cc:235-238).
  new key frame (`fresh`): the last frame becomes the key frame -- its state is the key frame's state from now on, and the key-frame
               record is new IMU::Preintegrated(its bias) (src/Tracking.cc:1339, ImuPreintegrator::Fresh).

Sequences (make_sequence): windows of 10 steps at consecutive k0, the stamp of a frame being the previous stamp of the next; one
resident map of K * M entries, frame k owning the entries k * M .. (k + 1) * M - 1 seen from the TRUE camera pose at frame k's stamp.

  nominal    the scenes' IMU noise; mbMapUpdated at frame 4                              [KF, F, F, F, KF, F]
  weak_imu   noise.cov x 1e4; the SAMPLES keep the scenes' noise (only the weight the optimiser gives the inertial edges falls, so the
             visual edges move the pose); mbMapUpdated at frame 4                        [KF, F, F, F, KF, F]
  events     weak_imu; frame 2 has one IMU sample; frame 3 has no keypoint (its last-frame result is rejected); mbMapUpdated and a new
             key frame at frame 5                                                        [KF, F, F, F(rejected), KF, KF]
"""
import numpy as np

import imu_preint_ref as R22
import imu_preint_scenarios as PS
import track_inertial_scenarios as TS
from mlpnp_scenarios import H, N_LEVELS, PINHOLE, W, _rodrigues

f32, f64 = np.float32, np.float64
KF, F = R22.FROM_KEYFRAME, R22.FROM_FRAME
M_SLOTS = 70
STEPS = 10
PRE = 30   # the key frame lies 30 steps before the frame in front of frame 0: the key-frame record holds them, as in imu_preint_scenarios
EXTRACTOR_ARGS = (1000, 40000, 1.2, 8, 20, 7, W, H)
SEQUENCES = {
    "nominal": dict(cov_scale=1.0, standing=(), empty=(), map_updated=(4,), fresh=()),
    "weak_imu": dict(cov_scale=1e4, standing=(), empty=(), map_updated=(4,), fresh=()),
    "events": dict(cov_scale=1e4, standing=(2,), empty=(3,), map_updated=(5,), fresh=(5,)),
    # not one of the three: the new key frame IS the rejected frame, the one place where the start state a rejection leaves reaches
    # the next frame's state_out (see test_wrong_rules_change_bytes)
    "events_kf_rejected": dict(cov_scale=1e4, standing=(2,), empty=(), few=(3,), map_updated=(4,), fresh=(4,)),
}
BRANCHES = {"nominal": [KF, F, F, F, KF, F], "weak_imu": [KF, F, F, F, KF, F], "events": [KF, F, F, F, KF, KF],
            "events_kf_rejected": [KF, F, F, F, KF, F]}
WRONG_RULES = ("stale_prior", "state_out_after_rejection")

_cache = {}


def _windows(rng, traj, K, b_true):
    """-> the window between the key frame and the frame before frame 0 (PRE steps), then the K frames' windows"""
    out = [PS._window(rng, traj, 40, PRE, b_true)]
    for k in range(K):
        w = PS._window(rng, traj, 40 + PRE + STEPS * k, STEPS, b_true)
        w["t_prev"], w["rel_prev"] = out[-1]["t_cur"], out[-1]["rel_cur"]   # the stamps abut as the samples do: the last frame's stamp
        out.append(w)
    return out


def _true_view(sc):
    Rt, tt = TS._camera_pose(sc)
    return dict(rcw=Rt.reshape(9), tcw=tt, twc=-Rt.T @ tt, fx=float(PINHOLE[0]), fy=float(PINHOLE[1]), cx=float(PINHOLE[2]), cy=float(PINHOLE[3]))


def _image_frame(fr, k, seed, M, capacity, wp_dtype, empty, last_kp):
    """the frame's keypoints from the C oracle's extraction of a synthetic image, its map entries on those keypoints under the true pose"""
    import frustum_scenarios as FS
    import oracle_py as O
    from orbfe import synth
    key = ("image", k, seed, empty)
    if key not in _cache:
        img = np.full((H, W), 128, np.uint8) if empty else synth.frame(W, H, 10 * seed + k)
        ex = O.Extractor(*EXTRACTOR_ARGS)
        kp, kdesc, _per = ex.extract(img)
        _cache[key] = (img, kp, kdesc)
    img, kp, kdesc = _cache[key]
    assert (len(kp) == 0) if empty else (len(kp) > 300), len(kp)
    src_kp, src_desc = (kp, kdesc) if len(kp) else last_kp   # a frame without keypoints still has local map points in view
    pts, mpd = FS.world_points_on_keypoints(src_kp, src_desc, _true_view(fr["sc"]), M, np.random.default_rng(2400 + 10 * seed + k), N_LEVELS, wp_dtype)
    ids = (fr["id_base"] + np.arange(M)).astype(np.int32)
    ids = np.where(pts["skip"] != 0, ~ids, ids).astype(np.int32)
    ids[4] = capacity + 1
    pts["skip"] = 0
    fr.update(image=img, kp=kp.view(fr["kp"].dtype).copy(), kp_desc=kdesc, n=len(kp), ids=ids, points=pts, desc=mpd, kp_of_slot={})
    return fr


def make_sequence(name, K=6, seed=0, form="planted", M=M_SLOTS):
    """-> dict(name, K, frames [K] (track_inertial_scenarios.make_frame's dicts, `image` added in the image form), capacity, points, desc,
    state_kf0 / state0 (the key frame's and the last frame's true state before frame 0), kf0 (the key-frame record between them),
    noise, map_updated, fresh, traj)"""
    key = (name, K, seed, form, M)
    if key in _cache:
        return _cache[key]
    import orbfe
    ev = SEQUENCES[name]
    rng = np.random.RandomState(2400 + 97 * seed)
    traj = PS.Trajectory(rng, False)
    b_true = np.concatenate([0.01 * rng.normal(size=3), 0.05 * rng.normal(size=3)])
    noise = R22.Noise()
    noise.cov = (noise.cov * f32(ev["cov_scale"])).astype(f32)
    Rcb = (_rodrigues((0.02, -1.55, 0.03)) @ _rodrigues((0.0, 0.0, 1.57))).astype(f32)
    tcb = np.array([0.05, -0.02, 0.01], f32)
    tbc = (-Rcb.astype(f64).T @ tcb.astype(f64)).astype(f32)
    pre_w, *wins = _windows(rng, traj, K, b_true)
    b1 = b_true.astype(f32)
    kf0, _, _ = R22.preintegrate_frame(noise, pre_w["t"], pre_w["a"], pre_w["w"], pre_w["t_prev"], pre_w["t_cur"], b1, R22.Record(b1),
                                       counts=R22.collections.Counter())
    capacity = K * M
    frames, last_kp = [], None
    for k, win in enumerate(wins):
        sc = dict(win)
        sc.update(noise=noise, gravity=PS.GRAVITY, Rcb=Rcb, tcb=tcb, tbc=tbc, traj=traj, kind="moving", n=STEPS, seed=seed)
        kind = "standing" if k in ev["standing"] else ("empty" if k in ev["empty"] else "ordinary")
        fr = TS.make_frame(kind, M, 100 * seed + k, k * M, capacity, orbfe.WP_DTYPE, orbfe.KP_DTYPE, n_kp=14 if k in ev.get("few", ()) else 150,
                           case=("moving", STEPS, seed), sc=sc)
        if form == "image":
            fr = _image_frame(fr, k, seed, M, capacity, orbfe.WP_DTYPE, kind == "empty", last_kp)
            if fr["n"]:
                last_kp = (fr["kp"], fr["kp_desc"])
        frames.append(fr)
    seq = dict(name=name, K=K, seed=seed, form=form, M=M, frames=frames, capacity=capacity, points=np.concatenate([f["points"] for f in frames]),
               desc=np.concatenate([f["desc"] for f in frames]), state_kf0=traj.state(pre_w["rel_prev"], b1), state0=traj.state(wins[0]["rel_prev"], b1), kf0=kf0, noise=noise,
               map_updated=tuple(ev["map_updated"]), fresh=tuple(ev["fresh"]), traj=traj)
    _cache[key] = seq
    return seq


def clamp_prior_hessian(H225):
    """the constructor of ConstraintPoseImu (include/G2oTypes.h:710-721) in numpy -> 225 doubles"""
    Hm = np.asarray(H225, f64).reshape(15, 15)
    Hm = (Hm + Hm) / 2.0                         # :714, as written: H + H, not H + H^T
    lam, V = np.linalg.eigh(Hm)                  # SelfAdjointEigenSolver reads the lower triangle, as eigh does
    lam = np.where(lam < 1e-12, 0.0, lam)
    return np.ascontiguousarray((V * lam[None, :]) @ V.T).reshape(225)


def prior_from(out, which, prior_mode):
    """the ConstraintPoseImu a frame leaves for the next one, or None"""
    if which == F and not out["accepted"]:
        return None
    Hm = np.asarray(out["Hprior"] if which == F else out["H"], f64).reshape(225)
    if prior_mode == "clamped":
        Hm = clamp_prior_hessian(Hm)
    else:
        assert prior_mode == "raw"
    s = np.asarray(out["state_out"], f32).astype(f64)
    return dict(Rwb=s[0:9], twb=s[9:12], vwb=s[12:15], bg=s[15:18], ba=s[18:21], H=Hm.copy())


def as_record(r, n_steps=None):
    """a Record of the restatement from what a stage left: a Record, or the bytes of an orbfe_imu_preint"""
    if r is None or isinstance(r, R22.Record):
        return r
    b = bytes(r)
    return R22.Record.from_floats(np.frombuffer(b, f32, 298, 8), int(np.frombuffer(b, np.int32, 1, 4)[0]))


def frame_inputs(seq, k, car):
    """frame k of the sequence with what is carried into it -> (frame dict for track_inertial_scenarios.chain, which, prior)"""
    if k in seq["fresh"]:   # the last frame became a key frame
        car["kf_state"] = car["last_state"]
        car["kf_rec"] = R22.Record(car["last_state"][15:21])
    which = F if (k not in seq["map_updated"] and car["prior"] is not None) else KF
    fr = dict(seq["frames"][k])
    sc = dict(fr["sc"])
    sc.update(kf=car["kf_rec"], state_kf=car["kf_state"], state_frame=car["last_state"], frame_bias=car["last_state"][15:21].copy())
    fr.update(sc=sc, records=(car["kf_rec"], car["frame_rec"]))
    return fr, which, (car["prior"] if which == F else None)


def carry_on(car, which, out, prior_mode, wrong=None):
    """the rules of the module's header: what frame k's outputs leave for frame k + 1"""
    rejected = which == F and not out["accepted"]
    left = prior_from(out, which, prior_mode)
    if not (rejected and wrong == "stale_prior"):
        car["prior"] = left
    if rejected and wrong != "state_out_after_rejection":
        car["last_state"] = np.asarray(out["state_in"], f32)[12:33].copy()
    else:
        car["last_state"] = np.asarray(out["state_out"], f32).copy()
    car["kf_rec"], car["frame_rec"] = as_record(out["kf_rec"]), as_record(out["frame_rec"])


def start_of(seq):
    return dict(kf_state=np.asarray(seq["state_kf0"], f32), last_state=np.asarray(seq["state0"], f32), kf_rec=seq["kf0"].copy(), frame_rec=None,
                prior=None)


def run_sequence(stages, seq, prior_mode, wrong=None):
    """the chain over the frames of `seq` through `stages` (CpuStages: the restatements; HostStages: the host-pointer entry points)
    -> per frame the dict of track_inertial_scenarios.chain plus which, prior (what went in), kf_rec / frame_rec / steps (what the
    IMU stage left; link_bytes with HostStages), start (the 21 floats the prediction started from) and, with CpuStages, pose (the
    optimiser's problem and the restatement's whole result).  `wrong`: one of WRONG_RULES, for the test that the
    comparison can tell the rules apart."""
    car = start_of(seq)
    outs = []
    for k in range(seq["K"]):
        fr, which, prior = frame_inputs(seq, k, car)
        out = TS.chain(stages, fr, which, seq["capacity"], seq["points"], seq["desc"], prior)
        last = stages.last
        out.update(which=which, prior=prior, kf_rec=last["kf"], frame_rec=last["frame"], steps=last["steps"],
                   start=TS.start_state(fr, which).copy(), frame_bias=fr["sc"]["frame_bias"], pose=getattr(stages, "last_pose", None), link_bytes=last.get("link"))
        carry_on(car, which, out, prior_mode, wrong)
        outs.append(out)
    return outs


def cpu_run(name, prior_mode="raw", seed=0, form="planted", wrong=None, K=6):
    """run_sequence(CpuStages) once per session"""
    key = ("run", name, prior_mode, seed, form, wrong, K)
    if key not in _cache:
        _cache[key] = run_sequence(TS.CpuStages(), make_sequence(name, K, seed, form), prior_mode, wrong)
    return _cache[key]


def true_state(seq, k):
    """the trajectory's Rwb (3 x 3), twb, v at frame k's stamp, binary64"""
    traj, t = seq["traj"], seq["frames"][k]["sc"]["rel_cur"]
    return traj.Rwb(t), traj.p(t), traj.v(t)

"""orbfe_track_inertial_batch_device and orbfe_track_frame_inertial on the GPU (SPEC DECISION S23).  The oracle is the chain of the
EXISTING host-pointer calls, taken through the host, per frame: orbfe_imu_preintegrate_frame + orbfe_imu_predict, the frustum in numpy
(track_inertial_ref), orbfe_project_map_points on the id-resolved points, orbfe_match_projection with init_obs = None,
orbfe_pose_inertial_optimization_last_keyframe / _last_frame with mp_index = the matches, the resident rows and the records'
track_depth, and the statistics in numpy.  Every output of the new calls is compared with it byte for byte; no tolerance.  The batch
call is compared a second time with the chain of restatements and the C oracle, which share no code with the device.

The shapes are the smallest at which the new kernels can go wrong: 3 frames with 70 id slots (over one wave, no multiple of 64) and
with 300 (two blocks of the gather kernel), 150 keypoints a frame, kp_stride 200; frame 0 ordinary, frame 1 with one IMU sample (the
records stand, the prediction reads them), frame 2 without keypoints; the planted slots of track_inertial_scenarios.  Before anything
is compared, the restatements alone (no GPU) must reach every planted verdict: a scene that does not fails the test."""
import numpy as np
import pytest

import imu_preint_ref as R22
import imu_preint_scenarios as PS
import track_inertial_ref as T
import track_inertial_scenarios as TS
from mlpnp_scenarios import H, PINHOLE, W

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
WHICH = ((R22.FROM_KEYFRAME, "keyframe"), (R22.FROM_FRAME, "frame"))
KP_STRIDE = 200
REC_BYTES = 1200
f32 = np.float32


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


def params_of(sc, which):
    import orbfe
    tp = orbfe.TrackParams()
    tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y = TS.GRID[0], TS.GRID[1], 0.0, 0.0
    tp.grid_inv_w, tp.grid_inv_h = float(f32(TS.GRID[0]) / f32(W)), float(f32(TS.GRID[1]) / f32(H))
    tp.th, tp.nn_ratio, tp.far_points, tp.th_far_points = TS.TH, TS.NN_RATIO, 0, 0.0
    cam = np.array(PINHOLE, f32)
    return orbfe.TrackInertialParams(track=tp, noise=orbfe.ImuNoise(sc["noise"].cov, sc["noise"].walk),
                                     predict=orbfe.ImuPredictParams(which, sc["gravity"], sc["Rcb"], sc["tcb"], sc["tbc"]),
                                     frustum=TS.frustum_template(orbfe.Frustum()), pose_keyframe=orbfe.PoseInertialParams(cam),
                                     pose_frame=orbfe.PoseInertialPrevParams(cam))


def _rec(orbfe, r):
    return orbfe.ImuPreint(r.floats(), r.n_steps)


class HostStages:
    """the stages of the chain as the existing host-pointer entry points; `last` keeps what the IMU stage left in the records"""

    def __init__(self, ex):
        import orbfe
        self.ex, self.o, self.m = ex, orbfe, orbfe.ORBmatcher(ex)

    def imu(self, fr, which):
        o, sc = self.o, fr["sc"]
        par = params_of(sc, which)
        kf_in, frame_in = TS.records_in(fr, which)
        kf = _rec(o, kf_in)
        frame, steps, n = o.imu_preintegrate_frame(self.ex, par.noise, fr["samples"], sc["t_prev"], sc["t_cur"], sc["frame_bias"], kf)
        if fr["kind"] == "standing":
            assert n == 0 and bytes(frame) == bytes(o.ImuPreint())        # fewer than two samples: nothing is touched
            frame = _rec(o, frame_in)
        state, link, ok = o.imu_predict(self.ex, par.predict, TS.start_state(fr, which), kf, frame)
        self.last = dict(kf=bytes(kf), frame=bytes(frame), steps=steps.tobytes(), link=bytes(link))
        return state, link, ok

    def project(self, state_in, seen):
        F = TS.set_frustum_pose(TS.frustum_template(self.o.Frustum()), state_in)
        return self.m.isInFrustum_batch(F, seen)[0]

    def match(self, kp, kdesc, mps, mpd):
        fv = self.o.make_frame_view(kp, kdesc, TS.GRID[0], TS.GRID[1], 0.0, 0.0, float(W), float(H), self.ex.mvScaleFactor)
        return self.m.SearchByProjection(fv, mps, mpd, TS.TH, False, 0.0, TS.NN_RATIO, None)

    def pose(self, which, link, prior, kp, match, xyz, depth, s):
        o = self.o
        cam = np.array(PINHOLE, f32)
        tail = (s[0:9], s[9:12], s[12:21], s[21:24], s[24:27], s[27:30], s[30:33])
        if which == R22.FROM_FRAME:
            r = o.pose_inertial_optimization_last_frame(self.ex, o.PoseInertialPrevParams(cam), link, prior, kp, match, xyz, depth, *tail,
                                                        want_info=False)
            return r, r["H30"], r["accepted"]
        r = o.pose_inertial_optimization_last_keyframe(self.ex, o.PoseInertialParams(cam), link, kp, match, xyz, depth, *tail, want_info=False)
        return r, r["H"], 1


def host_chain(ex, fr, which, capacity, points, desc, prior):
    st = HostStages(ex)
    out = TS.chain(st, fr, which, capacity, points, desc, prior)
    out.update(kf=st.last["kf"], frame=st.last["frame"], steps=st.last["steps"], link=st.last["link"])
    return out


def _dev(t, a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return t.zeros(16, dtype=t.uint8, device="cuda")
    return t.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def run_device(ex, frames, which, capacity, points, desc, priors, want_steps=True, want_hprior=True):
    """the frames as ONE orbfe_track_inertial_batch_device call on a stream of its own, every output poisoned first -> per frame the
    dict host_chain() gives, bytes where that has bytes"""
    import torch
    import orbfe
    B, M = len(frames), frames[0]["M"]
    from_frame = which == R22.FROM_FRAME
    mp = orbfe.MapPoints(ex, capacity)
    if M:
        mp.update(np.arange(capacity), points, desc)
    smp = np.concatenate([f["samples"] for f in frames])
    off = np.cumsum([0] + [len(f["samples"]) for f in frames]).astype(np.int32)
    kf = np.zeros((B, REC_BYTES), np.uint8)
    fr_in = np.full((B, REC_BYTES), 0xCD, np.uint8)
    kp = np.zeros((B, KP_STRIDE), orbfe.KP_DTYPE)
    kd = np.zeros((B, KP_STRIDE, 32), np.uint8)
    for b, f in enumerate(frames):
        k, fi = TS.records_in(f, which)
        kf[b] = np.frombuffer(bytes(_rec(orbfe, k)), np.uint8)
        if fi is not None:
            fr_in[b] = np.frombuffer(bytes(_rec(orbfe, fi)), np.uint8)
        kp[b, :f["n"]], kd[b, :f["n"]] = f["kp"], f["kp_desc"]
    sc0 = frames[0]["sc"]
    ins = dict(d_samples=smp, d_t_prev=np.array([f["sc"]["t_prev"] for f in frames], np.float64),
               d_t_cur=np.array([f["sc"]["t_cur"] for f in frames], np.float64),
               d_frame_bias=np.stack([f["sc"]["frame_bias"] for f in frames]).astype(f32),
               d_state1=np.stack([TS.start_state(f, which) for f in frames]).astype(f32), d_kf=kf, d_frame=fr_in, d_kp=kp, d_desc=kd,
               d_n=np.array([f["n"] for f in frames], np.int32), d_ids=np.stack([f["ids"] for f in frames]).astype(np.int32))
    if from_frame:
        ins["d_priors"] = np.frombuffer(b"".join(bytes(orbfe.PoseImuPrior(p)) for p in priors), np.uint8)
    dev = {k: _dev(torch, v) for k, v in ins.items()}
    hdoubles = 900 if from_frame else 225
    nsteps = max(int(off[-1]), 1)
    shapes = dict(d_steps_out=(nsteps * 32, torch.uint8, 0xAB), d_state_in=(B * 33, torch.float32, -7.0), d_info_ok=(B, torch.int32, -3),
                  d_mp_out=(max(B * M, 1) * 32, torch.uint8, 0xAB), d_match_out=(B * KP_STRIDE, torch.int32, -77),
                  d_n_matches=(B, torch.int32, -3), d_state_out=(B * 21, torch.float32, -7.0), d_H_out=(B * hdoubles, torch.float64, -7.0),
                  d_Hprior_out=(B * 225, torch.float64, -7.0), d_outlier=(B * KP_STRIDE, torch.uint8, 0xAB), d_n_inliers=(B, torch.int32, -3),
                  d_accepted=(B, torch.int32, -3), d_found=(max(B * M, 1), torch.uint8, 0xAB), d_matches_inliers=(B, torch.int32, -3),
                  d_tracked=(B, torch.int32, -3), d_Tcw_out=(B * 12, torch.float32, -7.0))
    for k, (n, dt, fill) in shapes.items():
        dev[k] = torch.full((n,), fill, dtype=dt, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    if not want_steps:
        ptrs["d_steps_out"] = None
    if not (from_frame and want_hprior):
        ptrs["d_Hprior_out"] = None
    if M == 0:
        ptrs["d_ids"] = ptrs["d_mp_out"] = ptrs["d_found"] = None
    io, keep = orbfe.track_inertial_io(off, **ptrs)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    orbfe.track_inertial_batch_device(ex, params_of(sc0, which), B, KP_STRIDE, mp, M, io, st.cuda_stream)
    st.synchronize()
    del keep
    host = {k: v.cpu().numpy() for k, v in dev.items() if k in shapes or k in ("d_kf", "d_frame")}
    mp.close()
    mp_dt = orbfe.MP_DTYPE
    out = []
    for b, f in enumerate(frames):
        n = f["n"]
        nst = max(len(f["samples"]) - 1, 0)
        lo = int(off[b]) * 32
        steps = host["d_steps_out"]
        if want_steps:
            assert (steps[lo + 32 * nst:int(off[b + 1]) * 32] == 0xAB).all(), "frame %d: bytes beyond its steps written" % b
        else:
            assert (steps == 0xAB).all()
        out.append(dict(
            state_in=host["d_state_in"].reshape(B, 33)[b], info_ok=int(host["d_info_ok"][b]),
            kf=host["d_kf"].reshape(B, REC_BYTES)[b].tobytes(), frame=host["d_frame"].reshape(B, REC_BYTES)[b].tobytes(),
            steps=steps[lo:lo + 32 * nst].tobytes() if want_steps else None,
            mps=host["d_mp_out"][:B * M * 32].view(mp_dt).reshape(B, M)[b] if M else np.zeros(0, mp_dt),
            match=host["d_match_out"].reshape(B, KP_STRIDE)[b, :n], n_matches=int(host["d_n_matches"][b]),
            state_out=host["d_state_out"].reshape(B, 21)[b], H=host["d_H_out"].reshape(B, hdoubles)[b],
            Hprior=host["d_Hprior_out"].reshape(B, 225)[b] if from_frame and want_hprior else None,
            outlier=host["d_outlier"].reshape(B, KP_STRIDE)[b, :n], n_inliers=int(host["d_n_inliers"][b]), accepted=int(host["d_accepted"][b]),
            found=host["d_found"][:B * M].reshape(B, M)[b] if M else np.zeros(0, np.uint8), matches_inliers=int(host["d_matches_inliers"][b]),
            tracked=int(host["d_tracked"][b]), Tcw=host["d_Tcw_out"].reshape(B, 12)[b],
            untouched=bool((host["d_outlier"].reshape(B, KP_STRIDE)[b, n:] == 0xAB).all())))
        if not (from_frame and want_hprior):
            assert (host["d_Hprior_out"] == -7.0).all()
    return out


INTS = ("info_ok", "n_matches", "n_inliers", "accepted", "matches_inliers", "tracked")
BYTES = ("state_in", "mps", "match", "state_out", "H", "outlier", "found", "Tcw")


def same(got, want, what, records=True):
    for k in INTS:
        assert got[k] == want[k], "%s: %s %r != %r" % (what, k, got[k], want[k])
    for k in BYTES:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), "%s: %s" % (what, k)
    if want.get("Hprior") is not None and got.get("Hprior") is not None:
        assert np.ascontiguousarray(got["Hprior"]).tobytes() == np.ascontiguousarray(want["Hprior"]).tobytes(), "%s: Hprior" % what
    if records:
        for k in ("kf", "frame"):
            assert got[k] == want[k], "%s: the %s record" % (what, k)
        if got.get("steps") is not None and want.get("steps") is not None:
            assert got["steps"] == want["steps"], "%s: steps" % what


def priors_of(frames, which):
    return [TS.prior_of(f, b) for b, f in enumerate(frames)] if which == R22.FROM_FRAME else [None] * len(frames)


def restatements_reach_the_planted_verdicts(frames, which, capacity, points, desc, priors):
    """no GPU: the chain of restatements (and the C oracle for isInFrustum / SearchByProjection) -> its outputs per frame"""
    outs = []
    for b, fr in enumerate(frames):
        out = TS.chain(TS.CpuStages(), fr, which, capacity, points, desc, priors[b])
        outs.append(out)
        if fr["n"] == 0:
            continue
        v = TS.planted_verdicts(fr, out)
        assert all(v.values()), (b, v)
        assert out["outlier"].sum() >= 1 and out["found"][TS.S_NO_OBS] == 1 and points["observations"][fr["id_base"] + TS.S_NO_OBS] == 0
    return outs


@pytest.mark.parametrize("which,wname", WHICH, ids=[w[1] for w in WHICH])
@pytest.mark.parametrize("M", (70, 300))
def test_batch_equals_the_chain_of_host_calls(ex, M, which, wname):
    import orbfe
    frames, capacity, points, desc = TS.make_batch(TS.KINDS, M, orbfe.WP_DTYPE, orbfe.KP_DTYPE)
    priors = priors_of(frames, which)
    restated = restatements_reach_the_planted_verdicts(frames, which, capacity, points, desc, priors)
    want = [host_chain(ex, f, which, capacity, points, desc, priors[b]) for b, f in enumerate(frames)]
    for b, f in enumerate(frames):
        if f["n"]:
            v = TS.planted_verdicts(f, want[b])
            assert all(v.values()), (b, v)      # found differs from "matched"; an inlier is not counted
            assert want[b]["n_matches"] > int(want[b]["found"].sum()) > want[b]["matches_inliers"] > 30
        else:
            assert want[b]["n_matches"] == 0 and want[b]["matches_inliers"] == 0 and want[b]["tracked"] == 0
    got = run_device(ex, frames, which, capacity, points, desc, priors)
    for b, (g, w) in enumerate(zip(got, want)):
        print(wname, M, b, frames[b]["kind"], "matches", g["n_matches"], "inliers", g["n_inliers"], "counted", g["matches_inliers"])
        same(g, w, "%s, M = %d, frame %d (%s)" % (wname, M, b, frames[b]["kind"]))
        same(g, restated[b], "%s, M = %d, frame %d against the restatements" % (wname, M, b), records=False)
        assert g["untouched"], "outlier flags beyond d_n written"
        assert not g["found"][[TS.S_SKIP, TS.S_NOPOINT, TS.S_BEHIND, TS.S_OUTSIDE, TS.S_UNMATCHED]].any()   # written, and 0
    # a second run, without the optional outputs, gives the same bytes
    again = run_device(ex, frames, which, capacity, points, desc, priors, want_steps=False, want_hprior=False)
    for b, (g, a) in enumerate(zip(got, again)):
        same(a, g, "second run, frame %d" % b)


@pytest.mark.parametrize("which,wname", WHICH, ids=[w[1] for w in WHICH])
def test_no_map_points_is_the_inertial_edges_alone(ex, which, wname):
    """M == 0: state and Hessian equal the pose optimisation with no visual edge; nothing is matched, found or counted"""
    import orbfe
    frames, capacity, points, desc = TS.make_batch(TS.KINDS, 0, orbfe.WP_DTYPE, orbfe.KP_DTYPE)
    priors = priors_of(frames, which)
    want = [host_chain(ex, f, which, capacity, points, desc, priors[b]) for b, f in enumerate(frames)]
    got = run_device(ex, frames, which, capacity, points, desc, priors)
    for b, (g, w) in enumerate(zip(got, want)):
        assert w["n_matches"] == 0 and w["n_inliers"] == 0 and w["matches_inliers"] == 0 and w["tracked"] == 0 and not w["outlier"].any()
        assert (w["match"] == -1).all() and len(w["match"]) == frames[b]["n"]
        same(g, w, "%s, no map points, frame %d" % (wname, b))


def test_batch_of_70_mixed_frames_equals_single_frame_batches(ex):
    """isolation: 70 frames (more blocks than a frame has waves) of all three kinds, windows of 1, 2, 3, 10, chunk - 1 and chunk + 1
    steps and their own points and keypoints, against the same frames one call each"""
    import orbfe
    counts = (1, 2, 3, 10, R22.CHUNK - 1, R22.CHUNK + 1)
    rng = np.random.RandomState(70)
    kinds = [TS.KINDS[i] for i in rng.permutation(np.repeat(np.arange(3), 24))[:70]]
    cases = [("bias_changed", 10, 0) if k == "standing" else ("moving", int(counts[rng.randint(len(counts))]), 0) for k in kinds]
    assert set(kinds) == set(TS.KINDS)
    M = 70
    frames, capacity, points, desc = TS.make_batch(kinds, M, orbfe.WP_DTYPE, orbfe.KP_DTYPE, seed0=100, cases=cases)
    for which, wname in WHICH:
        priors = priors_of(frames, which)
        got = run_device(ex, frames, which, capacity, points, desc, priors)
        for b in range(len(frames)):
            one = run_device(ex, frames[b:b + 1], which, capacity, points, desc, priors[b:b + 1])[0]
            same(got[b], one, "frame %d (%s, %s), %s" % (b, kinds[b], PS.case_id(cases[b]), wname))
        assert sum(g["tracked"] for g in got) == sum(k != "empty" for k in kinds)


@pytest.mark.parametrize("which,wname", WHICH, ids=[w[1] for w in WHICH])
def test_track_frame_inertial_equals_extract_and_the_chain(ex, which, wname):
    """the host-pointer call on a synthetic image: extraction, then the chain, bytes throughout"""
    import orbfe
    import frustum_scenarios as FS
    from orbfe import synth
    img = synth.frame(W, H, 3)
    kp, kdesc = ex.extractFeatures(img)
    assert len(kp) > 300
    fr = TS.make_frame("ordinary", 0, 0, 0, 1, orbfe.WP_DTYPE, orbfe.KP_DTYPE)
    st = HostStages(ex)
    state_in, _link, _ok = st.imu(fr, which)
    rcw, tcw, twc = T.frustum_pose(state_in)
    v = dict(rcw=rcw, tcw=tcw, twc=twc, fx=PINHOLE[0], fy=PINHOLE[1], cx=PINHOLE[2], cy=PINHOLE[3])
    M = 400
    pts, mpd = FS.world_points_on_keypoints(kp, kdesc, v, M, np.random.default_rng(23), ex.nlevels, orbfe.WP_DTYPE)
    capacity = M + 10
    ids = np.random.RandomState(5).permutation(capacity)[:M].astype(np.int32)
    ids[3], ids[4] = ~ids[3], capacity + 1
    points, desc = np.zeros(capacity, orbfe.WP_DTYPE), np.zeros((capacity, 32), np.uint8)
    stored = pts.copy()
    skipped = stored["skip"] != 0
    stored["skip"] = 0
    inside = ids < capacity
    points[np.where(ids < 0, ~ids, ids)[inside]], desc[np.where(ids < 0, ~ids, ids)[inside]] = stored[inside], mpd[inside]
    ids = np.where(skipped & (ids >= 0) & inside, ~ids, ids).astype(np.int32)
    fr.update(kp=kp, kp_desc=kdesc, n=len(kp), ids=ids, M=M)
    prior = TS.prior_of(fr, 0) if which == R22.FROM_FRAME else None
    want = host_chain(ex, fr, which, capacity, points, desc, prior)
    assert want["n_matches"] > 50 and want["matches_inliers"] >= 8 and want["tracked"] == 1

    mp = orbfe.MapPoints(ex, capacity)
    mp.update(np.arange(capacity), points, desc)
    sc = fr["sc"]
    kf = _rec(orbfe, sc["kf"])
    frame = orbfe.ImuPreint()
    got = orbfe.track_frame_inertial(ex, params_of(sc, which), img, fr["samples"], sc["t_prev"], sc["t_cur"], sc["frame_bias"],
                                     TS.start_state(fr, which), kf, frame, mp, ids, orbfe.PoseImuPrior(prior) if prior else None)
    mp.close()
    assert got["kp"].tobytes() == kp.tobytes() and got["desc"].tobytes() == kdesc.tobytes()
    got.update(n_matches=got["nmatches"], kf=bytes(kf), frame=bytes(frame), steps=got["steps"].tobytes())
    same(got, want, "track_frame_inertial, " + wname)
    assert bytes(got["link"]) == want["link"], "the link"

#!/usr/bin/env python3
"""Latency of the S23 calls (Tracking::TrackLocalMap with the IMU, batched and resident) next to what a caller has to do without
them, on ONE box:
  * orbfe_track_inertial_batch_device at 512 frames (32 distinct scenes of tests/track_inertial_scenarios.py, repeated): 1000
    keypoints, 2000 id slots and a window of 10 IMU steps a frame, either link kind.  Against it, the SAME stages through the entry
    points that existed before it, with the host hops they need: orbfe_imu_frame_batch_device -> D2H of the predicted states and a
    synchronisation -> the frusta on the host (numpy, all frames at once) -> orbfe_project_map_points_device, the frustum by value,
    one launch a frame, on point rows and descriptors the caller keeps gathered per frame in HBM -> orbfe_match_projection_batch_device
    -> the depths out of the records (one strided device copy) -> the S19 / S20 batch call -> D2H of matches, flags and states, a
    synchronisation, the statistics and the pose on the host (numpy, all frames at once).  The host time of the 512 projection
    enqueues (this tool calls through ctypes) is reported on its own.
    Both sides are timed on the host clock from the first enqueue to the end of the last synchronisation; the new call also with
    stream events around its launches.  `reps` timed runs after a warm-up, three alternations of the two sides, the middle median.
    Before timing, frame 0 and frame 511 of both sides are compared: states, matches, flags, counts must agree byte for byte.
  * orbfe_track_frame_inertial (one frame from host memory: a synthetic 752 x 480 image, about 1000 keypoints, 2000 id slots, 10
    steps) against the sum of the single calls it replaces on the same data: orbfe_imu_preintegrate_frame, orbfe_imu_predict,
    orbfe_track_frame_map, orbfe_pose_inertial_optimization_last_keyframe / _last_frame.
There is no acceptance ratio: the figures are reported.

usage: python3 tests/tools/track_inertial_latency.py [--reps 30] [--json profiles/r23_track_inertial_latency.json] [--git-head HEAD]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
import numpy as np  # noqa: E402

import imu_preint_ref as R22  # noqa: E402
import track_inertial_ref as T  # noqa: E402
import track_inertial_scenarios as TS  # noqa: E402
from mlpnp_scenarios import H, PINHOLE, W  # noqa: E402

NAME = {R22.FROM_KEYFRAME: "ORBFE_IMU_FROM_KEYFRAME", R22.FROM_FRAME: "ORBFE_IMU_FROM_FRAME"}
LINK_SIZE = {R22.FROM_KEYFRAME: 216 + 99 * 8, R22.FROM_FRAME: 424 + 99 * 8}
ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
f32 = np.float32


def params_of(orbfe, sc, which):
    tp = orbfe.TrackParams()
    tp.grid_cols, tp.grid_rows, tp.min_x, tp.min_y = TS.GRID[0], TS.GRID[1], 0.0, 0.0
    tp.grid_inv_w, tp.grid_inv_h = float(f32(TS.GRID[0]) / f32(W)), float(f32(TS.GRID[1]) / f32(H))
    tp.th, tp.nn_ratio, tp.far_points, tp.th_far_points = TS.TH, TS.NN_RATIO, 0, 0.0
    cam = np.array(PINHOLE, f32)
    return orbfe.TrackInertialParams(track=tp, noise=orbfe.ImuNoise(sc["noise"].cov, sc["noise"].walk),
                                     predict=orbfe.ImuPredictParams(which, sc["gravity"], sc["Rcb"], sc["tcb"], sc["tbc"]),
                                     frustum=TS.frustum_template(orbfe.Frustum()), pose_keyframe=orbfe.PoseInertialParams(cam),
                                     pose_frame=orbfe.PoseInertialPrevParams(cam))


def middle(xs):
    return float(sorted(xs)[len(xs) // 2])


def batch_rows(reps, B=512, N=1000, M=2000, steps=10, distinct=32):
    import torch
    import orbfe
    stride = 1024
    ex = orbfe.ORBextractor(*ARGS)
    base = [TS.make_frame("ordinary", M, s, s * M, distinct * M, orbfe.WP_DTYPE, orbfe.KP_DTYPE, n_kp=N, case=("moving", steps, s))
            for s in range(distinct)]
    frames = [base[b % distinct] for b in range(B)]
    capacity = distinct * M
    points, desc = np.concatenate([f["points"] for f in base]), np.concatenate([f["desc"] for f in base])
    mp = orbfe.MapPoints(ex, capacity)
    mp.update(np.arange(capacity), points, desc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    full = lambda n, dt, v=0: torch.full((n,), v, dtype=dt, device="cuda")  # noqa: E731
    off = np.cumsum([0] + [len(f["samples"]) for f in frames]).astype(np.int32)
    kp, kd = np.zeros((B, stride), orbfe.KP_DTYPE), np.zeros((B, stride, 32), np.uint8)
    recs = np.zeros((B, 1200), np.uint8)
    for b, f in enumerate(frames):
        kp[b, :N], kd[b, :N] = f["kp"], f["kp_desc"]
        recs[b] = np.frombuffer(bytes(orbfe.ImuPreint(f["sc"]["kf"].floats(), f["sc"]["kf"].n_steps)), np.uint8)
    ids = np.stack([f["ids"] for f in frames]).astype(np.int32)
    d = dict(smp=dev(np.concatenate([f["samples"] for f in frames])), tp=dev(np.array([f["sc"]["t_prev"] for f in frames])),
             tc=dev(np.array([f["sc"]["t_cur"] for f in frames])), fb=dev(np.stack([f["sc"]["frame_bias"] for f in frames]).astype(f32)),
             kf0=dev(recs), kp=dev(kp), desc=dev(kd), n=dev(np.full(B, N, np.int32)), ids=dev(ids))
    d["kf"] = d["kf0"].clone()
    # what a caller of the earlier entry points keeps per frame in HBM: the id-resolved point rows (skip set per frame) and descriptors
    seen = np.zeros((B, M), orbfe.WP_DTYPE)
    mpd = np.zeros((B, M, 32), np.uint8)
    for s, f in enumerate(base):
        a, dd, _rows = T.resolve_ids(f["ids"], capacity, points, desc)
        seen[s::distinct], mpd[s::distinct] = a, dd
    d["seen"], d["mpd"] = dev(seen), dev(mpd)
    obs_host = seen["observations"].copy()
    st = torch.cuda.Stream()
    sc0 = frames[0]["sc"]
    Rcb, tcb = sc0["Rcb"].astype(f32), sc0["tcb"].astype(f32)
    rows = []
    for which in (R22.FROM_KEYFRAME, R22.FROM_FRAME):
        ff = which == R22.FROM_FRAME
        par = params_of(orbfe, sc0, which)
        hd = 900 if ff else 225
        d["s1"] = dev(np.stack([TS.start_state(f, which) for f in frames]).astype(f32))
        pri = dev(np.frombuffer(b"".join(bytes(orbfe.PoseImuPrior(TS.prior_of(f, b % distinct))) for b, f in enumerate(frames)), np.uint8)) if ff else None
        o = {}
        for side in ("new", "old"):
            o[side] = dict(fr=full(B * 1200, torch.uint8), state_in=full(B * 33, torch.float32), ok=full(B, torch.int32),
                           mps=full(B * M * 32, torch.uint8), match=full(B * stride, torch.int32, -1), nm=full(B, torch.int32),
                           state_out=full(B * 21, torch.float32), Hm=full(B * hd, torch.float64), outl=full(B * stride, torch.uint8),
                           ninl=full(B, torch.int32), acc=full(B, torch.int32, 1), found=full(B * M, torch.uint8), mi=full(B, torch.int32),
                           tracked=full(B, torch.int32), Tcw=full(B * 12, torch.float32))
        old_links = full(B * LINK_SIZE[which], torch.uint8)
        n_ = o["new"]
        io, keep = orbfe.track_inertial_io(
            off, d_samples=d["smp"].data_ptr(), d_t_prev=d["tp"].data_ptr(), d_t_cur=d["tc"].data_ptr(), d_frame_bias=d["fb"].data_ptr(),
            d_state1=d["s1"].data_ptr(), d_kf=d["kf"].data_ptr(), d_frame=n_["fr"].data_ptr(), d_kp=d["kp"].data_ptr(),
            d_desc=d["desc"].data_ptr(), d_n=d["n"].data_ptr(), d_ids=d["ids"].data_ptr(), d_priors=pri.data_ptr() if ff else None,
            d_state_in=n_["state_in"].data_ptr(), d_info_ok=n_["ok"].data_ptr(), d_mp_out=n_["mps"].data_ptr(),
            d_match_out=n_["match"].data_ptr(), d_n_matches=n_["nm"].data_ptr(), d_state_out=n_["state_out"].data_ptr(),
            d_H_out=n_["Hm"].data_ptr(), d_outlier=n_["outl"].data_ptr(), d_n_inliers=n_["ninl"].data_ptr(), d_accepted=n_["acc"].data_ptr(),
            d_found=n_["found"].data_ptr(), d_matches_inliers=n_["mi"].data_ptr(), d_tracked=n_["tracked"].data_ptr(),
            d_Tcw_out=n_["Tcw"].data_ptr())

        def new_call():
            orbfe.track_inertial_batch_device(ex, par, B, stride, mp, M, io, st.cuda_stream)

        matcher = orbfe.ORBmatcher(ex)
        F = TS.frustum_template(orbfe.Frustum())
        host, loop_ms = {}, []

        def old_chain():
            q = o["old"]
            orbfe.imu_frame_batch_device(ex, par.noise, par.predict, B, d["smp"].data_ptr(), off, d["tp"].data_ptr(), d["tc"].data_ptr(),
                                         d["fb"].data_ptr(), d["s1"].data_ptr(), d["kf"].data_ptr(), q["fr"].data_ptr(), None,
                                         q["state_in"].data_ptr(), old_links.data_ptr(), q["ok"].data_ptr(), st.cuda_stream)
            with torch.cuda.stream(st):
                s_in = q["state_in"].cpu().numpy().reshape(B, 33)                  # hop 1: the predicted states come down
            R, t = s_in[:, 0:9].reshape(B, 3, 3), s_in[:, 9:12]
            twc = -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])
            t_loop = time.perf_counter()
            for b in range(B):                                                     # the frusta go up by value, one launch a frame
                F.rcw[:], F.tcw[:], F.twc[:] = s_in[b, 0:9].tolist(), t[b].tolist(), twc[b].tolist()
                matcher.isInFrustum_batch_device(F, M, d["seen"].data_ptr() + b * M * 32, q["mps"].data_ptr() + b * M * 32, None, st.cuda_stream)
            loop_ms.append((time.perf_counter() - t_loop) * 1e3)                   # host time of the B enqueues (through ctypes)
            matcher.SearchByProjection_batch_device(B, d["kp"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(), stride, TS.GRID[0], TS.GRID[1],
                                                    0.0, 0.0, float(W), float(H), M, q["mps"].data_ptr(), d["mpd"].data_ptr(), None, TS.TH,
                                                    TS.NN_RATIO, q["match"].data_ptr(), q["nm"].data_ptr(), stream=st.cuda_stream)
            with torch.cuda.stream(st):
                depth = q["mps"].view(torch.float32).view(B * M, 8)[:, 3].contiguous()   # the depths out of the records
            if ff:
                orbfe.pose_inertial_optimization_last_frame_batch_device(
                    ex, par.pose_frame, B, old_links.data_ptr(), pri.data_ptr(), d["kp"].data_ptr(), d["n"].data_ptr(), stride,
                    q["match"].data_ptr(), M, d["seen"].data_ptr(), M, depth.data_ptr(), q["state_in"].data_ptr(), q["state_out"].data_ptr(),
                    q["Hm"].data_ptr(), None, q["outl"].data_ptr(), q["ninl"].data_ptr(), q["acc"].data_ptr(), st.cuda_stream)
            else:
                orbfe.pose_inertial_optimization_batch_device(
                    ex, par.pose_keyframe, B, old_links.data_ptr(), d["kp"].data_ptr(), d["n"].data_ptr(), stride, q["match"].data_ptr(), M,
                    d["seen"].data_ptr(), M, depth.data_ptr(), q["state_in"].data_ptr(), q["state_out"].data_ptr(), q["Hm"].data_ptr(),
                    q["outl"].data_ptr(), q["ninl"].data_ptr(), st.cuda_stream)
            with torch.cuda.stream(st):                                            # hop 2: what the statistics read comes down
                match = q["match"].cpu().numpy().reshape(B, stride)[:, :N]
                outl = q["outl"].cpu().numpy().reshape(B, stride)[:, :N]
                s_out = q["state_out"].cpu().numpy().reshape(B, 21)
                acc = q["acc"].cpu().numpy()
            st.synchronize()
            found = np.zeros((B, M), np.uint8)
            bb, ii = np.nonzero(match >= 0)
            mm = match[bb, ii]
            inl = outl[bb, ii] == 0
            found[bb[inl], mm[inl]] = 1
            mi = np.bincount(bb[inl & (obs_host[bb, mm] > 0)], minlength=B)
            Rwb, twb = s_out[:, 0:9].reshape(B, 3, 3), s_out[:, 9:12]
            Rcw = np.einsum("ij,bkj->bik", Rcb, Rwb)
            tcw = -np.einsum("bij,bj->bi", Rcw, twb) + tcb
            host.update(found=found, mi=mi, tracked=mi >= 8, Tcw=np.concatenate([Rcw.reshape(B, 9), tcw], 1), match=match, outl=outl,
                        state_out=s_out, state_in=s_in, acc=acc)

        # ---- both sides once, compared ----
        new_call()
        st.synchronize()
        d["kf"].copy_(d["kf0"])
        old_chain()
        d["kf"].copy_(d["kf0"])
        g = {k: v.cpu().numpy() for k, v in n_.items()}
        for b in (0, B - 1):
            assert g["state_in"].reshape(B, 33)[b].tobytes() == host["state_in"][b].tobytes()
            assert g["match"].reshape(B, stride)[b, :N].tobytes() == host["match"][b].tobytes()
            assert g["outl"].reshape(B, stride)[b, :N].tobytes() == host["outl"][b].tobytes()
            assert g["state_out"].reshape(B, 21)[b].tobytes() == host["state_out"][b].tobytes()
            assert g["found"].reshape(B, M)[b].tobytes() == host["found"][b].tobytes() and int(g["mi"][b]) == int(host["mi"][b])
        inl_mean = float(g["mi"].mean())

        def timed(fn, events=False):
            ts, ev = [], []
            for _ in range(reps):
                d["kf"].copy_(d["kf0"])        # the records are integrated in place: every run starts from the same ones
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                if events:
                    a.record(st)
                fn()
                if events:
                    b.record(st)
                st.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                if events:
                    ev.append(a.elapsed_time(b))
            return float(np.median(ts)), (float(np.median(ev)) if events else None)
        for fn in (new_call, old_chain):
            for _ in range(3):
                d["kf"].copy_(d["kf0"])
                fn()
                st.synchronize()
        new_w, new_e, old_w = [], [], []
        for _ in range(3):
            w_, e_ = timed(new_call, True)
            new_w.append(w_)
            new_e.append(e_)
            old_w.append(timed(old_chain)[0])
        row = dict(entry="orbfe_track_inertial_batch_device", which=NAME[which], size="%d frames x %d keypoints x %d ids x %d steps" % (B, N, M, steps),
                   new_wall_ms=middle(new_w), new_events_ms=middle(new_e), staged_wall_ms=middle(old_w), staged_over_new=middle(old_w) / middle(new_w),
                   new_wall_runs_ms=new_w, new_events_runs_ms=new_e, staged_wall_runs_ms=old_w, mean_matches_inliers=inl_mean,
                   staged_projection_enqueue_loop_ms=float(np.median(loop_ms[-3 * reps:])))
        rows.append(row)
        print("batch %-24s new %8.2f ms (events %8.2f)   staged with host hops %8.2f ms (of which the %d projection enqueues %.2f ms)   x%.3f   "
              "runs new %s staged %s" % (NAME[which], row["new_wall_ms"], row["new_events_ms"], row["staged_wall_ms"], B,
                                         row["staged_projection_enqueue_loop_ms"], row["staged_over_new"], ["%.2f" % x for x in new_w],
                                         ["%.2f" % x for x in old_w]), flush=True)
        del keep
    mp.close()
    ex.close()
    return rows


def single_rows(reps, M=2000, steps=10):
    import orbfe
    import frustum_scenarios as FS
    from orbfe import synth
    ex = orbfe.ORBextractor(*ARGS)
    img = synth.frame(W, H, 3)
    kp, kdesc = ex.extractFeatures(img)
    fr = TS.make_frame("ordinary", 0, 0, 0, 1, orbfe.WP_DTYPE, orbfe.KP_DTYPE, case=("moving", steps, 0))
    sc = fr["sc"]
    tracker = orbfe.FrameTracker(ex, TS.GRID[0], TS.GRID[1], 0.0, 0.0, float(W), float(H))
    rows = []
    for which in (R22.FROM_KEYFRAME, R22.FROM_FRAME):
        ff = which == R22.FROM_FRAME
        par = params_of(orbfe, sc, which)
        s1 = TS.start_state(fr, which)
        prior = orbfe.PoseImuPrior(TS.prior_of(fr, 0)) if ff else None

        def imu():
            kf = orbfe.ImuPreint(sc["kf"].floats(), sc["kf"].n_steps)
            frame, _steps, _n = orbfe.imu_preintegrate_frame(ex, par.noise, fr["samples"], sc["t_prev"], sc["t_cur"], sc["frame_bias"], kf)
            return orbfe.imu_predict(ex, par.predict, s1, kf, frame)
        state_in, link, _ok = imu()
        rcw, tcw, twc = T.frustum_pose(state_in)
        v = dict(rcw=rcw, tcw=tcw, twc=twc, fx=PINHOLE[0], fy=PINHOLE[1], cx=PINHOLE[2], cy=PINHOLE[3])
        pts, mpd = FS.world_points_on_keypoints(kp, kdesc, v, M, np.random.default_rng(23), ex.nlevels, orbfe.WP_DTYPE)
        pts["skip"] = 0
        mp = orbfe.MapPoints(ex, M)
        mp.update(np.arange(M), pts, mpd)
        ids = np.arange(M, dtype=np.int32)
        xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(f32)
        F = TS.set_frustum_pose(TS.frustum_template(orbfe.Frustum()), state_in)
        cam = np.array(PINHOLE, f32)

        def track():
            return tracker.TrackFrameMap(img, F, mp, ids, TS.TH, TS.NN_RATIO)
        tr = track()

        def pose():
            tail = (state_in[0:9], state_in[9:12], state_in[12:21], state_in[21:24], state_in[24:27], state_in[27:30], state_in[30:33])
            dep = np.ascontiguousarray(tr["mps"]["track_depth"])
            if ff:
                return orbfe.pose_inertial_optimization_last_frame(ex, par.pose_frame, link, prior, tr["kp"], tr["match"], xyz, dep, *tail,
                                                                   want_info=False)
            return orbfe.pose_inertial_optimization_last_keyframe(ex, par.pose_keyframe, link, tr["kp"], tr["match"], xyz, dep, *tail, want_info=False)
        po = pose()

        def new():
            kf = orbfe.ImuPreint(sc["kf"].floats(), sc["kf"].n_steps)
            return orbfe.track_frame_inertial(ex, par, img, fr["samples"], sc["t_prev"], sc["t_cur"], sc["frame_bias"], s1, kf, orbfe.ImuPreint(),
                                              mp, ids, prior)
        g = new()
        assert g["match"].tobytes() == tr["match"].tobytes() and g["state_in"].tobytes() == state_in.tobytes()
        assert g["state_out"].tobytes() == np.concatenate([po[k] for k in ("Rwb", "twb", "v", "bg", "ba")]).tobytes()
        assert g["n_inliers"] == po["n_inliers"]

        def med(fn):
            for _ in range(5):
                fn()
            out = []
            for _ in range(3):
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e6)
                out.append(float(np.median(ts)))
            return out
        parts = dict(imu=med(imu), track_frame_map=med(track), pose=med(pose))
        new_runs = med(new)
        total = sum(middle(x) for x in parts.values())
        rows.append(dict(entry="orbfe_track_frame_inertial", which=NAME[which], size="%d keypoints x %d ids x %d steps" % (len(kp), M, steps),
                         new_us=middle(new_runs), single_calls_us={k: middle(x) for k, x in parts.items()}, single_calls_sum_us=total,
                         sum_over_new=total / middle(new_runs), new_runs_us=new_runs, single_calls_runs_us=parts, matches=int(g["nmatches"]),
                         matches_inliers=int(g["matches_inliers"])))
        print("single %-24s new %8.1f us   single calls %s = %8.1f us   x%.3f   runs new %s" % (
            NAME[which], middle(new_runs), {k: round(middle(x), 1) for k, x in parts.items()}, total, total / middle(new_runs),
            ["%.1f" % x for x in new_runs]), flush=True)
        mp.close()
    ex.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--git-head", default=None, help="recorded in _meta when the tree is not a git checkout")
    a = ap.parse_args()
    rows = batch_rows(a.reps) + single_rows(a.reps)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/track_inertial_latency.py"), host_cpus=os.cpu_count(),
                           reps=a.reps, rows=rows), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

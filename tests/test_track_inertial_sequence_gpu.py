"""The inertial TrackLocalMap chain (SPEC DECISION S23) over CONSECUTIVE frames on the GPU: six frames a sequence, the key-frame
record integrated in place from call to call, the start state and the prior carried by the rules of track_inertial_sequence.  Every
comparison is byte for byte (the same() of tests/test_track_inertial_gpu.py, records, steps and link included); the oracles are
run_sequence(CpuStages) -- the restatements and the C oracle -- and run_sequence(HostStages) -- the separate host-pointer calls.

  * orbfe_track_frame_inertial in a loop: the image form of nominal, weak_imu and events, the prior handed on raw and clamped; the
    ImuPreint objects are carried in place.  The extraction's keypoints must equal the C oracle's first.
  * orbfe_track_inertial_batch_device in lock step: B = 3 sequences in the planted-keypoint form, K = 6 calls on one stream.  d_kf and
    d_frame stay in HBM between the calls and are never re-uploaded (they are copied out for the comparison only); on a last-frame
    step d_state1 of call k + 1 IS d_state_out of call k, and d_frame_bias is a device-side copy of its bias columns.  The priors make
    the one declared host hop: H / Hprior and state_out come down, orbfe_pose_imu_prior blocks go up (the API has no device form of
    that).  The call has ONE noise block, so the sequences of a batch share their noise: the test runs once with three seeds of
    nominal and once with three seeds of weak_imu.  That every frame is accepted -- the state hand-over by pointer assumes it -- is
    asserted on the restatement before the GPU is touched."""
import numpy as np
import pytest

import track_inertial_scenarios as TS
import track_inertial_sequence as Q
from test_track_inertial_gpu import ARGS, KP_STRIDE, REC_BYTES, HostStages, _dev, _rec, params_of, same

pytestmark = pytest.mark.gpu
f32 = np.float32
KF, F = Q.KF, Q.F


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    assert tuple(ARGS) == tuple(Q.EXTRACTOR_ARGS)
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


def record_bytes(orbfe, rec):
    rec = Q.as_record(rec)
    return bytes(_rec(orbfe, rec)) if rec is not None else bytes(orbfe.ImuPreint())


def as_want(orbfe, o):
    """a frame of run_sequence in the shape same() reads: the records and the steps as bytes"""
    return dict(o, kf=record_bytes(orbfe, o["kf_rec"]), frame=record_bytes(orbfe, o["frame_rec"]),
                steps=o["steps"] if isinstance(o["steps"], bytes) else np.asarray(o["steps"], f32).tobytes())


@pytest.mark.parametrize("mode", ("raw", "clamped"))
@pytest.mark.parametrize("name", ("nominal", "weak_imu", "events"))
def test_track_frame_inertial_in_a_loop(ex, name, mode):
    import orbfe
    seq = Q.make_sequence(name, form="image")
    restated = Q.cpu_run(name, mode, 0, "image")
    assert [o["which"] for o in restated] == Q.BRANCHES[name]
    for o in restated:
        assert o["info_ok"] == 1 and o["pose"]["ref"]["round_ok"].all() and np.isfinite(o["state_out"]).all() and np.isfinite(o["H"]).all()
    hosted = [as_want(orbfe, o) for o in Q.run_sequence(HostStages(ex), seq, mode)]
    mp = orbfe.MapPoints(ex, seq["capacity"])
    mp.update(np.arange(seq["capacity"]), seq["points"], seq["desc"])
    car = Q.start_of(seq)
    kf, frame = _rec(orbfe, car["kf_rec"]), orbfe.ImuPreint()
    try:
        for k in range(seq["K"]):
            fr, which, prior = Q.frame_inputs(seq, k, car)
            sc = fr["sc"]
            if k in seq["fresh"]:      # ImuPreintegrator::Fresh: Reintegrate of no step at the last frame's bias
                kf = orbfe.imu_reintegrate(ex, params_of(sc, which).noise, car["last_state"][15:21], np.zeros(0, orbfe.IMU_STEP_DTYPE))
                assert bytes(kf) == record_bytes(orbfe, car["kf_rec"])
            got = orbfe.track_frame_inertial(ex, params_of(sc, which), fr["image"], fr["samples"], sc["t_prev"], sc["t_cur"], sc["frame_bias"],
                                             TS.start_state(fr, which), kf, frame, mp, fr["ids"], orbfe.PoseImuPrior(prior) if prior else None)
            what = "%s, %s prior, frame %d" % (name, mode, k)
            assert got["kp"].tobytes() == fr["kp"].tobytes() and got["desc"].tobytes() == fr["kp_desc"].tobytes(), what + ": extraction against the oracle"
            got.update(n_matches=got["nmatches"], kf=bytes(kf), frame=bytes(frame), steps=got["steps"].tobytes(), which=which)
            print(what, "KF" if which == KF else "F ", "matches", got["n_matches"], "inliers", got["n_inliers"], "accepted", got["accepted"], "tracked", got["tracked"])
            assert which == hosted[k]["which"] == restated[k]["which"], what
            same(got, hosted[k], what + " against the host-pointer calls")
            assert bytes(got["link"]) == hosted[k]["link_bytes"], what + ": the link"
            same(got, as_want(orbfe, restated[k]), what + " against the restatements")
            assert np.isfinite(got["state_out"]).all() and np.isfinite(got["H"]).all() and got["info_ok"] == 1
            got.update(kf_rec=bytes(kf), frame_rec=bytes(frame))
            Q.carry_on(car, which, got, mode)
    finally:
        mp.close()


def remap_ids(ids, cap_seq, off, cap_all):
    """a sequence's ids into the one map of the batch: its entries start at `off`; an id outside its own map stays outside"""
    ids = np.asarray(ids, np.int32)
    k = np.where(ids < 0, ~ids, ids).astype(np.int64)
    k = np.where(k >= cap_seq, cap_all + 5, k + off)
    return np.where(ids < 0, ~k, k).astype(np.int32)


@pytest.mark.parametrize("name", ("nominal", "weak_imu"))
def test_batch_device_in_lock_step(ex, name):
    import torch
    import orbfe
    seeds = (0, 1, 2)
    B, K, M = len(seeds), 6, Q.M_SLOTS
    seqs = [Q.make_sequence(name, K, s) for s in seeds]
    branches = Q.BRANCHES[name]
    # no GPU yet: every frame of every sequence is accepted on the restatement, so the last frame's state is state_out throughout
    for s in seeds:
        r = Q.cpu_run(name, "raw", s)
        assert [o["which"] for o in r] == branches == [KF, F, F, F, KF, F] and all(o["accepted"] == 1 and o["info_ok"] == 1 for o in r)
    want = [[as_want(orbfe, o) for o in Q.run_sequence(HostStages(ex), q, "raw")] for q in seqs]
    restated = [[as_want(orbfe, o) for o in Q.cpu_run(name, "raw", s)] for s in seeds]

    cap_seq = seqs[0]["capacity"]
    cap_all = B * cap_seq
    mp = orbfe.MapPoints(ex, cap_all)
    mp.update(np.arange(cap_all), np.concatenate([q["points"] for q in seqs]), np.concatenate([q["desc"] for q in seqs]))
    car0 = [Q.start_of(q) for q in seqs]
    # resident for the whole run
    d_kf = _dev(torch, np.stack([np.frombuffer(record_bytes(orbfe, c["kf_rec"]), np.uint8) for c in car0]))
    d_frame = _dev(torch, np.full((B, REC_BYTES), 0xCD, np.uint8))
    d_state_kf = _dev(torch, np.stack([c["kf_state"] for c in car0]).astype(f32)).view(torch.float32)
    d_state_last = _dev(torch, np.stack([c["last_state"] for c in car0]).astype(f32)).view(torch.float32)
    kf_ptr, frame_ptr = d_kf.data_ptr(), d_frame.data_ptr()
    # per call, uploaded up front
    calls = []
    for k in range(K):
        frs = [q["frames"][k] for q in seqs]
        smp = np.concatenate([f["samples"] for f in frs])
        off = np.cumsum([0] + [len(f["samples"]) for f in frs]).astype(np.int32)
        kp = np.zeros((B, KP_STRIDE), orbfe.KP_DTYPE)
        kd = np.zeros((B, KP_STRIDE, 32), np.uint8)
        for b, f in enumerate(frs):
            assert f["n"] <= KP_STRIDE and f["M"] == M
            kp[b, :f["n"]], kd[b, :f["n"]] = f["kp"], f["kp_desc"]
        ins = dict(d_samples=smp, d_t_prev=np.array([f["sc"]["t_prev"] for f in frs], np.float64),
                   d_t_cur=np.array([f["sc"]["t_cur"] for f in frs], np.float64), d_kp=kp, d_desc=kd, d_n=np.array([f["n"] for f in frs], np.int32),
                   d_ids=np.stack([remap_ids(f["ids"], cap_seq, b * cap_seq, cap_all) for b, f in enumerate(frs)]))
        calls.append(dict(off=off, frs=frs, dev={key: _dev(torch, v) for key, v in ins.items()}))
    torch.cuda.synchronize()

    st = torch.cuda.Stream()
    keep_alive = []
    try:
        with torch.cuda.stream(st):
            d_last, priors = d_state_last, None
            for k, call in enumerate(calls):
                which = branches[k]
                from_frame = which == F
                hdoubles = 900 if from_frame else 225
                off = call["off"]
                nsteps = max(int(off[-1]), 1)
                dev = dict(call["dev"])
                dev["d_state1"] = d_last if from_frame else d_state_kf            # on F steps: the pointer d_state_out of the call before
                dev["d_frame_bias"] = d_last.view(B, 21)[:, 15:21].contiguous()     # the last frame's bias, copied on the device
                if from_frame:
                    dev["d_priors"] = _dev(torch, np.frombuffer(b"".join(bytes(orbfe.PoseImuPrior(p)) for p in priors), np.uint8))
                shapes = dict(d_steps_out=(nsteps * 32, torch.uint8, 0xAB), d_state_in=(B * 33, torch.float32, -7.0), d_info_ok=(B, torch.int32, -3),
                              d_mp_out=(B * M * 32, torch.uint8, 0xAB), d_match_out=(B * KP_STRIDE, torch.int32, -77),
                              d_n_matches=(B, torch.int32, -3), d_state_out=(B * 21, torch.float32, -7.0), d_H_out=(B * hdoubles, torch.float64, -7.0),
                              d_Hprior_out=(B * 225, torch.float64, -7.0), d_outlier=(B * KP_STRIDE, torch.uint8, 0xAB),
                              d_n_inliers=(B, torch.int32, -3), d_accepted=(B, torch.int32, -3), d_found=(B * M, torch.uint8, 0xAB),
                              d_matches_inliers=(B, torch.int32, -3), d_tracked=(B, torch.int32, -3), d_Tcw_out=(B * 12, torch.float32, -7.0))
                for key, (n, dt, fill) in shapes.items():
                    dev[key] = torch.full((n,), fill, dtype=dt, device="cuda")
                ptrs = {key: v.data_ptr() for key, v in dev.items()}
                ptrs["d_kf"], ptrs["d_frame"] = kf_ptr, frame_ptr                  # the same HBM from the first call to the last
                if not from_frame:
                    ptrs["d_Hprior_out"] = None
                io, keep = orbfe.track_inertial_io(off, **ptrs)
                orbfe.track_inertial_batch_device(ex, params_of(call["frs"][0]["sc"], which), B, KP_STRIDE, mp, M, io, st.cuda_stream)
                st.synchronize()
                keep_alive.append((dev, keep))
                assert d_kf.data_ptr() == kf_ptr and d_frame.data_ptr() == frame_ptr
                host = {key: v.cpu().numpy() for key, v in dev.items() if key in shapes}
                host["d_kf"], host["d_frame"] = d_kf.cpu().numpy(), d_frame.cpu().numpy()      # copies for the comparison; nothing goes back up
                priors = []
                for b in range(B):
                    n = call["frs"][b]["n"]
                    nst = max(len(call["frs"][b]["samples"]) - 1, 0)
                    lo = int(off[b]) * 32
                    assert (host["d_steps_out"][lo + 32 * nst:int(off[b + 1]) * 32] == 0xAB).all(), "bytes beyond the frame's steps written"
                    assert (host["d_outlier"].reshape(B, KP_STRIDE)[b, n:] == 0xAB).all(), "outlier flags beyond d_n written"
                    got = dict(
                        state_in=host["d_state_in"].reshape(B, 33)[b], info_ok=int(host["d_info_ok"][b]),
                        kf=host["d_kf"].reshape(B, REC_BYTES)[b].tobytes(), frame=host["d_frame"].reshape(B, REC_BYTES)[b].tobytes(),
                        steps=host["d_steps_out"][lo:lo + 32 * nst].tobytes(), mps=host["d_mp_out"].view(orbfe.MP_DTYPE).reshape(B, M)[b],
                        match=host["d_match_out"].reshape(B, KP_STRIDE)[b, :n], n_matches=int(host["d_n_matches"][b]),
                        state_out=host["d_state_out"].reshape(B, 21)[b], H=host["d_H_out"].reshape(B, hdoubles)[b],
                        Hprior=host["d_Hprior_out"].reshape(B, 225)[b] if from_frame else None, outlier=host["d_outlier"].reshape(B, KP_STRIDE)[b, :n],
                        n_inliers=int(host["d_n_inliers"][b]), accepted=int(host["d_accepted"][b]), found=host["d_found"].reshape(B, M)[b],
                        matches_inliers=int(host["d_matches_inliers"][b]), tracked=int(host["d_tracked"][b]), Tcw=host["d_Tcw_out"].reshape(B, 12)[b])
                    what = "%s seed %d, call %d (%s)" % (name, seeds[b], k, "F" if from_frame else "KF")
                    same(got, want[b][k], what + " against the host-pointer loop")
                    same(got, restated[b][k], what + " against the restatements")
                    assert got["accepted"] == 1
                    priors.append(Q.prior_from(got, which, "raw"))                  # the one host hop
                if not from_frame:
                    assert (host["d_Hprior_out"] == -7.0).all()
                d_last = dev["d_state_out"]
    finally:
        torch.cuda.synchronize()
        mp.close()

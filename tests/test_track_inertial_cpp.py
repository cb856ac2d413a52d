"""tests/cpp/track_inertial.cpp: include/orbfe_adaptor.hpp's InertialFrameTracker -- the class that owns the two preintegration records
and the prior between frames and decides which optimisation runs -- over the `events` sequence of track_inertial_sequence in its image
form: frame 2 with one IMU sample, frame 3 without a keypoint (its last-frame result is rejected), mbMapUpdated and a new key frame at
frame 5.  The program derives the start state and lastFrameBias from the previous Result as INTEGRATION.md tells a caller to and
passes the prior on raw; every field of every Result, FromLastKF(), FromLastFrame(), HasPrior() and Prior() after each frame must
equal run_sequence(CpuStages, events, "raw"), byte for byte.

Before the fix of this header Track never cleared its prior flag on a rejected result: HasPrior() stayed 1 after frame 3 (where this
comparison stops first: "frame 3: has_prior 1 != 0") and frame 4 ran against the last frame, with the prior of frame 2 on the state
of frame 3, instead of against the last key frame.  The build-only test runs without a GPU, so the adaptor class is compiled on
every CPU run."""
import subprocess

import numpy as np
import pytest

import cpp_build
import track_inertial_sequence as Q

HEAD = ("kind", "n", "n_steps", "n_matches", "n_inliers", "matches_inliers", "accepted", "tracked", "info_ok", "has_prior")
REC_BYTES = 1200
f32 = np.float32


def _build():
    return cpp_build.build("track_inertial")


def test_track_inertial_program_builds_and_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def write_scene(path, seq, params):
    import orbfe
    a = Q.EXTRACTOR_ARGS
    with open(path, "wb") as f:
        f.write(np.array([a[0], a[1], a[3], a[4], a[5], a[6], a[7]], np.int32).tobytes() + np.array([a[2]], f32).tobytes())
        f.write(np.array([seq["K"], seq["M"], seq["capacity"], len(bytes(params))], np.int32).tobytes() + bytes(params))
        f.write(np.asarray(seq["state_kf0"], f32).tobytes() + np.asarray(seq["state0"], f32).tobytes())
        f.write(bytes(orbfe.ImuPreint(seq["kf0"].floats(), seq["kf0"].n_steps)))
        f.write(np.ascontiguousarray(seq["points"], orbfe.WP_DTYPE).tobytes() + np.ascontiguousarray(seq["desc"], np.uint8).tobytes())
        for k, fr in enumerate(seq["frames"]):
            smp = np.ascontiguousarray(fr["samples"], orbfe.IMU_SAMPLE_DTYPE)
            f.write(np.ascontiguousarray(fr["image"], np.uint8).tobytes() + np.array([len(smp)], np.int32).tobytes() + smp.tobytes())
            f.write(np.array([fr["sc"]["t_prev"], fr["sc"]["t_cur"]], np.float64).tobytes() + np.ascontiguousarray(fr["ids"], np.int32).tobytes())
            f.write(np.array([k in seq["map_updated"], k in seq["fresh"]], np.int32).tobytes())


def read_results(path, K, M):
    import orbfe
    b = open(path, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(b, dt, cnt, at[0])
        at[0] += a.nbytes
        return a
    out = []
    for _ in range(K):
        r = dict(zip(HEAD, (int(v) for v in take(np.int32, len(HEAD)))))
        n = r["n"]
        r["kp"], r["desc"], r["steps"] = take(orbfe.KP_DTYPE, n), take(np.uint8, 32 * n), take(orbfe.IMU_STEP_DTYPE, r["n_steps"])
        r["state_in"], r["state_out"], r["Tcw"] = take(f32, 33), take(f32, 21), take(f32, 12)
        r["mps"], r["match"], r["outlier"], r["found"] = take(orbfe.MP_DTYPE, M), take(np.int32, n), take(np.uint8, n), take(np.uint8, M)
        r["kf"], r["frame"] = take(np.uint8, REC_BYTES).tobytes(), take(np.uint8, REC_BYTES).tobytes()
        r["prior"] = take(np.uint8, orbfe.C.sizeof(orbfe.PoseImuPrior)).tobytes()
        out.append(r)
    assert at[0] == len(b)
    return out


def record_bytes(rec):
    import orbfe
    rec = Q.as_record(rec)
    return bytes(orbfe.ImuPreint(rec.floats(), rec.n_steps)) if rec is not None else bytes(orbfe.ImuPreint())


@pytest.mark.gpu
def test_adaptor_tracks_the_events_sequence_as_the_restatements_do(built, tmp_path):
    import orbfe
    from test_track_inertial_gpu import params_of
    seq = Q.make_sequence("events", form="image")
    want = Q.cpu_run("events", "raw", 0, "image")
    assert [w["which"] for w in want] == [Q.KF, Q.F, Q.F, Q.F, Q.KF, Q.KF] and [w["accepted"] for w in want] == [1, 1, 1, 0, 1, 1]
    write_scene(tmp_path / "scene.bin", seq, params_of(seq["frames"][0]["sc"], Q.KF))
    print(subprocess.check_output([_build(), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")]).decode())
    got = read_results(tmp_path / "out.bin", seq["K"], seq["M"])
    for k, (g, w) in enumerate(zip(got, want)):
        what = "frame %d" % k
        left = Q.prior_from(w, w["which"], "raw")
        exp = dict(kind=w["which"], n=seq["frames"][k]["n"], n_steps=len(w["steps"]), n_matches=w["n_matches"], n_inliers=w["n_inliers"],
                   matches_inliers=w["matches_inliers"], accepted=w["accepted"], tracked=w["tracked"], info_ok=w["info_ok"],
                   has_prior=int(left is not None))
        for key in HEAD:
            assert g[key] == exp[key], "%s: %s %d != %d" % (what, key, g[key], exp[key])
        assert g["kp"].tobytes() == seq["frames"][k]["kp"].tobytes() and g["desc"].tobytes() == seq["frames"][k]["kp_desc"].tobytes(), what
        assert g["steps"].tobytes() == np.asarray(w["steps"], f32).tobytes(), "%s: steps" % what
        for key in ("state_in", "state_out", "Tcw", "mps", "match", "outlier", "found"):
            assert g[key].tobytes() == np.ascontiguousarray(w[key]).tobytes(), "%s: %s" % (what, key)
        assert g["kf"] == record_bytes(w["kf_rec"]), "%s: FromLastKF()" % what
        assert g["frame"] == record_bytes(w["frame_rec"]), "%s: FromLastFrame()" % what
        if left is not None:
            assert g["prior"] == bytes(orbfe.PoseImuPrior(left)), "%s: Prior()" % what

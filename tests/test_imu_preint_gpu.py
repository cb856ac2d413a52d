"""The five S22 calls on the GPU against the restatement (imu_preint_ref, written from src/Tracking.cc:234-350, src/ImuTypes.cc,
src/Frame.cc:221-238, src/G2oTypes.cc:500-508) on the scenes of imu_preint_scenarios (test_imu_preint.py checks which branches they
reach).  Every comparison is exact: the bytes of both records, the steps, the 33-float state, the whole link block and info_ok.  No
tolerance and no skipped element.  The step counts are those at which a path can go wrong: 1 (the single-step branch), 2, 3, 10, and
the staging chunk of the kernel - 1, the chunk, the chunk + 1."""
import ctypes as C

import numpy as np
import pytest

import imu_preint_ref as R
import imu_preint_scenarios as PS
from test_imu_preint_cpp import link_bytes, samples_of

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
WHICH = ((R.FROM_KEYFRAME, "keyframe"), (R.FROM_FRAME, "frame"))
LINK_SIZE = {R.FROM_KEYFRAME: 216 + 99 * 8, R.FROM_FRAME: 424 + 99 * 8}


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


def blocks(sc, which, gravity=None, noise=None):
    import orbfe
    nz = noise if noise is not None else sc["noise"]
    return (orbfe.ImuNoise(nz.cov, nz.walk),
            orbfe.ImuPredictParams(which, sc["gravity"] if gravity is None else gravity, sc["Rcb"], sc["tcb"], sc["tbc"]))


def start_state(sc, which):
    return sc["state_frame"] if which == R.FROM_FRAME else sc["state_kf"]


def single(ex, sc, which, **kw):
    """the three host-pointer calls -> dict(kf, frame (floats), kf_steps, frame_steps, steps, state, link (bytes), ok, re (floats))"""
    import orbfe
    noise, par = blocks(sc, which, **kw)
    kf = orbfe.ImuPreint(sc["kf"].floats(), sc["kf"].n_steps)
    frame, steps, n = orbfe.imu_preintegrate_frame(ex, noise, samples_of(sc), sc["t_prev"], sc["t_cur"], sc["frame_bias"], kf)
    state, link, ok = orbfe.imu_predict(ex, par, start_state(sc, which), kf, frame)
    re = orbfe.imu_reintegrate(ex, noise, sc["frame_bias"], steps)
    return dict(kf=kf.floats(), frame=frame.floats(), kf_steps=kf.n_steps, frame_steps=frame.n_steps, n=n, steps=steps.tobytes(), state=state,
                link=bytes(link), ok=ok, re=re.floats(), re_steps=re.n_steps)


def same_as_ref(got, want, what, which):
    assert got["n"] == len(want["steps"]) and got["ok"] == int(want["ok"]), what
    assert got["kf_steps"] == want["kf"].n_steps and got["frame_steps"] == want["frame"].n_steps == got["re_steps"], what
    assert got["steps"] == want["steps"].astype(np.float32).tobytes(), "%s: steps" % what
    assert got["kf"].tobytes() == want["kf"].floats().tobytes(), "%s: the key-frame record" % what
    assert got["frame"].tobytes() == want["frame"].floats().tobytes(), "%s: the frame record" % what
    assert got["re"].tobytes() == want["frame"].floats().tobytes(), "%s: the reintegrated record" % what
    assert got["state"].tobytes() == want["state"].tobytes(), "%s: the predicted state" % what
    assert got["link"] == link_bytes(want["link"], which), "%s: the link" % what


def same_as_single(got, one, what):
    for k in ("n", "ok", "kf_steps", "frame_steps"):
        assert got[k] == one[k], "%s: %s" % (what, k)
    for k in ("kf", "frame", "state"):
        assert got[k].tobytes() == one[k].tobytes(), "%s: %s" % (what, k)
    assert got["link"] == one["link"], "%s: link" % what
    if got["steps"] is not None:
        assert got["steps"] == one["steps"], "%s: steps" % what


@pytest.mark.parametrize("which,wname", WHICH, ids=[w[1] for w in WHICH])
@pytest.mark.parametrize("case", PS.CASES, ids=PS.case_id)
def test_host_pointer_calls_equal_restatement(ex, case, which, wname):
    want = PS.ref_cached(case, which)
    if case[0] in PS.NATURAL and case[1] >= 2:
        assert want["ok"]
    same_as_ref(single(ex, PS.make(*case), which), want, PS.case_id(case) + " " + wname, which)


def _dev(t, a):
    return t.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def run_batch(ex, scs, which, want_steps=True, gravity=None, noise=None, two=False):
    """the scenes as one orbfe_imu_frame_batch_device call -> per frame the dict of single(); with `two`, the call is issued twice on
    fresh inputs and both results are returned"""
    import torch
    import orbfe
    B = len(scs)
    off = np.cumsum([0] + [len(sc["t"]) for sc in scs]).astype(np.int32)
    smp = np.concatenate([samples_of(sc) for sc in scs])
    recs = np.zeros((B, 300), np.float32)
    for b, sc in enumerate(scs):
        recs[b, :2].view(np.int32)[:] = (1200, sc["kf"].n_steps)
        recs[b, 2:] = sc["kf"].floats()
    tp, tc = np.array([sc["t_prev"] for sc in scs], np.float64), np.array([sc["t_cur"] for sc in scs], np.float64)
    fb = np.stack([sc["frame_bias"] for sc in scs]).astype(np.float32)
    s1 = np.stack([start_state(sc, which) for sc in scs]).astype(np.float32)
    noise_b, par = blocks(scs[0], which, gravity, noise)
    results = []
    for rep in range(2 if two else 1):
        d_smp, d_tp, d_tc, d_fb, d_s1, d_kf = (_dev(torch, a) for a in (smp, tp, tc, fb, s1, recs))
        d_fr = torch.full((B * 1200,), 0xCD, dtype=torch.uint8, device="cuda")
        d_steps = torch.full((int(off[-1]) * 32,), 0xCD, dtype=torch.uint8, device="cuda")
        d_state = torch.full((B * 33,), -7.0, dtype=torch.float32, device="cuda")
        d_links = torch.full((B * LINK_SIZE[which],), 0xCD, dtype=torch.uint8, device="cuda")
        d_ok = torch.full((B,), -3, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        orbfe.imu_frame_batch_device(ex, noise_b, par, B, d_smp.data_ptr(), off, d_tp.data_ptr(), d_tc.data_ptr(), d_fb.data_ptr(),
                                     d_s1.data_ptr(), d_kf.data_ptr(), d_fr.data_ptr(), d_steps.data_ptr() if want_steps else None,
                                     d_state.data_ptr(), d_links.data_ptr(), d_ok.data_ptr(), st.cuda_stream)
        st.synchronize()
        kf, fr = d_kf.cpu().numpy().view(np.float32).reshape(B, 300), d_fr.cpu().numpy().view(np.float32).reshape(B, 300)
        steps, state = d_steps.cpu().numpy(), d_state.cpu().numpy().reshape(B, 33)
        links, ok = d_links.cpu().numpy().tobytes(), d_ok.cpu().numpy()
        out = []
        for b, sc in enumerate(scs):
            n = max(len(sc["t"]) - 1, 0)
            lo = int(off[b]) * 32
            if want_steps:
                assert (steps[lo + 32 * n:int(off[b + 1]) * 32] == 0xCD).all(), "frame %d: bytes beyond its steps written" % b
            else:
                assert (steps == 0xCD).all()
            out.append(dict(kf=kf[b, 2:], frame=fr[b, 2:], kf_steps=int(kf[b, :2].view(np.int32)[1]), frame_steps=int(fr[b, :2].view(np.int32)[1]),
                            n=n, steps=steps[lo:lo + 32 * n].tobytes() if want_steps else None, state=state[b],
                            link=links[b * LINK_SIZE[which]:(b + 1) * LINK_SIZE[which]], ok=int(ok[b])))
            assert int(kf[b, :2].view(np.int32)[0]) == 1200 and int(fr[b, :2].view(np.int32)[0]) == 1200
        results.append(out)
    return results if two else results[0]


@pytest.mark.parametrize("which,wname", WHICH, ids=[w[1] for w in WHICH])
def test_batch_of_every_scene_equals_restatement(ex, which, wname):
    """every scene as one frame of one launch, against the restatement; the frame records again through the batched reintegration"""
    import torch
    import orbfe
    scs = [PS.make(*c) for c in PS.CASES]
    got = run_batch(ex, scs, which)
    for c, g in zip(PS.CASES, got):
        want = PS.ref_cached(c, which)
        g = dict(g, re=want["frame"].floats(), re_steps=want["frame"].n_steps)
        same_as_ref(g, want, PS.case_id(c) + " in the batch, " + wname, which)
    B = len(scs)
    steps = [PS.ref_cached(c, which)["steps"].astype(np.float32) for c in PS.CASES]
    off = np.cumsum([0] + [len(s) for s in steps]).astype(np.int32)
    d_steps = _dev(torch, np.concatenate(steps))
    d_bias = _dev(torch, np.stack([sc["frame_bias"] for sc in scs]).astype(np.float32))
    d_out = torch.full((B * 1200,), 0xCD, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    orbfe.imu_reintegrate_batch_device(ex, blocks(scs[0], which)[0], B, d_steps.data_ptr(), off, d_bias.data_ptr(), d_out.data_ptr(), st.cuda_stream)
    st.synchronize()
    out = d_out.cpu().numpy().view(np.float32).reshape(B, 300)
    for b, c in enumerate(PS.CASES):
        want = PS.ref_cached(c, which)["frame"]
        assert out[b, 2:].tobytes() == want.floats().tobytes(), PS.case_id(c)
        assert tuple(out[b, :2].view(np.int32)) == (1200, want.n_steps)


def test_batch_of_70_mixed_frames_equals_single_calls(ex):
    """70 frames (more than any block holds waves) with the step counts 1, 2, 3, 10, chunk - 1, chunk + 1 in shuffled order, every frame
    with its own bias and start; frame b equals the single calls"""
    counts = (1, 2, 3, 10, R.CHUNK - 1, R.CHUNK + 1)
    base = {n: PS.make("moving", n, 0) for n in counts}
    rng = np.random.RandomState(70)
    order = rng.permutation(np.repeat(counts, 12))[:70]
    assert set(order) == set(counts)
    for which, wname in WHICH:
        scs = []
        for b, n in enumerate(order):
            sc = dict(base[int(n)])
            sc["frame_bias"] = (sc["frame_bias"] + np.float32(1e-4) * rng.normal(size=6)).astype(np.float32)
            sc["state_kf"] = (sc["state_kf"] + np.float32(1e-3) * np.r_[np.zeros(9), rng.normal(size=12)]).astype(np.float32)
            sc["state_frame"] = (sc["state_frame"] + np.float32(1e-3) * np.r_[np.zeros(9), rng.normal(size=12)]).astype(np.float32)
            scs.append(sc)
        got = run_batch(ex, scs, which)
        for b, (sc, g) in enumerate(zip(scs, got)):
            same_as_single(g, single(ex, sc, which), "frame %d (%d steps), %s" % (b, order[b], wname))


def test_fewer_than_two_samples_change_nothing(ex):
    import orbfe
    sc = PS.make("moving", 3, 0)
    noise, _ = blocks(sc, R.FROM_KEYFRAME)
    for cut in (0, 1):
        kf = orbfe.ImuPreint(sc["kf"].floats(), sc["kf"].n_steps)
        frame, steps, n = orbfe.imu_preintegrate_frame(ex, noise, samples_of(sc)[:cut], sc["t_prev"], sc["t_cur"], sc["frame_bias"], kf)
        assert n == 0 and len(steps) == 0 and kf.floats().tobytes() == sc["kf"].floats().tobytes() and kf.n_steps == sc["kf"].n_steps
        assert bytes(frame) == bytes(orbfe.ImuPreint())


def test_steps_out_may_be_null_and_two_calls_give_equal_bytes(ex):
    scs = [PS.make(*c) for c in (("moving", 10, 0), ("moving", R.CHUNK + 1, 0), ("still", 3, 0))]
    a, b = run_batch(ex, scs, R.FROM_FRAME, two=True)
    c = run_batch(ex, scs, R.FROM_FRAME, want_steps=False)
    for i in range(len(scs)):
        same_as_single(b[i], a[i], "second call, frame %d" % i)
        same_as_single(c[i], a[i], "without steps_out, frame %d" % i)


def test_changed_gravity_and_noise_are_honoured(ex):
    """the parameters are the call's, not constants of the kernel"""
    case = ("moving", 3, 0)
    sc = PS.make(*case)
    noise = R.Noise(ng=3e-4, na=1e-3, ngw=4e-5, naw=1e-3, freq=100.0)
    g = np.float32(9.7)
    for which, wname in WHICH:
        kf, fr, steps = R.preintegrate_frame(noise, sc["t"], sc["a"], sc["w"], sc["t_prev"], sc["t_cur"], sc["frame_bias"], sc["kf"])
        state, link, ok = R.predict(which, start_state(sc, which), kf, fr, g, sc["Rcb"], sc["tcb"], sc["tbc"])
        want = dict(kf=kf, frame=fr, steps=steps, state=state, link=link, ok=ok)
        base = PS.ref_cached(case, which)
        assert want["state"].tobytes() != base["state"].tobytes() and want["kf"].floats().tobytes() != base["kf"].floats().tobytes()
        same_as_ref(single(ex, sc, which, gravity=g, noise=noise), want, "changed gravity and noise, " + wname, which)
        got = run_batch(ex, [sc], which, gravity=g, noise=noise)[0]
        same_as_ref(dict(got, re=fr.floats(), re_steps=fr.n_steps), want, "changed gravity and noise in the batch, " + wname, which)


HAND_OVER = (("moving", 10, 0), ("bias_changed", 10, 0))


def _visual_batch(torch, orbfe, vis):
    B, Ne = len(vis), len(vis[0]["kp_xy"])
    kp = np.zeros((B, Ne), orbfe.KP_DTYPE)
    pts = np.zeros((B, Ne), orbfe.WP_DTYPE)
    for b, v in enumerate(vis):
        kp[b]["x"], kp[b]["y"], kp[b]["octave"], kp[b]["size"] = v["kp_xy"][:, 0], v["kp_xy"][:, 1], v["kp_octave"], 31.0
        for i, f in enumerate("xyz"):
            pts[b][f] = v["points"][:, i]
    match = np.stack([v["mp_index"] for v in vis]).astype(np.int32)
    depth = np.stack([v["track_depth"] for v in vis]).astype(np.float32)
    n = np.full(B, Ne, np.int32)
    return [_dev(torch, a) for a in (kp, n, match, pts, depth)], Ne


def test_hand_over_to_the_inertial_pose_optimisations(ex):
    """d_state_in and d_links as orbfe_imu_frame_batch_device wrote them go, without leaving the device, into the S19 and S20 batch
    calls; the results equal those restatements fed the S22 restatement's link and state"""
    import torch
    import orbfe
    import pose_inertial_prev_ref as R20
    import pose_inertial_ref as R19
    from pose_inertial_scenarios import _spd
    scs = [PS.make(*c) for c in HAND_OVER]
    vis = [PS.visual_edges(sc, 40, i) for i, sc in enumerate(scs)]
    B = len(scs)
    (d_kp, d_n, d_match, d_pts, d_depth), Ne = _visual_batch(torch, orbfe, vis)
    for which, wname in WHICH:
        off = np.cumsum([0] + [len(sc["t"]) for sc in scs]).astype(np.int32)
        smp = np.concatenate([samples_of(sc) for sc in scs])
        recs = np.zeros((B, 300), np.float32)
        for b, sc in enumerate(scs):
            recs[b, :2].view(np.int32)[:] = (1200, sc["kf"].n_steps)
            recs[b, 2:] = sc["kf"].floats()
        d_in = [_dev(torch, a) for a in (smp, np.array([sc["t_prev"] for sc in scs]), np.array([sc["t_cur"] for sc in scs]),
                                         np.stack([sc["frame_bias"] for sc in scs]), np.stack([start_state(sc, which) for sc in scs]), recs)]
        d_fr = torch.zeros((B * 1200,), dtype=torch.uint8, device="cuda")
        d_state = torch.zeros((B * 33,), dtype=torch.float32, device="cuda")
        d_links = torch.zeros((B * LINK_SIZE[which],), dtype=torch.uint8, device="cuda")
        d_ok = torch.zeros((B,), dtype=torch.int32, device="cuda")
        d_out = torch.full((B * 21,), -7.0, dtype=torch.float32, device="cuda")
        d_outl = torch.full((B * Ne,), 0xAB, dtype=torch.uint8, device="cuda")
        d_ninl = torch.full((B,), -3, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        noise, par = blocks(scs[0], which)
        orbfe.imu_frame_batch_device(ex, noise, par, B, d_in[0].data_ptr(), off, d_in[1].data_ptr(), d_in[2].data_ptr(), d_in[3].data_ptr(),
                                     d_in[4].data_ptr(), d_in[5].data_ptr(), d_fr.data_ptr(), None, d_state.data_ptr(), d_links.data_ptr(),
                                     d_ok.data_ptr(), st.cuda_stream)
        refs = [PS.ref_cached(c, which) for c in HAND_OVER]
        if which == R.FROM_KEYFRAME:
            d_H = torch.full((B * 225,), -7.0, dtype=torch.float64, device="cuda")
            orbfe.pose_inertial_optimization_batch_device(ex, orbfe.PoseInertialParams(vis[0]["cam"]), B, d_links.data_ptr(), d_kp.data_ptr(),
                                                          d_n.data_ptr(), Ne, d_match.data_ptr(), Ne, d_pts.data_ptr(), Ne, d_depth.data_ptr(),
                                                          d_state.data_ptr(), d_out.data_ptr(), d_H.data_ptr(), d_outl.data_ptr(),
                                                          d_ninl.data_ptr(), st.cuda_stream)
        else:
            priors = []
            for b, sc in enumerate(scs):
                s = sc["state_frame"].astype(np.float64)
                Hp = _spd(np.random.RandomState(40 + b), [2e4] * 3 + [1e4] * 3 + [2e3] * 3 + [1e6] * 3 + [1e4] * 3, 0.2)
                priors.append(dict(Rwb=s[0:9], twb=s[9:12], vwb=s[12:15], bg=s[15:18], ba=s[18:21], H=Hp.reshape(225)))
            d_pr = _dev(torch, np.frombuffer(b"".join(bytes(orbfe.PoseImuPrior(p)) for p in priors), np.uint8))
            d_H = torch.full((B * 900,), -7.0, dtype=torch.float64, device="cuda")
            d_acc = torch.full((B,), -3, dtype=torch.int32, device="cuda")
            orbfe.pose_inertial_optimization_last_frame_batch_device(
                ex, orbfe.PoseInertialPrevParams(vis[0]["cam"]), B, d_links.data_ptr(), d_pr.data_ptr(), d_kp.data_ptr(), d_n.data_ptr(), Ne,
                d_match.data_ptr(), Ne, d_pts.data_ptr(), Ne, d_depth.data_ptr(), d_state.data_ptr(), d_out.data_ptr(), d_H.data_ptr(), None,
                d_outl.data_ptr(), d_ninl.data_ptr(), d_acc.data_ptr(), st.cuda_stream)
        st.synchronize()
        out, outl, ninl = d_out.cpu().numpy().reshape(B, 21), d_outl.cpu().numpy().reshape(B, Ne), d_ninl.cpu().numpy()
        Hs = d_H.cpu().numpy().reshape(B, -1)
        for b, (v, r) in enumerate(zip(vis, refs)):
            s = r["state"]
            a = (v["cam"], v["level_sigma2"], v["kp_xy"], v["kp_octave"], v["mp_index"], v["points"], v["track_depth"], r["link"])
            tail = (s[0:9], s[9:12], s[12:21], s[21:24], s[24:27], s[27:30], s[30:33])
            if which == R.FROM_KEYFRAME:
                want = R19.pose_inertial_optimization(*a, *tail)
                Hw = want["H"]
            else:
                want = R20.pose_inertial_optimization_last_frame(*a, priors[b], *tail)
                Hw = want["H30"]
                assert int(d_acc.cpu().numpy()[b]) == want["accepted"] == 1
            what = "%s, frame %d" % (wname, b)
            assert np.concatenate([want[k] for k in ("Rwb", "twb", "v", "bg", "ba")]).tobytes() == out[b].tobytes(), what + ": state"
            assert np.ascontiguousarray(Hw, np.float64).tobytes() == Hs[b].tobytes(), what + ": Hessian"
            assert outl[b].tobytes() == want["outlier"].tobytes() and int(ninl[b]) == want["n_inliers"] > 30, what

"""The batched form of the SearchByProjection resolve pass (256 threads, claim tables in LDS, frame records through L2),
which proj_launch selects for launches of at least kResolveBatchedMinFrames frames: every frame of a batched device call
must equal the CPU oracle and the single-frame host call (which keeps the 1024-thread form).  Frames in a batch cycle
through seven distinct scenarios, so a frame that read another frame's data would differ from its own reference."""
import os
import re
import sys

import numpy as np
import pytest

import match_scenarios as S
import oracle_py as O

pytestmark = pytest.mark.gpu
NAMES_O = ("projX", "projY", "viewCos", "trackDepth", "level", "inView", "bad", "observations")
THRESHOLD = 384  # proj::kResolveBatchedMinFrames (match_proj.h)
GRID = (64, 48)
N_DISTINCT = 7


def _extract(orbfe, W, H, nfeat, levels, n, seed0):
    from orbfe import synth
    ex = orbfe.ORBextractor(nfeat, 100000, 1.2, levels, 20, 7, W, H, device=0, max_batch=n)
    res = ex.extract_batch([synth.frame(W, H, seed0 + b) for b in range(n)])
    return ex, [(kp, desc) for kp, desc, _ in res]


def _look_alike(kp, seed):
    """every keypoint descriptor a near copy of one pattern: hundreds of survivors per map point, many exact rescans"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    return np.stack([S.flip_bits(base, int(rng.integers(0, 14)), rng) for _ in range(len(kp))])


def _claim_chain(kp, desc, M, seed):
    """many map points fighting for the same few keypoints: long greedy dependency chains"""
    rng = np.random.default_rng(seed)
    mps = np.zeros(M, O.MP_DTYPE)
    src = rng.integers(0, min(len(kp), 12), M)
    mpd = np.stack([S.flip_bits(desc[s], int(rng.integers(0, 6)), rng) for s in src]) if M else np.zeros((0, 32), np.uint8)
    mps["projX"] = kp["x"][src] + rng.uniform(-2, 2, M).astype(np.float32)
    mps["projY"] = kp["y"][src] + rng.uniform(-2, 2, M).astype(np.float32)
    mps["viewCos"] = 1.0
    mps["level"] = kp["octave"][src]
    mps["inView"] = 1
    mps["observations"] = rng.integers(0, 3, M)
    return mps, mpd, np.full(len(kp), -1, np.int32)


def _crowd(kp, desc, M, seed):
    """M map points with observations, all projected onto one keypoint and searching the same window of look-alike
    keypoints; nnRatio 1.0 lets every one of them claim: once the early ones have taken a later map point's 24 stored
    candidates, that map point is rescanned -- far more of them in one sweep than the batched form parks"""
    rng = np.random.default_rng(seed)
    k0 = int(np.argmin((kp["x"] - 0.5 * kp["x"].max()) ** 2 + (kp["y"] - 0.5 * kp["y"].max()) ** 2 + 1e6 * (kp["octave"] != 0)))
    mps = np.zeros(M, O.MP_DTYPE)
    mpd = np.stack([S.flip_bits(desc[k0], int(rng.integers(0, 8)), rng) for _ in range(M)])
    mps["projX"] = kp["x"][k0] + rng.uniform(-1, 1, M).astype(np.float32)
    mps["projY"] = kp["y"][k0] + rng.uniform(-1, 1, M).astype(np.float32)
    mps["viewCos"] = 0.9
    mps["level"] = 1
    mps["inView"] = 1
    mps["observations"] = 1
    return mps, mpd, np.full(len(kp), -1, np.int32)


def _cases(frames, M, levels, kind, seed):
    out = []
    for c, (kp, desc) in enumerate(frames):
        if kind == "crowd":
            desc = _look_alike(kp, seed + c)
            mps, mpd, obs = _crowd(kp, desc, M, seed + c)
        elif kind == "look_alike":
            desc = _look_alike(kp, seed + c)
            mps, mpd, obs = S.projection_scenario(kp, desc, M, seed + c, O.MP_DTYPE, NAMES_O, levels, jitter=6.0, max_flip=10)
        elif kind == "chain":
            mps, mpd, obs = _claim_chain(kp, desc, M, seed + c)
        else:
            mps, mpd, obs = S.projection_scenario(kp, desc, M, seed + c, O.MP_DTYPE, NAMES_O, levels)
        out.append((kp, desc, mps, mpd, obs))
    return out


def _run(orbfe, ex, W, H, cases, B, M, th, nn, use_obs, far=False, th_far=12.0):
    import torch
    cap = ex.cap
    m = orbfe.ORBmatcher(ex)
    refs = []
    for kp, desc, mps, mpd, obs in cases:
        io = obs if use_obs else None
        fvo = O.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
        ref = O.search_by_projection(fvo, mps, mpd, io, th, nn, far, th_far)
        fv = orbfe.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
        one = m.SearchByProjection(fv, mps.view(orbfe.MP_DTYPE), mpd, th, far, th_far, nn, io)  # B = 1: the 1024-thread form
        assert one[0] == ref[0] and np.array_equal(one[1], ref[1])
        refs.append(ref)
    kp_all = np.zeros((B, cap), orbfe.KP_DTYPE)
    desc_all = np.zeros((B, cap, 32), np.uint8)
    n_all = np.zeros(B, np.int32)
    mps_all = np.zeros((B, max(M, 1)), orbfe.MP_DTYPE)
    mpd_all = np.zeros((B, max(M, 1), 32), np.uint8)
    obs_all = np.full((B, cap), -1, np.int32)
    for b in range(B):
        kp, desc, mps, mpd, obs = cases[b % len(cases)]
        n_all[b] = len(kp)
        kp_all[b, :len(kp)] = kp
        desc_all[b, :len(kp)] = desc
        mps_all[b, :M] = mps.view(orbfe.MP_DTYPE)
        mpd_all[b, :M] = mpd
        obs_all[b, :len(kp)] = obs
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
    d_kp, d_desc, d_n, d_mps, d_mpd, d_obs = t(kp_all), t(desc_all), t(n_all), t(mps_all), t(mpd_all), t(obs_all)
    d_out = torch.full((B * cap,), 7, dtype=torch.int32, device=dev)
    d_nm = torch.full((B,), 7, dtype=torch.int32, device=dev)
    m.SearchByProjection_batch_device(B, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, GRID[0], GRID[1], 0.0, 0.0,
                                      float(W), float(H), M, d_mps.data_ptr(), d_mpd.data_ptr(),
                                      d_obs.data_ptr() if use_obs else None, th, nn, d_out.data_ptr(), d_nm.data_ptr(),
                                      bFarPoints=far, thFarPoints=th_far, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy().reshape(B, cap)
    nm = d_nm.cpu().numpy()
    for b in range(B):
        n_ref, out_ref = refs[b % len(cases)]
        assert nm[b] == n_ref, (b, nm[b], n_ref)
        assert np.array_equal(out[b, :n_all[b]], out_ref), b
    return [r[0] for r in refs]


@pytest.fixture(scope="module")
def euroc(built):
    import orbfe
    ex, frames = _extract(orbfe, 752, 480, 1000, 8, N_DISTINCT, 300)
    return orbfe, ex, frames


@pytest.mark.parametrize("B", [THRESHOLD - 1, THRESHOLD, 512])
def test_batched_default_scene(euroc, B):
    """the bench's shape: 2000 map points (not a multiple of 256), initial claims, th 20 / 0.85"""
    orbfe, ex, frames = euroc
    n = _run(orbfe, ex, 752, 480, _cases(frames, 2000, 8, "default", 11), B, 2000, 20.0, 0.85, True)
    assert min(n) > 200


@pytest.mark.parametrize("kind,M,th,nn,use_obs,far", [
    ("default", 2000, 40.0, 0.75, False, False),
    ("default", 1500, 20.0, 0.85, True, True),     # farPoints filter
    ("chain", 600, 20.0, 0.85, False, False),      # adversarial claim chain
    ("look_alike", 700, 40.0, 0.95, True, False),  # hundreds of survivors
    ("crowd", 1000, 20.0, 1.0, False, False),       # starved map points beyond the parking area
    ("default", 200, 20.0, 0.85, True, False),     # M < 256: one partial chunk
    ("default", 0, 20.0, 0.85, True, False),       # no map points
])
def test_batched_scenes(euroc, kind, M, th, nn, use_obs, far):
    orbfe, ex, frames = euroc
    n = _run(orbfe, ex, 752, 480, _cases(frames, M, 8, kind, 23), THRESHOLD, M, th, nn, use_obs, far)
    if M >= 600:
        assert min(n) > (5 if kind == "chain" else 20)  # the chain scene has only 12 distinct source keypoints


@pytest.mark.parametrize("nfeat,W,H,min_n", [(1600, 1280, 720, 1281), (3000, 1280, 720, 2049)])
def test_batched_large_frames(built, nfeat, W, H, min_n):
    """frames above the 1280-keypoint descriptor image of the 1024-thread form and above the 2048-keypoint LDS claim
    tables (kpStride > 2048: claim tables in global memory)"""
    import orbfe
    ex, frames = _extract(orbfe, W, H, nfeat, 8, N_DISTINCT, 400)
    assert max(len(kp) for kp, _ in frames) >= min_n and ex.cap >= min_n
    n = _run(orbfe, ex, W, H, _cases(frames, 2500, 8, "default", 31), THRESHOLD, 2500, 20.0, 0.85, True)
    assert min(n) > 200


def test_batched_form_forced_on_single_frame_paths(built):
    """Relocalisation mode (orbfe_match_projection_keyframe) and the single-frame host call with the batched form forced.
    The switch (ORBFE_RESOLVE_THREADS=0) exists only in the diagnostics build liborbfe_diag.so -- the shipped library reads
    no environment variable -- so this runs once in a child process that loads that build."""
    import subprocess
    import __graft_entry__ as g
    g.build_variant("diag")
    env = dict(os.environ, ORBFE_RESOLVE_THREADS="0", ORBFE_DEBUG_MATCH="1", ORBFE_TEST_LIB="liborbfe_diag.so")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "forced batched resolve: exact" in p.stdout, p.stdout[-1000:] + p.stderr[-2000:]
    # the crowd scene starves more map points in one sweep than the batched form parks (kFbBatched = 32): the rescans
    # beyond the parking area (window + descriptor re-read from global memory) ran, and the results above are exact
    unparked = [int(v) for v in re.findall(r"unparked_rescans=(\d+)", p.stderr)]
    assert unparked and max(unparked) > 0, p.stderr[-2000:]


def _forced_child():
    import frustum_scenarios as FS
    import orbfe
    import test_sim3_reloc as T3
    from test_frustum import ON, PN
    orbfe.LIB_PATH = os.path.join(orbfe.CSRC, os.environ["ORBFE_TEST_LIB"])
    assert os.environ.get("ORBFE_RESOLVE_THREADS") == "0"
    W, H = T3.W, T3.H
    ex = orbfe.ORBextractor(*T3.ARGS)
    m = orbfe.ORBmatcher(ex)
    for seed, M, th in ((1, 2000, 12.0), (3, 5000, 25.0), (6, 3000, 60.0)):
        eo, kp, desc = T3.extraction(40 + seed)
        Fo, Fp = O.Frustum(), orbfe.Frustum()
        v = FS.fill_frustum(Fo, ON, seed=50 + seed)
        FS.fill_frustum(Fp, PN, seed=50 + seed)
        pts, mpd, ang, has = T3.reloc_scenario(kp, desc, eo.scaleFactors, v, M, seed)
        fvo = O.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), eo.scaleFactors)
        fv = orbfe.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
        n_r, m_r = O.search_by_projection_kf(fvo, Fo, pts, mpd, ang, has, th, True)
        n, mm = m.SearchByProjection_keyframe(fv, Fp, pts.view(orbfe.WP_DTYPE), mpd, ang, has, th, True)
        assert n == n_r and np.array_equal(mm, m_r) and n > 150, ("reloc", seed)
    # single-frame host calls: the bench's scene, look-alike descriptors, a frame above 2048 keypoints
    exb, frames = _extract(orbfe, 1280, 720, 3000, 8, 1, 500)
    for kind, (kp, desc), M, nn in (("default", frames[0], 2000, 0.85), ("look_alike", frames[0], 700, 0.85),
                                    ("crowd", frames[0], 1000, 1.0), ("chain", frames[0], 600, 0.85)):
        assert len(kp) > 2048
        kp_, desc_, mps, mpd, obs = _cases([(kp, desc)], M, 8, kind, 41)[0]
        fvo = O.make_frame_view(kp_, desc_, GRID[0], GRID[1], 0.0, 0.0, 1280.0, 720.0, exb.mvScaleFactor)
        n_r, m_r = O.search_by_projection(fvo, mps, mpd, obs, 20.0, nn)
        fv = orbfe.make_frame_view(kp_, desc_, GRID[0], GRID[1], 0.0, 0.0, 1280.0, 720.0, exb.mvScaleFactor)
        n, mm = orbfe.ORBmatcher(exb).SearchByProjection(fv, mps.view(orbfe.MP_DTYPE), mpd, 20.0, False, 0.0, nn, obs)
        assert n == n_r and np.array_equal(mm, m_r), kind
    print("forced batched resolve: exact")


if __name__ == "__main__":  # child of test_batched_form_forced_on_single_frame_paths
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam3_v1.0_amd", "python"))
    _forced_child()

"""The thread-per-map-point top-K pass (proj_topk_kernel) parks the keys a lane finds and inserts them in wave-wide
rounds (topk_insert_round): every case runs 16 frames x ~2000 map points -- 128 blocks, the smallest launch that takes
that kernel -- through SearchByProjection_batch_device and compares match indices and counts with the CPU oracle, byte
for byte.  The scenes aim at the queue: back-to-back rounds and a stale bound (crowd), a lane that fills and drains
alone, keys still pending when the loops end (level 0 only), a partial last wave, the global-memory path and the
three-level relocalisation mode."""
import numpy as np
import pytest

import match_scenarios as S
import oracle_py as O
from orbfe import synth

pytestmark = pytest.mark.gpu
NAMES_O = ("projX", "projY", "viewCos", "trackDepth", "level", "inView", "bad", "observations")
GRID = (64, 48)
B = 16
TOPK = 24        # proj::kTopK (match_proj.h)
TOPK_LDS = 768   # kTopkLds (kernels_match_proj.hip)
DCUT = 118       # proj_dcut(0.85)
N_DISTINCT = 4   # distinct frames; the 16 frames of a call cycle through them with their own map points


def _frames(W, H, nfeat, index0):
    e = O.Extractor(nfeat, 40000, 1.2, 8, 20, 7, W, H)
    return e, [e.extract(im)[:2] for im in synth.stream(W, H, N_DISTINCT, index0=index0)]


@pytest.fixture(scope="module")
def euroc(built):
    import orbfe
    e, frames = _frames(752, 480, 1000, 40)
    ex = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480, device=0, max_batch=B)
    return orbfe, ex, e, frames


def _run(orbfe, ex, e, W, H, cases, M, th, nn, use_obs):
    """cases: B tuples (kp, desc, mps, mpd, init_obs); one batched device call against B oracle calls"""
    import torch
    assert len(cases) == B and (M + 255) // 256 * B >= 128  # proj_launch: thread-per-map-point kernel
    cap = ex.cap
    kp_all = np.zeros((B, cap), orbfe.KP_DTYPE)
    desc_all = np.zeros((B, cap, 32), np.uint8)
    n_all = np.zeros(B, np.int32)
    mps_all = np.zeros((B, M), orbfe.MP_DTYPE)
    mpd_all = np.zeros((B, M, 32), np.uint8)
    obs_all = np.full((B, cap), -1, np.int32)
    refs = []
    for b, (kp, desc, mps, mpd, obs) in enumerate(cases):
        assert len(kp) <= cap and len(mps) == M
        n_all[b] = len(kp)
        kp_all[b, :len(kp)] = kp
        desc_all[b, :len(kp)] = desc
        mps_all[b] = mps.view(orbfe.MP_DTYPE)
        mpd_all[b] = mpd
        obs_all[b, :len(kp)] = obs
        fvo = O.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), e.scaleFactors)
        refs.append(O.search_by_projection(fvo, mps, mpd, obs if use_obs else None, th, nn))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)
    d_kp, d_desc, d_n, d_mps, d_mpd, d_obs = t(kp_all), t(desc_all), t(n_all), t(mps_all), t(mpd_all), t(obs_all)
    d_out = torch.full((B * cap,), 7, dtype=torch.int32, device=dev)
    d_nm = torch.full((B,), 7, dtype=torch.int32, device=dev)
    orbfe.ORBmatcher(ex).SearchByProjection_batch_device(
        B, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H), M,
        d_mps.data_ptr(), d_mpd.data_ptr(), d_obs.data_ptr() if use_obs else None, th, nn, d_out.data_ptr(), d_nm.data_ptr(),
        stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy().reshape(B, cap)
    nm = d_nm.cpu().numpy()
    for b in range(B):
        assert nm[b] == refs[b][0], (b, nm[b], refs[b][0])
        assert out[b, :n_all[b]].tobytes() == refs[b][1].tobytes(), b
    return [r[0] for r in refs]


def _default_cases(frames, M, n_levels, seed):
    return [frames[b % len(frames)] + S.projection_scenario(*frames[b % len(frames)], M, seed + b, O.MP_DTYPE, NAMES_O, n_levels)
            for b in range(B)]


def _crowd_level(kp):
    """the level 0..3 with the most keypoints"""
    return int(np.argmax([(kp["octave"] == l).sum() for l in range(4)]))


def _crowd_case(kp, desc, M, seed, mp_level=None):
    """The keypoints of one level get near copies (0..3 flipped bits) of ONE descriptor; M map points sit on them with near
    copies of it too and a window of half the frame: each has far more than TOPK candidates under the cut-off, arriving in
    runs along the storage order -- a full queue in every iteration, back-to-back rounds, a bound that goes stale."""
    rng = np.random.default_rng(seed)
    lvl = _crowd_level(kp)
    members = np.flatnonzero(kp["octave"] == lvl)
    assert len(members) >= 200, len(members)
    desc = desc.copy()
    base = desc[members[0]].copy()
    for j in members:
        desc[j] = S.flip_bits(base, int(rng.integers(0, 4)), rng)
    src = members[rng.integers(0, len(members), M)]
    mps = np.zeros(M, O.MP_DTYPE)
    mpd = np.stack([S.flip_bits(base, int(rng.integers(0, 11)), rng) for _ in range(M)])
    mps["projX"] = kp["x"][src] + rng.uniform(-3, 3, M).astype(np.float32)
    mps["projY"] = kp["y"][src] + rng.uniform(-3, 3, M).astype(np.float32)
    mps["viewCos"] = np.where(rng.random(M) < 0.8, 1.0, 0.9)
    mps["trackDepth"] = 5.0
    mps["level"] = (lvl + (rng.random(M) < 0.3)) if mp_level is None else mp_level  # searches [level - 1, level]
    mps["inView"] = 1
    mps["observations"] = rng.integers(0, 4, M)
    obs = np.full(len(kp), -1, np.int32)
    return kp, desc, mps, mpd, obs


def _candidates(kp, desc, mp, mpd, th, sf):
    """number of keypoints inside the map point's window (src/Frame.cc:437-461) with distance < DCUT"""
    lvl = int(mp["level"])
    r = (2.5 if mp["viewCos"] > 0.998 else 4.0) * th * sf[lvl]
    inside = (np.abs(kp["x"] - mp["projX"]) < r) & (np.abs(kp["y"] - mp["projY"]) < r) & \
             (kp["octave"] >= lvl - 1) & (kp["octave"] <= lvl)
    dist = np.unpackbits(desc[inside] ^ mpd[None, :], axis=1).sum(axis=1)
    return int((dist < DCUT).sum())


CROWD_TH = 100.0  # radius 250 / 400 px at level 0: a window holds half the frame's keypoints of the level or more


def _assert_crowded(case, sf):
    kp, desc, mps, mpd, _ = case
    most = max(_candidates(kp, desc, mps[i], mpd[i], CROWD_TH, sf) for i in range(0, len(mps), 97))
    assert most >= 4 * TOPK, most


@pytest.fixture(scope="module")
def default_cases(euroc):
    _, _, e, frames = euroc
    return _default_cases(frames, 2000, e.nLevels, 60)  # shared, read only


@pytest.mark.parametrize("use_obs", [True, False])
def test_default_scene(euroc, default_cases, use_obs):
    orbfe, ex, e, _ = euroc
    n = _run(orbfe, ex, e, 752, 480, default_cases, 2000, 20.0, 0.85, use_obs)
    assert min(n) > 200


def test_crowd(euroc):
    orbfe, ex, e, frames = euroc
    cases = [_crowd_case(*frames[b % len(frames)], 2000, 70 + b) for b in range(B)]
    _assert_crowded(cases[0], e.scaleFactors)
    _run(orbfe, ex, e, 752, 480, cases, 2000, CROWD_TH, 0.85, False)


def test_lonely_lane(euroc):
    """64 q + 1 valid map points in a frame: the invalid ones sort behind the valid ones in the (level, tile) order, so one
    wave of the frame holds exactly ONE valid lane -- a crowd lane, which fills its queue and drains it alone.  q = 0..3
    over the frames: the lonely wave is the 1st .. 4th of its block."""
    orbfe, ex, e, frames = euroc
    cases = []
    for b in range(B):
        kp, desc, mps, mpd, obs = _crowd_case(*frames[b % len(frames)], 2000, 90 + b)
        wide = np.flatnonzero(mps["viewCos"] < 0.95)  # radius 400 px and more: most of the level's keypoints
        keep = np.random.default_rng(b).choice(wide, 64 * (b % 4) + 1, replace=False)
        mps["inView"] = 0
        mps["inView"][keep] = 1
        cases.append((kp, desc, mps, mpd, obs))
    kp, desc, mps, mpd, _ = cases[0]
    i = int(np.flatnonzero(mps["inView"])[0])
    assert _candidates(kp, desc, mps[i], mpd[i], CROWD_TH, e.scaleFactors) >= 4 * TOPK
    _run(orbfe, ex, e, 752, 480, cases, 2000, CROWD_TH, 0.85, False)


def test_level0_only(euroc):
    """map points at level 0: the second range of every lane is empty, keys are still pending when the loops end"""
    orbfe, ex, e, frames = euroc
    cases = []
    for b in range(B):
        kp, desc = frames[b % len(frames)]
        if b % 2:  # the default scene with every map point moved to level 0
            mps, mpd, obs = S.projection_scenario(kp, desc, 2000, 110 + b, O.MP_DTYPE, NAMES_O, e.nLevels)
            mps["level"] = 0
            cases.append((kp, desc, mps, mpd, obs))
        else:
            cases.append(_crowd_case(kp, desc, 2000, 110 + b, mp_level=0))
    assert _crowd_level(frames[0][0]) == 0
    _assert_crowded(cases[0], e.scaleFactors)
    _run(orbfe, ex, e, 752, 480, cases, 2000, CROWD_TH, 0.85, True)


def test_partial_last_wave(euroc):
    """M = 2000 leaves a 16-lane last wave (the cases above); 1999 a 15-lane one"""
    orbfe, ex, e, frames = euroc
    n = _run(orbfe, ex, e, 752, 480, _default_cases(frames, 1999, e.nLevels, 130), 1999, 20.0, 0.85, True)
    assert min(n) > 200


def test_global_memory_path(built):
    """1280 x 720 with 3000 features: levels 0 + 1 together exceed the kTopkLds keypoints a block stages in LDS, so the
    blocks of the map points at level 1 read records and descriptors from global memory"""
    import orbfe
    W, H = 1280, 720
    e, frames = _frames(W, H, 3000, 50)
    ex = orbfe.ORBextractor(3000, 40000, 1.2, 8, 20, 7, W, H, device=0, max_batch=B)
    cases = _default_cases(frames, 2000, e.nLevels, 150)
    for kp, _, mps, _, _ in cases:
        per_level = np.bincount(kp["octave"], minlength=8)
        assert per_level[0] + per_level[1] > TOPK_LDS and ((mps["level"] == 1) & (mps["inView"] != 0) & (mps["bad"] == 0)).sum() > 64
    n = _run(orbfe, ex, e, W, H, cases, 2000, 20.0, 0.85, True)
    assert min(n) > 200


def test_relocalisation(built):
    """kModeReloc: three levels per map point (the two-level body runs a second time), no ratio test.  The entry point
    takes one frame, so 33,000 map points make the 128 blocks; look-alike descriptors keep the queues busy."""
    import frustum_scenarios as FS
    import orbfe
    import test_sim3_reloc as T3
    from test_frustum import ON, PN
    M = 33000
    assert (M + 255) // 256 >= 128
    e = O.Extractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    kp, desc, _ = e.extract(synth.frame(752, 480, 2))
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = np.stack([S.flip_bits(base, int(rng.integers(0, 14)), rng) for _ in range(len(kp))])
    ex = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480, device=0, max_batch=1)
    Fo, Fp = O.Frustum(), orbfe.Frustum()
    v = FS.fill_frustum(Fo, ON, seed=78)
    FS.fill_frustum(Fp, PN, seed=78)
    pts, mpd, ang, has = T3.reloc_scenario(kp, desc, e.scaleFactors, v, M, 10)
    fvo = O.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, 752.0, 480.0, e.scaleFactors)
    fv = orbfe.make_frame_view(kp, desc, GRID[0], GRID[1], 0.0, 0.0, 752.0, 480.0, ex.mvScaleFactor)
    n_ref, out_ref = O.search_by_projection_kf(fvo, Fo, pts, mpd, ang, has, 25.0, True)
    n, out = orbfe.ORBmatcher(ex).SearchByProjection_keyframe(fv, Fp, pts.view(orbfe.WP_DTYPE), mpd, ang, has, 25.0, True)
    assert n == n_ref and out.tobytes() == out_ref.tobytes()
    assert n_ref > 50

"""The multi-device pool (orbfe_pool_*): the frames of a call sharded over N members (a handle + a ring each, devices may
repeat), every member on a worker thread of its own, all results in one frame-major layout.  Byte-equal to one plain handle
(orbfe_extract_batch, orbfe_track_frame_map) and to the oracle, whatever the member count; one map replicated on every
member; argument errors refused before any work; create / destroy cycles give their memory back."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import oracle_py as O
from test_pool_cpu import build_program
from test_stream_track_gpu import ARGS, GRID, build_scene, local_ids, oracle_frame

pytestmark = pytest.mark.gpu

MAX_BATCH, SLOT = 16, 8
W, H = ARGS[6], ARGS[7]


def _pinned(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().numpy()


def _frames(n, seed=0):
    from orbfe import synth
    return np.stack(list(synth.stream(W, H, n, index0=300 + seed)))


def _plain_extract(ex, frames):
    out = []
    for lo in range(0, len(frames), MAX_BATCH):
        out += ex.extract_batch(list(frames[lo:lo + MAX_BATCH]))
    return out


def _same(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "frame %d" % i


def test_pool_extract_equals_plain_handle_and_oracle(built):
    import orbfe
    frames = _frames(3 * SLOT + 1)
    ex = orbfe.ORBextractor(*ARGS, device=0, max_batch=MAX_BATCH)
    ref = _plain_extract(ex, frames)
    eo = O.Extractor(*ARGS)
    for f in (0, 5, 3 * SLOT):  # a sample against the oracle
        kp_r, desc_r, per_r = eo.extract(frames[f])
        assert ref[f][0].tobytes() == kp_r.tobytes() and np.array_equal(ref[f][1], desc_r) and len(kp_r) > 100
    padded = np.zeros((len(frames), H, W + 8), np.uint8)  # pitch W + 8
    padded[:, :, :W] = frames
    sources = {"pinned": (_pinned(frames), None), "pageable": (frames, None), "pinned_padded": (_pinned(padded), W + 8),
               "pageable_padded": (padded, W + 8), "pageable_odd_pitch": (np.ascontiguousarray(np.pad(frames, ((0, 0), (0, 0), (0, 3)))), W + 3)}
    for devices in ([0], [0, 0], [0, 0, 0]):
        pool = orbfe.Pool(ARGS, devices, slots=3, slot_frames=SLOT, max_batch=MAX_BATCH)
        assert pool.size == len(devices) and pool.cap == ex.cap and pool.nlevels == ex.nlevels
        expect = [0] * len(devices)
        for n in (1, 2, 7, 3 * SLOT + 1):
            for name, (src, pitch) in sources.items():
                if n < 3 * SLOT + 1 and name not in ("pinned", "pageable"):
                    continue
                got = pool.extract(src[:n], pitch=pitch)
                _same(got, ref[:n])
                for k in range(len(devices)):
                    lo, hi = orbfe.shard_range(n, k, len(devices))
                    expect[k] += hi - lo
                assert pool.member_frames() == expect, (devices, n, name)
        if len(devices) == 3:
            assert expect[2] > 0 and pool.member_frames()[1] > 0
        pool.close()
    # one frame over three members: two of them have nothing to do
    pool = orbfe.Pool(ARGS, [0, 0, 0], slots=2, slot_frames=SLOT, max_batch=MAX_BATCH)
    _same(pool.extract(frames[:1]), ref[:1])
    assert pool.member_frames() == [1, 0, 0]
    pool.close()


def _scene(n_frames, seed):
    eo, frames, frusta_o, frusta_p, map_pts, map_desc, owner = build_scene(n_frames, 260, seed=seed)
    cap_map = len(map_pts) + 100
    rng = np.random.default_rng(10 + seed)
    ids = np.stack([local_ids(f, owner, 900, cap_map, rng) for f in range(n_frames)])
    return eo, frames, frusta_o, frusta_p, map_pts, map_desc, cap_map, ids


def _plain_track(ex, mp, frames, frusta_p, ids):
    import orbfe
    trk = orbfe.FrameTracker(ex, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
    return [trk.TrackFrameMap(frames[f], frusta_p[f], mp, ids[f], 20.0, 0.85) for f in range(len(frames))]


def test_pool_track_equals_track_frame_map_and_oracle(built):
    import orbfe
    n_frames = 2 * SLOT + 1
    eo, frames, frusta_o, frusta_p, map_pts, map_desc, cap_map, ids = _scene(n_frames, seed=3)
    assert (ids < 0).any() and (ids >= cap_map).any()  # skipped and out-of-map ids are part of every frame's list
    ex = orbfe.ORBextractor(*ARGS, device=0, max_batch=MAX_BATCH)
    mp = orbfe.MapPoints(ex, cap_map)
    mp.update(np.arange(len(map_pts)), map_pts.view(orbfe.WP_DTYPE), map_desc)
    ref = _plain_track(ex, mp, frames, frusta_p, ids)
    pool = orbfe.Pool(ARGS, [0, 0, 0], slots=3, slot_frames=SLOT, max_batch=MAX_BATCH)
    pool.enable_track(cap_map, 900, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
    pool.map_update(np.arange(len(map_pts)), map_pts.view(orbfe.WP_DTYPE), map_desc)
    for src in (_pinned(frames), frames):
        got = pool.track(src, frusta_p, ids, 20.0, 0.85)
        total = 0
        for f in range(n_frames):
            kp, desc, per, match, nm = got[f]
            r = ref[f]
            assert kp.tobytes() == r["kp"].tobytes() and np.array_equal(desc, r["desc"]), f
            assert nm == r["nmatches"] and np.array_equal(match, r["match"]), "frame %d: %d vs %d" % (f, nm, r["nmatches"])
            kp_o, desc_o, per_o, match_o, n_o, _, _ = oracle_frame(eo, frames[f], frusta_o[f], ids[f], map_pts, map_desc, 20.0, 0.85)
            assert kp.tobytes() == kp_o.tobytes() and np.array_equal(per, per_o) and nm == n_o and np.array_equal(match, match_o), f
            total += nm
        assert total > 80 * n_frames
    assert pool.member_frames() == [12, 12, 10]
    pool.close()
    mp.close()


def test_pool_map_update_reaches_every_member(built):
    import orbfe
    n_frames = 3 * 4
    eo, frames, frusta_o, frusta_p, map_pts, map_desc, cap_map, ids = _scene(n_frames, seed=5)
    pool = orbfe.Pool(ARGS, [0, 0, 0], slots=2, slot_frames=4, max_batch=MAX_BATCH)
    pool.enable_track(cap_map, 900, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
    pool.map_update(np.arange(len(map_pts)), map_pts.view(orbfe.WP_DTYPE), map_desc)
    first = pool.track(frames, frusta_p, ids, 20.0, 0.85)
    # move a third of the points and give them other descriptors
    rng = np.random.default_rng(8)
    sel = np.flatnonzero(rng.random(len(map_pts)) < 0.35).astype(np.int32)
    moved, mdesc = map_pts.copy(), map_desc.copy()
    moved["x"][sel] += np.float32(0.05)
    mdesc[sel] = ~mdesc[sel]
    pool.map_update(sel, moved[sel].view(orbfe.WP_DTYPE), mdesc[sel])
    second = pool.track(frames, frusta_p, ids, 20.0, 0.85)
    for f in range(n_frames):  # frames 0-3 ran on member 0, 4-7 on member 1, 8-11 on member 2
        _, _, _, match_o, n_o, _, _ = oracle_frame(eo, frames[f], frusta_o[f], ids[f], moved, mdesc, 20.0, 0.85)
        assert second[f][4] == n_o and np.array_equal(second[f][3], match_o), f
        assert second[f][4] < first[f][4], f
    pool.close()


def _raw_outputs(pool, n):
    kp = np.full(n * pool.cap * 24, 0x5A, np.uint8)
    desc = np.full(n * pool.cap * 32, 0x5A, np.uint8)
    cnt = np.full(n, 0x5A5A5A5A, np.int32)
    per = np.full(n * pool.nlevels, 0x5A5A5A5A, np.int32)
    match = np.full(n * pool.cap, 0x5A5A5A5A, np.int32)
    nm = np.full(n, 0x5A5A5A5A, np.int32)
    return kp, desc, cnt, per, match, nm


def _untouched(arrs):
    return all((a.view(np.uint8) == 0x5A).all() for a in arrs)


def test_pool_argument_errors_write_nothing_and_the_next_call_is_exact(built):
    import orbfe
    import torch
    n_frames = 9
    eo, frames, frusta_o, frusta_p, map_pts, map_desc, cap_map, ids = _scene(n_frames, seed=6)
    ex = orbfe.ORBextractor(*ARGS, device=0, max_batch=MAX_BATCH)
    mp = orbfe.MapPoints(ex, cap_map)
    mp.update(np.arange(len(map_pts)), map_pts.view(orbfe.WP_DTYPE), map_desc)
    ref = _plain_track(ex, mp, frames, frusta_p, ids)
    pool = orbfe.Pool(ARGS, [0, 0], slots=3, slot_frames=4, max_batch=MAX_BATCH)
    L = pool.L
    ptrs = (C.c_void_p * n_frames)(*[frames[f].ctypes.data for f in range(n_frames)])
    fr = (orbfe.Frustum * n_frames)(*frusta_p)
    tp = pool.track_params(20.0, 0.85)
    out = _raw_outputs(pool, n_frames)
    P = [o.ctypes.data_as(C.c_void_p) for o in out]

    def track(n_points, frusta=fr, t=tp, pitch=W):
        return L.orbfe_pool_track(pool.h, ptrs, pitch, n_frames, C.byref(t), frusta, n_points, ids.ctypes.data, *P)

    assert track(ids.shape[1]) == 1  # before enable_track
    assert L.orbfe_pool_map_update(pool.h, 1, np.zeros(1, np.int32).ctypes.data, map_pts[:1].ctypes.data, map_desc[:1].ctypes.data) == 1
    pool.enable_track(cap_map, ids.shape[1], GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
    tp = pool.track_params(20.0, 0.85)
    assert L.orbfe_pool_enable_track(pool.h, cap_map, ids.shape[1]) == 1  # once per pool
    pool.map_update(np.arange(len(map_pts)), map_pts.view(orbfe.WP_DTYPE), map_desc)
    assert track(ids.shape[1] + 1, t=tp) == 1  # n_points > max_points
    bad = (orbfe.Frustum * n_frames)(*frusta_p)
    bad[n_frames - 1].n_levels = 0  # the last frame's frustum (member 1's block) is refused before member 0 starts
    assert track(ids.shape[1], frusta=bad, t=tp) == 1
    bad[n_frames - 1].n_levels = ARGS[3] + 1  # more levels than the extractor has
    assert track(ids.shape[1], frusta=bad, t=tp) == 1
    tp_bad = pool.track_params(20.0, 0.85)
    tp_bad.struct_size = 8
    assert track(ids.shape[1], t=tp_bad) == 1
    assert track(ids.shape[1], t=tp, pitch=W - 1) == 1
    assert L.orbfe_pool_extract(pool.h, ptrs, W, 0, *P[:4]) == 1
    assert L.orbfe_pool_extract(pool.h, ptrs, W, n_frames, None, *P[1:4]) == 1
    assert L.orbfe_pool_map_update(pool.h, 1, np.array([cap_map], np.int32).ctypes.data, map_pts[:1].ctypes.data, map_desc[:1].ctypes.data) == 1
    assert _untouched(out), "a refused call wrote output"
    assert pool.member_frames() == [0, 0]
    # the next valid call is exact
    got = pool.track(frames, frusta_p, ids, 20.0, 0.85)
    for f in range(n_frames):
        assert got[f][0].tobytes() == ref[f]["kp"].tobytes() and got[f][4] == ref[f]["nmatches"] and np.array_equal(got[f][3], ref[f]["match"])
    assert pool.member_frames() == [5, 4]
    pool.close()
    mp.close()
    with pytest.raises(orbfe.OrbfeError) as ei:
        orbfe.Pool(ARGS, [0, torch.cuda.device_count()], slot_frames=SLOT, max_batch=MAX_BATCH)
    assert ei.value.code == 1


def test_pool_create_use_destroy_gives_memory_back(built):
    import gc
    import orbfe
    import torch
    frames = _pinned(_frames(9, seed=4))
    eo, sframes, _, frusta_p, map_pts, map_desc, cap_map, ids = _scene(4, seed=9)

    def cycle():
        pool = orbfe.Pool(ARGS, [0, 0], slots=3, slot_frames=4, max_batch=MAX_BATCH)
        pool.extract(frames)
        pool.enable_track(cap_map, ids.shape[1], GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
        pool.map_update(np.arange(len(map_pts)), map_pts.view(orbfe.WP_DTYPE), map_desc)
        pool.track(sframes, frusta_p, ids, 20.0, 0.85)
        pool.close()

    for _ in range(2):  # warm-up
        cycle()
    gc.collect()
    free0 = torch.cuda.mem_get_info(0)[0] / 2 ** 20
    for _ in range(10):
        cycle()
    gc.collect()
    free1 = torch.cuda.mem_get_info(0)[0] / 2 ** 20
    assert free0 - free1 < 32, "device memory shrank by %.0f MB over 10 pools" % (free0 - free1)


def test_pool_on_two_devices_equals_plain_handle(built):
    import orbfe
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    frames = _pinned(_frames(2 * SLOT + 3, seed=2))
    ex = orbfe.ORBextractor(*ARGS, device=0, max_batch=MAX_BATCH)
    pool = orbfe.Pool(ARGS, [0, 1], slots=3, slot_frames=SLOT, max_batch=MAX_BATCH)
    _same(pool.extract(frames), _plain_extract(ex, frames))
    assert pool.member_frames() == [10, 9]
    pool.close()


def test_pool_cpp_program_agrees_with_plain_handle_and_oracle(built, tmp_path):
    n_frames = 11
    eo, frames, frusta_o, frusta_p, map_pts, map_desc, cap_map, ids = _scene(n_frames, seed=4)
    rec = np.zeros(len(map_pts), np.dtype([("wp", O.WP_DTYPE), ("d", np.uint8, 32)]))
    rec["wp"], rec["d"] = map_pts, map_desc
    (tmp_path / "g.raw").write_bytes(frames.tobytes())
    (tmp_path / "w.bin").write_bytes(rec.tobytes())
    (tmp_path / "f.bin").write_bytes(b"".join(bytes(f) for f in frusta_p))
    (tmp_path / "i.bin").write_bytes(np.ascontiguousarray(ids, np.int32).tobytes())
    out = subprocess.check_output([build_program(), str(W), str(H), str(n_frames), str(tmp_path / "g.raw"), str(tmp_path / "w.bin"),
                                   str(len(map_pts)), str(tmp_path / "f.bin"), str(tmp_path / "i.bin"), str(ids.shape[1]), "0,0"],
                                  timeout=300).decode()
    m = re.search(r"pool_cpp members=2 member_frames=(\S+) extract_same=1 track_same=1 matches=(\S+) rc=0", out)
    assert m, out
    assert m.group(1) == "12,10"  # extract + track, 6 + 5 frames each
    counts = [int(v) for v in m.group(2).split(",")]
    for f in range(n_frames):
        _, _, _, _, n_o, _, _ = oracle_frame(eo, frames[f], frusta_o[f], ids[f], map_pts, map_desc, 20.0, 0.85)
        assert counts[f] == n_o, f
    assert sum(counts) > 80 * n_frames

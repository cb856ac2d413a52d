"""Host frames in, host results out: frames/s of the multi-device pool (orbfe_pool_*) against one ring (orbfe_stream_*).

Forms, each for extract only and for extract + isInFrustum + SearchByProjection (1000 local map points per frame by id out
of a map resident in HBM):
  ring    one handle, one ring of 3 slots x 64 frames, driven as bench.py drives it for value_host_io / value_host_io_match:
          pinned frames, the ring kept full, every collected slot copied into arrays of the caller;
  pool    orbfe_pool_extract / orbfe_pool_track with 1024 and 4096 frames per call, same slots, on {0}, {0, 0} and, on a box
          with N > 1 GPUs, {0 .. N-1}.  The pointer, frustum and id arrays are built once, as a C caller would.
`ring` and `pool {0}` alternate (--alternations times each) so that a drift of the box shows in both.  Every form runs in a
child process of its own under its own time limit; the first child that fails ends the run.

    python tools/pool_rate.py [--alternations 3] [--out profiles/r06_pool_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)  # bench.py's default workload, euroc_752x480
SLOTS, SLOT_FRAMES = 3, 64
N_DISTINCT = 256          # distinct pinned frames; longer calls cycle over them
M = 1000                  # local map points per frame
GRID = (64, 48)
TH, NN = 20.0, 0.85
CALL_FRAMES = (1024, 4096)
RING_FRAMES = 8192        # frames per timed repetition of the ring


def setup(max_batch):
    """pinned frames, a frustum, a map of N_DISTINCT * M points that project near the frames' keypoints (the C3 recipe of
    bench.py, back-projected through the pose)"""
    import torch
    import orbfe
    from orbfe import synth
    W, H = ARGS[6], ARGS[7]
    frames = torch.from_numpy(np.stack(list(synth.stream(W, H, N_DISTINCT, index0=0)))).pin_memory().numpy()
    ex = orbfe.ORBextractor(*ARGS, device=0, max_batch=max_batch)
    res = []
    for i in range(0, N_DISTINCT, max_batch):
        res += ex.extract_batch(list(frames[i:i + max_batch]))
    F = orbfe.Frustum()
    F.rcw[0] = F.rcw[4] = F.rcw[8] = 1.0
    F.min_x, F.max_x, F.min_y, F.max_y = 0.0, float(W), 0.0, float(H)
    F.fx = F.fy = 458.0
    F.cx, F.cy, F.mbf = 0.5 * W, 0.5 * H, 40.0
    F.log_scale_factor, F.n_levels, F.camera_model = float(np.log(np.float32(1.2))), ARGS[3], 0
    rng = np.random.default_rng(99)
    pts = np.zeros((N_DISTINCT, M), orbfe.WP_DTYPE)
    mpd = np.zeros((N_DISTINCT, M, 32), np.uint8)
    for b, (kp, desc, _) in enumerate(res):
        src = rng.integers(0, max(len(kp), 1), M)
        px = kp["x"][src] + rng.uniform(-3, 3, M).astype(np.float32)
        py = kp["y"][src] + rng.uniform(-3, 3, M).astype(np.float32)
        level = np.minimum(kp["octave"][src], ARGS[3] - 1)
        d = desc[src].copy()
        nflip = rng.integers(0, 21, M)
        for j in range(20):
            act = np.nonzero(j < nflip)[0]
            pos = rng.integers(0, 256, len(act))
            np.bitwise_xor.at(d, (act, pos >> 3), (1 << (pos & 7)).astype(np.uint8))
        mpd[b] = d
        z = rng.uniform(2.0, 8.0, M)
        x, y = (px - F.cx) / F.fx * z, (py - F.cy) / F.fy * z
        pts[b]["x"], pts[b]["y"], pts[b]["z"] = x, y, z
        dist = np.sqrt(x * x + y * y + z * z)
        pts[b]["max_distance"] = dist * 1.2 ** (level - 0.5)
        pts[b]["min_distance"] = pts[b]["max_distance"] / 1.2 ** (ARGS[3] - 1)
        pts[b]["observations"] = rng.integers(0, 4, M)
    ids = np.arange(N_DISTINCT * M, dtype=np.int32).reshape(N_DISTINCT, M)
    return ex, frames, F, pts.reshape(-1), mpd.reshape(-1, 32), ids


def best_of(fn, frames_per_call, reps=3):
    """frames/s of the fastest of `reps` timed repetitions, each of enough calls for >= 8192 frames"""
    fn()  # warm: every slot used, result arrays touched
    calls = max(1, 8192 // frames_per_call)
    best = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        best = max(best, calls * frames_per_call / (time.perf_counter() - t0))
    return best


def run_ring():
    import orbfe
    ex, frames, F, pts, mpd, ids = setup(SLOT_FRAMES)
    W, H = ARGS[6], ARGS[7]
    chunks = [(i, SLOT_FRAMES) for i in range(0, N_DISTINCT, SLOT_FRAMES)] * (RING_FRAMES // N_DISTINCT)
    out = {}

    st = ex.stream(slots=SLOTS, slot_frames=SLOT_FRAMES)

    def extract():
        pos = 0
        while pos < len(chunks) or st.in_flight():
            while pos < len(chunks) and st.submit(frames[chunks[pos][0]:chunks[pos][0] + SLOT_FRAMES]):
                pos += 1
            st.collect_raw()

    out["extract_fps"] = best_of(extract, RING_FRAMES)
    st.close()
    mp = orbfe.MapPoints(ex, len(pts))
    mp.update(np.arange(len(pts)), pts, mpd)
    st = ex.stream(slots=SLOTS, slot_frames=SLOT_FRAMES)
    st.enable_track(mp, M, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
    frusta = (orbfe.Frustum * SLOT_FRAMES)(*([F] * SLOT_FRAMES))

    def track():
        pos = 0
        while pos < len(chunks) or st.in_flight():
            while pos < len(chunks):
                lo = chunks[pos][0]
                if not st.submit_track(frames[lo:lo + SLOT_FRAMES], frusta, ids[lo:lo + SLOT_FRAMES], TH, NN):
                    break
                pos += 1
            st.collect_track_raw()

    out["track_fps"] = best_of(track, RING_FRAMES)
    st.close()
    mp.close()
    return out


def run_pool(devices):
    import orbfe
    ex, frames, F, pts, mpd, ids = setup(SLOT_FRAMES)
    W, H = ARGS[6], ARGS[7]
    ex.close()
    pool = orbfe.Pool(ARGS, devices, slots=SLOTS, slot_frames=SLOT_FRAMES, max_batch=SLOT_FRAMES)
    L, cap, nl = pool.L, pool.cap, pool.nlevels
    nmax = max(CALL_FRAMES)
    ptrs = (C.c_void_p * nmax)(*[frames[i % N_DISTINCT].ctypes.data for i in range(nmax)])
    frusta = (orbfe.Frustum * nmax)(*([F] * nmax))
    call_ids = np.ascontiguousarray(ids[np.arange(nmax) % N_DISTINCT])
    kp = np.zeros(nmax * cap * 24, np.uint8)
    desc = np.zeros(nmax * cap * 32, np.uint8)
    n = np.zeros(nmax, np.int32)
    per = np.zeros(nmax * nl, np.int32)
    match = np.zeros(nmax * cap, np.int32)
    nm = np.zeros(nmax, np.int32)
    P = [a.ctypes.data for a in (kp, desc, n, per, match, nm)]
    out = {}
    for nf in CALL_FRAMES:
        out["extract_fps_%d" % nf] = best_of(lambda: pool._chk(L.orbfe_pool_extract(pool.h, ptrs, W, nf, *P[:4]), "orbfe_pool_extract"), nf)
    pool.enable_track(len(pts), M, GRID[0], GRID[1], 0.0, 0.0, float(W), float(H))
    pool.map_update(np.arange(len(pts)), pts, mpd)
    tp = pool.track_params(TH, NN)
    for nf in CALL_FRAMES:
        out["track_fps_%d" % nf] = best_of(lambda: pool._chk(L.orbfe_pool_track(pool.h, ptrs, W, nf, C.byref(tp), frusta, M, call_ids.ctypes.data, *P),
                                                              "orbfe_pool_track"), nf)
    out["mean_matches"] = float(nm[:nmax].mean())
    out["member_frames"] = pool.member_frames()
    pool.close()
    return out


def child(form):
    if form == "ring":
        res = run_ring()
    else:
        res = run_pool([int(d) for d in form.split("_")[1].split(",")])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_pool_rate.json"))
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    import torch
    ngpu = torch.cuda.device_count()
    plan = []
    for i in range(a.alternations):
        plan += [("ring", "ring"), ("pool {0}", "pool_0")]
    plan.append(("pool {0,0}", "pool_0,0"))
    if ngpu > 1:
        plan.append(("pool {0..%d}" % (ngpu - 1), "pool_" + ",".join(str(d) for d in range(ngpu))))
    runs = []
    for label, form in plan:
        t0 = time.time()
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form], capture_output=True, text=True, timeout=a.step_timeout)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit("%s failed with exit status %d: no further GPU steps" % (label, p.returncode))
        res = json.loads(line[0][7:])
        runs.append({"form": label, **res})
        print("%-12s %s  (%.0f s)" % (label, json.dumps(res), time.time() - t0), flush=True)
    rings = [r for r in runs if r["form"] == "ring"]
    pools = [r for r in runs if r["form"] == "pool {0}"]
    ratios = []
    for r, p in zip(rings, pools):
        ratios.append({k: p["%s_fps_%d" % (mode, nf)] / r["%s_fps" % mode]
                       for mode in ("extract", "track") for nf in CALL_FRAMES for k in ["%s_%d" % (mode, nf)]})
    doc = {
        "what": "host frames in, host results out: frames/s of one ring (orbfe_stream_*, driven as bench.py's host_io_rate / "
                "host_io_match_rate) and of orbfe_pool_extract / orbfe_pool_track; ring and pool {0} alternate",
        "workload": {"args": list(ARGS), "pinned_frames": N_DISTINCT, "map_points_per_frame": M, "grid": list(GRID), "th": TH, "nn_ratio": NN},
        "slots": SLOTS, "slot_frames": SLOT_FRAMES, "pool_frames_per_call": list(CALL_FRAMES), "ring_frames_per_rep": RING_FRAMES,
        "device_count": ngpu, "device": torch.cuda.get_device_name(0) if ngpu else None,
        "runs": runs,
        "pool0_over_ring": ratios,
        "pool0_over_ring_min": {k: min(r[k] for r in ratios) for k in ratios[0]} if ratios else {},
        "multi_gpu": "measured" if ngpu > 1 else "not measured: %d GPU visible" % ngpu,
    }
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc["pool0_over_ring_min"]))


if __name__ == "__main__":
    main()

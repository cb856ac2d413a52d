#!/usr/bin/env python3
"""Latency of orbfe_update_local_map_batch_device (Tracking::UpdateLocalMap from the resident covisibility graph, SPEC DECISION S24)
at the shape the benchmark line of the inertial chain implies: a line-shaped graph of 120 key frames x 1000 feature slots over 13 500
points, each point seen by about 6 key frames; 1000 voters a frame; 5 covisibles, 10 temporal key frames; M = 2000, which the local points exceed (the true count
is reported).  Two settings: max_local_kf = 15, what the nodes pass, which on this graph gives about 16 local key frames (the parent's
break and the temporal chain's stall end the expansion early), and max_local_kf = 28, which gives the 30 local key frames x 1000 slots
of the issue's shape.  32 distinct frames, repeated to batch = 1, 64 and 512.
Yardsticks: (a) the plain C++ restatement of tests/cpp/local_map.cpp on ONE core of this box, per frame, best of its passes -- flat
arrays and no allocation per frame, so it is friendlier to the CPU than the reference's walk over shared_ptr graphs, std::map
observations and mutexes; (b) BASELINE 3k's per-frame cost of the chain the id rows feed (printed, not measured here).
Method (BASELINE 3k's): warm-up, then medians of `reps` calls on the host clock from the enqueue to the end of the synchronisation and
with stream events around the launches; three alternations of GPU and host, the middle median; frame 0 and the last frame of every
batch are compared with tests/local_map_ref.py first.  No pass mark: the figures are reported.

usage: python3 tests/tools/local_map_latency.py [--reps 30] [--batches 1,64,512] [--max-local-kf 15,28]
       [--json profiles/r24_local_map_latency.json] [--git-head HEAD]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
import numpy as np  # noqa: E402

import cpp_build  # noqa: E402
import local_map_ref as R  # noqa: E402
import local_map_scenarios as S  # noqa: E402
from test_local_map_cpp import write_scene  # noqa: E402

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
CHAIN_US_PER_FRAME = dict(ORBFE_IMU_FROM_KEYFRAME=12.3, ORBFE_IMU_FROM_FRAME=31.2)   # BASELINE 3k, 512 frames


def middle(xs):
    return float(sorted(xs)[len(xs) // 2])


def scene(max_local_kf, distinct=32):
    return S.random_scene(seed=24, n_kf=120, kf_stride=1000, n_points=13500, window=1500, n_frames=distinct, n_voters=1000, vote_stride=1024,
                          M=2000, max_local_kf=max_local_kf, n_covisible=5, n_temporal=10, inertial=1, mark_voters_seen=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--batches", default="1,64,512")
    ap.add_argument("--max-local-kf", default="15,28")
    ap.add_argument("--git-head", default=None, help="recorded in _meta when the tree is not a git checkout")
    a = ap.parse_args()
    import torch
    import orbfe
    rows = []
    for max_local_kf in [int(v) for v in a.max_local_kf.split(",")]:
        sc = scene(max_local_kf)
        nd, M, stride = len(sc.frames), sc.M, 1024
        want = [sc.ref(f) for f in range(nd)]
        shape = dict(local_kfs_mean=float(np.mean([w["n_local_kfs"] for w in want])), local_points_mean=float(np.mean([w["n_local_points"] for w in want])),
                     walk_slots_mean=float(np.mean([sum(len(sc.g.points[s]) for s in w["local_kfs"][:w["n_local_kfs"]]) for w in want])),
                     observations_per_voter=float(np.mean([len(sc.g.obs[p]) for v, _ in sc.frames for p in v if 0 <= p < sc.g.capacity])))
        print("scene:", shape, flush=True)
        scene_path = os.path.join(ROOT, "tests", "cpp", "local_map_latency_scene.bin")
        write_scene(scene_path, sc)
        prog = cpp_build.build("local_map", opt="-O3")

        def host_ns():
            pin = ["taskset", "-c", "0"] if shutil.which("taskset") else []
            return json.loads(subprocess.check_output(pin + [prog, "time", scene_path, "20"]).decode())["host_ns_per_frame"]

        ex = orbfe.ORBextractor(*ARGS)
        mp, cv = S.upload(orbfe, ex, sc)
        st = torch.cuda.Stream()
        par = orbfe.LocalMapParams(**sc.params)
        for B in [int(v) for v in a.batches.split(",")]:
            votes = np.full((B, stride), -1, np.int32)
            for b in range(B):
                votes[b, :1000] = sc.frames[b % nd][0]
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
            full = lambda n: torch.full((n,), -77, dtype=torch.int32, device="cuda")   # noqa: E731
            d_votes, d_n = dev(votes), dev(np.full(B, 1000, np.int32))
            d_last = dev(np.array([sc.frames[b % nd][1] for b in range(B)], np.int32))
            d_ids, d_np, d_kfs, d_nk = full(B * M), full(B), full(B * R.LOCAL_KF_MAX), full(B)
            io = orbfe.LocalMapIO(d_vote_ids=d_votes.data_ptr(), d_n_votes=d_n.data_ptr(), d_last_kf=d_last.data_ptr(), d_ids_out=d_ids.data_ptr(),
                                  d_n_local_points=d_np.data_ptr(), d_local_kfs=d_kfs.data_ptr(), d_n_local_kfs=d_nk.data_ptr(), d_vote_ids_out=None)

            def call():
                orbfe.update_local_map_batch_device(ex, par, B, stride, cv, M, io, st.cuda_stream)
            call()
            st.synchronize()
            ids, kfs, npts = d_ids.cpu().numpy().reshape(B, M), d_kfs.cpu().numpy().reshape(B, R.LOCAL_KF_MAX), d_np.cpu().numpy()
            for b in (0, B - 1):
                w = want[b % nd]
                assert np.array_equal(ids[b], w["ids"]) and np.array_equal(kfs[b], w["local_kfs"]) and int(npts[b]) == w["n_local_points"], b

            def timed():
                ts, ev = [], []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record(st)
                    call()
                    e1.record(st)
                    st.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e6)
                    ev.append(e0.elapsed_time(e1) * 1e3)
                return float(np.median(ts)), float(np.median(ev))
            for _ in range(5):
                call()
            st.synchronize()
            wall, events, host = [], [], []
            for _ in range(3):
                w_, e_ = timed()
                wall.append(w_)
                events.append(e_)
                host.append(host_ns() / 1e3)
            row = dict(entry="orbfe_update_local_map_batch_device", max_local_kf=max_local_kf, scene=shape, batch=B, size="%d frames x 1000 voters x M = %d" % (B, M),
                       wall_us=middle(wall), events_us=middle(events), wall_us_per_frame=middle(wall) / B, events_us_per_frame=middle(events) / B,
                       host_one_core_us_per_frame=middle(host), host_over_gpu_per_frame=middle(host) / (middle(wall) / B),
                       wall_runs_us=wall, events_runs_us=events, host_runs_us_per_frame=host, chain_us_per_frame_baseline_3k=CHAIN_US_PER_FRAME)
            rows.append(row)
            print("max_local_kf %2d   batch %4d   wall %9.1f us (events %9.1f)   per frame %8.2f us (events %8.2f)   host restatement, one core %8.2f us a frame   "
                  "x%.2f   runs wall %s events %s host %s" % (max_local_kf, B, row["wall_us"], row["events_us"], row["wall_us_per_frame"], row["events_us_per_frame"],
                                                               row["host_one_core_us_per_frame"], row["host_over_gpu_per_frame"],
                                                               ["%.1f" % x for x in wall], ["%.1f" % x for x in events], ["%.2f" % x for x in host]),
                  flush=True)
        cv.close()
        mp.close()
        ex.close()
        os.remove(scene_path)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/local_map_latency.py"), host_cpus=os.cpu_count(), reps=a.reps,
                           rows=rows), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

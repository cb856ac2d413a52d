#!/usr/bin/env python3
"""Latency of inserting one key frame into the resident covisibility graph (SPEC DECISION S25): 1000 feature slots, every slot a map
point, connected to 20 and to 100 neighbours (each neighbour shares 1000 / N points with the new key frame; min_weight = 1000 / N, so
every one of them is connected, gets the reciprocal AddConnection and has its head re-sorted).
 (a) the path before S25: the plain C++ restatement of tests/cpp/covis_update.cpp computes ProcessNewKeyFrame's observations and
     UpdateConnections on the host (flat arrays, friendlier to the CPU than the reference's pointer graph) and pushes every key frame
     and point it touched through orbfe_covis_set_keyframes + orbfe_covis_set_observations (`push` mode: host clock around one pass);
 (b) orbfe_covis_add_keyframe_device + orbfe_covis_update_connections_device on one stream, and the download of the ordered list;
     host clock from the first enqueue to the end of the download, called through ctypes (a few microseconds of Python are in it).
     The graph is put back to its initial state before every pass, outside the clock.
Both on the same box in the same run, alternated three times; the middle of the three medians is reported.  (b) is checked against
tests/covis_update_ref.py first.  No pass mark: the figures are reported.

usage: python3 tests/tools/covis_update_latency.py [--reps 30] [--neighbours 20,100] [--json profiles/r25_covis_update_latency.json]"""
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

import covis_update_ref as U  # noqa: E402
import covis_update_scenarios as S  # noqa: E402
import cpp_build  # noqa: E402
from test_covis_update_cpp import write_scene  # noqa: E402

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
SLOTS = 1000


def middle(xs):
    return float(sorted(xs)[len(xs) // 2])


def scene(n):
    b = S.Builder(n + 1, SLOTS, kf_stride=SLOTS, obs_stride=8, child_stride=8, conn_stride=128)
    for s in range(1, n + 1):
        b.kf(s, s)
    for i in range(SLOTS):
        b.share([1 + i % n], 1)
    return S.Scene(b.done(), [S.add(0, n + 1, np.arange(SLOTS), prev=n), S.update(0, [1], min_weight=SLOTS // n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--neighbours", default="20,100")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import orbfe
    prog = cpp_build.build("covis_update", opt="-O3")
    rows = []
    for n in [int(v) for v in a.neighbours.split(",")]:
        sc = scene(n)
        cg, g = sc.cg, sc.cg.g
        want, after = sc.trace()
        assert want[1]["count"] == n and want[0]["status"] == want[1]["status"] == 0
        path = os.path.join(ROOT, "tests", "cpp", "covis_update_latency_scene.bin")
        write_scene(path, sc)
        ex = orbfe.ORBextractor(*ARGS)
        mp, cv = S.upload(orbfe, ex, cg)
        add, upd = sc.ops[0][1], sc.ops[1][1]
        touched = list(range(1, n + 1))
        d_ids = torch.from_numpy(np.ascontiguousarray(add["point_ids"], np.int32)).cuda()
        d_added, d_status = torch.zeros(SLOTS, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        d_s, d_w = (torch.zeros(cg.conn_stride, dtype=torch.int32, device="cuda") for _ in range(2))
        d_n, d_st = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        io = orbfe.CovisUpdateIO(d_slots=d_s.data_ptr(), d_weights=d_w.data_ptr(), d_count=d_n.data_ptr(), d_status=d_st.data_ptr())
        par = orbfe.CovisUpdateParams(upd["min_weight"])
        st = torch.cuda.Stream()
        empty = (np.arange(n + 1, dtype=np.int32), np.zeros(n + 2, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))

        def reset():
            cv.set_keyframes([g.record(s, with_points=False) for s in touched])
            cv.set_observations(*g.observations_csr(list(range(SLOTS))))
            cv.set_connections(*empty)

        def one_pass():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cv.add_keyframe_device(add["slot"], add["mn_id"], d_ids.data_ptr(), SLOTS, d_added.data_ptr(), d_status.data_ptr(), prev=add["prev"],
                                   stream=st.cuda_stream)
            cv.update_connections_device(upd["slots"], upd["flags"], io, par, st.cuda_stream)
            with torch.cuda.stream(st):
                out = (d_s.cpu(), d_w.cpu(), d_n.cpu())
            st.synchronize()
            return (time.perf_counter() - t0) * 1e6, out

        reset()
        _, out = one_pass()
        assert np.array_equal(out[0].numpy(), want[1]["slots"]) and np.array_equal(out[1].numpy(), want[1]["weights"]) and int(out[2]) == n
        assert int(d_status.cpu()) == 0 and np.array_equal(d_added.cpu().numpy(), want[0]["added"])
        for s in (0, 1, n):
            assert cv.get_keyframe(s) == after.keyframe(s), s

        def device_us():
            ts = []
            for _ in range(a.reps + 3):
                reset()
                ts.append(one_pass()[0])
            return middle(ts[3:])

        def push():
            return json.loads(subprocess.check_output([prog, "push", path, str(a.reps)]).decode())

        pa, pb, info = [], [], None
        for _ in range(3):
            info = push()
            pa.append(info["push_us_median"])
            pb.append(device_us())
        row = dict(neighbours=n, feature_slots=SLOTS, host_push_us=middle(pa), device_us=middle(pb), ratio_device_over_host=middle(pb) / middle(pa),
                   host_push_us_all=pa, device_us_all=pb, touched_kfs=info["touched_kfs"], touched_points=info["touched_points"], reps=a.reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
        cv.close()
        mp.close()
        ex.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows, _meta=dict(tool="tests/tools/covis_update_latency.py", launches_per_key_frame=5)), f, indent=1)


if __name__ == "__main__":
    main()

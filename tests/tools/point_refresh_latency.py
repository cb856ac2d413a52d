#!/usr/bin/env python3
"""Latency of refreshing 1000 map points from the resident graph (SPEC DECISION S26): UpdateDepth + ComputeDistinctiveDescriptors for
1000 points with 8 and with 40 observers each (the sizes of the SearchInNeighbors loop, src/LocalMapping.cc:866-867), 200 key frames of
1000 features.
 (a) the path before S26 for the same result: on one core, numpy gathers every point's observed descriptors from host copies of the key
     frames' descriptor matrices into one CSR block and computes the depth, orbfe_distinctive_descriptors selects, and the new records
     go up through orbfe_map_update; host clock around the three steps (the gather is vectorised, friendlier to the CPU than the
     reference's walk over std::map nodes);
 (b) one orbfe_covis_refresh_points_device call on a stream of its own with the id list already in HBM; host clock from the enqueue to
     the end of the stream, called through ctypes (a few microseconds of Python are in it).
Both on the same machine in the same run, alternated three times; the middle of the three medians and the range of all passes are
reported.  (b) is checked against tests/point_refresh_ref.py first, (a) against (b).  Also reported: the device time (events) of a call
whose list names one point outside the map -- both launches with nothing to do, an upper bound on what the rest-list launch costs when
its list is empty.  No pass mark: the figures are reported.

usage: python3 tests/tools/point_refresh_latency.py [--reps 30] [--observers 8,40] [--json profiles/r26_point_refresh_latency.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
import numpy as np  # noqa: E402

import point_refresh_ref as P  # noqa: E402
import point_refresh_scenarios as S  # noqa: E402

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
POINTS = 1000
FIELDS = ("status", "min_distance", "max_distance", "best_slot", "best_index", "best_median")


def middle(xs):
    return float(sorted(xs)[len(xs) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--observers", default="8,40")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import orbfe
    rows = []
    for n_obs in [int(v) for v in a.observers.split(",")]:
        rg = S.uniform_graph(POINTS, n_obs)
        g = rg.g
        want_rg = S.clone(rg)
        want = P.refresh_points(want_rg, np.arange(POINTS), 3)
        ex = orbfe.ORBextractor(*ARGS)
        mp, cv = S.upload(orbfe, ex, rg)
        matcher = orbfe.ORBmatcher(ex)
        d_ids = torch.arange(POINTS, dtype=torch.int32, device="cuda")
        bufs = {k: torch.zeros(POINTS, dtype=torch.float32 if "distance" in k else torch.int32, device="cuda") for k in FIELDS}
        io = orbfe.RefreshIO(**{"d_" + k: bufs[k].data_ptr() for k in FIELDS})
        st = torch.cuda.Stream()

        def device_pass(n=POINTS, ids=d_ids):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cv.refresh_points_device(n, ids.data_ptr(), 3, io, None, 0, st.cuda_stream)
            st.synchronize()
            return (time.perf_counter() - t0) * 1e6

        device_pass()
        for k in FIELDS:
            assert bufs[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        assert S.read_state(cv, want_rg, range(0, POINTS, 37)) == S.state(want_rg, range(0, POINTS, 37))

        # the host's own copies, as the mapping thread holds them
        kf_desc = np.stack([rg.desc[s] for s in range(g.kf_capacity)])                 # [K][stride][32]
        kf_oct = np.stack([rg.octave[s] for s in range(g.kf_capacity)])
        obs = np.array(g.obs, np.int64)                                                # [POINTS][n_obs]
        idx = np.array(rg.obs_idx, np.int64)
        off = np.arange(POINTS + 1, dtype=np.int32) * n_obs
        ref_idx = idx[:, 0]                                                            # uniform_graph: the reference key frame is the first observer
        pts = np.zeros(POINTS, orbfe.WP_DTYPE)
        pts["x"], pts["y"], pts["z"] = rg.pos.T
        pts["observations"] = n_obs
        all_ids = np.arange(POINTS, dtype=np.int32)
        # the selection's tie rule is the lowest mn_id: gathered in ascending mn_id (here mn_id == slot)
        order = np.argsort(obs, axis=1, kind="stable")
        obs_s, idx_s = np.take_along_axis(obs, order, 1), np.take_along_axis(idx, order, 1)

        def host_pass():
            t0 = time.perf_counter()
            desc = kf_desc[obs_s.ravel(), idx_s.ravel()]                               # the gather
            d = rg.pos - rg.centre[rg.ref]
            dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            mx = dist * rg.sf[kf_oct[rg.ref, ref_idx]]
            pts["max_distance"], pts["min_distance"] = mx, mx / rg.sf[-1]
            best, median = matcher.ComputeDistinctiveDescriptors(off, desc)
            mp.update(all_ids, pts, desc[off[:-1] + best])
            return (time.perf_counter() - t0) * 1e6, best, median

        _, best, median = host_pass()
        rows_of = np.arange(POINTS)
        assert np.array_equal(obs_s[rows_of, best], want["best_slot"]) and np.array_equal(median, want["best_median"])
        assert S.read_state(cv, want_rg, range(0, POINTS, 37)) == S.state(want_rg, range(0, POINTS, 37))   # the same records either way

        da, ha = [], []
        for _ in range(3):
            ha.append([host_pass()[0] for _ in range(a.reps + 3)][3:])
            da.append([device_pass() for _ in range(a.reps + 3)][3:])
        # both launches with nothing to do
        d_none = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps + 3)]
        for e0, e1 in ev:
            with torch.cuda.stream(st):
                e0.record()
                cv.refresh_points_device(1, d_none.data_ptr(), 3, io, None, 0, st.cuda_stream)
                e1.record()
        st.synchronize()
        idle = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev][3:]
        flat = lambda xs: [v for x in xs for v in x]   # noqa: E731
        row = dict(points=POINTS, observers=n_obs, host_us=middle([middle(x) for x in ha]), device_us=middle([middle(x) for x in da]),
                   host_us_range=[min(flat(ha)), max(flat(ha))], device_us_range=[min(flat(da)), max(flat(da))],
                   host_us_medians=[middle(x) for x in ha], device_us_medians=[middle(x) for x in da],
                   both_launches_idle_device_us=middle(idle), both_launches_idle_device_us_range=[min(idle), max(idle)], reps=a.reps)
        row["ratio_device_over_host"] = row["device_us"] / row["host_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        cv.close()
        mp.close()
        ex.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=rows, _meta=dict(tool="tests/tools/point_refresh_latency.py", launches_per_call=2)), f, indent=1)


if __name__ == "__main__":
    main()

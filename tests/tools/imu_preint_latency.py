#!/usr/bin/env python3
"""Latency of the S22 calls (IMU preintegration, state prediction, the inertial link) next to the host loop they relieve, on ONE box
(the `moving` scene of tests/imu_preint_scenarios.py):
  * the single calls -- orbfe_imu_preintegrate_frame followed by orbfe_imu_predict, two launches and two synchronisations -- at 10 and
    40 steps and the single-thread host loop of the same text (-O2, one pinned core), all from tests/cpp/imu_preint.cpp: three runs of
    the program, the middle of the three medians of `reps` calls; the program first checks that calls and host loop agree bit for bit;
  * orbfe_imu_frame_batch_device at 512 frames x 10 steps (32 distinct scenes, repeated, each with its own record, bias and start),
    for either link kind, timed with stream events around `reps` launches after a warm-up, three alternations, the middle median;
  * the bytes that go up per frame: before (one host-built link and the 33-float state) and after (the samples, the two stamps, the
    frame's bias, the start state and one offset; the key-frame record stays in HBM).
There is no acceptance ratio: the figures are reported.

usage: python3 tests/tools/imu_preint_latency.py [--reps 200] [--json profiles/r22_imu_preint_latency.json] [--git-head HEAD]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
import numpy as np  # noqa: E402

import imu_preint_ref as R  # noqa: E402
import imu_preint_scenarios as PS  # noqa: E402
import test_imu_preint_cpp as TC  # noqa: E402

LINK_SIZE = {R.FROM_KEYFRAME: 216 + 99 * 8, R.FROM_FRAME: 424 + 99 * 8}
NAME = {R.FROM_KEYFRAME: "ORBFE_IMU_FROM_KEYFRAME", R.FROM_FRAME: "ORBFE_IMU_FROM_FRAME"}


def single_rows(reps, tmp):
    rows = []
    exe = TC._build()
    for n in (10, 40):
        sc = PS.make("moving", n, 0)
        scene, out = os.path.join(tmp, "scene_%d.bin" % n), os.path.join(tmp, "out_%d.bin" % n)
        TC.write_scene(scene, sc, R.FROM_KEYFRAME)
        runs = []
        for _ in range(3):
            txt = subprocess.check_output([exe, scene, out, str(reps)], timeout=300).decode()
            lat = re.search(r"imu_preint_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) steps=(\d+) host_same=(\d)", txt)
            assert lat and lat.group(4) == "1" and int(lat.group(3)) == n, txt
            runs.append((float(lat.group(1)), float(lat.group(2))))
        call, host = (sorted(x[i] for x in runs)[1] for i in range(2))
        rows.append(dict(entry="orbfe_imu_preintegrate_frame + orbfe_imu_predict", reference="Tracking.cc:234-350", size="%d steps" % n,
                         call_us=call, host_one_thread_us=host, ratio=host / call, runs_us=runs))
        print("%2d steps   calls %8.1f us   host 1 thread %8.1f us   x%.2f" % (n, call, host, host / call), flush=True)
    return rows


def batch_rows(reps, host_us, B=512, n=10, distinct=32):
    import torch
    import orbfe
    scs = [PS.make("moving", n, s) for s in range(distinct)]
    scs = [scs[b % distinct] for b in range(B)]
    off = np.cumsum([0] + [len(sc["t"]) for sc in scs]).astype(np.int32)
    smp = np.concatenate([TC.samples_of(sc) for sc in scs])
    recs = np.zeros((B, 300), np.float32)
    for b, sc in enumerate(scs):
        recs[b, :2].view(np.int32)[:] = (1200, sc["kf"].n_steps)
        recs[b, 2:] = sc["kf"].floats()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_smp, d_tp, d_tc, d_fb = (dev(a) for a in (smp, np.array([sc["t_prev"] for sc in scs]), np.array([sc["t_cur"] for sc in scs]),
                                                np.stack([sc["frame_bias"] for sc in scs]).astype(np.float32)))
    d_fr = torch.zeros(B * 1200, dtype=torch.uint8, device="cuda")
    d_state = torch.zeros(B * 33, dtype=torch.float32, device="cuda")
    d_ok = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    noise = orbfe.ImuNoise(scs[0]["noise"].cov, scs[0]["noise"].walk)
    st = torch.cuda.Stream()
    out = []
    for which in (R.FROM_KEYFRAME, R.FROM_FRAME):
        par = orbfe.ImuPredictParams(which, scs[0]["gravity"], scs[0]["Rcb"], scs[0]["tcb"], scs[0]["tbc"])
        d_s1 = dev(np.stack([sc["state_frame"] if which == R.FROM_FRAME else sc["state_kf"] for sc in scs]).astype(np.float32))
        d_links = torch.zeros(B * LINK_SIZE[which], dtype=torch.uint8, device="cuda")
        d_kf0 = dev(recs)
        d_kf = d_kf0.clone()
        torch.cuda.synchronize()

        def launch():
            orbfe.imu_frame_batch_device(ex, noise, par, B, d_smp.data_ptr(), off, d_tp.data_ptr(), d_tc.data_ptr(), d_fb.data_ptr(),
                                         d_s1.data_ptr(), d_kf.data_ptr(), d_fr.data_ptr(), None, d_state.data_ptr(), d_links.data_ptr(),
                                         d_ok.data_ptr(), st.cuda_stream)
        launch()
        st.synchronize()
        want = PS.ref_cached(("moving", n, 0), which)
        assert want["state"].tobytes() == d_state.cpu().numpy().reshape(B, 33)[0].tobytes(), "batch frame 0 differs from the restatement"
        assert d_links.cpu().numpy().tobytes()[:LINK_SIZE[which]] == TC.link_bytes(want["link"], which)
        meds = []
        for _ in range(3):
            ts = []
            for _ in range(reps):
                d_kf.copy_(d_kf0)   # the record is integrated in place: every timed launch starts from the same one
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record(st)
                launch()
                b.record(st)
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            meds.append(float(np.median(ts)))
        launch_us = sorted(meds)[1]
        out.append(dict(entry="orbfe_imu_frame_batch_device", which=NAME[which], size="%d frames x %d steps" % (B, n), launch_us=launch_us,
                        per_frame_us=launch_us / B, host_one_thread_us_per_frame=host_us, ratio=host_us / (launch_us / B), medians_us=meds))
        print("batch %d x %d %-24s launch %9.1f us   per frame %7.2f us   host 1 thread %8.1f us per frame   x%.1f" % (
            B, n, NAME[which], launch_us, launch_us / B, host_us, out[-1]["ratio"]), flush=True)
    ex.close()
    return out


def upload_bytes(n):
    """per frame: what a caller of the S19 / S20 batch calls uploaded before, and what it uploads now"""
    state = 33 * 4
    before = {NAME[w]: LINK_SIZE[w] + state for w in LINK_SIZE}
    after = (n + 1) * 32 + 2 * 8 + 6 * 4 + 21 * 4 + 4
    return dict(steps=n, before_link_and_state=before, after_samples_stamps_bias_start_offset=after)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--git-head", default=None, help="recorded in _meta when the tree is not a git checkout")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="imu_preint_latency_")
    rows = single_rows(a.reps, tmp)
    rows += batch_rows(a.reps, rows[0]["host_one_thread_us"])
    shutil.rmtree(tmp, ignore_errors=True)
    up = [upload_bytes(10), upload_bytes(40)]
    for u in up:
        print("upload per frame at %d steps: before %s bytes, after %d bytes" % (u["steps"], u["before_link_and_state"],
                                                                               u["after_samples_stamps_bias_start_offset"]))
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/imu_preint_latency.py"), host_cpus=os.cpu_count(), reps=a.reps,
                           rows=rows, upload_bytes_per_frame=up), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

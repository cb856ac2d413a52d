#!/usr/bin/env python3
"""Latency of orbfe_pose_inertial_optimization_last_frame (SPEC DECISION S20) next to the host loop it relieves and next to S19's call,
on ONE box (the `general` scene of tests/pose_inertial_prev_scenarios.py at the reference's constants: 4 rounds of 15 Gauss-Newton
iterations on 30 unknowns):
  * the single call at N_e = 100, 300, 1000 and 3000, the same call without the marginalisation (Hprior_out == NULL: the epilogue's
    share is the difference) and the single-thread host loop of S20 (-O2, one pinned core), all from tests/cpp/pose_inertial_prev.cpp:
    three runs of the program, the middle of the three medians of `reps` calls; the program first checks that call and host loop agree
    bit for bit;
  * S19's single call and host loop at the same N_e, from tests/tools/pose_inertial_latency.py in the same process (S19's kernel is the
    parent's, untouched);
  * the batch call at 512 frames x 300 edges (32 distinct scenes, repeated, each with its own link, prior and state) with and without
    d_Hprior_out, timed with stream events around `reps` launches after a warm-up, three alternations, the middle median; and S19's batch.
There is no acceptance ratio: the figures are reported.

usage: python3 tests/tools/pose_inertial_prev_latency.py [--reps 200] [--json profiles/r21_pose_inertial_prev_latency.json] [--git-head HEAD]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
import numpy as np  # noqa: E402

import pose_inertial_latency as L19  # noqa: E402
import pose_inertial_prev_scenarios as PS  # noqa: E402
import test_pose_inertial_prev_cpp as TC  # noqa: E402

ENTRY = "orbfe_pose_inertial_optimization_last_frame"


def single_rows(reps, tmp):
    rows = []
    exe = TC._build()
    for N in (100, 300, 1000, 3000):
        sc = PS.make("general", N, 0)
        scene, out = os.path.join(tmp, "scene_%d.bin" % N), os.path.join(tmp, "out_%d.bin" % N)
        TC.write_scene(scene, sc)
        runs = []
        for _ in range(3):
            txt = subprocess.check_output([exe, scene, out, str(reps)], timeout=300).decode()
            lat = re.search(r"pose_inertial_prev_latency_us call=([0-9.]+) call_without_marginalisation=([0-9.]+) host_one_thread=([0-9.]+) "
                            r"host_same=(\d)", txt)
            assert lat and lat.group(4) == "1", txt
            runs.append(tuple(float(lat.group(i)) for i in (1, 2, 3)))
        r = TC.read_result(out, len(sc["kp_xy"]))
        call, bare, host = (sorted(x[i] for x in runs)[1] for i in range(3))
        rows.append(dict(entry=ENTRY, reference="Optimizer.cc:3846-4275", size="N_e=%d" % N, iterations=r["round_iterations"].tolist(),
                         call_us=call, call_without_marginalisation_us=bare, epilogue_us=call - bare, host_one_thread_us=host,
                         ratio=host / call, runs_us=runs))
        print("N_e=%-5d iterations %s   call %8.1f us (without the marginalisation %8.1f us)   host 1 thread %8.1f us   x%.2f" % (
            N, r["round_iterations"].tolist(), call, bare, host, host / call), flush=True)
    return rows


def batch_rows(reps, host_us_300, B=512, N=300, distinct=32):
    import torch
    import orbfe
    scs = [PS.make("general", N, s) for s in range(distinct)]
    stride = max(len(sc["kp_xy"]) for sc in scs)
    M = max(len(sc["points"]) for sc in scs)
    kp = np.zeros((B, stride), orbfe.KP_DTYPE)
    match = np.full((B, stride), -1, np.int32)
    pts = np.zeros((B, M), orbfe.WP_DTYPE)
    depth = np.zeros((B, M), np.float32)
    state = np.zeros((B, 33), np.float32)
    n = np.zeros(B, np.int32)
    links, priors = [], []
    for b in range(B):
        sc = scs[b % distinct]
        k = len(sc["kp_xy"])
        n[b] = k
        kp[b, :k]["x"], kp[b, :k]["y"], kp[b, :k]["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
        match[b, :k] = sc["mp_index"]
        pts[b, :len(sc["points"])]["x"], pts[b, :len(sc["points"])]["y"], pts[b, :len(sc["points"])]["z"] = sc["points"].T
        depth[b, :len(sc["points"])] = sc["track_depth"]
        state[b] = TC.state_in(sc)
        body = TC.link_bytes(sc["link"])
        links.append(np.array([len(body) + 8, 0], np.int32).tobytes() + body)
        body = TC.prior_bytes(sc["prior"])
        priors.append(np.array([len(body) + 8, 0], np.int32).tobytes() + body)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    d_kp, d_match, d_pts, d_depth, d_state, d_n = (dev(a) for a in (kp, match, pts, depth, state, n))
    d_links, d_priors = dev(np.frombuffer(b"".join(links), np.uint8)), dev(np.frombuffer(b"".join(priors), np.uint8))
    d_out = torch.zeros(B * 21, dtype=torch.float32, device="cuda")
    d_H = torch.zeros(B * 900, dtype=torch.float64, device="cuda")
    d_Hp = torch.zeros(B * 225, dtype=torch.float64, device="cuda")
    d_outl = torch.zeros(B * stride, dtype=torch.uint8, device="cuda")
    d_ninl = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_acc = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    prm = orbfe.PoseInertialPrevParams(scs[0]["cam"])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def launch(with_prior):
        orbfe.pose_inertial_optimization_last_frame_batch_device(
            ex, prm, B, d_links.data_ptr(), d_priors.data_ptr(), d_kp.data_ptr(), d_n.data_ptr(), stride, d_match.data_ptr(), M,
            d_pts.data_ptr(), M, d_depth.data_ptr(), d_state.data_ptr(), d_out.data_ptr(), d_H.data_ptr(),
            d_Hp.data_ptr() if with_prior else None, d_outl.data_ptr(), d_ninl.data_ptr(), d_acc.data_ptr(), st.cuda_stream)
    for _ in range(5):
        launch(True)
    st.synchronize()
    want = PS.ref(scs[0])
    assert np.concatenate([want[k] for k in ("Rwb", "twb", "v", "bg", "ba")]).tobytes() == d_out.cpu().numpy().reshape(B, 21)[0].tobytes()
    assert want["Hprior"].tobytes() == d_Hp.cpu().numpy().reshape(B, 225)[0].tobytes(), "batch frame 0 differs from the restatement"
    out = []
    for with_prior in (True, False):
        meds = []
        for _ in range(3):
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                launch(with_prior)
                b.record(st)
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            meds.append(float(np.median(ts)))
        launch_us = sorted(meds)[1]
        out.append(dict(entry=ENTRY + "_batch_device", size="%d frames x N_e=%d" % (B, N), marginalisation=with_prior, launch_us=launch_us,
                        per_frame_us=launch_us / B, host_one_thread_us_per_frame=host_us_300, ratio=host_us_300 / (launch_us / B),
                        medians_us=meds))
        print("batch %d x %d %s   launch %9.1f us   per frame %7.2f us   host 1 thread %8.1f us per frame   x%.1f" % (
            B, N, "with the marginalisation   " if with_prior else "without the marginalisation", launch_us, launch_us / B, host_us_300,
            out[-1]["ratio"]), flush=True)
    ex.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--git-head", default=None, help="recorded in _meta when the tree is not a git checkout")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="pose_inertial_prev_latency_")
    rows = single_rows(a.reps, tmp)
    rows += batch_rows(a.reps, rows[1]["host_one_thread_us"])
    s19 = L19.single_rows(a.reps, tmp)
    s19.append(L19.batch_row(a.reps, s19[1]["host_one_thread_us"]))
    shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/pose_inertial_prev_latency.py"), host_cpus=os.cpu_count(),
                           reps=a.reps, rows=rows, s19_same_run=s19), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

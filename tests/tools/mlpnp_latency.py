#!/usr/bin/env python3
"""Per-call latency of orbfe_mlpnp_ransac next to the host loop it relieves, on ONE box, at N = 100, 300 and 1000 correspondences
(the `general` scene of tests/mlpnp_scenarios.py with 30 % outliers, at the call site's parameters 0.95 / 50 / 300 / 12 / 0.5 / 5.991,
iterate(20)):
  * the call's median and the single-thread host loop of SPEC DECISION S13 (-O2, one pinned core), both from tests/cpp/mlpnp.cpp:
    three runs of the program (call and host loop alternate), the middle of the three medians; the program first checks that
    the two agree bit for bit;
  * the kernels' times from a `rocprofv3 --kernel-trace` run of their own (the program after `--`), median per kernel.
There is no acceptance ratio: the parent has nothing to compare with, the host loop is the yardstick, and the figures are reported.

usage: python3 tests/tools/mlpnp_latency.py [--reps 200] [--json profiles/r13_mlpnp_latency.json] [--git-head HEAD] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import mlpnp_scenarios as MS  # noqa: E402
import test_mlpnp_cpp as TC  # noqa: E402


def kernel_medians(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        return None
    per = {}
    for r in csv.DictReader(open(files[-1])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("orbfe::", "").split("(")[0]
        if "mlpnp" in name:
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: dict(calls=len(v), median_us=float(np.median(v))) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--git-head", default=None, help="recorded in _meta when the tree is not a git checkout")
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    TC._build()
    rows = []
    tmp = tempfile.mkdtemp(prefix="mlpnp_latency_")
    for N in (100, 300, 1000):
        sc = MS.make("general", N, 0, 0.3)
        scene, out = os.path.join(tmp, "scene_%d.bin" % N), os.path.join(tmp, "out_%d.bin" % N)
        TC.write_scene(scene, sc)
        runs = []
        for _ in range(3):
            txt = subprocess.check_output([TC.BIN, scene, out, str(a.reps)], timeout=300).decode()
            lat = re.search(r"mlpnp_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_same=(\d)", txt)
            assert lat and lat.group(3) == "1", txt
            runs.append((float(lat.group(1)), float(lat.group(2))))
        head = re.search(r"mlpnp N=(\d+) total=(\d+) solved=(\d) exit=(\d) it=(-?\d+) candidates=(\d+)", txt)
        call, host = sorted(r[0] for r in runs)[1], sorted(r[1] for r in runs)[1]
        kern = None
        if not a.no_trace and shutil.which("rocprofv3"):
            tdir = os.path.join(tmp, "trace_%d" % N)
            tr = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", TC.BIN, scene, out,
                                 str(min(a.reps, 50))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
            if tr.returncode != 0:  # nothing more is started on the device after a run that ended badly
                sys.stderr.write(tr.stdout.decode(errors="replace")[-4000:])
                sys.exit("the traced run at N = %d ended with status %d" % (N, tr.returncode))
            kern = kernel_medians(tdir)
        rows.append(dict(entry="orbfe_mlpnp_ransac", reference="MLPnPsolver.cpp:56-352", size="N=%d" % N, iterations=int(head.group(2)),
                         exit_kind=int(head.group(4)), returning_iteration=int(head.group(5)), candidates=int(head.group(6)),
                         call_us=call, host_one_thread_us=host, ratio=host / call, runs_us=runs, kernels=kern))
        print("N=%-5d iterations %s candidates %s   call %8.1f us   host 1 thread %9.1f us   x%.2f   kernels %s" % (
            N, head.group(2), head.group(6), call, host, host / call, {k: round(v["median_us"], 1) for k, v in (kern or {}).items()}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/mlpnp_latency.py"), host_cpus=os.cpu_count(),
                           reps=a.reps, rows=rows), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Per-call latency of orbfe_two_view_reconstruct next to the host loop it relieves, on ONE box, at N = 150, 300 and 1000
matches (the `general` scene of tests/twoview_scenarios.py with 30 % outliers, 200 iterations):
  * the call's median and the single- / two-thread host loop of SPEC DECISION S12 (-O2, one / two pinned cores): all three
    from tests/cpp/two_view.cpp, three alternations, the middle of the three medians; the program first checks that the three
    agree bit for bit;
  * the kernels' times from a `rocprofv3 --kernel-trace` run of their own (the program after `--`), median per kernel.
Acceptance (the issue's): the call's median is below the two-thread host form at all three sizes.

usage: python3 tests/tools/twoview_latency.py [--reps 200] [--json profiles/r10_twoview_latency.json] [--git-head HEAD] [--no-trace]"""
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

import test_twoview_cpp as TC  # noqa: E402
import twoview_scenarios as TS  # noqa: E402


def kernel_medians(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        return None
    per = {}
    for r in csv.DictReader(open(files[-1])):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("orbfe::", "").split("(")[0]
        if "twoview" in name:
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
    rows, ok = [], True
    tmp = tempfile.mkdtemp(prefix="twoview_latency_")
    for N in (150, 300, 1000):
        sc = TS.make("general", N, 0, 0.3, 200)
        scene, out = os.path.join(tmp, "scene_%d.bin" % N), os.path.join(tmp, "out_%d.bin" % N)
        TC.write_scene(scene, sc)
        txt = subprocess.check_output([TC.BIN, scene, out, str(a.reps)]).decode()
        lat = re.search(r"two_view_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_two_threads=([0-9.]+) host_same=(\d)", txt)
        rounds = re.search(r"two_view_rounds_us call=(\S+) host_one_thread=(\S+) host_two_threads=(\S+)", txt)
        assert lat and lat.group(4) == "1", txt
        call, h1, h2 = (float(lat.group(i)) for i in (1, 2, 3))
        kern = None
        if not a.no_trace and shutil.which("rocprofv3"):
            tdir = os.path.join(tmp, "trace_%d" % N)
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", TC.BIN, scene, out,
                            str(min(a.reps, 50))], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
            kern = kernel_medians(tdir)
        rows.append(dict(entry="orbfe_two_view_reconstruct", reference="TwoViewReconstruction.cc:40-127", size="N=%d iterations=200" % N,
                         call_us=call, host_one_thread_us=h1, host_two_threads_us=h2, ratio_two_threads=h2 / call,
                         rounds_us=dict(call=rounds.group(1), host_one_thread=rounds.group(2), host_two_threads=rounds.group(3)),
                         kernels=kern, below_two_thread_host=call < h2))
        ok = ok and call < h2
        print("N=%-5d call %8.1f us   host 1 thread %9.1f us   host 2 threads %9.1f us   x%.1f   kernels %s" % (
            N, call, h1, h2, h2 / call, {k: round(v["median_us"], 1) for k, v in (kern or {}).items()}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/twoview_latency.py"), host_cpus=os.cpu_count(),
                           reps=a.reps, acceptance_call_below_two_thread_host=ok, rows=rows), f, indent=1)
    print("acceptance (call below the two-thread host loop at all sizes):", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

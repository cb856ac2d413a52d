#!/usr/bin/env python3
"""Latency of orbfe_initial_bundle_adjustment next to the host loop it relieves, on ONE box (the `general` scene of
tests/initial_ba_scenarios.py at the reference's constants: one Levenberg run of at most 20 iterations, Huber on):
the call through the adaptor (InitialMapAdjuster::Adjust: the device call, then the median depth and the rescale on the host) at
N = 100, 300, 1000 and 3000 and the single-thread host loop of SPEC DECISION S17 (-O2, one pinned core) with the same host step, both
from tests/cpp/initial_ba.cpp: three runs of the program (call and host loop alternate), the middle of the three medians of `reps`
calls; the program first checks that the two agree bit for bit.
There is no acceptance ratio: the parent has nothing to compare with, the host loop is the yardstick, and the figures are reported.

usage: python3 tests/tools/initial_ba_latency.py [--reps 200] [--json profiles/r18_initial_ba_latency.json] [--git-head HEAD]"""
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

import initial_ba_scenarios as BS  # noqa: E402
import test_initial_ba_cpp as TC  # noqa: E402

SIZES = (100, 300, 1000, 3000)


def rows_of(reps, tmp):
    rows = []
    exe = TC._build()
    for N in SIZES:
        sc = BS.make("general", N, 0)
        scene, out = os.path.join(tmp, "scene_%d.bin" % N), os.path.join(tmp, "out_%d.bin" % N)
        TC.write_scene(scene, sc)
        runs = []
        for _ in range(3):
            txt = subprocess.check_output([exe, scene, out, str(reps)], timeout=300).decode()
            lat = re.search(r"initial_ba_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_same=(\d)", txt)
            assert lat and lat.group(3) == "1", txt
            runs.append((float(lat.group(1)), float(lat.group(2))))
        r = TC.read_result(out, len(sc["kp1_xy"]))
        call, host = sorted(x[0] for x in runs)[1], sorted(x[1] for x in runs)[1]
        rows.append(dict(entry="orbfe_initial_bundle_adjustment", reference="Tracking.cc:698-729 / Optimizer.cc:60-369", size="N=%d" % N,
                         iterations=r["iterations"], trials=r["trials"], call_us=call, host_one_thread_us=host, ratio=host / call,
                         runs_us=runs))
        print("N=%-5d iterations %d trials %d   call %9.1f us   host 1 thread %9.1f us   x%.2f" % (
            N, r["iterations"], r["trials"], call, host, host / call), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    ap.add_argument("--git-head", default=None, help="recorded in _meta when the tree is not a git checkout")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="initial_ba_latency_")
    rows = rows_of(a.reps, tmp)
    shutil.rmtree(tmp, ignore_errors=True)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or a.git_head, tool="tests/tools/initial_ba_latency.py"), host_cpus=os.cpu_count(),
                           reps=a.reps, rows=rows), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

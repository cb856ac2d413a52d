#!/usr/bin/env python3
"""What orbfe_create_new_points_batch costs and what it gives back, on ONE box in ONE run.

Builds tests/cpp/newpoints.cpp twice -- against the shipped library, and with -DNEWPOINTS_SEARCH_ONLY against every earlier
build under tools/ab/ (liborbfe_<name>.so; a library from before the new entry points) -- and alternates the programs for
three rounds on the same scene file:

  (a) orbfe_match_triangulation_batch, K = 20 neighbours           (earlier library and shipped library)
  (b) orbfe_create_new_points_batch on the same inputs              (shipped library)
  (c) the S11 geometry as a single-thread -O2 host loop on one core over the matches the K orbfe_triangulation_select
      calls return -- what the mapping thread computes itself when it only has (a); microseconds per pair

Two scenes: "extracted" = the K = 20 / N ~ 1012 inputs of tests/tools/matcher_latency.py (a real frame's keypoints,
descriptor-only neighbours displaced along x, the pose that displacement stands for), "geometry" = the scene of
test_newpoints_gpu.py::test_whole_loop_equals_sequential_reference (K = 20, N = 1000).  Every program run takes the median of
`--reps` calls after warm-up per figure, three times alternating (a) / (b) inside the run; the JSON keeps every figure.

usage: python3 tools/newpoints_ab.py [--reps 200] [--json profiles/NAME.json]"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def build(lib_dir, lib_name, out, search_only):
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "newpoints.cpp"),
           "-o", out, "-L", lib_dir, "-l" + lib_name, "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    if search_only:
        cmd.insert(1, "-DNEWPOINTS_SEARCH_ONLY")
        cmd.insert(1, "-Wno-unused-function")
    subprocess.check_call(cmd)


def scenes(tmp):
    import __graft_entry__ as g
    g.build()
    import orbfe
    import oracle_py as O
    import newpoints_ref as R
    import newpoints_scenarios as NS
    import test_newpoints_cpp as TC
    import test_newpoints_gpu as G
    import test_triangulation_batch as TB
    from orbfe import synth
    out = {}
    # the geometry scene of the whole-loop test
    K = 20
    sc = NS.scene(3, K=K)
    has1, has2, coarse, cams = G.search_inputs(sc, sc["nbs"], 60 + K)
    TC.write_scene(os.path.join(tmp, "geometry.bin"), sc, sc["nbs"], has1, has2, G.tri_params(sc["nbs"], coarse, cams),
                   [G.np_params(nb["np"]) for nb in sc["nbs"]])
    out["geometry"] = os.path.join(tmp, "geometry.bin")
    # matcher_latency's inputs: the oracle's keypoints of a synthetic frame, TB.neighbour (x-displaced, F12 of t12 = (0.11, 0, 0))
    W, H = 752, 480
    eo = O.Extractor(1000, 40000, 1.2, 8, 20, 7, W, H)
    kp, desc, _ = eo.extract(list(synth.stream(W, H, 2))[0])
    node1 = TB.nodes_of(kp)
    nbs = [TB.neighbour(kp, desc, 500 + k, True, False) for k in range(K)]
    sf = np.asarray(eo.scaleFactors, np.float32)
    sigma2 = (sf * sf).astype(np.float32)
    T1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    T2 = np.hstack([np.eye(3), [[-0.11], [0.0], [0.0]]])
    P = R.params(T1, T2, np.zeros(3), [0.11, 0.0, 0.0], sigma2, sigma2, np.float32(1.5) * np.float32(1.2), cam1=NS.PIN_CAM, cam2=NS.PIN_CAM)
    h1 = (np.random.default_rng(9).random(len(kp)) < 0.3).astype(np.uint8)
    sc2 = dict(kp1=kp, desc1=desc, node1=node1, sf=sf)
    TC.write_scene(os.path.join(tmp, "extracted.bin"), sc2, nbs, h1, [nb["has"] for nb in nbs],
                   [orbfe.tri_params(nb["F12"], nb["ep"], False, False, True) for nb in nbs], [G.np_params(P)] * K)
    out["extracted"] = os.path.join(tmp, "extracted.bin")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="newpoints_ab_")
    files = scenes(tmp)
    csrc = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
    progs = {"shipped": os.path.join(tmp, "shipped.bin")}
    build(csrc, "orbfe", progs["shipped"], False)
    for so in sorted(glob.glob(os.path.join(ROOT, "tools", "ab", "liborbfe_*.so"))):
        name = os.path.basename(so)[len("liborbfe_"):-3]
        progs[name] = os.path.join(tmp, name + ".bin")
        build(os.path.dirname(so), "orbfe_" + name, progs[name], True)
    runs = []
    for scene, path in files.items():
        for rnd in range(a.rounds):
            for name, prog in progs.items():
                out = subprocess.run(["timeout", "-k", "10", "240", prog, path, os.path.join(tmp, "out.bin"), str(a.reps)], check=True,
                                     stdout=subprocess.PIPE).stdout.decode()
                m = re.search(r"newpoints_rounds_us search_batch=([0-9.,]+) create_new_points_batch=([0-9.,]+)", out)
                lat = re.search(r"host_pairs=(\d+) host_loop=([0-9.]+) host_us_per_pair=([0-9.]+) host_same=(\d)", out)
                cr = re.search(r"created=(\d+) matched=(\d+) rc=(\d+)", out)
                rec = dict(scene=scene, round=rnd, library=name, search_batch_us=[float(x) for x in m.group(1).split(",")],
                           create_new_points_batch_us=[float(x) for x in m.group(2).split(",")] if name == "shipped" else None,
                           rc=int(cr.group(3)))
                if name == "shipped":
                    rec.update(created=int(cr.group(1)), matched=int(cr.group(2)), host_pairs=int(lat.group(1)), host_loop_us=float(lat.group(2)),
                               host_us_per_pair=float(lat.group(3)), host_same=int(lat.group(4)))
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    med = lambda v: float(np.median(v))
    summary = {}
    for scene in files:
        mine = [r for r in runs if r["scene"] == scene and r["library"] == "shipped"]
        s = dict(a_shipped_us=med([x for r in mine for x in r["search_batch_us"]]),
                 b_us=med([x for r in mine for x in r["create_new_points_batch_us"]]),
                 c_us_per_pair=med([r["host_us_per_pair"] for r in mine]), matches=mine[0]["matched"], created=mine[0]["created"],
                 host_same=min(r["host_same"] for r in mine))
        for name in progs:
            if name != "shipped":
                s["a_%s_us" % name] = med([x for r in runs if r["scene"] == scene and r["library"] == name for x in r["search_batch_us"]])
        base = s.get("a_parent_us", s["a_shipped_us"])
        s["b_minus_a_us"] = s["b_us"] - base
        s["host_would_spend_us"] = s["c_us_per_pair"] * s["matches"]
        summary[scene] = s
        print(scene, json.dumps(s), flush=True)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or None, tool="tools/newpoints_ab.py", reps=a.reps, rounds=a.rounds,
                                      note="medians of `reps` calls after 20 warm-up calls; three (a)/(b) alternations per run, "
                                           "`rounds` runs per library alternating; microseconds"),
                           summary=summary, runs=runs), f, indent=1)


if __name__ == "__main__":
    main()

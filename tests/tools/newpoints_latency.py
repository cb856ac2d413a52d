#!/usr/bin/env python3
"""Per-call latency of orbfe_create_new_points_batch next to orbfe_match_triangulation_batch, in the row format and on the
K = 20 / N ~ 1012 inputs of tests/tools/matcher_latency.py (a synthetic frame's keypoints, 20 descriptor-only neighbours
displaced along x, resident key frames, the C calls with pre-built argument arrays).  The neighbours are the key frame's
keypoints moved along x: the geometry block is the pose that displacement stands for (t12 = (0.11, 0, 0), the F12 of
test_triangulation_batch.neighbour).  Results are checked before timing: the replay of the raw matches against K oracle
searches, verdict and x3D of their matches against the numpy restatement of S11 (tests/newpoints_ref.py).  That checker is
NOT a fair time for the host's geometry (Python); tools/newpoints_ab.py times a single-thread C++ loop instead.

usage: python3 tests/tools/newpoints_latency.py [--reps 200] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import newpoints_ref as NR  # noqa: E402
import oracle_py as O  # noqa: E402
import orbfe  # noqa: E402
import test_triangulation_batch as TB  # noqa: E402
from orbfe import synth  # noqa: E402

W, H = 752, 480
ARGS = (1000, 40000, 1.2, 8, 20, 7, W, H)
CAM = [458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0]


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    eo = O.Extractor(*ARGS)
    ex = orbfe.ORBextractor(*ARGS)
    kp, desc, _ = eo.extract(list(synth.stream(W, H, 2))[0])
    n = len(kp)
    sf = eo.scaleFactors
    K = 20
    node1 = TB.nodes_of(kp)
    nbs = [TB.neighbour(kp, desc, 500 + k, True, False) for k in range(K)]
    csrs = [tuple(np.asarray(x, np.int32) for x in TB.csr(node1, nb["node"])) for nb in nbs]
    h1 = (np.random.default_rng(2).random(n) < 0.3).astype(np.uint8)
    has2 = [nb["has"] for nb in nbs]
    kf1 = orbfe.KeyFrame(ex, kp.view(orbfe.KP_DTYPE), desc, node1, ex.mvScaleFactor)
    kf2 = [orbfe.KeyFrame(ex, nb["kp"].view(orbfe.KP_DTYPE), nb["desc"], nb["node"], ex.mvScaleFactor) for nb in nbs]
    kfp = (C.c_void_p * K)(*[k.h.value for k in kf2])
    h2p = (C.c_void_p * K)(*[v.ctypes.data for v in has2])
    P = (orbfe.TriParams * K)(*[orbfe.tri_params(nb["F12"], nb["ep"], False, False, True) for nb in nbs])
    sf32 = np.asarray(sf, np.float32)
    geo = NR.params(np.eye(3, 4), np.hstack([np.eye(3), [[-0.11], [0.0], [0.0]]]), np.zeros(3), [0.11, 0.0, 0.0], sf32 * sf32, sf32 * sf32,
                    np.float32(1.5) * np.float32(1.2), cam1=CAM, cam2=CAM)
    Q = (orbfe.NewPointParams * K)(*[orbfe.newpoint_params(geo["Tcw1"], geo["Tcw2"], geo["twc1"], geo["twc2"], geo["sigma2_1"],
                                                           geo["sigma2_2"], geo["ratioFactor"], 0, 0, geo["cam1"], geo["cam2"])] * K)
    raw = np.full((K, n), -1, np.int32)
    rbin = np.zeros((K, n), np.uint8)
    x3d = np.zeros((K, n, 3), np.float32)
    verdict = np.zeros((K, n), np.uint8)
    vp = lambda a_: a_.ctypes.data_as(C.c_void_p)
    rows = []

    def row(name, ref, size, gpu_fn, cpu_fn, same):
        got, want = gpu_fn(), cpu_fn()
        assert same(got, want), name
        tg, tc = timed(gpu_fn, a.reps), timed(cpu_fn, a.cpu_reps)
        rows.append(dict(entry=name, reference=ref, size=size, gpu_ms_per_call=tg, oracle_ms_per_call=tc, ratio=tc / tg))
        print("%-36s %-44s gpu %7.3f ms   oracle(1 thread) %8.3f ms   x%.1f" % (name, size, tg, tc, tc / tg), flush=True)

    def batch_gpu():
        assert ex.L.orbfe_match_triangulation_batch(ex.h, kf1.h, vp(h1), K, kfp, h2p, P, vp(raw), vp(rbin)) == 0
        return raw, rbin

    def create_gpu():
        assert ex.L.orbfe_create_new_points_batch(ex.h, kf1.h, vp(h1), K, kfp, h2p, P, Q, vp(raw), vp(rbin), vp(x3d), vp(verdict)) == 0
        return raw, rbin, x3d, verdict

    def seq_cpu():
        return [O.search_for_triangulation(*csrs[k], kp, desc, h1, None, nbs[k]["kp"], nbs[k]["desc"], has2[k], None, sf,
                                           nbs[k]["F12"], nbs[k]["ep"], False, False, True) for k in range(K)]

    def create_cpu():
        out = []
        for k, (nm, m12) in enumerate(seq_cpu()):
            i1 = np.flatnonzero(m12 >= 0)
            out.append((nm, m12, i1) + NR.triangulate(geo, kp, nbs[k]["kp"], sf32, sf32, i1, m12[i1]))
        return out

    replay = lambda res: [orbfe.triangulation_select(res[0][k], res[1][k], h1, True) for k in range(K)]
    eqk = lambda got, want: all(x[0] == y[0] and np.array_equal(x[1], y[1]) for x, y in zip(got, want))

    def create_same(got, want):
        return eqk(replay(got), want) and all(np.array_equal(got[3][k][want[k][2]], want[k][3]) and
                                              got[2][k][want[k][2]].tobytes() == want[k][4].tobytes() for k in range(K))

    row("orbfe_match_triangulation_batch K=20", "LocalMapping.cc:455-488", "N=%d, 20 resident neighbours, C call" % n, batch_gpu, seq_cpu,
        lambda got, want: eqk(replay(got), want))
    row("orbfe_create_new_points_batch K=20", "LocalMapping.cc:455-705", "N=%d, search + S11 geometry of every raw partner" % n, create_gpu,
        create_cpu, create_same)
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        with open(a.json, "w") as f:
            json.dump(dict(_meta=dict(git_head=head or None, tool="tests/tools/newpoints_latency.py"), host_cpus=os.cpu_count(), reps=a.reps,
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

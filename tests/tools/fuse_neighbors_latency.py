#!/usr/bin/env python3
"""Latency of the first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:819-824), K = 20 targets of N ~ 1000
features, M = 2000 map points, th = 10, resident key frames and map, the C calls with pre-built argument arrays:
  (a) K sequential orbfe_fuse_search_keyframe calls (what the library offered before the batch call),
  (b) ONE orbfe_fuse_search_keyframes, cand_cap 0 and 4,
  (c) the whole replay through include/orbfe_adaptor.hpp (tests/cpp/fuse_neighbors.cpp: NeighbourFuseBatch against the loop of K
      ResidentFuse::Fuse calls with the map updated between them, mock graph types), default and sparse scene.
Legs (a) and (b) alternate three times on one box, `--reps` calls per leg, the median call of every leg is reported.  Every
row is checked against the oracle before timing.

usage: python3 tests/tools/fuse_neighbors_latency.py [--reps 300] [--json out.json] [--no-replay]"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "orb_slam3_v1.0_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import frustum_scenarios as FS  # noqa: E402
import neighbors_model as NM  # noqa: E402
import oracle_py as O  # noqa: E402
import orbfe  # noqa: E402
import test_fuse_neighbors_cpp as TC  # noqa: E402
from test_frustum import PN  # noqa: E402

W, H, ARGS = NM.W, NM.H, NM.ARGS


def median_ms(fn, reps):
    for _ in range(10):
        fn()
    t = np.zeros(reps)
    for i in range(reps):
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return float(np.median(t) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-replay", action="store_true")
    a = ap.parse_args()
    K, M, th = 20, 2000, 10.0
    sc = NM.scene(seed=5, K=K, M=M)
    ex = orbfe.ORBextractor(*ARGS)
    L = ex.L
    Fp = orbfe.Frustum()
    FS.fill_frustum(Fp, PN, seed=60)
    kfs = []
    for nb in sc["nbs"]:
        kf = orbfe.KeyFrame(ex, nb["kp"].view(orbfe.KP_DTYPE), nb["desc"], np.full(len(nb["kp"]), -1, np.int32), sc["eo"].scaleFactors)
        kf.set_grid(64, 48, 0.0, 0.0, float(W), float(H), sc["inv_s2"], None)
        kfs.append(kf)
    mp = orbfe.MapPoints(ex, M)
    ids = np.arange(M, dtype=np.int32)
    mp.update(ids, sc["pts"].view(orbfe.WP_DTYPE), sc["mpd"])
    skip = (np.random.default_rng(3).random((K, M)) < 0.3).astype(np.uint8)  # "IsInKeyFrame" for 30 % of the pairs
    ids_k = [np.where(skip[k] != 0, ~ids, ids).astype(np.int32) for k in range(K)]
    hs = (C.c_void_p * K)(*[kf.h.value for kf in kfs])
    fr = (orbfe.Frustum * K)()
    for k in range(K):
        C.memmove(C.byref(fr, k * C.sizeof(orbfe.Frustum)), C.byref(Fp), C.sizeof(orbfe.Frustum))
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    bi, bd = np.zeros((K, M), np.int32), np.zeros((K, M), np.int32)
    bi1, bd1 = np.zeros((K, M), np.int32), np.zeros((K, M), np.int32)
    ci, cc = np.zeros((K, M, 4), np.int32), np.zeros((K, M), np.int32)

    def sequential():
        for k in range(K):
            assert L.orbfe_fuse_search_keyframe(ex.h, kfs[k].h, mp.h, M, vp(ids_k[k]), C.byref(Fp), th, vp(bi1[k]), vp(bd1[k])) == 0

    def batch0():
        assert L.orbfe_fuse_search_keyframes(ex.h, K, hs, fr, mp.h, M, vp(ids), vp(skip), th, vp(bi), vp(bd), 0, None, None) == 0

    def batch4():
        assert L.orbfe_fuse_search_keyframes(ex.h, K, hs, fr, mp.h, M, vp(ids), vp(skip), th, vp(bi), vp(bd), 4, vp(ci), vp(cc)) == 0

    sequential()
    for fn in (batch0, batch4):
        bi[:], bd[:] = -5, -5
        fn()
        assert np.array_equal(bi, bi1) and np.array_equal(bd, bd1), "the batch call differs from the single calls"
    for k in range(K):
        call = sc["pts"].copy()
        call["skip"] = skip[k]
        bi_r, bd_r = O.fuse_search(sc["nbs"][k]["fv"], sc["inv_s2"], None, sc["Fo"], th, call, sc["mpd"])
        assert np.array_equal(bi[k], bi_r) and np.array_equal(bd[k], bd_r), "target %d differs from the oracle" % k
    rounds = []
    for r in range(3):
        row = dict(sequential_ms=median_ms(sequential, a.reps), batch_cap0_ms=median_ms(batch0, a.reps),
                   batch_cap4_ms=median_ms(batch4, a.reps))
        row["ratio_cap4"] = row["sequential_ms"] / row["batch_cap4_ms"]
        rounds.append(row)
        print("alternation %d: K sequential calls %.3f ms (%.4f per call)   one call cap 0 %.3f ms   cap 4 %.3f ms   x%.1f" % (
            r, row["sequential_ms"], row["sequential_ms"] / K, row["batch_cap0_ms"], row["batch_cap4_ms"], row["ratio_cap4"]), flush=True)
    out = dict(scene="K=%d N=%d..%d M=%d th=%g, 30%% of the pairs skipped" % (K, len(sc["nbs"][-1]["kp"]), len(sc["nbs"][0]["kp"]), M, th),
               reps=a.reps, rounds=rounds, download_bytes_cap4=int(K * M * (8 + 4 * 4 + 4)),
               pairs_above_cap4=int((cc > 4).sum()), candidate_counts={int(k): int(v) for k, v in zip(*np.unique(cc, return_counts=True))},
               single_call_th10_ms=float(np.median([r["sequential_ms"] for r in rounds]) / K))
    if not a.no_replay:
        if not os.path.exists(TC.BIN):
            TC._build()
        replay = {}
        for name, kw in NM.SCENES.items():
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "scene.bin")
                TC.write_scene(path, NM.scene(seed=5, K=K, M=1200))
                txt = subprocess.run([TC.BIN, path, str(kw["fobs"][0]), str(kw["fobs"][1]), str(kw["inkf"]), "15"], capture_output=True,
                                     text=True, timeout=900).stdout
            print(name, txt, flush=True)
            vals = {k: float(v) for k, v in re.findall(r"(\w+)=([0-9.]+)", txt)}
            replay[name] = vals
        out["replay_K20_M1200"] = replay
    if a.json:
        head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
        out["_meta"] = dict(git_head=head or None, tool="tests/tools/fuse_neighbors_latency.py")
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "replay_K20_M1200"}))


if __name__ == "__main__":
    main()

"""tests/cpp/fuse_neighbors.cpp: the first loop of LocalMapping::SearchInNeighbors from a plain C++ program through
include/orbfe_adaptor.hpp's NeighbourFuseBatch (mock MapPoint / KeyFrame types whose Replace really recomputes the survivor's
descriptor) against the loop of K ResidentFuse::Fuse calls, on two copies of one scene: identical graphs and nFused per
target, one submission plus fallbacks, and the timing line of the whole replay."""
import os
import re
import subprocess

import numpy as np
import pytest

import neighbors_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "fuse_neighbors.bin")


def _build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fuse_neighbors.cpp"), "-o", BIN, "-L", CSRC, "-lorbfe", "-Wl,-rpath," + CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"])


def write_scene(path, sc):
    """scene.bin of tests/cpp/fuse_neighbors.cpp: int32 K, M, levels; float32 scale factors, mvInvLevelSigma2; orbfe_frustum;
    orbfe_world_point[M]; descriptors[M][32]; per target int32 n, keypoints (24 B each), descriptors."""
    import orbfe
    import frustum_scenarios as FS
    from test_frustum import PN
    Fp = orbfe.Frustum()
    FS.fill_frustum(Fp, PN, seed=60)
    sf = np.ascontiguousarray(sc["eo"].scaleFactors, np.float32)
    with open(path, "wb") as f:
        f.write(np.array([sc["K"], sc["M"], len(sf)], np.int32).tobytes())
        f.write(sf.tobytes())
        f.write(np.ascontiguousarray(sc["inv_s2"], np.float32).tobytes())
        f.write(bytes(Fp))
        f.write(np.ascontiguousarray(sc["pts"]).view(orbfe.WP_DTYPE).tobytes())
        f.write(np.ascontiguousarray(sc["mpd"], np.uint8).tobytes())
        for nb in sc["nbs"]:
            f.write(np.array([len(nb["kp"])], np.int32).tobytes())
            f.write(np.ascontiguousarray(nb["kp"]).tobytes())
            f.write(np.ascontiguousarray(nb["desc"], np.uint8).tobytes())


def test_fuse_neighbors_program_links(built):
    _build()
    assert "gfx950" in subprocess.check_output([BIN]).decode()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,cap", [("default", 4), ("sparse", 4), ("default", 1)])
def test_fuse_neighbors_program_ends_with_the_sequential_graph(built, tmp_path, scene, cap):
    _build()
    K, M = 20, 1200
    sc = NM.scene(seed=5, K=K, M=M)
    write_scene(tmp_path / "scene.bin", sc)
    kw = NM.SCENES[scene]
    p = subprocess.run([BIN, str(tmp_path / "scene.bin"), str(kw["fobs"][0]), str(kw["fobs"][1]), str(kw["inkf"]), "5", str(cap)],
                       capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"fuse_neighbors K=20 M=1200 fused=(\d+) same=1 submissions=(\d+) host_selects=(\d+) overflows=(\d+) pairs_above_cap=(\d+)",
                  p.stdout)
    assert m, p.stdout
    fused, submissions, selects, overflows = (int(m.group(i)) for i in range(1, 5))
    lat = re.search(r"fuse_neighbors_latency_us sequential_loop=([0-9.]+) batch_replay=([0-9.]+) reps=5 select_us_per_call=([0-9.]+) "
                    r"select_us_total=([0-9.]+)", p.stdout)
    assert lat, p.stdout
    assert fused >= (1000 if scene == "default" else 100)  # the loop really fuses
    assert submissions <= 1 + K and (submissions == 1) == (overflows == 0)
    if cap == 4:
        assert overflows <= 0.01 * selects
    else:  # candCap = 1 truncates every list of two or more: the adaptor's fallback search really runs
        assert submissions >= 6 and overflows >= 50
    if scene == "default":
        assert selects >= 100  # descriptors really changed under the replay

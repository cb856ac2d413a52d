"""tests/cpp/newpoints.cpp: the neighbour loop of LocalMapping::CreateNewMapPoints from a plain C++ program through
include/orbfe_adaptor.hpp's NewMapPointsBatch (mock KeyFrame types, pKF1->AddMapPoint between the neighbours).  The created
points must equal those of K sequential oracle SearchForTriangulation calls, each followed by the S11 restatement on its
matches; the program's own single-thread host loop of S11 must agree with the library bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import newpoints_ref as R
import newpoints_scenarios as NS
import oracle_py as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "newpoints.bin")


def _build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "newpoints.cpp"), "-o", BIN, "-L", CSRC, "-lorbfe", "-Wl,-rpath," + CSRC,
                           "-Wl,-rpath,/opt/rocm/lib"])


def write_scene(path, sc, nbs, has1, has2, tri, geo):
    """scene.bin of tests/cpp/newpoints.cpp: int32 n1, K, levels; float32 scale factors; key frame 1; per neighbour int32 n2, the key
    frame, orbfe_tri_params, orbfe_newpoint_params.  A key frame = keypoints (24 B each), descriptors, int32 nodes, uint8 flags."""
    def kf(f, kp, desc, node, has):
        f.write(np.ascontiguousarray(kp).tobytes())
        f.write(np.ascontiguousarray(desc, np.uint8).tobytes())
        f.write(np.ascontiguousarray(node, np.int32).tobytes())
        f.write(np.ascontiguousarray(has, np.uint8).tobytes())
    with open(path, "wb") as f:
        f.write(np.array([len(sc["kp1"]), len(nbs), len(sc["sf"])], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["sf"], np.float32).tobytes())
        kf(f, sc["kp1"], sc["desc1"], sc["node1"], has1)
        for k, nb in enumerate(nbs):
            f.write(np.array([len(nb["kp"])], np.int32).tobytes())
            kf(f, nb["kp"], nb["desc"], nb["node"], has2[k])
            f.write(bytes(tri[k]))
            f.write(bytes(geo[k]))


def test_newpoints_program_links(built):
    _build()
    assert "gfx950" in subprocess.check_output([BIN]).decode()


@pytest.mark.gpu
def test_newpoints_program_creates_the_reference_points(built, tmp_path):
    import test_newpoints_gpu as G
    import test_triangulation_batch as TB
    _build()
    K = 20
    sc = NS.scene(3, K=K)
    nbs = sc["nbs"]
    has1, has2, coarse, cams = G.search_inputs(sc, nbs, 60 + K)
    write_scene(tmp_path / "scene.bin", sc, nbs, has1, has2, G.tri_params(nbs, coarse, cams), [G.np_params(nb["np"]) for nb in nbs])
    out = subprocess.check_output([BIN, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "200"]).decode()
    print(out)
    m = re.search(r"newpoints K=20 n1=1000 created=(\d+) matched=(\d+) rc=0", out)
    assert m, out
    lat = re.search(r"newpoints_latency_us search_batch=([0-9.]+) create_new_points_batch=([0-9.]+) host_pairs=(\d+) host_loop=([0-9.]+) "
                    r"host_us_per_pair=([0-9.]+) host_same=1 pinhole=1", out)
    assert lat, out
    want, has, matched = [], has1.copy(), 0
    for k, nb in enumerate(nbs):
        off1, idx1, off2, idx2 = TB.csr(sc["node1"], nb["node"])
        n, m12 = O.search_for_triangulation(off1, idx1, off2, idx2, sc["kp1"], sc["desc1"], has, None, nb["kp"], nb["desc"], has2[k], None,
                                            sc["sf"], nb["F12"], nb["ep"], False, coarse[k], True)
        matched += n
        i1 = np.flatnonzero(m12 >= 0)
        v, x = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], i1, m12[i1])
        for p in np.flatnonzero(v == R.ACCEPTED):
            want.append((k, int(i1[p]), int(m12[i1[p]]), x[p].tobytes()))
            has[i1[p]] = 1
    rec = np.fromfile(tmp_path / "out.bin", np.dtype([("k", "<i4"), ("i1", "<i4"), ("i2", "<i4"), ("x", "<f4", 3)]))
    got = [(int(r["k"]), int(r["i1"]), int(r["i2"]), r["x"].tobytes()) for r in rec]
    assert got == want and len(want) >= 100
    assert int(m.group(1)) == len(want) and int(m.group(2)) == matched and int(lat.group(3)) == matched

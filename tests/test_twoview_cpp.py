"""tests/cpp/two_view.cpp: TwoViewReconstruction::Reconstruct from a plain C++ program through include/orbfe_adaptor.hpp's
TwoViewReconstruction class.  The program carries its own host loop of SPEC DECISION S12 (single-thread, and H || F on two
threads as src/TwoViewReconstruction.cc:102-107): the library's arithmetic for the CPU -- csrc's host-safe headers compiled as host
C++, with only the ordering of the team-parallel parts restated; twoview_ref.py is the independent oracle of both.  The host loop is
built stand-alone with -fsanitize=address,undefined (a program with its own main, never loaded into Python) and compared with the
numpy restatement byte for byte without a GPU; on the GPU the library's results through the adaptor must equal both."""
import os
import re
import subprocess

import numpy as np
import pytest

import twoview_scenarios as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "two_view.bin")
BIN_SAN = os.path.join(ROOT, "tests", "cpp", "two_view_san.bin")
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
HOST_CASES = [("general", 300, 0.3, 200), ("plane", 300, 0.0, 200), ("lowpar", 300, 0.0, 200), ("rotation", 300, 0.0, 200),
              ("static", 100, 0.0, 200), ("few", 63, 0.3, 200), ("tinysigma", 100, 1.0, 200), ("general", 65, 0.0, 200)]


_built = {}


def _build(san=False):
    out = BIN_SAN if san else BIN
    if out in _built:  # once per session
        return out
    _built[out] = 1
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"),
                                             "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "two_view.cpp"), "-o", out, "-L", CSRC,
                                             "-lorbfe", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def write_scene(path, sc):
    fx, fy, cx, cy, sigma, iterations = sc["params"]
    with open(path, "wb") as f:
        f.write(np.array([len(sc["kp1"]), len(sc["kp2"]), iterations], np.int32).tobytes())
        f.write(np.array([fx, fy, cx, cy, sigma], np.float32).tobytes())
        for xy in (sc["kp1"], sc["kp2"]):
            kp = np.zeros(len(xy), KP)
            kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
            f.write(kp.tobytes())
        f.write(np.ascontiguousarray(sc["matches12"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["sets"], np.int32).tobytes())


def read_result(path, n1, iterations):
    b = open(path, "rb").read()
    at = [0]

    def take(dt, n):
        a = np.frombuffer(b, dt, n, at[0])
        at[0] += a.nbytes
        return a
    head = take(np.int32, 7)
    r = dict(zip(("reconstructed", "model", "exit_line", "best_it_H", "best_it_F", "n_hypotheses", "best_hypothesis"), (int(v) for v in head)))
    r["n_good"] = take(np.int32, 8)
    r["SH"], r["SF"], r["RH"] = take(np.float32, 3)
    for k, n in (("H21", 9), ("F21", 9), ("cos_parallax", 8), ("R21", 9), ("t21", 3), ("scores", 2 * iterations), ("p3d", 3 * n1)):
        r[k] = take(np.float32, n)
    r["triangulated"] = take(np.uint8, n1)
    assert at[0] == len(b)
    return r


def same(got, want, what):
    for k in ("reconstructed", "model", "exit_line", "best_it_H", "best_it_F", "n_hypotheses", "best_hypothesis"):
        assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    for k, dt in (("n_good", np.int32), ("SH", np.float32), ("SF", np.float32), ("RH", np.float32), ("H21", np.float32), ("F21", np.float32),
                  ("cos_parallax", np.float32), ("R21", np.float32), ("t21", np.float32), ("scores", np.float32), ("p3d", np.float32),
                  ("triangulated", np.uint8)):
        assert np.ascontiguousarray(got[k], dt).tobytes() == np.ascontiguousarray(want[k], dt).tobytes(), "%s: %s differs" % (what, k)


def test_two_view_program_links(built):
    _build()
    assert "gfx950" in subprocess.check_output([BIN]).decode()


@pytest.mark.parametrize("case", HOST_CASES, ids=TS.case_id)
def test_host_loop_equals_restatement(built, tmp_path, case):
    """the program's own S12 (one thread and two), built with AddressSanitizer and UBSan, against twoview_ref.reconstruct: every byte,
    no GPU"""
    exe = _build(san=True)
    sc = TS.make(case[0], case[1], 0, case[2], case[3])
    write_scene(tmp_path / "scene.bin", sc)
    out = subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"]).decode()
    assert "threads_same=1" in out, out
    same(read_result(tmp_path / "out.bin", len(sc["kp1"]), case[3]), TS.ref(sc), TS.case_id(case))


@pytest.mark.gpu
def test_two_view_program_equals_library_and_restatement(built, tmp_path):
    _build()
    for case in (("general", 300, 0.3, 200), ("plane", 300, 0.0, 200), ("lowpar", 300, 0.0, 200)):
        sc = TS.make(case[0], case[1], 0, case[2], case[3])
        write_scene(tmp_path / "scene.bin", sc)
        out = subprocess.check_output([BIN, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "40"]).decode()
        print(out)
        lat = re.search(r"two_view_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_two_threads=([0-9.]+) host_same=1", out)
        assert lat, out
        same(read_result(tmp_path / "out.bin", len(sc["kp1"]), case[3]), TS.ref(sc), TS.case_id(case))

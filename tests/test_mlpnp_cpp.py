"""tests/cpp/mlpnp.cpp: MLPnPsolver (constructor, SetRansacParameters, one iterate) from a plain C++ program through
include/orbfe_adaptor.hpp's MLPnPsolver class.  The program carries its own single-thread host loop of SPEC DECISION S13 (the kernels'
arithmetic for the CPU: csrc's host-safe headers compiled as host C++, with only the ordering of the team-parallel parts restated;
mlpnp_ref.py is the independent oracle of both).  The host loop is built stand-alone with -fsanitize=address,undefined (a program with
its own main, never loaded into Python) and compared with the numpy restatement byte for byte without a GPU; on the GPU the library's
results through the adaptor must equal both, and a second iterate() on one solver must be refused."""
import os
import re
import subprocess

import numpy as np
import pytest

import mlpnp_scenarios as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "mlpnp.bin")
BIN_SAN = os.path.join(ROOT, "tests", "cpp", "mlpnp_san.bin")
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
HOST_CASES = [c for c in MS.CASES if c[1] != 49]  # every scene that runs hypotheses
INT32 = ("solved", "n_inliers", "no_more", "N", "min_inliers", "max_its", "total_iterations", "exit_kind", "returning_iteration", "n_candidates")

_built = {}


def _build(san=False):
    out = BIN_SAN if san else BIN
    if out in _built:  # once per session
        return out
    _built[out] = 1
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if san else ["-O2"]
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                             os.path.join(ROOT, "tests", "cpp", "mlpnp.cpp"), "-o", out, "-L", CSRC, "-lorbfe",
                                             "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    return out


def write_scene(path, sc):
    rp = sc["ransac"]
    kp = np.zeros(len(sc["kp_xy"]), KP)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    with open(path, "wb") as f:
        f.write(np.array([len(kp), len(sc["points"]), len(sc["sets"]), rp["min_set"], sc["model"], len(sc["level_sigma2"]), rp["min_inliers"],
                          rp["max_iterations"], rp["n_iterations"]], np.int32).tobytes())
        f.write(np.array([rp["probability"]], np.float64).tobytes())
        f.write(np.concatenate([sc["cam"], [sc["precision"], rp["epsilon"], rp["th2"]]]).astype(np.float32).tobytes())
        f.write(np.ascontiguousarray(sc["level_sigma2"], np.float32).tobytes())
        f.write(kp.tobytes())
        f.write(np.ascontiguousarray(sc["mp_index"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["points"], np.float32).tobytes())
        f.write(np.ascontiguousarray(sc["sets"], np.int32).tobytes())


def read_result(path, n):
    b = open(path, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(b, dt, cnt, at[0])
        at[0] += a.nbytes
        return a
    r = dict(zip(INT32, (int(v) for v in take(np.int32, 10))))
    T, nc, N = r["total_iterations"], r["n_candidates"], r["N"]
    r["Tcw"] = take(np.float32, 16)
    r["inliers"] = take(np.uint8, n)
    r["hyp_Rt"] = take(np.float64, 12 * T)
    for k in ("hyp_inliers", "hyp_planar", "hyp_gn_evals", "hyp_gn_exit"):
        r[k] = take(np.int32, T)
    r["candidates"] = take(np.int32, nc)
    r["cand_Rt"] = take(np.float64, 12 * nc)
    r["cand_inliers"], r["cand_planar"] = take(np.int32, nc), take(np.int32, nc)
    r["cand_mask"] = take(np.uint8, nc * N)
    assert at[0] == len(b)
    return r


def same(got, want, what):
    for k in INT32:
        assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    for k, dt in (("Tcw", np.float32), ("inliers", np.uint8), ("hyp_Rt", np.float64), ("hyp_inliers", np.int32), ("hyp_planar", np.int32),
                  ("hyp_gn_evals", np.int32), ("hyp_gn_exit", np.int32), ("candidates", np.int32), ("cand_Rt", np.float64),
                  ("cand_inliers", np.int32), ("cand_planar", np.int32), ("cand_mask", np.uint8)):
        assert np.ascontiguousarray(got[k], dt).tobytes() == np.ascontiguousarray(want[k], dt).reshape(-1).tobytes(), "%s: %s differs" % (what, k)


def test_mlpnp_program_links(built):
    _build()
    assert "gfx950" in subprocess.check_output([BIN]).decode()


@pytest.mark.parametrize("case", HOST_CASES, ids=MS.case_id)
def test_host_loop_equals_restatement(built, tmp_path, case):
    """the program's own S13, built with AddressSanitizer and UBSan, against mlpnp_ref.ransac: every byte, no GPU"""
    exe = _build(san=True)
    sc = MS.make_case(case)
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"])
    same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), MS.ref(sc), MS.case_id(case))


@pytest.mark.gpu
def test_mlpnp_program_equals_library_and_restatement(built, tmp_path):
    _build()
    for case in (MS.CASES[0], MS.CASES[2], MS.CASES[6], MS.CASES[10], MS.CASES[-1]):
        sc = MS.make_case(case)
        write_scene(tmp_path / "scene.bin", sc)
        out = subprocess.check_output([BIN, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "20"]).decode()
        print(out)
        assert re.search(r"mlpnp_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_same=1 second_iterate_refused=1", out), out
        same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), MS.ref(sc), MS.case_id(case))

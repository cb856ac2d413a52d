"""tests/cpp/poseopt.cpp: Optimizer::PoseOptimization from a plain C++ program through include/orbfe_adaptor.hpp's wrapper.  The program
carries its own single-thread host loop of SPEC DECISION S14 (the kernel's arithmetic written out for the CPU; poseopt_ref.py is the
independent oracle of both).  The host loop is built stand-alone with -fsanitize=address,undefined (a program with its own main, never
loaded into Python) and compared with the numpy restatement byte for byte without a GPU; on the GPU the library's results through the
adaptor must equal both."""
import re
import subprocess

import numpy as np
import pytest

import cpp_build
import poseopt_scenarios as PS

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
HOST_CASES = [("general", 300, 0), ("outliers", 300, 1), ("far", 65, 0), ("zero_depth", 10, 0), ("general", 2, 0), ("general", 9, 0)]
SCALARS = ("n_inliers", "N_e", "rounds_run")


def _build(san=False):
    return cpp_build.build("poseopt", san)


def write_scene(path, sc, iterations=25, rounds=4, chi2_threshold=5.991, huber_delta2=7.815):
    kp = np.zeros(len(sc["kp_xy"]), KP)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    s2 = np.asarray(sc["level_sigma2"], np.float32)
    with open(path, "wb") as f:
        f.write(np.array([len(kp), len(sc["points"]), len(s2), iterations, rounds], np.int32).tobytes())
        f.write(np.array([huber_delta2], np.float64).tobytes())
        f.write(np.concatenate([sc["cam"], [chi2_threshold]]).astype(np.float32).tobytes())
        f.write((np.float32(1.0) / s2).astype(np.float32).tobytes())
        f.write(np.ascontiguousarray(sc["Rcw"], np.float32).tobytes())
        f.write(np.ascontiguousarray(sc["tcw"], np.float32).tobytes())
        f.write(kp.tobytes())
        f.write(np.ascontiguousarray(sc["mp_index"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["points"], np.float32).tobytes())


def read_result(path, n):
    b = open(path, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(b, dt, cnt, at[0])
        at[0] += a.nbytes
        return a
    r = dict(zip(SCALARS, (int(v) for v in take(np.int32, 3))))
    nr, Ne = r["rounds_run"], r["N_e"]
    for k in ("round_iterations", "round_trials", "round_nbad", "round_exit"):
        r[k] = take(np.int32, 4)[:nr]
    r["Tcw"] = take(np.float32, 16).reshape(4, 4)
    r["outlier"] = take(np.uint8, n)
    r["round_pose"] = take(np.float64, 48).reshape(4, 12)[:nr]
    r["round_lambda"], r["round_chi2"] = take(np.float64, 4)[:nr], take(np.float64, 4)[:nr]
    r["round_outlier"] = take(np.uint8, 4 * Ne).reshape(4, Ne)[:nr]
    assert at[0] == len(b)
    return r


FIELDS = (("Tcw", np.float32), ("outlier", np.uint8), ("round_pose", np.float64), ("round_iterations", np.int32), ("round_trials", np.int32),
          ("round_lambda", np.float64), ("round_chi2", np.float64), ("round_nbad", np.int32), ("round_exit", np.int32),
          ("round_outlier", np.uint8))


def same(got, want, what, nonfinite_by_kind=False):
    """every byte; with nonfinite_by_kind (the zero_depth scenes) non-finite values are compared by position and kind -- isnan, isinf
    and the sign of an infinity -- because NaN payloads differ between hosts and the GPU"""
    for k in SCALARS:
        assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    for k, dt in FIELDS:
        g, w = np.ascontiguousarray(got[k], dt).reshape(-1), np.ascontiguousarray(want[k], dt).reshape(-1)
        assert g.shape == w.shape, "%s: %s has another size" % (what, k)
        if nonfinite_by_kind and dt in (np.float32, np.float64):
            fin = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), fin) and np.array_equal(np.isnan(g), np.isnan(w)), "%s: %s non-finite pattern" % (what, k)
            assert np.array_equal(np.sign(g[np.isinf(g)]), np.sign(w[np.isinf(w)])), "%s: %s sign of infinity" % (what, k)
            g, w = g[fin], w[fin]
        assert g.tobytes() == w.tobytes(), "%s: %s differs" % (what, k)


def test_poseopt_program_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


@pytest.mark.parametrize("case", HOST_CASES, ids=PS.case_id)
def test_host_loop_equals_restatement_under_sanitizers(built, tmp_path, case):
    """the program's own S14, built with AddressSanitizer and UBSan, against poseopt_ref.pose_optimization: every byte, no GPU"""
    exe = _build(san=True)
    sc = PS.make_case(case)
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"])
    same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), PS.ref_cached(case), PS.case_id(case), case[0] == "zero_depth")


@pytest.mark.gpu
def test_poseopt_program_equals_library_and_restatement(built, tmp_path):
    exe = _build()
    for case in (("general", 300, 0), ("outliers", 300, 1), ("far", 65, 0)):
        sc = PS.make_case(case)
        write_scene(tmp_path / "scene.bin", sc)
        out = subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "20"]).decode()
        print(out)
        assert re.search(r"poseopt_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_same=1", out), out
        same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), PS.ref_cached(case), PS.case_id(case))

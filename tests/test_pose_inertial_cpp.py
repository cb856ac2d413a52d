"""tests/cpp/pose_inertial.cpp: Optimizer::PoseInertialOptimizationLastKeyFrame from a plain C++ program through
include/orbfe_adaptor.hpp's wrapper.  The program carries its own single-thread host loop of SPEC DECISION S19 (the kernel's arithmetic
written out for the CPU, on csrc/poseimu_math.h and csrc/ldlt.h; pose_inertial_ref.py is the independent oracle of both).  The host
loop is built stand-alone with -fsanitize=address,undefined (a program with its own main, never loaded into Python) and compared with
the numpy restatement byte for byte without a GPU, on one case of every kind; so are the four SO(3) functions on inputs of every
branch, and ldlt_solve_n<6> against ldlt_solve6.  On the GPU the library's results through the adaptor must equal both."""
import collections
import re
import subprocess

import numpy as np
import pytest

import cpp_build
import pose_inertial_ref as R
import pose_inertial_scenarios as PS

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
LINK_FLOATS = ("Rwb1", "twb1", "v1", "bg1", "ba1", "dR", "dV", "dP", "dt", "Rcb", "tcb", "tbc")
SCALARS = ("n_inliers", "N_e", "rounds_run", "recovered")


def _build(san=False, opt="-O2"):
    return cpp_build.build("pose_inertial", san, opt)


def link_bytes(link):
    fl = np.concatenate([np.asarray(link[k], np.float32).reshape(-1) for k in LINK_FLOATS])
    assert len(fl) == 52
    return fl.tobytes() + np.concatenate([np.asarray(link[k], np.float64).reshape(-1) for k in ("info9", "infoG", "infoA")]).tobytes()


def state_in(sc):
    return np.concatenate([np.asarray(sc[k], np.float32).reshape(-1) for k in ("Rcw", "tcw", "Rwb", "twb", "v", "bg", "ba")])


def write_scene(path, sc, **kw):
    prm = dict(R.PARAMS)
    prm.update(kw)
    kp = np.zeros(len(sc["kp_xy"]), KP)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    s2 = np.asarray(sc["level_sigma2"], np.float32)
    with open(path, "wb") as f:
        f.write(np.array([len(kp), len(sc["points"]), len(s2), prm["iterations"], prm["rounds"], prm["rec_init"], prm["recover_below"]],
                         np.int32).tobytes())
        f.write(np.array([prm["huber_delta2"], prm["close_factor"]], np.float64).tobytes())
        f.write(np.concatenate([sc["cam"], prm["chi2"], [prm["close_depth"], prm["recover_chi2"], prm["gravity"]]]).astype(np.float32).tobytes())
        f.write((np.float32(1.0) / s2).astype(np.float32).tobytes())
        f.write(link_bytes(sc["link"]))
        f.write(state_in(sc).tobytes())
        f.write(kp.tobytes())
        f.write(np.ascontiguousarray(sc["mp_index"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["points"], np.float32).tobytes())
        f.write(np.ascontiguousarray(sc["track_depth"], np.float32).tobytes())


def read_result(path, n):
    b = open(path, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(b, dt, cnt, at[0])
        at[0] += a.nbytes
        return a
    r = dict(zip(SCALARS, (int(v) for v in take(np.int32, 4))))
    nr, Ne = r["rounds_run"], r["N_e"]
    for k in ("round_iterations", "round_ok", "round_nbad"):
        r[k] = take(np.int32, 4)[:nr]
    st = take(np.float32, 21)
    r.update(Rwb=st[:9], twb=st[9:12], v=st[12:15], bg=st[15:18], ba=st[18:21])
    r["H"] = take(np.float64, 225).reshape(15, 15)
    r["outlier"] = take(np.uint8, n)
    r["round_state"] = take(np.float64, 84).reshape(4, 21)[:nr]
    r["round_outlier"] = take(np.uint8, 4 * Ne).reshape(4, Ne)[:nr]
    assert at[0] == len(b)
    return r


FIELDS = (("Rwb", np.float32), ("twb", np.float32), ("v", np.float32), ("bg", np.float32), ("ba", np.float32), ("H", np.float64),
          ("outlier", np.uint8), ("round_state", np.float64), ("round_iterations", np.int32), ("round_ok", np.int32),
          ("round_nbad", np.int32), ("round_outlier", np.uint8))


def same(got, want, what, nonfinite_by_kind=False):
    """every byte of every output and every info field; with nonfinite_by_kind (the zero_depth scenes) non-finite values are compared
    by position and kind -- isnan, isinf and the sign of an infinity -- because NaN payloads differ between hosts and the GPU"""
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


def test_pose_inertial_program_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def test_ldlt_solve_n_equals_ldlt_solve6_under_sanitizers(built):
    """the indexed form against the select form on 600 positive definite, indefinite and singular 6 x 6 systems: every byte, the flag"""
    out = subprocess.check_output([_build(san=True), "ldlt"]).decode()
    m = re.search(r"ldlt_same=1 cases=600 same=600 positive=(\d+)", out)
    assert m and 150 <= int(m.group(1)) <= 250, out   # the positive definite third, and no other


def test_so3_functions_equal_restatement_under_sanitizers(built, tmp_path):
    """ExpSO3, LogSO3 and the two Jacobians of csrc/poseimu_math.h on inputs of every branch against pose_inertial_ref"""
    rng = np.random.RandomState(5)
    v = np.concatenate([rng.normal(size=(20, 3)), 1e-6 * rng.normal(size=(6, 3)), np.zeros((1, 3)), 3.0 * rng.normal(size=(5, 3))])
    cnt = collections.Counter()
    Rm = [R.exp_so3(w, cnt) for w in v[:26]]
    Rm += [np.eye(3).reshape(9) * (1.0 + 1e-6), -np.eye(3).reshape(9) * 1.001, np.eye(3).reshape(9), R.exp_so3(np.array([np.pi, 0.0, 0.0]), cnt)]
    Rm = np.array(Rm, np.float64)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(v), len(Rm)], np.int32).tobytes() + v.tobytes() + Rm.tobytes())
    subprocess.check_call([_build(san=True), "so3", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.float64)
    cnt = collections.Counter()
    want = np.concatenate([np.concatenate([R.exp_so3(w, cnt), R.inverse_right_jacobian_so3(w, cnt), R.right_jacobian_so3(w, cnt)])
                           for w in v] + [R.log_so3(M, cnt) for M in Rm])
    assert got.tobytes() == want.tobytes()
    for k in ("exp_small", "exp_general", "invjr_small", "invjr_general", "jr_small", "jr_general", "log_outside", "log_small", "log_general"):
        assert cnt[k] > 0, k


@pytest.mark.parametrize("case", PS.HOST_CASES, ids=PS.case_id)
def test_host_loop_equals_restatement_under_sanitizers(built, tmp_path, case):
    """the program's own S19, built with AddressSanitizer and UBSan, against pose_inertial_ref: every byte, no GPU"""
    exe = _build(san=True)
    sc = PS.make_case(case)
    write_scene(tmp_path / "scene.bin", sc, **PS.case_kw(case))
    subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"])
    same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), PS.ref_cached(case), PS.case_id(case), case[0] == "zero_depth")


@pytest.mark.gpu
def test_pose_inertial_program_equals_library_and_restatement(built, tmp_path):
    exe = _build()
    for case in (("general", 300, 0), ("outliers", 300, 0), ("far", 65, 0), ("few", 0, 0)):
        sc = PS.make_case(case)
        write_scene(tmp_path / "scene.bin", sc)
        out = subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "5"]).decode()
        print(out)
        assert re.search(r"pose_inertial_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_same=1", out), out
        same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), PS.ref_cached(case), PS.case_id(case))

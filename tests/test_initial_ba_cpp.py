"""tests/cpp/initial_ba.cpp: the bundle adjustment of the initial map from a plain C++ program through include/orbfe_adaptor.hpp's
InitialMapAdjuster::Adjust.  The program carries its own single-thread host loop of SPEC DECISION S17 (the kernel's arithmetic, from
the shared headers, ordered for one CPU thread; initial_ba_ref.py is the independent oracle of both).  The host loop is built
stand-alone with -fsanitize=address,undefined (a program with its own main, never loaded into Python) and compared with the numpy
restatement byte for byte without a GPU; on the GPU the library's results through the adaptor must equal both.  The adaptor's median
depth and rescale (InitialMapAdjuster::MedianDepthScale: one text, run by the host mode on the host loop's results and by Adjust on the
library's) must equal their numpy restatement (initial_ba_ref.median_depth_scale) on scenes that take each return: true, N < 50,
median < 0 (the `behind` scene) and a NaN depth (the `nan_depth` scene)."""
import re
import subprocess

import numpy as np
import pytest

import cpp_build
import initial_ba_ref as R
import initial_ba_scenarios as BS

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
SCALARS = ("N", "iterations", "trials", "exit")
FIELDS = (("Tcw2", np.float32), ("points", np.float32), ("pose", np.float64), ("it_cost", np.float64), ("it_lambda", np.float64),
          ("it_trials", np.int32), ("chi2", np.float64), ("depth_positive", np.uint8))


def _build(san=False):
    return cpp_build.build("initial_ba", san)


def keypoints(xy, octave, dtype=KP):
    kp = np.zeros(len(xy), dtype)
    kp["x"], kp["y"], kp["octave"] = xy[:, 0], xy[:, 1], octave
    kp["size"] = 31.0
    return kp


def write_scene(path, sc, iterations=20, inertial=False, huber_delta2=5.99):
    kp1, kp2 = keypoints(sc["kp1_xy"], sc["kp1_octave"]), keypoints(sc["kp2_xy"], sc["kp2_octave"])
    s2 = np.asarray(sc["level_sigma2"], np.float32)
    with open(path, "wb") as f:
        f.write(np.array([len(kp1), len(kp2), len(s2), iterations, int(sc["robust"]), int(inertial)], np.int32).tobytes())
        f.write(np.array([huber_delta2], np.float64).tobytes())
        f.write(np.asarray(sc["cam"], np.float32).tobytes())
        f.write((np.float32(1.0) / s2).astype(np.float32).tobytes())
        for k in ("Rcw1", "tcw1", "Rcw2", "tcw2"):
            f.write(np.ascontiguousarray(sc[k], np.float32).tobytes())
        f.write(kp1.tobytes())
        f.write(kp2.tobytes())
        f.write(np.ascontiguousarray(sc["matches12"], np.int32).tobytes())
        f.write(np.ascontiguousarray(sc["points"], np.float32).tobytes())


def read_result(path, n1):
    b = open(path, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(b, dt, cnt, at[0])
        at[0] += a.nbytes
        return a
    r = dict(zip(SCALARS, (int(v) for v in take(np.int32, 4))))
    N, ni = r["N"], r["iterations"]
    r["it_trials"] = take(np.int32, 64)[:ni]
    r["Tcw2"] = take(np.float32, 16).reshape(4, 4)
    r["points"] = take(np.float32, 3 * n1).reshape(n1, 3)
    r["it_cost"], r["it_lambda"] = take(np.float64, 64)[:ni], take(np.float64, 64)[:ni]
    r["pose"] = take(np.float64, 12)
    r["chi2"] = take(np.float64, 2 * N).reshape(2, N)
    r["depth_positive"] = take(np.uint8, 2 * N).reshape(2, N)
    r["ok"] = bool(take(np.int32, 1)[0])
    r["median"] = take(np.float32, 1)[0]
    r["scaled_tcw2"] = take(np.float32, 3)
    r["scaled_points"] = take(np.float32, 3 * n1).reshape(n1, 3)
    assert at[0] == len(b)
    return r


def same(got, want, what, nonfinite_by_kind=False, fields=FIELDS, scalars=SCALARS):
    """every byte; with nonfinite_by_kind (the zero_depth scenes) non-finite values are compared by position and kind -- isnan, isinf
    and the sign of an infinity -- because NaN payloads differ between hosts and the GPU"""
    for k in scalars:
        assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    for k, dt in fields:
        g, w = np.ascontiguousarray(got[k], dt).reshape(-1), np.ascontiguousarray(want[k], dt).reshape(-1)
        assert g.shape == w.shape, "%s: %s has another size" % (what, k)
        if nonfinite_by_kind and dt in (np.float32, np.float64):
            fin = np.isfinite(w)
            assert np.array_equal(np.isfinite(g), fin) and np.array_equal(np.isnan(g), np.isnan(w)), "%s: %s non-finite pattern" % (what, k)
            assert np.array_equal(np.sign(g[np.isinf(g)]), np.sign(w[np.isinf(w)])), "%s: %s sign of infinity" % (what, k)
            g, w = g[fin], w[fin]
        assert g.tobytes() == w.tobytes(), "%s: %s differs" % (what, k)


def same_adaptor_step(got, want, sc, what, inertial=False):
    """the program's median depth and rescale against the numpy restatement of the adaptor's host step, applied to the restatement's
    own results"""
    ok, t2, pts, med = R.median_depth_scale(want, sc["Rcw1"], sc["tcw1"], sc["matches12"], inertial)
    assert got["ok"] == ok, "%s: ok" % what
    assert np.array_equal(np.isnan(got["median"]), np.isnan(med)) and (np.isnan(med) or np.float32(got["median"]).tobytes() == med.tobytes())
    fin = np.isfinite(pts)
    assert np.array_equal(np.isfinite(got["scaled_points"]), fin)
    assert got["scaled_points"][fin].tobytes() == pts[fin].tobytes(), "%s: scaled points" % what
    assert got["scaled_tcw2"].tobytes() == t2.tobytes(), "%s: scaled tcw2" % what


def test_initial_ba_program_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


# what the adaptor's host step returns on each case: every return of InitialMapAdjuster::MedianDepthScale is taken by one of them
ADAPTOR_STEP = {("general", 65, 0): "scaled", ("outliers", 63, 0): "scaled", ("far", 65, 0): "scaled", ("zero_depth", 257, 0): "scaled",
                ("unmatched", 64, 0): "scaled", ("general", 1, 0): "few", ("general", 2, 0): "few", ("behind", 257, 0): "negative",
                ("nan_depth", 257, 0): "nan", ("general", 257, 0): "scaled", ("general_pose1", 65, 0): "scaled", ("far", 1025, 0): "scaled"}


def check_adaptor_step(got, case, sc, inertial=False):
    """the program's result of the adaptor's host step against its numpy restatement, and the return the case is there for: scaled
    (true), few (N < 50), negative (median < 0: a median of exactly 0 would scale), nan (a NaN depth)"""
    want = BS.ref_cached(case)
    same_adaptor_step(got, want, sc, BS.case_id(case), inertial)
    ok, _, _, med = R.median_depth_scale(want, sc["Rcw1"], sc["tcw1"], sc["matches12"], inertial)
    kind = ADAPTOR_STEP[case]
    assert got["ok"] == (kind == "scaled")
    if kind == "few":
        assert want["N"] < 50 and got["median"] > 0
    if kind == "negative":
        assert want["N"] >= 50 and got["median"] < 0 and got["scaled_points"].tobytes() == got["points"].tobytes()
    if kind == "nan":
        assert want["N"] >= 50 and np.isnan(got["median"]) and np.isnan(got["points"]).sum() == 1


@pytest.mark.parametrize("case", BS.HOST_CASES, ids=BS.case_id)
def test_host_loop_equals_restatement_under_sanitizers(built, tmp_path, case):
    """the program's own S17, built with AddressSanitizer and UBSan, against initial_ba_ref.initial_bundle_adjustment: every byte, no
    GPU.  The median-depth step is the adaptor's own text (InitialMapAdjuster::MedianDepthScale, called on the host loop's results)
    against its numpy restatement; the cases take each of its returns: true, N < 50 (general N = 1), median < 0 (behind), a NaN depth
    (nan_depth)."""
    exe = _build(san=True)
    sc = BS.make_case(case)
    write_scene(tmp_path / "scene.bin", sc)
    subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"])
    got = read_result(tmp_path / "out.bin", len(sc["kp1_xy"]))
    same(got, BS.ref_cached(case), BS.case_id(case), case[0] in BS.NONFINITE)
    check_adaptor_step(got, case, sc)


def test_median_of_zero_is_not_negative():
    """the boundary of `median < 0` in the numpy restatement the C++ is compared with: a median of exactly 0 is not refused"""
    sc = BS.make_case(("general", 65, 0))
    out = dict(BS.ref_cached(("general", 65, 0)))
    out["points"] = out["points"].copy()
    idx = np.flatnonzero(sc["matches12"] >= 0)
    z = out["points"][idx, 2].copy()
    out["points"][idx, 2] = z - np.sort(z)[(len(z) - 1) // 2]   # pose 1 is the identity: depth = Z
    with np.errstate(all="ignore"):
        ok, _, _, med = R.median_depth_scale(out, sc["Rcw1"], sc["tcw1"], sc["matches12"])
    assert med == 0 and ok


@pytest.mark.gpu
def test_initial_ba_program_equals_library_and_restatement(built, tmp_path):
    """the library through InitialMapAdjuster::Adjust, the host loop and the restatement agree, and Adjust takes each of its returns"""
    exe = _build()
    for case, inertial in ((("general", 257, 0), False), (("general_pose1", 65, 0), True), (("far", 1025, 0), False), (("general", 2, 0), False),
                           (("behind", 257, 0), False), (("nan_depth", 257, 0), True)):
        sc = BS.make_case(case)
        write_scene(tmp_path / "scene.bin", sc, inertial=inertial)
        out = subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "5"]).decode()
        print(out)
        assert re.search(r"initial_ba_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) host_same=1", out), out
        got = read_result(tmp_path / "out.bin", len(sc["kp1_xy"]))
        same(got, BS.ref_cached(case), BS.case_id(case), case[0] in BS.NONFINITE)
        check_adaptor_step(got, case, sc, inertial)

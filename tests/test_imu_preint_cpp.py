"""tests/cpp/imu_preint.cpp: IMU preintegration, state prediction and the inertial links (SPEC DECISION S22) from a plain C++ program.
The program carries the single-thread host loop -- the kernel's own text (csrc/imu_preint_math.h) run item by item; imu_preint_ref.py is
the independent oracle of both.  The host loop is built stand-alone with -fsanitize=address,undefined (a program with its own main,
never loaded into Python) and compared with the numpy restatement byte for byte without a GPU, on one scene of every kind and both link
kinds; so is the 9 x 9 L D L^T inverse (against the restatement by bytes, against numpy to a stated residual).  On the GPU the
library's results must equal both."""
import re
import subprocess

import numpy as np
import pytest

import cpp_build
import imu_preint_ref as R
import imu_preint_scenarios as PS

LINK_KF_FLOATS = ("Rwb1", "twb1", "v1", "bg1", "ba1", "dR", "dV", "dP", "dt", "Rcb", "tcb", "tbc")
LINK_FREE_FLOATS = ("Rwb1", "twb1", "v1", "bg1", "ba1", "dR0", "dV0", "dP0", "bg0", "ba0", "JRg", "JVg", "JVa", "JPg", "JPa", "dt", "Rcb",
                    "tcb", "tbc")
SAMPLE = np.dtype([("t", "<f8"), ("a", "<f4", 3), ("w", "<f4", 3)])


def _build(san=False, opt="-O2"):
    return cpp_build.build("imu_preint", san, opt)


def link_bytes(link, which):
    """orbfe_imu_link / orbfe_imu_link_free whole: struct_size, reserved, the floats, the doubles"""
    if which == R.FROM_FRAME:
        fl = np.concatenate([np.asarray(link[k], np.float32).reshape(-1) for k in LINK_FREE_FLOATS] + [np.zeros(1, np.float32)])
        assert len(fl) == 104
    else:
        fl = np.concatenate([np.asarray(link[k], np.float32).reshape(-1) for k in LINK_KF_FLOATS])
        assert len(fl) == 52
    db = np.concatenate([np.asarray(link[k], np.float64).reshape(-1) for k in ("info9", "infoG", "infoA")])
    return np.array([8 + fl.nbytes + db.nbytes, 0], np.int32).tobytes() + fl.tobytes() + db.tobytes()


def samples_of(sc):
    s = np.zeros(len(sc["t"]), SAMPLE)
    s["t"], s["a"], s["w"] = sc["t"], sc["a"], sc["w"]
    return s


def write_scene(path, sc, which):
    s1 = sc["state_frame"] if which == R.FROM_FRAME else sc["state_kf"]
    with open(path, "wb") as f:
        f.write(np.array([len(sc["t"]), which, sc["kf"].n_steps], np.int32).tobytes())
        f.write(np.array([sc["t_prev"], sc["t_cur"]], np.float64).tobytes())
        f.write(np.concatenate([sc["noise"].cov, sc["noise"].walk, sc["frame_bias"], s1, [sc["gravity"]], sc["Rcb"].reshape(9), sc["tcb"],
                                sc["tbc"]]).astype(np.float32).tobytes())
        f.write(sc["kf"].floats().astype(np.float32).tobytes())
        f.write(samples_of(sc).tobytes())


def read_result(path, which):
    b = open(path, "rb").read()
    at = [0]

    def take(dt, cnt):
        a = np.frombuffer(b, dt, cnt, at[0])
        at[0] += a.nbytes
        return a
    r = dict(zip(("n_steps", "info_ok", "kf_steps", "frame_steps"), (int(v) for v in take(np.int32, 4))))
    r["kf"], r["frame"], r["re"] = take(np.float32, 298), take(np.float32, 298), take(np.float32, 298)
    r["steps"] = take(np.float32, 8 * r["n_steps"]).reshape(-1, 8)
    r["state"] = take(np.float32, 33)
    r["link"] = b[at[0]:]
    assert len(r["link"]) == (424 + 99 * 8 if which == R.FROM_FRAME else 216 + 99 * 8)
    return r


def same(got, want, sc, which, what):
    """every byte of every output against the restatement's (imu_preint_scenarios.ref_cached)"""
    assert got["n_steps"] == len(want["steps"]) == sc["n"], what
    assert got["info_ok"] == int(want["ok"]), "%s: info_ok %d" % (what, got["info_ok"])
    assert got["kf_steps"] == want["kf"].n_steps and got["frame_steps"] == want["frame"].n_steps, what
    assert got["steps"].tobytes() == want["steps"].astype(np.float32).tobytes(), "%s: steps differ" % what
    for k, rec in (("kf", want["kf"]), ("frame", want["frame"]), ("re", want["frame"])):
        g, w = got[k], rec.floats().astype(np.float32)
        assert g.tobytes() == w.tobytes(), "%s: record %s differs at floats %s" % (what, k, np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))[:8])
    assert got["state"].tobytes() == want["state"].astype(np.float32).tobytes(), "%s: the predicted state differs" % what
    assert got["link"] == link_bytes(want["link"], which), "%s: the link differs" % what


def test_imu_preint_program_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def test_ldlt_inverse_9_under_sanitizers(built, tmp_path):
    """the 9 x 9 L D L^T inverse of preint_info9 on covariance-like symmetric positive definite matrices (entries spanning 1e-12 ..
    1e-4, as C.block<9,9> does) and on one with a negative leading entry.  Against the restatement by bytes; against the identity to a
    relative residual |A x - e| / (|A| |x| + |e|) <= 9 * 2^-52 for every column (n eps, as test_ldlt_solve_30_...: without pivoting the
    factorisation is backward stable for a positive definite matrix)."""
    rng = np.random.RandomState(5)
    mats = []
    for rep in range(6):
        M = rng.normal(size=(9, 9))
        d = 10.0 ** rng.uniform(-6, -2, 9)
        A = (M @ M.T / 9.0 + np.eye(9)) * d[:, None] * d[None, :]
        if rep == 5:
            A[0, 0] = -A[0, 0]
        mats.append(((A + A.T) / 2.0).astype(np.float32))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(mats)], np.int32).tobytes() + b"".join(A.tobytes() for A in mats))
    subprocess.check_call([_build(san=True), "inv9", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == len(mats) * 652
    for i, A in enumerate(mats):
        X = np.frombuffer(raw, np.float64, 81, i * 652).reshape(9, 9)
        ok = int(np.frombuffer(raw, np.int32, 1, i * 652 + 648)[0])
        Xr, okr = R.ldlt_inverse9(A.astype(np.float64))
        assert X.tobytes() == Xr.tobytes() and ok == int(okr) == int(i != 5)
        Ad = np.triu(A.astype(np.float64)) + np.triu(A.astype(np.float64), 1).T
        if i != 5:
            for c in range(9):
                e = np.zeros(9)
                e[c] = 1.0
                res = np.linalg.norm(Ad @ X[:, c] - e) / (np.linalg.norm(Ad) * np.linalg.norm(X[:, c]) + 1.0)
                print("matrix %d column %d: residual %.3g" % (i, c, res))
                assert res <= 9 * 2.0 ** -52
            assert np.allclose(X, np.linalg.inv(Ad), rtol=1e-7)


@pytest.mark.parametrize("which", (R.FROM_KEYFRAME, R.FROM_FRAME), ids=("keyframe", "frame"))
@pytest.mark.parametrize("case", PS.HOST_CASES, ids=PS.case_id)
def test_host_loop_equals_restatement_under_sanitizers(built, tmp_path, case, which):
    """the program's own S22, built with AddressSanitizer and UBSan, against imu_preint_ref: every byte, no GPU"""
    exe = _build(san=True)
    sc = PS.make(*case)
    write_scene(tmp_path / "scene.bin", sc, which)
    subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"])
    same(read_result(tmp_path / "out.bin", which), PS.ref_cached(case, which), sc, which, PS.case_id(case))


@pytest.mark.gpu
def test_imu_preint_program_equals_library_and_restatement(built, tmp_path):
    exe = _build()
    for case, which in ((("moving", 10, 0), R.FROM_KEYFRAME), (("moving", R.CHUNK + 1, 0), R.FROM_FRAME), (("bias_changed", 10, 0), R.FROM_KEYFRAME),
                        (("clamped", 3, 0), R.FROM_KEYFRAME)):
        sc = PS.make(*case)
        write_scene(tmp_path / "scene.bin", sc, which)
        out = subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "3"]).decode()
        print(out)
        assert re.search(r"imu_preint_latency_us call=([0-9.]+) host_one_thread=([0-9.]+) steps=%d host_same=1" % case[1], out), out
        assert "imu_preint_adaptor_same=1" in out, out   # include/orbfe_adaptor.hpp's ImuPreintegrator gives the library's bytes
        same(read_result(tmp_path / "out.bin", which), PS.ref_cached(case, which), sc, which, PS.case_id(case))

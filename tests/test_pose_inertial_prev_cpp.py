"""tests/cpp/pose_inertial_prev.cpp: Optimizer::PoseInertialOptimizationLastFrame from a plain C++ program through the C ABI.  The
program carries the single-thread host loop of SPEC DECISION S20 -- the kernel's own text (csrc/poseimu_prev_math.h, csrc/marginalize.h)
run item by item, with ldlt.h's indexed ldlt_solve_n<30>; pose_inertial_prev_ref.py is the independent oracle of both.  The host loop
is built stand-alone with -fsanitize=address,undefined (a program with its own main, never loaded into Python) and compared with the
numpy restatement byte for byte without a GPU, on one case of every kind; so are ldlt_solve_n<30> (against numpy.linalg.solve, to a
stated residual) and orbfe_marginalize_pose_imu (against the restatement, by bytes, threshold branch included).  On the GPU the
library's results must equal both."""
import re
import subprocess

import numpy as np
import pytest

import cpp_build
import pose_inertial_prev_ref as R
import pose_inertial_prev_scenarios as PS

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<i4"), ("size", "<f4"), ("octave", "<i4"), ("angle", "<f4")])
LINK_FLOATS = ("Rwb1", "twb1", "v1", "bg1", "ba1", "dR0", "dV0", "dP0", "bg0", "ba0", "JRg", "JVg", "JVa", "JPg", "JPa", "dt", "Rcb", "tcb",
               "tbc")
PRIOR_FIELDS = ("Rwb", "twb", "vwb", "bg", "ba", "H")
SCALARS = ("n_inliers", "accepted", "N_e", "rounds_run", "recovered")


def _build(san=False, opt="-O2"):
    return cpp_build.build("pose_inertial_prev", san, opt)


def link_bytes(link):
    """orbfe_imu_link_free behind its two leading ints"""
    fl = np.concatenate([np.asarray(link[k], np.float32).reshape(-1) for k in LINK_FLOATS] + [np.zeros(1, np.float32)])
    assert len(fl) == 104
    return fl.tobytes() + np.concatenate([np.asarray(link[k], np.float64).reshape(-1) for k in ("info9", "infoG", "infoA")]).tobytes()


def prior_bytes(prior):
    """orbfe_pose_imu_prior behind its two leading ints"""
    d = np.concatenate([np.asarray(prior[k], np.float64).reshape(-1) for k in PRIOR_FIELDS])
    assert len(d) == 246
    return d.tobytes()


def state_in(sc):
    return np.concatenate([np.asarray(sc[k], np.float32).reshape(-1) for k in ("Rcw", "tcw", "Rwb", "twb", "v", "bg", "ba")])


def write_scene(path, sc, **kw):
    prm = dict(R.PARAMS)
    prm.update(kw)
    kp = np.zeros(len(sc["kp_xy"]), KP)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    s2 = np.asarray(sc["level_sigma2"], np.float32)
    with open(path, "wb") as f:
        f.write(np.array([len(kp), len(sc["points"]), len(s2), prm["iterations"], prm["rounds"], prm["rec_init"], prm["recover_below"],
                          prm["inlier_threshold"]], np.int32).tobytes())
        f.write(np.array([prm["huber_delta2"], prm["close_factor"], prm["prior_huber_delta"]], np.float64).tobytes())
        f.write(np.concatenate([sc["cam"], prm["chi2"], [prm["close_depth"], prm["recover_chi2"], prm["gravity"]]]).astype(np.float32).tobytes())
        f.write((np.float32(1.0) / s2).astype(np.float32).tobytes())
        f.write(link_bytes(sc["link"]))
        f.write(prior_bytes(sc["prior"]))
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
    r = dict(zip(SCALARS, (int(v) for v in take(np.int32, 5))))
    nr, Ne = r["rounds_run"], r["N_e"]
    for k in ("round_iterations", "round_ok", "round_nbad"):
        r[k] = take(np.int32, 4)[:nr]
    st = take(np.float32, 21)
    r.update(Rwb=st[:9], twb=st[9:12], v=st[12:15], bg=st[15:18], ba=st[18:21])
    r["H30"] = take(np.float64, 900).reshape(30, 30)
    r["Hprior"] = take(np.float64, 225).reshape(15, 15)
    r["outlier"] = take(np.uint8, n)
    r["round_state"] = take(np.float64, 4 * 42).reshape(4, 42)[:nr]
    r["round_prior_chi2"] = take(np.float64, 4)[:nr]
    r["round_prior_weight"] = take(np.float64, 4)[:nr]
    r["round_outlier"] = take(np.uint8, 4 * Ne).reshape(4, Ne)[:nr]
    assert at[0] == len(b)
    return r


FIELDS = (("Rwb", np.float32), ("twb", np.float32), ("v", np.float32), ("bg", np.float32), ("ba", np.float32), ("H30", np.float64),
          ("Hprior", np.float64), ("outlier", np.uint8), ("round_state", np.float64), ("round_prior_chi2", np.float64),
          ("round_prior_weight", np.float64), ("round_iterations", np.int32), ("round_ok", np.int32), ("round_nbad", np.int32),
          ("round_outlier", np.uint8))


def same(got, want, what, nonfinite_by_kind=False, fields=FIELDS, scalars=SCALARS):
    """every byte of every output and every info field; with nonfinite_by_kind (the zero_depth scenes) non-finite values are compared
    by position and kind -- isnan, isinf and the sign of an infinity -- because NaN payloads differ between hosts and the GPU"""
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


def test_pose_inertial_prev_program_links(built):
    assert "gfx950" in subprocess.check_output([_build()]).decode()


def test_ldlt_solve_30_on_permuted_spd_under_sanitizers(built, tmp_path):
    """ldlt_solve_n<30> on symmetric positive definite matrices whose diagonal is out of order (so that every step pivots) and on one
    indefinite matrix.  Against numpy: the restatement's solve by bytes; numpy.linalg.solve to a relative residual
    |A x - b| / (|A| |x| + |b|) <= 30 * 2^-52 (n eps: a backward-stable factorisation of a 30 x 30)."""
    rng = np.random.RandomState(3)
    systems = []
    for rep in range(6):
        M = rng.normal(size=(30, 30))
        A = M @ M.T + 30.0 * np.diag(rng.uniform(0.1, 10.0, 30) ** 2)
        p = rng.permutation(30)
        A = A[p][:, p]
        if rep == 5:
            A[7, 7] = -A[7, 7]   # indefinite: a pivot is not positive
        A = (A + A.T) / 2.0
        systems.append((A, rng.normal(size=30)))
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(systems)], np.int32).tobytes())
        for A, b in systems:
            f.write(A.tobytes() + b.tobytes())
    subprocess.check_call([_build(san=True), "ldlt30", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == len(systems) * 244
    for i, (A, b) in enumerate(systems):
        x = np.frombuffer(raw, np.float64, 30, i * 244)
        pos = int(np.frombuffer(raw, np.int32, 1, i * 244 + 240)[0])
        xr, okr = R.ldlt_solve(A, b)
        assert x.tobytes() == xr.tobytes() and pos == int(okr) == int(i != 5)
        res = np.linalg.norm(A @ x - b) / (np.linalg.norm(A) * np.linalg.norm(x) + np.linalg.norm(b))
        print("system %d: residual %.3g" % (i, res))
        assert res <= 30 * 2.0 ** -52
        assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)


def constructed_hessians():
    """30 x 30 matrices whose Hbb has one eigenvalue below 1e-6, one eigenvalue exactly 0, and Hbb = 0 (the result is Hcc)"""
    rng = np.random.RandomState(11)
    out = {}
    for name, small in (("below_threshold", 3e-7), ("exact_zero", 0.0)):
        M = rng.normal(size=(30, 30))
        Hm = M @ M.T + np.eye(30)
        lam = rng.uniform(0.5, 50.0, 15)
        lam[4] = small
        if small == 0.0:   # a diagonal Hbb: the zero is exact and no rotation touches it
            Hm[:15, :15] = np.diag(lam)
            Hm[4, 15:] = Hm[15:, 4] = 0.0
        else:
            Q, _ = np.linalg.qr(rng.normal(size=(15, 15)))
            Hm[:15, :15] = (Q * lam[None, :]) @ Q.T
        out[name] = (Hm + Hm.T) / 2.0
    M = rng.normal(size=(30, 30))
    Hz = M @ M.T
    Hz[:15, :15] = 0.0
    out["all_zero"] = Hz
    return out


def test_marginalize_equals_restatement_under_sanitizers(built, tmp_path):
    """orbfe_marginalize_pose_imu (the kernel epilogue's text on the host) against pose_inertial_prev_ref.marginalize by bytes: scene
    Hessians and the constructed ones that reach the |lambda| <= 1e-6 branch"""
    Hs = [PS.ref_cached(c)["H30"] for c in (("general", 257, 0), ("prior_far", 65, 0), ("rank_deficient_prior", 64, 0), ("few", 0, 0))]
    con = constructed_hessians()
    Hs += [con[k] for k in ("below_threshold", "exact_zero", "all_zero")]
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(Hs)], np.int32).tobytes() + b"".join(np.ascontiguousarray(H, np.float64).tobytes() for H in Hs))
    subprocess.check_call([_build(san=True), "marg", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(Hs), 15, 15)
    before = R.COUNTS["marg_below_threshold"]
    for i, H in enumerate(Hs):
        assert got[i].tobytes() == R.marginalize(H).tobytes(), i
    assert R.COUNTS["marg_below_threshold"] - before == 3   # the three constructed matrices, and no scene
    assert got[6].tobytes() == np.ascontiguousarray(con["all_zero"][15:, 15:]).tobytes()   # Hbb = 0: Hp = Hcc - 0
    lam = np.linalg.eigvalsh(con["below_threshold"][:15, :15])
    assert 0.0 < lam[0] < 1e-6 < lam[1]
    # the dropped direction matters: the literal SVD form agrees, a plain inverse does not
    for k in ("below_threshold", "exact_zero"):
        ms = R.marginalize_svd(con[k])[15:, 15:]
        g = got[4 if k == "below_threshold" else 5]
        assert np.linalg.norm(g - ms) / np.linalg.norm(ms) < 1e-12


@pytest.mark.parametrize("case", PS.HOST_CASES, ids=PS.case_id)
def test_host_loop_equals_restatement_under_sanitizers(built, tmp_path, case):
    """the program's own S20, built with AddressSanitizer and UBSan, against pose_inertial_prev_ref: every byte, no GPU"""
    exe = _build(san=True)
    sc = PS.make_case(case)
    write_scene(tmp_path / "scene.bin", sc, **PS.case_kw(case))
    subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "host"])
    same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), PS.ref_cached(case), PS.case_id(case), case[0] == "zero_depth")


@pytest.mark.gpu
def test_pose_inertial_prev_program_equals_library_and_restatement(built, tmp_path):
    exe = _build()
    for case in (("general", 257, 0), ("outliers", 257, 0), ("prior_far", 65, 0), ("few", 0, 0)):
        sc = PS.make_case(case)
        write_scene(tmp_path / "scene.bin", sc)
        out = subprocess.check_output([exe, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin"), "3"]).decode()
        print(out)
        assert re.search(r"pose_inertial_prev_latency_us call=([0-9.]+) call_without_marginalisation=([0-9.]+) host_one_thread=([0-9.]+) "
                         r"host_same=1", out), out
        assert "pose_inertial_prev_adaptor_same=1" in out, out   # the adaptor's wrapper: 1000 without a prior, applied only when accepted
        same(read_result(tmp_path / "out.bin", len(sc["kp_xy"])), PS.ref_cached(case), PS.case_id(case))

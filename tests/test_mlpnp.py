"""SPEC DECISION S13 (mlpnp_ref.ransac: the pinned sequences) measured against the same function on numpy.linalg.svd / eigh / solve
and numpy's sin / cos / arccos / cbrt (mlpnp_ref.ransac_f64) on the scenes of mlpnp_scenarios, and the properties S13 states about
itself: the Jacobian against central differences, the pinned functions against numpy, the sweep count, which exits and branches
the scenes reach, orbfe_mlpnp_plan against the formula.  No GPU: the kernels are compared with `ransac` byte for byte in
test_mlpnp_gpu.py.

Gates: DESIGN.md S13 records the worst values of the two measured seeds (0 and 1) over all scenes; every gate here is twice that
worst value -- a margin for the second seed pair the test adds (2 and 3), not for the kernels.  The discrete outcome (exit kind,
returning iteration, candidate list) must be equal."""
import functools
import os
import re

import numpy as np
import pytest

import mlpnp_ref as R
import mlpnp_scenarios as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 2, 3)
# measured worst over seeds 0 and 1 x MS.CASES -> gate = 2 x worst: share of N of flipped inlier flags (the call's
# and, per hypothesis, the count difference), angle between the two returned rotations (degrees, from the Frobenius distance) and
# distance between the two returned translations -- of Tcw, the binary32 pose the call returns: the poses agree in every entry
# except entries near zero of the identity / near-identity scenes.  (The binary64 poses behind them differ by rounding noise, at
# most 1.4e-13 degrees and 2.4e-14 over all four seeds; the maximum of such noise over a few scenes is no stable figure, so it
# is printed, not gated.)
WORST = dict(flips=0.0, hyp_flips=0.0, rot_deg=5.19e-14, t_dist=1.13e-14)
GATE = {k: 2.0 * v for k, v in WORST.items()}


def returned_pose(o):
    """the binary64 pose behind the call's Tcw"""
    if o["exit_kind"] == R.EXIT_REFINED:
        return o["cand_Rt"][list(o["candidates"]).index(o["returning_iteration"])]
    return o["hyp_Rt"][o["returning_iteration"]]


def compare(s, e):
    m = dict(same_exit=s["exit_kind"] == e["exit_kind"], same_it=s["returning_iteration"] == e["returning_iteration"],
             same_cands=list(s["candidates"]) == list(e["candidates"]), flips=0.0, hyp_flips=0.0, rot_deg=0.0, t_dist=0.0)
    if s["N"] == 0 or s["total_iterations"] == 0:
        return m
    m["flips"] = float((s["inliers"] != e["inliers"]).sum()) / s["N"]
    m["hyp_flips"] = float(np.abs(s["hyp_inliers"].astype(np.int64) - e["hyp_inliers"]).max()) / s["N"]
    if s["solved"] and e["solved"] and m["same_exit"] and m["same_it"]:
        a, b = s["Tcw"].astype(np.float64), e["Tcw"].astype(np.float64)
        m["rot_deg"] = float(np.degrees(np.linalg.norm(a[:3, :3] - b[:3, :3]) / np.sqrt(2.0)))
        m["t_dist"] = float(np.linalg.norm(a[:3, 3] - b[:3, 3]))
        a, b = returned_pose(s), returned_pose(e)
        m["rot_deg64"] = float(np.degrees(np.linalg.norm(a[:9] - b[:9]) / np.sqrt(2.0)))
        m["t_dist64"] = float(np.linalg.norm(a[9:] - b[9:]))
    return m


@functools.lru_cache(maxsize=None)
def figures(case, seed):
    sc = MS.make(case[0], case[1], seed, case[2], case[3], case[4])
    return compare(MS.ref(sc), MS.ref(sc, exact=True))


@pytest.mark.parametrize("seed", SEEDS)
def test_distance_to_binary64(seed):
    worst = {k: 0.0 for k in GATE}
    for case in MS.CASES:
        m = figures(case, seed)
        assert m["same_exit"] and m["same_it"] and m["same_cands"], (MS.case_id(case), seed, m)
        for k in GATE:
            worst[k] = max(worst[k], m[k])
        for k in ("rot_deg64", "t_dist64"):
            worst[k] = max(worst.get(k, 0.0), m.get(k, 0.0))
    print("seed %d worst: %s" % (seed, worst))
    for k in GATE:
        assert worst[k] <= GATE[k], (k, worst[k], GATE[k])


@functools.lru_cache(maxsize=None)
def refs():
    return [MS.ref(MS.make_case(c)) for c in MS.CASES]


def test_scenes_reach_every_exit_and_branch():
    outs = refs()
    assert {o["exit_kind"] for o in outs} == {R.EXIT_ABORT, R.EXIT_REFINED, R.EXIT_BEST, R.EXIT_FAILED}
    assert {int(p) for o in outs for p in o["hyp_planar"]} == {0, 1} and {int(p) for o in outs for p in o["cand_planar"]} == {0, 1}
    assert {int(k) for o in outs for k in o["hyp_gn_exit"]} >= {R.GN_SPURIOUS, R.GN_CONVERGED}
    # a second or later candidate is the one that returns
    assert any(o["exit_kind"] == R.EXIT_REFINED and o["n_candidates"] >= 2 and o["returning_iteration"] != o["candidates"][0] for o in outs)
    # N == min_inliers: one planned iteration, twenty run, the clean scene qualifies, fails Refine's strict '>' and leaves unrefined
    o = outs[[MS.case_id(c) for c in MS.CASES].index("general-N50-o0-s12-e50-seed0")]
    assert (o["min_inliers"], o["max_its"], o["total_iterations"]) == (50, 1, 20) and o["exit_kind"] == R.EXIT_BEST and o["cand_inliers"].max() == 50
    assert {o["total_iterations"] for o in outs} >= {0, 20, 23, 300}


def test_sweep_count():
    """S13 fixes 12 sweeps: on the scenes nothing changes from 7 sweeps on (checked here at 7 and 9 against 12 on
    three scenes, the planar one among them)"""
    for case in (MS.CASES[0], MS.CASES[2], MS.CASES[5]):
        sc = MS.make_case(case)
        b = MS.ref(sc)
        for sweeps in (7, 9):
            a = MS.ref(sc, sweeps=sweeps)
            assert a["hyp_Rt"].tobytes() == b["hyp_Rt"].tobytes() and a["cand_Rt"].tobytes() == b["cand_Rt"].tobytes(), (MS.case_id(case), sweeps)


def test_jacobian_against_central_differences():
    rng = np.random.RandomState(3)
    B, n = 6, 7
    X = rng.uniform(-2, 2, (B, n, 3)) + np.array([0, 0, 6.0])
    f = rng.uniform(-0.5, 0.5, (B, n, 3))
    f[..., 2] = 1.0
    nr, ns = R.null_space(f)
    x = np.concatenate([rng.uniform(-1.5, 1.5, (B, 3)), rng.uniform(-0.5, 0.5, (B, 3))], 1)
    x[0, :3] = (np.pi - 1e-4) * np.array([0.6, 0.0, 0.8])  # near pi
    x[1, :3] = 1e-6 * np.array([1.0, -2.0, 0.5])           # near 0
    r, J = R.residuals_and_jacs(x, X, nr, ns)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        num = (R.residuals_and_jacs(x + d, X, nr, ns, exact=True)[0] - R.residuals_and_jacs(x - d, X, nr, ns, exact=True)[0]) / (2 * h)
        # central differences in binary64: truncation h^2 |f'''| / 6 ~ 1e-12, rounding eps |r| / h ~ 1e-10 -> 1e-8 is a safe bound
        assert np.abs(num - J[:, :, k]).max() < 1e-8, (k, np.abs(num - J[:, :, k]).max())
    # omega = 0: S13 takes the limit dR/dw_k = [e_k]x, which is the derivative there
    x0 = np.zeros((1, 6))
    J0 = R.residuals_and_jacs(x0, X[:1], nr[:1], ns[:1])[1]
    for k in range(3):
        d = np.zeros(6)
        d[k] = h
        num = (R.residuals_and_jacs(x0 + d, X[:1], nr[:1], ns[:1], exact=True)[0] - R.residuals_and_jacs(x0 - d, X[:1], nr[:1], ns[:1], exact=True)[0]) / (2 * h)
        assert np.isfinite(J0).all() and np.abs(num - J0[:, :, k]).max() < 1e-8


def test_null_space_is_orthonormal_and_orthogonal_to_the_bearing():
    rng = np.random.RandomState(5)
    f = rng.uniform(-1.5, 1.5, (1000, 3))
    f[:, 2] = 1.0
    r, s = R.null_space(f)
    fn = f / np.linalg.norm(f, axis=1)[:, None]
    for a, b, want in ((r, fn, 0), (s, fn, 0), (r, s, 0), (r, r, 1), (s, s, 1)):
        assert np.abs((a * b).sum(1) - want).max() < 8 * R.EPS


def _ulp(a, b):
    return float(np.max(np.abs(a - b) / np.spacing(np.abs(b))))


def test_pinned_functions_against_numpy():
    """each sequence is a polynomial whose truncation error is below 0.01 ulp, evaluated with a handful of roundings whose last
    three (the final multiply-add of Horner and the reconstruction) dominate: at most 2 ulp from the true value, numpy within 1"""
    x = np.linspace(0.0, np.pi, 200001)
    s, c = R.sincos64(x)
    assert _ulp(s[1:-1], np.sin(x[1:-1])) <= 3.0
    assert np.abs(c - np.cos(x)).max() <= 2 * R.EPS and np.abs(s - np.sin(x)).max() <= 2 * R.EPS
    big = np.random.RandomState(0).uniform(0, 100, 100000)
    s, c = R.sincos64(big)
    assert np.abs(s - np.sin(big)).max() <= 2 * R.EPS and np.abs(c - np.cos(big)).max() <= 2 * R.EPS
    y = np.concatenate([np.linspace(-1, 1, 400001)[1:-1], 1 - np.logspace(-16, -1, 1000), np.logspace(-16, -1, 1000) - 1])
    assert _ulp(R.acos64(y), np.arccos(y)) <= 3.0
    assert R.acos64(np.array([1.0]))[0] == 0.0 and R.acos64(np.array([-1.0]))[0] == np.pi and np.isnan(R.acos64(np.array([1.0 + 1e-9]))[0])
    z = 10.0 ** np.random.RandomState(1).uniform(-300, 300, 200000)
    assert _ulp(R.cbrt64(z), np.cbrt(z)) <= 3.0
    assert R.cbrt64(np.array([0.0]))[0] == 0.0 and R.cbrt64(np.array([27.0]))[0] == 3.0


def test_device_tables_are_the_restatements():
    """spec_math.h and mlpnp_ref.py share their constants"""
    txt = open(os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc", "spec_math.h")).read()

    def table(name):
        body = re.search(r"constexpr double %s\[\d+\] = \{([^}]*)\}" % name, txt).group(1)
        return [float.fromhex(v.strip()) for v in body.split(",")]

    def scalar(name):
        return float.fromhex(re.search(r"\b%s = (-?0x[0-9a-fp.+-]+)" % name, txt).group(1))

    assert table("kSinC") == R.SIN_C and table("kCosC") == R.COS_C and table("kAsinC") == R.ASIN_C
    assert [scalar(n) for n in ("kTwoOverPi", "kPio2_1", "kPio2_2", "kPio2_3", "kPio2Hi", "kPio2Lo", "kPiHi", "kPiLo")] == [
        R.TWO_OVER_PI, R.PIO2_1, R.PIO2_2, R.PIO2_3, R.PIO2_HI, R.PIO2_LO, R.PI_HI, R.PI_LO]
    jac = open(os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc", "jacobi.h")).read()
    assert int(re.search(r"kMlpnpSweeps = (\d+)", jac).group(1)) == R.SWEEPS12
    hip = open(os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc", "kernels_mlpnp.hip")).read()
    assert int(re.search(r"kMlpnpRefineThreads = (\d+)", hip).group(1)) == MS.REFINE_BLOCK


def test_plan_against_the_formula(built):
    """orbfe_mlpnp_plan (host only) for every N from 0 to 4000 at the call site's parameters and at epsilon 0.2"""
    import orbfe
    for eps in (0.5, 0.2):
        P = orbfe.MlpnpParams(epsilon=eps)
        for N in range(0, 4001):
            assert orbfe.mlpnp_plan(P, N) == R.plan(N, epsilon=eps), (eps, N)
    P = orbfe.MlpnpParams()
    P.struct_size -= 4
    with pytest.raises(orbfe.OrbfeError):
        orbfe.mlpnp_plan(P, 100)
    for bad in (dict(min_set=5), dict(min_set=65), dict(epsilon=0.0), dict(probability=1.0), dict(max_iterations=0)):
        with pytest.raises(orbfe.OrbfeError):
            orbfe.mlpnp_plan(orbfe.MlpnpParams(**bad), 100)

"""SPEC DECISION S14 (poseopt_ref.pose_optimization: Optimizer::PoseOptimization restated) checked against itself and against libraries,
without a GPU (the kernel is compared with the restatement byte for byte in test_poseopt_gpu.py):
  - the Jacobian against central differences of the residual under exp(eps e_k) . T;
  - the tree sum against math.fsum (the gap is printed, not gated: the tree is the definition);
  - the accepted costs, which must not increase within a round;
  - which exits and branches every scene of poseopt_scenarios reaches, so that no scene can silently stop covering its case;
  - the rotation's drift from orthonormal at every round's end (printed; the pose is kept as a matrix, S14);
  - the restatement against scipy.optimize.least_squares from the same start: round 0 against loss='huber', f_scale=delta on the
    whitened residuals, round 3 against loss='linear' on round 2's inlier set, and the inlier flags against the same four-round
    protocol run on scipy's poses.

Measured on seeds 0 and 1 of general / outliers / far at N_e = 300 (distances as degrees from the Frobenius distance of
the two rotations, and metres between the translations):
    round 0 vs huber    general 1.3e-09 deg 1.1e-10 m | outliers 5.2e-02 deg 7.1e-03 m | far 1.2e-09 deg 1.5e-10 m
    round 3 vs linear   general 6.7e-09 deg 7.5e-10 m | outliers 7.0e-10 deg 6.1e-11 m | far 1.3e-09 deg 1.4e-10 m
    flag flips over the four rounds (of 4 x 300)        general 0 | outliers 9 | far 0
scipy applies its Huber loss to every scalar residual, g2o to the edge's chi2 (the squared norm of its two residuals): with 30 % gross
outliers the two round-0 optima differ by the figures above; where no active edge sits in Huber's linear region at the optimum (general,
far, and round 3 everywhere) what remains is the two solvers' termination noise.
Gates (the project's rule from S13: twice the worst figure of seeds 0 and 1, to hold on seeds 2 and 3 as well):
  - round 0 and the flips PER KIND: the outliers figures are seven orders of magnitude above the other two kinds', so one gate over all
    kinds could not fail for general and far; the flips gate is the kind's worst count itself;
  - round 3 over the three kinds together: it is the same plain least-squares problem in every kind (round 2's inliers, no kernel), its
    figures are termination noise of one magnitude (2e-10 .. 7e-9 deg) with nothing kind-specific in them, and the maximum of such
    noise over two seeds of one kind is no stable figure (S13 met the same and did not gate it at all)."""
import functools
import math

import numpy as np
import pytest

import poseopt_ref as R
import poseopt_scenarios as PS

SEEDS = (0, 1, 2, 3)
KINDS = ("general", "outliers", "far")
# seeds 0 and 1, measured
WORST_R0 = {"general": dict(r0_deg=1.302e-9, r0_m=1.129e-10, flips=0), "outliers": dict(r0_deg=5.232e-2, r0_m=7.097e-3, flips=9),
            "far": dict(r0_deg=1.219e-9, r0_m=1.468e-10, flips=0)}
WORST_R3 = dict(r3_deg=6.669e-9, r3_m=7.536e-10)
GATE_R0 = {kind: {k: (v if k == "flips" else 2.0 * v) for k, v in w.items()} for kind, w in WORST_R0.items()}
GATE_R3 = {k: 2.0 * v for k, v in WORST_R3.items()}


def test_jacobian_against_central_differences():
    """J = d e / d xi at xi = 0 under T <- exp(xi) T.  Step h = 1e-6: the truncation term h^2 f''' / 6 is below 1e-9 for these scenes
    (|f'''| ~ fx times a few), the rounding term 2 eps |e| / h below 2e-7 for residuals of up to a few hundred pixels; the bound
    1e-6 max(1, |J|) leaves a factor of five."""
    sc = PS.make("general", 64, 0)
    first, obs, w, Xw = R.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
    R0, t0 = sc["Rcw"].astype(np.float64), sc["tcw"].astype(np.float64)
    _, _, x, y, z = R.residual(R0, t0, sc["cam"], obs, Xw)
    J0, J1 = R.jacobian(sc["cam"], x, y, z)
    h = 1e-6
    worst = 0.0
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Rp, tp = R.apply_update(d, R0, t0)
        Rm, tm = R.apply_update(-d, R0, t0)
        ep, em = R.residual(Rp, tp, sc["cam"], obs, Xw), R.residual(Rm, tm, sc["cam"], obs, Xw)
        for row, J in ((0, J0), (1, J1)):
            num = (ep[row] - em[row]) / (2 * h)
            err = np.abs(num - J[k]) / np.maximum(1.0, np.abs(J[k]))
            worst = max(worst, float(err.max()))
    print("Jacobian vs central differences: worst relative gap %.3g" % worst)
    assert worst < 1e-6


def test_tree_sum_against_fsum():
    rng = np.random.RandomState(3)
    for n in (1, 2, 3, 63, 64, 65, 300, 4097):
        v = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 6, n)
        t, exact = float(R.tree_sum(v)), math.fsum(v)
        print("tree sum n=%d: %.17g, fsum %.17g, gap %.3g (%.3g relative to sum |v|)" % (n, t, exact, t - exact, abs(t - exact) / np.abs(v).sum()))
    assert float(R.tree_sum(np.array([1.0, 2.0, 3.0]))) == (1.0 + 2.0) + (3.0 + 0.0)
    # the padding is +0.0 only up to P: a sum of -0.0 terms stays -0.0 when N_e is a power of two and turns +0.0 when it is not
    assert math.copysign(1.0, float(R.tree_sum(np.full(4, -0.0)))) == -1.0 and math.copysign(1.0, float(R.tree_sum(np.full(3, -0.0)))) == 1.0


@functools.lru_cache(maxsize=None)
def traced(case):
    R.COUNTS.clear()
    traces = []
    sc = PS.make_case(case)
    out = PS.ref(sc, traces=traces)
    return sc, out, traces, dict(R.COUNTS)


@pytest.mark.parametrize("case", PS.CASES, ids=PS.case_id)
def test_accepted_costs_do_not_increase_and_rotation_stays_orthonormal(case):
    sc, out, traces, _ = traced(case)
    for rnd, tr in enumerate(traces):
        fin = [c for c in tr if math.isfinite(c)]
        assert all(b <= a for a, b in zip(fin, fin[1:])), (PS.case_id(case), rnd, tr)
    for rnd, p in enumerate(out["round_pose"]):
        Rm = p[:9].reshape(3, 3)
        if np.isfinite(Rm).all():
            drift = float(np.linalg.norm(Rm @ Rm.T - np.eye(3)))
            print("%s round %d: |R R^T - I| = %.3g" % (PS.case_id(case), rnd, drift))
            # the caller's float rotation is orthonormal to binary32 rounding only (about 1e-7); the products add binary64 rounding
            assert drift < 1e-6


def test_scenes_reach_their_exits_and_branches():
    by = {c: traced(c) for c in PS.CASES}
    out = lambda c: by[c][1]
    cnt = lambda c: by[c][3]
    # the two early exits (:949, :1055) and the edge counts around them
    assert out(("general", 2, 0))["rounds_run"] == 0 and out(("general", 2, 0))["n_inliers"] == 0
    assert np.array_equal(out(("general", 2, 0))["Tcw"][:3, :3].reshape(-1), PS.make_case(("general", 2, 0))["Rcw"])
    assert out(("general", 3, 0))["rounds_run"] == 1 and out(("general", 9, 0))["rounds_run"] == 1
    assert all(out(("general", n, 0))["rounds_run"] == 4 for n in PS.NE_LIST if n >= 10)
    assert [out(("general", n, 0))["N_e"] for n in PS.NE_LIST] == PS.NE_LIST
    # converged: dx -> 0 reaches the small-theta branch of exp, and the pose stays where it started to binary32
    for c in (("converged", 64, 0), ("converged", 300, 0)):
        assert cnt(c).get("small_theta", 0) > 0
        sc = by[c][0]
        assert np.abs(out(c)["Tcw"][:3, :3].reshape(-1) - sc["Rcw"]).max() < 1e-6
    assert cnt(("general", 300, 0)).get("large_theta", 0) > 0
    # far: rejected trials (lambda grows) and Huber's linear region on the way
    for c in (("far", 65, 0), ("far", 300, 0), ("far", 1025, 0)):
        assert cnt(c).get("rejected", 0) > 0 and cnt(c).get("huber_linear_region", 0) > 0
        assert (out(c)["round_trials"] > out(c)["round_iterations"]).all()
    # outliers: a third of the matches are flagged and at least one flag changes twice over the rounds
    for c in (("outliers", 63, 24), ("outliers", 300, 1), ("outliers", 1000, 1)):
        ro = out(c)["round_outlier"].astype(int)
        assert (np.abs(np.diff(ro, axis=0)).sum(0) >= 2).any(), PS.case_id(c)
        assert 0.25 * c[1] < out(c)["round_nbad"][-1] < 0.5 * c[1]
    # huber_off: round 3 (no kernel) runs on the inlier set of round 2 and ends at another pose
    for c in (("huber_off", 300, 0), ("huber_off", 65, 0)):
        o = out(c)
        assert o["round_pose"][3].tobytes() != o["round_pose"][2].tobytes()
        assert (o["round_iterations"][3], o["round_trials"][3]) != (o["round_iterations"][2], o["round_trials"][2])
        assert cnt(c).get("huber_linear_region", 0) > 0
    # collapsed: H has rank 2.  With Levenberg's lambda > 0 the damped system keeps positive pivots, so the solve succeeds and the rounds
    # end on rho == 0 near the start; the !ok path is reached by zero_depth below and the 10-trial Terminate by general-N63
    for c in (("collapsed", 10, 0), ("collapsed", 300, 0)):
        assert cnt(c).get("not_ok", 0) == 0 and (out(c)["round_exit"] == R.EXIT_RHO_ZERO).all()
        assert out(c)["round_nbad"][-1] == 0
    assert (out(("general", 63, 0))["round_exit"] == R.EXIT_TRIALS).any()
    # behind: points with z < 0 at the initial pose take part like any other
    for c in (("behind", 64, 0), ("behind", 300, 0)):
        sc = by[c][0]
        first, obs, w, Xw = R.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
        z = R.residual(sc["Rcw"].astype(np.float64), sc["tcw"].astype(np.float64), sc["cam"], obs, Xw)[4]
        assert (z < 0).sum() >= c[1] // 6 and out(c)["rounds_run"] == 4
    # zero_depth: Xc.z == 0 exactly at the initial pose -> non-finite sums: every solve of round 0 fails (!ok), no trial is accepted, the
    # round runs all its iterations at the initial pose; the edge's chi2 is +inf there, so it is flagged and the later rounds are finite
    for c in (("zero_depth", 10, 0), ("zero_depth", 300, 0)):
        sc, o = by[c][0], out(c)
        first, obs, w, Xw = R.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
        z = R.residual(sc["Rcw"].astype(np.float64), sc["tcw"].astype(np.float64), sc["cam"], obs, Xw)[4]
        assert (z == 0.0).sum() == 1
        assert cnt(c).get("not_ok", 0) >= 25 and not math.isfinite(o["round_chi2"][0])
        assert o["round_exit"][0] == R.EXIT_RAN_ALL and o["round_iterations"][0] == 25 and o["round_trials"][0] == 25
        assert o["round_pose"][0].tobytes() == np.concatenate([sc["Rcw"], sc["tcw"]]).astype(np.float64).tobytes()
        assert o["round_outlier"][0][int(np.flatnonzero(z == 0.0)[0])] == 1 and np.isfinite(o["round_pose"][1:]).all()
    # every exit kind occurs somewhere
    kinds = set(int(k) for c in PS.CASES for k in out(c)["round_exit"])
    assert kinds == {R.EXIT_RAN_ALL, R.EXIT_TRIALS, R.EXIT_RHO_ZERO}


# ---------------------------------------------------------------------------------------------------------------------
# scipy
# ---------------------------------------------------------------------------------------------------------------------
def _exp_np(x):
    om, up = x[:3], x[3:]
    th = float(np.linalg.norm(om))
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    if th < 1e-10:
        return np.eye(3) + Om, (np.eye(3) + 0.5 * Om) @ up
    Re = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * Om @ Om
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Om + (th - np.sin(th)) / th ** 3 * Om @ Om
    return Re, V @ up


def _fit(sc, obs, w, Xw, act, loss, delta):
    from scipy.optimize import least_squares
    cam = sc["cam"].astype(np.float64)
    R0, t0 = sc["Rcw"].astype(np.float64).reshape(3, 3), sc["tcw"].astype(np.float64)
    sw = np.sqrt(w[act])

    def fun(x):
        Re, tu = _exp_np(x)
        Rn, tn = Re @ R0, Re @ t0 + tu
        Xc = Xw[act] @ Rn.T + tn
        u, v = cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2], cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]
        return np.concatenate([sw * (obs[act, 0] - u), sw * (obs[act, 1] - v)])
    r = least_squares(fun, np.zeros(6), loss=loss, f_scale=delta, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=500, x_scale=1.0)
    Re, tu = _exp_np(r.x)
    return Re @ R0, Re @ t0 + tu


def _dist(Ra, ta, pose):
    Rb, tb = pose[:9].reshape(3, 3), pose[9:]
    d = float(np.linalg.norm(Ra - Rb)) / math.sqrt(2.0)
    return math.degrees(2.0 * math.asin(min(d / 2.0, 1.0))), float(np.linalg.norm(ta - tb))


@functools.lru_cache(maxsize=None)
def scipy_figures(kind, seed):
    sc = PS.make(kind, 300, seed)
    ours = PS.ref(sc)
    first, obs, w, Xw = R.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
    delta = R.delta_of(7.815)
    act = np.ones(len(first), bool)
    flips, r0 = 0, None
    for rnd in range(4):   # the four-round protocol on scipy's poses
        Rs, ts = _fit(sc, obs, w, Xw, act, "huber" if rnd <= 2 else "linear", delta)
        if rnd == 0:
            r0 = _dist(Rs, ts, ours["round_pose"][0])
        e0, e1, _, _, _ = R.residual(Rs.reshape(9), ts, sc["cam"], obs, Xw)
        bad = R.chi2_of(e0, e1, w).astype(np.float32) > np.float32(5.991)
        flips += int((bad != ours["round_outlier"][rnd].astype(bool)).sum())
        act = ~bad
    Rs, ts = _fit(sc, obs, w, Xw, ~ours["round_outlier"][2].astype(bool), "linear", delta)
    r3 = _dist(Rs, ts, ours["round_pose"][3])
    return dict(r0_deg=r0[0], r0_m=r0[1], r3_deg=r3[0], r3_m=r3[1], flips=flips)


@pytest.mark.parametrize("seed", SEEDS)
def test_distance_to_scipy(seed):
    worst3 = {k: 0.0 for k in GATE_R3}
    for kind in KINDS:
        m = scipy_figures(kind, seed)
        print("%s seed %d: %s" % (kind, seed, {k: ("%.3e" % v if isinstance(v, float) else v) for k, v in m.items()}))
        for k, gate in GATE_R0[kind].items():
            assert m[k] <= gate, (kind, seed, k, m[k], gate)
        for k in GATE_R3:
            worst3[k] = max(worst3[k], m[k])
    for k in GATE_R3:
        assert worst3[k] <= GATE_R3[k], (seed, k, worst3[k], GATE_R3[k])

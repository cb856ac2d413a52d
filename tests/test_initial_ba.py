"""SPEC DECISION S17 without a GPU: the restatement (tests/initial_ba_ref.py) reaches the exits and branches its scenes are built for, and
it agrees with an independent solver -- scipy.optimize.least_squares on the same 6 + 3N unknowns -- where both are converged.

The comparison with scipy.  Kinds general, general_pose1, converged, far at N = 300, iterations = 64 so that the restatement is
converged, loss = 'linear' and the same start on scipy's side.  No edge of these kinds ends above delta^2 (asserted), so the Huber
kernel is the identity at the optimum and the kernel choice cannot matter.  scipy's unknowns are a rotation vector w (pose 2 =
exp(w) R0), t and the points; its Jacobian is analytic in the points and a central difference in the six pose columns, handed over
sparse.  Two-view adjustment has a free scale, so both sides are compared after the adaptor's median-depth normalisation
(initial_ba_ref.median_depth_scale, binary32 as the adaptor's).  The free scale is a scaling about key frame 1's centre; dividing
world coordinates by the median depth, as the reference and the adaptor do, removes it only when pose 1 is the identity -- which it is
at that call site.  general_pose1 has another pose 1, so every estimate is first moved into key frame 1's coordinates (X -> R1 X + t1,
t2 -> t2 - R2 R1^T t1; a no-op for the other kinds) and normalised there.  Quantities: the rotation between the two pose estimates in degrees
(from the binary64 poses), the largest difference of the normalised translation, the largest relative difference of a normalised
point, the relative difference of the final cost.
Gates: twice the worst figure measured on seeds 0 and 1 (the constants below, the measurement beside them; DESIGN.md S17 repeats
them); they must hold on seeds 2 and 3 as well.
scipy's stopping rule: ftol is switched off (ftol=None) and xtol = gtol = 1e-15 end the run.  least_squares' ftol test compares the
change of the cost with ftol times the cost, 1e-15 x 73 here, which is below the rounding noise of a binary64 sum of 1200 squares: it
fires on noise, before the step has become small.  With ftol = 1e-15 the run of far / seed 2 stopped (status 2) 3.9e-8 degrees from
the optimum -- measured as the rotation part of one Gauss-Newton step from its result, which a restart of least_squares from that
result confirmed by moving there -- while the restatement's result was 5.2e-9 degrees from it; the difference of the two, 2.95e-8,
was the reference's own error.  "Both sides converged" is what the comparison needs, so the step-size rule decides.

Measured, not gated: ||R R^T - I||_F of the final pose 2, which is kept as a matrix and multiplied by one exp per accepted step.  It
stays at the level the caller's binary32 start pose has: 3.5e-8 .. 1.1e-7 over these 16 runs (the start's own figure is the same to
two digits; the products add about 1e-15)."""
import numpy as np
import pytest

import initial_ba_ref as R
import initial_ba_scenarios as BS
import poseopt_ref as P14

SCIPY_KINDS = ("general", "general_pose1", "converged", "far")
# twice the worst of seeds 0 and 1 over the four kinds.  Measured worst: rotation 9.54e-9 degrees (general, seed 0), translation 3.73e-9
# (one binary32 step of the normalised baseline), points 2.19e-7 relative (general, seed 1: binary32 again), cost 3.37e-10 relative
# (converged, seed 0, whose cost is 3e-9 in absolute terms; the other kinds measure 6e-15 at most)
GATE_ROT_DEG, GATE_T, GATE_POINTS, GATE_COST = 1.908e-8, 7.46e-9, 4.38e-7, 6.74e-10


def _counts(kind, N, seed=0, **kw):
    R.COUNTS.clear()
    P14.COUNTS.clear()
    out = BS.ref(BS.make(kind, N, seed), **kw)
    return out, dict(R.COUNTS), dict(P14.COUNTS)


def test_scenes_reach_their_branches():
    """the exits and branches the scenes are there for.  zero_depth: the issue expected `!ok and a 10-trial Terminate`; the text of the
    loop gives `!ok` in every trial (tmp = DBL_MAX) but rho is a NaN there -- the sums are non-finite -- and a NaN rho ends the trial
    loop (`rho < 0` is false) without Terminate, so every iteration takes one rejected trial and the run ends RAN_ALL with the input
    estimate.  The 10-trial Terminate is reached by general-N4097 and general-N300-seed1 instead."""
    o, c, c14 = _counts("general", 257)
    assert c["accepted"] > 5 and c14["large_theta"] > 0 and o["it_cost"][-1] < o["it_cost"][0]
    o, c, c14 = _counts("converged", 257)
    assert c14.get("large_theta", 0) == 0 and c14["small_theta"] == o["trials"] and c.get("rejected", 0) == 0
    o, c, _ = _counts("far", 65)
    assert c["rejected"] > 0 and c["accepted"] > 0 and (o["it_trials"] > 1).any()
    o, c, _ = _counts("outliers", 257)
    assert c["huber_linear_region"] == o["iterations"] and (o["chi2"][1] > 5.99).sum() > 20   # still there at the end
    o2, c2, _ = _counts("robust_off", 257)
    assert "huber_linear_region" not in c2 and o2["pose"].tobytes() != o["pose"].tobytes()
    o, c, _ = _counts("low_parallax", 65)
    assert c["accepted"] > 5 and np.isfinite(o["pose"]).all()
    o, c, _ = _counts("zero_depth", 257)
    assert c["not_ok"] == c["nonfinite_block"] == c["rejected"] == o["trials"] == 20 and "accepted" not in c
    assert o["exit"] == R.EXIT_RAN_ALL and not np.isfinite(o["it_cost"]).any() and np.isinf(o["chi2"][1]).sum() == 1
    sc = BS.make("zero_depth", 257)
    assert o["points"].tobytes() == sc["points"].tobytes() and o["pose"][9:].tobytes() == sc["tcw2"].astype(np.float64).tobytes()
    assert o["depth_positive"][1].sum() == 256
    o, c, _ = _counts("general", 4097)
    assert o["exit"] == R.EXIT_TRIALS and o["it_trials"][-1] == R.MAX_TRIALS
    o, c, _ = _counts("general", 65)
    assert o["exit"] == R.EXIT_RHO_ZERO
    o, c, _ = _counts("general", 65, iterations=3)
    assert o["exit"] == R.EXIT_RAN_ALL and o["iterations"] == 3
    sc = BS.make("unmatched", 64)
    o = BS.ref(sc)
    un = sc["matches12"] < 0
    assert o["N"] == 64 and un.sum() > 64 and len(sc["kp1_xy"]) != len(sc["kp2_xy"])
    assert o["points"][un].tobytes() == sc["points"][un].tobytes() and (o["points"][~un] != sc["points"][~un]).any()


def test_no_match_returns_the_inputs():
    sc = BS.make("general", 10)
    sc["matches12"][:] = -1
    o = BS.ref(sc)
    assert o["N"] == 0 and o["iterations"] == 0 and o["points"].tobytes() == sc["points"].tobytes()
    assert o["Tcw2"][:3, 3].tobytes() == sc["tcw2"].tobytes()


def test_inv3_sym_inverts():
    rng = np.random.RandomState(3)
    A = rng.normal(size=(50, 3, 3))
    A = A @ A.transpose(0, 2, 1) + 0.1 * np.eye(3)
    inv = R.inv3_sym([A[:, j, k] for j, k in R.SYM])
    full = np.array([[R.sym_at(inv, j, k) for k in range(3)] for j in range(3)]).transpose(2, 0, 1)
    assert np.abs(full @ A - np.eye(3)).max() < 1e-9


def _scipy_solve(sc):
    """least_squares on the 6 + 3N unknowns from the same start -> (R2 [3, 3], t2 [3], X [N, 3], cost)"""
    from scipy.optimize import least_squares
    from scipy.sparse import csr_matrix
    from scipy.spatial.transform import Rotation
    idx, obs1, w1, obs2, w2, X0 = R.points_of(sc["level_sigma2"], sc["kp1_xy"], sc["kp1_octave"], sc["kp2_xy"], sc["kp2_octave"],
                                              sc["matches12"], sc["points"])
    fx, fy, cx, cy = (float(v) for v in sc["cam"][:4])
    Ra, ta = sc["Rcw1"].astype(np.float64).reshape(3, 3), sc["tcw1"].astype(np.float64)
    R0, t0 = sc["Rcw2"].astype(np.float64).reshape(3, 3), sc["tcw2"].astype(np.float64)
    n = len(X0)
    rows = np.arange(n)

    def parts(p):
        return Rotation.from_rotvec(p[:3]).as_matrix() @ R0, p[3:6], p[6:].reshape(-1, 3)

    def res(p):
        Rb, tb, X = parts(p)
        out = []
        for Rc, tc, ob, w in ((Ra, ta, obs1, w1), (Rb, tb, obs2, w2)):
            Xc = X @ Rc.T + tc
            s = np.sqrt(w)
            out += [(ob[:, 0] - (fx * Xc[:, 0] / Xc[:, 2] + cx)) * s, (ob[:, 1] - (fy * Xc[:, 1] / Xc[:, 2] + cy)) * s]
        return np.concatenate(out)

    def jac(p):
        Rb, tb, X = parts(p)
        J = np.zeros((4 * n, 6 + 3 * n))
        for e, (Rc, tc, w) in enumerate(((Ra, ta, w1), (Rb, tb, w2))):
            Xc = X @ Rc.T + tc
            s, z = np.sqrt(w), Xc[:, 2]
            du = np.stack([fx / z, np.zeros(n), -fx * Xc[:, 0] / z ** 2], 1) @ Rc
            dv = np.stack([np.zeros(n), fy / z, -fy * Xc[:, 1] / z ** 2], 1) @ Rc
            for k in range(3):
                J[2 * e * n + rows, 6 + 3 * rows + k] = -du[:, k] * s
                J[(2 * e + 1) * n + rows, 6 + 3 * rows + k] = -dv[:, k] * s
        h = 1e-6
        for k in range(6):
            d = np.zeros_like(p)
            d[k] = h
            J[2 * n:, k] = ((res(p + d) - res(p - d)) / (2 * h))[2 * n:]
        return csr_matrix(J)
    p0 = np.concatenate([np.zeros(3), t0, X0.reshape(-1)])
    s = least_squares(res, p0, jac=jac, loss="linear", xtol=1e-15, ftol=None, gtol=1e-15, method="trf", tr_solver="lsmr",
                      tr_options=dict(atol=1e-14, btol=1e-14, maxiter=20000), x_scale="jac")
    Rb, tb, X = parts(s.x)
    return Rb, tb, X, float((s.fun ** 2).sum())


def _figures(kind, seed):
    sc = BS.make(kind, 300, seed)
    ours = BS.ref(sc, iterations=64)
    delta2 = R.delta_of(5.99) ** 2
    assert ours["chi2"].max() < delta2, "an edge ends in Huber's linear region: the comparison with a linear loss would not hold"
    Rs, ts, Xs, cost = _scipy_solve(sc)
    idx = np.flatnonzero(sc["matches12"] >= 0)
    R1, t1 = sc["Rcw1"].astype(np.float64).reshape(3, 3), sc["tcw1"].astype(np.float64)
    eye, zero = np.eye(3, dtype=np.float32).reshape(9), np.zeros(3, np.float32)

    def normalised(R2, t2, X):
        """the estimate in key frame 1's coordinates, then the adaptor's step with pose 1 = identity"""
        est = dict(points=sc["points"].copy(), Tcw2=np.eye(4, dtype=np.float32))
        est["points"][idx] = (X @ R1.T + t1).astype(np.float32)
        est["Tcw2"][:3, 3] = (t2 - R2 @ R1.T @ t1).astype(np.float32)
        return R.median_depth_scale(est, eye, zero, sc["matches12"])
    a = normalised(ours["pose"][:9].reshape(3, 3), ours["pose"][9:], ours["points"][idx].astype(np.float64))
    b = normalised(Rs, ts, Xs)
    assert a[0] and b[0]
    Ro = ours["pose"][:9].reshape(3, 3)
    M = Rs @ np.linalg.inv(Ro)
    rot = np.degrees(np.arcsin(min(1.0, np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / 2)))
    dt = float(np.abs(a[1].astype(np.float64) - b[1]).max())
    pa, pb = a[2][idx].astype(np.float64), b[2][idx].astype(np.float64)
    dp = float((np.linalg.norm(pa - pb, axis=1) / np.linalg.norm(pb, axis=1)).max())
    dc = abs(float(ours["it_cost"][-1]) - cost) / cost
    orth = float(np.linalg.norm(Ro @ Ro.T - np.eye(3)))
    print("%s seed %d: rotation %.3g deg, translation %.3g, points %.3g, cost %.3g (%.12g / %.12g), ||R R^T - I||_F %.3g, iterations %d"
          % (kind, seed, rot, dt, dp, dc, ours["it_cost"][-1], cost, orth, ours["iterations"]))
    return rot, dt, dp, dc, orth


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", SCIPY_KINDS)
def test_agrees_with_scipy_least_squares(kind, seed):
    rot, dt, dp, dc, orth = _figures(kind, seed)
    assert rot <= GATE_ROT_DEG and dt <= GATE_T and dp <= GATE_POINTS and dc <= GATE_COST
    assert orth < 2e-7   # the level of a binary32 rotation matrix; measured 3.5e-8 .. 1.1e-7

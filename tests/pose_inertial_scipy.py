"""The independent solver of tests/test_pose_inertial.py (S19, 15 unknowns: *15 / link64_kf) and tests/test_pose_inertial_prev.py (S20,
30 unknowns: *30 / link64_free / prior64), moved here unchanged so that tests/test_track_inertial_sequence.py runs the same text on
the problems a sequence of frames produces: scipy.optimize.least_squares in binary64 with scipy's Rotation and plain numpy, nothing
shared with the restatements.  Residuals are whitened by the Cholesky factors of info9 / infoG / infoA / the prior's H and by sqrt(w).
Round 0 is compared with loss='huber' (f_scale = delta) from the same start, round 3 with loss='linear' on round 2's inlier set from
round 2's state."""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation


# ---- S19: the frame's 15 unknowns against the fixed last key frame ----
def unpack15(x0, x):
    Rwb = x0["Rwb"] @ Rotation.from_rotvec(x[0:3]).as_matrix()
    return Rwb, x0["twb"] + x[3:6], x0["v"] + x[6:9], x0["bg"] + x[9:12], x0["ba"] + x[12:15]


def residuals15(x, x0, sc, K, obs, w, Xw, keep, gravity):
    Rwb, twb, v, bg, ba = unpack15(x0, x)
    Rcb, tcb = K["Rcb"], K["tcb"]
    Rcw = Rcb @ Rwb.T
    tcw = Rcb @ (-Rwb.T @ twb) + tcb
    Xc = Xw[keep] @ Rcw.T + tcw
    fx, fy, cx, cy = (float(c) for c in sc["cam"][:4])
    proj = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    r_mono = ((obs[keep] - proj) * np.sqrt(w[keep])[:, None]).reshape(-1)
    g = np.array([0.0, 0.0, -gravity])
    dt = K["dt"]
    Rbw1 = K["Rwb1"].T
    er = Rotation.from_matrix(K["dR"].T @ Rbw1 @ Rwb).as_rotvec()
    ev = Rbw1 @ (v - K["v1"] - g * dt) - K["dV"]
    ep = Rbw1 @ (twb - K["twb1"] - K["v1"] * dt - g * dt * dt / 2.0) - K["dP"]
    r_imu = K["L9"].T @ np.concatenate([er, ev, ep])
    return np.concatenate([r_mono, r_imu, K["LG"].T @ (bg - K["bg1"]), K["LA"].T @ (ba - K["ba1"])])


def link64_kf(link):
    K = {k: np.asarray(link[k], np.float32).astype(np.float64) for k in ("twb1", "v1", "bg1", "ba1", "dV", "dP", "tcb")}
    for k in ("Rwb1", "dR", "Rcb"):
        K[k] = np.asarray(link[k], np.float32).astype(np.float64).reshape(3, 3)
    K["dt"] = float(np.float32(link["dt"]))
    # dR as the caller's floats is not exactly a rotation; the independent solver takes the nearest one
    U, _, Vt = np.linalg.svd(K["dR"])
    K["dR"] = U @ Vt
    K["L9"] = np.linalg.cholesky(np.asarray(link["info9"], np.float64).reshape(9, 9))
    K["LG"] = np.linalg.cholesky(np.asarray(link["infoG"], np.float64).reshape(3, 3))
    K["LA"] = np.linalg.cholesky(np.asarray(link["infoA"], np.float64).reshape(3, 3))
    return K


def state15(vec):
    return dict(Rwb=vec[:9].reshape(3, 3), twb=vec[9:12], v=vec[12:15], bg=vec[15:18], ba=vec[18:21])


def distance15(vec, x0, x):
    Rwb, twb, v, bg, ba = unpack15(x0, x)
    s = state15(vec)
    rot = float(np.linalg.norm(Rotation.from_matrix(Rwb.T @ s["Rwb"]).as_rotvec()))
    return (rot,) + tuple(float(np.linalg.norm(a - b)) for a, b in ((twb, s["twb"]), (v, s["v"]), (bg, s["bg"]), (ba, s["ba"])))


def measure15(R, sc, ref, rounds=(0, 3)):
    """R: pose_inertial_ref; sc: the problem (cam, level_sigma2, kp_xy, kp_octave, mp_index, points, link, Rwb twb v bg ba);
    ref: the restatement's result -> {round: distances (rot, twb, v, bg, ba)} between the restatement and scipy"""
    first, obs, w, Xw = R.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
    K = link64_kf(sc["link"])
    gravity = float(np.float32(9.81))
    delta = R.delta_of(5.991)
    out = {}
    start = np.concatenate([np.asarray(sc[k], np.float32).astype(np.float64).reshape(-1) for k in ("Rwb", "twb", "v", "bg", "ba")])
    for rnd, x0vec, keep, loss in ((0, start, np.ones(len(first), bool), "huber"),
                                   (3, ref["round_state"][2], ref["round_outlier"][2] == 0, "linear")):
        if rnd not in rounds:
            continue
        x0 = state15(x0vec)
        sol = least_squares(residuals15, np.zeros(15), args=(x0, sc, K, obs, w, Xw, keep, gravity), loss=loss, f_scale=delta, method="trf",
                            x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
        out[rnd] = distance15(ref["round_state"][rnd], x0, sol.x)
    return out


# ---- S20: the frame's and the previous frame's 30 unknowns, with the prior on the previous frame ----
def unpack30(x0, x):
    out = []
    for h in (0, 1):
        s, d = x0[h], x[15 * h:15 * h + 15]
        out.append((s["Rwb"] @ Rotation.from_rotvec(d[0:3]).as_matrix(), s["twb"] + d[3:6], s["v"] + d[6:9], s["bg"] + d[9:12], s["ba"] + d[12:15]))
    return out


def residuals30(x, x0, sc, K, Pr, obs, w, Xw, keep, gravity):
    (Rwb, twb, v, bg, ba), (Rwb1, twb1, v1, bg1, ba1) = unpack30(x0, x)
    Rcb, tcb = K["Rcb"], K["tcb"]
    Rcw = Rcb @ Rwb.T
    tcw = Rcb @ (-Rwb.T @ twb) + tcb
    Xc = Xw[keep] @ Rcw.T + tcw
    fx, fy, cx, cy = (float(c) for c in sc["cam"][:4])
    proj = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1)
    r_mono = ((obs[keep] - proj) * np.sqrt(w[keep])[:, None]).reshape(-1)
    g = np.array([0.0, 0.0, -gravity])
    dt = K["dt"]
    dbg, dba = bg1 - K["bg0"], ba1 - K["ba0"]
    dR = K["dR0"] @ Rotation.from_rotvec(K["JRg"] @ dbg).as_matrix()
    dV = K["dV0"] + K["JVg"] @ dbg + K["JVa"] @ dba
    dP = K["dP0"] + K["JPg"] @ dbg + K["JPa"] @ dba
    Rbw1 = Rwb1.T
    er = Rotation.from_matrix(dR.T @ Rbw1 @ Rwb).as_rotvec()
    ev = Rbw1 @ (v - v1 - g * dt) - dV
    ep = Rbw1 @ (twb - twb1 - v1 * dt - g * dt * dt / 2.0) - dP
    r_imu = K["L9"].T @ np.concatenate([er, ev, ep])
    e_pr = np.concatenate([Rotation.from_matrix(Pr["Rwb"].T @ Rwb1).as_rotvec(), Pr["Rwb"].T @ (twb1 - Pr["twb"]), v1 - Pr["vwb"],
                           bg1 - Pr["bg"], ba1 - Pr["ba"]])
    return np.concatenate([r_mono, r_imu, K["LG"].T @ (bg - bg1), K["LA"].T @ (ba - ba1), Pr["L"].T @ e_pr])


def link64_free(link):
    K = {k: np.asarray(link[k], np.float32).astype(np.float64) for k in ("dV0", "dP0", "bg0", "ba0", "tcb")}
    for k in ("dR0", "Rcb", "JRg", "JVg", "JVa", "JPg", "JPa"):
        K[k] = np.asarray(link[k], np.float32).astype(np.float64).reshape(3, 3)
    K["dt"] = float(np.float32(link["dt"]))
    U, _, Vt = np.linalg.svd(K["dR0"])   # dR0 as the caller's floats is not exactly a rotation; the independent solver takes the nearest one
    K["dR0"] = U @ Vt
    K["L9"] = np.linalg.cholesky(np.asarray(link["info9"], np.float64).reshape(9, 9))
    K["LG"] = np.linalg.cholesky(np.asarray(link["infoG"], np.float64).reshape(3, 3))
    K["LA"] = np.linalg.cholesky(np.asarray(link["infoA"], np.float64).reshape(3, 3))
    return K


def prior64(prior):
    Pr = {k: np.asarray(prior[k], np.float64) for k in ("twb", "vwb", "bg", "ba")}
    Pr["Rwb"] = np.asarray(prior["Rwb"], np.float64).reshape(3, 3)
    Hm = np.asarray(prior["H"], np.float64).reshape(15, 15)
    Pr["L"] = np.linalg.cholesky((Hm + Hm.T) / 2.0 + 1e-9 * np.eye(15))   # (a rank-deficient H would be regularised here, and only here)
    return Pr


def states30(vec):
    return [dict(Rwb=vec[o:o + 9].reshape(3, 3), twb=vec[o + 9:o + 12], v=vec[o + 12:o + 15], bg=vec[o + 15:o + 18], ba=vec[o + 18:o + 21])
            for o in (0, 21)]


def distance30(vec, x0, x):
    out = []
    for (Rwb, twb, v, bg, ba), s in zip(unpack30(x0, x), states30(vec)):
        out.append(float(np.linalg.norm(Rotation.from_matrix(Rwb.T @ s["Rwb"]).as_rotvec())))
        out += [float(np.linalg.norm(a - b)) for a, b in ((twb, s["twb"]), (v, s["v"]), (bg, s["bg"]), (ba, s["ba"]))]
    return tuple(out)


def measure30(R, sc, ref, rounds=(0, 3)):
    """R: pose_inertial_prev_ref; sc: the problem, with `prior`; ref: the restatement's result -> {round: the ten distances (the frame's
    five, then the previous frame's five)} between the restatement and scipy"""
    first, obs, w, Xw = R.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
    K, Pr = link64_free(sc["link"]), prior64(sc["prior"])
    gravity = float(np.float32(9.81))
    delta = R.delta_of(5.991)
    out = {}
    start = np.concatenate([np.asarray(sc[k], np.float32).astype(np.float64).reshape(-1) for k in ("Rwb", "twb", "v", "bg", "ba")] +
                           [np.asarray(sc["link"][k], np.float32).astype(np.float64).reshape(-1) for k in ("Rwb1", "twb1", "v1", "bg1", "ba1")])
    for rnd, x0vec, keep, loss in ((0, start, np.ones(len(first), bool), "huber"),
                                   (3, ref["round_state"][2], ref["round_outlier"][2] == 0, "linear")):
        if rnd not in rounds:
            continue
        x0 = states30(x0vec)
        sol = least_squares(residuals30, np.zeros(30), args=(x0, sc, K, Pr, obs, w, Xw, keep, gravity), loss=loss, f_scale=delta, method="trf",
                            x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=400)
        out[rnd] = distance30(ref["round_state"][rnd], x0, sol.x)
    return out

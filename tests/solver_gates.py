"""Scenes that sit exactly on the solvers' gates (helper module, not a test).

The solver kernels (S12 two-view reconstruction, S13 MLPnP, S14 pose optimisation, S19 / S20 inertial pose optimisation) are compared
byte for byte with their numpy restatements.  The scenes of the *_scenarios modules are seeded random geometry: a residual comes
near a gate but never onto it, so `a > b` and `a >= b` never differ there.  Planting geometry whose chi2 after fifteen solver steps
equals a constant is not feasible; but almost every gate compares against a CALL PARAMETER.  So the parameter is moved onto the
value: the restatement runs on a small seeded scene, the compared quantity is read where the gate reads it, and the scene is that
geometry with the parameter set to exactly that number.  Ties between hypotheses (S12, S13) are made by repeating a min-set, which
both calls allow.

A scene is a dict: `family` (which restatement / library call takes it), `name`, `sc` (the scenario dict of the family's
*_scenarios module), `kw` (the parameters that differ from the defaults), `want` (the restatement's result for sc and kw) and `ties`:
a list of (round or iteration, index, gate name) saying where a compared value sits exactly on its bound.  verify(scene) re-derives
every listed equality from the restatement alone; tests/test_solver_gates.py calls it for every scene, proves with the mutants of
tests/solver_mutants.py that the scenes tell every one-token mistake from the real restatement, and tests/test_solver_gates_gpu.py
runs the library on them.

scenes(family) builds every scene of a family; names(family) lists them without running anything and build(family, name) builds one,
so that a test can be parametrised by name.  The seeds in SEEDS_POSEOPT and SEEDS_IMU were looked through (search_seeds_poseopt,
search_seeds_imu) for base scenes in which the tie holds on every wanted edge and the
restatement keeps at least MIN_ACTIVE active edges in every round: with `thr` an edge's own chi2, whatever its size, most seeds leave
too few."""
import functools

import numpy as np

import mlpnp_ref as MR
import mlpnp_scenarios as MS
import pose_inertial_prev_ref as R20
import pose_inertial_prev_scenarios as S20
import pose_inertial_ref as R19
import pose_inertial_scenarios as S19
import poseopt_ref as PR
import poseopt_scenarios as PS
import twoview_ref as TR
import twoview_scenarios as TS

f32, f64 = np.float32, np.float64
FAMILIES = ("poseopt", "inertial", "inertial_prev", "twoview", "mlpnp")
REAL = dict(poseopt=PR, inertial=R19, inertial_prev=R20, twoview=TR, mlpnp=MR)
MIN_ACTIVE = 10
WAVE = 64
SKIP_KEYS = ("details", "first")   # of a restatement's result: python lists and index helpers no library call returns


def positions(Ne):
    """where a per-edge tie is built: edge 0, the two edges either side of the first wave boundary, the last edge"""
    return sorted({0, WAVE - 1, WAVE, Ne - 1} & set(range(Ne)))


def run(family, sc, kw, mod=None):
    """the restatement (or a mutant of it: `mod`) on a scene's arguments"""
    mod = mod or REAL[family]
    if family == "poseopt":
        return mod.pose_optimization(sc["cam"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"], sc["Rcw"],
                                     sc["tcw"], **kw)
    if family == "inertial":
        return mod.pose_inertial_optimization(sc["cam"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"],
                                              sc["track_depth"], sc["link"], sc["Rcw"], sc["tcw"], sc["Rwb"], sc["twb"], sc["v"], sc["bg"],
                                              sc["ba"], **kw)
    if family == "inertial_prev":
        return mod.pose_inertial_optimization_last_frame(sc["cam"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"],
                                                         sc["points"], sc["track_depth"], sc["link"], sc["prior"], sc["Rcw"], sc["tcw"],
                                                         sc["Rwb"], sc["twb"], sc["v"], sc["bg"], sc["ba"], **kw)
    if family == "twoview":
        fx, fy, cx, cy, sigma, iterations = sc["params"]
        return mod.reconstruct(fx, fy, cx, cy, sigma, iterations, sc["kp1"], sc["kp2"], sc["matches12"], sc["sets"])
    if family == "mlpnp":
        prm = dict(sc["ransac"])
        prm.update(kw)
        return mod.ransac(sc["cam"], sc["model"], sc["precision"], sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"],
                          sc["points"], sc["sets"], **prm)
    raise ValueError(family)


def same_result(a, b):
    """two results of a restatement: every field, NaN equal to NaN"""
    if a.keys() != b.keys():
        return False
    for k in a:
        if k in SKIP_KEYS:
            continue
        x, y = a[k], b[k]
        if isinstance(x, tuple):
            x, y = np.array(x), np.array(y)
        x, y = np.asarray(x), np.asarray(y)
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if not (np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y)):
            return False
    return True


def scene(family, name, sc, kw, ties, want=None):
    return dict(family=family, name=name, sc=sc, kw=kw, ties=ties, want=run(family, sc, kw) if want is None else want)


# ---------------------------------------------------------------------------------------------------------------------
# S14: chi2_threshold on an edge's chi2
# ---------------------------------------------------------------------------------------------------------------------
# (N_e, kind, seed, edges).  12: the 64-thread launch; 257: RUN 2; 1025: RUN 0, the flags read back from memory.  At N_e = 12 an
# edge can be tied only when it is one of the three largest residuals (ten edges must stay active), so each edge has its own seed.
SEEDS_POSEOPT = ((12, "general", 8, (0,)), (12, "general", 4, (11,)), (257, "general", 5, (0, 63, 64, 256)),
                 (1025, "general", 2, (0, 63, 64, 1024)))


def poseopt_chi2(sc, want):
    """[rounds_run, N_e] float32: chi2 of every edge at each round's final pose, as the gate reads it (poseopt_ref :320-322)"""
    _, obs, w, Xw = PR.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
    out = []
    for p in want["round_pose"]:
        e0, e1, _, _, _ = PR.residual(p[:9], p[9:], sc["cam"], obs, Xw)
        with np.errstate(all="ignore"):
            out.append(PR.chi2_of(e0, e1, w).astype(f32))
    return np.array(out, f32).reshape(len(want["round_pose"]), -1)


def enough_active(want):
    return want["rounds_run"] == 4 and bool(np.all(want["N_e"] - np.asarray(want["round_nbad"]) >= MIN_ACTIVE))


def poseopt_tie(sc, rnd, edge, tries=6):
    """chi2_threshold = the chi2 of `edge` at the end of round `rnd`, bit for bit.  Round 0 does not depend on the threshold, so one
    rerun gives it; a later round's pose depends on the flags of the rounds before, so the threshold is iterated to a fixed point.
    -> (kw, want) or None"""
    want = PS.ref(sc)
    if want["rounds_run"] <= rnd:
        return None
    thr = poseopt_chi2(sc, want)[rnd, edge]
    for _ in range(tries):
        if not np.isfinite(thr):
            return None
        kw = dict(chi2_threshold=float(thr))
        want = PS.ref(sc, **kw)
        got = poseopt_chi2(sc, want)[rnd, edge]
        if got == thr:
            return (kw, want) if enough_active(want) and want["round_outlier"][rnd, edge] == 0 else None
        thr = got
    return None


POSEOPT_ROUNDS = ((0,), (2, 1, 3))   # round 0 and one later round (the first of these in which the tie holds)


@functools.lru_cache(maxsize=None)
def _poseopt_make(kind, Ne, seed):
    return PS.make(kind, Ne, seed)


def poseopt_one(kind, Ne, seed, edge, group):
    """the tie on `edge` in the first round of `group` in which it holds -> (round, kw, want) or None"""
    for rnd in group:
        hit = poseopt_tie(_poseopt_make(kind, Ne, seed), rnd, edge)
        if hit:
            return (rnd,) + hit
    return None


def search_seeds_poseopt(Ne, edges=None, kinds=("general", "outliers"), seeds=range(40)):
    for kind in kinds:
        for seed in seeds:
            if all(poseopt_one(kind, Ne, seed, e, g) for e in (positions(Ne) if edges is None else edges) for g in POSEOPT_ROUNDS):
                return kind, seed
    return None


def poseopt_specs():
    out = []
    for Ne, kind, seed, edges in SEEDS_POSEOPT:
        assert set(edges) <= set(positions(Ne))
        for edge in edges:
            for group in POSEOPT_ROUNDS:
                out.append(("%s-N%d-seed%d-edge%d-%s" % (kind, Ne, seed, edge, "round0" if group == (0,) else "later"),
                            poseopt_scene, (kind, Ne, seed, edge, group)))
    return out


def poseopt_scene(name, kind, Ne, seed, edge, group):
    hit = poseopt_one(kind, Ne, seed, edge, group)
    assert hit, "S14 %s N_e %d seed %d: edge %d no longer ties" % (kind, Ne, seed, edge)
    rnd, kw, want = hit
    return scene("poseopt", name, _poseopt_make(kind, Ne, seed), kw, [(rnd, edge, "chi2_threshold")], want)


def verify_poseopt(s):
    sc, want = s["sc"], s["want"]
    assert enough_active(want), "%s: fewer than %d active edges in a round" % (s["name"], MIN_ACTIVE)
    chi2 = poseopt_chi2(sc, want)
    thr = f32(s["kw"]["chi2_threshold"])
    assert float(thr) == s["kw"]["chi2_threshold"]   # the parameter is a binary32 number: the call's float takes it unchanged
    for rnd, edge, gate in s["ties"]:
        assert gate == "chi2_threshold"
        assert chi2[rnd, edge].tobytes() == thr.tobytes(), "%s: chi2 %r is not on the threshold %r" % (s["name"], chi2[rnd, edge], thr)
        assert want["round_outlier"][rnd, edge] == 0
    assert np.array_equal(want["round_outlier"], (chi2 > thr).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# S19 / S20: the per-round chi2 gates (far and close), close_depth, the recovery pass, an edge at depth 0
# ---------------------------------------------------------------------------------------------------------------------
IMU = {"inertial": (R19, S19), "inertial_prev": (R20, S20)}
GEOMETRY = ("kp_xy", "kp_octave", "mp_index", "points", "track_depth", "Rcw", "tcw", "Rwb", "twb", "v", "bg", "ba", "Ne")
# family: {(kind, N_e): seed}.  40: one wave; 257: T.run = 2 (csrc/kernels_poseimu.hip: P = 512 > kTreeThreads), so 1025 adds no shape
SEEDS_IMU = {"inertial": {("outliers", 40): 2, ("outliers", 257): 0, ("close_boundary", 257): 0, ("recover", 25): 0},
             "inertial_prev": {("outliers", 40): 2, ("outliers", 257): 2, ("close_boundary", 257): 0, ("recover", 25): 0}}
RECOVERY = 4   # the index of the recovery pass's scoring among the calls of score(): after the four rounds


def imu_make(family, kind, Ne, seed):
    """the family's scene of a kind; S20 has no close_boundary / recover kind of its own: the geometry of S19's, S20's general link and
    prior (the key frame's and the frame's true states are the same in every kind)"""
    if family == "inertial":
        return S19.make(kind, Ne, seed)
    if kind in S20.BASE:
        return S20.make(kind, Ne, seed)
    sc, geo = dict(S20.make("general", Ne, seed)), S19.make(kind, Ne, seed)
    for k in GEOMETRY:
        sc[k] = geo[k]
    sc["kind"] = kind
    return sc


def imu_params(family, kw):
    prm = dict(IMU[family][0].PARAMS)
    prm.update(kw)
    return prm


def imu_traced(family, sc, kw):
    """-> (result, [(chi2 float32 [N_e], front [N_e])]): what pose_inertial_ref.score returned, call by call -- once at the end of
    every round and once in the recovery pass -- which is what the gates compare"""
    calls, real = [], R19.score

    def spy(*a):
        out = real(*a)
        calls.append(out)
        return out
    R19.score = spy
    try:
        want = run(family, sc, kw)
    finally:
        R19.score = real
    return want, calls


def imu_close(family, sc, kw):
    first = np.flatnonzero(np.asarray(sc["mp_index"]) >= 0)
    depth = np.asarray(sc["track_depth"], f32)[np.asarray(sc["mp_index"])[first]]
    return depth < f32(imu_params(family, kw)["close_depth"]), depth


def thr_close_of(thr, factor):
    return f32(f64(factor) * f64(f32(thr)))


def thr_for_close(chi2, factor, reach=3):
    """a threshold whose close bound f32(factor * thr) is exactly `chi2`, within `reach` units in the last place of chi2 / factor"""
    t = f32(f64(chi2) / f64(factor))
    cand = [t]
    lo = hi = t
    for _ in range(reach):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        cand += [lo, hi]
    for c in cand:
        if thr_close_of(c, factor).tobytes() == f32(chi2).tobytes():
            return c
    return None


def with_chi2(family, rnd, thr, kw=None):
    kw = dict(kw or {})
    chi2 = list(imu_params(family, kw)["chi2"])
    chi2[rnd] = float(thr)
    kw["chi2"] = tuple(chi2)
    return kw


def imu_round_tie(family, sc, rnd, edge, base=None):
    """chi2[rnd] such that the bound of `edge` (far: thr, close: f32(close_factor * thr)) is its chi2 at the end of round `rnd`.
    chi2[rnd] is read after round rnd's optimisation, so the rounds up to rnd do not move -> (kw, gate) or None"""
    want, calls = base or imu_traced(family, sc, {})
    if len(calls) <= rnd:
        return None
    c = calls[rnd][0][edge]
    if not np.isfinite(c) or not calls[rnd][1][edge]:
        return None
    close, _ = imu_close(family, sc, {})
    thr = thr_for_close(c, imu_params(family, {})["close_factor"]) if close[edge] else c
    if thr is None:
        return None
    return with_chi2(family, rnd, thr), "chi2_close" if close[edge] else "chi2_far"


@functools.lru_cache(maxsize=None)
def imu_base(family, kind, Ne, seed):
    """-> (scene arguments, the restatement's result with the default parameters, its score() calls)"""
    sc = imu_make(family, kind, Ne, seed)
    return (sc,) + imu_traced(family, sc, {})


def imu_round_scene(name, family, kind, Ne, seed, rnd, edge):
    """(a) / (b): one position in one round; None when the tie fails or a round keeps fewer than MIN_ACTIVE edges"""
    sc, want, calls = imu_base(family, kind, Ne, seed)
    hit = imu_round_tie(family, sc, rnd, edge, (want, calls))
    if not hit:
        return None
    s = scene(family, name, sc, hit[0], [(rnd, edge, hit[1])])
    return s if enough_active(s["want"]) else None


def search_seeds_imu(family, Ne, kinds=("outliers", "general"), seeds=range(30), rounds=range(4)):
    for kind in kinds:
        for seed in seeds:
            got = [imu_round_scene("", family, kind, Ne, seed, rnd, e) for e in positions(Ne) for rnd in rounds]
            if all(got) and {t[2] for s in got for t in s["ties"]} >= ({"chi2_far", "chi2_close"} if Ne > WAVE else {"chi2_far"}):
                return kind, seed
    return None


def imu_close_depth_scene(name, family, kind, Ne, seed):
    """(c): close_depth = the track_depth of a close edge whose chi2 lies between thr and thrClose in the last round; `<` makes it a
    far edge, and it is flagged.  The edge nearest to the default close_depth is taken, so that as few other edges as possible change
    sides; for those that do, the restatement says what happens."""
    sc, want, calls = imu_base(family, kind, Ne, seed)
    prm = imu_params(family, {})
    close, depth = imu_close(family, sc, {})
    last = want["rounds_run"] - 1
    thr = f32(prm["chi2"][last])
    c = calls[last][0]
    for edge in sorted(np.flatnonzero(close & (c > thr) & (c < thr_close_of(thr, prm["close_factor"]))), key=lambda e: -depth[e]):
        kw = dict(close_depth=float(depth[edge]))
        s = scene(family, name, sc, kw, [(last, int(edge), "close_depth")])
        c2 = imu_traced(family, sc, kw)[1][last][0][edge]
        if c2 > thr and c2 < thr_close_of(thr, prm["close_factor"]) and enough_active(s["want"]):
            return s
    return None


CLOSE_FACTOR_INEXACT = 1.3   # not a binary32 number: f32(1.3 * thr) in binary64 and f32(1.3) * thr in binary32 differ for some thr


def imu_close_factor_scene(name, family, kind, Ne, seed):
    """(b) once more with a close_factor that binary32 does not hold: the first close edge, in the last round, for which the bound
    computed in binary64 lands on the chi2 and the one computed in binary32 does not"""
    sc = imu_make(family, kind, Ne, seed)
    kw0 = dict(close_factor=CLOSE_FACTOR_INEXACT)
    want, calls = imu_traced(family, sc, kw0)
    close, _ = imu_close(family, sc, kw0)
    last = want["rounds_run"] - 1
    for edge in np.flatnonzero(close & np.isfinite(calls[last][0]) & calls[last][1]):
        c = calls[last][0][edge]
        thr = thr_for_close(c, CLOSE_FACTOR_INEXACT)
        if thr is not None and f32(f32(CLOSE_FACTOR_INEXACT) * thr) != c:
            s = scene(family, name, sc, with_chi2(family, last, thr, kw0), [(last, int(edge), "chi2_close")])
            if enough_active(s["want"]):
                return s
    return None


RECOVER_WHAT = ("recover_below", "recover_below+1", "recover_chi2-first", "recover_chi2-last", "recover_chi2-kept")


def imu_recover_scene(name, family, kind, Ne, seed, what):
    """(d): recover_below = N_e - n_bad (no recovery: `<`) and that + 1 (recovery); (e): recover_chi2 = the chi2 at the final state of
    the first and of the last flagged edge (not taken back: `<`), and of an edge that no round flagged: it is not `good`, so the count
    of the recovery pass (~good) takes it although its flag (bad & ~good) stays clear"""
    sc, want, calls = imu_base(family, kind, Ne, seed)
    left = int(want["N_e"] - want["round_nbad"][-1])
    if what in ("recover_below", "recover_below+1"):
        return scene(family, name, sc, dict(recover_below=left + (what == "recover_below+1")), [(RECOVERY, -1, what)])
    if not want["recovered"] or len(calls) != RECOVERY + 1:
        return None
    c = calls[RECOVERY][0]
    if what == "recover_chi2-kept":
        kept = np.flatnonzero((want["round_outlier"][-1] == 0) & np.isfinite(c))
        edge, gate = kept[np.argsort(c[kept])[len(kept) // 2]], "recover_chi2_kept"
    else:
        flagged = np.flatnonzero(want["round_outlier"][-1] & np.isfinite(c))
        if not len(flagged):
            return None
        edge, gate = flagged[0 if what == "recover_chi2-first" else -1], "recover_chi2"
    return scene(family, name, sc, dict(recover_chi2=float(c[edge])), [(RECOVERY, int(edge), gate)])


ORIGIN = (-0.25, 0.125, -0.5)   # -tcw of the zero_depth kind (identity rotations, exact floats): Xc = Xw + tcw = (0, 0, 0)


def imu_origin_scene(name, family, Ne, seed=0):
    """(f): the zero_depth kind with its planted point moved to the camera centre: Xc == (0, 0, 0) at the caller's state, so u and v
    are 0 / 0, chi2 is NaN -- `chi2 > thr` is false -- and only `z > 0` flags the edge.  Round 0's sums are not finite, its solve is
    refused and it ends with the state kept: the tie is confirmed there.  From round 1 on the edge is inactive and the state moves."""
    sc = dict(imu_make(family, "zero_depth", Ne, seed))
    pts = sc["points"].copy()
    row = np.flatnonzero((pts == np.array((1.0, 0.5, -0.5), f32)).all(1))
    assert len(row) == 1
    pts[row[0]] = ORIGIN
    sc["points"] = pts
    edge = int(np.flatnonzero(np.asarray(sc["mp_index"])[np.flatnonzero(np.asarray(sc["mp_index"]) >= 0)] == row[0])[0])
    return scene(family, name, sc, {}, [(0, edge, "depth_zero")])


def imu_specs(family):
    out = []
    for (kind, Ne), seed in SEEDS_IMU[family].items():
        name = "%s-N%d-seed%d-" % (kind, Ne, seed)
        if kind == "close_boundary":
            out.append((name + "close_depth", imu_close_depth_scene, (family, kind, Ne, seed)))
            out.append((name + "close_factor", imu_close_factor_scene, (family, kind, Ne, seed)))
        elif kind == "recover":
            out += [(name + what, imu_recover_scene, (family, kind, Ne, seed, what)) for what in RECOVER_WHAT]
        else:
            out += [(name + "edge%d-round%d" % (edge, rnd), imu_round_scene, (family, kind, Ne, seed, rnd, edge)) for edge in positions(Ne)
                    for rnd in range(4)]
    out.append(("origin-N40-seed0", imu_origin_scene, (family, 40)))
    return out


def verify_imu(s):
    family, sc, kw = s["family"], s["sc"], s["kw"]
    want, calls = imu_traced(family, sc, kw)
    assert same_result(want, s["want"])
    prm = imu_params(family, kw)
    close, depth = imu_close(family, sc, kw)
    for rnd, edge, gate in s["ties"]:
        if gate in ("chi2_far", "chi2_close"):
            assert enough_active(want), "%s: fewer than %d active edges in a round" % (s["name"], MIN_ACTIVE)
            thr = f32(prm["chi2"][rnd])
            assert float(thr) == prm["chi2"][rnd]
            bound = thr_close_of(thr, prm["close_factor"]) if gate == "chi2_close" else thr
            if prm["close_factor"] == CLOSE_FACTOR_INEXACT:
                assert f32(f32(prm["close_factor"]) * thr) != bound   # the binary32 product misses the bound
            assert bool(close[edge]) == (gate == "chi2_close") and calls[rnd][1][edge]
            assert calls[rnd][0][edge].tobytes() == bound.tobytes(), "%s: chi2 %r is not on the bound %r" % (s["name"], calls[rnd][0][edge], bound)
            assert want["round_outlier"][rnd, edge] == 0
        elif gate == "close_depth":
            assert enough_active(want)
            thr = f32(prm["chi2"][rnd])
            assert rnd == want["rounds_run"] - 1 and depth[edge].tobytes() == f32(prm["close_depth"]).tobytes() and not close[edge]
            assert float(f32(prm["close_depth"])) == prm["close_depth"]
            assert thr < calls[rnd][0][edge] < thr_close_of(thr, prm["close_factor"]) and calls[rnd][1][edge]
            assert want["round_outlier"][rnd, edge] == 1
        elif gate in ("recover_below", "recover_below+1"):
            left = int(want["N_e"] - want["round_nbad"][-1])
            assert prm["recover_below"] == left + (gate == "recover_below+1") and want["recovered"] == (gate == "recover_below+1")
            assert len(calls) == RECOVERY + want["recovered"]
        elif gate == "recover_chi2":
            assert want["recovered"] == 1 and len(calls) == RECOVERY + 1 and float(f32(prm["recover_chi2"])) == prm["recover_chi2"]
            assert calls[RECOVERY][0][edge].tobytes() == f32(prm["recover_chi2"]).tobytes()
            first = np.flatnonzero(np.asarray(sc["mp_index"]) >= 0)
            assert want["round_outlier"][-1, edge] == 1 and want["outlier"][first[edge]] == 1
        elif gate == "recover_chi2_kept":
            assert want["recovered"] == 1 and len(calls) == RECOVERY + 1 and float(f32(prm["recover_chi2"])) == prm["recover_chi2"]
            assert calls[RECOVERY][0][edge].tobytes() == f32(prm["recover_chi2"]).tobytes()
            first = np.flatnonzero(np.asarray(sc["mp_index"]) >= 0)
            assert want["round_outlier"][-1, edge] == 0 and want["outlier"][first[edge]] == 0
            assert want["n_inliers"] == int((calls[RECOVERY][0] < f32(prm["recover_chi2"])).sum()) < int((want["outlier"][first] == 0).sum())
        elif gate == "depth_zero":
            assert rnd == 0 and want["round_ok"][0] == 0 and want["round_iterations"][0] == 1   # the state of round 0 is the caller's
            _, obs, w, Xw = PR.edges_of(sc["level_sigma2"], sc["kp_xy"], sc["kp_octave"], sc["mp_index"], sc["points"])
            S = R19.State(sc["Rcw"], sc["tcw"], sc["Rwb"], sc["twb"], sc["v"], sc["bg"], sc["ba"])
            _, _, x, y, z = PR.residual(S.Rcw, S.tcw, sc["cam"], obs, Xw)
            assert x[edge] == 0.0 and y[edge] == 0.0 and z[edge] == 0.0
            assert np.isnan(calls[0][0][edge]) and not calls[0][1][edge] and want["round_outlier"][0, edge] == 1
            assert np.isfinite(np.delete(calls[0][0], edge)).all()
        else:
            raise AssertionError(gate)


# ---------------------------------------------------------------------------------------------------------------------
# S12: equal maximal scores.  A min-set may occur twice (only a repeat inside a set is refused), so the winner's set is copied
# ---------------------------------------------------------------------------------------------------------------------
TV_N, TV_ITERATIONS, TV_LANES = 64, 200, 64
# where the copies go: (name, iterations).  twoview_select_kernel gives lane l the iterations l, l + 64, l + 128, l + 192
TV_LAYOUTS = (("same_lane", (37, 101)),          # (a) two iterations of one lane
              ("lower_iteration_higher_lane", (10, 69)),     # (b) a reduction that prefers the lower lane returns 69
              ("lower_iteration_lower_lane", (5, 74)),       # (c) the mirror: one that prefers the higher lane returns 74
              ("four_strides", (7, 71, 135, 199)))           # (d) all four strides of one lane
TV_BASES = (("plane", 0), ("general", 0))   # an H winner and an F winner to copy


def tv_planted(sc, source, its):
    """the scene with the set of iteration `source` copied to the iterations `its`; `source` itself, when it is not one of them, gets
    the set of an iteration that scores less, so that the maximum occurs at `its` only"""
    out = dict(sc)
    sets = sc["sets"].copy()
    for it in its:
        sets[it] = sc["sets"][source]
    if source not in its:
        sets[source] = sc["sets"][next(i for i in range(len(sets)) if i != source and i not in its)]
    out["sets"] = sets
    return out


def tv_models(want, its):
    """which models the planted iterations tie: all their scores are bit-equal and the maximum"""
    n, sc = len(want["scores"]) // 2, want["scores"]
    out = []
    for m, name in enumerate("HF"):
        s = sc[m * n:(m + 1) * n]
        if s[list(its)].tobytes() == np.full(len(its), s.max(), f32).tobytes() and s.max() > 0 and int((s == s.max()).sum()) == len(its):
            out.append(name)
    return out


@functools.lru_cache(maxsize=None)
def tv_base(kind, seed):
    sc = TS.make(kind, TV_N, seed, 0.0, TV_ITERATIONS)
    return sc, run("twoview", sc, {})


def tv_scene(name, kind, seed, model, its):
    base, want = tv_base(kind, seed)
    sc = tv_planted(base, int(want["best_it_" + model]), its)
    w = run("twoview", sc, {})
    ties = [(min(its), -1, "select_" + m) for m in tv_models(w, its)]
    assert ("select_" + model) in [t[2] for t in ties], name
    return scene("twoview", name, dict(sc, planted=its), {}, ties, w)


def tv_no_score_scene(name):
    """random correspondences and sigma = 1e-10: every term of every hypothesis is rejected, no iteration scores above 0"""
    return scene("twoview", name, dict(TS.make("tinysigma", 12, 0, 1.0, TV_ITERATIONS), planted=()), {}, [(-1, -1, "select_none")])


def twoview_specs():
    out = [("%s-seed%d-%s-%s" % (kind, seed, model, name), tv_scene, (kind, seed, model, its)) for kind, seed in TV_BASES for model in "HF"
           for name, its in TV_LAYOUTS]
    return out + [("tinysigma-N12-no_score", tv_no_score_scene, ())]


def verify_twoview(s):
    want = run("twoview", s["sc"], {})
    assert same_result(want, s["want"])
    its = s["sc"]["planted"]
    n = len(want["scores"]) // 2
    assert n == TV_ITERATIONS and want["n_matches"] == s["sc"]["N"]
    for it, _, gate in s["ties"]:
        if gate == "select_none":
            assert not want["scores"].any() and want["best_it_H"] == -1 and want["best_it_F"] == -1 and want["exit_line"] == 110
            continue
        model = gate[-1]
        assert model in tv_models(want, its) and it == min(its) and want["best_it_" + model] == it, (s["name"], want["best_it_" + model])
    assert {gate[-1] for _, _, gate in s["ties"] if gate != "select_none"} == set(tv_models(want, its))


# ---------------------------------------------------------------------------------------------------------------------
# S13: equal inlier counts, min_inliers on a count, th2 on an error
# ---------------------------------------------------------------------------------------------------------------------
ML_N, ML_ITERATIONS = 60, 300   # 300 iterations: the `beaten` loop of mlpnp_refine_kernel (256 threads) makes a second trip
ML_BASE = ("general", ML_N, 0.2, 12, 0.5, 0)   # (kind, N, outliers, min_set, epsilon, seed)
ML_MIN_INLIERS = 20   # below int(N * epsilon) = 30, which is then the solver's mRansacMinInliers
ML_TRIP = MS.REFINE_BLOCK


def ml_base():
    kind, N, outliers, min_set, epsilon, seed = ML_BASE
    sc = MS.make(kind, N, seed, outliers, min_set, epsilon, n_iterations=ML_ITERATIONS, min_inliers=ML_MIN_INLIERS)
    assert len(sc["sets"]) == ML_ITERATIONS
    return sc


def ml_with_sets(sc, moves):
    """moves: [(destination iteration, source iteration)], all read from the scene's own sets"""
    out = dict(sc)
    sets = sc["sets"].copy()
    for dst, src in moves:
        sets[dst] = sc["sets"][src]
    out["sets"] = sets
    return out


def ml_error2(sc, want, it):
    """error2 of every correspondence under hypothesis `it`'s pose, by the lines of mlpnp_ref.check_inliers (:583-592)"""
    idx = want["first"]
    P2D = np.asarray(sc["kp_xy"], f32)[idx]
    X32 = np.asarray(sc["points"], f32)[np.asarray(sc["mp_index"])[idx]]
    Rt = want["hyp_Rt"][it]
    R, t, Xd = Rt[:9].reshape(3, 3), Rt[9:], X32.astype(f64)
    with np.errstate(all="ignore"):
        pc = [(((R[i, 0] * Xd[:, 0] + R[i, 1] * Xd[:, 1]) + R[i, 2] * Xd[:, 2]) + t[i]).astype(f32) for i in range(3)]
        u, v = MR.NR.project(np.asarray(sc["cam"], f32), sc["model"], pc[0], pc[1], pc[2])
        dX, dY = P2D[:, 0] - u, P2D[:, 1] - v
        return dX * dX + dY * dY, P2D, X32


def ml_inlier_at(sc, want, it, corr, bound):
    """mlpnp_ref.check_inliers itself for one correspondence under hypothesis `it`'s pose, with the bound given"""
    idx = want["first"]
    P2D = np.asarray(sc["kp_xy"], f32)[idx][corr:corr + 1]
    X32 = np.asarray(sc["points"], f32)[np.asarray(sc["mp_index"])[idx]][corr:corr + 1]
    Rt = want["hyp_Rt"][it]
    return bool(MR.check_inliers(Rt[None, :9].reshape(1, 3, 3), Rt[None, 9:], np.asarray(sc["cam"], f32), sc["model"], P2D, X32,
                                 np.array([bound], f32))[0, 0])


@functools.lru_cache(maxsize=None)
def ml_base_run():
    base = ml_base()
    want = run("mlpnp", base, {})
    cnt = want["hyp_inliers"]
    best, dull = int(np.argmax(cnt)), int(np.argmin(cnt))   # the first of the largest counts; one that does not qualify
    assert 5 < best < ML_TRIP - 20 and cnt[best] >= want["min_inliers"] and cnt[dull] < want["min_inliers"]
    assert want["n_candidates"] == ML_CANDIDATES
    return base, want, best, dull


ML_CANDIDATES = 2   # of the base scene
ML_WHAT = ("copies_after_best", "copies_in_second_trip") + tuple("min_inliers-cand%d%s" % (c, p) for c in range(ML_CANDIDATES) for p in ("", "+1")) + (
    "refined_min_inliers", "th2-largest", "th2-median")


def ml_scene(name):
    base, want, best, dull = ml_base_run()
    cnt = want["hyp_inliers"]
    if name == "copies_after_best":
        # (a) the best hypothesis's set again later in the first trip of the `beaten` loop and beyond it: equal counts, beaten by the first
        later = (best + 5, ML_TRIP + 14)
        return scene("mlpnp", name, ml_with_sets(base, [(it, best) for it in later]), {}, [(it, -1, "beaten") for it in later])
    if name == "copies_in_second_trip":
        # the best set only beyond the first trip, twice: the second copy is beaten by nothing but an iteration >= 256
        later = (ML_TRIP + 4, ML_TRIP + 30)
        sc = ml_with_sets(base, [(int(j), dull) for j in np.flatnonzero(cnt == cnt[best])] + [(it, best) for it in later])
        return scene("mlpnp", name, sc, {}, [(later[1], -1, "beaten")])
    if name.startswith("min_inliers-cand"):
        # (b) min_inliers on a candidate's count (no earlier iteration reaches it): it qualifies (`>=`); one more and it does not
        it = int(want["candidates"][int(name[len("min_inliers-cand")])])
        plus = name.endswith("+1")
        return scene("mlpnp", name, base, dict(min_inliers=int(cnt[it]) + plus), [(it, -1, "min_inliers+1" if plus else "min_inliers")])
    if name == "refined_min_inliers":
        # (c) min_inliers on a refined count: `candCount > minInliers` fails
        for c in sorted({int(x) for x in want["cand_inliers"]}):
            w = run("mlpnp", base, dict(min_inliers=c))
            hit = np.flatnonzero(w["cand_inliers"] == c)
            if len(hit):
                return scene("mlpnp", name, base, dict(min_inliers=c), [(int(w["candidates"][hit[0]]), -1, "refined")], w)
        return None
    # (d) th2 on the error of an octave-0 correspondence under the best hypothesis's pose (maxErr = sigma2[0] * th2 = th2 exactly)
    e2, _, _ = ml_error2(base, want, best)
    octave = np.asarray(base["kp_octave"])[want["first"]]
    inl = np.flatnonzero((octave == 0) & (e2 < f32(base["ransac"]["th2"])))
    corr = inl[np.argmax(e2[inl])] if name == "th2-largest" else inl[np.argsort(e2[inl])[len(inl) // 2]]
    return scene("mlpnp", name, base, dict(th2=float(e2[corr])), [(best, int(corr), "max_err")])


def mlpnp_specs():
    return [(name, ml_scene, ()) for name in ML_WHAT]


def verify_mlpnp(s):
    sc, kw = s["sc"], s["kw"]
    want = run("mlpnp", sc, kw)
    assert same_result(want, s["want"])
    prm = dict(sc["ransac"])
    prm.update(kw)
    N = want["N"]
    assert MR.plan(N, prm["probability"], prm["min_inliers"], prm["max_iterations"], prm["min_set"], prm["epsilon"], prm["n_iterations"]) == (
        want["min_inliers"], want["max_its"], ML_ITERATIONS) and want["total_iterations"] == ML_ITERATIONS == len(sc["sets"])
    cnt, nMin, cands = want["hyp_inliers"], want["min_inliers"], list(want["candidates"])
    for it, corr, gate in s["ties"]:
        if gate == "beaten":
            first = int(np.flatnonzero(cnt == cnt[it])[0])
            assert cnt[it] == cnt.max() >= nMin and first < it and first in cands and it not in cands
            assert np.array_equal(sc["sets"][it], sc["sets"][first])
            if s["name"] == "copies_in_second_trip":
                assert first >= ML_TRIP and not (cnt[:first] >= cnt[it]).any()
            else:
                assert first < ML_TRIP and any(i < ML_TRIP for i, _, _ in s["ties"]) and any(i >= ML_TRIP for i, _, _ in s["ties"])
        elif gate == "min_inliers":
            assert cnt[it] == nMin == prm["min_inliers"] and it in cands
        elif gate == "min_inliers+1":
            assert cnt[it] + 1 == nMin == prm["min_inliers"] and it not in cands
        elif gate == "refined":
            c = cands.index(it)
            assert want["cand_inliers"][c] == nMin == prm["min_inliers"]
            assert want["exit_kind"] == MR.EXIT_BEST or want["returning_iteration"] > it
        elif gate == "max_err":
            e2 = ml_error2(sc, want, it)[0][corr]
            assert float(f32(prm["th2"])) == prm["th2"] and e2.tobytes() == f32(prm["th2"]).tobytes()
            assert np.asarray(sc["kp_octave"])[want["first"]][corr] == 0 and f32(sc["level_sigma2"][0]) == 1.0
            # the restatement's own check: not an inlier at the bound, an inlier one unit in the last place above it
            assert not ml_inlier_at(sc, want, it, corr, f32(prm["th2"]))
            assert ml_inlier_at(sc, want, it, corr, np.nextafter(f32(prm["th2"]), f32(np.inf)))
        else:
            raise AssertionError(gate)


# ---------------------------------------------------------------------------------------------------------------------
SPECS = dict(poseopt=poseopt_specs, inertial=lambda: imu_specs("inertial"), inertial_prev=lambda: imu_specs("inertial_prev"),
             twoview=twoview_specs, mlpnp=mlpnp_specs)
VERIFY = dict(poseopt=verify_poseopt, inertial=verify_imu, inertial_prev=verify_imu, twoview=verify_twoview, mlpnp=verify_mlpnp)
# every gate a family's scenes must hit exactly
GATES = dict(poseopt={"chi2_threshold"},
             inertial={"chi2_far", "chi2_close", "close_depth", "recover_below", "recover_below+1", "recover_chi2", "recover_chi2_kept",
                      "depth_zero"},
             inertial_prev={"chi2_far", "chi2_close", "close_depth", "recover_below", "recover_below+1", "recover_chi2", "recover_chi2_kept",
                      "depth_zero"},
             twoview={"select_H", "select_F", "select_none"},
             mlpnp={"beaten", "min_inliers", "min_inliers+1", "refined", "max_err"})


def names(family):
    """the scenes of a family by name, without building any (no restatement runs)"""
    return [name for name, _, _ in SPECS[family]()]


@functools.lru_cache(maxsize=None)
def build(family, name):
    """one scene: the restatement runs once or twice; base runs are shared"""
    fn, args = {n: (f, a) for n, f, a in SPECS[family]()}[name]
    s = fn(name, *args)
    assert s, "%s %s no longer gives its tie" % (family, name)
    return s


def scenes(family):
    return [build(family, name) for name in names(family)]


def verify(s):
    VERIFY[s["family"]](s)

"""SPEC DECISION S12 (twoview_ref.reconstruct: binary32 + the pinned Jacobi sequences) measured against the same function in
binary64 with numpy.linalg.svd for all four decompositions (twoview_ref.reconstruct_f64) on the scenes of twoview_scenarios,
and the properties S12 states about itself (sweep count, which exits the scenes reach).  No GPU: the kernels are compared
with `reconstruct` byte for byte in test_twoview_gpu.py.

Gates: DESIGN.md S12 records the worst values of the two measured seeds (0 and 3) over all scenes; every gate here is twice
that worst value -- a margin for the second seed pair the test adds (2 and 5), not for the kernels.  The motion (c) and the
points (d) are those the call returns, so they are compared where both runs reconstruct; the flags (a) are compared for
every motion hypothesis of every scene."""
import functools

import numpy as np
import pytest

import twoview_ref as R
import twoview_scenarios as TS

SEEDS = (0, 3, 2, 5)
# measured worst over seeds 0 and 3 x TS.CASES -> gate = 2 x worst:
#   share of flipped inlier-mask entries / CheckRT flags, relative difference of SH and SF, angle between the returned rotations
#   / translations (degrees), relative distance of the returned points, relative distance of a flipped flag from its threshold
WORST = dict(mask_flips=0.0, rt_flips=0.00167, score_rel=3.54e-05, rot_deg=0.0338, t_deg=0.000174, x3d_rel=1.87e-05, flip_dist=8.82e-08)
GATE = {k: 2.0 * v for k, v in WORST.items()}


def _angle_deg(c):
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def rot_angle(Ra, Rb):
    return _angle_deg((np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1.0) / 2.0)


def vec_angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return _angle_deg(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def match_hypotheses(s, e):
    """the two runs list the same motion hypotheses in an order that depends on the signs their decompositions came with:
    pair every S12 hypothesis with the closest binary64 one"""
    n = s["n_hypotheses"]
    pairs = []
    for h in range(n):
        cost = [rot_angle(s["hyp_R"][h], e["hyp_R"][k]) + vec_angle(s["hyp_t"][h], e["hyp_t"][k]) for k in range(n)]
        pairs.append(int(np.argmin(cost)))
    return pairs


def _flip_distance(th, *values):
    """relative distance to the threshold of the nearest gate value of every flipped entry"""
    d = np.min([np.abs(np.asarray(v, np.float64) - th) / th for v in values], axis=0)
    return d


def compare(s, e):
    """S12 result s against the binary64 result e -> dict of figures (and the discrete agreements)"""
    m = dict(same_itH=s["best_it_H"] == e["best_it_H"], same_itF=s["best_it_F"] == e["best_it_F"], same_model=s["model"] == e["model"],
             same_flag=bool(s["reconstructed"]) == bool(e["reconstructed"]), same_exit=s["exit_line"] == e["exit_line"],
             RH64=float(e["RH"]), mask_flips=0.0, rt_flips=0.0, score_rel=0.0, rot_deg=0.0, t_deg=0.0, x3d_rel=0.0, flip_dist=0.0)
    if s["n_matches"] < 8:
        return m
    N = s["n_matches"]
    flips, dist = 0, [0.0]
    for key, chi, th in (("inliers_H", "chi_H", 5.991), ("inliers_F", "chi_F", 3.841)):
        if s["best_it_" + key[-1]] < 0 or not m["same_it" + key[-1]]:
            continue
        bad = np.flatnonzero(s[key] != e[key])
        flips += len(bad)
        if len(bad):
            dist.append(float(_flip_distance(th, e[chi][0][bad], e[chi][1][bad]).max()))
    m["mask_flips"] = flips / (2.0 * N)
    for a, b in ((s["SH"], e["SH"]), (s["SF"], e["SF"])):
        if b != 0:
            m["score_rel"] = max(m["score_rel"], abs(float(a) - float(b)) / float(b))
    if s["n_hypotheses"] and s["n_hypotheses"] == e["n_hypotheses"] and m["same_model"]:
        pairs = match_hypotheses(s, e)
        rt, th2 = 0, 4.0 * float(np.float32(1.0))
        for h, k in enumerate(pairs):
            bad = np.flatnonzero(s["rt_flags"][h] != e["rt_flags"][k])
            rt += len(bad)
            if len(bad):
                d = e["details"][k]
                near = np.min([np.abs(d["err1"][bad] - th2) / th2, np.abs(d["err2"][bad] - th2) / th2,
                               np.abs(d["cos"][bad] - 0.99998) / 0.99998, np.abs(d["Z"][bad]) / (np.abs(d["Z"][bad]) + 1.0),
                               np.abs(d["Z2"][bad]) / (np.abs(d["Z2"][bad]) + 1.0)], axis=0)
                dist.append(float(near.max()))
        if s["reconstructed"] and e["reconstructed"]:  # the motion and the points the call returns
            m["rot_deg"] = rot_angle(s["R21"], e["R21"])
            m["t_deg"] = vec_angle(s["t21"], e["t21"])
            both = s["triangulated"].astype(bool) & e["triangulated"].astype(bool)
            xs, xe = s["p3d"][both].astype(np.float64), e["p3d"][both]
            m["x3d_rel"] = float((np.linalg.norm(xs - xe, axis=1) / np.linalg.norm(xe, axis=1)).max())
        m["rt_flips"] = rt / float(s["n_hypotheses"] * N)
    m["flip_dist"] = max(dist)
    return m


@functools.lru_cache(maxsize=None)
def runs(case, seed):
    sc = TS.make(case[0], case[1], seed, case[2], case[3])
    return TS.ref(sc), TS.ref(sc, exact=True)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("case", TS.CASES, ids=TS.case_id)
def test_s12_against_binary64(case, seed):
    s, e = runs(case, seed)
    m = compare(s, e)
    print(TS.case_id(case), seed, m)
    assert not 0.35 <= m["RH64"] <= 0.45, "RH %.3f: the scene sits on the model threshold" % m["RH64"]
    assert m["same_itH"] and m["same_itF"], "winning iterations differ: %d / %d vs %d / %d" % (
        s["best_it_H"], s["best_it_F"], e["best_it_H"], e["best_it_F"])
    assert m["same_model"] and m["same_flag"] and m["same_exit"]
    for k in GATE:
        assert m[k] <= GATE[k], "%s = %.3g above the gate %.3g" % (k, m[k], GATE[k])


def test_scenes_reach_every_exit_and_both_models():
    """seed 0 (the scenes of test_twoview_gpu.py) reaches every `return false` and a success of each model, in both runs"""
    for which in (0, 1):
        exits, ok = set(), set()
        for case in TS.CASES:
            s = runs(case, 0)[which]
            exits.add(s["exit_line"])
            if s["reconstructed"]:
                ok.add(s["model"])
        assert exits >= {0, 110, 528, 580, 609, 746}, exits
        assert ok == {R.MODEL_H, R.MODEL_F}, ok


def test_ten_and_twelve_sweeps_give_the_same_scores():
    """S12 fixes the sweep count at 10: 12 sweeps change no score byte on the test scenes.  One stated exception: `static`
    (the same keypoints twice) makes the 8 x 9 system of ComputeF21 exactly degenerate -- columns 1 / 3, 2 / 6 and 5 / 7 of A are
    equal, so the null space is three-dimensional and an eigenvector inside it is not determined by any sweep count (measured:
    1 of the 200 F scores moves by one unit in the last place between 10 and 12 sweeps).  There the H scores, both winners and
    their scores are still byte-equal."""
    for case in TS.CASES[:10]:
        sc = TS.make(case[0], case[1], 0, case[2], case[3])
        fx, fy, cx, cy, sigma, it = sc["params"]
        a = runs(case, 0)[0]
        b = R.reconstruct(fx, fy, cx, cy, sigma, it, sc["kp1"], sc["kp2"], sc["matches12"], sc["sets"], sweeps=12)
        if case[0] != "static":
            assert a["scores"].tobytes() == b["scores"].tobytes(), TS.case_id(case)
            continue
        assert a["scores"][:it].tobytes() == b["scores"][:it].tobytes()
        moved = np.flatnonzero(a["scores"][it:] != b["scores"][it:])
        assert len(moved) <= 2 and np.all(np.abs(a["scores"][it:][moved] - b["scores"][it:][moved]) <= 2e-7 * b["scores"][it:][moved])
        for k in ("SH", "SF", "best_it_H", "best_it_F", "inliers_H", "inliers_F", "H21", "F21"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_round_order_and_set_drawing():
    """the pair order of S12: 9 rounds of 4 disjoint pairs that cover all 36 pairs once; mvSets as :75-94 draws them"""
    seen = [p for r in R.ROUNDS9 for p in r]
    assert len(seen) == 36 and len(set(seen)) == 36 and all(i < j and (i + j) % 9 == r for r, ps in enumerate(R.ROUNDS9) for i, j in ps)
    assert R.ROUNDS9[0] == [(1, 8), (2, 7), (3, 6), (4, 5)] and R.ROUNDS9[1] == [(0, 1), (2, 8), (3, 7), (4, 6)]
    vals = iter([0, 2 ** 31 - 1, 2 ** 30] + [12345678 * k % (2 ** 31) for k in range(1, 30)])
    sets = R.draw_sets(20, 2, lambda: next(vals))
    assert sets[0, 0] == 0 and sets[0, 1] == 18 and sets[0, 2] == 9  # rand() = 0, RAND_MAX, 2^30 on 20, 19, 18 candidates
    assert all(len(set(row)) == 8 and min(row) >= 0 and max(row) < 20 for row in sets)


def test_fewer_than_eight_matches_and_normalize():
    sc = TS.make("general", 64, 0, 0.0, 7)
    m12 = sc["matches12"].copy()
    m12[np.flatnonzero(m12 >= 0)[7:]] = -1
    r = R.reconstruct(*sc["params"], sc["kp1"], sc["kp2"], m12, None)
    assert not r["reconstructed"] and r["exit_line"] == 62 and r["n_matches"] == 7
    pts, T = R.normalize(sc["kp1"], np.float32)
    assert pts.dtype == np.float32 and abs(float(np.abs(pts[:, 0]).mean()) - 1.0) < 1e-4 and T[2, 2] == 1.0

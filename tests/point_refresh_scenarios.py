"""Graphs for the S26 tests (tests/point_refresh_ref.py): ONE planted graph in which every point is a case worked out by hand, with the
mutants each case tells from the rule; the shapes at which the kernels change path (observer counts around the 64 lanes of the wave
path); and a random graph.  No orbfe import except in upload()."""
import copy

import numpy as np

import point_refresh_ref as P

f32 = np.float32
N_LEVELS = 8
SCALE_FACTORS = np.array([f32(1.2) ** i for i in range(N_LEVELS)], f32)   # mvScaleFactors of ORBextractor(scaleFactor = 1.2, nlevels = 8)


def bits(k):
    """the descriptor whose first k bits are set: the Hamming distance of bits(a) and bits(b) is |a - b|"""
    d = np.zeros(32, np.uint8)
    d[:k // 8] = 255
    if k % 8:
        d[k // 8] = (1 << (k % 8)) - 1
    return d


# ---- the planted graph ----
# Ten key frames; mn_id runs against the slot so that "lowest mn_id" and "lowest slot / first in the list" differ.  Key frame 8 is bad,
# key frame 6 has only 3 features, the others 16.  Every octave is 7 (the last level, where min = max / sf[level] either way) except
# where a case says otherwise.  Point c uses feature index c in each of its observers unless the case says otherwise; a feature's
# descriptor is bits(v) for the value v the case gives, so a row of distances is the row of |v - v'|.
PLANTED_MN_ID = [50, 9, 5, 7, 30, 31, 32, 33, 3, 35]
PLANTED_BAD_KF = 8
PLANTED_SHORT_KF, PLANTED_SHORT_N = 6, 3
# name: (point id, {slot: value}, reference slot, what it must give, the mutants that change it and ONLY these).  A mutant is planted
# in the case whose comment works it out; it also shows wherever its rule is in play: every N = 2 case reports the distance instead of 0
# as its median under the two median mutants, and the closest pair of any small set ties, so the tie mutant shows in most cases.
CASES = {}


def _case(name, p, values, ref, expect, mutants, idx=None, bad=False, octave=None):
    CASES[name] = dict(p=p, values=values, ref=ref, expect=expect, mutants=tuple(mutants), idx=idx or {}, bad=bad, octave=octave or {})


# N = 6, position (size_t)2.5 = 2.  Rows sorted (value: row): 0: 0 4 9 15 22 40; 4: 0 4 5 11 18 36; 9: 0 5 6 9 13 31; 15: 0 6 7 11 15 25;
# 22: 0 7 13 18 18 22; 40: 0 18 25 31 36 40.  Position 2: 9 5 6 7 13 25 -> key frame 1 (value 4), median 5.  Position 3 (rounded up, and
# also what leaving the self-distance out reads): 15 11 9 11 18 31 -> key frame 2.
_case("even_n", 0, {0: 0, 1: 4, 2: 9, 3: 15, 4: 22, 5: 40}, 0, dict(best=(1, 0, 5), status=3), ("median_rounded_up", "no_self_distance"))
# N = 5, position 2 exactly.  0: 0 4 9 15 30; 4: 0 4 5 11 26; 9: 0 5 6 9 21; 15: 0 6 11 15 15; 30: 0 15 21 26 30.  Position 2: 9 5 6 11 21 ->
# key frame 1, median 5.  Without the self-distance position 2 reads 15 11 9 15 26 -> key frame 2.
_case("odd_n", 1, {0: 0, 1: 4, 2: 9, 3: 15, 4: 30}, 0, dict(best=(1, 1, 5), status=3), ("no_self_distance",))
# N = 2: position (size_t)0.5 = 0, both medians are the self-distance 0 whatever the descriptors: the lower mn_id (key frame 1: 9 < 50)
_case("two", 2, {0: 3, 1: 200}, 0, dict(best=(1, 2, 0), status=3), ("median_rounded_up", "no_self_distance", "ties_highest_id"))
# N = 3, a descriptor duplicated: rows 0 0 77 | 0 0 77 | 0 77 77, position 1: 0 0 77: key frames 0 (mn_id 50) and 3 (7) tie -> 3
_case("dup3", 3, {0: 100, 3: 100, 2: 177}, 3, dict(best=(3, 3, 0), status=3), ("no_self_distance", "ties_highest_id"))
# N = 4, two pairs: every row is 0 0 d d, position 1: all four medians 0 -> the lowest mn_id of the four (key frame 2: 5)
_case("dup4", 4, {0: 10, 4: 10, 2: 60, 5: 60}, 4, dict(best=(2, 4, 0), status=3), ("median_rounded_up", "no_self_distance", "ties_highest_id"))
# a bad observer (key frame 8, mn_id 3) between two good ones: N = 2 -> key frame 1.  Collected, rows 0 1 20 | 0 1 19 | 0 19 20, position 1:
# 1 1 19 -> key frames 0 and 8 tie and 8 wins
_case("bad_observer", 5, {0: 0, 8: 1, 1: 20}, 0, dict(best=(1, 5, 0), status=3),
      ("median_rounded_up", "no_self_distance", "ties_highest_id", "bad_observers_collected"))
# index -1 (key frame 1): N = 2 -> key frame 2 (5 < 50).  Collected (the mutant reads the key frame's last feature, planted as bits(1)):
# 1 1 19 -> key frames 0 and 1 tie and 1 wins
_case("index_minus_one", 6, {0: 0, 1: None, 2: 20}, 0, dict(best=(2, 6, 0), status=3),
      ("median_rounded_up", "no_self_distance", "ties_highest_id", "index_minus_one_collected"),
      idx={1: -1})
# the depth: reference key frame 1 whose feature has octave 3 (max = dist sf[3], min = max / sf[7]); the descriptor comes from key frame
# 2 (rows 0 30 60 | 0 30 30 | 0 30 60, position 1: all three medians are 30 -> the lowest mn_id), whose feature has octave 5
_case("depth_level", 7, {0: 0, 2: 30, 1: 60}, 1, dict(best=(2, 7, 30), status=3, level=3), ("ties_highest_id", "min_by_level_scale", "level_from_winner"),
      octave={1: 3, 2: 5})
# the reference key frame 4 does not observe the point: index 0 as written, level = the octave of key frame 4's feature 0
_case("ref_not_observer", 8, {0: 0, 1: 9}, 4, dict(best=(1, 8, 0), status=3, level=7),
      ("median_rounded_up", "no_self_distance", "ties_highest_id", "ref_not_observer_nothing"))
# a bad point is left alone
_case("bad_point", 9, {0: 0, 1: 9}, 0, dict(best=(-1, -1, -1), status=0), ("bad_point_refreshed",), bad=True)
# no observations: left alone
_case("no_observers", 10, {}, 0, dict(best=(-1, -1, -1), status=0), ())
# no reference key frame: the descriptor alone
_case("ref_none", 11, {0: 0, 1: 9, 2: 30}, -1, dict(best=(1, 11, 9), status=2), ("no_self_distance", "ties_highest_id"))
# the reference key frame's observation has index -1: no depth; it is not collected either: N = 2 -> key frame 2
_case("ref_index_minus_one", 12, {0: 0, 1: None, 2: 9}, 1, dict(best=(2, 12, 0), status=2),
      ("median_rounded_up", "no_self_distance", "ties_highest_id", "index_minus_one_collected"),
      idx={1: -1})
# the reference key frame 6 has 3 features and the observation names feature 13: no depth, not collected
_case("ref_index_beyond", 13, {0: 0, 6: None, 2: 9}, 6, dict(best=(2, 13, 0), status=2), ("median_rounded_up", "no_self_distance", "ties_highest_id"))
# nothing collected (a bad observer and an index of -1) but a depth: the reference key frame 0 is no observer, index 0
_case("none_collected", 14, {8: 5, 1: None}, 0, dict(best=(-1, -1, -1), status=1, level=7),
      ("bad_observers_collected", "index_minus_one_collected", "ref_not_observer_nothing"), idx={1: -1})
# the reference key frame is bad: not tested (:458), the depth is written; the bad observer is not collected
_case("ref_bad", 15, {8: 0, 0: 7, 2: 9}, 8, dict(best=(2, 15, 0), status=3, level=7),
      ("median_rounded_up", "no_self_distance", "ties_highest_id", "bad_observers_collected"))
PLANTED_IDS = [c["p"] for c in CASES.values()]


def planted_graph():
    g = P.new_graph(10, 20)
    for s, mn in enumerate(PLANTED_MN_ID):
        g.set_keyframe(s, mn, bad=s == PLANTED_BAD_KF, points=[])
    rg = P.RefreshGraph(g, kf_stride=16, obs_stride=8, scale_factors=SCALE_FACTORS)
    rng = np.random.default_rng(26)
    desc = [rng.integers(0, 256, (PLANTED_SHORT_N if s == PLANTED_SHORT_KF else 16, 32)).astype(np.uint8) for s in range(10)]
    octave = [np.full(len(d), 7, np.int32) for d in desc]
    rg.centre[:] = rng.uniform(-2, 2, (10, 3)).astype(f32)
    rg.pos[:] = rng.uniform(-9, 9, (20, 3)).astype(f32)
    rg.min_distance[:], rg.max_distance[:] = f32(0.25), f32(64)          # what an untouched record keeps
    rg.map_desc[:] = 0xa5
    for c in CASES.values():
        p = c["p"]
        slots = list(c["values"])
        rg.set_observations(p, slots, [c["idx"].get(s, p) for s in slots])
        rg.ref[p] = c["ref"]
        g.point_bad[p] = c["bad"]
        for s, v in c["values"].items():
            if v is not None:
                desc[s][p] = bits(v)
        for s, o in c["octave"].items():
            octave[s][p] = o
    desc[1][15] = bits(1)                                                # what "index -1 collected" reads in key frame 1
    for s in range(10):
        rg.set_features(s, octave[s], desc[s])
    return rg


def expected(rg, name):
    """the outputs of a planted case from its hand-worked `expect`, the depth from the formula"""
    c = CASES[name]
    e = c["expect"]
    out = dict(status=e["status"], best_slot=e["best"][0], best_index=e["best"][1], best_median=e["best"][2], min_distance=f32(0), max_distance=f32(0))
    if e["status"] & 1:
        dist = P.point_distance(rg.pos[c["p"]], rg.centre[c["ref"]])
        out["max_distance"] = f32(dist * SCALE_FACTORS[e.get("level", 7)])
        out["min_distance"] = f32(out["max_distance"] / SCALE_FACTORS[N_LEVELS - 1])
    return out


# ---- shapes ----
OBSERVER_COUNTS = (0, 1, 2, 3, 4, 63, 64, 65, 130)
GPU_KF_CAPACITY, GPU_KF_STRIDE, GPU_OBS_STRIDE = 140, 40, 160


def shapes_graph(seed=5):
    """kf_capacity 140, kf_stride 40, obs_stride 160, 8 levels.  Point k of the first len(OBSERVER_COUNTS) has OBSERVER_COUNTS[k] observers;
    the points behind them are random (0..12 observers) and carry the corner cases at random: bad key frames, indices of -1, a bad point,
    a reference key frame that is no observer or none, an index beyond a short key frame.  Descriptors are drawn around a few centres with
    few bits flipped, so equal medians are common and mn_id decides often."""
    rng = np.random.default_rng(seed)
    K, C = GPU_KF_CAPACITY, 96
    g = P.new_graph(K, C)
    mn = rng.permutation(K) + 10
    for s in range(K - 2):                                               # the last two slots stay unset (bad, no features)
        g.set_keyframe(s, int(mn[s]), bad=bool(rng.random() < 0.1), points=[])
    rg = P.RefreshGraph(g, GPU_KF_STRIDE, GPU_OBS_STRIDE, SCALE_FACTORS)
    centres = rng.integers(0, 256, (4, 32)).astype(np.uint8)
    for s in range(K - 2):
        n = GPU_KF_STRIDE if s % 7 else 5                                # short key frames
        d = centres[rng.integers(0, 4, n)].copy()
        flips = rng.integers(0, 256, (n, 3))
        for i in range(n):
            for b in flips[i][:rng.integers(0, 4)]:
                d[i, b // 8] ^= 1 << (b % 8)
        rg.set_features(s, rng.integers(0, N_LEVELS, n), d)
    rg.centre[:] = rng.uniform(-3, 3, (K, 3)).astype(f32)
    rg.pos[:] = rng.uniform(-20, 20, (C, 3)).astype(f32)
    rg.min_distance[:], rg.max_distance[:] = f32(0.5), f32(32)
    rg.map_desc[:] = 0x5a
    for p in range(C):
        n = OBSERVER_COUNTS[p] if p < len(OBSERVER_COUNTS) else int(rng.integers(0, 13))
        slots = rng.permutation(K)[:n]
        idx = [int(rng.integers(0, GPU_KF_STRIDE)) if rng.random() > 0.08 else -1 for _ in slots]
        rg.set_observations(p, slots, idx)
        u = rng.random()
        rg.ref[p] = -1 if u < 0.05 else (int(rng.integers(0, K)) if u < 0.15 or n == 0 else int(slots[rng.integers(0, n)]))
        g.point_bad[p] = p >= len(OBSERVER_COUNTS) and rng.random() < 0.08
    return rg


def uniform_graph(n_points, n_obs, seed=1):
    """the shapes of tests/tools/point_refresh_latency.py: n_points points with n_obs observers each out of 200 key frames of 1000 features"""
    rng = np.random.default_rng(seed)
    K, stride = 200, 1000
    g = P.new_graph(K, n_points)
    for s in range(K):
        g.set_keyframe(s, s, points=[])
    rg = P.RefreshGraph(g, stride, max(n_obs, 1), SCALE_FACTORS)
    for s in range(K):
        rg.set_features(s, rng.integers(0, N_LEVELS, stride), rng.integers(0, 256, (stride, 32)).astype(np.uint8))
    rg.centre[:] = rng.uniform(-3, 3, (K, 3)).astype(f32)
    rg.pos[:] = rng.uniform(-20, 20, (n_points, 3)).astype(f32)
    for p in range(n_points):
        slots = rng.permutation(K)[:n_obs]
        rg.set_observations(p, slots, rng.integers(0, stride, n_obs))
        rg.ref[p] = int(slots[0])
    return rg


def state(rg, ids=None):
    """every point as orbfe_covis_get_point reads it back, as plain data"""
    out = []
    for p in (range(rg.g.capacity) if ids is None else ids):
        q = rg.point(p)
        out.append((q["obs"], q["ref"], np.float32(q["min_distance"]).tobytes(), np.float32(q["max_distance"]).tobytes(), q["desc"].tobytes()))
    return out


def same_outputs(a, b):
    """exact: the distances as bit patterns"""
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).astype(np.asarray(a[k]).dtype).tobytes() for k in a)


def upload(orbfe, ex, rg, child_stride=4, enable=True):
    """-> (MapPoints, Covisibility) holding the graph with its refresh state"""
    g = rg.g
    mp = orbfe.MapPoints(ex, g.capacity)
    pts = np.zeros(g.capacity, orbfe.WP_DTYPE)
    pts["x"], pts["y"], pts["z"] = rg.pos[:, 0], rg.pos[:, 1], rg.pos[:, 2]
    pts["min_distance"], pts["max_distance"] = rg.min_distance, rg.max_distance
    pts["bad"] = g.point_bad
    pts["observations"] = [len(o) for o in g.obs]
    mp.update(np.arange(g.capacity), pts, rg.map_desc)
    cv = orbfe.Covisibility(ex, mp, g.kf_capacity, rg.kf_stride, rg.obs_stride, child_stride)
    cv.set_keyframes([g.record(s) for s in range(g.kf_capacity) if g.is_set[s]])
    if not enable:
        return mp, cv
    cv.enable_refresh(rg.sf)
    for s in range(g.kf_capacity):
        if len(rg.desc[s]):
            kp = np.zeros(len(rg.desc[s]), orbfe.KP_DTYPE)
            kp["octave"] = rg.octave[s]
            cv.set_features(s, kp, rg.desc[s])
    cv.set_centres(np.arange(g.kf_capacity), rg.centre)
    ids = [p for p in range(g.capacity) if g.obs[p]]
    off = np.zeros(len(ids) + 1, np.int32)
    off[1:] = np.cumsum([len(g.obs[p]) for p in ids])
    cv.set_observations_indexed(ids, off, [s for p in ids for s in g.obs[p]], [i for p in ids for i in rg.obs_idx[p]])
    cv.set_ref_keyframes(np.arange(g.capacity), rg.ref)
    return mp, cv


def read_state(cv, rg, ids=None):
    """the same tuple as state(), read back from the device"""
    out = []
    for p in (range(rg.g.capacity) if ids is None else ids):
        q = cv.get_point(p)
        out.append((q["obs"], q["ref"], np.float32(q["record"]["min_distance"]).tobytes(), np.float32(q["record"]["max_distance"]).tobytes(),
                    q["desc"].tobytes()))
    return out


def clone(rg):
    return copy.deepcopy(rg)

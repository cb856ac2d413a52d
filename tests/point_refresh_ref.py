"""MapPoint::UpdateDepth (src/MapPoint.cc:440-474) and MapPoint::ComputeDistinctiveDescriptors (:343-417) restated on the flat tables of
orbfe_covis: SPEC DECISION S26, normative for orbfe_covis_refresh_points_device / _refresh_points, for the index
that orbfe_covis_add_keyframe* store on a graph with refresh state, and for the host restatement of tests/cpp/point_refresh.cpp.
Written from the reference's lines, which the comments cite; where the reference leaves the result open (the iteration order of a
std::map keyed by pointer, reads outside a container) S26 pins it and the comment says so.

RefreshGraph holds the Graph of tests/local_map_ref.py (key frames, observation lists as slots, bad flags) and adds what S26 keeps: per
key frame the descriptors, octaves and camera centre, per point the feature index of every observation and mpRefKF, and the map's own
records that the call writes.  Binary32 where S26 says so: every operation of the depth is one numpy float32 operation.  MUTANTS are
deliberate mis-readings of one rule each; tests/test_point_refresh.py proves that the planted scene tells every mutant from the rule."""
import numpy as np

import local_map_ref as R

DEPTH, DESCRIPTOR = 1, 2
MUTANTS = ("median_rounded_up", "no_self_distance", "ties_highest_id", "bad_observers_collected", "index_minus_one_collected",
           "min_by_level_scale", "level_from_winner", "ref_not_observer_nothing", "bad_point_refreshed")
f32 = np.float32
_POP = np.array([bin(v).count("1") for v in range(256)], np.int32)


class RefreshGraph:
    def __init__(self, g, kf_stride, obs_stride, scale_factors):
        self.g = g
        self.kf_stride, self.obs_stride = int(kf_stride), int(obs_stride)
        self.sf = np.asarray(scale_factors, f32).copy()
        self.n_levels = len(self.sf)
        K, C = g.kf_capacity, g.capacity
        self.desc = [np.zeros((0, 32), np.uint8) for _ in range(K)]       # mDescriptors; its length is the feature count
        self.octave = [np.zeros(0, np.int32) for _ in range(K)]          # mvKeysUn[i].octave
        self.centre = np.zeros((K, 3), f32)                              # GetTranslationInverse()
        self.obs_idx = [[-1] * len(o) for o in g.obs]                    # leftIndex, parallel to g.obs[p]
        self.ref = np.full(C, -1, np.int64)                              # mpRefKF as a slot
        self.pos = np.zeros((C, 3), f32)                                 # the map's records: position (never written here) ...
        self.min_distance = np.zeros(C, f32)                             # ... and what the call writes
        self.max_distance = np.zeros(C, f32)
        self.map_desc = np.zeros((C, 32), np.uint8)

    def set_features(self, slot, octave, desc):
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        assert len(octave) == len(desc) <= self.kf_stride
        self.desc[slot] = desc.copy()
        self.octave[slot] = np.clip(np.asarray(octave, np.int32), 0, self.n_levels - 1)   # the device form clamps; the host form refuses

    def set_observations(self, p, slots, idx=None):
        self.g.obs[p] = [int(s) for s in slots]
        self.obs_idx[p] = [-1] * len(slots) if idx is None else [int(i) for i in idx]

    def point(self, p):
        """what orbfe_covis_get_point reads back"""
        return dict(obs=list(zip(self.g.obs[p], self.obs_idx[p])), ref=int(self.ref[p]), min_distance=f32(self.min_distance[p]),
                    max_distance=f32(self.max_distance[p]), desc=self.map_desc[p].copy())

    def index_added(self, slot, point_ids, added):
        """behind add_keyframe on a graph with refresh state: feature slot i with added[i] == 1 is the index of the observation that
        tests/covis_update_ref.py add_keyframe just appended; the lists that grew are brought to length first"""
        for p in range(self.g.capacity):
            self.obs_idx[p] += [-1] * (len(self.g.obs[p]) - len(self.obs_idx[p]))
        for i, (p, a) in enumerate(zip(point_ids, added)):
            if a == 1:
                self.obs_idx[int(p)][self.g.obs[int(p)].index(slot)] = i


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def point_distance(pos, centre):
    """|Pos - centre| in binary32: sqrt((x x + y y) + z z), every operation rounded once (Eigen's norm() is not pinned, S26)"""
    d = [f32(f32(pos[i]) - f32(centre[i])) for i in range(3)]
    xx, yy, zz = f32(d[0] * d[0]), f32(d[1] * d[1]), f32(d[2] * d[2])
    return f32(np.sqrt(f32(f32(xx + yy) + zz)))


def _feature(rg, slot, idx):
    """(slot, idx) names a feature of a key frame of the graph"""
    return 0 <= slot < rg.g.kf_capacity and 0 <= idx < len(rg.desc[slot])


def distinctive(rg, p, mutant=None):
    """ComputeDistinctiveDescriptors -> (slot, index, median) of the chosen observation, or None when nothing is collected"""
    g = rg.g
    got = []                                                             # (position in the list, slot, index)
    for j, (s, i) in enumerate(zip(g.obs[p], rg.obs_idx[p])):
        if not (0 <= s < g.kf_capacity):
            continue
        if g.kf_bad[s] and mutant != "bad_observers_collected":          # :366
            continue
        if i == -1:                                                      # :370
            if mutant != "index_minus_one_collected" or len(rg.desc[s]) == 0:
                continue
            i = len(rg.desc[s]) - 1                                      # (the mutant reads the row "before the first": the last)
        if not _feature(rg, s, i):                                       # S26: an index that names no feature is not collected
            continue
        got.append((j, s, i))
    N = len(got)
    if N == 0:                                                           # :379
        return None
    D = np.array([[hamming(rg.desc[sa][ia], rg.desc[sb][ib]) for _, sb, ib in got] for _, sa, ia in got], np.int32)
    k = int(0.5 * (N - 1))                                               # :404, the double truncated
    if mutant == "median_rounded_up":
        k = int(np.ceil(0.5 * (N - 1)))
    best = None
    for r, (j, s, i) in enumerate(got):
        row = D[r]
        if mutant == "no_self_distance":
            row = np.delete(row, r)
            if len(row) == 0:
                row = np.zeros(1, np.int32)
        # the element at position k of the sorted row = the smallest v with #{dist <= v} >= k + 1
        kk = min(k, len(row) - 1)
        median = next(v for v in range(257) if int((row <= v).sum()) >= kk + 1)
        # S26: least (median, mn_id, position); the reference keeps the first minimum of a map ordered by address (:406)
        mn = int(g.mn_id[s])
        key = (median, -mn if mutant == "ties_highest_id" else mn, j)
        if best is None or key < best[0]:
            best = (key, s, rg.obs_idx[p][j], median)
    return best[1], best[2], best[3]


def refresh_point(rg, p, what, mutant=None):
    """one entry -> dict(status, min_distance, max_distance, best_slot, best_index, best_median); writes rg's map records"""
    assert mutant is None or mutant in MUTANTS
    g = rg.g
    out = dict(status=0, min_distance=f32(0), max_distance=f32(0), best_slot=-1, best_index=-1, best_median=-1)
    if not (0 <= p < g.capacity):
        return out
    if g.point_bad[p] and mutant != "bad_point_refreshed":               # :352, :448
        return out
    if len(g.obs[p]) == 0:                                               # :357, :455
        return out
    chosen = distinctive(rg, p, mutant) if (what & DESCRIPTOR) or mutant == "level_from_winner" else None
    if what & DEPTH:
        r = int(rg.ref[p])
        if r in g.obs[p]:
            idx = rg.obs_idx[p][g.obs[p].index(r)]
        elif mutant == "ref_not_observer_nothing":
            idx = -1
        else:
            idx = 0                                                      # observations[pRefKF] default-constructs (0, 0) (:461)
        lr, li = r, idx
        if mutant == "level_from_winner" and chosen is not None:
            lr, li = chosen[0], chosen[1]
        # undefined in the reference, nothing written here: r outside the graph, an index of -1, an index beyond r's features
        if 0 <= r < g.kf_capacity and _feature(rg, r, idx) and _feature(rg, lr, li):
            level = int(rg.octave[lr][li])
            dist = point_distance(rg.pos[p], rg.centre[r])               # r is not tested for bad
            mx = f32(dist * rg.sf[level])                                # :471
            mn = f32(mx / (rg.sf[level] if mutant == "min_by_level_scale" else rg.sf[rg.n_levels - 1]))   # :472
            rg.min_distance[p], rg.max_distance[p] = mn, mx
            out.update(min_distance=mn, max_distance=mx)
            out["status"] |= DEPTH
    if (what & DESCRIPTOR) and chosen is not None:
        s, i, median = chosen
        src = i if i != -1 else len(rg.desc[s]) - 1
        rg.map_desc[p] = rg.desc[s][src]                                 # :415
        out.update(best_slot=s, best_index=i, best_median=median)
        out["status"] |= DESCRIPTOR
    return out


OUT_DTYPES = dict(status=np.int32, min_distance=f32, max_distance=f32, best_slot=np.int32, best_index=np.int32, best_median=np.int32)


def refresh_points(rg, ids, what, select=None, select_value=0, mutant=None):
    """the call: entry e is processed when select is None or select[e] == select_value -> dict of arrays, one element per entry"""
    assert what in (1, 2, 3)
    outs = []
    for e, p in enumerate(ids):
        if select is not None and int(select[e]) != select_value:
            outs.append(refresh_point(rg, -1, what))
        else:
            outs.append(refresh_point(rg, int(p), what, mutant))
    return {k: np.array([o[k] for o in outs], dt) for k, dt in OUT_DTYPES.items()}


def brute_force_descriptor(descs, mn_ids):
    """the reference's own form on N gathered descriptors: fill the matrix, sort every row, take vDists[0.5 * (N - 1)], keep the least
    (median, mn_id, position) -> (position, median)"""
    N = len(descs)
    best = None
    for i in range(N):
        row = sorted(sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(descs[i], descs[j])) for j in range(N))
        median = row[int(0.5 * (N - 1))]
        key = (median, int(mn_ids[i]), i)
        if best is None or key < best:
            best = key
    return best[2], best[0]


def new_graph(kf_capacity, capacity):
    g = R.Graph(kf_capacity, capacity)
    g.point_bad[:] = False
    return g

"""Tracking::UpdateLocalMap (src/Tracking.cc:1119-1324) restated on flat arrays: SPEC DECISION S24, normative for
orbfe_update_local_map_batch_device / orbfe_update_local_map and for the host restatement of tests/cpp/local_map.cpp.  Written from the
reference's lines, which the comments cite; where the reference leaves the result open S24 pins it and the comment says so.

The graph is what orbfe_covis holds: key-frame SLOTS stand for the key frames (mn_id differs between slots), point ids are those of the
resident map.  MUTANTS are deliberate mis-readings of one rule each; tests/test_local_map.py proves that every planted scene tells its
mutant from the rule, so that the exact comparison of the GPU outputs says something about that rule."""
import numpy as np

NO_POINT = 0x7fffffff
LOCAL_KF_MAX = 288
MAX_COVISIBLE = 16
MUTANTS = ("ties_descending_id", "parent_continue", "temporal_advance", "forward_kf_order", "last_occurrence", "bad_kf_keeps_place_off")


class Graph:
    """The tables of orbfe_covis plus the `bad` field of the map's points.  A key-frame slot that was never set is a bad key frame with
    mn_id == slot and nothing attached; a point that was never set is bad (orbfe_map_create) and observed by nobody."""

    def __init__(self, kf_capacity, capacity):
        self.kf_capacity, self.capacity = int(kf_capacity), int(capacity)
        self.mn_id = np.arange(kf_capacity, dtype=np.int64)
        self.kf_bad = np.ones(kf_capacity, bool)
        self.is_set = np.zeros(kf_capacity, bool)
        self.parent = np.full(kf_capacity, -1, np.int64)
        self.prev = np.full(kf_capacity, -1, np.int64)
        self.points = [np.empty(0, np.int32) for _ in range(kf_capacity)]     # GetMapPointMatches(): id per feature slot, < 0 = none
        self.covisible = [[] for _ in range(kf_capacity)]                     # the head of mvpOrderedConnectedKeyFrames (<= 16)
        self.children = [[] for _ in range(kf_capacity)]                      # S24: in the caller's order
        self.point_bad = np.ones(capacity, bool)
        self.obs = [[] for _ in range(capacity)]                              # GetObservations(): key-frame slots

    def set_keyframe(self, slot, mn_id, bad=False, parent=-1, prev=-1, points=None, covisible=(), children=()):
        self.mn_id[slot], self.kf_bad[slot], self.parent[slot], self.prev[slot] = mn_id, bool(bad), parent, prev
        self.is_set[slot] = True
        if points is not None:
            self.points[slot] = np.asarray(points, np.int32).copy()
        self.covisible[slot], self.children[slot] = list(covisible), list(children)

    def record(self, slot, with_points=True):
        """the arguments of set_keyframe as the dict orbfe.Covisibility.set_keyframes takes"""
        return dict(slot=slot, mn_id=int(self.mn_id[slot]), bad=int(self.kf_bad[slot]), parent=int(self.parent[slot]), prev=int(self.prev[slot]),
                    point_ids=self.points[slot] if with_points else None, covisible=self.covisible[slot], children=self.children[slot])

    def observations_csr(self, ids):
        off = np.zeros(len(ids) + 1, np.int32)
        off[1:] = np.cumsum([len(self.obs[int(p)]) for p in ids])
        flat = [s for p in ids for s in self.obs[int(p)]]
        return np.asarray(ids, np.int32), off, np.asarray(flat, np.int32)


def update_local_map(g, vote_ids, last_kf, M, max_local_kf=10, n_covisible=5, n_temporal=10, inertial=1, mark_voters_seen=0, mutant=None):
    """-> dict(ids [M], n_local_points, local_kfs [LOCAL_KF_MAX], n_local_kfs, vote_ids [n])"""
    assert mutant is None or mutant in MUTANTS
    vote_ids = np.asarray(vote_ids, np.int64)
    in_map = lambda p: 0 <= p < g.capacity   # noqa: E731
    in_kfs = lambda s: 0 <= s < g.kf_capacity   # noqa: E731

    # 1. votes (:1164-1211): a bad point casts none and is cleared (:1181, :1207); a point at two keypoints votes twice
    counter, voted, votes_out = {}, set(), vote_ids.copy()
    for i, p in enumerate(vote_ids):
        if not in_map(p):
            continue
        if g.point_bad[p]:
            votes_out[i] = -1
            continue
        voted.add(int(p))
        for s in g.obs[p]:
            counter[s] = counter.get(s, 0) + 1

    # 2. ranking (:1213-1224): vPairs in ascending mnId (the std::map), then std::sort by count descending.  std::sort leaves equal
    #    counts in no particular order; S24 pins a STABLE sort: equal counts stay in ascending mn_id
    id_sign = -1 if mutant == "ties_descending_id" else 1
    pairs = sorted(counter.items(), key=lambda kv: (-kv[1], id_sign * int(g.mn_id[kv[0]]), kv[0]))

    # 3. first phase (:1226-1243): the first nKFs entries; a bad one is skipped but has used its place
    nkfs = min(max_local_kf, len(pairs))
    local, listed = [], set()

    def append(s):
        local.append(int(s))
        listed.add(int(s))
    if mutant == "bad_kf_keeps_place_off":
        for s, _ in [kv for kv in pairs if not g.kf_bad[kv[0]]][:nkfs]:
            append(s)
    else:
        for s, _ in pairs[:nkfs]:
            if not g.kf_bad[s]:
                append(s)

    # 4. expansion (:1246-1295) over the key frames of the first phase only (S24: by index, the reference iterates the vector it grows)
    for s in list(local):
        # (a) GetBestCovisibilityKeyFrames(N) (KeyFrame.cc:245-253): the first min(size, N) of the ordered list, bad ones included
        for c in g.covisible[s][:min(n_covisible, MAX_COVISIBLE)]:
            if in_kfs(c) and not g.kf_bad[c] and c not in listed:
                append(c)
                break
        # (b) GetChilds() is a std::set ordered by address; S24: the caller's order
        for c in g.children[s]:
            if in_kfs(c) and not g.kf_bad[c] and c not in listed:
                append(c)
                break
        # (c) the parent: no bad test, and the break of :1292 leaves the OUTER loop
        par = int(g.parent[s])
        if in_kfs(par) and par not in listed:
            append(par)
            if mutant != "parent_continue":
                break

    # 5. temporal key frames (:1298-1314): a key frame that is already listed is not stepped over -- t does not advance (as written)
    if inertial:
        t = int(last_kf)
        for _ in range(n_temporal):
            if not in_kfs(t):
                break
            if t not in listed:
                append(t)
                t = int(g.prev[t])
            elif mutant == "temporal_advance":
                t = int(g.prev[t])
    assert len(local) <= LOCAL_KF_MAX

    # 6. points (:1135-1153): the list in REVERSE, feature slots ascending, first occurrence of a point that is not bad
    walk = [int(p) for s in (local if mutant == "forward_kf_order" else local[::-1]) for p in g.points[s]]
    if mutant == "last_occurrence":
        walk = walk[::-1]
    seen, out = set(), []
    for p in walk:
        if in_map(p) and p not in seen and not g.point_bad[p]:
            seen.add(p)
            out.append(~p if (mark_voters_seen and p in voted) else p)   # :1040-1056: the frame's own points are already matched
    if mutant == "last_occurrence":
        out = out[::-1]

    # 7. the output row
    ids = np.full(M, NO_POINT, np.int32)
    ids[:min(len(out), M)] = out[:M]
    kfs = np.full(LOCAL_KF_MAX, -1, np.int32)
    kfs[:len(local)] = local
    return dict(ids=ids, n_local_points=len(out), local_kfs=kfs, n_local_kfs=len(local), vote_ids=votes_out.astype(np.int32))


def frame_points(ids, match, outlier, n, observations, capacity):
    """orbfe_frame_points_batch_device for one frame (src/Tracking.cc:504-533): match / outlier over kp_stride keypoints -> ids or -1"""
    out = np.full(len(match), -1, np.int32)
    for i in range(min(int(n), len(match))):
        m = int(match[i])
        if 0 <= m < len(ids) and not outlier[i]:
            p = int(ids[m])
            if 0 <= p < capacity and observations[p] >= 1:
                out[i] = p
    return out

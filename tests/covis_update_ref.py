"""KeyFrame::UpdateConnections (src/KeyFrame.cc:459-553) with AddConnection (:191-204) and UpdateBestCovisibles (:206-228), and the graph
part of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:338-361), restated on the flat tables of orbfe_covis: SPEC DECISION S25
(DESIGN.md section 2), normative for orbfe_covis_add_keyframe_device, orbfe_covis_update_connections_device / _update_connections and
for the host restatement of tests/cpp/covis_update.cpp.  Written from the reference's lines, which the comments cite; where the
reference leaves the result open (the iteration order of a std::map keyed by pointer) S25 pins it and the comment says so.

ConnGraph holds the Graph of tests/local_map_ref.py (the tables UpdateLocalMap reads) and adds what S25 keeps per key frame: the full
mConnectedKeyFrameWeights.  MUTANTS are deliberate mis-readings of one rule each; tests/test_covis_update.py proves that every planted
scene tells its mutant from the rule."""
import numpy as np

import local_map_ref as R

MIN_WEIGHT = 50            # `th` of KeyFrame.cc:500 in this fork (upstream: 15)
MAX_COVISIBLE = R.MAX_COVISIBLE
MUTANTS = ("threshold_strict", "own_row_connected_only", "equal_weight_resorts", "ties_ascending_id", "max_first_highest_id",
           "bad_observer_counted", "parent_every_time", "duplicate_slot_adds_twice")
OK, NO_COUNTS, REFUSED = 0, 1, 2


class ConnGraph:
    """R.Graph by composition, its strides (the capacities of the resident rows) and the connection rows: conn[slot] maps a connected
    key-frame slot to its weight.  The order of a row is not observable."""

    def __init__(self, g, kf_stride, obs_stride, child_stride, conn_stride):
        self.g = g
        self.kf_stride, self.obs_stride, self.child_stride, self.conn_stride = int(kf_stride), int(obs_stride), int(child_stride), int(conn_stride)
        self.conn = [dict() for _ in range(g.kf_capacity)]

    def keyframe(self, slot):
        """what orbfe_covis_get_keyframe reads back"""
        g = self.g
        return dict(mn_id=int(g.mn_id[slot]), bad=int(g.kf_bad[slot]), parent=int(g.parent[slot]), prev=int(g.prev[slot]),
                    n_features=len(g.points[slot]), covisible=[int(c) for c in g.covisible[slot]], children=[int(c) for c in g.children[slot]],
                    conn=dict(self.conn[slot]))

    def connections_csr(self, slots):
        off = np.zeros(len(slots) + 1, np.int32)
        off[1:] = np.cumsum([len(self.conn[int(s)]) for s in slots])
        flat = [kv for s in slots for kv in sorted(self.conn[int(s)].items())]
        return (np.asarray(slots, np.int32), off, np.asarray([k for k, _ in flat], np.int32), np.asarray([w for _, w in flat], np.int32))


def _order(g, pairs, mutant=None):
    """sort ascending on (weight, pointer) followed by push_front (:528-535, :214-224): weight descending.  S25 lets mn_id stand for the
    pointer: equal weights in DESCENDING mn_id, then descending slot."""
    sign = 1 if mutant == "ties_ascending_id" else -1
    return sorted(pairs, key=lambda sw: (-sw[1], sign * int(g.mn_id[sw[0]]), sign * sw[0]))


def _best_covisibles(cg, q, mutant=None):
    """UpdateBestCovisibles (:206-228): every entry of the row whose key frame is not bad now, ordered; the resident head is its first 16"""
    g = cg.g
    ordered = _order(g, [(s, w) for s, w in cg.conn[q].items() if not g.kf_bad[s]], mutant)
    g.covisible[q] = [s for s, _ in ordered[:MAX_COVISIBLE]]


def add_keyframe(cg, slot, mn_id, point_ids, bad=False, parent=-1, prev=-1, mutant=None):
    """orbfe_covis_add_keyframe_device: the key frame's row and point list, then LocalMapping.cc:340-359 -> (added [n], status)"""
    assert mutant is None or mutant in MUTANTS
    g = cg.g
    ids = np.asarray(point_ids, np.int64)
    assert len(ids) <= cg.kf_stride
    added = np.zeros(len(ids), np.int32)
    appends, seen = [], set()
    for i, p in enumerate(ids):
        if not (0 <= p < g.capacity) or g.point_bad[p]:
            continue
        p = int(p)
        first = p not in seen or mutant == "duplicate_slot_adds_twice"
        seen.add(p)
        if first and slot not in g.obs[p]:                  # IsInKeyFrame (:347)
            appends.append(p)
            added[i] = 1
        else:                                               # :353-356, and the second feature slot of the same point
            added[i] = 2
    grow = {}
    for p in appends:
        grow[p] = grow.get(p, 0) + 1
    if any(len(g.obs[p]) + k > cg.obs_stride for p, k in grow.items()):   # decided before anything is written
        return np.zeros(len(ids), np.int32), REFUSED
    g.set_keyframe(slot, mn_id, bad=bad, parent=parent, prev=prev, points=ids.astype(np.int32), covisible=(), children=())
    cg.conn[slot] = dict()
    for p in appends:
        g.obs[p].append(int(slot))
    return added, OK


def update_connections(cg, s, flag=0, min_weight=MIN_WEIGHT, mutant=None):
    """one key frame of orbfe_covis_update_connections_device -> dict(slots [conn_stride], weights [conn_stride], count, status)"""
    assert mutant is None or mutant in MUTANTS
    g = cg.g
    out = dict(slots=np.full(cg.conn_stride, -1, np.int32), weights=np.zeros(cg.conn_stride, np.int32), count=0, status=OK)

    # counting (:471-490): a point at two feature slots counts twice; one graph is one map
    counter = {}
    for p in g.points[s]:
        p = int(p)
        if not (0 <= p < g.capacity) or g.point_bad[p]:
            continue
        for o in g.obs[p]:
            if o == s or not (0 <= o < g.kf_capacity):
                continue
            if g.kf_bad[o] and mutant != "bad_observer_counted":
                continue
            counter[o] = counter.get(o, 0) + 1
    if not counter:                                          # :493
        out["status"] = NO_COUNTS
        return out

    # selection (:498-526).  KFcounter iterates in pointer order; S25: in ascending mn_id, so `>` keeps the lowest mn_id among maxima
    walk = sorted(counter.items(), key=lambda kv: (int(g.mn_id[kv[0]]), kv[0]))
    if mutant == "max_first_highest_id":
        walk = walk[::-1]
    nmax, kfmax = 0, -1
    for o, c in walk:
        if c > nmax:
            nmax, kfmax = c, o
    over = (lambda c: c > min_weight) if mutant == "threshold_strict" else (lambda c: c >= min_weight)
    connected = [(o, c) for o, c in walk if over(c)]
    if not connected:
        connected = [(kfmax, nmax)]
    ordered = _order(g, connected, mutant)
    own_row = dict(connected) if mutant == "own_row_connected_only" else dict(counter)
    set_parent = (flag & 1) or mutant == "parent_every_time"
    par = ordered[0][0]

    # capacity, decided before anything of this key frame is written
    refused = len(counter) > cg.conn_stride
    refused = refused or any(s not in cg.conn[q] and len(cg.conn[q]) >= cg.conn_stride for q, _ in connected)
    refused = refused or (set_parent and s not in g.children[par] and len(g.children[par]) >= cg.child_stride)
    if refused:
        out["status"] = REFUSED
        return out

    # the reciprocal AddConnection (:518, :525, :191-204): an equal weight changes nothing at all
    for q, w in connected:
        if cg.conn[q].get(s) == w and mutant != "equal_weight_resorts":
            continue
        cg.conn[q][s] = w
        _best_covisibles(cg, q, mutant)

    # own lists (:528-543): the row is the whole counter, the ordered list the connected ones; no bad test (bad observers did not count)
    cg.conn[s] = own_row
    g.covisible[s] = [q for q, _ in ordered[:MAX_COVISIBLE]]
    if set_parent:                                           # :545-550; S24: children in the caller's order -- appended
        g.parent[s] = par
        if s not in g.children[par]:
            g.children[par].append(int(s))
    n = len(ordered)
    out["slots"][:n] = [q for q, _ in ordered]
    out["weights"][:n] = [w for _, w in ordered]
    out["count"] = n
    return out

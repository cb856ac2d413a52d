"""Graphs and operations for the S25 tests (tests/covis_update_ref.py): one hand-written scene per rule with what it must give and the
mutants it tells apart, and the shapes at which the kernels change path (the vote table's switch count, heads around 16, rows around
their strides).  A scene is a ConnGraph in its initial state plus a list of operations; trace() plays them on the restatement, the GPU
test plays them on the resident graph.  No orbfe import."""
import copy

import numpy as np

import covis_update_ref as U
import local_map_ref as R


class Builder:
    """key frames that share freshly numbered points: share([a, b], n) gives a and b n common points, observed by both"""

    def __init__(self, n_kf, capacity, kf_stride=None, obs_stride=None, child_stride=4, conn_stride=8):
        self.g = R.Graph(n_kf, capacity)
        self.g.point_bad[:] = False
        self.pts = [[] for _ in range(n_kf)]
        self.next = 0
        self.strides = dict(kf_stride=kf_stride, obs_stride=obs_stride, child_stride=child_stride, conn_stride=conn_stride)

    def kf(self, slot, mn_id, **kw):
        self.g.set_keyframe(slot, mn_id, points=[], **kw)
        return self

    def share(self, kfs, n, observed_by=None):
        """n new points held by every key frame of kfs; observed_by (default: kfs) are the ones the points' lists name"""
        for _ in range(n):
            p, self.next = self.next, self.next + 1
            assert p < self.g.capacity
            for s in kfs:
                self.pts[s].append(p)
            self.g.obs[p] = list(kfs if observed_by is None else observed_by)
        return self

    def done(self):
        g = self.g
        for s in range(g.kf_capacity):
            if g.is_set[s]:
                g.points[s] = np.asarray(self.pts[s], np.int32)
        st = dict(self.strides)
        st["kf_stride"] = st["kf_stride"] or max(1, max(len(p) for p in self.pts)) + 3
        st["obs_stride"] = st["obs_stride"] or max(1, max(len(o) for o in g.obs)) + 1
        return U.ConnGraph(g, **st)


class Scene:
    """ops: ("add", dict(slot, mn_id, point_ids, bad, parent, prev)) | ("update", dict(slots, flags, min_weight))"""

    def __init__(self, cg, ops, kills=(), expect=None):
        self.cg, self.ops, self.kills, self.expect = cg, ops, tuple(kills), expect

    def trace(self, mutant=None):
        """-> (outputs of every operation, the final graph): everything S25 can write"""
        cg = copy.deepcopy(self.cg)
        outs = []
        for kind, a in self.ops:
            if kind == "add":
                added, status = U.add_keyframe(cg, a["slot"], a["mn_id"], a["point_ids"], bad=a.get("bad", False), parent=a.get("parent", -1),
                                               prev=a.get("prev", -1), mutant=mutant)
                outs.append(dict(added=added, status=status))
            else:
                for s, f in zip(a["slots"], a["flags"]):
                    outs.append(U.update_connections(cg, s, f, a.get("min_weight", U.MIN_WEIGHT), mutant=mutant))
        return outs, cg


def state(cg):
    """the whole observable graph as plain data"""
    g = cg.g
    return dict(kfs=[cg.keyframe(s) for s in range(g.kf_capacity)], obs=[list(map(int, o)) for o in g.obs])


def same_outputs(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.keys() != y.keys() or any(not np.array_equal(x[k], y[k]) for k in x):
            return False
    return True


def update(slots, flags=None, min_weight=U.MIN_WEIGHT):
    slots = [slots] if np.isscalar(slots) else list(slots)
    return ("update", dict(slots=slots, flags=list(flags) if flags is not None else [0] * len(slots), min_weight=min_weight))


def add(slot, mn_id, point_ids, **kw):
    return ("add", dict(slot=slot, mn_id=mn_id, point_ids=np.asarray(point_ids, np.int32), **kw))


def planted_scenes():
    """name -> Scene; `expect` is worked out by hand in the comments and checked by tests/test_covis_update.py"""
    out = {}

    # counts of min_weight - 1, min_weight, min_weight + 1 at the default 50: 2 and 3 are connected, the row holds all three
    b = Builder(4, 256)
    for s in range(4):
        b.kf(s, 10 + s)
    b.share([0, 1], 49).share([0, 2], 50).share([0, 3], 51)
    out["threshold"] = Scene(b.done(), [update(0)], ("threshold_strict",),
                             expect=dict(ordered=[(3, 51), (2, 50)], row={1: 49, 2: 50, 3: 51}, head={0: [3, 2], 2: [0], 3: [0], 1: []}))

    # A = 0 counts {B = 1: 60, C = 2: 10}: connected to B alone, but its row keeps C (:540).  Then D = 3 arrives with 55 points of A:
    # AddConnection(A, D, 55) re-sorts A's whole row: B, D, C -- C, which A never connected to, is now in A's head
    b = Builder(4, 256, obs_stride=4)
    for s in range(3):
        b.kf(s, s)
    b.share([0, 1], 60).share([0, 2], 10)
    first_d = b.next
    b.share([0], 55)                                    # the points D will hold too
    cg = b.done()
    out["row_keeps_unconnected"] = Scene(cg, [update(0), add(3, 3, np.arange(first_d, first_d + 55)), update(3)], ("own_row_connected_only",),
                                         expect=dict(head={0: [1, 3, 2], 3: [0]}, row0={1: 60, 2: 10, 3: 55}))

    # q = 1 has the row {X = 2: 70, s = 0: 60} and the head [X, s]; X has gone bad since.  s counts q at 60 again: nothing happens to q
    b = Builder(3, 256)
    b.kf(0, 0).kf(1, 1, covisible=[2, 0]).kf(2, 2, bad=True)
    b.share([0, 1], 60)
    cg = b.done()
    cg.conn[1] = {2: 70, 0: 60}
    out["equal_weight_is_left_alone"] = Scene(cg, [update(0)], ("equal_weight_resorts",), expect=dict(head={1: [2, 0], 0: [1]}))

    # equal weights: descending mn_id.  mn_id runs against the slot, so descending slot would give the other order
    b = Builder(4, 256)
    b.kf(0, 50).kf(1, 9).kf(2, 5).kf(3, 7)
    b.share([0, 1], 50).share([0, 2], 50).share([0, 3], 50)
    out["ties"] = Scene(b.done(), [update(0)], ("ties_ascending_id",), expect=dict(ordered=[(1, 50), (3, 50), (2, 50)]))

    # nothing reaches the threshold: the largest count, and among the two maxima the LOWEST mn_id (slot 2)
    b = Builder(4, 64)
    b.kf(0, 50).kf(1, 7).kf(2, 4).kf(3, 1)
    b.share([0, 1], 3).share([0, 2], 3).share([0, 3], 2)
    out["maximum_fallback"] = Scene(b.done(), [update(0)], ("max_first_highest_id",),
                                    expect=dict(ordered=[(2, 3)], row={1: 3, 2: 3, 3: 2}, head={0: [2], 2: [0], 1: [], 3: []}))

    # a bad observer is not counted: 60 points with the bad key frame 1, 55 with key frame 2
    b = Builder(3, 256)
    b.kf(0, 0).kf(1, 1, bad=True).kf(2, 2)
    b.share([0, 1], 60).share([0, 2], 55)
    out["bad_observer"] = Scene(b.done(), [update(0)], ("bad_observer_counted",), expect=dict(ordered=[(2, 55)], row={2: 55}))

    # the parent is set with flags & 1 only: a later UpdateConnections of key frame 2, whose parent is 1, leaves it there although
    # key frame 0 is now the front of its list
    b = Builder(3, 256)
    b.kf(0, 0).kf(1, 1, children=[2]).kf(2, 2, parent=1)
    b.share([2, 0], 60).share([2, 1], 55)
    out["parent_on_first_connection_only"] = Scene(b.done(), [update(2, [0])], ("parent_every_time",),
                                                   expect=dict(ordered=[(0, 60), (1, 55)], parent=1, children={0: [], 1: [2]}))

    # the observation append: point 5 at two feature slots (the lowest adds, the other reads "already in"), an empty slot, a bad
    # point, an id outside the map, and point 7 that names the key frame already (:353-356)
    b = Builder(3, 16, kf_stride=8, obs_stride=3)
    b.kf(0, 0).kf(1, 1)
    b.share([0], 8)
    cg = b.done()
    cg.g.point_bad[6] = True
    cg.g.obs[7] = [0, 2]
    out["observation_append"] = Scene(cg, [add(2, 2, [5, 5, 3, -1, 6, 99, 7])], ("duplicate_slot_adds_twice",),
                                      expect=dict(added=[1, 2, 1, 0, 0, 0, 2], obs={5: [0, 2], 3: [0, 2], 7: [0, 2], 6: [0]}))
    return out


def reciprocal_scene(case):
    """the three-way rule of AddConnection for one neighbour, or all three in one call: s = 0 connects to 1 (absent from its row), 2
    (present with the same weight; its head is stale: it lists the bad key frame 4) and 3 (present with another weight; the bad key
    frame 4 leaves its head)"""
    b = Builder(5, 64, conn_stride=4)
    for s in range(5):
        b.kf(s, 20 - s, bad=s == 4)
    which = dict(absent=[1], equal=[2], different=[3], mixed=[1, 2, 3])[case]
    for q in which:
        b.share([0, q], 3 + q)
    cg = b.done()
    cg.conn[2], cg.g.covisible[2] = {4: 9, 0: 5}, [4, 0]
    cg.conn[3], cg.g.covisible[3] = {4: 9, 0: 2, 1: 2}, [4, 0, 1]
    return Scene(cg, [update(0, min_weight=3)])


def head_scene(n_good, n_bad=3):
    """a neighbour q = 1 whose row holds n_good - 1 key frames that are not bad and n_bad bad ones, with equal weights in pairs; s = 0
    arrives as the n_good-th: the head is the best 16 that are not bad"""
    n = 2 + n_good - 1 + n_bad
    b = Builder(n, 64, conn_stride=n_good + n_bad + 1)
    rng = np.random.default_rng(n_good)
    mn = rng.permutation(n) + 100
    for s in range(n):
        b.kf(s, int(mn[s]), bad=s >= 2 + n_good - 1)
    b.share([0, 1], 4)
    cg = b.done()
    cg.conn[1] = {s: 2 + (s // 2) % 5 for s in range(2, n)}
    return Scene(cg, [update(0, min_weight=3)])


def observers_scene(n_obs, th=3):
    """s = 0 shares points with n_obs distinct key frames (the vote table's switch count is 512): key frame k gets 1 + k % 4 common
    points, so some reach th and there are many equal weights; mn_id is a permutation"""
    n = n_obs + 1
    b = Builder(n, 4 * n + 8, child_stride=2, conn_stride=n_obs)
    rng = np.random.default_rng(n_obs)
    mn = rng.permutation(n)
    for s in range(n):
        b.kf(s, int(mn[s]))
    for k in range(1, n):
        b.share([0, k], 1 + k % 4)
    return Scene(b.done(), [update(0, [1], min_weight=th)])


def double_slot_scene():
    """point 0 sits at two feature slots of s = 0: it counts twice (2 + 1 = 3 reaches min_weight 3, 2 would not)"""
    b = Builder(2, 16)
    b.kf(0, 0).kf(1, 1)
    b.share([0, 1], 2)
    cg = b.done()
    cg.g.points[0] = np.array([0, 1, 0, -1, 99], np.int32)
    cg.kf_stride = 8
    return Scene(cg, [update(0, min_weight=3)])


def invalid_scene():
    """bad points, ids outside the map, bad observers, an observer slot outside the graph cannot occur (the setters refuse it)"""
    b = Builder(4, 64)
    b.kf(0, 0).kf(1, 1).kf(2, 2, bad=True).kf(3, 3)
    b.share([0, 1], 5).share([0, 2], 6).share([0, 3], 4)
    cg = b.done()
    cg.g.point_bad[[0, 1, 11]] = True
    cg.g.points[0] = np.concatenate([cg.g.points[0], np.array([-1, 64, 1000, -5], np.int32)])
    cg.kf_stride = len(cg.g.points[0]) + 1
    return Scene(cg, [update(0, min_weight=3)])


def no_counts_scene():
    b = Builder(3, 16)
    b.kf(0, 0).kf(1, 1, bad=True).kf(2, 2)
    b.share([0, 1], 3).share([2], 3)
    cg = b.done()
    cg.g.points[0] = np.concatenate([cg.g.points[0], np.array([-1, 99], np.int32)])
    cg.kf_stride = 8
    return Scene(cg, [update(0, [1], min_weight=3)])


def capacity_scene(what, delta=0):
    """the four refusals, and the last shape that still fits.
    conn_stride: conn_stride + delta distinct counted key frames; neighbour_row: the neighbour's row is full (delta = 0) or has one
    place (delta = -1), or is full but holds s already (delta = 1); children: the parent's children row full / one place / holds s"""
    if what == "conn_stride":
        S = 6
        b = Builder(S + 3, 64, conn_stride=S)
        for s in range(S + 3):
            b.kf(s, s)
        for k in range(1, S + delta + 1):
            b.share([0, k], 3)
        return Scene(b.done(), [update(0, [1], min_weight=3)])
    S = 3
    b = Builder(6, 64, conn_stride=S, child_stride=2)
    for s in range(6):
        b.kf(s, s)
    b.share([0, 1], 4).share([0, 2], 3)
    cg = b.done()
    if what == "neighbour_row":
        cg.conn[2] = {3: 1, 4: 1, 5: 1} if delta == 0 else ({3: 1, 4: 1} if delta < 0 else {3: 1, 4: 1, 0: 1})
    else:
        cg.g.children[1] = [3, 4] if delta == 0 else ([3] if delta < 0 else [3, 0])
    return Scene(cg, [update(0, [1], min_weight=3)])


def full_observation_list_scene(delta=0):
    """add_keyframe where one point's observation list is full (delta = 0: refused, nothing written), has one place (-1), or is full but
    names the key frame already (1)"""
    b = Builder(4, 16, kf_stride=6, obs_stride=2)
    b.kf(0, 0).kf(1, 1)
    b.share([0], 6)
    cg = b.done()
    cg.g.obs[4] = [0, 1] if delta == 0 else ([0] if delta < 0 else [0, 3])
    return Scene(cg, [add(3, 3, [1, 2, 4, 4, 5])])


def sequence_scene():
    """three key frames in one call, each seeing what the one before wrote: 5 connects to 1 and 2; 6 then finds 5 in its counts and
    becomes a child of the same parent; 7 changes a weight that 5 set"""
    b = Builder(8, 256, conn_stride=6, child_stride=3)
    for s in range(8):
        b.kf(s, 30 + s)
    b.share([5, 1], 5).share([5, 2], 4).share([6, 5], 6).share([6, 1], 5).share([7, 5], 3).share([7, 2], 4).share([7, 6], 3)
    return Scene(b.done(), [update([5, 6, 7], [1, 1, 1], min_weight=3)])


def initialisation_scene():
    """Tracking.cc:690-691: the initial key frame and the current one share every point; neither has mbFirstConnection && id != init for
    the first, the second does"""
    b = Builder(2, 128)
    b.kf(0, 0).kf(1, 1)
    b.share([0, 1], 100)
    return Scene(b.done(), [update([0, 1], [0, 1])])


def gpu_scenes():
    out = dict(planted_scenes())
    for case in ("absent", "equal", "different", "mixed"):
        out["reciprocal_" + case] = reciprocal_scene(case)
    for n in (15, 16, 17):
        out["head_%d" % n] = head_scene(n)
    out.update(double_slot=double_slot_scene(), invalid=invalid_scene(), no_counts=no_counts_scene(), sequence=sequence_scene(),
               initialisation=initialisation_scene(), observers_1=observers_scene(1))
    for what in ("conn_stride", "neighbour_row", "children"):
        for d in (-1, 0, 1):
            out["capacity_%s_%+d" % (what, d)] = capacity_scene(what, d)
    for d in (-1, 0, 1):
        out["observation_list_%+d" % d] = full_observation_list_scene(d)
    return out


def upload(orbfe, ex, cg):
    """-> (MapPoints, Covisibility) holding the graph, connection rows included"""
    g = cg.g
    mp = orbfe.MapPoints(ex, g.capacity)
    pts = np.zeros(g.capacity, orbfe.WP_DTYPE)
    pts["bad"] = g.point_bad
    pts["observations"] = [len(o) for o in g.obs]
    mp.update(np.arange(g.capacity), pts, np.zeros((g.capacity, 32), np.uint8))
    cv = orbfe.Covisibility(ex, mp, g.kf_capacity, cg.kf_stride, cg.obs_stride, cg.child_stride)
    cv.set_keyframes([g.record(s) for s in range(g.kf_capacity) if g.is_set[s]])
    cv.set_observations(*g.observations_csr([p for p in range(g.capacity) if g.obs[p]]))
    cv.enable_connections(cg.conn_stride)
    rows = [s for s in range(g.kf_capacity) if cg.conn[s]]
    if rows:
        cv.set_connections(*cg.connections_csr(rows))
    return mp, cv

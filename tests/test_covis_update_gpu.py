"""orbfe_covis_add_keyframe_device, orbfe_covis_update_connections_device / _update_connections, orbfe_covis_set_connections and
orbfe_covis_get_keyframe on the GPU (SPEC DECISION S25).  Every comparison is exact equality with tests/covis_update_ref.py: every
output row of every operation, and afterwards every key frame read back (scalars, head, children, connection row as a set of pairs --
the order of a row is not observable) and the observation lists as orbfe_update_local_map sees them.  The shapes are the smallest at
which each mechanism can go wrong (tests/covis_update_scenarios.py; tests/test_covis_update.py proves the scenes tell the rules from
their mutants): counts around min_weight, the maximum fallback with ties, the vote table's switch count, heads around 16, every row at
its stride and one either side, key frames that see what the one before them wrote."""
import copy

import numpy as np
import pytest

import covis_update_ref as U
import covis_update_scenarios as S
import local_map_ref as R
import local_map_scenarios as LS

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
POISON = -77
GUARD = 8


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


class Resident:
    """a ConnGraph in HBM and, beside it, the restatement's copy that the same operations are played on"""

    def __init__(self, ex, cg):
        import orbfe
        self.o, self.ex, self.cg = orbfe, ex, copy.deepcopy(cg)
        self.mp, self.cv = S.upload(orbfe, ex, cg)

    def close(self):
        self.cv.close()
        self.mp.close()

    def add(self, a, d_ids=None):
        """one add_keyframe_device on a stream of its own, outputs poisoned, GUARD words behind d_added -> dict(added, status)"""
        import torch
        ids = np.ascontiguousarray(a["point_ids"], np.int32)
        n = len(ids)
        d_ids = torch.from_numpy(ids if n else np.zeros(1, np.int32)).cuda() if d_ids is None else d_ids
        d_added = torch.full((n + GUARD,), POISON, dtype=torch.int32, device="cuda")
        d_status = torch.full((1 + GUARD,), POISON, dtype=torch.int32, device="cuda")
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        self.cv.add_keyframe_device(a["slot"], a["mn_id"], d_ids.data_ptr(), n, d_added.data_ptr(), d_status.data_ptr(), bad=int(a.get("bad", 0)),
                                    parent=a.get("parent", -1), prev=a.get("prev", -1), stream=st.cuda_stream)
        st.synchronize()
        added, status = d_added.cpu().numpy(), d_status.cpu().numpy()
        assert (added[n:] == POISON).all() and (status[1:] == POISON).all(), "guard words written"
        return dict(added=added[:n], status=int(status[0]))

    def update(self, a):
        """the key frames of one update op as ONE device call -> a dict per key frame"""
        import torch
        n, Sd = len(a["slots"]), self.cv.conn_stride
        full = lambda k: torch.full((k + GUARD,), POISON, dtype=torch.int32, device="cuda")   # noqa: E731
        d_s, d_w, d_n, d_st = full(n * Sd), full(n * Sd), full(n), full(n)
        io = self.o.CovisUpdateIO(d_slots=d_s.data_ptr(), d_weights=d_w.data_ptr(), d_count=d_n.data_ptr(), d_status=d_st.data_ptr())
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        self.cv.update_connections_device(a["slots"], a["flags"], io, self.o.CovisUpdateParams(a.get("min_weight", U.MIN_WEIGHT)), st.cuda_stream)
        st.synchronize()
        s_, w_, n_, st_ = (t.cpu().numpy() for t in (d_s, d_w, d_n, d_st))
        for arr, k in ((s_, n * Sd), (w_, n * Sd), (n_, n), (st_, n)):
            assert (arr[k:] == POISON).all(), "guard words behind the rows written"
        return [dict(slots=s_[k * Sd:(k + 1) * Sd], weights=w_[k * Sd:(k + 1) * Sd], count=int(n_[k]), status=int(st_[k])) for k in range(n)]

    def play(self, ops):
        """the operations on the device and on the restatement; every output compared"""
        for i, (kind, a) in enumerate(ops):
            if kind == "add":
                got = [self.add(a)]
                added, status = U.add_keyframe(self.cg, a["slot"], a["mn_id"], a["point_ids"], bad=a.get("bad", False), parent=a.get("parent", -1),
                                               prev=a.get("prev", -1))
                want = [dict(added=added, status=status)]
            else:
                got = self.update(a)
                want = [U.update_connections(self.cg, s, f, a.get("min_weight", U.MIN_WEIGHT)) for s, f in zip(a["slots"], a["flags"])]
            same_outputs(got, want, "operation %d (%s)" % (i, kind))

    def state(self):
        return [self.cv.get_keyframe(s) for s in range(self.cg.g.kf_capacity)]

    def check_state(self, what):
        """every key frame read back, and the observation lists through orbfe_update_local_map: every point with a list votes"""
        g = self.cg.g
        for s, got in enumerate(self.state()):
            assert got == self.cg.keyframe(s), "%s: key frame %d\n%r\n%r" % (what, s, got, self.cg.keyframe(s))
        voters = [p for p in range(g.capacity) if g.obs[p]] or [0]
        par = dict(max_local_kf=64, n_covisible=5, n_temporal=0, inertial=0, mark_voters_seen=0)
        got = self.o.update_local_map(self.ex, self.o.LocalMapParams(**par), voters, -1, self.cv, 64)
        want = R.update_local_map(g, voters, -1, 64, **par)
        for k in ("n_local_kfs", "n_local_points"):
            assert got[k] == want[k], "%s: %s" % (what, k)
        for k in ("local_kfs", "ids", "vote_ids"):
            assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)


def same_outputs(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        for name in a:
            assert np.array_equal(a[name], b[name]), "%s, key frame %d: %s\n%r\n%r" % (what, k, name, a[name], b[name])


@pytest.mark.parametrize("name", sorted(S.gpu_scenes()))
def test_scene_equals_the_restatement(ex, name):
    sc = S.gpu_scenes()[name]
    r = Resident(ex, sc.cg)
    try:
        before = r.state()
        r.check_state(name + ", as uploaded (orbfe_covis_set_connections)")
        r.play(sc.ops)
        r.check_state(name)
        outs, _ = sc.trace()
        if len(outs) == 1 and outs[0]["status"] != U.OK:                       # refused, or no counts: the graph as it was
            assert r.state() == before, name
    finally:
        r.close()


@pytest.mark.parametrize("n_obs", (512, 513))
def test_vote_table_and_counters_give_the_same(ex, n_obs):
    """the LDS table at its last key and the counters in HBM one past it; twice (the second call changes nothing: every weight is the
    same), and then orbfe_update_local_map on the same graph: the counters were put back"""
    import orbfe
    assert orbfe.LOCAL_MAP_VOTE_TABLE == 512
    sc = S.observers_scene(n_obs)
    r = Resident(ex, sc.cg)
    try:
        r.play(sc.ops)
        r.check_state("%d observers" % n_obs)
        first = r.state()
        r.play(sc.ops)
        assert r.state() == first
        r.check_state("%d observers, second call" % n_obs)
    finally:
        r.close()


def test_three_key_frames_in_one_call_equal_three_calls(ex):
    sc = S.sequence_scene()
    a = sc.ops[0][1]
    one, three = Resident(ex, sc.cg), Resident(ex, sc.cg)
    try:
        got = one.update(a)
        split = [three.update(dict(a, slots=[s], flags=[f]))[0] for s, f in zip(a["slots"], a["flags"])]
        same_outputs(got, split, "one call against three")
        same_outputs(got, sc.trace()[0], "one call against the restatement")
        assert one.state() == three.state()
        assert [o["status"] for o in got] == [0, 0, 0] and got[1]["count"] >= 2
    finally:
        one.close()
        three.close()


def test_host_form_equals_the_device_form(ex):
    import orbfe
    for name in ("threshold", "reciprocal_mixed", "maximum_fallback", "no_counts"):
        sc = S.gpu_scenes()[name]
        a = sc.ops[-1][1]
        dev, host = Resident(ex, sc.cg), Resident(ex, sc.cg)
        try:
            want = dev.update(a)[0]
            got = host.cv.update_connections(a["slots"][0], a["flags"][0], orbfe.CovisUpdateParams(a.get("min_weight", U.MIN_WEIGHT)))
            same_outputs([got], [want], name)
            assert host.state() == dev.state(), name
        finally:
            dev.close()
            host.close()
    sc = S.capacity_scene("neighbour_row", 0)                                   # refused: ORBFE_ERR_OUT_OF_MEMORY, the graph as it was
    r = Resident(ex, sc.cg)
    try:
        before = r.state()
        with pytest.raises(orbfe.OrbfeError) as e:
            r.cv.update_connections(0, 1, orbfe.CovisUpdateParams(3))
        assert "full" in str(e.value)
        assert r.state() == before
    finally:
        r.close()


def test_host_form_of_add_keyframe_equals_the_device_form(ex):
    import orbfe
    for name in ("observation_append", "observation_list_-1", "observation_list_+1"):
        sc = S.gpu_scenes()[name]
        a = sc.ops[0][1]
        dev, host = Resident(ex, sc.cg), Resident(ex, sc.cg)
        try:
            want = dev.add(a)
            got = host.cv.add_keyframe(a["slot"], a["mn_id"], a["point_ids"])
            same_outputs([got], [want], name)
            same_outputs([got], sc.trace()[0], name + " against the restatement")
            assert host.state() == dev.state(), name
            U.add_keyframe(host.cg, a["slot"], a["mn_id"], a["point_ids"])
            host.check_state(name + ", host form")
        finally:
            dev.close()
            host.close()
    sc = S.full_observation_list_scene(0)                                       # refused: ORBFE_ERR_OUT_OF_MEMORY, the graph as it was
    r = Resident(ex, sc.cg)
    try:
        a = sc.ops[0][1]
        with pytest.raises(orbfe.OrbfeError) as e:
            r.cv.add_keyframe(a["slot"], a["mn_id"], a["point_ids"])
        assert "full" in str(e.value)
        r.check_state("refused host add")
    finally:
        r.close()


def _insertion_order(sc):
    g = sc.g
    return sorted((s for s in range(g.kf_capacity) if g.is_set[s]), key=lambda s: int(g.mn_id[s]))


def test_graph_built_on_the_device_serves_update_local_map(ex):
    """the random graph of local_map_scenarios.py built key frame by key frame through add_keyframe_device + update_connections_device
    only; after every insertion orbfe_update_local_map on it equals the S24 restatement on the graph the S25 restatement built.  At the
    end one more key frame whose point row comes straight from orbfe_frame_points_batch_device."""
    import torch
    import orbfe
    sc = LS.random_scene()
    src, n_pts = sc.g, sc.g.capacity
    g = R.Graph(src.kf_capacity, n_pts)
    g.point_bad[:] = src.point_bad
    cg = U.ConnGraph(g, kf_stride=sc.kf_stride, obs_stride=16, child_stride=16, conn_stride=32)
    r = Resident(ex, cg)
    pts = np.zeros(n_pts, orbfe.WP_DTYPE)
    pts["bad"], pts["observations"] = src.point_bad, 1
    r.mp.update(np.arange(n_pts), pts, np.zeros((n_pts, 32), np.uint8))
    par = orbfe.LocalMapParams(**sc.params)
    try:
        connected = 0
        for k, s in enumerate(_insertion_order(sc)):
            r.play([S.add(s, int(src.mn_id[s]), src.points[s], bad=bool(src.kf_bad[s]), prev=int(src.prev[s])),
                    S.update(s, [1 if k else 0], min_weight=15)])
            connected += len(r.cg.conn[s])
            votes, last = sc.frames[k % len(sc.frames)]
            got = orbfe.update_local_map(ex, par, votes, last, r.cv, sc.M)
            want = R.update_local_map(r.cg.g, votes, last, sc.M, **sc.params)
            for key in ("n_local_kfs", "n_local_points"):
                assert got[key] == want[key], (k, key)
            for key in ("local_kfs", "ids", "vote_ids"):
                assert np.array_equal(got[key], want[key]), (k, key)
        r.check_state("after %d insertions" % (k + 1))
        assert connected > 200 and sum(len(c) for c in r.cg.g.children) > 40    # the scene exercises what it is for

        # the next key frame's point row from orbfe_frame_points_batch_device, handed over in HBM
        M, stride = 64, sc.kf_stride
        rng = np.random.default_rng(11)
        ids = rng.integers(5000, 5600, M).astype(np.int32)
        match = rng.integers(-1, M + 2, stride).astype(np.int32)
        outl = (rng.random(stride) < 0.1).astype(np.uint8)
        n = np.array([stride - 7], np.int32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()         # noqa: E731
        d_ids, d_match, d_outl, d_n = up(ids), up(match), up(outl), up(n)
        d_row = torch.full((stride,), POISON, dtype=torch.int32, device="cuda")
        orbfe.frame_points_batch_device(ex, r.mp, 1, stride, M, d_ids.data_ptr(), d_match.data_ptr(), d_outl.data_ptr(), d_n.data_ptr(),
                                        d_row.data_ptr())
        torch.cuda.synchronize()
        row = R.frame_points(ids, match, outl, n[0], pts["observations"], n_pts)
        assert (row >= 0).sum() > 100
        spare = next(s for s in range(g.kf_capacity) if not src.is_set[s])
        a = S.add(spare, 1000, row)[1]
        got = r.add(a, d_ids=d_row)
        added, status = U.add_keyframe(r.cg, spare, 1000, row)
        same_outputs([got], [dict(added=added, status=status)], "the row from frame_points")
        assert (added == 1).sum() > 50 and (added == 2).sum() > 0
        r.play([S.update(spare, [1], min_weight=15)])
        r.check_state("the key frame from frame_points")
    finally:
        r.close()


def test_refusals_with_a_handle(ex):
    """every refusal the header lists that needs a graph to be decided; each leaves the graph as it was"""
    import ctypes as C
    import orbfe
    sc = S.planted_scenes()["threshold"]
    g = sc.cg.g
    mp = orbfe.MapPoints(ex, g.capacity)
    cv = orbfe.Covisibility(ex, mp, g.kf_capacity, sc.cg.kf_stride, sc.cg.obs_stride, sc.cg.child_stride)
    L, INVALID = orbfe.lib(), 1
    arr = lambda *v: np.array(v, np.int32)   # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        one = 4096
        io = orbfe.CovisUpdateIO(d_slots=one, d_weights=one, d_count=one, d_status=one)
        par = orbfe.CovisUpdateParams()
        upd = lambda s: L.orbfe_covis_update_connections_device(ex.h, C.byref(par), cv.h, 1, p(arr(s)), p(arr(0)), C.byref(io), None)   # noqa: E731
        assert upd(0) == INVALID                                                # connections not enabled
        assert L.orbfe_covis_set_connections(ex.h, cv.h, 1, p(arr(0)), p(arr(0, 0)), None, None) == INVALID
        rec = orbfe.CovisKeyframe()
        buf = np.zeros(16, np.int32)
        assert L.orbfe_covis_get_keyframe(ex.h, cv.h, 0, C.byref(rec), p(buf), p(buf), p(buf), None, None) == INVALID
        assert cv.get_keyframe(1)["conn"] is None and cv.get_keyframe(1)["bad"] == 1    # a graph without connections reads back as before
        for stride in (0, -1, orbfe.COVIS_MAX_CONN_STRIDE + 1):
            assert L.orbfe_covis_enable_connections(ex.h, cv.h, stride) == INVALID
        cv.enable_connections(4)
        assert L.orbfe_covis_enable_connections(ex.h, cv.h, 4) == INVALID       # a second call
        assert upd(-1) == INVALID and upd(g.kf_capacity) == INVALID

        def setc(slots, off, conn, w):
            return L.orbfe_covis_set_connections(ex.h, cv.h, len(slots), p(arr(*slots)), p(arr(*off)), p(arr(*conn)), p(arr(*w)))
        assert setc([g.kf_capacity], [0, 1], [0], [1]) == INVALID and setc([-1], [0, 1], [0], [1]) == INVALID
        assert setc([1, 1], [0, 1, 2], [0, 2], [1, 1]) == INVALID               # named twice
        assert setc([1], [1, 0], [0], [1]) == INVALID                           # descending offsets
        assert setc([1], [0, 5], [0, 2, 3, 0, 2], [1] * 5) == INVALID           # longer than conn_stride
        assert setc([1], [0, 1], [g.kf_capacity], [1]) == INVALID and setc([1], [0, 1], [0], [-1]) == INVALID
        assert L.orbfe_covis_get_keyframe(ex.h, cv.h, g.kf_capacity, C.byref(rec), p(buf), p(buf), None, None, None) == INVALID
        assert cv.get_keyframe(1)["conn"] == {}                                 # nothing was written by the refused calls

        def add(n=2, **k):
            r_ = orbfe.CovisKeyframe(**{**dict(slot=0, mn_id=0), **k})
            return L.orbfe_covis_add_keyframe_device(ex.h, cv.h, C.byref(r_), one, n, one, one, None)
        assert add(slot=-1) == INVALID and add(slot=g.kf_capacity) == INVALID and add(mn_id=-1) == INVALID
        assert add(parent=g.kf_capacity) == INVALID and add(prev=-2) == INVALID and add(n=sc.cg.kf_stride + 1) == INVALID
        other = orbfe.ORBextractor(*ARGS)
        try:
            assert L.orbfe_covis_enable_connections(other.h, cv.h, 4) == INVALID     # a graph of another handle
            assert L.orbfe_covis_add_keyframe_device(other.h, cv.h, C.byref(orbfe.CovisKeyframe(slot=0, mn_id=0)), one, 2, one, one, None) == INVALID
        finally:
            other.close()
        mp.close()                                                              # the map goes first: every later call is refused
        assert upd(0) == INVALID and add() == INVALID
    finally:
        cv.close()
        mp.close()

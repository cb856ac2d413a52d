"""orbfe_covis_refresh_points_device / _refresh_points, the refresh setters, orbfe_covis_get_point and the index that
orbfe_covis_add_keyframe* store, on the GPU (SPEC DECISION S26).  Every comparison is exact equality with tests/point_refresh_ref.py: the
status, both distances as bit patterns, the best slot / index / median of every entry, and afterwards every point read back (observation
slots and indices, reference slot, the map record's distances and the 32 descriptor bytes).  The shapes are the smallest that reach
every path (tests/point_refresh_scenarios.py; tests/test_point_refresh.py proves the planted cases tell the rules from their mutants):
observer counts either side of the 64 lanes of the wave path, list lengths either side of a wave and of a block of waves."""
import copy

import numpy as np
import pytest

import covis_update_ref as U
import covis_update_scenarios as CS
import local_map_ref as R
import local_map_scenarios as LS
import point_refresh_ref as P
import point_refresh_scenarios as S

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
POISON = -77
GUARD = 8
FIELDS = ("status", "min_distance", "max_distance", "best_slot", "best_index", "best_median")


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


@pytest.fixture(scope="module")
def shapes():
    return S.shapes_graph()


class Resident:
    """a RefreshGraph in HBM and, beside it, the restatement's copy that the same calls are played on"""

    def __init__(self, ex, rg):
        import orbfe
        self.o, self.ex, self.rg = orbfe, ex, copy.deepcopy(rg)
        self.mp, self.cv = S.upload(orbfe, ex, rg)

    def close(self):
        self.cv.close()
        self.mp.close()

    def device(self, ids, what, select=None, select_value=1, stream=None, d_ids=None, d_select=None):
        """one refresh_points_device on a stream of its own, outputs poisoned, GUARD words behind each -> dict of arrays"""
        import torch
        n = len(ids)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()   # noqa: E731
        d_ids = up(ids) if d_ids is None else d_ids
        if select is not None and d_select is None:
            d_select = up(select)
        bufs = {k: torch.full((n + GUARD,), POISON, dtype=torch.float32 if "distance" in k else torch.int32, device="cuda") for k in FIELDS}
        io = self.o.RefreshIO(**{"d_" + k: bufs[k].data_ptr() for k in FIELDS})
        st = torch.cuda.Stream() if stream is None else stream
        torch.cuda.synchronize()
        self.cv.refresh_points_device(n, d_ids.data_ptr(), what, io, d_select.data_ptr() if d_select is not None else None, select_value,
                                      st.cuda_stream)
        st.synchronize()
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
        for k, v in out.items():
            assert (v[n:] == POISON).all(), "guard words behind %s written" % k
        return {k: v[:n] for k, v in out.items()}

    def check(self, got, ids, what, select=None, select_value=1, note=""):
        """the same call on the restatement; outputs and then every point compared"""
        want = P.refresh_points(self.rg, ids, what, select, select_value)
        for k in FIELDS:
            assert got[k].tobytes() == want[k].tobytes(), "%s: %s\n%r\n%r" % (note, k, got[k], want[k])
        self.check_state(note)

    def check_state(self, note="", ids=None):
        got, want = S.read_state(self.cv, self.rg, ids), S.state(self.rg, ids)
        for p, (a, b) in enumerate(zip(got, want)):
            assert a == b, "%s: point %d\n%r\n%r" % (note, p if ids is None else ids[p], a, b)


def test_planted_graph_equals_the_restatement(ex):
    rg = S.planted_graph()
    r = Resident(ex, rg)
    try:
        r.check_state("as uploaded (the setters and orbfe_covis_get_point)")
        ids = S.PLANTED_IDS + [16, 19, -1, 20, 1 << 30]                        # points never set, ids outside the map
        got = r.device(ids, 3)
        for name, c in S.CASES.items():                                      # the hand-worked values themselves
            want = S.expected(rg, name)
            at = ids.index(c["p"])
            assert all(np.asarray(got[k][at]).tobytes() == np.asarray(want[k], got[k].dtype).tobytes() for k in want), name
        r.check(got, ids, 3, note="planted")
    finally:
        r.close()


@pytest.mark.parametrize("what", (1, 2, 3))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_lists_on_the_shapes_graph(ex, shapes, what, n):
    """every observer count, ids repeated and outside the map, all three masks, with and without d_select"""
    rng = np.random.default_rng(100 * n + what)
    C = shapes.g.capacity
    ids = rng.integers(-2, C + 3, n).astype(np.int32)
    ids[:min(n, len(S.OBSERVER_COUNTS))] = rng.permutation(len(S.OBSERVER_COUNTS))[:min(n, len(S.OBSERVER_COUNTS))]
    if n == 1:
        ids[0] = 8                                                          # the 130-observer point alone: a list of one rest entry
    r = Resident(ex, shapes)
    try:
        got = r.device(ids, what)
        r.check(got, ids, what, note="n = %d, what = %d" % (n, what))
        if n > 1:
            assert len(set(ids.tolist())) < n or n < 64                     # repeated ids occur
        select = rng.integers(0, 3, n).astype(np.int32)
        got = r.device(ids, what, select, 2)
        r.check(got, ids, what, select, 2, note="n = %d, what = %d, selected" % (n, what))
        assert (got["status"][select != 2] == 0).all()
    finally:
        r.close()


def test_lists_of_one_path_only(ex, shapes):
    rest = [p for p in range(shapes.g.capacity) if len(shapes.g.obs[p]) > 64]
    wave = [p for p in range(shapes.g.capacity) if len(shapes.g.obs[p]) <= 64]
    assert len(rest) == 2 and [len(shapes.g.obs[p]) for p in rest] == [65, 130]
    r = Resident(ex, shapes)
    try:
        for ids, note in ((rest * 3, "rest list only"), (wave, "wave path only"), (rest + wave, "both"), (wave + rest, "both, rest last")):
            got = r.device(ids, 3)
            r.check(got, ids, 3, note=note)
    finally:
        r.close()


def test_existing_distinctive_descriptors_agrees(ex, shapes):
    """a second yardstick from existing code: the collected descriptors of every point gathered on the host in ascending mn_id and
    passed through orbfe_distinctive_descriptors (first minimum = lowest mn_id) give the same observer and median"""
    import orbfe
    g = shapes.g
    r = Resident(ex, shapes)
    try:
        ids = np.arange(g.capacity)
        got = r.device(ids, 2)
        rows, off, desc = [], [0], []
        for p in ids:
            c = sorted((int(g.mn_id[s]), j, s, i) for j, (s, i) in enumerate(zip(g.obs[p], shapes.obs_idx[p]))
                       if not g.kf_bad[s] and 0 <= i < len(shapes.desc[s]) and not g.point_bad[p])
            rows.append(c)
            off.append(off[-1] + len(c))
            desc += [shapes.desc[s][i] for _, _, s, i in c]
        idx, median = orbfe.ORBmatcher(ex).ComputeDistinctiveDescriptors(np.array(off, np.int32), np.array(desc, np.uint8))
        paths = set()
        for p in ids:
            if rows[p]:
                _, _, s, i = rows[p][idx[p]]
                assert (got["best_slot"][p], got["best_index"][p], got["best_median"][p]) == (s, i, median[p]), p
                paths.add(len(g.obs[p]) > 64)
            else:
                assert got["status"][p] == 0 and got["best_slot"][p] == -1
        assert paths == {False, True}
    finally:
        r.close()


def test_host_form_and_split_calls_give_the_same(ex, shapes):
    C = shapes.g.capacity
    ids = np.concatenate([np.arange(C), [3, 8, 8, -1, C]]).astype(np.int32)
    one, two, host = Resident(ex, shapes), Resident(ex, shapes), Resident(ex, shapes)
    try:
        for what in (3, 1, 2):
            a = one.device(ids, what)
            h = 37
            b1, b2 = two.device(ids[:h], what), two.device(ids[h:], what)
            c = host.cv.refresh_points(ids, what)
            for k in FIELDS:
                assert a[k].tobytes() == np.concatenate([b1[k], b2[k]]).tobytes() == c[k].tobytes(), (what, k)
            one.check(a, ids, what, note="one call")
        assert S.read_state(one.cv, shapes) == S.read_state(two.cv, shapes) == S.read_state(host.cv, shapes)
        a = one.device(ids[::-1].copy(), 3)                                 # the order of the list
        b = two.device(ids, 3)
        for k in FIELDS:
            assert a[k][::-1].tobytes() == b[k].tobytes(), k
    finally:
        one.close()
        two.close()
        host.close()


def test_old_observation_setter_writes_no_index(ex):
    rg = S.planted_graph()
    r = Resident(ex, rg)
    try:
        ids = [0, 5]
        off = np.cumsum([0] + [len(rg.g.obs[p]) for p in ids]).astype(np.int32)
        r.cv.set_observations(ids, off, [s for p in ids for s in rg.g.obs[p]])
        for p in ids:
            r.rg.set_observations(p, rg.g.obs[p])
        r.check_state("orbfe_covis_set_observations on a graph with refresh state")
        got = r.device(ids, 3)
        r.check(got, ids, 3, note="indices of -1")
        assert got["status"].tolist() == [0, 0]                              # nothing collected, the reference key frame's index is -1
    finally:
        r.close()


def _features(rng, n):
    import orbfe
    kp = np.zeros(n, orbfe.KP_DTYPE)
    kp["octave"] = rng.integers(-1, S.N_LEVELS + 2, n)                      # the device form clamps
    centres = rng.integers(0, 256, (3, 32)).astype(np.uint8)
    d = centres[rng.integers(0, 3, n)].copy()
    d[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
    return kp, d


def test_chain_on_a_graph_built_on_the_device(ex):
    """set_features_device -> add_keyframe_device -> refresh_points_device(d_point_ids, d_added, 1) -> update_connections_device on ONE
    stream, for the random graph of local_map_scenarios.py key frame by key frame; the restatements are run in the same order and every
    output, every point and every key frame is compared at the end of each key frame's chain (outputs) and of the run (state)."""
    import torch
    import orbfe
    sc = LS.random_scene()
    src, n_pts = sc.g, sc.g.capacity
    g = R.Graph(src.kf_capacity, n_pts)
    g.point_bad[:] = src.point_bad
    cg = U.ConnGraph(g, kf_stride=sc.kf_stride, obs_stride=16, child_stride=16, conn_stride=32)
    rg = P.RefreshGraph(g, sc.kf_stride, 16, S.SCALE_FACTORS)
    rng = np.random.default_rng(3)
    rg.pos[:] = rng.uniform(-9, 9, (n_pts, 3)).astype(np.float32)
    mp, cv = CS.upload(orbfe, ex, cg)
    pts = np.zeros(n_pts, orbfe.WP_DTYPE)
    pts["x"], pts["y"], pts["z"] = rg.pos.T
    pts["bad"], pts["observations"] = src.point_bad, 1
    mp.update(np.arange(n_pts), pts, np.zeros((n_pts, 32), np.uint8))
    cv.enable_refresh(S.SCALE_FACTORS)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype.names else np.ascontiguousarray(a)).cuda()   # noqa: E731
    st = torch.cuda.Stream()
    order = sorted((s for s in range(src.kf_capacity) if src.is_set[s]), key=lambda s: int(src.mn_id[s]))
    touched, refreshed = set(), 0
    try:
        for k, s in enumerate(order):
            row = np.ascontiguousarray(src.points[s], np.int32)
            n = len(row)
            kp, desc = _features(rng, n)
            centre = rng.uniform(-2, 2, 3).astype(np.float32)
            ref_ids = [int(p) for p in set(row.tolist()) if 0 <= p < n_pts and rg.ref[p] < 0]
            cv.set_centres([s], centre)                                      # host setters: the mapping thread's side
            if ref_ids:
                cv.set_ref_keyframes(ref_ids, [s] * len(ref_ids))           # a new point's mpRefKF is the key frame that made it
            d_kp, d_desc, d_row = up(kp), up(desc), up(row if n else np.zeros(1, np.int32))   # (keypoint records go up as bytes)
            d_added = torch.full((max(n, 1) + GUARD,), POISON, dtype=torch.int32, device="cuda")
            d_status = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
            bufs = {f: torch.full((max(n, 1),), POISON, dtype=torch.float32 if "distance" in f else torch.int32, device="cuda") for f in FIELDS}
            Sd = cv.conn_stride
            d_cs, d_cw = torch.zeros(Sd, dtype=torch.int32, device="cuda"), torch.zeros(Sd, dtype=torch.int32, device="cuda")
            d_cn, d_cst = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            cv.set_features_device(s, d_kp.data_ptr(), d_desc.data_ptr(), n, st.cuda_stream)
            cv.add_keyframe_device(s, int(src.mn_id[s]), d_row.data_ptr(), n, d_added.data_ptr(), d_status.data_ptr(), bad=int(src.kf_bad[s]),
                                   prev=int(src.prev[s]), stream=st.cuda_stream)
            if n:
                cv.refresh_points_device(n, d_row.data_ptr(), 3, orbfe.RefreshIO(**{"d_" + f: bufs[f].data_ptr() for f in FIELDS}),
                                         d_added.data_ptr(), 1, st.cuda_stream)
            cv.update_connections_device([s], [1 if k else 0], orbfe.CovisUpdateIO(d_slots=d_cs.data_ptr(), d_weights=d_cw.data_ptr(),
                                                                                   d_count=d_cn.data_ptr(), d_status=d_cst.data_ptr()),
                                         orbfe.CovisUpdateParams(15), st.cuda_stream)
            st.synchronize()
            # the restatements, in the same order
            rg.centre[s] = centre
            rg.ref[ref_ids] = s
            rg.set_features(s, kp["octave"], desc)
            added, status = U.add_keyframe(cg, s, int(src.mn_id[s]), row, bad=bool(src.kf_bad[s]), prev=int(src.prev[s]))
            rg.index_added(s, row, added)
            assert int(d_status.cpu()[0]) == status == U.OK and np.array_equal(d_added.cpu().numpy()[:n], added)
            if n:
                want = P.refresh_points(rg, row, 3, added, 1)
                for f in FIELDS:
                    assert bufs[f].cpu().numpy().tobytes() == want[f].tobytes(), (k, f)
                refreshed += int((want["status"] == 3).sum())
            touched |= set(int(p) for p in row[added == 1])
            wantc = U.update_connections(cg, s, 1 if k else 0, 15)
            assert int(d_cn.cpu()[0]) == wantc["count"] and np.array_equal(d_cs.cpu().numpy(), wantc["slots"])
        ids = sorted(touched)
        assert S.read_state(cv, rg, ids) == S.state(rg, ids)
        for s in order:
            assert cv.get_keyframe(s) == cg.keyframe(s), s
        assert len(ids) > 300 and refreshed > 500                           # the scene exercises what it is for
    finally:
        cv.close()
        mp.close()


def test_a_graph_without_refresh_state_is_what_it_was(ex):
    """one S25 scene on a graph without and on a graph with the refresh state: the same outputs, the same key frames; the new calls are
    refused on the first"""
    import ctypes as C
    import orbfe
    import test_covis_update_gpu as G
    sc = CS.planted_scenes()["row_keeps_unconnected"]
    plain, enabled = G.Resident(ex, sc.cg), G.Resident(ex, sc.cg)
    L, INVALID, one = orbfe.lib(), 1, 4096
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    try:
        buf, f3 = np.zeros(64, np.int32), np.zeros(3, np.float32)
        n = C.c_int(0)
        io = orbfe.RefreshIO()
        assert L.orbfe_covis_refresh_points_device(ex.h, plain.cv.h, 1, one, None, 0, 3, C.byref(io), None) == INVALID
        assert L.orbfe_covis_refresh_points(ex.h, plain.cv.h, 1, p(buf), 3, None, None, None, None, None, None) == INVALID
        assert L.orbfe_covis_set_features(ex.h, plain.cv.h, 0, 0, None, None) == INVALID
        assert L.orbfe_covis_set_features_device(ex.h, plain.cv.h, 0, one, one, 1, None) == INVALID
        assert L.orbfe_covis_set_centres(ex.h, plain.cv.h, 1, p(buf), p(f3)) == INVALID
        assert L.orbfe_covis_set_observations_indexed(ex.h, plain.cv.h, 1, p(buf), p(np.array([0, 1], np.int32)), p(buf), p(buf)) == INVALID
        assert L.orbfe_covis_set_ref_keyframes(ex.h, plain.cv.h, 1, p(buf), p(buf)) == INVALID
        assert L.orbfe_covis_get_point(ex.h, plain.cv.h, 0, C.byref(n), p(buf), p(buf), C.byref(n), None, None) == INVALID
        enabled.cv.enable_refresh(S.SCALE_FACTORS)
        for r in (plain, enabled):
            r.play(sc.ops)
            r.check_state("row_keeps_unconnected")
        assert plain.state() == enabled.state()
    finally:
        plain.close()
        enabled.close()

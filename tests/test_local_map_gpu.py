"""orbfe_update_local_map_batch_device, orbfe_update_local_map and orbfe_frame_points_batch_device on the GPU (SPEC DECISION S24).
Every comparison is exact equality of every output array with tests/local_map_ref.py.  The shapes are the smallest at which each
mechanism can go wrong: the random scene (more than one block's worth of walk per frame, 20 frames), the planted scene of every rule
(tests/test_local_map.py proves that each tells its mutants apart), walks around the block size, rows around M, the vote table's switch
count, no voter at all, a graph that changes between calls, and the hand-over of the id rows to the inertial chain."""
import numpy as np
import pytest

import local_map_ref as R
import local_map_scenarios as S

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
    """a scene's graph in HBM, and its frames through the batch call"""

    def __init__(self, ex, sc):
        import orbfe
        self.o, self.ex, self.sc = orbfe, ex, sc
        self.mp, self.cv = S.upload(orbfe, ex, sc)

    def close(self):
        self.cv.close()
        self.mp.close()

    def run(self, frames, vote_stride=None, alias_votes=False, **over):
        """the frames (indices into sc.frames) as ONE batch call on a stream of its own, every output poisoned first, GUARD words
        behind the id rows -> per frame the restatement's dict"""
        import torch
        o, sc = self.o, self.sc
        B, M = len(frames), sc.M
        stride = vote_stride or max(1, max(len(sc.frames[f][0]) for f in frames)) + 3
        votes = np.full((B, stride), 1, np.int32)                   # beyond n_votes: a valid id that must not vote
        for b, f in enumerate(frames):
            votes[b, :len(sc.frames[f][0])] = sc.frames[f][0]
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d_votes, d_n = dev(votes), dev(np.array([len(sc.frames[f][0]) for f in frames], np.int32))
        d_last = dev(np.array([sc.frames[f][1] for f in frames], np.int32))
        full = lambda n: torch.full((n,), POISON, dtype=torch.int32, device="cuda")   # noqa: E731
        d_ids, d_np, d_kfs, d_nk, d_vout = full(B * M + GUARD), full(B), full(B * R.LOCAL_KF_MAX + GUARD), full(B), full(B * stride)
        io = o.LocalMapIO(d_vote_ids=d_votes.data_ptr(), d_n_votes=d_n.data_ptr(), d_last_kf=d_last.data_ptr(), d_ids_out=d_ids.data_ptr(),
                          d_n_local_points=d_np.data_ptr(), d_local_kfs=d_kfs.data_ptr(), d_n_local_kfs=d_nk.data_ptr(),
                          d_vote_ids_out=d_votes.data_ptr() if alias_votes else d_vout.data_ptr())
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        o.update_local_map_batch_device(self.ex, o.LocalMapParams(**{**sc.params, **over}), B, stride, self.cv, M, io, st.cuda_stream)
        st.synchronize()
        ids, kfs = d_ids.cpu().numpy(), d_kfs.cpu().numpy()
        assert (ids[B * M:] == POISON).all() and (kfs[B * R.LOCAL_KF_MAX:] == POISON).all(), "guard words behind the rows written"
        vout = (d_votes if alias_votes else d_vout).cpu().numpy().reshape(B, stride)
        out = []
        for b, f in enumerate(frames):
            n = len(sc.frames[f][0])
            assert (vout[b, n:] == (1 if alias_votes else POISON)).all(), "vote ids beyond n_votes written"
            out.append(dict(ids=ids[b * M:(b + 1) * M], n_local_points=int(d_np[b]), local_kfs=kfs[b * R.LOCAL_KF_MAX:(b + 1) * R.LOCAL_KF_MAX],
                            n_local_kfs=int(d_nk[b]), vote_ids=vout[b, :n]))
        self.d_ids = d_ids
        return out


def same(got, want, what):
    for k in ("n_local_kfs", "n_local_points"):
        assert got[k] == want[k], "%s: %s %r != %r" % (what, k, got[k], want[k])
    for k in ("local_kfs", "ids", "vote_ids"):
        assert np.array_equal(got[k], want[k]), "%s: %s\n%r\n%r" % (what, k, got[k][:24], want[k][:24])


@pytest.fixture(scope="module")
def random_resident(ex):
    r = Resident(ex, S.random_scene())
    yield r
    r.close()


@pytest.mark.parametrize("mark", (0, 1))
@pytest.mark.parametrize("inertial", (0, 1))
def test_random_scene_as_one_batch_and_as_single_frames(random_resident, inertial, mark):
    r, sc = random_resident, random_resident.sc
    nf = len(sc.frames)
    want = [sc.ref(f, inertial=inertial, mark_voters_seen=mark) for f in range(nf)]
    batch = r.run(list(range(nf)), vote_stride=256, inertial=inertial, mark_voters_seen=mark)
    for f in range(nf):
        same(batch[f], want[f], "batch of %d, frame %d" % (nf, f))
        single = r.run([f], vote_stride=256, inertial=inertial, mark_voters_seen=mark)[0]
        same(single, want[f], "batch of 1, frame %d" % f)
        same(single, batch[f], "batch of 1 against the batch, frame %d" % f)
    if mark:
        assert sum(int((w["ids"] < 0).sum()) for w in want) > 100          # voters were emitted complemented
    print("local key frames", [w["n_local_kfs"] for w in want], "points", [w["n_local_points"] for w in want])


@pytest.mark.parametrize("name", sorted(S.planted_scenes()))
def test_planted_rule_scenes(ex, name):
    sc = S.planted_scenes()[name]
    r = Resident(ex, sc)
    try:
        same(r.run([0])[0], sc.ref(0), name)
        same(r.run([0], alias_votes=True)[0], sc.ref(0), name + ", vote ids cleared in place")
        same(r.run([0], mark_voters_seen=1)[0], sc.ref(0, mark_voters_seen=1), name + ", voters marked")
    finally:
        r.close()


def test_voter_that_is_a_local_point_is_emitted_complemented(ex):
    sc = S.planted_scenes()["first_occurrence"]
    sc.g.obs[7] = [1]
    sc.frames = [([50, 7, 51], -1)]
    r = Resident(ex, sc)
    try:
        got = r.run([0], mark_voters_seen=1)[0]
        same(got, sc.ref(0, mark_voters_seen=1), "voter 7")
        assert list(got["ids"][:5]) == [~7, 30, 31, 20, 21]
        same(r.run([0])[0], sc.ref(0), "voter 7, not marked: the mark of the call before is gone")
    finally:
        r.close()


def _walks():
    import orbfe
    T = orbfe.LOCAL_MAP_BLOCK
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1]


def test_walk_boundaries(ex):
    walks = _walks()
    for W in walks:
        sc = S.walk_scene(W, first_recurs_last=W == walks[-1])
        r = Resident(ex, sc)
        try:
            got, want = r.run([0])[0], sc.ref(0)
            same(got, want, "walk of %d" % W)
            assert got["n_local_points"] == (W - 1 if W == walks[-1] else W)     # the recurrence in the last chunk is not emitted again
        finally:
            r.close()


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_truncation_at_the_row_length(ex, delta):
    M = 64
    sc = S.truncation_scene(M + delta, M)
    r = Resident(ex, sc)
    try:
        got = r.run([0])[0]                                                     # (run() checks the guard words behind the row)
        same(got, sc.ref(0), "unique = M %+d" % delta)
        assert got["n_local_points"] == M + delta
        assert (got["ids"][-1] == R.NO_POINT) == (delta < 0)
    finally:
        r.close()


@pytest.mark.parametrize("extra", (0, 1))
def test_vote_table_switch_count(ex, extra):
    """the LDS table at its last key and one past it (the HBM counters), every count 1: the max_local_kf smallest mn_id; twice, and
    then a frame that fits the table on the same graph: the counters were put back"""
    import orbfe
    sc = S.vote_table_scene(orbfe.LOCAL_MAP_VOTE_TABLE + extra)
    sc.frames.append(([8, 9, 10], -1))
    sc.g.obs[8], sc.g.obs[9], sc.g.obs[10] = [3, 4], [3], [5]
    r = Resident(ex, sc)
    try:
        want = sc.ref(0)
        assert list(want["local_kfs"][:10]) == list(range(sc.g.kf_capacity - 1, sc.g.kf_capacity - 11, -1))
        same(r.run([0])[0], want, "first call")
        same(r.run([0])[0], want, "second call")
        same(r.run([1])[0], sc.ref(1), "a frame in the table after one in the counters")
        both = r.run([0, 1, 0])
        for b, f in enumerate((0, 1, 0)):
            same(both[b], sc.ref(f), "mixed batch, frame %d" % b)
    finally:
        r.close()


def test_no_voters(ex):
    sc = S.no_voter_scene()
    r = Resident(ex, sc)
    try:
        got = r.run([0, 1])
        same(got[0], sc.ref(0), "temporal chain alone")
        same(got[1], sc.ref(1), "no last key frame")
        assert got[0]["n_local_kfs"] == 3 and got[1]["n_local_kfs"] == 0
        for f in (0, 1):
            g = r.run([f], inertial=0)[0]
            same(g, sc.ref(f, inertial=0), "not inertial")
            assert g["n_local_kfs"] == 0 and g["n_local_points"] == 0 and (g["ids"] == R.NO_POINT).all()
    finally:
        r.close()


def test_stale_state_and_graph_updates(ex):
    sc = S.random_scene(seed=3, n_frames=2)
    r = Resident(ex, sc)
    try:
        for f in (0, 1, 0):
            same(r.run([f], vote_stride=256)[0], sc.ref(f), "frame %d of A, B, A" % f)
        # one key frame of frame 0's local map loses its first 40 features and turns up with a new list; one voter's observations move
        before = sc.ref(0)
        s = int(before["local_kfs"][0])
        sc.g.points[s] = np.concatenate([sc.g.points[s][40:], np.array([5, 6, 7], np.int32)])
        voter = next(int(p) for p in sc.frames[0][0] if 0 <= p < sc.g.capacity and not sc.g.point_bad[p] and len(sc.g.obs[p]) > 1)
        sc.g.obs[voter] = sc.g.obs[voter][:1]
        r.cv.set_keyframes([sc.g.record(s)])
        r.cv.set_observations(*sc.g.observations_csr([voter]))
        after = sc.ref(0)
        assert not np.array_equal(after["ids"], before["ids"])
        same(r.run([0], vote_stride=256)[0], after, "frame A on the updated graph")
        # scalars alone: the key frame turns bad, its stored feature list stays
        sc.g.kf_bad[s] = True
        r.cv.set_keyframes([sc.g.record(s, with_points=False)])
        same(r.run([0], vote_stride=256)[0], sc.ref(0), "frame A with the key frame bad")
    finally:
        r.close()


def test_host_call_equals_batch_of_one(random_resident):
    import orbfe
    r, sc = random_resident, random_resident.sc
    for f in (0, 7):
        for mark in (0, 1):
            votes, last = sc.frames[f]
            got = orbfe.update_local_map(r.ex, orbfe.LocalMapParams(**{**sc.params, "mark_voters_seen": mark}), votes, last, r.cv, sc.M)
            same(got, r.run([f], vote_stride=256, mark_voters_seen=mark)[0], "host call, frame %d" % f)
            same(got, sc.ref(f, mark_voters_seen=mark), "host call against the restatement, frame %d" % f)


def test_refusals_with_a_handle(ex):
    import ctypes as C
    import orbfe
    sc = S.planted_scenes()["double_vote"]
    r = Resident(ex, sc)
    try:
        L, g = orbfe.lib(), sc.g
        pts = np.arange(5, dtype=np.int32)
        rec = orbfe.CovisKeyframe(slot=0, mn_id=0, n_features=5, point_ids=pts.ctypes.data)
        call = lambda k: L.orbfe_covis_set_keyframes(ex.h, r.cv.h, 1, C.byref(k))   # noqa: E731
        rec.n_features = sc.kf_stride + 1
        assert call(rec) == 1                                                   # a list longer than its stride
        rec.n_features, rec.parent = 3, g.kf_capacity
        assert call(rec) == 1
        rec.parent, rec.slot = -1, g.kf_capacity
        assert call(rec) == 1
        ids, off, slots = np.array([50], np.int32), np.array([0, sc.obs_stride + 1], np.int32), np.zeros(8, np.int32)
        obs = lambda: L.orbfe_covis_set_observations(ex.h, r.cv.h, 1, ids.ctypes.data, off.ctypes.data, slots.ctypes.data)   # noqa: E731
        assert obs() == 1
        off[1], slots[0] = 1, g.kf_capacity
        assert obs() == 1
        same(r.run([0])[0], sc.ref(0), "nothing was written by the refused calls")
        other = orbfe.ORBextractor(*ARGS)
        try:
            with pytest.raises(orbfe.OrbfeError):
                orbfe.update_local_map(other, orbfe.LocalMapParams(), [50], -1, r.cv, 16)   # a graph of another handle
        finally:
            other.close()
    finally:
        r.close()


def test_hand_over_to_the_inertial_chain(ex, monkeypatch):
    """the id rows the batch call wrote go, as the device buffer they are in, to orbfe_track_inertial_batch_device: every output equals
    the same call with those rows uploaded from the host; orbfe_frame_points_batch_device on that call's outputs equals its statement"""
    import torch
    import orbfe
    import test_track_inertial_gpu as TG
    import track_inertial_scenarios as TS
    M = 70
    frames, capacity, points, desc = TS.make_batch(("ordinary", "ordinary"), M, orbfe.WP_DTYPE, orbfe.KP_DTYPE)
    # frame b's local map: ONE key frame that holds the scene's points of that frame but the "no point" slot, voted for by the point
    # of the skipped slot -- which, as a voter, comes out complemented, as the scene has it
    g = R.Graph(len(frames), capacity)
    g.point_bad[:] = points["bad"] != 0
    votes = []
    for b, f in enumerate(frames):
        keep = [int(~i) if i < 0 else int(i) for k, i in enumerate(f["ids"]) if k != TS.S_NOPOINT]
        g.set_keyframe(b, b, points=keep)
        g.obs[keep[0]] = [b]
        votes.append(([keep[0]], -1))
    sc = S.Scene(g, votes, M, inertial=0, mark_voters_seen=1)
    mp = orbfe.MapPoints(ex, capacity)
    mp.update(np.arange(capacity), points, desc)
    cv = orbfe.Covisibility(ex, mp, g.kf_capacity, sc.kf_stride, sc.obs_stride, sc.child_stride)
    cv.set_keyframes([g.record(s) for s in range(g.kf_capacity)])
    cv.set_observations(*g.observations_csr([v[0][0] for v in votes]))
    r = Resident.__new__(Resident)
    r.o, r.ex, r.sc, r.mp, r.cv = orbfe, ex, sc, mp, cv
    try:
        rows = r.run([0, 1])
        for b, f in enumerate(frames):
            same(rows[b], sc.ref(b), "the scene's row, frame %d" % b)
            want_row = np.array([i for k, i in enumerate(f["ids"]) if k != TS.S_NOPOINT] + [R.NO_POINT], np.int32)
            assert np.array_equal(rows[b]["ids"], want_row)
            f["ids"] = rows[b]["ids"].copy()
        priors = TG.priors_of(frames, 0)
        from_host = TG.run_device(ex, frames, 0, capacity, points, desc, priors)
        d_rows = r.d_ids[:len(frames) * M]
        plain = TG._dev

        def dev(t, a):
            a = np.asarray(a)
            if a.dtype == np.int32 and a.shape == (len(frames), M):
                return d_rows                                                   # the buffer the batch call wrote, unchanged
            return plain(t, a)
        monkeypatch.setattr(TG, "_dev", dev)
        handed = TG.run_device(ex, frames, 0, capacity, points, desc, priors)
        monkeypatch.setattr(TG, "_dev", plain)
        for b in range(len(frames)):
            TG.same(handed[b], from_host[b], "ids handed over in HBM, frame %d" % b)
            assert handed[b]["n_matches"] > 30 and handed[b]["matches_inliers"] > 30
        # the frames' mvpMapPoints from those outputs
        n = np.array([f["n"] for f in frames], np.int32)
        match = np.full((len(frames), TG.KP_STRIDE), M + 3, np.int32)           # beyond d_n: matches that must be ignored
        outl = np.zeros((len(frames), TG.KP_STRIDE), np.uint8)
        for b, h in enumerate(handed):
            match[b, :n[b]], outl[b, :n[b]] = h["match"], h["outlier"]
        match[0, 0] = M - 1                                                     # a match on the pad: no point
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()         # noqa: E731
        d_match, d_outl, d_n = up(match), up(outl), up(n)
        d_out = torch.full((len(frames) * TG.KP_STRIDE,), POISON, dtype=torch.int32, device="cuda")
        orbfe.frame_points_batch_device(ex, mp, len(frames), TG.KP_STRIDE, M, d_rows.data_ptr(), d_match.data_ptr(), d_outl.data_ptr(),
                                        d_n.data_ptr(), d_out.data_ptr())
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().reshape(len(frames), TG.KP_STRIDE)
        for b, f in enumerate(frames):
            want = R.frame_points(f["ids"], match[b], outl[b], n[b], points["observations"], capacity)
            assert np.array_equal(out[b], want), b
            assert (want >= 0).sum() > 30 and (want[:n[b]] == -1).any()
    finally:
        cv.close()
        mp.close()


def test_lifetime_in_any_order(built):
    """the handle first, then the graph and the map (only shells are left); the map first: the graph refuses every later call"""
    import orbfe
    sc = S.planted_scenes()["double_vote"]
    e = orbfe.ORBextractor(*ARGS)
    mp, cv = S.upload(orbfe, e, sc)
    e.close()
    cv.close()
    mp.close()
    e = orbfe.ORBextractor(*ARGS)
    mp, cv = S.upload(orbfe, e, sc)
    votes, last = sc.frames[0]
    par = orbfe.LocalMapParams(**sc.params)
    same(orbfe.update_local_map(e, par, votes, last, cv, sc.M), sc.ref(0), "before the map goes")
    mp.close()
    with pytest.raises(orbfe.OrbfeError):
        orbfe.update_local_map(e, par, votes, last, cv, sc.M)
    with pytest.raises(orbfe.OrbfeError):
        cv.set_keyframes([sc.g.record(0)])
    cv.close()
    e.close()

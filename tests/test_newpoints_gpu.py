"""orbfe_triangulate_pairs / orbfe_create_new_points_batch on the GPU against the restatement of SPEC DECISION S11
(newpoints_ref, written from src/LocalMapping.cc:571-705 and src/GeometricTools.cc:47-66) on the scenes of
newpoints_scenarios (test_newpoints.py checks that they reach every gate).  Every comparison is exact: verdict bytes equal
and ALL x3d bytes equal (three zeros where no point exists: verdicts 1, 2 and 255), no tolerance, no skipped pair."""
import threading

import numpy as np
import pytest

import newpoints_ref as R
import newpoints_scenarios as NS
import oracle_py as O
import test_triangulation_batch as TB

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
CAMERAS = {"pinhole": dict(), "kb8": dict(model1=1, model2=1, cam1=NS.KB_CAM, height=512),
           "kb8-pinhole": dict(model1=1, model2=0, cam1=NS.KB_CAM, cam2=NS.PIN_CAM, height=512)}


def np_params(P):
    import orbfe
    return orbfe.newpoint_params(P["Tcw1"], P["Tcw2"], P["twc1"], P["twc2"], P["sigma2_1"], P["sigma2_2"], P["ratioFactor"], P["model1"],
                                 P["model2"], P["cam1"], P["cam2"], P["precision"], P["inertial"], P["farPoints"], P["thFarPoints"])


def keyframes(ex, sc, nbs=None):
    import orbfe
    kf1 = orbfe.KeyFrame(ex, sc["kp1"].view(orbfe.KP_DTYPE), sc["desc1"], sc["node1"], sc["sf"])
    kf2 = [orbfe.KeyFrame(ex, nb["kp"].view(orbfe.KP_DTYPE), nb["desc"], nb["node"], sc["sf"]) for nb in (sc["nbs"] if nbs is None else nbs)]
    return kf1, kf2


def same(got_x, got_v, want_v, want_x, what):
    assert got_v.dtype == np.uint8 and got_x.dtype == np.float32
    bad = np.flatnonzero(got_v != want_v)
    assert len(bad) == 0, "%s: %d verdicts differ, first pair %d: %d, restatement %d" % (what, len(bad), bad[0], got_v[bad[0]], want_v[bad[0]])
    assert got_x.tobytes() == np.ascontiguousarray(want_x, np.float32).tobytes(), "%s: x3D bytes differ" % what


@pytest.mark.parametrize("cams", ["pinhole", "kb8", "kb8-pinhole"])
def test_triangulate_pairs_equals_restatement(built, cams):
    """every neighbour's pair list with its own flags; inertial x far-point gate on two neighbours; n_pairs 0, 1, 63, 64, 65 and
    5200 (the scene's pairs of a neighbour + arbitrary pairs of the two key frames)"""
    import orbfe
    ex = orbfe.ORBextractor(*ARGS)
    sc = NS.scene(1, **CAMERAS[cams])
    kf1, kf2 = keyframes(ex, sc)
    seen = np.zeros(256, int)
    for k, nb in enumerate(sc["nbs"]):
        v, x = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], nb["idx1"], nb["idx2"])
        gx, gv = orbfe.triangulate_pairs(ex, kf1, kf2[k], np_params(nb["np"]), nb["idx1"], nb["idx2"])
        same(gx, gv, v, x, "%s neighbour %d" % (cams, k))
        seen += np.bincount(gv, minlength=256)
    assert all(seen[c] >= 8 for c in (0, 1, 3, 4, 5, 6, 8, 9)), seen[:10]
    for k in (6, 15):
        nb = sc["nbs"][k]
        for inertial in (False, True):
            for far in (False, True):
                P = dict(nb["np"], inertial=inertial, farPoints=far)
                v, x = R.triangulate(P, sc["kp1"], nb["kp"], sc["sf"], sc["sf"], nb["idx1"], nb["idx2"])
                gx, gv = orbfe.triangulate_pairs(ex, kf1, kf2[k], np_params(P), nb["idx1"], nb["idx2"])
                same(gx, gv, v, x, "%s neighbour %d inertial %d far %d" % (cams, k, inertial, far))
    rng = np.random.default_rng(11)
    nb = sc["nbs"][8]
    for n in (0, 1, 63, 64, 65, 5200):
        i1 = np.concatenate([nb["idx1"], rng.integers(0, len(sc["kp1"]), 5200)])[:n].astype(np.int32)
        i2 = np.concatenate([nb["idx2"], rng.integers(0, len(nb["kp"]), 5200)])[:n].astype(np.int32)
        v, x = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], i1, i2)
        gx, gv = orbfe.triangulate_pairs(ex, kf1, kf2[8], np_params(nb["np"]), i1, i2)
        assert len(gv) == n and gx.shape == (n, 3)
        same(gx, gv, v, x, "%s n_pairs %d" % (cams, n))
    # the two hand-built gates
    P, kp1, kp2, sf = NS.infinity_case()
    a = orbfe.KeyFrame(ex, kp1.view(orbfe.KP_DTYPE), np.zeros((1, 32), np.uint8), [0], sf)
    b = orbfe.KeyFrame(ex, kp2.view(orbfe.KP_DTYPE), np.zeros((1, 32), np.uint8), [0], sf)
    gx, gv = orbfe.triangulate_pairs(ex, a, b, np_params(P), [0], [0])
    assert gv[0] == orbfe.NEWPT_AT_INFINITY and not gx.any()
    P, kp1, kp2, sf, i1, i2 = NS.centre_case()
    a = orbfe.KeyFrame(ex, kp1.view(orbfe.KP_DTYPE), np.zeros((len(kp1), 32), np.uint8), np.zeros(len(kp1), np.int32), sf)
    b = orbfe.KeyFrame(ex, kp2.view(orbfe.KP_DTYPE), np.zeros((len(kp2), 32), np.uint8), np.zeros(len(kp2), np.int32), sf)
    v, x = R.triangulate(P, kp1, kp2, sf, sf, i1, i2)
    gx, gv = orbfe.triangulate_pairs(ex, a, b, np_params(P), i1, i2)
    assert gv[0] == orbfe.NEWPT_ZERO_DISTANCE
    same(gx, gv, v, x, "camera centre")
    # indices out of range
    for i1, i2 in (([len(sc["kp1"])], [0]), ([0], [len(nb["kp"])]), ([-1], [0]), ([0], [-1])):
        with pytest.raises(orbfe.OrbfeError) as e:
            orbfe.triangulate_pairs(ex, kf1, kf2[8], np_params(nb["np"]), i1, i2)
        assert e.value.code == orbfe.ERR_INVALID_ARG
    ex.close()


def search_inputs(sc, nbs, seed, coarse_every=4):
    """flags and SearchForTriangulation parameters of a scene: 10 % of key frame 1 and 5 % of every neighbour have a map point;
    every coarse_every-th neighbour is searched with bCoarse (no epipolar test: wrong partners reach the geometry)"""
    rng = np.random.default_rng(seed)
    has1 = (rng.random(len(sc["kp1"])) < 0.10).astype(np.uint8)
    has2 = [(rng.random(len(nb["kp"])) < 0.05).astype(np.uint8) for nb in nbs]
    coarse = [k % coarse_every == coarse_every - 1 for k in range(len(nbs))]
    kb = sc["model1"] == 1
    return has1, has2, coarse, [nb["cameras"] if kb else None for nb in nbs]


def tri_params(nbs, coarse, cams):
    import orbfe
    return [orbfe.tri_params(nb["F12"], nb["ep"], False, coarse[k], True, cams[k]) for k, nb in enumerate(nbs)]


def check_batch(ex, sc, nbs, seed, what):
    """one orbfe_create_new_points_batch call: raw results byte-equal to orbfe_match_triangulation_batch, verdict / x3D of
    EVERY raw partner equal to the restatement, 255 and zeros elsewhere; returns the call's results and inputs"""
    import orbfe
    has1, has2, coarse, cams = search_inputs(sc, nbs, seed)
    kf1, kf2 = keyframes(ex, sc, nbs)
    tp = tri_params(nbs, coarse, cams)
    raw0, bin0 = orbfe.SearchForTriangulation_batch(ex, kf1, has1, kf2, has2, tp)
    raw, rbin, x3d, verdict = orbfe.CreateNewMapPoints_batch(ex, kf1, has1, kf2, has2, tp, [np_params(nb["np"]) for nb in nbs])
    assert raw.tobytes() == raw0.tobytes() and rbin.tobytes() == bin0.tobytes(), what
    for k, nb in enumerate(nbs):
        want_v = np.full(len(sc["kp1"]), R.NO_PARTNER, np.uint8)
        want_x = np.zeros((len(sc["kp1"]), 3), np.float32)
        i1 = np.flatnonzero(raw[k] >= 0)
        want_v[i1], want_x[i1] = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], i1, raw[k][i1])
        same(np.ascontiguousarray(x3d[k]), np.ascontiguousarray(verdict[k]), want_v, want_x, "%s neighbour %d" % (what, k))
    for kf in [kf1] + kf2:
        kf.close()
    return raw, rbin, x3d, verdict, has1, has2, coarse, cams


@pytest.mark.parametrize("cams,K", [("pinhole", 1), ("pinhole", 7), ("pinhole", 20), ("kb8", 7), ("kb8-pinhole", 20)])
def test_batch_equals_search_plus_restatement(built, cams, K):
    import orbfe
    ex = orbfe.ORBextractor(*ARGS)
    sc = NS.scene(2, K=max(K, 5), **CAMERAS[cams])
    nbs = sc["nbs"][-K:] if K < 5 else sc["nbs"]   # K == 1: a neighbour with a baseline
    raw, _, _, verdict = check_batch(ex, sc, nbs, 40 + K, "%s K=%d" % (cams, K))[:4]
    partners = int((raw >= 0).sum())
    assert partners >= 30 * K, partners
    assert (verdict[raw < 0] == R.NO_PARTNER).all() and (verdict[raw >= 0] != R.NO_PARTNER).all()
    if K == 20:
        assert len(set(verdict[raw >= 0].tolist())) >= 5, np.bincount(verdict[raw >= 0])
    ex.close()


@pytest.mark.parametrize("cams,K", [("pinhole", 20), ("kb8", 7)])
def test_whole_loop_equals_sequential_reference(built, cams, K):
    """CreateNewMapPoints' neighbour loop: K sequential oracle SearchForTriangulation calls, each followed by the restatement
    on ITS matches and has_mp1[idx1] = 1 for the accepted ones, against ONE batch call + orbfe_triangulation_select"""
    import orbfe
    ex = orbfe.ORBextractor(*ARGS)
    sc = NS.scene(3, K=K, **CAMERAS[cams])
    nbs = sc["nbs"]
    raw, rbin, x3d, verdict, has1, has2, coarse, cam_dicts = check_batch(ex, sc, nbs, 60 + K, "%s loop" % cams)
    want, has = [], has1.copy()
    rejected_at = {}
    revived = 0
    for k, nb in enumerate(nbs):
        off1, idx1, off2, idx2 = TB.csr(sc["node1"], nb["node"])
        n, m12 = O.search_for_triangulation(off1, idx1, off2, idx2, sc["kp1"], sc["desc1"], has, None, nb["kp"], nb["desc"], has2[k], None,
                                            sc["sf"], nb["F12"], nb["ep"], False, coarse[k], True, cameras=cam_dicts[k])
        i1 = np.flatnonzero(m12 >= 0)
        assert n == len(i1)
        v, x = R.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], i1, m12[i1])
        for p in range(len(i1)):
            if v[p] == R.ACCEPTED:
                want.append((k, int(i1[p]), int(m12[i1[p]]), x[p].tobytes()))
                has[i1[p]] = 1
                revived += int(i1[p]) in rejected_at
            else:
                rejected_at.setdefault(int(i1[p]), k)
    got, has = [], has1.copy()
    for k in range(K):
        n, m12 = orbfe.triangulation_select(raw[k], rbin[k], has, True)
        for i in np.flatnonzero(m12 >= 0):
            if verdict[k][i] == orbfe.NEWPT_ACCEPTED:
                got.append((k, int(i), int(m12[i]), x3d[k][i].tobytes()))
                has[i] = 1
    assert got == want, (len(got), len(want))
    assert len(want) >= (100 if K == 20 else 30), len(want)
    assert revived >= 1   # matched in an early neighbour, rejected there, accepted in a later one
    ex.close()


def test_edge_cases(built):
    import orbfe
    ex = orbfe.ORBextractor(*ARGS)
    other = orbfe.ORBextractor(*ARGS)
    sc = NS.scene(4, K=5)
    nbs = sc["nbs"]
    has1, has2, coarse, cams = search_inputs(sc, nbs, 9)
    kf1, kf2 = keyframes(ex, sc)
    tp = tri_params(nbs, coarse, cams)
    q = [np_params(nb["np"]) for nb in nbs]
    KP = orbfe.KP_DTYPE
    empty = orbfe.KeyFrame(ex, nbs[4]["kp"][:0].view(KP), nbs[4]["desc"][:0], nbs[4]["node"][:0], sc["sf"])
    apart = orbfe.KeyFrame(ex, nbs[4]["kp"].view(KP), nbs[4]["desc"], nbs[4]["node"] + 100000, sc["sf"])   # shares no node
    raw, rbin, x3d, verdict = orbfe.CreateNewMapPoints_batch(ex, kf1, has1, [empty, kf2[4], apart], [has2[4][:0], has2[4], has2[4]],
                                                             [tp[4]] * 3, [q[4]] * 3)
    for k in (0, 2):
        assert (raw[k] == -1).all() and (verdict[k] == orbfe.NEWPT_NO_PARTNER).all() and not x3d[k].any()
    i1 = np.flatnonzero(raw[1] >= 0)
    v, x = R.triangulate(nbs[4]["np"], sc["kp1"], nbs[4]["kp"], sc["sf"], sc["sf"], i1, raw[1][i1])
    assert len(i1) > 30 and np.array_equal(verdict[1][i1], v) and x3d[1][i1].tobytes() == x.tobytes()
    out = orbfe.CreateNewMapPoints_batch(ex, kf1, has1, [], [], [], [])   # K == 0
    assert out[0].shape[0] == 0 and out[3].shape[0] == 0
    nothing = orbfe.KeyFrame(ex, sc["kp1"][:0].view(KP), sc["desc1"][:0], sc["node1"][:0], sc["sf"])   # n1 == 0
    out = orbfe.CreateNewMapPoints_batch(ex, nothing, has1[:0], [kf2[4]], [has2[4]], [tp[4]], [q[4]])
    assert out[0].shape == (1, 0)
    # a key frame with stereo flags: the stereo branches are not built
    st = orbfe.KeyFrame(ex, nbs[4]["kp"].view(KP), nbs[4]["desc"], nbs[4]["node"], sc["sf"], np.zeros(len(nbs[4]["kp"]), np.uint8))
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.CreateNewMapPoints_batch(ex, kf1, has1, [st], [has2[4]], [tp[4]], [q[4]])
    assert e.value.code == orbfe.ERR_UNSUPPORTED
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.triangulate_pairs(ex, kf1, st, q[4], [0], [0])
    assert e.value.code == orbfe.ERR_UNSUPPORTED
    # key frames of another handle
    foreign = orbfe.KeyFrame(other, nbs[4]["kp"].view(KP), nbs[4]["desc"], nbs[4]["node"], sc["sf"])
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.CreateNewMapPoints_batch(ex, kf1, has1, [foreign], [has2[4]], [tp[4]], [q[4]])
    assert e.value.code == orbfe.ERR_INVALID_ARG
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.triangulate_pairs(ex, foreign, kf2[4], q[4], [0], [0])
    assert e.value.code == orbfe.ERR_INVALID_ARG
    # a parameter block of another layout
    short = np_params(nbs[4]["np"])
    short.struct_size -= 4
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.CreateNewMapPoints_batch(ex, kf1, has1, [kf2[4]], [has2[4]], [tp[4]], [short])
    assert e.value.code == orbfe.ERR_INVALID_ARG
    # the same call still works afterwards
    again = orbfe.CreateNewMapPoints_batch(ex, kf1, has1, [kf2[4]], [has2[4]], [tp[4]], [q[4]])
    assert again[0].tobytes() == raw[1].tobytes() and again[3].tobytes() == verdict[1].tobytes()
    ex.close()
    other.close()


def test_two_threads_on_two_handles(built):
    import orbfe
    scs = [NS.scene(5 + t, K=7) for t in range(2)]
    exs = [orbfe.ORBextractor(*ARGS) for _ in range(2)]
    outs, errs = [[], []], []

    def work(t, sink):
        sc = scs[t]
        has1, has2, coarse, cams = search_inputs(sc, sc["nbs"], 20 + t)
        kf1, kf2 = keyframes(exs[t], sc)
        tp = tri_params(sc["nbs"], coarse, cams)
        q = [np_params(nb["np"]) for nb in sc["nbs"]]
        for _ in range(20):
            r = orbfe.CreateNewMapPoints_batch(exs[t], kf1, has1, kf2, has2, tp, q)
            sink.append(tuple(a.tobytes() for a in r))

    def run(t):
        try:
            work(t, outs[t])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=240)
        assert not th.is_alive(), "a thread did not finish"
    assert not errs, errs
    for t in range(2):
        want = []
        work(t, want)
        assert outs[t] == want, "thread %d changed under concurrency" % t
    # and the first call of every thread against the restatement
    check_batch(exs[0], scs[0], scs[0]["nbs"], 20, "thread scene")
    for ex in exs:
        ex.close()


def test_gnss_operating_point(built):
    """the fork's GNSS node: ~10^4 keypoints per key frame, 6 levels, scale 1.2, 1228 x 921 (the geometry of
    test_operating_points_gpu), K = 5: same exact comparison"""
    import orbfe
    from test_operating_points_gpu import GEOMETRY
    a = GEOMETRY["GNSS"]["args"]
    W, H, levels, scale = a[6], a[7], a[3], a[2]
    assert (levels, W, H) == (6, 1228, 921) and abs(scale - 1.2) < 1e-6
    ex = orbfe.ORBextractor(*a)
    cam = np.array([750.0, 750.0, W / 2.0, H / 2.0, 0, 0, 0, 0])
    sc = NS.scene(8, K=10, n_points=10000, n_levels=levels, scale=scale, cam1=cam, height=H)
    nbs = sc["nbs"][4:9]   # baselines 0.3, 0.6 (turned away), 1, 1.5 (moved forward), 2.5
    raw, _, _, verdict = check_batch(ex, sc, nbs, 77, "GNSS")[:4]
    assert int((raw >= 0).sum()) > 2000 and int((verdict == R.ACCEPTED).sum()) > 300
    ex.close()

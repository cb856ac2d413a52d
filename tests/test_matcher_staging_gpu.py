"""Every host-pointer entry point that lays its call out with csrc/staging.h, on a handle of its own: a small shape, a large one, the
small one again.  The large shape is at least 8 x the small in every count, so with arenas that grow by 1.5 x both the device and the
pinned arena are replaced between the two small calls: a pointer kept across the growth, or a result read at a mirror offset that is
off by a block, changes the second small call's bytes.  Both small calls must give equal bytes and equal what the entry point's own
suite compares with (the C oracle or the restatement); where the call has one, a degenerate shape (M == 0, no groups, no sets, fewer
than two samples, no pairs, K == 0, an empty second frame) gives the documented defaults and leaves the bytes of a small call behind
it unchanged.  The IMU calls' layouts are a few fixed records, so their own large shape cannot outgrow 1.5 x: there the growth
between the two small calls comes from a large descriptor-set call on the same handle (test_imu_calls says so).
orbfe_mlpnp_ransac, orbfe_two_view_reconstruct and the two triangulation batch calls keep their hand-written layouts (their call times
moved in the A/B of profiles/r25_host_staging_ab.json); they run through the same check, which any later conversion then meets.
Small: <= 64 keypoints, 48 points, 2 groups / targets; large: ~700 keypoints, 600 points, 16 groups / targets."""
import numpy as np
import pytest

import frustum_scenarios as FS
import imu_preint_ref as IR
import imu_preint_scenarios as PS
import initial_ba_scenarios as BS
import local_map_scenarios as LS
import match_scenarios as S
import mlpnp_scenarios as MS
import newpoints_ref as NR
import newpoints_scenarios as NS
import oracle_py as O
import twoview_scenarios as TS
from test_frustum import ON, PN

pytestmark = pytest.mark.gpu

W, H = 752, 480
ARGS = (1000, 40000, 1.2, 8, 20, 7, W, H)
MP_NAMES_O = ("projX", "projY", "viewCos", "trackDepth", "level", "inView", "bad", "observations")
N_SMALL, N_LARGE, M_SMALL, M_LARGE, K_SMALL, K_LARGE = 64, 700, 48, 600, 2, 16


def blob(x):
    """every byte of a call's results, whatever their nesting"""
    if isinstance(x, dict):
        return b"".join(k.encode() + blob(x[k]) for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return b"".join(blob(v) for v in x)
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x).tobytes()
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if hasattr(x, "floats"):   # an ImuPreint record
        return x.floats().tobytes() + repr(x.n_steps).encode()
    return repr(x).encode()


def small_large_small(small, large, check, degenerate=None):
    """small() -> results; check(results) compares with the oracle; degenerate() runs and checks its own defaults"""
    a = small()
    check(a)
    got = large()
    assert got is not None
    b = small()
    assert blob(a) == blob(b), "the small call behind the large one gives other bytes"
    check(b)
    if degenerate:
        degenerate()
        assert blob(small()) == blob(a), "the small call behind the degenerate one gives other bytes"


def eq2(g, c):
    assert g[0] == c[0] and np.array_equal(g[1], c[1])


def eqp(g, c):
    assert np.array_equal(g[0], c[0]) and np.array_equal(g[1], c[1])


@pytest.fixture(scope="module")
def world(built):
    """two extracted frames of the synthetic stream, cut to the small and the large keypoint count (every octave stays present)"""
    import orbfe
    from orbfe import synth
    eo = O.Extractor(*ARGS)
    frames = list(synth.stream(W, H, 2))
    (kp, desc, _), (kpb, descb, _) = eo.extract(frames[0]), eo.extract(frames[1])
    assert len(kp) >= N_LARGE and len(kpb) >= N_LARGE
    sf = eo.scaleFactors
    Fo, Fp = O.Frustum(), orbfe.Frustum()
    v = FS.fill_frustum(Fo, ON, seed=3)
    FS.fill_frustum(Fp, PN, seed=3)

    def cut(k, d, n):
        idx = np.linspace(0, len(k) - 1, n).astype(int)
        return k[idx].copy(), d[idx].copy()

    w = dict(orbfe=orbfe, sf=sf, Fo=Fo, Fp=Fp, v=v)
    for name, n in (("s", N_SMALL), ("l", N_LARGE)):
        a, b = cut(kp, desc, n), cut(kpb, descb, n)
        w[name] = dict(kp=a[0], desc=a[1], kpb=b[0], descb=b[1], M=M_SMALL if name == "s" else M_LARGE, K=K_SMALL if name == "s" else K_LARGE,
                       fvo=O.make_frame_view(a[0], a[1], 64, 48, 0.0, 0.0, float(W), float(H), sf),
                       fvbo=O.make_frame_view(b[0], b[1], 64, 48, 0.0, 0.0, float(W), float(H), sf))
    return w


@pytest.fixture
def ex(built):
    """a handle of its own for every entry point: its arenas start empty"""
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


def views(orbfe, ex, z):
    fv = orbfe.make_frame_view(z["kp"], z["desc"], 64, 48, 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
    fvb = orbfe.make_frame_view(z["kpb"], z["descb"], 64, 48, 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
    return fv, fvb


def test_match_projection(world, ex):
    o, m = world["orbfe"], world["orbfe"].ORBmatcher(ex)

    def case(z, M=None):
        M = z["M"] if M is None else M
        mps, mpd, obs = S.projection_scenario(z["kp"], z["desc"], max(M, 1), 1, O.MP_DTYPE, MP_NAMES_O, 8)
        mps, mpd = mps[:M], mpd[:M]
        fv, _ = views(o, ex, z)
        return (lambda: m.SearchByProjection(fv, mps.view(o.MP_DTYPE), mpd, 20.0, False, 0.0, 0.85, obs),
                lambda g: eq2(g, O.search_by_projection(z["fvo"], mps, mpd, obs, 20.0, 0.85)))
    small, check = case(world["s"])
    none, _ = case(world["s"], 0)

    def degenerate():
        n, match = none()
        assert n == 0 and (match == -1).all() and len(match) == N_SMALL
    small_large_small(small, case(world["l"])[0], check, degenerate)


def test_match_bow(world, ex):
    m = world["orbfe"].ORBmatcher(ex)

    def case(z, nodes):
        c = S.bow_scenario(z["kp"], z["desc"], z["kpb"], z["descb"], nodes, 3)
        a = c[:4] + (z["desc"], z["kp"]["angle"], c[4], z["descb"], z["kpb"]["angle"], 0.75, True)
        return (lambda: m.SearchByBoW(*a)), (lambda g: eq2(g, O.search_by_bow(*a))), len(c[0]) - 1
    small, check, groups = case(world["s"], K_SMALL)
    assert 1 <= groups <= K_SMALL
    large, _, groups = case(world["l"], K_LARGE)
    assert groups == K_LARGE
    z = world["s"]
    empty = np.zeros(1, np.int32), np.zeros(0, np.int32)

    def degenerate():
        n, match = m.SearchByBoW(empty[0], empty[1], empty[0], empty[1], z["desc"], z["kp"]["angle"], np.ones(N_SMALL, np.uint8), z["descb"],
                                 z["kpb"]["angle"], 0.75, True)
        assert n == 0 and (match == -1).all() and len(match) == N_SMALL
    small_large_small(small, large, check, degenerate)


def test_match_initialization(world, ex):
    o, m = world["orbfe"], world["orbfe"].ORBmatcher(ex)

    def case(z):
        fv, fvb = views(o, ex, z)
        return (lambda: m.SearchForInitialization(fv, fvb, 100, 0.9, True)), (lambda g: eq2(g, O.search_for_initialization(z["fvo"], z["fvbo"], 100, 0.9, True)))
    small, check = case(world["s"])
    z = world["s"]
    fv, _ = views(o, ex, z)
    fv_empty = o.make_frame_view(z["kpb"][:0], z["descb"][:0], 64, 48, 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)

    def degenerate():   # an empty second frame: vnMatches12 all -1
        n, match = m.SearchForInitialization(fv, fv_empty, 100, 0.9, True)
        assert n == 0 and (match == -1).all() and len(match) == N_SMALL
    small_large_small(small, case(world["l"])[0], check, degenerate)


def fuse_case(world, z, M=None):
    import test_fuse
    M = z["M"] if M is None else M
    pts, mpd, _, inv_s2 = test_fuse.scenario(z["kp"], z["desc"], world["sf"], world["v"], max(M, 1), 1, False)
    return pts[:M], mpd[:M], inv_s2


def test_fuse_search_and_its_sim3_form(world, ex):
    o, m, Fo, Fp = world["orbfe"], world["orbfe"].ORBmatcher(ex), world["Fo"], world["Fp"]

    def case(z, M=None):
        pts, mpd, inv_s2 = fuse_case(world, z, M)
        fv, _ = views(o, ex, z)
        return (lambda: (m.Fuse_search(fv, inv_s2, None, Fp, 3.0, pts.view(o.WP_DTYPE), mpd), m.Fuse_search_sim3(fv, Fp, 4.0, pts.view(o.WP_DTYPE), mpd)),
                lambda g: (eqp(g[0], O.fuse_search(z["fvo"], inv_s2, None, Fo, 3.0, pts, mpd)), eqp(g[1], O.fuse_search_sim3(z["fvo"], Fo, 4.0, pts, mpd))))
    small, check = case(world["s"])
    none, _ = case(world["s"], 0)

    def degenerate():
        for idx, dist in none():
            assert len(idx) == 0 and len(dist) == 0
    small_large_small(small, case(world["l"])[0], check, degenerate)


def resident_targets(world, ex, z, K):
    """K resident key frames with a grid (the frame itself, then jittered copies), a map of the fuse scenario's points -> the calls' inputs"""
    o = world["orbfe"]
    pts, mpd, inv_s2 = fuse_case(world, z)
    rng = np.random.default_rng(9)
    kfs, fvos = [], []
    for k in range(K):
        kpk = z["kp"].copy()
        if k:
            kpk["x"] += rng.normal(0, 0.3, len(kpk)).astype(np.float32)
            kpk["y"] += rng.normal(0, 0.3, len(kpk)).astype(np.float32)
        kf = o.KeyFrame(ex, kpk.view(o.KP_DTYPE), z["desc"], np.full(len(kpk), -1, np.int32), ex.mvScaleFactor)
        kf.set_grid(64, 48, 0.0, 0.0, float(W), float(H), inv_s2, None)
        kfs.append(kf)
        fvos.append(O.make_frame_view(kpk, z["desc"], 64, 48, 0.0, 0.0, float(W), float(H), world["sf"]))
    mp = o.MapPoints(ex, len(pts))
    stored = pts.copy()
    stored["skip"] = 0
    mp.update(np.arange(len(pts)), stored.view(o.WP_DTYPE), mpd)
    ids = np.where(pts["skip"] != 0, ~np.arange(len(pts), dtype=np.int32), np.arange(len(pts), dtype=np.int32)).astype(np.int32)
    want = [O.fuse_search(f, inv_s2, None, world["Fo"], 3.0, pts, mpd) for f in fvos]
    return kfs, mp, ids, want


def test_fuse_search_keyframe_and_keyframes(world, ex):
    m, Fp = world["orbfe"].ORBmatcher(ex), world["Fp"]
    s_kfs, s_mp, s_ids, s_want = resident_targets(world, ex, world["s"], K_SMALL)
    l_kfs, l_mp, l_ids, _ = resident_targets(world, ex, world["l"], K_LARGE)

    def check_one(g):
        eqp(g, s_want[0])

    def none_one():
        idx, dist = m.Fuse_search_keyframe(s_kfs[0], s_mp, s_ids[:0], Fp, 3.0)
        assert len(idx) == 0 and len(dist) == 0
    small_large_small(lambda: m.Fuse_search_keyframe(s_kfs[0], s_mp, s_ids, Fp, 3.0), lambda: m.Fuse_search_keyframe(l_kfs[0], l_mp, l_ids, Fp, 3.0),
                      check_one, none_one)

    def check_all(g):
        for k in range(K_SMALL):
            eqp((g[0][k], g[1][k]), s_want[k])

    def none_targets():   # K == 0, then M == 0: nothing to write
        idx, dist = m.Fuse_search_keyframes([], s_mp, s_ids, [], 3.0)
        assert idx.shape == (0, len(s_ids)) and dist.shape == (0, len(s_ids))
        idx, dist = m.Fuse_search_keyframes(s_kfs, s_mp, s_ids[:0], [Fp] * K_SMALL, 3.0)
        assert idx.shape == (K_SMALL, 0) and dist.shape == (K_SMALL, 0)
    small_large_small(lambda: m.Fuse_search_keyframes(s_kfs, s_mp, s_ids, [Fp] * K_SMALL, 3.0)[:2],
                      lambda: m.Fuse_search_keyframes(l_kfs, l_mp, l_ids, [Fp] * K_LARGE, 3.0, cand_cap=4), check_all, none_targets)
    for x in s_kfs + l_kfs + [s_mp, l_mp]:
        x.close()


def test_match_triangulation(world, ex):
    import test_triangulation
    o, m = world["orbfe"], world["orbfe"].ORBmatcher(ex)

    def case(z):
        off1, idx1, off2, idx2, kp2, d2, h1, h2, s1, s2, F12, ep = test_triangulation.scenario(z["kp"], z["desc"], 2, True, False)
        off1, idx1, off2, idx2 = (np.asarray(x, np.int32) for x in (off1, idx1, off2, idx2))
        h1, h2 = h1.astype(np.uint8), h2.astype(np.uint8)
        return (lambda: m.SearchForTriangulation(off1, idx1, off2, idx2, z["kp"].view(o.KP_DTYPE), z["desc"], h1, s1, kp2.view(o.KP_DTYPE), d2, h2, s2,
                                                 ex.mvScaleFactor, F12, ep, False, False, True),
                lambda g: eq2(g, O.search_for_triangulation(off1, idx1, off2, idx2, z["kp"], z["desc"], h1, s1, kp2, d2, h2, s2, world["sf"], F12, ep,
                                                            False, False, True)),
                (kp2, d2, h1, h2, F12, ep))
    small, check, (kp2, d2, h1, h2, F12, ep) = case(world["s"])
    z, empty = world["s"], (np.zeros(1, np.int32), np.zeros(0, np.int32))

    def degenerate():
        n, match = m.SearchForTriangulation(empty[0], empty[1], empty[0], empty[1], z["kp"].view(o.KP_DTYPE), z["desc"], h1, None, kp2.view(o.KP_DTYPE), d2,
                                            h2, None, ex.mvScaleFactor, F12, ep, False, False, True)
        assert n == 0 and (match == -1).all() and len(match) == N_SMALL
    small_large_small(small, case(world["l"])[0], check, degenerate)


def newpoints_case(o, ex, K, n_points):
    import test_newpoints_gpu as TN
    sc = NS.scene(1, K=K, n_points=n_points)
    kf1, kf2 = TN.keyframes(ex, sc)
    has1, has2, coarse, cams = TN.search_inputs(sc, sc["nbs"], 4)
    tp = TN.tri_params(sc["nbs"], coarse, cams)
    npp = [TN.np_params(nb["np"]) for nb in sc["nbs"]]
    return sc, kf1, kf2, has1, has2, tp, npp


def test_triangulation_batch_new_points_and_pairs(world, ex):
    import test_newpoints_gpu as TN
    o = world["orbfe"]
    S_, L_ = newpoints_case(o, ex, K_SMALL, N_SMALL), newpoints_case(o, ex, K_LARGE, N_LARGE)

    def search(c):
        return lambda: o.SearchForTriangulation_batch(ex, c[1], c[3], c[2], c[4], c[5])

    def create(c):
        return lambda: o.CreateNewMapPoints_batch(ex, c[1], c[3], c[2], c[4], c[5], c[6])
    sc = S_[0]
    import test_triangulation_batch as TB
    coarse = TN.search_inputs(sc, sc["nbs"], 4)[2]

    def check_search(g):   # every neighbour's raw results through the host selection == the C oracle's SearchForTriangulation
        raw, rbin = g[0], g[1]
        for k, nb in enumerate(sc["nbs"]):
            c = [np.asarray(x, np.int32) for x in TB.csr(sc["node1"], nb["node"])]
            want = O.search_for_triangulation(*c, sc["kp1"], sc["desc1"], S_[3], None, nb["kp"], nb["desc"], S_[4][k], None, sc["sf"], nb["F12"],
                                              nb["ep"], False, coarse[k], True)
            eq2(o.triangulation_select(np.ascontiguousarray(raw[k]), np.ascontiguousarray(rbin[k]), S_[3], True), want)

    def none_neighbours():   # K == 0: nothing to write
        raw, rbin = o.SearchForTriangulation_batch(ex, S_[1], S_[3], [], [], [])
        assert raw.shape == (0, N_SMALL) and rbin.shape == (0, N_SMALL)
        assert all(a.shape[0] == 0 for a in o.CreateNewMapPoints_batch(ex, S_[1], S_[3], [], [], [], []))

    def check_create(g):
        raw, rbin, x3d, verdict = g
        check_search(g)
        for k, nb in enumerate(sc["nbs"]):
            want_v = np.full(len(sc["kp1"]), NR.NO_PARTNER, np.uint8)
            want_x = np.zeros((len(sc["kp1"]), 3), np.float32)
            i1 = np.flatnonzero(raw[k] >= 0)
            want_v[i1], want_x[i1] = NR.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], i1, raw[k][i1])
            TN.same(np.ascontiguousarray(x3d[k]), np.ascontiguousarray(verdict[k]), want_v, want_x, "neighbour %d" % k)
    small_large_small(create(S_), create(L_), check_create, none_neighbours)
    small_large_small(search(S_), search(L_), check_search, none_neighbours)

    def pairs(c, k=0):
        nb = c[0]["nbs"][k]
        return (lambda: o.triangulate_pairs(ex, c[1], c[2][k], TN.np_params(nb["np"]), nb["idx1"], nb["idx2"])), nb
    small, nb = pairs(S_)
    assert 1 <= len(nb["idx1"]) <= N_SMALL
    want_v, want_x = NR.triangulate(nb["np"], sc["kp1"], nb["kp"], sc["sf"], sc["sf"], nb["idx1"], nb["idx2"])

    def degenerate():
        gx, gv = o.triangulate_pairs(ex, S_[1], S_[2][0], TN.np_params(nb["np"]), [], [])
        assert len(gv) == 0 and gx.shape == (0, 3)
    small_large_small(small, pairs(L_)[0], lambda g: TN.same(g[0], g[1], want_v, want_x, "pairs"), degenerate)
    for c in (S_, L_):
        for kf in [c[1]] + c[2]:
            kf.close()


def test_search_by_sim3_and_relocalisation_projection(world, ex):
    import test_sim3_reloc as T3
    o, m, Fo, Fp, sf = world["orbfe"], world["orbfe"].ORBmatcher(ex), world["Fo"], world["Fp"], world["sf"]

    def sim3(z):
        sc = T3.sim3_scenario(z["kp"], z["desc"], sf, 1)
        d12o, d21o, d12, d21 = O.Sim3Dir(), O.Sim3Dir(), o.Sim3View(), o.Sim3View()
        sc["fill12"](d12o, T3.SN_O), sc["fill21"](d21o, T3.SN_O), sc["fill12"](d12, T3.SN_P), sc["fill21"](d21, T3.SN_P)
        fv2o = O.make_frame_view(sc["kp2"], sc["desc2"], 64, 48, 0.0, 0.0, float(W), float(H), sf)
        fv, _ = views(o, ex, z)
        fv2 = o.make_frame_view(sc["kp2"], sc["desc2"], 64, 48, 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
        return (lambda: m.SearchBySim3(fv, fv2, d12, d21, sc["mp1"].view(o.WP_DTYPE), sc["mpd1"], sc["mp2"].view(o.WP_DTYPE), sc["mpd2"], 7.5),
                lambda g: eq2(g, O.search_by_sim3(z["fvo"], fv2o, d12o, d21o, sc["mp1"], sc["mpd1"], sc["mp2"], sc["mpd2"], 7.5)))
    small, check = sim3(world["s"])
    z = world["s"]
    fv1, _ = views(o, ex, z)
    fv_empty = o.make_frame_view(z["kpb"][:0], z["descb"][:0], 64, 48, 0.0, 0.0, float(W), float(H), ex.mvScaleFactor)
    sc0 = T3.sim3_scenario(z["kp"], z["desc"], sf, 1)
    e12, e21 = o.Sim3View(), o.Sim3View()
    sc0["fill12"](e12, T3.SN_P), sc0["fill21"](e21, T3.SN_P)

    def no_second_keyframe():   # n2 == 0: no match
        n, match = m.SearchBySim3(fv1, fv_empty, e12, e21, sc0["mp1"].view(o.WP_DTYPE), sc0["mpd1"], sc0["mp2"][:0].view(o.WP_DTYPE), sc0["mpd2"][:0], 7.5)
        assert n == 0 and (match == -1).all() and len(match) == N_SMALL
    small_large_small(small, sim3(world["l"])[0], check, no_second_keyframe)   # the large call takes two table sets behind a layout that grew

    def reloc(z, M=None):
        M = z["M"] if M is None else M
        pts, mpd, ang, has = T3.reloc_scenario(z["kp"], z["desc"], sf, world["v"], max(M, 1), 2)
        pts, mpd, ang = pts[:M], mpd[:M], ang[:M]
        fv, _ = views(o, ex, z)
        return (lambda: m.SearchByProjection_keyframe(fv, Fp, pts.view(o.WP_DTYPE), mpd, ang, has, 12.0, True),
                lambda g: eq2(g, O.search_by_projection_kf(z["fvo"], Fo, pts, mpd, ang, has, 12.0, True)))
    small, check = reloc(world["s"])
    none, _ = reloc(world["s"], 0)

    def degenerate():
        n, match = none()
        assert n == 0 and (match == -1).all() and len(match) == N_SMALL
    small_large_small(small, reloc(world["l"])[0], check, degenerate)


def test_distinctive_descriptors(world, ex):
    import test_distinct
    m = world["orbfe"].ORBmatcher(ex)

    def case(seed, n_sets, hi):
        off, desc = test_distinct.make_sets(seed, [int(x) for x in np.random.default_rng(seed).integers(2, hi, n_sets)])
        return (lambda: m.ComputeDistinctiveDescriptors(off, desc)), (lambda g: eqp(g, O.distinctive_descriptors(off, desc)))
    small, check = case(3, K_SMALL, 24)
    large, _ = case(4, K_LARGE, 80)

    def degenerate():
        idx, med = m.ComputeDistinctiveDescriptors(np.zeros(1, np.int32), np.zeros((0, 32), np.uint8))
        assert len(idx) == 0 and len(med) == 0
    small_large_small(small, large, check, degenerate)


def test_mlpnp(world, ex):
    import test_mlpnp_gpu as T
    assert ex.mvLevelSigma2.tobytes() == MS.level_sigma2().tobytes()
    s, l_ = MS.make("general", M_SMALL, 0, 0.3, min_inliers=20), MS.make("general", M_LARGE, 0, 0.3)   # (50 inliers of 48 points: an abort)
    want = MS.ref(s)
    assert want["solved"] and len(s["sets"])
    small_large_small(lambda: T.call(ex, s), lambda: T.call(ex, l_), lambda g: T.same(g, want, "N = %d" % M_SMALL))


def test_two_view(world, ex):
    import test_twoview_gpu as T
    s, l_ = TS.make("general", M_SMALL, 0, 0.3, 8), TS.make("general", M_LARGE, 0, 0.3, 64)
    want = TS.ref(s)   # (48 matches end at the 50 triangulated points a reconstruction needs: both submissions ran, every field compared)
    assert want["n_hypotheses"] > 0
    small_large_small(lambda: T.call(ex, s), lambda: T.call(ex, l_), lambda g: T.same(g, want, "N = %d" % M_SMALL))


def test_initial_ba(world, ex):
    import test_initial_ba_gpu as T
    s, l_ = BS.make("general", M_SMALL, 0), BS.make("general", M_LARGE, 0)
    want = BS.ref(s)
    small_large_small(lambda: T.call(ex, s), lambda: T.call(ex, l_), lambda g: T.same(g, want, "N = %d" % M_SMALL))


@pytest.mark.parametrize("which", (IR.FROM_KEYFRAME, IR.FROM_FRAME), ids=("keyframe", "frame"))
def test_imu_calls(world, ex, which):
    import test_distinct
    import test_imu_preint_gpu as T
    o = world["orbfe"]
    m = o.ORBmatcher(ex)
    s, l_ = PS.make("moving", 4, 0), PS.make("moving", 40, 0)
    # The three layouts are a few 1200-byte records: 40 steps stay inside the 1.5 x the 4-step calls allocated, and the prediction has no
    # block that varies at all.  What replaces both arenas between the two small calls is the descriptor-set call of ~80 KB below, on
    # the same handle (its layout is 10 x the largest IMU layout on either side); the 40-step calls then run in the new arenas.
    off, desc = test_distinct.make_sets(4, [int(x) for x in np.random.default_rng(4).integers(120, 200, K_LARGE)])
    assert len(desc) * 32 > 10 * 5376

    def large():
        m.ComputeDistinctiveDescriptors(off, desc)
        return T.single(ex, l_, which)
    want = PS.ref_cached(("moving", 4, 0), which)

    def degenerate():   # fewer than two samples: nothing changes, the frame record is the empty one
        noise, _ = T.blocks(s, which)
        kf = o.ImuPreint(s["kf"].floats(), s["kf"].n_steps)
        frame, steps, n = o.imu_preintegrate_frame(ex, noise, T.samples_of(s)[:1], s["t_prev"], s["t_cur"], s["frame_bias"], kf)
        assert n == 0 and len(steps) == 0 and kf.floats().tobytes() == s["kf"].floats().tobytes() and bytes(frame) == bytes(o.ImuPreint())
    small_large_small(lambda: T.single(ex, s, which), large, lambda g: T.same_as_ref(g, want, "4 steps", which), degenerate)


def test_update_local_map_and_the_graph_setters(world, ex):
    """the graph goes up through the two staged setters, the frame through the host call: a small graph, a large one, the small one again"""
    import test_local_map_gpu as T
    o = world["orbfe"]
    small = dict(seed=1, n_kf=8, kf_stride=48, n_points=200, n_frames=2, n_voters=24, vote_stride=24, M=M_SMALL, window=60)
    large = dict(seed=2, n_kf=64, kf_stride=300, n_points=4000, n_frames=2, n_voters=200, vote_stride=256, M=M_LARGE, window=500)

    def run(cfg, f=0, votes=None):
        sc = LS.random_scene(**cfg)
        mp, cv = LS.upload(o, ex, sc)
        v, last = sc.frames[f]
        got = o.update_local_map(ex, o.LocalMapParams(**sc.params), v if votes is None else votes, last, cv, sc.M)
        cv.close()
        mp.close()
        return got, sc
    want = LS.random_scene(**small).ref(0)

    def degenerate():   # no voters: what the restatement gives for them
        got, sc = run(small, votes=np.zeros(0, np.int32))
        from local_map_ref import update_local_map
        T.same(got, update_local_map(sc.g, np.zeros(0, np.int32), sc.frames[0][1], sc.M, **sc.params), "no voters")
    small_large_small(lambda: run(small)[0], lambda: run(large)[0], lambda g: T.same(g, want, "small graph"), degenerate)

"""Parity at the two configurations the fork runs the front-end in, with content that fills their keypoint budgets:

  NODE  mono_inertial_node:       614 x 460 (2048 x 1536 x 0.3), nFeatures 10000 / nFast 16000, scale 2.0, 1 level,
                                  FAST 100 / 80, frame grid 64 x 48 -- per-frame capacity 10003
  GNSS  mono_inertial_gnss_node: 1228 x 921 (2048 x 1536 x 0.6), nFeatures 50000 / nFast 86000, scale 1.2, 6 levels,
                                  FAST 40 / 35, frame grid 512 x 512 -- per-frame capacity ~50000

Every chain the tracking and mapping threads call is compared bit for bit with the oracle at the live call parameters:
extraction, orbfe_track_frame (th 20 / nn 0.85 and 40 / 0.75), orbfe_track_initialization + orbfe_match_initialization
(40, 0.45, true), orbfe_track_reference_keyframe (nn 0.75, orientation on, levelsup 4), orbfe_match_triangulation_batch +
orbfe_triangulation_select (K = 5 neighbours) and Fuse at th = 10 (src/LocalMapping.cc:822,852).  Both capacities are
above the 7168 keypoints the BoW matcher keeps in LDS.  A module-scoped fixture per geometry holds the handle and the
oracle's extraction of the two frames (the chain helpers of the other test modules extract again inside, about a second
per GNSS frame); floors on keypoint, match and node counts keep the content from quietly turning a case trivial."""
import numpy as np
import pytest

import frustum_scenarios as FS
import oracle_py as O
import test_fuse as TF
import test_track_frame_gpu as TT
import test_track_initialization_gpu as TI
import test_track_reference_keyframe_gpu as TR
import test_triangulation_batch as TB
from test_frustum import ON, PN

pytestmark = pytest.mark.gpu

# args of ORBextractor, frame grid, and the keypoint floor of the content below (oracle: 10000 / 10000 keypoints for NODE,
# 50001 / 50003 for GNSS on the two frames)
GEOMETRY = {
    "NODE": dict(args=(10000, 16000, 2.0, 1, 100, 80, 614, 460), grid=(64, 48), kp_floor=9500),
    "GNSS": dict(args=(50000, 86000, 1.2, 6, 40, 35, 1228, 921), grid=(512, 512), kp_floor=40000),
}


def scene(name, count):
    """`count` frames of one scene translating by (3, 2) px per frame.  NODE: bright dots (150-255) on a period-4 lattice,
    85 % occupied, over a dark background (0-40) -- no dot lies on another's radius-3 FAST circle, so every dot is a
    full-contrast corner at threshold 100 and the 10000 features fill up.  GNSS: 2 x 2 blocks of black / white (fills all
    50000 features over 6 levels)."""
    a = GEOMETRY[name]["args"]
    W, H = a[6], a[7]
    rng = np.random.default_rng(2024 if name == "NODE" else 2025)
    pad = 16
    if name == "NODE":
        big = rng.integers(0, 41, (H + 2 * pad, W + 2 * pad)).astype(np.uint8)
        ys, xs = np.mgrid[0:H + 2 * pad:4, 0:W + 2 * pad:4]
        on = rng.random(ys.shape) < 0.85
        big[ys[on], xs[on]] = rng.integers(150, 256, int(on.sum()))
    else:
        cells = (rng.integers(0, 2, ((H + 2 * pad) // 2 + 1, (W + 2 * pad) // 2 + 1)) * 255).astype(np.uint8)
        big = np.repeat(np.repeat(cells, 2, 0), 2, 1)
    return [np.ascontiguousarray(big[pad + 2 * i:pad + 2 * i + H, 3 * i:3 * i + W]) for i in range(count)]


@pytest.fixture(scope="module", params=["NODE", "GNSS"])
def geo(request, built):
    """the oracle's extraction of frames 0 and 1 of the geometry's scene, one handle and its tracker; closed at teardown"""
    import orbfe
    g = dict(GEOMETRY[request.param], name=request.param)
    a = g["args"]
    g["W"], g["H"], g["levels"], g["scale"] = a[6], a[7], a[3], a[2]
    g["eo"] = O.Extractor(*a)
    g["frames"] = scene(request.param, 2)
    g["ref"] = [g["eo"].extract(img) for img in g["frames"]]
    assert min(len(kp) for kp, _, _ in g["ref"]) >= g["kp_floor"], [len(kp) for kp, _, _ in g["ref"]]
    g["ex"] = orbfe.ORBextractor(*a)
    assert g["ex"].cap > 7168  # the BoW matcher's LDS limit: every geometry here is above it
    g["trk"] = orbfe.FrameTracker(g["ex"], g["grid"][0], g["grid"][1], 0.0, 0.0, float(g["W"]), float(g["H"]))
    yield g
    g["ex"].close()


def frusta(g, seed):
    """camera of the geometry: its image size, levels and scale, the principal point at the image centre"""
    import orbfe
    Fo, Fp = O.Frustum(), orbfe.Frustum()
    kw = dict(W=float(g["W"]), H=float(g["H"]), n_levels=g["levels"], scale=g["scale"], seed=seed, cx=g["W"] / 2.0, cy=g["H"] / 2.0)
    v = FS.fill_frustum(Fo, ON, **kw)
    FS.fill_frustum(Fp, PN, **kw)
    return Fo, Fp, v


def frame_view_o(g, kp, desc):
    return O.make_frame_view(kp, desc, g["grid"][0], g["grid"][1], 0.0, 0.0, float(g["W"]), float(g["H"]), g["eo"].scaleFactors)


def frame_view_p(g, kp, desc):
    import orbfe
    return orbfe.make_frame_view(kp, desc, g["grid"][0], g["grid"][1], 0.0, 0.0, float(g["W"]), float(g["H"]), g["ex"].mvScaleFactor)


def test_extraction(geo):
    """(a) both frames: keypoints, descriptors; GNSS at its real 1228 x 921"""
    for i, (img, (kp_r, desc_r, _)) in enumerate(zip(geo["frames"], geo["ref"])):
        kp, desc = geo["ex"].extractFeatures(img)
        assert len(kp) == len(kp_r), "frame %d: keypoint count %d vs %d" % (i, len(kp), len(kp_r))
        assert kp.tobytes() == kp_r.tobytes(), "frame %d: keypoints" % i
        assert np.array_equal(desc, desc_r), "frame %d: descriptors" % i


@pytest.mark.parametrize("th,nn", [(20.0, 0.85), (40.0, 0.75)])
def test_track_frame(geo, th, nn):
    """(b) orbfe_track_frame with a local map of M = 10000 points on frame 1's keypoints; with (20, 0.85) also == the three
    calls orbfe_extract + orbfe_project_map_points + orbfe_match_projection on the same handle"""
    import orbfe
    img = geo["frames"][1]
    kp_r, desc_r, _ = geo["ref"][1]
    Fo, Fp, v = frusta(geo, 31)
    pts, mpd = FS.world_points_on_keypoints(kp_r, desc_r, v, 10000, np.random.default_rng(7), geo["levels"])
    ref = TT.oracle_chain(geo["eo"], img, Fo, pts, mpd, th, nn, grid=geo["grid"])
    got = geo["trk"].TrackFrame(img, Fp, pts.view(orbfe.WP_DTYPE), mpd, th, nn)
    TT.same(got, ref, "%s (%g, %g)" % (geo["name"], th, nn))
    assert ref["n"] > 5000, ref["n"]
    if th == 20.0:
        m = orbfe.ORBmatcher(geo["ex"])
        kp0, desc0 = geo["ex"].extractFeatures(img)
        mps, xr = m.isInFrustum_batch(Fp, pts.view(orbfe.WP_DTYPE))
        n3, match3 = m.SearchByProjection(frame_view_p(geo, kp0, desc0), mps, mpd, th, False, 0.0, nn, None)
        assert got["kp"].tobytes() == kp0.tobytes() and np.array_equal(got["desc"], desc0)
        assert got["mps"].tobytes() == mps.tobytes() and got["proj_xr"].tobytes() == xr.tobytes()
        assert got["nmatches"] == n3 and np.array_equal(got["match"], match3)


def test_track_initialization(geo):
    """(c) orbfe_track_initialization of frame 1 against frame 0 resident as the initial frame, and orbfe_match_initialization
    on the oracle's two frames, at (40, 0.45, true) -- every keypoint of NODE is on level 0"""
    import orbfe
    kp0, d0, _ = geo["ref"][0]
    kp1, d1, _ = geo["ref"][1]
    eo = geo["eo"]
    ref = TI.oracle_chain(eo, kp0, d0, geo["frames"][1], geo["grid"], 40, 0.45, True)
    ini = orbfe.InitialFrame(geo["ex"], kp0.view(orbfe.KP_DTYPE), d0)
    got = geo["trk"].TrackInitialization(geo["frames"][1], ini, 40, 0.45, True)
    ini.close()
    TI.same(got, ref, geo["name"])
    m = orbfe.ORBmatcher(geo["ex"])
    n, m12 = m.SearchForInitialization(frame_view_p(geo, kp0.view(orbfe.KP_DTYPE), d0), frame_view_p(geo, kp1.view(orbfe.KP_DTYPE), d1),
                                       40, 0.45, True)
    assert n == ref["n"] and np.array_equal(m12, ref["m12"])
    assert ref["n"] > 5000, ref["n"]


def _track_reference_keyframe(geo, k, L, levelsup, min_matches):
    import orbfe
    eo, ex = geo["eo"], geo["ex"]
    t = TR.tree_for_images(k, L, seed=3 * k + L)
    voc = orbfe.ORBVocabulary(ex, t["childOff"], t["childIdx"], t["nodeDesc"], t["wordId"], t["weight"], L)
    kf = TR.make_kf(eo, t, levelsup, geo["frames"][0])
    res = orbfe.KeyFrame(ex, kf["kp"].view(orbfe.KP_DTYPE), kf["desc"], kf["node"], eo.scaleFactors)
    has = (np.random.default_rng(k + L).random(len(kf["kp"])) < 0.7).astype(np.uint8)
    img = geo["frames"][1]
    got = geo["trk"].TrackReferenceKeyFrame(img, voc, levelsup, res, has, 0.75, True)
    ref = TR.oracle_chain(eo, t, levelsup, img, kf, has, 0.75, True)
    TR.same(got, ref, "%s k=%d L=%d levelsup=%d" % (geo["name"], k, L, levelsup))
    assert ref["n"] > min_matches, ref["n"]
    # == orbfe_extract -> orbfe_bow_transform -> orbfe_match_bow on the same handle
    m = orbfe.ORBmatcher(ex)
    kp0, desc0 = ex.extractFeatures(img)
    w0, n0, wt0 = voc.transform(desc0, levelsup)
    kfOff, kfIdx, fOff, fIdx = TR.csr(kf["node"], np.where(wt0 > 0, n0, -1))
    n3, match3 = m.SearchByBoW(kfOff, kfIdx, fOff, fIdx, kf["desc"], kf["kp"]["angle"], has, desc0, kp0["angle"], 0.75, True)
    assert np.array_equal(got["word"], w0) and np.array_equal(got["node"], n0)
    assert got["nmatches"] == n3 and np.array_equal(got["match"], match3)
    res.close()
    voc.close()
    return len(set(kf["node"].tolist()) - {-1})


def test_track_reference_keyframe(geo):
    """(d) orbfe_track_reference_keyframe against frame 0 as the resident key frame: the vocabulary of INTEGRATION.md
    (k = 10, L = 6, levelsup 4).  The per-frame capacity is above 7168, where the matcher refused before."""
    nodes = _track_reference_keyframe(geo, 10, 6, 4, 3000)
    assert nodes > 50, nodes


@pytest.mark.parametrize("geo", ["NODE"], indirect=True)
def test_track_reference_keyframe_one_node(geo):
    """(d) NODE with a degenerate vocabulary position (levelsup >= L): one node holds the whole frame"""
    assert _track_reference_keyframe(geo, 6, 4, 4, 3000) == 1


def fine_nodes(kp):
    """vocabulary nodes of 8 x 8 px cells: far more distinct nodes than the 4096 the triangulation kernel stages in LDS"""
    return ((kp["y"] // 8).astype(np.int32) * 1024 + (kp["x"] // 8).astype(np.int32)).astype(np.int32)


def _triangulation(geo, K, nodes_fn, stereo, seed):
    """frame 0 as key frame 1 against K neighbours: one orbfe_match_triangulation_batch launch + orbfe_triangulation_select in
    neighbour order == K sequential oracle calls (TB.sequential_reference); returns (total matches, distinct nodes of
    every neighbour)"""
    import orbfe
    kp, desc, _ = geo["ref"][0]
    ex = geo["ex"]
    rng = np.random.default_rng(seed)
    node1 = nodes_fn(kp)
    node1[rng.random(len(kp)) < 0.03] = -1
    has1 = (rng.random(len(kp)) < 0.3).astype(np.uint8)
    s1 = (rng.random(len(kp)) < 0.4).astype(np.uint8) if stereo else None
    nbs = [TB.neighbour(kp, desc, seed + k, consistent=(k % 4 != 3), stereo=stereo, width=geo["W"], cx=geo["W"] / 2.0,
                        cy=geo["H"] / 2.0, nodes=node1) for k in range(K)]
    ref = TB.sequential_reference(kp, desc, node1, has1, s1, nbs, geo["eo"].scaleFactors, False, False, True, seed)
    kf1 = orbfe.KeyFrame(ex, kp.view(orbfe.KP_DTYPE), desc, node1, ex.mvScaleFactor, s1)
    kf2 = [orbfe.KeyFrame(ex, nb["kp"].view(orbfe.KP_DTYPE), nb["desc"], nb["node"], ex.mvScaleFactor, nb["stereo"]) for nb in nbs]
    params = [orbfe.tri_params(nb["F12"], nb["ep"], False, False, True) for nb in nbs]
    raw, rbin = orbfe.SearchForTriangulation_batch(ex, kf1, has1, kf2, [nb["has"] for nb in nbs], params)
    coins = np.random.default_rng(seed)  # the coins of sequential_reference
    has = has1.copy()
    total = 0
    for k in range(K):
        n, m12 = orbfe.triangulation_select(raw[k], rbin[k], has, True)
        assert n == ref[k][0] and np.array_equal(m12, ref[k][1]), "%s neighbour %d: %d vs %d matches" % (geo["name"], k, n, ref[k][0])
        new = np.flatnonzero(m12 >= 0)
        new = new[coins.random(len(new)) < 0.7]
        has[new] = 1
        total += n
    for kf in [kf1] + kf2:
        kf.close()
    return total, [len(set(nb["node"].tolist()) - {-1}) for nb in nbs]


@pytest.mark.parametrize("stereo", [False, True])
def test_triangulation_batch(geo, stereo):
    """(e) SearchForTriangulation of one key frame against K = 5 neighbours (nodes of 40-px rows and the octave)"""
    total, _ = _triangulation(geo, 5, TB.nodes_of, stereo, 700 + int(stereo))
    assert total > 5000, total  # oracle: 7039 / 6934 (NODE), 34647 / 34789 (GNSS)


@pytest.mark.parametrize("geo", ["GNSS"], indirect=True)
def test_triangulation_batch_many_nodes(geo):
    """(e) neighbours of more than kTriNodeLds = 4096 distinct nodes: the node search of the triangulation kernel reads the
    neighbour's node list from global memory (kernels_match_tri.hip, nodesInLds false)"""
    total, nodes = _triangulation(geo, 5, fine_nodes, False, 800)
    assert min(nodes) > 4096, nodes  # oracle: ~20000 per neighbour
    assert total > 20000, total  # oracle: 34537


@pytest.mark.parametrize("stereo", [False, True])
def test_fuse_th10(geo, stereo):
    """(f) the search part of Fuse at th = 10 (src/LocalMapping.cc:822,852) with M = 10000 map points: the resident entry
    point orbfe_fuse_search_keyframe == the host one orbfe_fuse_search == O.fuse_search"""
    import orbfe
    import test_fuse_keyframe_gpu as TK
    kp, desc, _ = geo["ref"][0]
    eo, ex = geo["eo"], geo["ex"]
    Fo, Fp, v = frusta(geo, 41 + int(stereo))
    M = 10000
    pts, mpd, u_right, inv_s2 = TF.scenario(kp, desc, eo.scaleFactors, v, M, 9 + int(stereo), stereo)
    bi_r, bd_r = O.fuse_search(frame_view_o(geo, kp, desc), inv_s2, u_right, Fo, 10.0, pts, mpd)
    kf = orbfe.KeyFrame(ex, kp.view(orbfe.KP_DTYPE), desc, np.full(len(kp), -1, np.int32), eo.scaleFactors)
    kf.set_grid(geo["grid"][0], geo["grid"][1], 0.0, 0.0, float(geo["W"]), float(geo["H"]), inv_s2, u_right)
    mp = orbfe.MapPoints(ex, M)
    stored = pts.copy()
    stored["skip"] = 0
    mp.update(np.arange(M), stored.view(orbfe.WP_DTYPE), mpd)
    m = orbfe.ORBmatcher(ex)
    bi, bd = m.Fuse_search_keyframe(kf, mp, TK.ids_of(pts), Fp, 10.0)
    assert np.array_equal(bd, bd_r) and np.array_equal(bi, bi_r)
    bi_h, bd_h = m.Fuse_search(frame_view_p(geo, kp.view(orbfe.KP_DTYPE), desc), inv_s2, u_right, Fp, 10.0, pts.view(orbfe.WP_DTYPE), mpd)
    assert np.array_equal(bi_h, bi_r) and np.array_equal(bd_h, bd_r)
    assert (bd_r <= orbfe.ORBmatcher.TH_LOW).sum() > M // 4
    kf.close()
    mp.close()

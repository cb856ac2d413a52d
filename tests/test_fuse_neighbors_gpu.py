"""orbfe_fuse_search_keyframes: the Fuse searches of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:819-824) into all K
targets in ONE submission, with the gated candidates of every pair in visit order, and orbfe_fuse_select, the host scan over such a
list.  Bit-exact throughout: every row equals orbfe_fuse_search_keyframe on the same inputs AND the oracle's fuse_search; the
candidate lists reproduce the best candidate under the point's own and under replacement descriptors; the full replay of the loop
(tests/neighbors_model.py with the library as the searcher: one batch call, host selects, fallbacks) equals K sequential oracle
searches with the graph edits between them."""
import ctypes as C
import threading

import numpy as np
import pytest

import frustum_scenarios as FS
import match_scenarios as S
import neighbors_model as NM
import oracle_py as O
import test_fuse as TF
from test_frustum import ON, PN

pytestmark = pytest.mark.gpu

W, H, ARGS = TF.W, TF.H, TF.ARGS
M_MAX, BASE = 2000, 7


@pytest.fixture(scope="module")
def world(built):
    """K = 20 neighbours built like test_search_in_neighbors_sequence (every fourth stereo) plus: a KannalaBrandt8 target, a target
    with another grid (32 x 20), an empty key frame, and neighbour 2 a second time.  One resident map of M_MAX points at BASE."""
    import orbfe
    from orbfe import synth
    eo = O.Extractor(*ARGS)
    ex = orbfe.ORBextractor(*ARGS)
    kp0, desc0, _ = eo.extract(synth.frame(W, H, 90))
    rng = np.random.default_rng(5)
    Fo0 = O.Frustum()
    v0 = FS.fill_frustum(Fo0, ON, seed=60)
    pts, mpd, _, _ = TF.scenario(kp0, desc0, eo.scaleFactors, v0, M_MAX, 3, False)
    inv_s2 = (1.0 / (eo.scaleFactors.astype(np.float32) ** 2)).astype(np.float32)
    sf = eo.scaleFactors
    targets = []

    def add(kpk, desck, ur, grid=(64, 48), kb8=False, kf=None):
        Fo, Fp = O.Frustum(), orbfe.Frustum()
        FS.fill_frustum(Fo, ON, seed=60, kb8=kb8)
        FS.fill_frustum(Fp, PN, seed=60, kb8=kb8)
        if kf is None:
            kf = orbfe.KeyFrame(ex, kpk.view(orbfe.KP_DTYPE), desck, np.full(len(kpk), -1, np.int32), sf)
            kf.set_grid(grid[0], grid[1], 0.0, 0.0, float(W), float(H), inv_s2, ur)
        fvo = O.make_frame_view(kpk, desck, grid[0], grid[1], 0.0, 0.0, float(W), float(H), sf) if len(kpk) else None
        targets.append(dict(kp=kpk, desc=desck, ur=ur, Fo=Fo, Fp=Fp, kf=kf, fvo=fvo, grid=grid, kb8=kb8))

    def view(k):
        perm = rng.permutation(len(kp0))[:len(kp0) - 10 * k]
        kpk = kp0[perm].copy()
        kpk["x"] += rng.normal(0, 0.3, len(kpk)).astype(np.float32)
        kpk["y"] += rng.normal(0, 0.3, len(kpk)).astype(np.float32)
        desck = np.stack([S.flip_bits(desc0[i], int(rng.integers(0, 12)), rng) for i in perm])
        ur = None
        if k % 4 == 1:
            ur = np.where(rng.random(len(kpk)) < 0.5, kpk["x"] - rng.uniform(2, 30, len(kpk)), -1.0).astype(np.float32)
        return kpk, desck, ur

    for k in range(20):
        add(*view(k))
    add(*view(3)[:2], None, kb8=True)
    add(*view(6)[:2], None, grid=(32, 20))
    add(kp0[:0].copy(), desc0[:0].copy(), None)
    t2 = targets[2]
    add(t2["kp"], t2["desc"], t2["ur"], kf=t2["kf"])  # the same key frame twice
    mp = orbfe.MapPoints(ex, BASE + M_MAX + 50)
    stored = pts.copy()
    stored["skip"] = 0
    mp.update(np.arange(BASE, BASE + M_MAX), stored.view(orbfe.WP_DTYPE), mpd)
    w = dict(orbfe=orbfe, ex=ex, eo=eo, m=orbfe.ORBmatcher(ex), pts=pts, mpd=mpd, inv_s2=inv_s2, targets=targets, mp=mp, sf=sf)
    yield w
    mp.close()
    for t in targets[:23]:
        t["kf"].close()


def make_ids(w, M, seed):
    """ids of a call: entry BASE + i; ~id where the scenario's own skip flag is set; from M >= 63 on also an unwritten entry, an id
    beyond the map and the complement of one.  -> (ids, none): none[i] = the id names no point"""
    rng = np.random.default_rng(seed)
    ids = np.arange(BASE, BASE + M, dtype=np.int32)
    ids = np.where(w["pts"]["skip"][:M] != 0, ~ids, ids).astype(np.int32)
    none = np.zeros(M, bool)
    if M >= 63:
        odd = rng.choice(M, 3, replace=False)
        ids[odd[0]] = 3
        ids[odd[1]] = w["mp"].capacity + 1000
        ids[odd[2]] = ~(w["mp"].capacity + 1000)
        none[odd] = True
    return ids, none


def oracle_row(w, t, th, M, skipped, mpd=None):
    if t["fvo"] is None:
        return np.full(M, -1, np.int32), np.full(M, 256, np.int32)
    call = w["pts"][:M].copy()
    call["skip"] = skipped
    return O.fuse_search(t["fvo"], w["inv_s2"], t["ur"], t["Fo"], th, call, (w["mpd"] if mpd is None else mpd)[:M])


def batch(w, ids, th, skip=None, cand_cap=0, targets=None):
    ts = w["targets"] if targets is None else targets
    return w["m"].Fuse_search_keyframes([t["kf"] for t in ts], w["mp"], ids, [t["Fp"] for t in ts], th, skip=skip, cand_cap=cand_cap)


@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("th", [3.0, 10.0])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 2000])
def test_rows_equal_single_call_and_oracle(world, M, th, with_skip):
    w = world
    K = len(w["targets"])
    ids, none = make_ids(w, M, M)
    skip = (np.random.default_rng(M + 1).random((K, M)) < 0.2).astype(np.uint8) if with_skip else None
    bi, bd, ci, cc = batch(w, ids, th, skip, cand_cap=4)
    bi0, bd0 = batch(w, ids, th, skip, cand_cap=0)
    assert bi.shape == (K, M) and ci.shape == (K, M, 4) and cc.shape == (K, M)
    assert np.array_equal(bi, bi0) and np.array_equal(bd, bd0)
    fused = 0
    for k, t in enumerate(w["targets"]):
        row_skip = (ids < 0) | none | (skip[k] != 0 if with_skip else False)
        ids_k = np.where((skip[k] != 0) & (ids >= 0), ~ids, ids).astype(np.int32) if with_skip else ids
        bi_s, bd_s = w["m"].Fuse_search_keyframe(t["kf"], w["mp"], ids_k, t["Fp"], th)
        bi_r, bd_r = oracle_row(w, t, th, M, row_skip)
        assert np.array_equal(bi[k], bi_s) and np.array_equal(bd[k], bd_s), "target %d differs from the single call" % k
        assert np.array_equal(bi[k], bi_r) and np.array_equal(bd[k], bd_r), "target %d differs from the oracle" % k
        assert (cc[k][row_skip] == 0).all() and (ci[k][row_skip] == -1).all()
        fused += int((bd_r <= 50).sum())
    if not with_skip:  # the same key frame twice (with skip flags the two rows have flags of their own)
        assert np.array_equal(bi[23], bi[2]) and np.array_equal(ci[23], ci[2])
    assert (bi[22] == -1).all() and (bd[22] == 256).all() and (cc[22] == 0).all()  # the empty key frame
    if M == 2000:
        assert fused > 8000
        assert int((bd[20] <= 50).sum()) > 100 and int((bd[21] <= 50).sum()) > 100  # KannalaBrandt8, the 32 x 20 grid


def visit_key(t, idx):
    """(cell x, cell y, index): the order in which GetFeaturesInArea returns features (src/KeyFrame.cc:814-830)"""
    f32 = np.float32
    cols, rows = t["grid"]
    invw, invh = f32(cols) / f32(W), f32(rows) / f32(H)
    k = t["kp"][idx]
    return int(np.round(f32(k["x"] * invw))), int(np.round(f32(k["y"] * invh))), int(idx)


def test_candidate_lists(world):
    w = world
    orbfe = w["orbfe"]
    th, M = 10.0, M_MAX
    K = len(w["targets"])
    ids, none = make_ids(w, M, 11)
    bi, bd, ci, cc = batch(w, ids, th, None, cand_cap=16)
    unskipped = ~((ids < 0) | none)
    live = unskipped & (w["pts"]["bad"][:M] == 0)
    assert cc.max() <= 16, "a pair with more than 16 gated candidates: %d" % cc.max()
    print("gated candidates per pair (count: pairs):", dict(zip(*np.unique(cc[:, live], return_counts=True))))
    # cand_count == 0 <=> nothing qualified
    assert np.array_equal(cc[:, unskipped] == 0, (bi[:, unskipped] == -1) & (bd[:, unskipped] == 256))
    assert ((ci >= 0).sum(axis=2) == np.minimum(cc, 16)).all()
    # the lists are in visit order, across the two levels a pair walks
    checked = 0
    for k, i in np.argwhere(cc >= 2)[::7]:
        keys = [visit_key(w["targets"][k], j) for j in ci[k, i, :cc[k, i]]]
        assert keys == sorted(keys), (k, i, keys)
        checked += 1
    assert checked >= 50
    # the select with the point's own descriptor reproduces the row
    for k in (0, 1, 5, 20, 21, 23):
        t = w["targets"][k]
        for i in np.flatnonzero(cc[k] > 0):
            assert orbfe.fuse_select(ci[k, i], cc[k, i], 16, t["desc"], w["mpd"][i]) == (bi[k, i], bd[k, i]), (k, i)
    # cand_cap = 4 and 1: the same counts (the TRUE count), the same leading entries, truncation reported
    for cap in (4, 1):
        bi_c, bd_c, ci_c, cc_c = batch(w, ids, th, None, cand_cap=cap)
        assert np.array_equal(bi_c, bi) and np.array_equal(bd_c, bd) and np.array_equal(cc_c, cc)
        assert np.array_equal(ci_c, ci[:, :, :cap])
    trunc = np.argwhere(cc >= 2)
    assert len(trunc) >= 50, len(trunc)
    for k, i in trunc[::9]:
        with pytest.raises(orbfe.OrbfeError) as e:
            orbfe.fuse_select(ci_c[k, i], cc_c[k, i], 1, w["targets"][k]["desc"], w["mpd"][i])
        assert e.value.code == orbfe.ERR_UNSUPPORTED
    # 8 replacement descriptors, written into the map: the select on the OLD lists (cand_cap = 4) equals the oracle's search with
    # the new descriptor for every pair whose list is not truncated -- and the device agrees once the map holds the new bytes
    bi4, bd4, ci4, cc4 = batch(w, ids, th, None, cand_cap=4)
    rng = np.random.default_rng(17)
    rep = rng.choice(np.flatnonzero(live & (cc[:20] > 0).sum(axis=0).astype(bool)), 8, replace=False)
    mpd_new = w["mpd"].copy()
    for i in rep:
        k = int(np.flatnonzero(cc[:, i] > 0)[0])
        mpd_new[i] = S.flip_bits(w["targets"][k]["desc"][ci[k, i, cc[k, i] - 1]], int(rng.integers(0, 30)), rng)
    stored = w["pts"][rep].copy()
    stored["skip"] = 0
    w["mp"].update(BASE + rep, stored.view(orbfe.WP_DTYPE), mpd_new[rep])
    try:
        bi_n, bd_n = batch(w, ids, th, None)
        compared = changed = 0
        for k, t in enumerate(w["targets"]):
            bi_r, bd_r = oracle_row(w, t, th, M, ~unskipped, mpd_new)
            assert np.array_equal(bi_n[k], bi_r) and np.array_equal(bd_n[k], bd_r)
            for i in rep:
                if cc4[k, i] > 4:
                    continue
                got = (-1, 256) if t["fvo"] is None else orbfe.fuse_select(ci4[k, i], cc4[k, i], 4, t["desc"], mpd_new[i])
                assert got == (bi_r[i], bd_r[i]), (k, i)
                compared += 1
                changed += got != (bi4[k, i], bd4[k, i])
        assert compared >= 8 * (K - 1) * 0.9 and changed >= 20
    finally:
        stored = w["pts"][rep].copy()
        stored["skip"] = 0
        w["mp"].update(BASE + rep, stored.view(orbfe.WP_DTYPE), w["mpd"][rep])


@pytest.mark.parametrize("scene,cap", [("default", 4), ("sparse", 4), ("default", 1)])
def test_full_replay_with_the_library(built, scene, cap):
    """The model of tests/neighbors_model.py with the library as the searcher: ONE orbfe_fuse_search_keyframes (cand_cap = 4) on the
    start-of-loop state, orbfe_fuse_select for the dirty points, one orbfe_fuse_search_keyframe per target for the dirty points whose
    list is truncated -- against the K sequential oracle searches.  Floors as in tests/test_neighbors_model.py.  cand_cap = 4 is
    a condition here (at most 1 % of the dirty selects may need the fallback); counted on MI355X: no pair of either scene has more
    than 4 gated candidates (default: 4694 selects, sparse: 24 selects, 0 fallbacks, 1 submission each).  The third case runs
    the default scene with cand_cap = 1, where the fallback searches really happen."""
    import orbfe
    K, M, th = 20, 1200, 10.0
    sc = NM.scene(seed=5, K=K, M=M)
    kw = NM.SCENES[scene]
    seq, final_seq, st = NM.sequential(sc, th, **kw)
    ex = orbfe.ORBextractor(*ARGS)
    m = orbfe.ORBmatcher(ex)
    Fp = orbfe.Frustum()
    FS.fill_frustum(Fp, PN, seed=60)
    kfs = []
    for nb in sc["nbs"]:
        kf = orbfe.KeyFrame(ex, nb["kp"].view(orbfe.KP_DTYPE), nb["desc"], np.full(len(nb["kp"]), -1, np.int32), sc["eo"].scaleFactors)
        kf.set_grid(64, 48, 0.0, 0.0, float(W), float(H), sc["inv_s2"], None)
        kfs.append(kf)
    mp = orbfe.MapPoints(ex, M)
    ids = np.arange(M, dtype=np.int32)
    box = dict(submissions=0, selects=0, fallback_selects=0, fallback_targets=0)

    def push(mps, sel):
        pts = sc["pts"][sel].copy()
        pts["bad"] = [mps[i].bad for i in sel]
        mp.update(ids[sel], pts.view(orbfe.WP_DTYPE), np.stack([mps[i].desc for i in sel]))

    def search_all(mps):
        push(mps, ids)
        skip = np.array([[k in p.kfs for p in mps] for k in range(K)], np.uint8)
        bi, bd, box["ci"], box["cc"] = m.Fuse_search_keyframes(kfs, mp, ids, [Fp] * K, th, skip=skip, cand_cap=cap)
        box["submissions"] += 1
        return [(bi[k], bd[k]) for k in range(K)]

    def resolve(k, dirty, mps):
        a, b = np.zeros(len(dirty), np.int32), np.zeros(len(dirty), np.int32)
        over = []
        for j, i in enumerate(dirty):
            box["selects"] += 1
            if box["cc"][k, i] > cap:
                over.append(j)
                continue
            a[j], b[j] = orbfe.fuse_select(box["ci"][k, i], box["cc"][k, i], cap, sc["nbs"][k]["desc"], mps[i].desc)
        if over:  # truncated lists: one single call for just those points, after the map holds their bytes of now
            sel = dirty[over]
            push(mps, sel)
            a[over], b[over] = m.Fuse_search_keyframe(kfs[k], mp, ids[sel], Fp, th)
            box["submissions"] += 1
            box["fallback_targets"] += 1
            box["fallback_selects"] += len(over)
        return a, b

    used, final_rep, st2, cnt = NM.replay(sc, th, search_all, resolve, **kw)
    print(scene, st2, cnt, {k: v for k, v in box.items() if k not in ("ci", "cc")}, "pairs above the cap:", int((box["cc"] > cap).sum()),
          "max count:", int(box["cc"].max()))
    for k in range(K):
        assert np.array_equal(used[k][0], seq[k][0]) and np.array_equal(used[k][1], seq[k][1]), "target %d" % k
    assert final_rep == final_seq and st2 == st
    if scene == "default":
        assert st["fused"] >= 2000 and st["bad"] >= 100 and st["dirty"] >= 100 and cnt["stale_differs"] >= 100
    else:
        assert st["dirty"] >= 10
    assert box["submissions"] == 1 + box["fallback_targets"]
    assert box["selects"] == cnt["dirty_pairs"]
    if cap == 4:
        assert box["fallback_selects"] <= 0.01 * box["selects"]
    else:  # cand_cap = 1 truncates every list of two or more: the fallback path really runs
        assert box["fallback_targets"] >= 5 and box["fallback_selects"] >= 50
    mp.close()
    for kf in kfs:
        kf.close()


def test_errors(world):
    w = world
    orbfe, ex, L = w["orbfe"], w["ex"], w["orbfe"].lib()
    M = 64
    ids, _ = make_ids(w, M, 2)
    ts = list(w["targets"][:10])
    bare = orbfe.KeyFrame(ex, ts[7]["kp"].view(orbfe.KP_DTYPE), ts[7]["desc"], np.full(len(ts[7]["kp"]), -1, np.int32), w["sf"])
    ts[7] = dict(ts[7], kf=bare)  # target 7 has no grid
    K = len(ts)
    hs = (C.c_void_p * K)(*[t["kf"].h.value for t in ts])
    fr = (orbfe.Frustum * K)()
    for k in range(K):
        C.memmove(C.byref(fr, k * C.sizeof(orbfe.Frustum)), C.byref(ts[k]["Fp"]), C.sizeof(orbfe.Frustum))
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def raw(K_, hs_, fr_, cap, bi, bd, ci, cc):
        return L.orbfe_fuse_search_keyframes(ex.h, K_, hs_, fr_, w["mp"].h, M, p(ids), None, 10.0, p(bi), p(bd), cap, p(ci), p(cc))

    outs = [np.full(K * M * n, -777, np.int32) for n in (1, 1, 4, 1)]
    assert raw(K, hs, fr, 4, *outs) == orbfe.ERR_INVALID_ARG
    assert all((o == -777).all() for o in outs), "a refused call wrote results"
    with pytest.raises(orbfe.OrbfeError) as e:
        batch(w, ids, 10.0, targets=ts)
    assert e.value.code == orbfe.ERR_INVALID_ARG and "grid" in str(e.value) and "7" in str(e.value)
    bare.close()
    ts = w["targets"][:10]
    hs = (C.c_void_p * K)(*[t["kf"].h.value for t in ts])
    assert raw(K, hs, fr, 17, *outs) == orbfe.ERR_INVALID_ARG and raw(K, hs, fr, -1, *outs) == orbfe.ERR_INVALID_ARG
    assert raw(K, hs, None, 4, *outs) == orbfe.ERR_INVALID_ARG and raw(K, None, fr, 4, *outs) == orbfe.ERR_INVALID_ARG
    assert L.orbfe_fuse_search_keyframes(ex.h, K, hs, fr, w["mp"].h, M, None, None, 10.0, p(outs[0]), p(outs[1]), 0, None, None) == 1
    assert L.orbfe_fuse_search_keyframes(ex.h, K, hs, fr, w["mp"].h, M, p(ids), None, 10.0, p(outs[0]), p(outs[1]), 4, None, None) == 1
    assert raw(0, None, None, 4, *outs) == 0 and all((o == -777).all() for o in outs)  # K = 0: fine, nothing written
    bi, bd = batch(w, ids, 10.0, targets=[])
    assert bi.shape == (0, M)
    bi, bd, ci, cc = batch(w, ids[:0], 10.0, cand_cap=4)
    assert bi.shape == (len(w["targets"]), 0) and ci.shape == (len(w["targets"]), 0, 4)
    assert raw(K, hs, fr, 4, *outs) == 0 and not (outs[0] == -777).any()  # and the handle still works


def test_single_call_unchanged_around_a_batch_and_tracking_thread_on_the_same_handle(world):
    """The batch call shares the handle's matcher scratch with every other matcher call: the single call gives the same answers
    before and after a batch call, and a second thread that runs orbfe_track_frame on the SAME handle meanwhile still matches
    the oracle (as tests/test_two_threads_gpu.py: the calls serialise on the handle's lock)."""
    from orbfe import synth
    w = world
    orbfe, ex, eo = w["orbfe"], w["ex"], w["eo"]
    ids, none = make_ids(w, M_MAX, 3)
    t5 = w["targets"][5]
    before = w["m"].Fuse_search_keyframe(t5["kf"], w["mp"], ids, t5["Fp"], 10.0)
    want = batch(w, ids, 10.0, None, cand_cap=4)
    after = w["m"].Fuse_search_keyframe(t5["kf"], w["mp"], ids, t5["Fp"], 10.0)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and np.array_equal(want[0][5], before[0])
    bi_r, bd_r = oracle_row(w, t5, 10.0, M_MAX, (ids < 0) | none)
    assert np.array_equal(before[0], bi_r) and np.array_equal(before[1], bd_r)
    # the tracking thread's expectation, from the oracle
    img = synth.frame(W, H, 41)
    kp_r, desc_r, _ = eo.extract(img)
    Fo, Fp = O.Frustum(), orbfe.Frustum()
    v = FS.fill_frustum(Fo, ON, W=float(W), H=float(H), seed=21)
    FS.fill_frustum(Fp, PN, W=float(W), H=float(H), seed=21)
    pts, wdesc = FS.world_points_on_keypoints(kp_r, desc_r, v, 1500, np.random.default_rng(1), 8)
    fvo = O.make_frame_view(kp_r, desc_r, 64, 48, 0.0, 0.0, float(W), float(H), eo.scaleFactors)
    mps_o, _ = O.is_in_frustum(Fo, pts)
    n_t, out_t = O.search_by_projection(fvo, mps_o, wdesc, None, 20.0, 0.85)
    assert n_t > 300
    trk = orbfe.FrameTracker(ex, 64, 48, 0.0, 0.0, float(W), float(H))
    got_t, got_b, errs = [], [], []

    def tracking():
        try:
            for _ in range(30):
                r = trk.TrackFrame(img, Fp, pts.view(orbfe.WP_DTYPE), wdesc, 20.0, 0.85)
                got_t.append((r["kp"].tobytes(), r["mps"].tobytes(), r["match"].tobytes(), r["nmatches"]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    def mapping():
        try:
            for j in range(30):
                got_b.append(batch(w, ids, 10.0, None, cand_cap=4 if j % 2 == 0 else 0))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=tracking), threading.Thread(target=mapping)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout=240)
        assert not t.is_alive(), "a thread did not finish"
    assert not errs, errs
    assert len(got_t) == 30 and len(got_b) == 30
    for g in got_t:
        assert g == (kp_r.tobytes(), mps_o.tobytes(), out_t.tobytes(), n_t), "track_frame changed next to the batch call"
    for g in got_b:
        assert all(np.array_equal(a, b) for a, b in zip(g, want)), "the batch call changed next to track_frame"

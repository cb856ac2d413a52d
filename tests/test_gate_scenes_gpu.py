"""The planted gate-boundary scenes of tests/gate_scenes.py through every library entry point that runs a matcher on
caller-supplied keypoints: each output array equals the oracle's, no tolerance, no skipped element.  tests/test_gate_scenes.py
proves on the CPU that a kernel with any of the mistakes listed in tests/gate_mutants.py differs from the oracle on these scenes."""
import numpy as np
import pytest

import gate_scenes as GS
import oracle_py as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import orbfe
    ex = orbfe.ORBextractor(1000, 40000, 1.2, GS.NLEVELS, 20, 7, 752, 480, device=0, max_batch=1)
    assert np.asarray(ex.mvScaleFactor, np.float32).tobytes() == GS.SF.tobytes()
    scenes = GS.scenes()
    return dict(orbfe=orbfe, ex=ex, m=orbfe.ORBmatcher(ex), scenes=scenes, ref=[GS.run_oracle(s) for s in scenes])


def of(gpu, *matchers):
    out = [(s, r) for s, r in zip(gpu["scenes"], gpu["ref"]) if s["matcher"] in matchers]
    assert {s["size"] == "bare" for s, _ in out} == {True, False}
    return out


def equal(got, ref, where):
    assert got.keys() == ref.keys()
    for k in ref:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), "%s: %s differs at %s" % (where, k, np.flatnonzero(g.reshape(-1) != r.reshape(-1))[:10])


def lib_view(gpu, kp, desc):
    return gpu["orbfe"].make_frame_view(kp.view(gpu["orbfe"].KP_DTYPE), desc, GS.COLS, GS.ROWS, GS.MINX, GS.MINY, GS.MAXX, GS.MAXY, gpu["ex"].mvScaleFactor)


def test_projection_host(gpu):
    orbfe, m = gpu["orbfe"], gpu["m"]
    for s, ref in of(gpu, "projection"):
        a = s["args"]
        n, out = m.SearchByProjection(lib_view(gpu, a["kp"], a["desc"]), a["mps"].view(orbfe.MP_DTYPE), a["mpDesc"], a["th"], a["bFarPoints"],
                                      a["thFarPoints"], a["nnRatio"], a["initObs"])
        equal(dict(n=np.int64(n), match=out), ref, s["name"] + " " + s["size"])


@pytest.mark.parametrize("B", GS.BATCHES)
def test_projection_batch_device(gpu, B):
    """B identical frames: every frame's row equals the oracle's"""
    import torch
    orbfe, m = gpu["orbfe"], gpu["m"]
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
    for s, ref in of(gpu, "projection"):
        a = s["args"]
        n, M = len(a["kp"]), len(a["mps"])
        rep = lambda x: up(x).repeat(B)
        d_kp, d_desc, d_mps, d_mpd, d_obs = rep(a["kp"]), rep(a["desc"]), rep(a["mps"]), rep(a["mpDesc"]), rep(a["initObs"])
        d_n = torch.full((B,), n, dtype=torch.int32, device=dev)
        d_out = torch.full((B * n,), -7, dtype=torch.int32, device=dev)
        d_nm = torch.full((B,), -7, dtype=torch.int32, device=dev)
        m.SearchByProjection_batch_device(B, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), n, GS.COLS, GS.ROWS, GS.MINX, GS.MINY, GS.MAXX,
                                          GS.MAXY, M, d_mps.data_ptr(), d_mpd.data_ptr(), d_obs.data_ptr(), a["th"], a["nnRatio"], d_out.data_ptr(),
                                          d_nm.data_ptr(), bFarPoints=a["bFarPoints"], thFarPoints=a["thFarPoints"],
                                          stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        out, nm = d_out.cpu().numpy().reshape(B, n), d_nm.cpu().numpy()
        assert (nm == ref["n"]).all(), (s["size"], nm[:8], ref["n"])
        bad = np.flatnonzero((out != ref["match"][None, :]).any(axis=1))
        assert len(bad) == 0, "%s: frames %s differ" % (s["size"], bad[:8])


def test_fuse_host(gpu):
    orbfe, m = gpu["orbfe"], gpu["m"]
    Fp = GS.frustum(orbfe.Frustum)
    for s, ref in of(gpu, "fuse", "fuse_right", "fuse_sim3"):
        a = s["args"]
        fv, pts = lib_view(gpu, a["kp"], a["desc"]), a["pts"].view(orbfe.WP_DTYPE)
        if s["matcher"] == "fuse":
            bi, bd = m.Fuse_search(fv, a["invLevelSigma2"], a["uRight"], Fp, a["th"], pts, a["mpDesc"])
        elif s["matcher"] == "fuse_right":
            bi, bd = m.Fuse_search_right(fv, a["nRight"], a["invLevelSigma2"], a["uRight"], Fp, a["th"], pts, a["mpDesc"])
        else:
            bi, bd = m.Fuse_search_sim3(fv, Fp, a["th"], pts, a["mpDesc"])
        equal(dict(bestIdx=bi, bestDist=bd), ref, s["name"] + " " + s["size"])


def test_fuse_resident_and_candidate_crowd(gpu):
    """KeyFrame + MapPoints: Fuse_search_keyframe, Fuse_search_keyframes at cand_cap 0, 4 and 16.  The crowd points have 16, 17 and
    24 keypoints that pass every gate: cand_count is the true count, the list holds the 16 first visited in visit order, and
    fuse_select refuses a truncated list."""
    orbfe, m, ex = gpu["orbfe"], gpu["m"], gpu["ex"]
    Fp = GS.frustum(orbfe.Frustum)
    for s, ref in of(gpu, "fuse"):
        a, where = s["args"], s["name"] + " " + s["size"]
        n, M = len(a["kp"]), len(a["pts"])
        stereo = None if a["uRight"] is None else (a["uRight"] >= 0).astype(np.uint8)
        kf = orbfe.KeyFrame(ex, a["kp"].view(orbfe.KP_DTYPE), a["desc"], np.full(n, -1, np.int32), GS.SF, stereo)
        kf.set_grid(GS.COLS, GS.ROWS, GS.MINX, GS.MINY, GS.MAXX, GS.MAXY, a["invLevelSigma2"], a["uRight"])
        mp = orbfe.MapPoints(ex, M)
        stored = a["pts"].copy()
        stored["skip"] = 0
        ids = np.arange(M, dtype=np.int32)
        mp.update(ids, stored.view(orbfe.WP_DTYPE), a["mpDesc"])
        skip = a["pts"]["skip"] != 0
        bi, bd = m.Fuse_search_keyframe(kf, mp, np.where(skip, ~ids, ids).astype(np.int32), Fp, a["th"])
        equal(dict(bestIdx=bi, bestDist=bd), ref, where + " keyframe")
        skip2 = np.stack([skip, skip]).astype(np.uint8)
        lists = {}
        for cap in (0, 4, 16):
            got = m.Fuse_search_keyframes([kf, kf], mp, ids, [Fp, Fp], a["th"], skip=skip2, cand_cap=cap)
            for k in (0, 1):
                equal(dict(bestIdx=got[0][k], bestDist=got[1][k]), ref, where + " keyframes cand_cap %d target %d" % (cap, k))
            if cap:
                lists[cap] = got[2:]
        ci, cc = lists[16]
        assert np.array_equal(lists[4][1], cc) and np.array_equal(lists[4][0], ci[:, :, :4])
        assert np.array_equal(cc[0] == 0, ref["bestIdx"] == -1)
        assert len(s["crowd"]) == 3
        for i, mine in s["crowd"]:
            order = GS.visit_order(a["kp"], a["desc"], mine)
            for k in (0, 1):
                assert cc[k, i] == len(mine), (where, i, cc[k, i], len(mine))
                assert list(ci[k, i]) == order[:16], (where, i, list(ci[k, i]), order[:16])
                assert list(lists[4][0][k, i]) == order[:4]
                if len(mine) > 16:
                    assert ref["bestIdx"][i] not in order[:16]   # the best comes late: a select on the truncated list would be wrong
                    with pytest.raises(orbfe.OrbfeError) as e:
                        orbfe.fuse_select(ci[k, i], cc[k, i], 16, a["desc"], a["mpDesc"][i])
                    assert e.value.code == orbfe.ERR_UNSUPPORTED
                else:
                    assert orbfe.fuse_select(ci[k, i], cc[k, i], 16, a["desc"], a["mpDesc"][i]) == (ref["bestIdx"][i], ref["bestDist"][i])
        assert sorted(len(mine) for _, mine in s["crowd"]) == [16, 17, 24]
        kf.close()
        mp.close()


def test_bow(gpu):
    m = gpu["m"]
    for s, ref in of(gpu, "bow"):
        a = s["args"]
        n, out = m.SearchByBoW(a["kfOff"], a["kfIdx"], a["fOff"], a["fIdx"], a["kfDesc"], a["kfAngle"], a["kfHasMP"], a["fDesc"], a["fAngle"],
                               a["nnRatio"], a["checkOrientation"], nLeft=a["nLeft"])
        equal(dict(n=np.int64(n), match=out), ref, s["name"] + " " + s["size"])


def test_frustum_host_and_device(gpu):
    import torch
    orbfe, m = gpu["orbfe"], gpu["m"]
    Fp = GS.frustum(orbfe.Frustum)
    dev = torch.device("cuda", 0)
    for s, ref in of(gpu, "frustum"):
        pts = s["args"]["pts"].view(orbfe.WP_DTYPE)
        out, xr = m.isInFrustum_batch(Fp, pts)
        equal(dict(records=out.view(O.MP_DTYPE), projXR=xr), ref, s["size"] + " host")
        n = len(pts)
        d_pts = torch.from_numpy(pts.view(np.uint8).reshape(-1).copy()).to(dev)
        d_out = torch.zeros(n * orbfe.MP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_xr = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
        m.isInFrustum_batch_device(Fp, n, d_pts.data_ptr(), d_out.data_ptr(), d_xr.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        equal(dict(records=d_out.cpu().numpy().view(O.MP_DTYPE), projXR=d_xr.cpu().numpy()), ref, s["size"] + " device")


def test_relocalisation(gpu):
    orbfe, m = gpu["orbfe"], gpu["m"]
    Fp = GS.frustum(orbfe.Frustum)
    for s, ref in of(gpu, "projection_kf"):
        a = s["args"]
        n, out = m.SearchByProjection_keyframe(lib_view(gpu, a["kp"], a["desc"]), Fp, a["pts"].view(orbfe.WP_DTYPE), a["mpDesc"], a["kfAngle"],
                                               a["frameHasMP"], a["th"], a["checkOrientation"])
        equal(dict(n=np.int64(n), match=out), ref, s["size"])


def test_search_by_sim3(gpu):
    orbfe, m = gpu["orbfe"], gpu["m"]
    for s, ref in of(gpu, "sim3"):
        a = s["args"]
        n, out = m.SearchBySim3(lib_view(gpu, a["kp1"], a["desc1"]), lib_view(gpu, a["kp2"], a["desc2"]), GS.sim3_dir(orbfe.Sim3View),
                                GS.sim3_dir(orbfe.Sim3View), a["mp1"].view(orbfe.WP_DTYPE), a["mpDesc1"], a["mp2"].view(orbfe.WP_DTYPE), a["mpDesc2"], a["th"])
        equal(dict(n=np.int64(n), match=out), ref, s["size"])


def test_search_for_initialization(gpu):
    m = gpu["m"]
    for s, ref in of(gpu, "initialization"):
        a = s["args"]
        n, out = m.SearchForInitialization(lib_view(gpu, a["kp1"], a["desc1"]), lib_view(gpu, a["kp2"], a["desc2"]), a["windowSize"], a["nnRatio"],
                                           a["checkOrientation"])
        equal(dict(n=np.int64(n), matches12=out), ref, s["name"] + " " + s["size"])


def test_search_for_triangulation(gpu):
    orbfe, m = gpu["orbfe"], gpu["m"]
    for s, ref in of(gpu, "triangulation"):
        a = s["args"]
        n, out = m.SearchForTriangulation(a["off1"], a["idx1"], a["off2"], a["idx2"], a["kp1"].view(orbfe.KP_DTYPE), a["desc1"], a["hasMP1"], a["stereo1"],
                                          a["kp2"].view(orbfe.KP_DTYPE), a["desc2"], a["hasMP2"], a["stereo2"], a["scaleFactors2"], a["F12"], a["ep"],
                                          a["bOnlyStereo"], a["bCoarse"], a["checkOrientation"], cameras=a["cameras"])
        equal(dict(n=np.int64(n), matches12=out), ref, s["name"] + " " + s["size"])


def test_search_for_triangulation_batch(gpu):
    """the mapping thread's call shape: resident KeyFrames, one launch against two neighbours (the same key frame twice), the host
    replay with the flags of key frame 1 unchanged -> both neighbours equal the oracle's single call"""
    orbfe, ex = gpu["orbfe"], gpu["ex"]
    for s, ref in of(gpu, "triangulation"):
        a = s["args"]
        node1, node2 = np.full(len(a["kp1"]), -1, np.int32), np.full(len(a["kp2"]), -1, np.int32)
        for g in range(len(a["off1"]) - 1):   # a node's features are walked in ascending index; the filler, which a padded scene lists
            node1[a["idx1"][a["off1"][g]:a["off1"][g + 1]]] = g   # around the planted features, is never accepted, so its place does not matter
            node2[a["idx2"][a["off2"][g]:a["off2"][g + 1]]] = g
        kf1 = orbfe.KeyFrame(ex, a["kp1"].view(orbfe.KP_DTYPE), a["desc1"], node1, GS.SF, a["stereo1"])
        kf2 = orbfe.KeyFrame(ex, a["kp2"].view(orbfe.KP_DTYPE), a["desc2"], node2, GS.SF, a["stereo2"])
        P = orbfe.tri_params(a["F12"], a["ep"], a["bOnlyStereo"], a["bCoarse"], a["checkOrientation"], a["cameras"])
        raw, rbin = orbfe.SearchForTriangulation_batch(ex, kf1, a["hasMP1"], [kf2, kf2], [a["hasMP2"], a["hasMP2"]], [P, P])
        for k in (0, 1):
            n, m12 = orbfe.triangulation_select(raw[k], rbin[k], a["hasMP1"], a["checkOrientation"])
            equal(dict(n=np.int64(n), matches12=m12), ref, "%s %s neighbour %d" % (s["name"], s["size"], k))
        kf1.close()
        kf2.close()

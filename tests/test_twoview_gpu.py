"""orbfe_two_view_reconstruct on the GPU against the restatement of SPEC DECISION S12 (twoview_ref.reconstruct, written from
src/TwoViewReconstruction.cc) on the scenes of twoview_scenarios (test_twoview.py checks which exits they reach).  Every
comparison is exact: the bytes of all 2 x iterations scores, both winning matrices, their iterations and inlier masks, SH, SF,
RH, the model, every motion hypothesis with its nGood / cosine / flags / x3D, R21, t21, p3d, triangulated and the flag.  No
tolerance, no skipped element."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import twoview_ref as R
import twoview_scenarios as TS

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
F32_FIELDS = ("R21", "t21", "p3d", "SH", "SF", "RH", "H21", "F21", "cos_parallax", "hyp_R", "hyp_t", "scores", "rt_x3d", "rt_cos")
INT_FIELDS = ("n_matches", "model", "exit_line", "best_it_H", "best_it_F", "n_hypotheses", "best_hypothesis")
U8_FIELDS = ("triangulated", "inliers_H", "inliers_F", "rt_flags")


def keypoints(xy):
    import orbfe
    kp = np.zeros(len(xy), orbfe.KP_DTYPE)
    kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
    kp["size"] = 31.0
    return kp


def tv_params(sc):
    import orbfe
    fx, fy, cx, cy, sigma, iterations = sc["params"]
    return orbfe.TwoViewParams(fx, fy, cx, cy, sigma, iterations)


@functools.lru_cache(maxsize=None)
def scene_and_ref(case, seed=0):
    sc = TS.make(case[0], case[1], seed, case[2], case[3])
    return sc, TS.ref(sc)


def call(ex, sc, want_info=True):
    import orbfe
    return orbfe.two_view_reconstruct(ex, tv_params(sc), keypoints(sc["kp1"]), keypoints(sc["kp2"]), sc["matches12"], sc["sets"], want_info)


def same(got, want, what, info=True):
    assert got["reconstructed"] == bool(want["reconstructed"]), "%s: reconstructed %s, restatement %s (exit %s)" % (
        what, got["reconstructed"], want["reconstructed"], want["exit_line"])
    fields = F32_FIELDS + INT_FIELDS + U8_FIELDS + ("n_good",) if info else ("R21", "t21", "p3d", "triangulated")
    for k in fields:
        if k in INT_FIELDS:
            assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
            continue
        dt = np.float32 if k in F32_FIELDS else (np.int32 if k == "n_good" else np.uint8)
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k], dt)
        assert g.dtype == dt and g.shape == w.shape, "%s: %s has %s %s, restatement %s" % (what, k, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8 if dt == np.uint8 else np.uint32) != w.reshape(-1).view(np.uint8 if dt == np.uint8 else np.uint32))
            raise AssertionError("%s: %s differs in %d of %d elements, first %d: %r, restatement %r" % (
                what, k, len(bad), g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]]))


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    yield e
    e.close()


@pytest.mark.parametrize("case", TS.CASES, ids=TS.case_id)
def test_equals_restatement(ex, case):
    sc, want = scene_and_ref(case)
    got = call(ex, sc)
    same(got, want, TS.case_id(case))


def test_scenes_reach_every_exit_and_both_models():
    exits, models = set(), set()
    for case in TS.CASES:
        want = scene_and_ref(case)[1]
        exits.add(want["exit_line"])
        if want["reconstructed"]:
            models.add(want["model"])
    assert exits >= {0, 110, 528, 580, 609, 746}, exits
    assert models == {R.MODEL_H, R.MODEL_F}


def test_fewer_than_eight_matches(ex):
    """*reconstructed = 0, status ok, no GPU work; the sets are not looked at"""
    import orbfe
    sc, _ = scene_and_ref(("general", 64, 0.0, 7))
    for keep in (0, 7):
        m12 = sc["matches12"].copy()
        m12[np.flatnonzero(m12 >= 0)[keep:]] = -1
        got = orbfe.two_view_reconstruct(ex, tv_params(sc), keypoints(sc["kp1"]), keypoints(sc["kp2"]), m12, None)
        want = R.reconstruct(*sc["params"], sc["kp1"], sc["kp2"], m12, None)
        same(got, want, "%d matches" % keep)
        assert not got["reconstructed"] and got["exit_line"] == 62 and got["n_matches"] == keep
    empty = np.zeros(0, orbfe.KP_DTYPE)
    got = orbfe.two_view_reconstruct(ex, tv_params(sc), empty, empty, np.zeros(0, np.int32), None)
    assert not got["reconstructed"] and got["n_matches"] == 0


def test_invalid_arguments_and_a_call_after_a_refused_call(ex):
    import orbfe
    case = ("general", 65, 0.0, 200)
    sc, want = scene_and_ref(case)
    kp1, kp2 = keypoints(sc["kp1"]), keypoints(sc["kp2"])

    def refused(params=None, m12=None, sets=None, info=None):
        P = params if params is not None else tv_params(sc)
        m = np.ascontiguousarray(sc["matches12"] if m12 is None else m12, np.int32)
        s = np.ascontiguousarray(sc["sets"] if sets is None else sets, np.int32)
        rec = C.c_int(7)
        out = [np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros((len(kp1), 3), np.float32), np.zeros(len(kp1), np.uint8)]
        rc = ex.L.orbfe_two_view_reconstruct(ex.h, C.byref(P), len(kp1), kp1.ctypes.data, len(kp2), kp2.ctypes.data, m.ctypes.data,
                                             s.ctypes.data, C.byref(rec), *[o.ctypes.data for o in out],
                                             C.byref(info) if info is not None else None)
        assert rc == orbfe.ERR_INVALID_ARG, rc
        same(call(ex, sc), want, "after a refused call")

    s = sc["sets"].copy()
    s[3, 5] = sc["N"]
    refused(sets=s)                        # a set index outside the match list
    s = sc["sets"].copy()
    s[199, 0] = -1
    refused(sets=s)
    s = sc["sets"].copy()
    s[7, 6] = s[7, 2]
    refused(sets=s)                        # repeated inside a set
    m = sc["matches12"].copy()
    m[np.flatnonzero(m >= 0)[4]] = len(kp2)
    refused(m12=m)                         # a match index outside frame 2
    for it in (0, -3, 4097):
        P = tv_params(sc)
        P.iterations = it
        refused(params=P)
    P = tv_params(sc)
    P.struct_size -= 4
    refused(params=P)                      # a wrong struct_size
    P = tv_params(sc)
    P.min_parallax_deg = 2.0
    refused(params=P)
    info = orbfe.TwoViewInfo()
    info.struct_size += 8
    refused(info=info)
    rec = C.c_int(0)
    assert ex.L.orbfe_two_view_reconstruct(ex.h, None, 0, None, 0, None, None, None, C.byref(rec), None, None, None, None, None) == orbfe.ERR_INVALID_ARG
    assert ex.L.orbfe_two_view_reconstruct(None, C.byref(tv_params(sc)), 0, None, 0, None, None, None, C.byref(rec), None, None, None,
                                           None, None) == orbfe.ERR_INVALID_ARG


def test_info_null_and_same_call_twice(ex):
    for case in (("general", 300, 0.3, 200), ("plane", 300, 0.0, 200)):
        sc, want = scene_and_ref(case)
        a, b = call(ex, sc), call(ex, sc)
        for k in F32_FIELDS + U8_FIELDS + ("n_good",):
            assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
        got = call(ex, sc, want_info=False)
        assert set(got) == {"reconstructed", "R21", "t21", "p3d", "triangulated"}
        same(got, want, TS.case_id(case) + " without info", info=False)
        assert got["reconstructed"]


def test_two_threads_on_two_handles(built):
    import orbfe
    cases = [("general", 300, 0.3, 200), ("plane", 300, 0.3, 200)]
    exs = [orbfe.ORBextractor(*ARGS) for _ in range(2)]
    outs, errs = [[], []], []

    def digest(r):
        return tuple(np.ascontiguousarray(r[k]).tobytes() for k in F32_FIELDS + U8_FIELDS + ("n_good",))

    def run(t):
        try:
            sc = scene_and_ref(cases[t])[0]
            for _ in range(20):
                outs[t].append(digest(call(exs[t], sc)))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    for t in range(2):
        scene_and_ref(cases[t])  # (the cache is filled before the threads start)
    ths = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=240)
        assert not th.is_alive(), "a thread did not finish"
    assert not errs, errs
    for t in range(2):
        sc, want = scene_and_ref(cases[t])
        assert len(outs[t]) == 20 and all(o == outs[t][0] for o in outs[t]), "thread %d changed under concurrency" % t
        same(call(exs[t], sc), want, "thread %d" % t)
        assert digest(call(exs[t], sc)) == outs[t][0]
    for e in exs:
        e.close()


def test_chained_behind_track_initialization(built):
    """two synthetic frames related by a shift: the chain's kp / matches12 go straight into the call, and the result equals the
    restatement on the same inputs"""
    import orbfe
    from orbfe import synth
    W, H = ARGS[6], ARGS[7]
    e = orbfe.ORBextractor(*ARGS)
    trk = orbfe.FrameTracker(e, 64, 48, 0.0, 0.0, float(W), float(H))
    big = synth.frame(W + 32, H + 32, 900)
    img1 = np.ascontiguousarray(big[16:16 + H, 16:16 + W])
    img2 = np.ascontiguousarray(big[10:10 + H, 4:4 + W])  # shifted by (12, 6) pixels
    kp1, d1 = e.extractFeatures(img1)
    ini = orbfe.InitialFrame(e, kp1, d1)
    got = trk.TrackInitialization(img2, ini, 40, 0.9, True)
    m12, kp2 = got["matches12"], got["kp"]
    N = int((m12 >= 0).sum())
    assert got["nmatches"] == N and N >= 100  # FEAT_INIT_COUNT: the call site's own condition (src/Tracking.cc:609)
    rng = np.random.RandomState(4)
    sets = R.draw_sets(N, 200, lambda: int(rng.randint(0, 2 ** 31 - 1)))
    P = orbfe.TwoViewParams(458.654, 457.296, 367.215, 248.375, 1.0, 200)
    res = orbfe.two_view_reconstruct(e, P, kp1, kp2, m12, sets)
    xy1 = np.stack([kp1["x"], kp1["y"]], 1)
    xy2 = np.stack([kp2["x"], kp2["y"]], 1)
    want = R.reconstruct(P.fx, P.fy, P.cx, P.cy, 1.0, 200, xy1, xy2, m12, sets)
    same(res, want, "chained")
    assert want["n_matches"] == N and want["model"] != R.MODEL_NONE
    ini.close()
    e.close()

"""orbfe_mlpnp_ransac on the GPU against the restatement of SPEC DECISION S13 (mlpnp_ref.ransac, written from
src/MLPnPsolver.cpp) on the scenes of mlpnp_scenarios (test_mlpnp.py checks which exits and branches they reach).  Every
comparison is exact: the bytes of the pose, the inlier flags, the counts and flags of the call, and of every field of
orbfe_mlpnp_info -- all hypotheses' poses (binary64), inlier counts, planar flags, Gauss-Newton evaluations and exits, the candidate
list and every candidate's refined pose, count, planar flag and mask.  No tolerance, no skipped element."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import mlpnp_ref as R
import mlpnp_scenarios as MS

pytestmark = pytest.mark.gpu

ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)
OUT_FIELDS = (("Tcw", np.float32), ("inliers", np.uint8))
INT_FIELDS = ("n_inliers", "N", "min_inliers", "max_its", "total_iterations", "exit_kind", "returning_iteration", "n_candidates")
INFO_ARRAYS = (("hyp_Rt", np.float64), ("hyp_inliers", np.int32), ("hyp_planar", np.uint8), ("hyp_gn_evals", np.int32),
               ("hyp_gn_exit", np.int32), ("candidates", np.int32), ("cand_Rt", np.float64), ("cand_inliers", np.int32),
               ("cand_planar", np.uint8), ("cand_mask", np.uint8))


def keypoints(sc):
    import orbfe
    kp = np.zeros(len(sc["kp_xy"]), orbfe.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = sc["kp_xy"][:, 0], sc["kp_xy"][:, 1], sc["kp_octave"]
    kp["size"] = 31.0
    return kp


def params(sc):
    import orbfe
    return orbfe.MlpnpParams(sc["cam"], sc["model"], sc["precision"], **sc["ransac"])


@functools.lru_cache(maxsize=None)
def scene_and_ref(case):
    sc = MS.make_case(case)
    return sc, MS.ref(sc)


def call(ex, sc, want_info=True):
    import orbfe
    return orbfe.mlpnp_ransac(ex, params(sc), keypoints(sc), sc["mp_index"], sc["points"], sc["sets"] if len(sc["sets"]) else None, want_info)


def same(got, want, what, info=True):
    for k in ("solved", "no_more"):
        assert got[k] == bool(want[k]), "%s: %s %s, restatement %s (exit %s)" % (what, k, got[k], want[k], want["exit_kind"])
    for k in INT_FIELDS[:1] + (INT_FIELDS[1:] if info else ()):
        assert int(got[k]) == int(want[k]), "%s: %s = %d, restatement %d" % (what, k, got[k], want[k])
    for k, dt in OUT_FIELDS + (INFO_ARRAYS if info else ()):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k], dt)
        assert g.dtype == dt and g.shape == w.shape, "%s: %s has %s %s, restatement %s" % (what, k, g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)) // g.dtype.itemsize
            raise AssertionError("%s: %s differs in %d of %d elements, first %d: %r, restatement %r" % (
                what, k, len(set(bad.tolist())), g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]]))


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(*ARGS)
    assert e.mvLevelSigma2.tobytes() == MS.level_sigma2().tobytes()  # the scenes' table is the handle's
    yield e
    e.close()


@pytest.mark.parametrize("case", MS.CASES, ids=MS.case_id)
def test_equals_restatement(ex, case):
    sc, want = scene_and_ref(case)
    same(call(ex, sc), want, MS.case_id(case))


def test_plan_equals_restatement(built):
    import orbfe
    for eps in (0.5, 0.2):
        P = orbfe.MlpnpParams(epsilon=eps)
        for N in (0, 49, 50, 51, 99, 100, 101, 300, 1000):
            assert orbfe.mlpnp_plan(P, N) == R.plan(N, epsilon=eps)


def test_info_null_and_same_call_twice(ex):
    for case in (MS.CASES[0], MS.CASES[2], MS.CASES[10]):
        sc, want = scene_and_ref(case)
        a, b = call(ex, sc), call(ex, sc)
        for k, _ in OUT_FIELDS + INFO_ARRAYS:
            assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
        got = call(ex, sc, want_info=False)
        assert set(got) == {"solved", "Tcw", "inliers", "n_inliers", "no_more"}
        same(got, want, MS.case_id(case) + " without info", info=False)
        assert got["solved"]


def test_invalid_arguments_and_a_call_after_a_refused_call(ex):
    import orbfe
    case = MS.CASES[12]  # general, N = 65
    sc, want = scene_and_ref(case)
    kp = keypoints(sc)

    def refused(P=None, mp=None, sets=None, n_sets=None, info=None, n_points=None):
        P = P if P is not None else params(sc)
        m = np.ascontiguousarray(sc["mp_index"] if mp is None else mp, np.int32)
        s = np.ascontiguousarray(sc["sets"] if sets is None else sets, np.int32)
        pts = np.ascontiguousarray(sc["points"], np.float32)
        solved, ninl, nomore = C.c_int(7), C.c_int(7), C.c_int(7)
        Tcw, inl = np.zeros(16, np.float32), np.zeros(len(kp), np.uint8)
        rc = ex.L.orbfe_mlpnp_ransac(ex.h, C.byref(P), len(kp), kp.ctypes.data, m.ctypes.data, len(pts) if n_points is None else n_points,
                                     pts.ctypes.data, s.ctypes.data, len(sc["sets"]) if n_sets is None else n_sets, C.byref(solved),
                                     Tcw.ctypes.data, inl.ctypes.data, C.byref(ninl), C.byref(nomore),
                                     C.byref(info) if info is not None else None)
        assert rc == orbfe.ERR_INVALID_ARG, rc
        same(call(ex, sc), want, "after a refused call")

    P = params(sc)
    P.struct_size -= 4
    refused(P=P)                                   # struct_size of the parameters
    info = orbfe.MlpnpInfo()
    info.struct_size += 8
    refused(info=info)                             # ... and of the info block
    refused(n_sets=len(sc["sets"]) - 1)            # n_sets != the plan's total_iterations
    refused(n_sets=len(sc["sets"]) + 1)
    s = sc["sets"].copy()
    s[3, 5] = want["N"]
    refused(sets=s)                                # a set index out of range
    s = sc["sets"].copy()
    s[len(s) - 1, 0] = -1
    refused(sets=s)
    s = sc["sets"].copy()
    s[7, 6] = s[7, 2]
    refused(sets=s)                                # a set index repeated
    m = sc["mp_index"].copy()
    m[np.flatnonzero(m >= 0)[4]] = len(sc["points"])
    refused(mp=m)                                  # mp_index beyond the points
    for ms in (5, 65, 0, -1):
        P = params(sc)
        P.min_set = ms
        refused(P=P)                               # min_set outside [6, 64]
    solved = C.c_int(0)
    assert ex.L.orbfe_mlpnp_ransac(ex.h, None, 0, None, None, 0, None, None, 0, C.byref(solved), None, None, None, None, None) == orbfe.ERR_INVALID_ARG
    assert ex.L.orbfe_mlpnp_ransac(None, C.byref(params(sc)), 0, None, None, 0, None, None, 0, C.byref(solved), None, None, None, None,
                                   None) == orbfe.ERR_INVALID_ARG


def test_abort_needs_no_sets(ex):
    """N < min_inliers: solved = 0, no_more = 1, status ok, no GPU work; the sets are not looked at"""
    sc, want = scene_and_ref(MS.CASES[9])  # N = 49
    got = call(ex, sc)
    same(got, want, "abort")
    assert not got["solved"] and got["no_more"] and got["exit_kind"] == R.EXIT_ABORT and got["total_iterations"] == 0


def test_two_threads_on_two_handles(built):
    import orbfe
    cases = [MS.CASES[0], MS.CASES[2]]
    exs = [orbfe.ORBextractor(*ARGS) for _ in range(2)]
    outs, errs = [[], []], []

    def digest(r):
        return tuple(np.ascontiguousarray(r[k]).tobytes() for k, _ in OUT_FIELDS + INFO_ARRAYS)

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
    for e in exs:
        e.close()

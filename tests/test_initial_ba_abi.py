"""Argument refusals of orbfe_initial_bundle_adjustment.  What the parameter block alone decides -- struct sizes, the unsupported
branches, the ranges -- is checked before the handle is looked at, so those refusals need no device (the first three tests).  The
octave check, a match >= n2, n1 or n2 > 65536 and the N = 0 return read the handle's level count; the call decides them before it
touches the device, but a handle cannot be created without one (orbfe_create, test_abi.py), so those tests carry the gpu mark."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import initial_ba_scenarios as BS
from test_initial_ba_cpp import keypoints

INVALID, UNSUPPORTED = 1, 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbfe.h")


def _args(sc):
    import orbfe
    return (keypoints(sc["kp1_xy"], sc["kp1_octave"], orbfe.KP_DTYPE), keypoints(sc["kp2_xy"], sc["kp2_octave"], orbfe.KP_DTYPE),
            sc["matches12"], sc["points"], sc["Rcw1"], sc["tcw1"], sc["Rcw2"], sc["tcw2"])


def _code(fn):
    import orbfe
    with pytest.raises(orbfe.OrbfeError) as ei:
        fn()
    return ei.value.code


def test_blocks_match_the_header(built):
    import orbfe
    p = orbfe.InitialBAParams()
    assert p.struct_size == C.sizeof(orbfe.InitialBAParams) == 64
    assert orbfe.InitialBAInfo().struct_size == C.sizeof(orbfe.InitialBAInfo) == 20 + 4 + 64 * 4 + 2 * 64 * 8 + 12 * 8 + 2 * 8
    assert (p.camera_model, p.robust, p.iterations, p.stereo) == (0, 1, 20, 0) and p.huber_delta2 == 5.99
    text = open(HEADER).read()
    init = re.search(r"#define ORBFE_INITIAL_BA_PARAMS_INIT \{(.*)\}\n", text).group(1)
    assert init.replace(" ", "").endswith("},5.99,1,20,0")   # huber_delta2, robust, iterations, stereo
    fields = re.search(r"typedef struct orbfe_initial_ba_params \{(.*?)\} orbfe_initial_ba_params;", text, re.S).group(1)
    names = re.findall(r"^\s*(?:int|float|double)\s+(\w+)", fields, re.M)
    assert names == [f[0] for f in orbfe.InitialBAParams._fields_]
    fields = re.search(r"typedef struct orbfe_initial_ba_info \{(.*?)\} orbfe_initial_ba_info;", text, re.S).group(1)
    names = re.findall(r"^\s*(?:int|float|double|uint8_t)\s+\*?(\w+)", fields, re.M)
    assert names == [f[0].rstrip("_") for f in orbfe.InitialBAInfo._fields_]


def test_unsupported_branches_without_a_device(built):
    """KannalaBrandt8 and the stereo edges are refused as UNSUPPORTED before anything else is looked at: no handle, no device"""
    import orbfe
    sc = BS.make("general", 10, 0)
    a = _args(sc)
    assert _code(lambda: orbfe.initial_bundle_adjustment(None, orbfe.InitialBAParams(sc["cam"], camera_model=1), *a)) == UNSUPPORTED
    assert _code(lambda: orbfe.initial_bundle_adjustment(None, orbfe.InitialBAParams(sc["cam"], stereo=1), *a)) == UNSUPPORTED


def test_struct_size_and_ranges_without_a_device(built):
    import orbfe
    sc = BS.make("general", 10, 0)
    a = _args(sc)
    for kw in (dict(iterations=0), dict(iterations=65), dict(huber_delta2=0.0), dict(huber_delta2=float("nan")), dict(robust=2),
               dict(robust=-1), dict(camera_model=7)):
        assert _code(lambda: orbfe.initial_bundle_adjustment(None, orbfe.InitialBAParams(sc["cam"], **kw), *a)) == INVALID, kw
    p = orbfe.InitialBAParams(sc["cam"])
    p.struct_size -= 4
    assert _code(lambda: orbfe.initial_bundle_adjustment(None, p, *a)) == INVALID
    # a sound block and no handle is INVALID_ARG too; so is a NULL block
    assert _code(lambda: orbfe.initial_bundle_adjustment(None, orbfe.InitialBAParams(sc["cam"]), *a)) == INVALID
    assert orbfe.lib().orbfe_initial_bundle_adjustment(None, None, 0, None, 0, None, None, None, None, None, None, None, None, None, None) == INVALID


@pytest.fixture(scope="module")
def ex(built):
    import orbfe
    e = orbfe.ORBextractor(1000, 40000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.gpu
def test_refusals_that_need_the_handle(ex):
    import orbfe
    sc = BS.make("general", 10, 0)
    kp1, kp2, m, pts, R1, t1, R2, t2 = _args(sc)
    p = orbfe.InitialBAParams(sc["cam"])
    i0 = np.flatnonzero(m >= 0)[0]
    bad = m.copy()
    bad[i0] = len(kp2)                             # a match >= n2
    assert _code(lambda: orbfe.initial_bundle_adjustment(ex, p, kp1, kp2, bad, pts, R1, t1, R2, t2)) == INVALID
    for octave in (-1, 8):                         # an octave of a MATCHED keypoint, in either frame, outside the handle's levels
        k = kp1.copy()
        k["octave"][i0] = octave
        assert _code(lambda: orbfe.initial_bundle_adjustment(ex, p, k, kp2, m, pts, R1, t1, R2, t2)) == INVALID
        k = kp2.copy()
        k["octave"][m[i0]] = octave
        assert _code(lambda: orbfe.initial_bundle_adjustment(ex, p, kp1, k, m, pts, R1, t1, R2, t2)) == INVALID
    k1, k2 = kp1.copy(), kp2.copy()                # ... of an unmatched one is never read
    k1["octave"][np.flatnonzero(m < 0)[0]] = 99
    k2["octave"][np.setdiff1d(np.arange(len(kp2)), m[m >= 0])[0]] = 99
    a = orbfe.initial_bundle_adjustment(ex, p, k1, k2, m, pts, R1, t1, R2, t2)
    b = orbfe.initial_bundle_adjustment(ex, p, kp1, kp2, m, pts, R1, t1, R2, t2)
    assert a["Tcw2"].tobytes() == b["Tcw2"].tobytes() and a["points"].tobytes() == b["points"].tobytes()
    big = np.zeros(65537, orbfe.KP_DTYPE)
    none = np.full(65537, -1, np.int32)
    assert _code(lambda: orbfe.initial_bundle_adjustment(ex, p, big, kp2, none, np.zeros((65537, 3), np.float32), R1, t1, R2, t2)) == INVALID
    assert _code(lambda: orbfe.initial_bundle_adjustment(ex, p, kp1, big, m, pts, R1, t1, R2, t2)) == INVALID
    info = orbfe.InitialBAInfo()
    info.struct_size += 8
    Tcw, out = np.zeros(16, np.float32), np.zeros((len(kp1), 3), np.float32)
    rc = ex.L.orbfe_initial_bundle_adjustment(ex.h, C.byref(p), len(kp1), kp1.ctypes.data, len(kp2), kp2.ctypes.data, m.ctypes.data,
                                              np.ascontiguousarray(pts).ctypes.data, R1.ctypes.data, t1.ctypes.data, R2.ctypes.data,
                                              t2.ctypes.data, Tcw.ctypes.data, out.ctypes.data, C.byref(info))
    assert rc == INVALID


@pytest.mark.gpu
def test_no_match_is_ok_and_returns_the_inputs(ex):
    """N = 0: ORBFE_OK, the outputs equal the inputs, nothing is launched (the info block says 0 iterations)"""
    import orbfe
    sc = BS.make("general", 10, 0)
    kp1, kp2, m, pts, R1, t1, R2, t2 = _args(sc)
    o = orbfe.initial_bundle_adjustment(ex, orbfe.InitialBAParams(sc["cam"]), kp1, kp2, np.full_like(m, -1), pts, R1, t1, R2, t2)
    assert o["N"] == 0 and o["iterations"] == 0 and o["trials"] == 0 and o["points"].tobytes() == pts.tobytes()
    assert o["Tcw2"][:3, :3].reshape(-1).tobytes() == R2.tobytes() and o["Tcw2"][:3, 3].tobytes() == t2.tobytes()
    assert o["Tcw2"][3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert o["pose"].tobytes() == np.concatenate([R2, t2]).astype(np.float64).tobytes()
    empty = np.zeros(0, orbfe.KP_DTYPE)
    o = orbfe.initial_bundle_adjustment(ex, orbfe.InitialBAParams(sc["cam"]), empty, empty, np.zeros(0, np.int32), np.zeros((0, 3), np.float32),
                                        R1, t1, R2, t2)
    assert o["N"] == 0 and len(o["points"]) == 0

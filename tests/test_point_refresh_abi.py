"""The ABI of the S26 calls: the symbols, the block and the constants against the header; the refusals that the arguments alone decide,
which come back before a handle or a device is looked at; and, on the GPU, every refusal the header lists that needs a graph to be
decided -- each leaves the graph and the map as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import point_refresh_ref as P
import point_refresh_scenarios as S

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbfe_covis_enable_refresh", "orbfe_covis_set_features", "orbfe_covis_set_features_device", "orbfe_covis_set_centres",
         "orbfe_covis_set_observations_indexed", "orbfe_covis_set_ref_keyframes", "orbfe_covis_get_point",
         "orbfe_covis_refresh_points_device", "orbfe_covis_refresh_points")
ARGS = (1000, 40000, 1.2, 8, 20, 7, 752, 480)


def _header():
    return open(os.path.join(ROOT, "include", "orbfe.h")).read()


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in orbfe.SYMBOLS
        assert re.search(r"\b%s\(" % name, _header())


def test_constants_and_block_match_the_header(built):
    import orbfe
    txt = _header()
    define = lambda name: int(re.search(r"#define %s\s+(\S+)" % name, txt).group(1), 0)   # noqa: E731
    assert define("ORBFE_REFRESH_MAX_LEVELS") == orbfe.REFRESH_MAX_LEVELS == 32
    assert (define("ORBFE_REFRESH_DEPTH"), define("ORBFE_REFRESH_DESCRIPTOR")) == (orbfe.REFRESH_DEPTH, orbfe.REFRESH_DESCRIPTOR) == \
        (P.DEPTH, P.DESCRIPTOR) == (1, 2)
    body = re.search(r"typedef struct orbfe_refresh_io \{(.*?)\} orbfe_refresh_io;", txt, re.S).group(1)
    assert re.findall(r"^\s*(?:int|float) \*?(\w+);", body, re.M) == [n for n, _ in orbfe.RefreshIO._fields_]
    IO = orbfe.RefreshIO
    assert IO().struct_size == C.sizeof(IO) == 8 + 8 * len(orbfe.REFRESH_IO_FIELDS) == 56
    assert [getattr(IO, n).offset for n in orbfe.REFRESH_IO_FIELDS] == [8, 16, 24, 32, 40, 48]
    # what S26 must leave as it was
    assert C.sizeof(orbfe.CovisKeyframe) == 64 and C.sizeof(orbfe.CovisUpdateIO) == 40 and orbfe.WP_DTYPE.itemsize == 32


def test_argument_errors_without_a_device(built):
    import orbfe
    L = orbfe.lib()
    N, B = None, C.byref
    one = 4096   # a non-NULL stand-in for device pointers and the graph: the call is refused before any of them is read
    io = orbfe.RefreshIO()
    dev = lambda g=one, n=2, ids=one, what=3, io_=io: L.orbfe_covis_refresh_points_device(N, g, n, ids, N, 0, what, B(io_) if io_ else N, N)   # noqa: E731
    assert dev() == INVALID and dev(io_=False) == INVALID and dev(g=N) == INVALID
    short = orbfe.RefreshIO()
    short.struct_size -= 8
    assert dev(io_=short) == INVALID
    out = np.full(4, 7, np.int32)
    assert L.orbfe_covis_refresh_points(N, one, 2, one, 3, out.ctypes.data_as(C.c_void_p), N, N, N, N, N) == INVALID
    assert (out == 7).all()
    sf = np.ones(8, np.float32)
    assert L.orbfe_covis_enable_refresh(N, one, 8, sf.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.orbfe_covis_enable_refresh(one, N, 8, sf.ctypes.data_as(C.c_void_p)) == INVALID
    assert L.orbfe_covis_set_features(N, one, 0, 0, N, N) == INVALID and L.orbfe_covis_set_features_device(N, one, 0, one, one, 1, N) == INVALID
    assert L.orbfe_covis_set_centres(N, one, 0, N, N) == INVALID and L.orbfe_covis_set_ref_keyframes(N, one, 0, N, N) == INVALID
    assert L.orbfe_covis_set_observations_indexed(N, one, 0, N, N, N, N) == INVALID
    n = C.c_int(7)
    assert L.orbfe_covis_get_point(N, one, 0, B(n), one, one, B(n), N, N) == INVALID and n.value == 7


@pytest.mark.gpu
def test_refusals_with_a_handle_leave_graph_and_map_unchanged(built):
    import orbfe
    ex = orbfe.ORBextractor(*ARGS)
    rg = S.planted_graph()
    mp, cv = S.upload(orbfe, ex, rg, enable=False)
    L = orbfe.lib()
    K, C_, stride, obs = rg.g.kf_capacity, rg.g.capacity, rg.kf_stride, rg.obs_stride
    arr = lambda *v: np.array(v, np.int32)   # noqa: E731
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    sf = S.SCALE_FACTORS
    one = 4096
    try:
        # enable_refresh
        for n in (0, -1, orbfe.REFRESH_MAX_LEVELS + 1):
            assert L.orbfe_covis_enable_refresh(ex.h, cv.h, n, p(np.ones(40, np.float32))) == INVALID
        assert L.orbfe_covis_enable_refresh(ex.h, cv.h, 8, None) == INVALID
        other = orbfe.ORBextractor(*ARGS)
        try:
            assert L.orbfe_covis_enable_refresh(other.h, cv.h, 8, p(sf)) == INVALID   # a graph of another handle
        finally:
            other.close()
        cv.close()
        mp.close()
        mp, cv = S.upload(orbfe, ex, rg)                                     # enabled, fully set
        assert L.orbfe_covis_enable_refresh(ex.h, cv.h, 8, p(sf)) == INVALID   # a second call
        before = S.read_state(cv, rg)
        assert before == S.state(rg)

        kp = np.zeros(stride + 1, orbfe.KP_DTYPE)
        d = np.zeros((stride + 1, 32), np.uint8)
        feat = lambda slot, n, k=kp: L.orbfe_covis_set_features(ex.h, cv.h, slot, n, p(k), p(d))   # noqa: E731
        assert feat(-1, 2) == INVALID and feat(K, 2) == INVALID and feat(0, stride + 1) == INVALID and feat(0, -1) == INVALID
        bad_oct = kp.copy()
        bad_oct["octave"][1] = 8
        assert feat(0, 2, bad_oct) == INVALID
        bad_oct["octave"][1] = -1
        assert feat(0, 2, bad_oct) == INVALID
        assert L.orbfe_covis_set_features(ex.h, cv.h, 0, 2, None, p(d)) == INVALID
        fdev = lambda slot, n: L.orbfe_covis_set_features_device(ex.h, cv.h, slot, one, one, n, None)   # noqa: E731
        assert fdev(-1, 1) == INVALID and fdev(K, 1) == INVALID and fdev(0, stride + 1) == INVALID and fdev(0, -1) == INVALID
        assert L.orbfe_covis_set_features_device(ex.h, cv.h, 0, None, one, 1, None) == INVALID

        f3 = np.zeros(6, np.float32)
        cen = lambda slots, t=f3: L.orbfe_covis_set_centres(ex.h, cv.h, len(slots), p(arr(*slots)), p(t))   # noqa: E731
        assert cen([K]) == INVALID and cen([-1]) == INVALID and cen([1, 1]) == INVALID
        assert cen([0], np.array([0, np.nan, 0], np.float32)) == INVALID and cen([0], np.array([np.inf, 0, 0], np.float32)) == INVALID

        def seto(ids, off, slots, idx):
            return L.orbfe_covis_set_observations_indexed(ex.h, cv.h, len(ids), p(arr(*ids)), p(arr(*off)), p(arr(*slots)), p(arr(*idx)))
        assert seto([0], [0, 1], [1], [stride]) == INVALID and seto([0], [0, 1], [1], [-2]) == INVALID
        assert seto([0], [0, 1], [K], [0]) == INVALID and seto([C_], [0, 1], [1], [0]) == INVALID and seto([0, 0], [0, 1, 2], [1, 2], [0, 0]) == INVALID
        assert seto([0], [1, 0], [1], [0]) == INVALID and seto([0], [0, obs + 1], [1] * (obs + 1), [0] * (obs + 1)) == INVALID
        assert L.orbfe_covis_set_observations_indexed(ex.h, cv.h, 1, p(arr(0)), p(arr(0, 1)), p(arr(1)), None) == INVALID

        ref = lambda ids, r: L.orbfe_covis_set_ref_keyframes(ex.h, cv.h, len(ids), p(arr(*ids)), p(arr(*r)))   # noqa: E731
        assert ref([0], [K]) == INVALID and ref([0], [-2]) == INVALID and ref([C_], [0]) == INVALID and ref([-1], [0]) == INVALID
        assert ref([2, 2], [0, 1]) == INVALID

        buf, n = np.zeros(obs, np.int32), C.c_int(0)
        assert L.orbfe_covis_get_point(ex.h, cv.h, C_, C.byref(n), p(buf), p(buf), C.byref(n), None, None) == INVALID
        assert L.orbfe_covis_get_point(ex.h, cv.h, -1, C.byref(n), p(buf), p(buf), C.byref(n), None, None) == INVALID
        assert L.orbfe_covis_get_point(ex.h, cv.h, 0, None, p(buf), p(buf), C.byref(n), None, None) == INVALID

        io = orbfe.RefreshIO()
        dev = lambda n_=1, ids=one, what=3, io_=io: L.orbfe_covis_refresh_points_device(ex.h, cv.h, n_, ids, None, 0, what, C.byref(io_), None)   # noqa: E731
        assert dev(n_=0) == INVALID and dev(n_=-3) == INVALID and dev(ids=None) == INVALID and dev(what=0) == INVALID and dev(what=4) == INVALID
        longer = orbfe.RefreshIO()
        longer.struct_size += 8                                             # a caller built against a later header
        assert dev(io_=longer) == INVALID
        ids = arr(0, 1)
        host = lambda n_=2, i=p(ids), what=3: L.orbfe_covis_refresh_points(ex.h, cv.h, n_, i, what, None, None, None, None, None, None)   # noqa: E731
        assert host(n_=0) == INVALID and host(i=None) == INVALID and host(what=0) == INVALID and host(what=4) == INVALID

        assert S.read_state(cv, rg) == before                               # graph and map as they were
        mp.close()                                                          # the map goes first: every later call is refused
        assert dev() == INVALID and host() == INVALID and feat(0, 2) == INVALID and cen([0]) == INVALID and ref([0], [0]) == INVALID
        assert L.orbfe_covis_get_point(ex.h, cv.h, 0, C.byref(n), p(buf), p(buf), C.byref(n), None, None) == INVALID
    finally:
        cv.close()
        mp.close()
        ex.close()

"""The ABI of the S25 calls: the symbols, the blocks and the constants against the header, and the refusals that the arguments alone
decide, which come back before a handle or a device is looked at (the handle is NULL throughout), as test_local_map_abi.py does for
S24."""
import ctypes as C
import os
import re

import numpy as np

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbfe_covis_enable_connections", "orbfe_covis_set_connections", "orbfe_covis_get_keyframe",
         "orbfe_covis_update_connections_device", "orbfe_covis_update_connections", "orbfe_covis_add_keyframe_device",
         "orbfe_covis_add_keyframe")


def _header():
    return open(os.path.join(ROOT, "include", "orbfe.h")).read()


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in orbfe.SYMBOLS
        assert re.search(r"\b%s\(" % name, _header())


def test_constants_and_defaults_match_the_header(built):
    import orbfe
    import covis_update_ref as U
    txt = _header()
    define = lambda name: int(re.search(r"#define %s\s+(\S+)" % name, txt).group(1), 0)   # noqa: E731
    assert define("ORBFE_COVIS_MAX_CONN_STRIDE") == orbfe.COVIS_MAX_CONN_STRIDE == 4096
    assert (define("ORBFE_COVIS_STATUS_OK"), define("ORBFE_COVIS_STATUS_NO_COUNTS"), define("ORBFE_COVIS_STATUS_REFUSED")) == \
        (orbfe.COVIS_STATUS_OK, orbfe.COVIS_STATUS_NO_COUNTS, orbfe.COVIS_STATUS_REFUSED) == (U.OK, U.NO_COUNTS, U.REFUSED)
    init = re.search(r"#define ORBFE_COVIS_UPDATE_PARAMS_INIT \{\(int\)sizeof\(orbfe_covis_update_params\), ([^}]*)\}", txt).group(1)
    assert [int(v) for v in init.split(",")] == [orbfe.CovisUpdateParams().min_weight] == [U.MIN_WEIGHT] == [50]


def test_blocks_match_the_header(built):
    import orbfe
    P, IO = orbfe.CovisUpdateParams, orbfe.CovisUpdateIO
    txt = _header()
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S).group(1)   # noqa: E731
    fields = lambda name: re.findall(r"^\s*(?:const )?int \*?(\w+);", body(name), re.M)   # noqa: E731
    assert fields("orbfe_covis_update_params") == [n for n, _ in P._fields_]
    assert fields("orbfe_covis_update_io") == [n for n, _ in IO._fields_]
    assert P().struct_size == C.sizeof(P) == 8 and P.min_weight.offset == 4
    assert IO().struct_size == C.sizeof(IO) == 8 + 8 * len(orbfe.COVIS_UPDATE_IO_FIELDS) == 40
    assert [getattr(IO, n).offset for n in orbfe.COVIS_UPDATE_IO_FIELDS] == [8, 16, 24, 32]
    # what S25 must leave as it was
    assert C.sizeof(orbfe.CovisKeyframe) == 64 and C.sizeof(orbfe.LocalMapParams) == 24


def test_argument_errors_without_a_device(built):
    import orbfe
    L = orbfe.lib()
    N, B = None, C.byref
    one = 4096   # a non-NULL stand-in for device pointers and the graph: the call is refused before any of them is read
    slots, flags = np.zeros(2, np.int32), np.zeros(2, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def io_of(**over):
        k = {name: one for name in orbfe.COVIS_UPDATE_IO_FIELDS}
        k.update(over)
        return orbfe.CovisUpdateIO(**k)

    def dev(p=None, g=one, n=2, s=ptr(slots), f=ptr(flags), io=None):
        p = orbfe.CovisUpdateParams() if p is None else p
        io = io_of() if io is None else io
        return L.orbfe_covis_update_connections_device(N, B(p) if p else N, g, n, s, f, B(io) if io else N, N)

    def wrong(**k):
        p = orbfe.CovisUpdateParams()
        for name, v in k.items():
            setattr(p, name, v)
        return p

    assert dev() == INVALID                                   # everything in order but the NULL handle
    assert dev(p=False) == INVALID and dev(io=False) == INVALID and dev(g=N) == INVALID
    assert dev(p=wrong(struct_size=12)) == INVALID
    for mw in (0, -1, (1 << 20) + 1):
        assert dev(p=wrong(min_weight=mw)) == INVALID, mw
    io = io_of()
    io.struct_size -= 8
    assert dev(io=io) == INVALID
    assert dev(n=0) == INVALID and dev(s=N) == INVALID and dev(f=N) == INVALID
    for name in orbfe.COVIS_UPDATE_IO_FIELDS:
        assert dev(io=io_of(**{name: None})) == INVALID, name

    out_s, out_w, cnt, st = np.zeros(8, np.int32), np.zeros(8, np.int32), C.c_int(7), C.c_int(7)

    def host(p=None, g=one, slot=0, os_=ptr(out_s), ow=ptr(out_w), c=B(cnt), s=B(st)):
        p = orbfe.CovisUpdateParams() if p is None else p
        return L.orbfe_covis_update_connections(N, B(p) if p else N, g, slot, 0, os_, ow, c, s)
    assert host() == INVALID and host(p=False) == INVALID and host(p=wrong(struct_size=4)) == INVALID and host(p=wrong(min_weight=0)) == INVALID
    assert host(g=N) == INVALID and host(os_=N) == INVALID and host(ow=N) == INVALID and host(c=N) == INVALID and host(s=N) == INVALID
    assert cnt.value == 7 and st.value == 7 and not out_s.any()

    rec = orbfe.CovisKeyframe(slot=0, mn_id=0)
    add = lambda r=rec, g=one, ids=one, n=4, a=one, s=one: L.orbfe_covis_add_keyframe_device(N, g, B(r) if r else N, ids, n, a, s, N)   # noqa: E731
    assert add() == INVALID and add(r=False) == INVALID and add(g=N) == INVALID and add(ids=N) == INVALID and add(n=-1) == INVALID
    assert add(a=N) == INVALID and add(s=N) == INVALID
    short = orbfe.CovisKeyframe(slot=0, mn_id=0)
    short.struct_size = 56
    assert add(r=short) == INVALID

    hostadd = lambda r=rec, g=one, a=one, s=B(st): L.orbfe_covis_add_keyframe(N, g, B(r) if r else N, a, s)   # noqa: E731
    assert hostadd() == INVALID and hostadd(r=False) == INVALID and hostadd(g=N) == INVALID and hostadd(s=N) == INVALID and hostadd(r=short) == INVALID
    assert st.value == 7

    assert L.orbfe_covis_enable_connections(N, one, 8) == INVALID and L.orbfe_covis_enable_connections(one, N, 8) == INVALID
    assert L.orbfe_covis_set_connections(N, one, 0, N, N, N, N) == INVALID and L.orbfe_covis_set_connections(one, N, 0, N, N, N, N) == INVALID
    assert L.orbfe_covis_get_keyframe(N, one, 0, B(rec), one, one, N, N, N) == INVALID
    assert L.orbfe_covis_get_keyframe(one, N, 0, B(rec), one, one, N, N, N) == INVALID

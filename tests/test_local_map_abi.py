"""The ABI of the S24 calls: the symbols, the blocks and the constants against the header, and the refusals that the arguments alone
decide, which come back before a handle or a device is looked at (the handle is NULL throughout), as test_track_inertial_abi.py does
for S23."""
import ctypes as C
import os
import re

import numpy as np

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("orbfe_covis_create", "orbfe_covis_destroy", "orbfe_covis_set_keyframes", "orbfe_covis_set_observations",
         "orbfe_update_local_map_batch_device", "orbfe_update_local_map", "orbfe_frame_points_batch_device")


def test_symbols_exported(built):
    import orbfe
    L = orbfe.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in orbfe.SYMBOLS


def test_constants_match_the_header(built):
    import orbfe
    import local_map_ref as R
    txt = open(os.path.join(ROOT, "include", "orbfe.h")).read()
    define = lambda name: int(re.search(r"#define %s\s+(\S+)" % name, txt).group(1), 0)   # noqa: E731
    assert define("ORBFE_COVIS_MAX_COVISIBLE") == orbfe.COVIS_MAX_COVISIBLE == R.MAX_COVISIBLE == 16
    assert define("ORBFE_LOCAL_KF_MAX") == orbfe.LOCAL_KF_MAX == R.LOCAL_KF_MAX == 4 * 64 + 32
    assert define("ORBFE_NO_POINT") == orbfe.NO_POINT == R.NO_POINT == 0x7fffffff
    assert define("ORBFE_LOCAL_MAP_BLOCK") == orbfe.LOCAL_MAP_BLOCK and orbfe.LOCAL_MAP_BLOCK % 64 == 0
    assert define("ORBFE_LOCAL_MAP_VOTE_TABLE") == orbfe.LOCAL_MAP_VOTE_TABLE
    init = re.search(r"#define ORBFE_LOCAL_MAP_PARAMS_INIT \{\(int\)sizeof\(orbfe_local_map_params\), ([^}]*)\}", txt).group(1)
    p = orbfe.LocalMapParams()
    assert [int(v) for v in init.split(",")] == [p.max_local_kf, p.n_covisible, p.n_temporal, p.inertial, p.mark_voters_seen]


def test_blocks_match_the_header(built):
    import orbfe
    K, P, IO = orbfe.CovisKeyframe, orbfe.LocalMapParams, orbfe.LocalMapIO
    assert K().struct_size == C.sizeof(K) == 64
    assert [getattr(K, n).offset for n in ("slot", "mn_id", "bad", "parent", "prev", "n_features", "n_covisible", "n_children", "reserved",
                                           "point_ids", "covisible", "children")] == [4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56]
    assert P().struct_size == C.sizeof(P) == 24 and (P.max_local_kf.offset, P.mark_voters_seen.offset) == (4, 20)
    assert IO().struct_size == C.sizeof(IO) == 8 + 8 * len(orbfe.LOCAL_MAP_IO_FIELDS) == 72
    assert (IO.d_vote_ids.offset, IO.d_last_kf.offset, IO.d_ids_out.offset, IO.d_vote_ids_out.offset) == (8, 24, 32, 64)


def test_argument_errors_without_a_device(built):
    import orbfe
    L = orbfe.lib()
    N, B = None, C.byref
    one = 4096   # a non-NULL stand-in for device pointers, the graph and the map: the call is refused before any of them is read

    def io_of(**over):
        k = {name: one for name in orbfe.LOCAL_MAP_IO_FIELDS}
        k.update(over)
        return orbfe.LocalMapIO(**k)

    def bat(p=None, batch=3, vote_stride=200, covis=one, M=70, io=None):
        p = orbfe.LocalMapParams() if p is None else p
        io = io_of() if io is None else io
        return L.orbfe_update_local_map_batch_device(N, B(p) if p else N, batch, vote_stride, covis, M, B(io) if io else N, N)

    def wrong(**k):
        p = orbfe.LocalMapParams()
        for name, v in k.items():
            setattr(p, name, v)
        return p

    # every argument in order, a NULL handle: INVALID_ARG at the end of the ladder, and only there
    assert bat() == INVALID
    assert bat(p=False) == INVALID and bat(io=False) == INVALID
    assert bat(p=wrong(struct_size=20)) == INVALID
    io = io_of()
    io.struct_size -= 8
    assert bat(io=io) == INVALID
    for k in (dict(max_local_kf=0), dict(max_local_kf=65), dict(n_covisible=-1), dict(n_covisible=17), dict(n_temporal=-1),
              dict(n_temporal=33)):
        assert bat(p=wrong(**k)) == INVALID, k
    assert bat(batch=0) == INVALID and bat(vote_stride=0) == INVALID and bat(M=0) == INVALID and bat(covis=N) == INVALID
    for name in orbfe.LOCAL_MAP_IO_FIELDS:
        if name != "d_vote_ids_out":
            assert bat(io=io_of(**{name: None})) == INVALID, name
    assert bat(io=io_of(d_vote_ids_out=None)) == INVALID                      # optional: what is left to refuse is the NULL handle
    assert bat(p=wrong(inertial=0), io=io_of(d_last_kf=None)) == INVALID      # (and the last key frame is not read when not inertial)

    # ---- the single-frame call ----
    votes, ids, kfs = np.zeros(8, np.int32), np.zeros(70, np.int32), np.zeros(orbfe.LOCAL_KF_MAX, np.int32)
    n1, n2 = C.c_int(7), C.c_int(7)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def host(p=None, n=8, v=ptr(votes), covis=one, M=70, ids_=ptr(ids), np_=B(n1), kfs_=ptr(kfs), nk_=B(n2)):
        p = orbfe.LocalMapParams() if p is None else p
        return L.orbfe_update_local_map(N, B(p) if p else N, n, v, 0, covis, M, ids_, np_, kfs_, nk_, N)
    assert host() == INVALID and host(p=False) == INVALID and host(p=wrong(struct_size=28)) == INVALID and host(p=wrong(max_local_kf=0)) == INVALID
    assert host(n=-1) == INVALID and host(v=N) == INVALID and host(covis=N) == INVALID and host(M=0) == INVALID
    assert host(ids_=N) == INVALID and host(np_=N) == INVALID and host(kfs_=N) == INVALID and host(nk_=N) == INVALID
    assert host(n=0, v=N) == INVALID                                          # no voters is valid: the NULL handle refuses it
    assert n1.value == 7 and n2.value == 7 and not ids.any()

    # ---- the graph and the companion ----
    out = C.c_void_p(5)
    assert L.orbfe_covis_create(N, one, 8, 8, 8, 8, B(out)) == INVALID and L.orbfe_covis_create(one, N, 8, 8, 8, 8, B(out)) == INVALID
    assert L.orbfe_covis_set_keyframes(N, one, 0, N) == INVALID and L.orbfe_covis_set_keyframes(one, N, 0, N) == INVALID
    assert L.orbfe_covis_set_observations(N, one, 0, N, N, N) == INVALID and L.orbfe_covis_set_observations(one, N, 0, N, N, N) == INVALID
    L.orbfe_covis_destroy(N)
    fp = lambda h=N, m=one, b=2, s=200, M=70, ptrs=(one,) * 5: L.orbfe_frame_points_batch_device(h, m, b, s, M, *ptrs, N)   # noqa: E731
    assert fp() == INVALID and fp(m=N) == INVALID and fp(b=0) == INVALID and fp(s=0) == INVALID and fp(M=0) == INVALID
    for k in range(5):
        assert fp(ptrs=tuple(N if j == k else one for j in range(5))) == INVALID

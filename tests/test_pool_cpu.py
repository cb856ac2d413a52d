"""The multi-device pool (orbfe_pool_*) without a GPU: its sharding rule is shard.py's, every argument error is refused before
the HIP runtime is asked anything, a valid pool on a box without a GPU fails loudly, and tests/cpp/test_pool.cpp (the
adaptor's FramePool) compiles and links against liborbfe.so."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "test_pool.bin")
ARGS = (600, 24000, 1.2, 6, 20, 7, 376, 240)


def build_program():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_pool.cpp"),
                           "-o", BIN, "-L", CSRC, "-lorbfe", "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"])
    return BIN


def test_shard_range_equals_shard_py(built):
    import orbfe
    from orbfe.shard import shard_range
    for n_frames in range(0, 301):
        for n_members in range(1, 17):
            prev = 0
            for k in range(n_members):
                lo, hi = orbfe.shard_range(n_frames, k, n_members)
                assert (lo, hi) == shard_range(n_frames, k, n_members), (n_frames, k, n_members)
                assert lo == prev and lo <= hi, (n_frames, k, n_members)  # ordered, disjoint, no gap
                prev = hi
            assert prev == n_frames


def test_shard_range_refuses_bad_arguments(built):
    import orbfe
    L = orbfe.lib()
    lo, hi = C.c_int(), C.c_int()
    assert L.orbfe_shard_range(10, 0, 0, C.byref(lo), C.byref(hi)) == 1
    assert L.orbfe_shard_range(10, 2, 2, C.byref(lo), C.byref(hi)) == 1
    assert L.orbfe_shard_range(10, -1, 2, C.byref(lo), C.byref(hi)) == 1
    assert L.orbfe_shard_range(-1, 0, 2, C.byref(lo), C.byref(hi)) == 1
    assert L.orbfe_shard_range(10, 0, 2, None, C.byref(hi)) == 1


def _create(L, prm, devs, slots=3, slot_frames=8, n=None):
    import orbfe  # noqa: F401
    arr = (C.c_int * max(1, len(devs)))(*devs) if devs is not None else None
    h = C.c_void_p()
    rc = L.orbfe_pool_create(C.byref(prm) if prm is not None else None, arr, len(devs) if n is None else n, slots, slot_frames, C.byref(h))
    assert rc != 0 or h.value, "a successful create returns a pool"
    if rc == 0:
        L.orbfe_pool_destroy(h)
    return rc


def test_pool_create_refuses_bad_arguments(built):
    import orbfe
    L = orbfe.lib()
    prm = orbfe.Params(*ARGS, 0, 16)
    h = C.c_void_p()
    assert L.orbfe_pool_create(None, (C.c_int * 1)(0), 1, 3, 8, C.byref(h)) == 1
    assert L.orbfe_pool_create(C.byref(prm), None, 1, 3, 8, C.byref(h)) == 1
    assert L.orbfe_pool_create(C.byref(prm), (C.c_int * 1)(0), 1, 3, 8, None) == 1
    assert _create(L, prm, [0], n=0) == 1
    assert _create(L, prm, [0] * 17) == 1
    assert _create(L, prm, [0, -1]) == 1
    assert _create(L, prm, [0], slots=1) == 1
    assert _create(L, prm, [0], slots=65) == 1
    assert _create(L, prm, [0], slot_frames=0) == 1
    assert _create(L, prm, [0], slot_frames=17) == 1  # > max_batch


def test_every_pool_call_refuses_a_null_pool(built):
    import orbfe
    L = orbfe.lib()
    tp = orbfe.TrackParams()
    L.orbfe_pool_destroy(None)
    assert L.orbfe_pool_size(None) == 0
    assert L.orbfe_pool_member(None, 0) is None
    assert L.orbfe_pool_member_frames(None, 0) == 0
    assert L.orbfe_pool_last_error(None) == b""
    assert L.orbfe_pool_extract(None, None, 376, 1, None, None, None, None) == 1
    assert L.orbfe_pool_enable_track(None, 100, 10) == 1
    assert L.orbfe_pool_map_update(None, 0, None, None, None) == 1
    assert L.orbfe_pool_track(None, None, 376, 1, C.byref(tp), None, 0, None, None, None, None, None, None, None) == 1


def test_pool_create_fails_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import orbfe
    L = orbfe.lib()
    assert _create(L, orbfe.Params(*ARGS, 0, 16), [0, 0]) == 3  # ORBFE_ERR_NO_DEVICE: no CPU fallback exists
    with pytest.raises(orbfe.OrbfeError) as ei:
        orbfe.Pool(ARGS, [0], slot_frames=8, max_batch=16)
    assert ei.value.code == 3


def test_pool_program_links(built):
    out = subprocess.check_output([build_program()]).decode()
    assert "gfx950" in out and "host_only=1" in out

"""orbfe_fuse_search_keyframes / orbfe_fuse_select: declared in include/orbfe.h, exported by the built library; the host-only
select (the strict "<" scan of src/ORBmatcher.cc:824-832 over a candidate list) through ctypes on hand-made lists; and the
compiler's resource report of the batched kernel (no scratch memory).  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 2


def test_declared_and_exported(built):
    import orbfe
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "orbfe.h")).read(), flags=re.S)
    L = orbfe.lib()
    for name in ("orbfe_fuse_search_keyframes", "orbfe_fuse_select"):
        assert re.search(r"\b%s\s*\(" % name, txt), name + " is not declared in include/orbfe.h"
        assert hasattr(L, name), "liborbfe.so does not export " + name
        assert name in orbfe.SYMBOLS
    # a refusal that needs no GPU: no handle
    assert L.orbfe_fuse_search_keyframes(None, 0, None, None, None, 0, None, None, 10.0, None, None, 0, None, None) == INVALID_ARG


def _select(L, cand, count, cap, kf_desc, mp_desc):
    cand = np.ascontiguousarray(cand, np.int32)
    kf_desc = np.ascontiguousarray(kf_desc, np.uint8)
    bi, bd = C.c_int(12345), C.c_int(12345)
    rc = L.orbfe_fuse_select(cand.ctypes.data_as(C.c_void_p), count, cap, kf_desc.ctypes.data_as(C.c_void_p), len(kf_desc),
                             np.ascontiguousarray(mp_desc, np.uint8).ctypes.data_as(C.c_void_p), C.byref(bi), C.byref(bd))
    return rc, bi.value, bd.value


def test_fuse_select_on_hand_made_lists(built):
    import orbfe
    L = orbfe.lib()
    rng = np.random.default_rng(1)
    mp = rng.integers(0, 256, 32, dtype=np.uint8)
    kf = np.tile(mp, (6, 1))
    kf[0, 0] ^= 0x0f   # 4 bits away
    kf[1, 3] ^= 0x03   # 2 bits
    kf[2, 7] ^= 0x81   # 2 bits: ties with row 1
    kf[3, 9] ^= 0xff   # 8 bits
    kf[4, 1] ^= 0x01   # 1 bit
    kf[5] = ~mp        # 256 bits: never below the initial bestDist
    # ties keep the earlier entry of the LIST (the strict "<" of :828), whatever the feature indices are
    assert _select(L, [0, 1, 2, 3], 4, 4, kf, mp) == (OK, 1, 2)
    assert _select(L, [0, 2, 1, 3], 4, 4, kf, mp) == (OK, 2, 2)
    assert _select(L, [3, 2, 1, 4], 4, 8, kf, mp) == (OK, 4, 1)
    assert _select(L, [3, -1, -1, -1], 1, 4, kf, mp) == (OK, 3, 8)      # entries beyond the count are not read
    assert _select(L, [5], 1, 1, kf, mp) == (OK, -1, 256)               # a distance of 256 is not "< 256"
    for d in (kf[0], kf[3]):  # == the plain restatement with another descriptor
        dist = [int(np.unpackbits(kf[i] ^ d).sum()) for i in (4, 1, 0, 3)]
        want = (OK, (4, 1, 0, 3)[int(np.argmin(dist))], min(dist))
        assert _select(L, [4, 1, 0, 3], 4, 4, kf, d) == want
    # an empty list
    assert _select(L, [-1, -1, -1, -1], 0, 4, kf, mp) == (OK, -1, 256)
    assert _select(L, [-1], 0, 0, kf, mp) == (OK, -1, 256)
    # a truncated list: the caller must search that pair again
    assert _select(L, [0, 1], 3, 2, kf, mp)[0] == UNSUPPORTED
    assert _select(L, [0], 1, 0, kf, mp)[0] == UNSUPPORTED
    # an index outside the key frame
    assert _select(L, [0, 6], 2, 4, kf, mp)[0] == INVALID_ARG
    assert _select(L, [0, -1], 2, 4, kf, mp)[0] == INVALID_ARG
    assert _select(L, [0, 1], 2, 17, kf, mp)[0] == INVALID_ARG         # cand_cap outside [0, 16]
    # the Python wrapper
    assert orbfe.fuse_select([0, 1, 2, 3], 4, 4, kf, mp) == (1, 2)
    with pytest.raises(orbfe.OrbfeError) as e:
        orbfe.fuse_select([0, 1], 3, 2, kf, mp)
    assert e.value.code == UNSUPPORTED


def test_batched_kernel_uses_no_scratch(tmp_path):
    """fuse_neighbors_kernel keeps its candidate sink in registers (compare-select insertion, no array indexed at run time):
    ScratchSize 0 in the compiler's resource report for gfx950, for the form with and the form without candidate lists, and
    the single-target kernels that share the walk keep theirs at 0 too."""
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "--cuda-device-only", "-c", os.path.join(CSRC, "kernels_match_kf.hip"), "-o", str(tmp_path / "k.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    funcs, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = funcs.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/(?:lane|block)\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    batched = {k: v for k, v in funcs.items() if "fuse_neighbors_kernel" in k}
    single = {k: v for k, v in funcs.items() if "fuse_search_kernel" in k}
    assert len(batched) == 2 and len(single) == 2, sorted(funcs)
    for name, r in list(batched.items()) + list(single.items()):
        assert r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, (name, r)  # at least four waves per SIMD

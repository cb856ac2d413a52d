"""The batched form of the SearchByProjection resolve pass must fit on a CU beside seven blocks of the FAST kernel
(256 threads, 56 VGPRs allocated, 16,908 B of LDS each): at most 120 VGPRs (unified with AGPRs), no scratch memory and
at most 163,840 - 7 * 16,908 = 45,484 B of LDS.  Read from the compiler's resource report for gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# proj_resolve_kernel<LDS, 256, kResN, DESC = false, IMG = false, FB>: the two instantiations proj_launch picks for
# launches of at least kResolveBatchedMinFrames frames (claim tables in LDS / in global memory)
BATCHED = re.compile(r"proj_resolve_kernelILb([01])ELi256ELi2048ELb0ELb0ELi32EE")  # FB = kFbBatched = 32


def _resource_report(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "--cuda-device-only", "-c", os.path.join(CSRC, "kernels_match_proj.hip"), "-o", str(tmp_path / "k.o"),
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
    return funcs


def test_batched_resolve_fits_beside_seven_fast_blocks(tmp_path):
    funcs = _resource_report(tmp_path)
    batched = {k: v for k, v in funcs.items() if BATCHED.search(k)}
    assert len(batched) == 2, sorted(funcs)
    for name, r in batched.items():
        vgprs = r["VGPRs"] + r.get("AGPRs", 0)
        assert vgprs <= 120, (name, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] <= 163840 - 7 * 16908, (name, r)

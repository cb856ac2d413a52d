"""Every fast_blur_kernel instantiation of the shipped library (with and without the fused level build) must keep the
footprint tests/test_resolve_budget.py rests on -- 256-thread blocks of at most 56 VGPRs, no scratch memory and at most
16,908 B of LDS, eight waves per SIMD -- so that the batched resolve block still fits beside seven of them.  Read from the
compiler's resource report for gfx950; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# fast_blur_kernel<MODE = 3, BUILD>: one FAST launch over all levels (BUILD = false) / one per level that also writes the
# next unblurred level (BUILD = true)
SHIPPED = re.compile(r"fast_blur_kernelILi3ELb([01])EE")


def _resource_report(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "--cuda-device-only", "-c", os.path.join(CSRC, "kernels_fast.hip"), "-o", str(tmp_path / "k.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    funcs, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = funcs.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return funcs


def test_fast_kernels_keep_their_footprint(tmp_path):
    funcs = _resource_report(tmp_path)
    fast = {k: v for k, v in funcs.items() if "fast_blur_kernel" in k}
    # the shipped library holds exactly the two MODE 3 instantiations (the truncated ones exist in the ablation build only)
    assert len(fast) == 2 and all(SHIPPED.search(k) for k in fast), sorted(funcs)
    assert {SHIPPED.search(k).group(1) for k in fast} == {"0", "1"}
    for name, r in fast.items():
        print(name, r)
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 56, (name, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] <= 16908, (name, r)
        assert r["Occupancy"] == 8, (name, r)

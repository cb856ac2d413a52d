"""Resource budgets of the three block-per-call solver kernels, read from the compiler's resource report for gfx950; no GPU needed.
One 256-thread block is one wave a SIMD, so 512 registers a lane are there to be used; the ceilings are the figures the kernels had
before the wave-walked run moved to csrc/block_tree.h.
pose_imu_kernel (S19) uses no scratch memory: no thread owns a run of edges (runs are walked by the wave, the binary-counter stack lives
in lane registers), the 15 x 15 factorisation is spread over a wave with compile-time register indices, and a lane's own entry of an
array is picked by masking bit patterns, not by a select chain the compiler would turn into an indexed load.
initial_ba_kernel (S17) uses no scratch memory: a point's 27-double linearisation is held in registers for runs of at most two points
and parked in the arena beyond, and the binary-counter stack of the parked path lives in lane registers with compile-time indices.
pose_opt_kernel (S14) keeps the figures it has had since its tree helpers first moved to a header -- 256 VGPRs, 135 AGPRs, 2304 bytes of
scratch a lane (the dynamically indexed stack of its thread-owned runs), 1808 bytes of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_v1.0_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
POSE_OPT = dict(VGPRs=256, AGPRs=135, ScratchSize=2304, LDS=1808)


def _resource_report(tmp_path, source):
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "--cuda-device-only", "-c", os.path.join(CSRC, source), "-o", str(tmp_path / "k.o"),
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


def _kernel(funcs, name):
    hit = {k: v for k, v in funcs.items() if name in k}
    assert len(hit) == 1, sorted(funcs)
    return next(iter(hit.values()))


def test_pose_imu_kernel_uses_no_scratch(tmp_path):
    funcs = _resource_report(tmp_path, "kernels_poseimu.hip")
    hit = {k: v for k, v in funcs.items() if "pose_imu_kernel" in k}
    assert len(hit) == 1, sorted(funcs)
    r = next(iter(hit.values()))
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 512, r          # one 256-thread block: one wave a SIMD


def test_initial_ba_kernel_uses_no_scratch(tmp_path):
    r = _kernel(_resource_report(tmp_path, "kernels_initial_ba.hip"), "initial_ba_kernel")
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 512, r          # one 256-thread block: one wave a SIMD


def test_pose_opt_kernel_is_the_parents(tmp_path):
    r = _kernel(_resource_report(tmp_path, "kernels_poseopt.hip"), "pose_opt_kernel")
    assert (r["VGPRs"], r["AGPRs"], r["ScratchSize"], r["LDS Size"]) == (POSE_OPT["VGPRs"], POSE_OPT["AGPRs"], POSE_OPT["ScratchSize"],
                                                                       POSE_OPT["LDS"]), r

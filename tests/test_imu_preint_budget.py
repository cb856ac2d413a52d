"""Resource budget of the two S22 kernels (csrc/kernels_imu_preint.hip), read from the compiler's resource report for gfx950 as
test_solver_budget.py reads it; no GPU needed.  Everything indexed at run time -- the records, A, B, the staged steps, the 9 x 9
matrices of the factorisation and of the Jacobi rounds -- lives in LDS, so neither kernel uses scratch memory or spills; a block is one
wave of 64 lanes, so its LDS is what bounds the waves of a CU: the static 64 KiB a block may declare is far away, and so is 160 KiB a CU
divided by the 8 blocks a CU's SIMDs can hold at the kernel's register count."""
import pytest

from test_solver_budget import _kernel, _resource_report

LDS_STATIC_LIMIT = 64 * 1024
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _resource_report(tmp_path_factory.mktemp("imu_preint"), "kernels_imu_preint.hip")


@pytest.mark.parametrize("name", ("imu_frame_kernel", "imu_reintegrate_kernel"))
def test_imu_preint_kernels_use_no_scratch(report, name):
    r = _kernel(report, name)
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 512, r          # one 64-thread block: one wave
    assert r["LDS Size"] <= LDS_STATIC_LIMIT and 8 * r["LDS Size"] <= LDS_PER_CU, r

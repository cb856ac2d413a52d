"""Resource budget of the two S23 kernels, read from the compiler's resource report for gfx950 as test_solver_budget.py reads it; no
GPU needed.  track_frustum_gather_kernel (csrc/kernels_frustum.hip) is a thread per id slot: the frustum it builds from the predicted
state is block-uniform and the record frustum_point fills never leaves registers.  track_stats_kernel (csrc/kernels_track_inertial.hip)
holds one counter per wave in LDS.  Neither indexes a private array at run time, so neither may use scratch memory or spill."""
import pytest

from test_solver_budget import _kernel, _resource_report

KERNELS = (("kernels_frustum.hip", "track_frustum_gather_kernel"), ("kernels_track_inertial.hip", "track_stats_kernel"))


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    return {unit: _resource_report(tmp_path_factory.mktemp(unit.split(".")[0]), unit) for unit, _ in KERNELS}


@pytest.mark.parametrize("unit,name", KERNELS, ids=[k[1] for k in KERNELS])
def test_track_inertial_kernels_use_no_scratch(reports, unit, name):
    r = _kernel(reports[unit], name)
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 128, r      # at 128 registers a lane a SIMD's 512 hold four waves
    assert r["LDS Size"] <= 64, r                         # four wave counters, or nothing

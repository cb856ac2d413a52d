"""Resource budget of every kernel of csrc/kernels_covis_refresh.hip (SPEC DECISION S26), read from the compiler's resource report for
gfx950 as test_covis_update_budget.py reads it; no GPU needed.  None of them indexes a private array at run time, so none may use
scratch memory or spill a register of either kind, and none may need more than 64 VGPRs: the unit runs eight waves a SIMD beside the
tracking chains.  The wave kernel holds a descriptor in 8 registers and uses no LDS at all; the rest kernel's LDS is one int per
observer of the longest list a graph can hold (obs_stride <= 4096) and a few words of block state."""
import pytest

from test_solver_budget import _kernel, _resource_report

UNIT = "kernels_covis_refresh.hip"
KERNELS = ("refresh_wave_kernel", "refresh_rest_kernel", "refresh_set_features_kernel", "refresh_scatter_centres_kernel",
           "refresh_scatter_indices_kernel", "refresh_scatter_ref_kernel", "refresh_index_added_kernel")
STATE = 64             # bytes: 4 waves x 8 for the reduction's keys, two counters


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _resource_report(tmp_path_factory.mktemp("covis_refresh"), UNIT)


def test_the_list_names_every_kernel_of_the_unit(report):
    own = [k for k in report if "fill_kernel" not in k]        # (match_common.h's, compiled into every unit that includes it)
    assert len(own) == len(KERNELS) and all(sum(name in k for k in own) == 1 for name in KERNELS), sorted(report)


@pytest.mark.parametrize("name", KERNELS)
def test_covis_refresh_kernels_use_no_scratch_and_spill_nothing(report, name):
    r = _kernel(report, name)
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r            # eight waves a SIMD
    lists = 4 * 4096 if name == "refresh_rest_kernel" else 0
    assert r["LDS Size"] <= lists + STATE, r

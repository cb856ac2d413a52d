"""Resource budget of every kernel of csrc/kernels_covis_update.hip (SPEC DECISION S25), read from the compiler's resource report for
gfx950 as test_solver_budget.py reads it; no GPU needed.  None of them indexes a private array at run time, so none may use scratch
memory or spill a register of either kind.  The counting kernel's LDS is its table: two ints (key, count) for each of the
2 x ORBFE_LOCAL_MAP_VOTE_TABLE entries; everything else is a few words of block state (at most a 64-bit key and a slot per wave)."""
import pytest

from test_solver_budget import _kernel, _resource_report

UNIT = "kernels_covis_update.hip"
KERNELS = ("covis_count_kernelILb0E", "covis_count_kernelILb1E", "covis_select_kernel", "covis_apply_kernel", "covis_add_keyframe_kernel",
           "covis_scatter_connections_kernel")
STATE = 128            # bytes: 4 waves x (8 + 4) for the selection's reduction, and fewer than 16 ints of flags and counts


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _resource_report(tmp_path_factory.mktemp("covis_update"), UNIT)


def test_the_list_names_every_kernel_of_the_unit(report):
    own = [k for k in report if "fill_kernel" not in k]        # (match_common.h's, compiled into every unit that includes it)
    assert len(own) == len(KERNELS) and all(sum(name in k for k in own) == 1 for name in KERNELS), sorted(report)


@pytest.mark.parametrize("name", KERNELS)
def test_covis_update_kernels_use_no_scratch_and_spill_nothing(report, name):
    import orbfe
    r = _kernel(report, name)
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r            # eight waves a SIMD
    table = 2 * 4 * 2 * orbfe.LOCAL_MAP_VOTE_TABLE if name == "covis_count_kernelILb0E" else 0
    assert r["LDS Size"] <= table + STATE, r

"""Resource budget of every kernel of csrc/kernels_local_map.hip (SPEC DECISION S24), read from the compiler's resource report for
gfx950 as test_solver_budget.py reads it; no GPU needed.  None of them indexes a private array at run time, so none may use scratch
memory or spill a register of either kind (the project's rule since S17).  The vote kernel's LDS is its table: three ints for each of
the 2 x ORBFE_LOCAL_MAP_VOTE_TABLE entries, and a few hundred bytes of selection state."""
import pytest

from test_solver_budget import _kernel, _resource_report

UNIT = "kernels_local_map.hip"
KERNELS = ("local_votes_kernelILb0E", "local_votes_kernelILb1E", "local_list_kernel", "local_points_kernel", "covis_init_kernel",
           "covis_scatter_keyframes_kernel", "covis_scatter_observations_kernel", "frame_points_kernel")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _resource_report(tmp_path_factory.mktemp("local_map"), UNIT)


def test_the_list_names_every_kernel_of_the_unit(report):
    own = [k for k in report if "fill_kernel" not in k]        # (match_common.h's, compiled into every unit that includes it)
    assert len(own) == len(KERNELS) and all(sum(name in k for k in own) == 1 for name in KERNELS), sorted(report)


@pytest.mark.parametrize("name", KERNELS)
def test_local_map_kernels_use_no_scratch_and_spill_nothing(report, name):
    import orbfe
    r = _kernel(report, name)
    print(name, r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 64, r            # eight waves a SIMD
    table = 3 * 4 * 2 * orbfe.LOCAL_MAP_VOTE_TABLE if name == "local_votes_kernelILb0E" else 0
    assert r["LDS Size"] <= table + 4 * (2 * orbfe.LOCAL_KF_MAX + 1) + 512, r   # static LDS; the list kernel adds kf_capacity bits at launch

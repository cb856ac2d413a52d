"""Resource budget of pose_prev_kernel (SPEC DECISION S20), read from the compiler's resource report for gfx950 exactly as
test_solver_budget.py reads it; no GPU needed.  One 256-thread block is one wave a SIMD, so 512 registers a lane are there to be used.
The kernel uses no scratch memory and spills no vector register: everything indexed at run time -- the Jacobian blocks, the edge
Hessians, the 30 x 30 system and its factor, the matrices of the marginalisation, and the one copy of the state -- lives in LDS, which
takes dynamic indices without scratch; the tree over the mono edges is S19's."""
from test_solver_budget import _kernel, _resource_report

LDS_LIMIT = 64 * 1024   # a statically declared __shared__ block


def test_pose_prev_kernel_uses_no_scratch(tmp_path):
    r = _kernel(_resource_report(tmp_path, "kernels_poseimu_prev.hip"), "pose_prev_kernel")
    print(r)
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 512, r          # one 256-thread block: one wave a SIMD
    assert r["LDS Size"] <= LDS_LIMIT, r


def test_the_new_file_leaves_pose_imu_kernel_alone(tmp_path):
    """kernels_poseimu.hip still holds exactly one pose_imu_kernel, and the new kernel's name does not contain that substring"""
    funcs = _resource_report(tmp_path, "kernels_poseimu_prev.hip")
    assert not [k for k in funcs if "pose_imu_kernel" in k] and len([k for k in funcs if "pose_prev_kernel" in k]) == 1, sorted(funcs)

"""Resource budgets of the rigid-body kernels (claymore_amd/csrc/mpm_rigid_body.hpp), read from the kernel descriptors and the
metadata of the assembly the build flags produce (CPU only, in the manner of tests/test_collider_loads_isa.py): grid_update_body_kernel - the
load frame with the stores -, the frame's read-only entry point that serves mpm_collider_loads with a body installed
(collider_loads_kernel<BodyArgs>), body_step_kernel and the contact map's BodyArgs instantiation cross-compile for gfx950 with no scratch and no spilled register, and their LDS is the stated size.  Nothing is asserted
about which instructions appear."""
import pytest

from test_collider_loads_isa import descriptor
from test_isa_invariants import device_asm  # noqa: F401  (the module-scoped cross-compile fixture)

KERNELS = {"grid_update_body_kernel<BodyArgs>": "_ZN3mpm23grid_update_body_kernelINS_8BodyArgsEEE",
           "collider_loads_kernel<BodyArgs>": "_ZN3mpm21collider_loads_kernelINS_8BodyArgsEEE",
           "body_step_kernel": "_ZN3mpm16body_step_kernelE",
           "collider_contacts_kernel<BodyArgs>": "_ZN3mpm24collider_contacts_kernelINS_8BodyArgsEEE"}
LDS = {"grid_update_body_kernel<BodyArgs>": 4 * 6 * 8 * 8, "collider_loads_kernel<BodyArgs>": 4 * 6 * 8 * 8,                     # a wave's [row][8] doubles, four waves
       "body_step_kernel": (16 + 1) * 6 * 8 * 8,                                                                         # 16 waves' sums and the totals
       "collider_contacts_kernel<BodyArgs>": 0}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_rigid_body_kernels_use_no_scratch_and_spill_nothing(device_asm, name):
    d, meta = descriptor(device_asm, KERNELS[name])
    print(name, "vgprs", meta.get("vgpr_count"), "sgprs", meta.get("sgpr_count"), "lds", d[".amdhsa_group_segment_fixed_size"])
    assert d[".amdhsa_private_segment_fixed_size"] == 0, name
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
    assert meta["vgpr_count"] <= 128, (name, meta["vgpr_count"])                            # four waves a SIMD, as the load kernels
    assert d[".amdhsa_group_segment_fixed_size"] == LDS[name]

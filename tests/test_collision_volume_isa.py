"""Resource budgets of the volume collider's kernels (claymore_amd/csrc/mpm_collision_volume.hpp, mpm_kernels.hpp), read from the
directives and the text of the assembly the build flags produce (CPU only, as tests/test_grid_update_isa.py does): the two grid-update frames
instantiated for VolumeColliderArgs keep the collider kernels' budget - no scratch, at most 80 VGPRs -, and the kernel that builds a table
from a mesh uses no scratch and the LDS its comment states."""
import pytest

from test_isa_invariants import device_asm, directive, instr, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

VGPR_STEP = 80          # six waves per SIMD: tests/test_grid_update_isa.py's budget of every collider kernel
GRID = {"stand-alone": "_ZN3mpm27grid_update_collider_kernelINS_18VolumeColliderArgsEEE", "carry": "_ZN3mpm17carry_grid_kernelILb1ENS_18VolumeColliderArgsEEE"}
BUILD = "_ZN3mpm27collision_mesh_table_kernelE"    # the level-set field's kernel too (claymore_amd/csrc/mpm_collision_mesh.hpp)


@pytest.mark.parametrize("name", sorted(GRID))
def test_volume_grid_kernels_use_no_scratch_and_at_most_80_vgprs(device_asm, name):
    """Built: 74 / 75 VGPRs, 100 / 100 SGPRs (stand-alone / carry) - the slot loop is a real loop over the kernel arguments, so the volume branch shares its
    registers with the shapes' and the heightfield's.  The eight corner loads are 16-byte global loads."""
    body = kernel_body(device_asm, GRID[name])
    vgpr, scratch = directive(body, ".amdhsa_next_free_vgpr"), directive(body, ".amdhsa_private_segment_fixed_size")
    print(name, "vgpr", vgpr, "sgpr", directive(body, ".amdhsa_next_free_sgpr"), "private segment", scratch)
    assert scratch == 0, name
    assert not any(instr(l).startswith("scratch_") for l in body), name
    assert vgpr <= VGPR_STEP, (name, vgpr)
    assert sum(instr(l).startswith("global_load_dwordx4") for l in body) >= 8, name


def test_volume_mesh_kernel_uses_no_scratch_and_its_stated_lds(device_asm):
    body = kernel_body(device_asm, BUILD)
    print("build", "vgpr", directive(body, ".amdhsa_next_free_vgpr"), "lds", directive(body, ".amdhsa_group_segment_fixed_size"))
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0
    assert not any(instr(l).startswith("scratch_") for l in body)
    assert directive(body, ".amdhsa_group_segment_fixed_size") == 128 * (48 + 4)

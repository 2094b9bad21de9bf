"""Resource budget of the mesh-to-field kernel (claymore_amd/csrc/mpm_collision_mesh.hpp), read from the directives of the assembly the build
flags produce (CPU only, as tests/test_grid_isosurface_isa.py does): no scratch - the walk's small arrays are indexed by constants, the winner's
pseudonormal is read by address - and the LDS the file states: one chunk of 128 records of 48 bytes with their 4-byte indices."""
from test_isa_invariants import device_asm, directive, instr, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

KERNEL = "_ZN3mpm27collision_mesh_table_kernelE"


def test_collision_mesh_kernel_uses_no_scratch_and_its_stated_lds(device_asm):
    body = kernel_body(device_asm, KERNEL)
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0
    assert not any(instr(l).startswith("scratch_") for l in body)
    assert directive(body, ".amdhsa_group_segment_fixed_size") == 128 * (48 + 4)

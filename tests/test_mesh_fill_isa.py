"""Resource budgets of the mesh-fill kernels (claymore_amd/csrc/mpm_mesh_fill.hpp), read from the directives of the assembly the build flags
produce (CPU only, as tests/test_collision_mesh_isa.py does): no scratch in any of them - the classify kernel's 8 (q, T) pairs are read and
written through select chains, never by a run-time index - and the LDS the file states: the field kernel's chunk of 128 records of 48 bytes
with their 4-byte indices for classify, one word per wave for the two scan levels (4 x 4 B, 16 x 8 B), none for emit."""
import pytest

from test_isa_invariants import device_asm, directive, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

LDS = {"_ZN3mpm25mesh_fill_classify_kernelE": 128 * (48 + 4), "_ZN3mpm27mesh_fill_scan_block_kernelE": 4 * 4,
       "_ZN3mpm25mesh_fill_scan_top_kernelE": 16 * 8, "_ZN3mpm21mesh_fill_emit_kernelE": 0}


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_mesh_fill_kernels_use_no_scratch_and_their_stated_lds(device_asm, kernel):
    body = kernel_body(device_asm, kernel)
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0
    assert directive(body, ".amdhsa_group_segment_fixed_size") == LDS[kernel]

"""Resource budgets of the per-particle set-up kernels (claymore_amd/csrc/mpm_particle_init.hpp), read from the directives of the assembly the
build flags produce (CPU only, as tests/test_mesh_fill_isa.py does): no scratch in any of them; the LDS the file states - four images of the
8^3 node cube, 4 x 512 x 4 B, for both instantiations of the rasteriser, none for the other two; and the rasteriser's float atomics on global
memory are the hardware's add, not a compare-and-swap loop."""
import pytest

from test_isa_invariants import device_asm, directive, instr, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

RASTER = ("_ZN3mpm26rasterize_particles_kernelILb0EE", "_ZN3mpm26rasterize_particles_kernelILb1EE")
LDS = {RASTER[0]: 4 * 512 * 4, RASTER[1]: 4 * 512 * 4, "_ZN3mpm22fill_bins_state_kernelE": 0, "_ZN3mpm29validate_particle_init_kernelE": 0}


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_particle_init_kernels_use_no_scratch_and_their_stated_lds(device_asm, kernel):
    body = kernel_body(device_asm, kernel)
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0
    assert not any(instr(l).startswith("scratch_") for l in body)
    assert directive(body, ".amdhsa_group_segment_fixed_size") == LDS[kernel]


@pytest.mark.parametrize("kernel", RASTER)
def test_rasteriser_adds_with_hardware_float_atomics(device_asm, kernel):
    body = [instr(l) for l in kernel_body(device_asm, kernel)]
    assert not any("cmpswap" in l for l in body)
    assert sum(l.startswith("global_atomic_add_f32") for l in body) >= 4, "one global add per channel"
    assert any(l.startswith("ds_add_f32") for l in body), "the cube is summed with LDS float atomics"

"""Resource budget of the surface readout kernels (claymore_amd/csrc/mpm_grid_isosurface.hpp), read from the directives of the
assembly the build flags produce (CPU only, as tests/test_grid_field_isa.py does): no scratch - the corners of a tetrahedron are picked by
selects, the case table is a switch - in either instantiation."""
import pytest

from test_isa_invariants import device_asm, directive, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

KERNELS = {"positions": "_ZN3mpm22grid_isosurface_kernelILb0EE", "positions and velocities": "_ZN3mpm22grid_isosurface_kernelILb1EE"}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_grid_isosurface_kernels_use_no_scratch(device_asm, name):
    body = kernel_body(device_asm, KERNELS[name])
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0, name

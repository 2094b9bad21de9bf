"""Resource budgets of the Eulerian readout kernels (claymore_amd/csrc/mpm_grid_field.hpp), read from the directives of the
assembly the build flags produce (CPU only, as tests/test_particle_stress_isa.py does): no scratch - the sample kernel picks each node's block
among its eight looked-up numbers by selects, not by an indexed array -, no LDS in the sample kernel, and a staged node box in the volume
kernels that leaves room for four workgroups on a compute unit."""
import pytest

from test_isa_invariants import device_asm, directive, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

KERNELS = {"sample": "_ZN3mpm18grid_sample_kernelE", "volume<1>": "_ZN3mpm18grid_volume_kernelILi1EE", "volume<2>": "_ZN3mpm18grid_volume_kernelILi2EE",
           "volume<4>": "_ZN3mpm18grid_volume_kernelILi4EE", "box_totals": "_ZN3mpm22grid_box_totals_kernelE"}


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_grid_field_kernels_use_no_scratch(device_asm, name):
    body = kernel_body(device_asm, KERNELS[name])
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0, name
    lds = directive(body, ".amdhsa_group_segment_fixed_size")
    if name == "sample":
        assert lds == 0
    elif name == "box_totals":
        assert lds < 1024
    else:
        assert 36 * 1024 <= lds <= 40 * 1024, (name, lds)      # 36 blocks of 1 KiB and the padding of the x planes; 160 KiB a compute unit

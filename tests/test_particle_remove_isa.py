"""Resource budgets of the removal kernels (claymore_amd/csrc/mpm_particle_remove.hpp), read from the directives of the assembly the build flags
produce (CPU only, as tests/test_particle_emit_isa.py does): no scratch in any of them, and the group segment the file's header states - none.
The gather fetches a particle's record with 16-byte loads."""
import os
import re

import pytest

import __graft_entry__ as entry
from test_isa_invariants import device_asm, directive, instr, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

KERNELS = {"sink_bitmap_kernel": 0, "sink_count_kernel": 0, "sink_gather_kernel": 0, "sink_mark_kernel": 0, "sink_carry_grid_kernel": 0, "sink_rescale_grid_kernel": 0}
LDS = {f"_ZN3mpm{len(k)}{k}E": v for k, v in KERNELS.items()}


def test_the_header_states_these_group_segments():
    """the numbers above are the ones the file's header comment gives, kernel by kernel"""
    head = open(os.path.join(entry.CSRC, "mpm_particle_remove.hpp")).read().split("#pragma once")[0]
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"(sink_\w+_kernel) (\d+) B", head)}
    assert stated == KERNELS


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_sink_kernels_use_no_scratch_and_their_stated_lds(device_asm, kernel):
    body = kernel_body(device_asm, kernel)
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0
    assert not any(instr(l).startswith("scratch_") for l in body)
    assert directive(body, ".amdhsa_group_segment_fixed_size") == LDS[kernel]


def test_the_gather_loads_a_record_sixteen_bytes_at_a_time(device_asm):
    gather = [instr(l) for l in kernel_body(device_asm, "_ZN3mpm18sink_gather_kernelE")]
    assert sum(l.startswith("global_load_dwordx4") for l in gather) >= 2, "the record: one 16-byte load for the J-fluid, two for a solid"

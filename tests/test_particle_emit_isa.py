"""Resource budgets of the emission kernels (claymore_amd/csrc/mpm_particle_emit.hpp), read from the directives of the assembly the build flags
produce (CPU only, as tests/test_particle_init_isa.py does): no scratch in any of them, and the group segment the file's header states - the
gather's 16 bytes (its block's output range), none for the others.  The gather fetches a particle's record with 16-byte loads, and the grid
carry moves a block with one 16-byte load and store per lane."""
import os
import re

import pytest

import __graft_entry__ as entry
from test_isa_invariants import device_asm, directive, instr, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

LDS = {"_ZN3mpm18emit_gather_kernelE": 16, "_ZN3mpm18emit_append_kernelE": 0, "_ZN3mpm17emit_count_kernelE": 0, "_ZN3mpm16emit_bins_kernelE": 0,
       "_ZN3mpm20emit_fill_ids_kernelE": 0, "_ZN3mpm22emit_carry_grid_kernelE": 0}


def test_the_header_states_these_group_segments():
    """the numbers above are the ones the file's header comment gives, kernel by kernel"""
    head = open(os.path.join(entry.CSRC, "mpm_particle_emit.hpp")).read().split("#pragma once")[0]
    stated = {m.group(1): int(m.group(2)) for m in re.finditer(r"(emit_\w+_kernel) (\d+) B", head)}
    assert stated == {re.match(r"_ZN3mpm\d+(\w+)E$", k).group(1): v for k, v in LDS.items()}


@pytest.mark.parametrize("kernel", sorted(LDS))
def test_emit_kernels_use_no_scratch_and_their_stated_lds(device_asm, kernel):
    body = kernel_body(device_asm, kernel)
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0
    assert not any(instr(l).startswith("scratch_") for l in body)
    assert directive(body, ".amdhsa_group_segment_fixed_size") == LDS[kernel]


def test_gather_and_carry_move_sixteen_bytes_at_a_time(device_asm):
    gather = [instr(l) for l in kernel_body(device_asm, "_ZN3mpm18emit_gather_kernelE")]
    assert sum(l.startswith("global_load_dwordx4") for l in gather) >= 2, "the record: one 16-byte load for the J-fluid, two for a solid"
    carry = [instr(l) for l in kernel_body(device_asm, "_ZN3mpm22emit_carry_grid_kernelE")]
    assert any(l.startswith("global_load_dwordx4") for l in carry) and any(l.startswith("global_store_dwordx4") for l in carry)

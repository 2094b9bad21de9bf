"""Resource budgets of the stress readout kernels (claymore_amd/csrc/mpm_readout.hpp), read from the directives of the
assembly the build flags produce (CPU only: hipcc cross-compiles the device code in ~10 s, as tests/test_isa_invariants.py does): no scratch
- at 256 lanes a workgroup the register budget is 512 a lane - and, like the state readout, no staged grid cube: under 1 KiB of LDS.  The
three older readouts keep their symbols, which tests/test_isa_invariants.py finds by mangled name."""
import pytest

from test_isa_invariants import device_asm, directive, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

READOUT = "_ZN3mpm14readout_kernelILNS_11ReadoutKindE{}E"
STRESS_KINDS = {"kReadStress": 3, "kReadStressTotals": 4}


@pytest.mark.parametrize("name", sorted(STRESS_KINDS))
def test_stress_readout_budgets(device_asm, name):
    body = kernel_body(device_asm, READOUT.format(STRESS_KINDS[name]))
    assert directive(body, ".amdhsa_private_segment_fixed_size") == 0, name
    assert directive(body, ".amdhsa_group_segment_fixed_size") < 1024, name


def test_the_older_readouts_keep_their_symbols(device_asm):
    for kind in range(3):       # kReadState, kReadVelocity, kReadMomentum
        assert kernel_body(device_asm, READOUT.format(kind)), kind

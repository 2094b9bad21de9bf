"""Resource budgets of the force fields' kernels (claymore_amd/csrc/mpm_force_field.hpp), read from the kernel descriptors and
the metadata of the assembly the build flags produce (CPU only, in the manner of tests/test_collider_loads_isa.py): grid_force_kernel
cross-compiles for gfx950 with no scratch and no spilled register - the slot the loop is at is read from the kernel arguments, never from a
private array - and its register count is printed (pytest -s) and kept within the 80 registers that let six waves share a SIMD, the step the
shape kernels are held to; the load readouts, which now take the fields, stay within the limits of their own test.  Nothing is asserted about
which instructions appear."""
import pytest

from test_isa_invariants import device_asm  # noqa: F401  (the module-scoped cross-compile fixture)
from test_collider_loads_isa import COLLIDERS, descriptor

FORCE_KERNEL = "_ZN3mpm17grid_force_kernelE"
READOUTS = {f"{k}<{name}>": f"_ZN3mpm{len(k)}{k}INS_{tag}EEE" for k in ("collider_loads_kernel", "collider_contacts_kernel") for name, tag in COLLIDERS.items()}
READOUTS["collider_loads_kernel<BodyArgs>"] = "_ZN3mpm21collider_loads_kernelINS_8BodyArgsEEE"


def test_grid_force_kernel_uses_no_scratch_and_spills_nothing(device_asm):
    d, meta = descriptor(device_asm, FORCE_KERNEL)
    print("grid_force_kernel vgprs", meta.get("vgpr_count"), "sgprs", meta.get("sgpr_count"), "lds", d[".amdhsa_group_segment_fixed_size"])
    assert d[".amdhsa_private_segment_fixed_size"] == 0
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, meta
    assert d[".amdhsa_group_segment_fixed_size"] == 0
    assert meta["vgpr_count"] <= 80, meta["vgpr_count"]                      # 512 registers a lane and SIMD: six waves
    assert meta["kernarg_segment_size"] >= 4 * (1 + 4 * 32)                   # the four slots travel by value


@pytest.mark.parametrize("name", sorted(READOUTS))
def test_load_readouts_with_fields_stay_within_their_limits(device_asm, name):
    d, meta = descriptor(device_asm, READOUTS[name])
    print(name, "vgprs", meta.get("vgpr_count"), "sgprs", meta.get("sgpr_count"), "lds", d[".amdhsa_group_segment_fixed_size"])
    assert d[".amdhsa_private_segment_fixed_size"] == 0, name
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
    assert meta["vgpr_count"] <= 128, (name, meta["vgpr_count"])
    assert d[".amdhsa_group_segment_fixed_size"] == (4 * 6 * 8 * 8 if name.startswith("collider_loads_kernel") else 0)

"""Resource budgets of the collider-load kernels (claymore_amd/csrc/mpm_collider_loads.hpp), read from the kernel descriptors
and the metadata of the assembly the build flags produce (CPU only, in the manner of tests/test_grid_field_isa.py): for every collider
type with_collider hands out, the totals kernel, the contacts kernel and the reduction cross-compile for gfx950 with no scratch and no
spilled register - the row a lane is at is never the index of a private array -, and their register counts are printed (pytest -s) and
kept within what lets four workgroups of 256 share a compute unit.  Nothing is asserted about which instructions appear."""
import re

import pytest

from test_isa_invariants import device_asm  # noqa: F401  (the module-scoped cross-compile fixture)

COLLIDERS = {"NoCollision": "11NoCollision", "CollisionArgs": "13CollisionArgs", "ShapeArgs": "9ShapeArgs", "TerrainArgs": "11TerrainArgs",
             "VolumeColliderArgs": "18VolumeColliderArgs"}
KERNELS = {f"{k}<{name}>": f"_ZN3mpm{len(k)}{k}INS_{tag}EEE" for k in ("collider_loads_kernel", "collider_contacts_kernel") for name, tag in COLLIDERS.items()}
KERNELS["reduce"] = "_ZN3mpm28collider_loads_reduce_kernelE"


def descriptor(lines, sym):
    """The .amdhsa_kernel block of the one kernel whose symbol starts with sym, as {directive: int}, and its metadata entry's text."""
    starts = [i for i, l in enumerate(lines) if l.strip().startswith(".amdhsa_kernel ") and l.split()[1].startswith(sym)]
    assert len(starts) == 1, (sym, len(starts))
    end = next(i for i in range(starts[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    d = {}
    for l in lines[starts[0] + 1:end]:
        t = l.split()
        if len(t) == 2 and t[0].startswith(".amdhsa_") and re.fullmatch(r"-?\d+", t[1]):
            d[t[0]] = int(t[1])
    full = lines[starts[0]].split()[1]
    at = next(i for i, l in enumerate(lines) if l.strip() == f".name:           {full}" or (l.strip().startswith(".name:") and l.split()[-1] == full))
    lo = max(i for i in range(at + 1) if lines[i].lstrip().startswith("- .agpr_count") or lines[i].lstrip().startswith("- .args"))
    hi = next((i for i in range(at + 1, len(lines)) if lines[i].lstrip().startswith("- .a")), len(lines))
    meta = {}
    for l in lines[lo:hi]:
        m = re.match(r"\s*-?\s*\.(\w+):\s+(\d+)\s*$", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    return d, meta


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_collider_load_kernels_use_no_scratch_and_spill_nothing(device_asm, name):
    d, meta = descriptor(device_asm, KERNELS[name])
    print(name, "vgprs", meta.get("vgpr_count"), "sgprs", meta.get("sgpr_count"), "lds", d[".amdhsa_group_segment_fixed_size"])
    assert d[".amdhsa_private_segment_fixed_size"] == 0, name
    assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
    # 512 registers a lane and SIMD: 128 leaves room for four waves a SIMD, one workgroup of 256 per SIMD quartet four times over
    assert meta["vgpr_count"] <= 128, (name, meta["vgpr_count"])
    if name.startswith("collider_loads_kernel"):
        assert d[".amdhsa_group_segment_fixed_size"] == 4 * 6 * 8 * 8                                    # a wave's [row][8] doubles, four waves
    elif name.startswith("collider_contacts_kernel"):
        assert d[".amdhsa_group_segment_fixed_size"] == 0

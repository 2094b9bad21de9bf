"""Resource budgets of the grid update with a collider (claymore_amd/csrc/mpm_kernels.hpp): the stand-alone frame
grid_update_collider_kernel<Collider> and the carry-over frame carry_grid_kernel<true, Collider>, each instantiated for the level-set object
(CollisionArgs), the analytic shapes (ShapeArgs) and the shapes with a heightfield (TerrainArgs), and the plain carry_grid_kernel<true>.  Read
from the directives and the text of the assembly the build flags produce (CPU only)."""
import pytest

from test_isa_invariants import device_asm, directive, instr, kernel_body  # noqa: F401  (device_asm: the module-scoped cross-compile fixture)

VGPR_STEP = 80          # six waves per SIMD: the budget of the level-set kernels, and the occupancy step the shapes and terrain kernels are built in
COLLIDERS = {"level-set": "NS_13CollisionArgsE", "shapes": "NS_9ShapeArgsE", "terrain": "NS_11TerrainArgsE"}
KERNELS = {f"{frame} {kind}": sym.format(arg) for kind, arg in COLLIDERS.items()
           for frame, sym in (("stand-alone", "_ZN3mpm27grid_update_collider_kernelI{}EE"), ("carry", "_ZN3mpm17carry_grid_kernelILb1E{}EE"))}
KERNELS["carry plain"] = "_ZN3mpm17carry_grid_kernelILb1ENS_11NoCollisionEEE"


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_grid_update_kernels_use_no_scratch_and_keep_their_registers(device_asm, name):
    """No scratch segment and no scratch instruction anywhere.  The collider kernels leave registers for at least six waves per SIMD (<= 80
    VGPRs; the per-node sinf / cosf version of the stand-alone level-set kernel needed 81; the slot loop of the shapes is a real loop over the
    kernel arguments, so four slots cost the registers of one) - built: level-set 67 / 69, shapes 72 / 74, terrain 72 / 75 (stand-alone /
    carry).  The plain carry_grid_kernel<true> keeps the 22 VGPRs it had before it shared a template.  The level-set pair gets its pose from
    the host: no range reduction, no polynomial."""
    body = kernel_body(device_asm, KERNELS[name])
    vgpr, scratch = directive(body, ".amdhsa_next_free_vgpr"), directive(body, ".amdhsa_private_segment_fixed_size")
    print(name, "vgpr", vgpr, "sgpr", directive(body, ".amdhsa_next_free_sgpr"), "private segment", scratch)
    assert scratch == 0, name
    assert not any(instr(l).startswith("scratch_") for l in body), name
    assert vgpr <= (22 if name == "carry plain" else VGPR_STEP), (name, vgpr)
    if name.endswith("level-set"):
        assert not any("v_sin_f32" in l or "v_cos_f32" in l for l in body), name

"""The collider-load readout without a GPU: the ABI surface of include/claymore_amd.h / claymore_amd/_ffi.py, and tests/collider_load_model.py -
the model tests/test_collider_loads_gpu.py holds the kernels to - against closed forms, the momentum ledger of one grid update and the slot
order.  The closed forms use masses that are powers of two and velocities with few bits, gravity 0 and colliders at rest, so that every
float32 statement of the update is exact and the expected impulse is an equality, not a tolerance."""
import ctypes as C
import os
import re

import numpy as np

import collider_load_model as lm
import collision_shape_model as sm
import grid_update_model as gm
from claymore_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, BOUNDARY, DX = gm.G_BLOCKS, 2, sm.DX
F32 = np.float32


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    """The four entry points resolve with the header's signatures, MPM_LOAD_ROWS is 6 in the header and in the binding, and a NULL context is
    refused by each - with a dt <= 0 too - before anything is touched (no device is needed for a refusal)."""
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert re.search(r"#define\s+MPM_LOAD_ROWS\s+6\b", hdr) and _ffi.LOAD_ROWS == 6 == lm.ROWS and len(_ffi.LOAD_ROW_NAMES) == 6 == len(lm.ROW_NAMES)
    assert C.sizeof(_ffi.LoadOptions) == 6 * 4 + 6 * 3 * 4
    hip = _ffi.load_hip()
    for name in ("collider_loads", "collider_contacts", "load_gauge", "load_gauge_read"):
        assert "mpm_" + name in hdr and callable(getattr(hip, name))
    out = (C.c_double * 8 * 6)()
    n = C.c_size_t(0)
    for dt in (1e-4, 0.0, -1.0, float("nan")):
        assert hip.collider_loads(None, dt, None, out) != _ffi.MPM_OK
        assert hip.collider_contacts(None, dt, None, None, C.byref(n)) != _ffi.MPM_OK
    assert hip.load_gauge(None, 1, None) != _ffi.MPM_OK and hip.load_gauge_read(None, out, None, None, 0) != _ffi.MPM_OK
    assert all(v == 0.0 for row in out for v in row) and n.value == 0


# ---- closed forms ---------------------------------------------------------------------------------------------------------------------------
SLAB_KEYS = np.array([[7, 7, 7], [8, 7, 7]], dtype=np.int32)         # 8 x 4 x 4 nodes (28..35, 28..31, 28..31), interior blocks
SLAB_CENTRE = (31.5 * DX, 29.5 * DX, 29.5 * DX)


def slab(mass, v):
    """Every node of the slab with mass `mass` (a power of two) and velocity v (few bits): the momentum m v is exact, and so is p / m."""
    grid = np.zeros((len(SLAB_KEYS), 4, 64), np.float32)
    grid[:, 0] = F32(mass)
    for d in range(3):
        grid[:, 1 + d] = F32(mass) * F32(v[d])
    return grid


def rows_of(grid, colliders, dt=1e-3, gravity=0.0, t=0.0):
    nr = lm.node_rows(SLAB_KEYS, G, BOUNDARY, gravity, dt, grid, colliders, t, DX)
    tot, _ = lm.totals(nr, lm.default_pivots(colliders, t))
    return nr, tot


def test_sticky_half_space_takes_all_the_momentum():
    m, v = 2.0 ** -10, (0.5, -1.25, 0.375)
    c = sm.collider("halfspace", a=(0.5, 40 * DX, 0.5), b=(0.0, 1.0, 0.0), type=sm.STICKY)          # the solid is y <= 40 dx: the whole slab
    nr, tot = rows_of(slab(m, v), [c])
    assert tot[1, 0] == 128 and tot[1, 7] == 128 * m
    assert np.array_equal(tot[1, 1:4], 128 * m * np.array(v))                                        # J = sum m v, exactly
    assert (tot[[0, 2, 3, 4, 5]] == 0).all() and (nr["v_final"] == 0).all()


def test_slip_half_space_takes_the_normal_part_only():
    m, v = 2.0 ** -10, (0.5, -1.25, 0.375)
    c = sm.collider("halfspace", a=(0.5, 40 * DX, 0.5), b=(0.0, 1.0, 0.0), type=sm.SLIP, friction=0.0)
    nr, tot = rows_of(slab(m, v), [c])
    assert tot[1, 0] == 128 and np.array_equal(tot[1, 1:4], [0.0, 128 * m * v[1], 0.0])
    assert np.array_equal(nr["v_final"], np.broadcast_to(np.array([0.5, 0.0, 0.375], np.float32), (128, 3)))


def test_separate_half_space_leaves_receding_nodes_alone():
    m, v = 2.0 ** -10, (0.5, 1.25, 0.375)                                                            # v . n > 0: the material leaves
    c = sm.collider("halfspace", a=(0.5, 40 * DX, 0.5), b=(0.0, 1.0, 0.0), type=sm.SEPARATE, friction=0.3)
    nr, tot = rows_of(slab(m, v), [c])
    assert (tot == 0).all() and not nr["touched"][1].any()
    approaching, tot2 = rows_of(slab(m, (0.5, -1.25, 0.375)), [sm.collider("halfspace", a=(0.5, 40 * DX, 0.5), b=(0.0, 1.0, 0.0), type=sm.SEPARATE, friction=0.0)])
    assert tot2[1, 0] == 128 and np.array_equal(tot2[1, 1:4], [0.0, 128 * m * -1.25, 0.0])


def test_pure_rotation_gives_no_net_impulse_but_an_angular_one():
    """A sticky sphere about the slab's centre that only turns, material at rest: the velocity it imposes is odd in the node's offset from the
    centre (the response's `cross product` is linear in it), the slab is point-symmetric about the centre and every float32 statement keeps
    the sign symmetry, so the impulses cancel in pairs - exactly, fsum adds exactly - while the moments r x (-j), even in the offset, add up."""
    m = 2.0 ** -10
    c = sm.collider("sphere", a=SLAB_CENTRE, radius=8 * DX, type=sm.STICKY, trans=SLAB_CENTRE, omega=(0.0, 0.0, 3.0))
    nr, tot = rows_of(slab(m, (0.0, 0.0, 0.0)), [c])
    assert tot[1, 0] == 128 and np.array_equal(tot[1, 1:4], [0.0, 0.0, 0.0])
    assert abs(tot[1, 6]) > 1e-6 and (np.abs(nr["dv"][1]).max(axis=0)[:2] > 0).all()


def test_wall_row_and_gravity():
    """A block in the low x wall zone: the wall row takes the x momentum (0 - p / m per node, so J = sum m fl(p / m) = sum p here), gravity moves
    v_y and belongs to no row."""
    keys = np.array([[1, 7, 7]], dtype=np.int32)
    m, v = 2.0 ** -8, (0.75, -0.5, 0.25)
    grid = np.zeros((1, 4, 64), np.float32)
    grid[:, 0] = F32(m)
    for d in range(3):
        grid[:, 1 + d] = F32(m) * F32(v[d])
    nr = lm.node_rows(keys, G, BOUNDARY, -9.8, 1e-3, grid, [], 0.0, DX)
    tot, _ = lm.totals(nr, lm.default_pivots([], 0.0))
    assert nr["used"] == [lm.WALLS] and tot[5, 0] == 64 and np.array_equal(tot[5, 1:4], [64 * m * 0.75, 0.0, 0.0]) and (tot[:5] == 0).all()
    assert (nr["v_final"][:, 0] == 0).all() and (nr["v_final"][:, 1] == F32(F32(-0.5) + gm.gdt32(-9.8, 1e-3))).all()


# ---- the ledger --------------------------------------------------------------------------------------------------------------------------------
def test_momentum_ledger_of_one_grid_update():
    """grid_update_model's scene (222 blocks, all 27 wall classes), the generator's finite tier, two overlapping moving shapes and gravity:
    sum m v_final = sum p + M g dt e_y - sum_rows J per component.  The bound is float32 rounding alone: per node fl(p / m) carries at most
    1.5 ulp, the gravity addition half an ulp of its sum, each dv = fl(after - before) half an ulp of itself, and m times each is exact in
    float64 - at most 8 * 2^-24 * sum_nodes m (|v_free| + |g dt| + sum_k |dv_k|) with room to spare."""
    keys = gm.scene_keys()
    dt, gravity = 1e-4, -9.8
    a = sm.make("halfspace_tilted", type=sm.SLIP, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    b = sm.make("sphere", type=sm.SEPARATE, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    for seed in (1, 2):
        pat = gm.generate(len(keys), seed, "finite")[0]
        nr = lm.node_rows(keys, G, BOUNDARY, gravity, dt, pat.view(np.float32), [a, b], 0.0, DX)
        tot, _ = lm.totals(nr, lm.default_pivots([a, b], 0.0))
        assert tot[1, 0] > 500 and tot[2, 0] > 500 and tot[5, 0] > 500
        lv = nr["live"]
        m = nr["m"][lv].astype(np.float64)
        p = pat.view(np.float32)[:, 1:4].transpose(0, 2, 1).reshape(-1, 3)[lv].astype(np.float64)
        gdt = float(gm.gdt32(gravity, dt))
        left = np.array([np.sum(m * nr["v_final"][lv, d].astype(np.float64)) for d in range(3)])
        right = p.sum(axis=0) + np.array([0.0, m.sum() * gdt, 0.0]) - tot[:, 1:4].sum(axis=0)
        moved = sum(np.abs(nr["dv"][r][lv].astype(np.float64)) for r in nr["used"])
        bound = 8 * 2.0 ** -24 * np.sum(m[:, None] * (np.abs(p / m[:, None]) + abs(gdt) + moved), axis=0)
        print(seed, "ledger residual", np.abs(left - right), "bound", bound)
        assert (np.abs(left - right) <= bound).all(), (left - right, bound)


# ---- the slot order ------------------------------------------------------------------------------------------------------------------------------
def test_swapped_slots_give_different_rows():
    keys = gm.scene_keys()
    a = sm.make("halfspace_tilted", type=sm.SLIP, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    b = sm.make("sphere", type=sm.SEPARATE, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    pat = gm.generate(len(keys), 4, "finite")[0].view(np.float32)
    tot = {}
    for order, cols in (("ab", [a, b]), ("ba", [b, a])):
        nr = lm.node_rows(keys, G, BOUNDARY, -9.8, 1e-4, pat, cols, 0.0, DX)
        tot[order], _ = lm.totals(nr, lm.default_pivots(cols, 0.0))
        nodes_rows, rec = lm.contacts(nr)
        assert len(nodes_rows) == len(rec) == int(tot[order][:, 0].sum())
        both = nr["touched"][1] & nr["touched"][2]
        assert both.sum() > 100                                                                      # (the shapes do overlap)
    # a shape acting first sees the free velocity, acting second what the other left: neither shape's row survives the swap
    assert not np.array_equal(tot["ab"][2, 1:4], tot["ba"][1, 1:4]) and not np.array_equal(tot["ab"][1, 1:4], tot["ba"][2, 1:4])
    assert np.array_equal(tot["ab"][5], tot["ba"][5])                                                # (the walls act before either)

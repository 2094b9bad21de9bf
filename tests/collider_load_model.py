"""The collider-load readout (claymore_amd/csrc/mpm_collider_loads.hpp) restated with numpy.  Not a test:
tests/test_collider_loads_cpu.py judges this model against closed forms and the momentum ledger, tests/test_collider_loads_gpu.py judges the
kernels against it.

Per node, in float32, the grid update's own statements: walls and gravity from grid_update_model.cell_update (the `strict` candidate: the
collider kernels are compiled without contraction), then the level-set object through collision_shape_model.field_resolve and the slots in
order through collision_volume_model.resolve (which hands shapes and heightfields on to their own models), each on the velocity the
previous one left.  Row r's dv is v_after - v_before, three float32 subtractions; the wall row's is 0 - fl32(p / m) on each axis a wall
zeroes.  In float64: j = m dv (exact), the load -j, the arm r = X - pivot with X = fl32(node * dx), the torque r x (-j) with every product
and difference rounded (no contraction - numpy has none).  Totals: math.fsum, the correctly rounded sum."""
import math

import numpy as np

import collision_shape_model as sm
import collision_volume_model as cvm
import grid_update_model as gm

F32 = np.float32
ROWS, WALLS = 6, 5
ROW_NAMES = ("field", "slot0", "slot1", "slot2", "slot3", "walls")


def node_rows(keys, G, boundary, gravity, dt, grid, colliders, t, dx, field=None):
    """-> dict: nodes (n, 3) int64 and m (n,) float32 of every cell, row = block * 64 + cell; live (n,); per row r in 0 .. 5: dv[r] (n, 3) float32,
    after[r] (n, 3) float32 (the velocity that row's collider left; the wall row's: after walls and gravity), touched[r] (n,) bool;
    used: the rows that exist, in the order they act (walls, field, slots); v_final (n, 3)."""
    grid = np.ascontiguousarray(grid, dtype=np.float32)
    n = len(keys) * 64
    w = gm.wall_flags(keys, G, boundary)
    wx, wy, wz = (np.broadcast_to(w[:, d, None], grid[:, 0].shape) for d in range(3))
    live, (v0, v1s, _, v2) = gm.cell_update(grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 3], wx, wy, wz, gm.gdt32(gravity, dt))
    lv = live.reshape(-1)
    m = grid[:, 0].reshape(-1)
    with np.errstate(all="ignore"):
        inv = (F32(1.0) / np.where(live, grid[:, 0], F32(1.0))).astype(np.float32)
        quot = [gm.mul32(grid[:, 1 + d], inv) for d in range(3)]
        wall_dv = np.stack([np.where(wd, (F32(0.0) - q).astype(np.float32), F32(0.0)).reshape(-1) for wd, q in zip((wx, wy, wz), quot)], axis=1).astype(np.float32)
    nodes = gm.node_coords(keys).transpose(0, 2, 1).reshape(-1, 3)
    X = (nodes.astype(np.float32) * F32(dx)).astype(np.float32)
    vel = np.stack([v0.reshape(-1), v1s.reshape(-1), v2.reshape(-1)], axis=1).astype(np.float32)
    zero = np.zeros((n, 3), np.float32)
    dv, after, touched, used = [zero] * ROWS, [zero] * ROWS, [np.zeros(n, bool)] * ROWS, [WALLS]

    def touch(d):
        return lv & ~((d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] == 0))                    # (a NaN compares unequal: touched)

    dv[WALLS], after[WALLS] = np.where(lv[:, None], wall_dv, zero), vel.copy()
    touched[WALLS] = touch(dv[WALLS])
    acting = ([(0, field)] if field is not None else []) + [(1 + s, c) for s, c in enumerate(colliders) if c is not None]
    for r, c in acting:
        with np.errstate(all="ignore"):
            new, _ = sm.field_resolve(c[0], t, nodes, dx, boundary, G, c[1], c[2], vel) if r == 0 else cvm.resolve(c, t, X, vel)
            new = np.where(lv[:, None], new, vel).astype(np.float32)
            dv[r] = np.where(lv[:, None], (new - vel).astype(np.float32), zero)
        vel = new
        after[r], touched[r] = vel.copy(), touch(dv[r])
        used.append(r)
    return dict(nodes=nodes, X=X, m=m, live=lv, dv=dv, after=after, touched=touched, used=used, v_final=vel)


def contacts(nr):
    """One record per touched (node, row), sorted by (node, row): nodes_rows (k, 4) int32, rec (k, 8) float32 {m, dv, v_after, 0}."""
    out_n, out_r = [], []
    for r in range(ROWS):
        idx = np.flatnonzero(nr["touched"][r])
        out_n.append(np.concatenate([nr["nodes"][idx], np.full((len(idx), 1), r)], axis=1).astype(np.int32))
        out_r.append(np.concatenate([nr["m"][idx, None], nr["dv"][r][idx], nr["after"][r][idx], np.zeros((len(idx), 1), np.float32)], axis=1).astype(np.float32))
    nodes_rows, rec = np.concatenate(out_n), np.concatenate(out_r)
    order = np.lexsort(nodes_rows.T[::-1])
    return nodes_rows[order], rec[order]


def sort_contacts(nodes, rows, mass, dv, v_after):
    """Engine.collider_contacts' arrays in contacts()' layout and order."""
    nodes_rows = np.concatenate([nodes, rows[:, None]], axis=1).astype(np.int32)
    rec = np.concatenate([mass[:, None], dv, v_after, np.zeros((len(mass), 1), np.float32)], axis=1).astype(np.float32)
    order = np.lexsort(nodes_rows.T[::-1])
    return nodes_rows[order], rec[order]


def default_pivots(colliders, t, field=None):
    """(6, 3) float64: the collider's shift at t (collision_pose: trans + trans_vel t in float32), the origin for the walls and for empty rows."""
    piv = np.zeros((ROWS, 3), np.float64)
    for r, c in ([(0, field[0])] if field is not None else []) + [(1 + s, c) for s, c in enumerate(colliders) if c is not None]:
        piv[r] = sm.pose(c, t)["shift"].astype(np.float64)
    return piv


def terms(nr, pivots):
    """Per row the per-node float64 terms of the touched nodes: (k, 7) {-jx, -jy, -jz, lx, ly, lz, m} - the bits a device lane forms."""
    out = []
    for r in range(ROWS):
        idx = np.flatnonzero(nr["touched"][r])
        with np.errstate(all="ignore"):
            m = nr["m"][idx].astype(np.float64)
            j = -(m[:, None] * nr["dv"][r][idx].astype(np.float64))
            arm = nr["X"][idx].astype(np.float64) - np.asarray(pivots, np.float64)[r][None]
            lx = arm[:, 1] * j[:, 2] - arm[:, 2] * j[:, 1]
            ly = arm[:, 2] * j[:, 0] - arm[:, 0] * j[:, 2]
            lz = arm[:, 0] * j[:, 1] - arm[:, 1] * j[:, 0]
        out.append(np.concatenate([j, np.stack([lx, ly, lz], axis=1), m[:, None]], axis=1))
    return out


def totals(nr, pivots):
    """-> (6, 8) float64 {n_touched, Jx, Jy, Jz, Lx, Ly, Lz, m_touched} with math.fsum, and (6, 8) the sums of the terms' absolute values."""
    tot, mag = np.zeros((ROWS, 8)), np.zeros((ROWS, 8))
    for r, tr in enumerate(terms(nr, pivots)):
        tot[r, 0] = mag[r, 0] = len(tr)
        for c in range(7):
            tot[r, 1 + c] = math.fsum(tr[:, c].tolist()) if np.isfinite(tr[:, c]).all() else tr[:, c].sum()
            mag[r, 1 + c] = math.fsum(np.abs(tr[:, c]).tolist()) if np.isfinite(tr[:, c]).all() else np.inf
    return tot, mag

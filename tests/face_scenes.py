"""Scenes in the outer shell of the domain (tests/test_domain_faces_gpu.py, tests/test_rasterize_faces_model.py): particles in the
wall zone of all six faces, in cells -2 / -1 of the lower faces (node index 0 / 1, truncated into block 0) and in the top cells of every axis,
at B-spline rounding ties.  Positions are given in cell units p = x / dx and converted with an exact float32 product (dx is a power of two),
so a tie p = k + 0.5 reaches both engines as an exact tie.

Also: a float64 restatement of the set-up rasterization (rasterize, mgmpm_kernels.cuh:153-219) - the grid both engines must build from a
scene - and the per-axis index arithmetic of rasterize_blocks_kernel (claymore_amd/csrc/mpm_kernels.hpp)."""
import itertools

import numpy as np

from claymore_amd import _ffi, scenes

# cell offsets from a lower face; an upper face uses n - offset (n - 0.01 for 0: x = 1 is outside [0, 1))
FACE_OFFSETS = (0.0, 0.25, 0.49, 0.5, 0.51, 1.0, 1.5, 2.0, 2.5, 3.5)
CORNER_OFFSETS = (0.0, 0.49, 0.5, 1.5, 2.5)      # exact ties at even (0, 2) and odd (1) k


def upper(n, off):
    return n - (0.01 if off == 0.0 else off)


def to_world(p, bits):
    """Cell units -> world units, exactly: float32(p) * 2^-bits."""
    return (np.asarray(p, dtype=np.float32) * np.float32(1.0 / (1 << bits))).astype(np.float32)


def _grid_points(axes):
    X, Y, Z = np.meshgrid(*[np.asarray(a, dtype=np.float64) for a in axes], indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def setup_slab_cells(bits):
    """Cell-unit positions: a thin slab at FACE_OFFSETS against each of the six faces (a 4 x 4 patch in the middle of the face), the eight
    corners (CORNER_OFFSETS on all three axes) and the twelve edges (three offsets on the two axes that meet there).  No duplicates."""
    n = 1 << bits
    mid = n / 2 - 1.75 + 0.5 * np.arange(4)
    pts = []
    for axis, side in itertools.product(range(3), ("lo", "hi")):
        face = np.array(FACE_OFFSETS if side == "lo" else [upper(n, o) for o in FACE_OFFSETS])
        axes = [mid, mid, mid]
        axes[axis] = face
        pts.append(_grid_points(axes))
    lo_c = np.array(CORNER_OFFSETS)
    hi_c = np.array([upper(n, o) for o in CORNER_OFFSETS])
    for sides in itertools.product((lo_c, hi_c), repeat=3):
        pts.append(_grid_points(sides))
    edge = np.array([0.25, 0.5, 1.5])
    for along in range(3):
        for s0, s1 in itertools.product((edge, n - edge), repeat=2):
            axes = [None, None, None]
            axes[along] = mid[1:3]
            others = [d for d in range(3) if d != along]
            axes[others[0]], axes[others[1]] = s0, s1
            pts.append(_grid_points(axes))
    return np.unique(np.concatenate(pts).astype(np.float32), axis=0)


def setup_slab_scene(bits=5, v0=(0.5, -1.0, 0.25)):
    xyz = to_world(setup_slab_cells(bits), bits)
    prm = {"volume": scenes._vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "face_slabs", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": xyz, "v0": tuple(v0), "params": prm}]}


def face_box_cells(bits, axis, side, depth=12, width=12):
    """A box against one face: `depth` layers along the face's normal from p = 0.25 (lower face: cells -2, -1, 0, ...; upper face: the mirror,
    n - 0.25, n - 0.75, ...) and a width x width patch in the middle of the face, two particles per cell and axis (the reference's lattice
    density, 8 per cell)."""
    n = 1 << bits
    normal = 0.25 + 0.5 * np.arange(depth)
    if side == "hi":
        normal = n - normal
    across = n / 2 - width / 4.0 + 0.25 + 0.5 * np.arange(width)
    axes = [across, across, across]
    axes[axis] = normal
    return _grid_points(axes).astype(np.float32)


def _prm(bits, material):
    return {"volume": scenes._vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3} if material == _ffi.FIXED_COROTATED else {}


def wall_zone_scene(bits=5, direction="out", speed=2.0, material=_ffi.FIXED_COROTATED):
    """One body per face (six models), 12 cells deep: from the outer two cells through the 8-cell wall zone (where the slip walls zero the
    normal velocity whatever its sign) into the free interior; v0 along the outward normal (direction 'out') or the inward one ('in')."""
    models = []
    for axis, side in itertools.product(range(3), ("lo", "hi")):
        outward = -1.0 if side == "lo" else 1.0
        v = [0.0, 0.0, 0.0]
        v[axis] = speed * (outward if direction == "out" else -outward)
        models.append({"material": material, "xyz": to_world(face_box_cells(bits, axis, side, depth=24), bits), "v0": tuple(v), "params": _prm(bits, material)})
    return {"name": f"wall_zone_{direction}", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128}, "models": models}


def lower_face_materials_scene(bits=5, speed=1.5):
    """Four materials against the three lower faces (cells -2 and -1 are wrapped into block 0): J-fluid on x = 0, fixed-corotated on the floor,
    sand on z = 0, NACC in the x = 0 / y = 0 edge; every body moves toward its face."""
    n = 1 << bits
    nacc = face_box_cells(bits, 0, "lo", depth=8, width=8)
    nacc[:, 1] = nacc[:, 1] - nacc[:, 1].min() + 0.25          # slide it down into the floor corner
    nacc[:, 2] += n / 4                                          # (away from the fixed-corotated body in the middle of the floor)
    bodies = [(_ffi.J_FLUID, face_box_cells(bits, 0, "lo", depth=8, width=8) - np.float32([0, n / 4, 0]), (-speed, 0.0, 0.0)),
              (_ffi.FIXED_COROTATED, face_box_cells(bits, 1, "lo", depth=8, width=8), (0.0, -speed, 0.0)),
              (_ffi.SAND, face_box_cells(bits, 2, "lo", depth=8, width=8) + np.float32([n / 4, 0, 0]), (0.0, 0.0, -speed)),
              (_ffi.NACC, nacc, (-speed, -speed, 0.0))]
    models = [{"material": m, "xyz": to_world(c, bits), "v0": v, "params": _prm(bits, m)} for m, c, v in bodies]
    return {"name": "lower_face_materials", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128}, "models": models}


def corner_obstacle_scene(bits=5, boundary="slip", friction=0.3, speed=2.0):
    """A level-set sphere of radius 6 cells centred 5 / 6 cells from the x = 0 / y = 0 faces, and a body against x = 0 that falls onto it.
    The object's nodes lie both inside the wall zone - where query_sdf's box (boundary_condition.cuh:141-146) must leave them to the slip walls -
    and outside it, in neighbouring blocks of the same grid update."""
    n = 1 << bits
    dx = 1.0 / n
    sdf, grad = scenes.sphere_level_set(bits, (5.0 * dx, 6.0 * dx, 0.5), 6.0 * dx)
    body = _grid_points([0.25 + 0.5 * np.arange(24), 12.25 + 0.5 * np.arange(12), n / 2 - 2.75 + 0.5 * np.arange(12)]).astype(np.float32)
    return {"name": f"corner_obstacle_{boundary}", "bits": bits, "dt": 1e-4, "config": {},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": to_world(body, bits), "v0": (-0.5, -speed, 0.0), "params": _prm(bits, _ffi.FIXED_COROTATED)}],
            "collision": {"sdf": sdf, "grad": grad, "type": {"sticky": 0, "slip": 1, "separate": 2}[boundary], "friction": friction}}


# ---- the set-up rasterization --------------------------------------------------------------------------------------------------------------
def lround_half_away(p):
    """The reference's lround (utility_funcs.hpp:21-23) for p >= 0, in float64 (exact for float32 inputs)."""
    return np.floor(np.asarray(p, dtype=np.float64) + 0.5).astype(np.int64)


def bspline64(d):
    """Quadratic B-spline weights of the three stencil nodes, d = p - base in cells (float64)."""
    d = np.asarray(d, dtype=np.float64)
    return np.stack([0.5 * (1.5 - d) ** 2, 0.75 - (d - 1.0) ** 2, 0.5 * (d - 0.5) ** 2], axis=-1)


def reference_setup_grid(scene):
    """The grid both engines must hold after initial_setup, in float64: every particle spreads mass * w (and mass * w * v0) over its 27 stencil
    nodes; a node outside [0, n)^3 has no block and receives nothing (its key is out of the table's range).  Returns {node (3-tuple): [m, mv]}
    and the per-node contributions that fall outside the domain, split by face (mass only)."""
    n = 1 << scene["bits"]
    grid, outside = {}, {"lo": 0.0, "hi": 0.0}
    for m in scene["models"]:
        p = m["xyz"].astype(np.float64) * n
        mass = float(np.float32(m["params"].get("volume", scenes._vol(scene["bits"]))) * np.float32(m["params"].get("rho", 1e3)))
        base = lround_half_away(p) - 1
        w = bspline64(p - base)                        # (N, 3 axes, 3 nodes)
        v0 = np.asarray(m.get("v0", (0, 0, 0)), dtype=np.float64)
        for i, j, k in itertools.product(range(3), repeat=3):
            node = base + np.array([i, j, k])
            wm = mass * w[:, 0, i] * w[:, 1, j] * w[:, 2, k]
            inside = np.all((node >= 0) & (node < n), axis=1)
            outside["lo"] += float(wm[np.any(node < 0, axis=1)].sum())
            outside["hi"] += float(wm[np.any(node >= n, axis=1) & ~np.any(node < 0, axis=1)].sum())
            for nd, q in zip(map(tuple, node[inside]), wm[inside]):
                e = grid.setdefault(nd, np.zeros(4))
                e[0] += q
                e[1:] += q * v0
    return grid, outside


def grid_to_nodes(keys, blocks):
    """{node: [m, mv]} of a dumped grid (keys (B, 3), blocks (B, 4, 64)), non-empty nodes only."""
    out = {}
    for key, blk in zip(keys, blocks):
        for cell in np.nonzero(np.any(blk != 0, axis=0))[0]:
            nd = (int(key[0]) * 4 + (cell >> 4), int(key[1]) * 4 + ((cell >> 2) & 3), int(key[2]) * 4 + (cell & 3))
            out[nd] = blk[:, cell].astype(np.float64)
    return out


# ---- rasterize_blocks_kernel's index arithmetic, one axis -------------------------------------------------------------------------------------
def lround_pos(p):
    """mpm_device_math.hpp lround_pos: rintf (ties to even) + 1 where p - rint(p) == +0.5, on float32."""
    p = np.asarray(p, dtype=np.float32)
    r = np.rint(p)
    return r.astype(np.int64) + ((p - r) == np.float32(0.5)).astype(np.int64)


def block_key(cell):
    """C++ truncating division cell / 4 (particle_block_key)."""
    cell = np.asarray(cell, dtype=np.int64)
    return np.where(cell < 0, -((-cell) // 4), cell // 4)


def kernel_axis(p):
    """(node N, stencil base N - 1, block key, cube offset l = base - 4 * key) of rasterize_blocks_kernel along one axis."""
    N = lround_pos(p)
    key = block_key(N - 2)
    base = N - 1
    return N, base, key, base - 4 * key

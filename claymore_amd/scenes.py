"""Deterministic synthetic scenes of BASELINE.json's configs.

Particles come from the reference's lattice rule `sample_uniform_box`
(Library/MnBase/Geometry/GeometrySampler.h:11-37): 8 particles per grid node at node +- 0.25 dx;
spheres are that lattice clipped by |x - c| <= R.  No RNG, no Data/ files.
"""
import numpy as np

from ._ffi import FIXED_COROTATED, J_FLUID, NACC, SAND  # noqa: F401


def lattice_box(bits, minc, maxc):
    """All lattice particles of nodes minc <= (i,j,k) < maxc; float32 (n,3)."""
    dx = np.float32(1.0 / (1 << bits))
    ax = [np.arange(minc[d], maxc[d], dtype=np.float64) for d in range(3)]
    off = np.array([-0.25, 0.25])
    # per axis: node*dx +- 0.25dx  (exact in fp32: dx is a power of two)
    coords = [((a[:, None] + off[None, :]) * float(dx)).reshape(-1) for a in ax]
    # the reference nests i,j,k then ii,jj,kk; the order of particles is irrelevant to the physics,
    # a plain tensor product is used here
    X, Y, Z = np.meshgrid(coords[0], coords[1], coords[2], indexing="ij")
    out = np.empty((X.size, 3), dtype=np.float32)
    out[:, 0] = X.reshape(-1)
    out[:, 1] = Y.reshape(-1)
    out[:, 2] = Z.reshape(-1)
    return out


def lattice_sphere(bits, center, radius_cells):
    dx = 1.0 / (1 << bits)
    c = np.asarray(center, dtype=np.float64)
    r = radius_cells * dx
    lo = np.floor((c - r) / dx).astype(int) - 1
    hi = np.ceil((c + r) / dx).astype(int) + 2
    pts = lattice_box(bits, lo, hi)
    d2 = ((pts.astype(np.float64) - c[None, :]) ** 2).sum(axis=1)
    return np.ascontiguousarray(pts[d2 <= r * r])


def _vol(bits):
    dx = 1.0 / (1 << bits)
    return float(np.float32(dx * dx * dx / 8.0))


def two_spheres(bits=7, radius_cells=9.0, gap_cells=None, speed=0.5, material=FIXED_COROTATED, youngs=5e3):
    """C1: two elastic spheres colliding (BASELINE config 1).  Default: centres (0.40,0.5,0.5)/(0.60,0.5,0.5),
    R = 9 dx, v = (+-0.5, 0, 0), fixed-corotated E = 5e3, nu = 0.4, rho = 1e3, vol = dx^3/8."""
    dx = 1.0 / (1 << bits)
    if gap_cells is None:
        c0, c1 = (0.40, 0.5, 0.5), (0.60, 0.5, 0.5)
    else:
        half = (radius_cells + gap_cells / 2.0) * dx
        c0, c1 = (0.5 - half, 0.5, 0.5), (0.5 + half, 0.5, 0.5)
    prm = {"volume": _vol(bits), "youngs_modulus": youngs, "poisson_ratio": 0.4, "rho": 1e3}
    return {
        "name": "two_spheres", "bits": bits, "dt": 1e-4,
        "config": {"max_ppc": 128},
        "models": [
            {"material": material, "xyz": lattice_sphere(bits, c0, radius_cells), "v0": (speed, 0.0, 0.0), "params": dict(prm)},
            {"material": material, "xyz": lattice_sphere(bits, c1, radius_cells), "v0": (-speed, 0.0, 0.0), "params": dict(prm)},
        ],
    }


def two_spheres_c4(bits=9, radius_cells=84.0, speed=1.0):
    """C4 (BASELINE config 4): two fixed-corotated spheres of R = 84 dx on a 512^3 grid, centres (0.30, 0.5, 0.5) / (0.70, 0.5, 0.5),
    approaching each other at +-1 m/s: 2 x 19.9 M particles; run as MGSP with 4 ranks (static particle partition, two slabs per sphere)."""
    prm = {"volume": _vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    return {
        "name": "two_spheres_c4", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128},
        "models": [
            {"material": FIXED_COROTATED, "xyz": lattice_sphere(bits, (0.30, 0.5, 0.5), radius_cells), "v0": (speed, 0.0, 0.0), "params": dict(prm)},
            {"material": FIXED_COROTATED, "xyz": lattice_sphere(bits, (0.70, 0.5, 0.5), radius_cells), "v0": (-speed, 0.0, 0.0), "params": dict(prm)},
        ],
    }


def sphere_drop(bits=8, radius_cells=53.0, center=(0.5, 0.6, 0.5), material=FIXED_COROTATED):
    """C2: one elastic sphere dropped under gravity (~5.0 M particles at bits 8, R = 53 dx)."""
    prm = {"volume": _vol(bits)} if material != SAND else {}
    return {"name": "sphere_drop", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128},
            "models": [{"material": material, "xyz": lattice_sphere(bits, center, radius_cells), "v0": (0, 0, 0), "params": prm}]}


def sand_column(bits=9, size_cells=(128, 306, 128), min_corner=None):
    """C3: Drucker-Prager sand column collapse; at bits 9 the default box holds 128*306*128*8 = 40.1 M particles.
    Reference sand defaults (particle_buffer.cuh:202-218) incl. its volume."""
    if min_corner is None:
        n = 1 << bits
        min_corner = ((n - size_cells[0]) // 2, 12, (n - size_cells[2]) // 2)
    lo = np.array(min_corner)
    hi = lo + np.array(size_cells)
    return {"name": "sand_column", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128},
            "models": [{"material": SAND, "xyz": lattice_box(bits, lo, hi), "v0": (0, 0, 0), "params": {}}]}


def scaled_sand_column(bits, fraction):
    """A geometrically similar, smaller sand column (same aspect ratio) for bounded CPU samples / tests."""
    s = fraction ** (1.0 / 3.0)
    full = np.array([128, 306, 128]) * (1 << bits) / 512.0
    size = np.maximum(4, np.round(full * s)).astype(int)
    return sand_column(bits, tuple(int(x) for x in size))


def sand_columns_layout(world, bits=9, size_cells=(128, 306, 128)):
    """Min corners of `world` adjacent sand columns on the floor of the domain, ceil(sqrt(world)) per row along x, rows
    along z, centred and block-aligned: the weak-scaling workload of bench.py (one C3 column per rank; touching columns
    share a face, so every rank has halo blocks from the first substep)."""
    n = 1 << bits
    cols = int(np.ceil(np.sqrt(world)))
    rows = (world + cols - 1) // cols
    x0 = ((n - size_cells[0] * cols) // 2) & ~3
    z0 = ((n - size_cells[2] * rows) // 2) & ~3
    if x0 < 12 or z0 < 12 or 12 + size_cells[1] > n - 12:
        raise ValueError(f"{world} columns of {size_cells} cells do not fit a {n}^3 grid")
    return [(x0 + size_cells[0] * (r % cols), 12, z0 + size_cells[2] * (r // cols)) for r in range(world)]


def sand_columns_rank(rank, world, bits=9, size_cells=(128, 306, 128)):
    """The particles of ONE rank of the weak-scaling workload (a rank never builds the other ranks' columns)."""
    return sand_column(bits, size_cells, sand_columns_layout(world, bits, size_cells)[rank])


def fluid_dam(bits=10, size_cells=(256, 192, 256), min_corner=(12, 12, 12)):
    """C5: weakly compressible J-fluid dam break (reference defaults particle_buffer.cuh:148-153).  The fixed substep of the
    bench / tests follows the acoustic CFL limit: sound speed sqrt(bulk * gamma / rho) = 16.9, dx / c = 2.3e-4 at bits 8 and
    5.8e-5 at bits 10 - dt = 1e-4 is fine up to bits 8 and halves with every bit beyond (2.5e-5 at bits 10; at 1e-4 the
    1024^3 run blows up within 2000 substeps, which bench.py's self-check reports as lost particles)."""
    lo = np.array(min_corner)
    hi = lo + np.array(size_cells)
    dt = 1e-4 if bits <= 8 else 1e-4 * 2.0 ** (8 - bits)
    return {"name": "fluid_dam", "bits": bits, "dt": dt, "config": {"max_ppc": 128},
            "models": [{"material": J_FLUID, "xyz": lattice_box(bits, lo, hi), "v0": (0, 0, 0), "params": {}}]}


def spinning_ball(bits=6, radius_cells=6.0, omega=(0.0, 0.0, 20.0), center=(0.5, 0.5, 0.5), v0=(0.0, 0.0, 0.0), youngs=5e3):
    """A fixed-corotated sphere in free space (gravity 0) that starts in rigid rotation `omega` (rad/s) about its centre: the velocity field
    v = v0 + omega x (x - centre), given to the engine as a model-level field (Engine.set_model_velocity_field)."""
    prm = {"volume": _vol(bits), "youngs_modulus": youngs, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "spinning_ball", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128, "gravity": 0.0},
            "models": [{"material": FIXED_COROTATED, "xyz": lattice_sphere(bits, center, radius_cells), "v0": tuple(v0), "omega": tuple(omega),
                        "pivot": tuple(center), "params": prm}]}


def sheared_block(bits=6, size_cells=(10, 8, 6), rate=15.0, v0=(0.25, 0.0, -0.5), youngs=5e3):
    """A fixed-corotated block in the middle of the domain (gravity 0) that starts in the shear flow v = v0 + G (x - centre) with
    G = rate * [[0, 1, 0], [0, 0, 0.5], [0, 0, 0]] (dv_x / dy = rate, dv_y / dz = rate / 2), a model-level field like spinning_ball's."""
    n = 1 << bits
    lo = np.array([(n - s) // 2 for s in size_cells])
    hi = lo + np.array(size_cells)
    centre = tuple(float(c) for c in (lo + hi - 1) * 0.5 / n)  # the lattice nodes lo .. hi - 1 carry the particles
    G = [0.0, rate, 0.0, 0.0, 0.0, 0.5 * rate, 0.0, 0.0, 0.0]  # row-major: G[r][c] = dv_r / dx_c
    prm = {"volume": _vol(bits), "youngs_modulus": youngs, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "sheared_block", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128, "gravity": 0.0},
            "models": [{"material": FIXED_COROTATED, "xyz": lattice_box(bits, lo, hi), "v0": tuple(v0), "velocity_gradient": G, "pivot": centre,
                        "params": prm}]}


def model_velocity_field(m):
    """(a, A) of a model dict's velocity field v = a + A x in float64 - A = "velocity_gradient" (row-major) + skew("omega"), a = v0 - A pivot -
    or None for a model without one."""
    if m.get("omega") is None and m.get("velocity_gradient") is None:
        return None
    A = np.zeros((3, 3))
    if m.get("velocity_gradient") is not None:
        A += np.asarray(m["velocity_gradient"], dtype=np.float64).reshape(3, 3)
    if m.get("omega") is not None:
        wx, wy, wz = (float(x) for x in m["omega"])
        A += np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    return np.asarray(m.get("v0", (0, 0, 0)), dtype=np.float64) - A @ np.asarray(m.get("pivot", (0, 0, 0)), dtype=np.float64), A


def split_slabs(xyz, parts, axis=0, block=None, tolerance=0.10, return_index=False):
    """Static particle partition of MGSP: equal-count slabs of the initial lattice along `axis`.

    block = (origin, width): the particle blocks' faces along the axis lie at origin + k * width (block_faces()).  The equal-count cuts are then
    moved to the nearest face, so that no particle block is shared by two ranks at the start: a slab whose two cut planes pass through blocks
    owns two layers of half-filled blocks, and G2P2G's cost is per iteration of a block, not per particle (C3 cut 8 ways along y: 77 block layers,
    9.6 per rank - an equal-count slab touches 11 layers, an aligned one holds 9 or 10).  Kept only if no piece grows beyond (1 + tolerance) of
    the equal share (and none is empty); otherwise the equal-count cut stands.

    return_index=True: (pieces, indices) - indices[i] the rows of `xyz` that piece i holds, in its order (pieces[i] == xyz[indices[i]]), so
    that per-particle arrays (velocity, affine, state ...) can be split with the positions."""
    col = xyz[:, axis]
    n = xyz.shape[0]
    sorted_already = col.size < 2 or bool(np.all(col[1:] >= col[:-1]))  # the lattice samplers emit particles sorted along x
    bounds = np.linspace(0, n, parts + 1).astype(np.int64)
    if block is not None and parts > 1 and n >= parts:
        order = None if sorted_already else np.argsort(col, kind="stable")
        cs = col if sorted_already else col[order]
        origin, width = block
        cuts = 0.5 * (cs[bounds[1:-1] - 1].astype(np.float64) + cs[bounds[1:-1]].astype(np.float64))  # between the two particles an equal-count cut separates
        faces = origin + np.round((cuts - origin) / width) * width
        snapped = np.concatenate([[0], np.searchsorted(cs, faces.astype(cs.dtype), side="left"), [n]]).astype(np.int64)
        sizes = np.diff(snapped)
        if sizes.min() > 0 and sizes.max() <= (1.0 + tolerance) * n / parts:
            bounds = snapped
        if order is not None:
            return _slab_pieces(xyz, [order[bounds[i]:bounds[i + 1]] for i in range(parts)], return_index)
        return _slab_pieces(xyz, [slice(bounds[i], bounds[i + 1]) for i in range(parts)], return_index)
    if sorted_already:
        return _slab_pieces(xyz, [slice(bounds[i], bounds[i + 1]) for i in range(parts)], return_index)
    order = np.argsort(col, kind="stable")
    return _slab_pieces(xyz, np.array_split(order, parts), return_index)


def _slab_pieces(xyz, rows, return_index):
    """split_slabs' return: the pieces xyz[rows[i]] (rows: slices or index arrays) and, if asked for, the rows as int64 index arrays."""
    pieces = [np.ascontiguousarray(xyz[r]) for r in rows]
    if not return_index:
        return pieces
    return pieces, [np.arange(r.start, r.stop, dtype=np.int64) if isinstance(r, slice) else np.asarray(r, dtype=np.int64) for r in rows]


def block_faces(bits):
    """(origin, width) of the particle blocks' faces along any axis, in world units: a particle at x belongs to block (lround(x / dx) - 2) / 4
    (particle_block_key, mpm_kernels.hpp; reference: Projects/GMPM/mgmpm_kernels.cuh:21-36), i.e. block k holds x / dx in [4 k + 1.5, 4 k + 5.5)."""
    dx = 1.0 / (1 << bits)
    return 1.5 * dx, 4.0 * dx


def split_boxes(xyz, shape, block=None, return_index=False):
    """Static particle partition into shape = (nx, ny, nz) equal-count boxes of the initial lattice: nx slabs along x, each cut into ny along
    y, each of those into nz along z; block: cut planes moved to particle-block faces (split_slabs) (the reference's scenarios put their per-GPU bodies side by side in x and z, Projects/MGSP/mgsp.cu:52-57,
    :67-72; SURVEY 8(e): "slabs / octants").  Returns the nx * ny * nz particle arrays, x-major; return_index=True: (arrays, indices) with
    arrays[i] == xyz[indices[i]] (split_slabs)."""
    parts = [xyz]
    index = [np.arange(xyz.shape[0], dtype=np.int64)] if return_index else None
    for axis, n in enumerate(shape):
        if n <= 1:
            continue
        if return_index:
            cut = [split_slabs(p, n, axis, block=block, return_index=True) for p in parts]
            index = [rows[sub] for rows, (_, subs) in zip(index, cut) for sub in subs]
            parts = [q for pieces, _ in cut for q in pieces]
        else:
            parts = [q for p in parts for q in split_slabs(p, n, axis, block=block)]
    return (parts, index) if return_index else parts


PARTITION_SHAPES = {  # name -> world size -> (nx, ny, nz); "octants" halves every axis it can (x first: 2 -> x, 4 -> x z, 8 -> x y z)
    "y": lambda w: (1, w, 1), "x": lambda w: (w, 1, 1), "z": lambda w: (1, 1, w),
    "octants": lambda w: {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 1, 2), 8: (2, 2, 2)}[w],
    "xz-columns": lambda w: {1: (1, 1, 1), 2: (2, 1, 1), 4: (2, 1, 2), 8: (4, 1, 2)}[w],
    "y-x": lambda w: {1: (1, 1, 1), 2: (1, 2, 1), 4: (2, 2, 1), 8: (2, 4, 1)}[w],
}


def total_particles(scene):
    return int(sum(m["xyz"].shape[0] for m in scene["models"]))


def sphere_level_set(bits, centre, radius):
    """Node-sampled signed distance (negative inside) and gradient of a sphere, in the layout of the reference's
    `<name>_sdf.bin` / `_grad_{0,1,2}.bin` files (Projects/MGSP/boundary_condition.cuh:252-321): (N, N, N) and (3, N, N, N)."""
    n = 1 << bits
    ax = np.arange(n, dtype=np.float64) / n
    X, Y, Z = np.meshgrid(ax - centre[0], ax - centre[1], ax - centre[2], indexing="ij")
    r = np.sqrt(X * X + Y * Y + Z * Z)
    rs = np.maximum(r, 1e-12)
    return (r - radius).astype(np.float32), np.stack([X / rs, Y / rs, Z / rs]).astype(np.float32)


def sphere_on_obstacle(bits=6, radius_cells=5.0, obstacle_cells=6.0, boundary="slip", friction=0.3, speed=1.0, material=FIXED_COROTATED):
    """An elastic sphere thrown onto a fixed spherical level-set obstacle (the MGSP collision-object path)."""
    dx = 1.0 / (1 << bits)
    c_obs = (0.5, 0.34, 0.5)
    c_sph = (0.5 + 1.5 * dx, c_obs[1] + (obstacle_cells + radius_cells + 1.5) * dx, 0.5)
    vol = float(np.float32(dx ** 3 / 8))
    sdf, grad = sphere_level_set(bits, c_obs, obstacle_cells * dx)
    return {"name": "sphere_on_obstacle", "bits": bits, "dt": 1e-4, "config": {},
            "models": [{"material": material, "xyz": lattice_sphere(bits, c_sph, radius_cells), "v0": (0.0, -speed, 0.0),
                        "params": {"volume": vol, "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}],
            "collision": {"sdf": sdf, "grad": grad, "type": {"sticky": 0, "slip": 1, "separate": 2}[boundary], "friction": friction}}


def sphere_through_block(bits=6, block_cells=(20, 10, 20), radius_cells=5.0, gap_cells=2.0, speed=1.0, boundary="sticky", friction=0.3,
                         omega=(0.0, 0.0, 0.0), dsdt=0.0, rot_mat=None, animate=True, dt=1e-4, material=FIXED_COROTATED):
    """A block of material at rest (no gravity) and a spherical level set that starts `gap_cells` clear of its -x face and translates
    through it along +x (the moving collision object: the clock runs unless animate=False).  The level set is centred at `trans`, so
    omega / dsdt / rot_mat turn and grow the sphere about its own moving centre."""
    dx, n = 1.0 / (1 << bits), 1 << bits
    lo = [n // 2 - int(block_cells[d]) // 2 for d in range(3)]
    hi = [lo[d] + int(block_cells[d]) for d in range(3)]
    # (the centre sits off the block's mid-planes by fractions of a cell, so that no node lies on a symmetry plane of the contact)
    centre = ((lo[0] - gap_cells - radius_cells) * dx, (lo[1] + hi[1]) / 2 * dx + 0.75 * dx, (lo[2] + hi[2]) / 2 * dx - 0.5 * dx)
    sdf, grad = sphere_level_set(bits, centre, radius_cells * dx)
    col = {"sdf": sdf, "grad": grad, "type": {"sticky": 0, "slip": 1, "separate": 2}[boundary], "friction": friction,
           "trans": centre, "trans_vel": (speed, 0.0, 0.0), "omega": omega, "dsdt": dsdt, "animate": animate}
    if rot_mat is not None:
        col["rot_mat"] = rot_mat
    return {"name": "sphere_through_block", "bits": bits, "dt": dt, "config": {"gravity": 0.0},
            "models": [{"material": material, "xyz": lattice_box(bits, lo, hi), "v0": (0.0, 0.0, 0.0),
                        "params": {"volume": _vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}],
            "collision": col}


def _as_shape(scene, radius):
    """The level-set sphere of a scene as the same sphere given in closed form: scene["colliders"] instead of scene["collision"].  The
    level set is centred at the domain point `centre` and sampled in domain coordinates, so the shape's centre `a` is that point."""
    col = scene.pop("collision")
    centre = col.pop("centre")
    shape = {k: v for k, v in col.items() if k not in ("sdf", "grad")}
    shape.update(kind="sphere", a=tuple(float(c) for c in centre), radius=float(radius))
    scene["colliders"] = [shape]
    scene["name"] += "_analytic"
    return scene


def sphere_on_obstacle_analytic(bits=6, radius_cells=5.0, obstacle_cells=6.0, boundary="slip", friction=0.3, speed=1.0, material=FIXED_COROTATED):
    """sphere_on_obstacle with the obstacle as an analytic sphere (Engine.set_collision_shape): no level set is rasterised or stored."""
    sc = sphere_on_obstacle(bits, radius_cells, obstacle_cells, boundary, friction, speed, material)
    sc["collision"]["centre"] = (0.5, 0.34, 0.5)
    return _as_shape(sc, obstacle_cells / (1 << bits))


def sphere_through_block_analytic(bits=6, block_cells=(20, 10, 20), radius_cells=5.0, gap_cells=2.0, speed=1.0, boundary="sticky", friction=0.3,
                                  omega=(0.0, 0.0, 0.0), dsdt=0.0, rot_mat=None, animate=True, dt=1e-4, material=FIXED_COROTATED):
    """sphere_through_block with the moving sphere as an analytic shape: same centre, radius, motion and clock."""
    sc = sphere_through_block(bits, block_cells, radius_cells, gap_cells, speed, boundary, friction, omega, dsdt, rot_mat, animate, dt, material)
    sc["collision"]["centre"] = sc["collision"]["trans"]
    return _as_shape(sc, radius_cells / (1 << bits))


def ball_into_sand(bits=6, radius_cells=4.0, density=8e3, drop_cells=2.0, bed_cells=(32, 12, 32), friction=0.4, speed=0.0, dt=1e-4):
    """A dense sphere - a rigid body (Engine.set_collider_body: the material pushes it back) - dropped from `drop_cells` above (or thrown down at `speed` onto) a bed of
    Drucker-Prager sand (rho 1e3) that lies on the floor.  The sphere is eight times as dense as the sand, so the mass of the nodes it touches
    stays well below its own (the explicit coupling's stable range; Engine.collider_body(0)["max_mass_ratio"] tells)."""
    dx, n = 1.0 / (1 << bits), 1 << bits
    lo = [(n - bed_cells[0]) // 2, 8, (n - bed_cells[2]) // 2]
    hi = [lo[d] + int(bed_cells[d]) for d in range(3)]
    centre = (0.5 + 0.25 * dx, (hi[1] + drop_cells + radius_cells) * dx, 0.5 - 0.25 * dx)
    return {"name": "ball_into_sand", "bits": bits, "dt": dt, "config": {"max_ppc": 128},
            "models": [{"material": SAND, "xyz": lattice_box(bits, lo, hi), "v0": (0.0, 0.0, 0.0), "params": {"volume": _vol(bits)}}],
            "colliders": [{"kind": "sphere", "a": centre, "radius": radius_cells * dx, "type": 2, "friction": friction, "trans_vel": (0.0, -speed, 0.0),
                           "body": {"density": density}}]}


def floating_box(bits=6, half_cells=(6, 8, 6), density=5e2, pool_cells=(40, 20, 40), speed=0.0, dt=1e-4):
    """A box of half the fluid's density - a rigid body - set down half submerged (or pushed down at `speed`) in a pool of the J-fluid (rho 1e3) on the floor: it bobs
    about the depth at which it displaces its own weight.  The box is 16 cells tall by default: the nodes it touches form a one-cell shell
    around its wetted faces, whose mass then stays near a fifth of the box's (max_mass_ratio)."""
    dx, n = 1.0 / (1 << bits), 1 << bits
    lo = [(n - pool_cells[0]) // 2, 8, (n - pool_cells[2]) // 2]
    hi = [lo[d] + int(pool_cells[d]) for d in range(3)]
    centre = (0.5, hi[1] * dx, 0.5)
    xyz = lattice_box(bits, lo, hi)
    b = np.array(half_cells, dtype=np.float64) * dx
    inside = np.all(np.abs(xyz.astype(np.float64) - np.array(centre)) < b + 0.5 * dx, axis=1)  # no fluid where the box stands
    return {"name": "floating_box", "bits": bits, "dt": dt, "config": {"max_ppc": 128},
            "models": [{"material": J_FLUID, "xyz": np.ascontiguousarray(xyz[~inside]), "v0": (0.0, 0.0, 0.0), "params": {"volume": _vol(bits)}}],
            "colliders": [{"kind": "box", "a": centre, "b": tuple(float(v) for v in b), "type": 1, "friction": 0.0, "trans_vel": (0.0, -speed, 0.0),
                           "body": {"density": density}}]}


def colliders_demo(bits=6, boundary="slip", friction=0.3, speed=1.0, dt=1e-4):
    """One of each: an elastic block falls onto a tilted floor wedge (half-space) beside a sticky box and a fixed rod (capsule), while a sphere
    sweeps through along +x; the clock runs.  Four analytic colliders, no level set."""
    dx, n = 1.0 / (1 << bits), 1 << bits
    lo, hi = [n // 2 - 6, n // 2 - 2, n // 2 - 6], [n // 2 + 6, n // 2 + 6, n // 2 + 6]
    kind = {"sticky": 0, "slip": 1, "separate": 2}[boundary]
    y0 = lo[1] * dx
    cols = [{"kind": "halfspace", "a": (0.5, y0 - 3 * dx, 0.5), "b": (0.2, -1.0, 0.0), "inside_out": True, "type": kind, "friction": friction},
            {"kind": "box", "a": (0.5 + 9 * dx, y0 - 2 * dx, 0.5), "b": (2 * dx, 3 * dx, 4 * dx), "type": 0},
            {"kind": "capsule", "a": (0.5 - 8 * dx, y0 - 2 * dx, 0.5 - 6 * dx), "b": (0.5 - 8 * dx, y0 - 2 * dx, 0.5 + 6 * dx), "radius": 1.5 * dx, "type": kind,
             "friction": friction},
            {"kind": "sphere", "a": ((lo[0] - 7) * dx, 0.5 + 2 * dx, 0.5), "radius": 4 * dx, "type": kind, "friction": friction,
             "trans_vel": (speed, 0.0, 0.0), "animate": True}]
    return {"name": "colliders_demo", "bits": bits, "dt": dt, "config": {},
            "models": [{"material": FIXED_COROTATED, "xyz": lattice_box(bits, lo, hi), "v0": (0.0, 0.0, 0.0),
                        "params": {"volume": _vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}],
            "colliders": cols}


def ramp_heights(bits=6, slope=0.3, base_cells=None, berm_cells=1.5, berm_at_cells=-8.0, berm_width_cells=3.0, ripple_cells=0.25):
    """The terrain of block_on_ramp: (N + 1) x (N + 1) heights at the grid nodes' (x, z) (spacing dx, origin 0), float32 [nx, nz].  A ramp that
    rises along +x (downhill is -x) through `base_cells` at the domain's centre, a Gaussian berm across it `berm_at_cells` from the centre, and
    a shallow ripple along z, so that neither gradient is zero anywhere near the block."""
    n, dx = 1 << bits, 1.0 / (1 << bits)
    base = (n // 2 - 1 if base_cells is None else base_cells) * dx
    X, Z = np.meshgrid(np.arange(n + 1) * dx, np.arange(n + 1) * dx, indexing="ij")
    h = base + slope * (X - 0.5)
    h = h + berm_cells * dx * np.exp(-(((X - 0.5) - berm_at_cells * dx) / (berm_width_cells * dx)) ** 2)
    h = h + ripple_cells * dx * np.sin(2 * np.pi * 3 * Z + 0.4)
    return h.astype(np.float32)


def block_on_ramp(bits=6, block_cells=(6, 4, 6), speed=0.5, boundary="slip", friction=0.1, slope=0.3, trans_vel=(0.0, 0.0, 0.0), animate=False, dt=1e-4,
                  material=FIXED_COROTATED):
    """A small elastic block dropped (v0 = (0, -speed, 0)) onto terrain given as a heightfield (Engine.set_collision_heightfield): a ramp with
    a berm downhill of the block (ramp_heights).  The block's lowest particle layer starts within a cell of the highest ground under it, so
    the contact begins in the first substeps; trans_vel / animate move the terrain.  No level set is rasterised or stored."""
    n, dx = 1 << bits, 1.0 / (1 << bits)
    heights = ramp_heights(bits, slope)
    lo = [n // 2 - int(block_cells[0]) // 2, 0, n // 2 - int(block_cells[2]) // 2]
    hi = [lo[0] + int(block_cells[0]), 0, lo[2] + int(block_cells[2])]
    ground = float(heights[lo[0]:hi[0] + 1, lo[2]:hi[2] + 1].max())
    lo[1] = int(np.floor(ground / dx)) + 1
    hi[1] = lo[1] + int(block_cells[1])
    col = {"kind": "heightfield", "heights": heights, "origin": (0.0, 0.0), "spacing": dx, "type": {"sticky": 0, "slip": 1, "separate": 2}[boundary],
           "friction": friction, "trans_vel": trans_vel, "animate": animate}
    return {"name": "block_on_ramp", "bits": bits, "dt": dt, "config": {},
            "models": [{"material": material, "xyz": lattice_box(bits, lo, hi), "v0": (0.0, -speed, 0.0),
                        "params": {"volume": _vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}],
            "colliders": [col]}


def box_mesh(lo, hi):
    """The box lo .. hi as a closed triangle mesh for Engine.set_collision_mesh: (8, 3) float32 vertices - vertex 4 i + 2 j + k takes hi on the
    axes whose bit is set - and (12, 3) int32 faces, two per side, counter-clockwise seen from outside."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if i else lo)[0], (hi if j else lo)[1], (hi if k else lo)[2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # -x, +x, -y, +y, -z, +z
    f = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    return v, f


def icosphere(centre, radius, subdivisions):
    """A sphere as a closed triangle mesh: the icosahedron, every triangle split in four `subdivisions` times with the new vertices pushed
    onto the sphere (20 x 4^subdivisions faces, welded, counter-clockwise seen from outside).  Returns (nv, 3) float32, (nt, 3) int32."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.sqrt(1.0 + g * g) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        nf = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.asarray(centre, dtype=np.float64)[None, :] + float(radius) * np.array(v)
    return verts.astype(np.float32), np.array(f, dtype=np.int32)


def sphere_on_obstacle_mesh(bits=6, radius_cells=5.0, obstacle_cells=6.0, boundary="slip", friction=0.3, speed=1.0, material=FIXED_COROTATED, subdivisions=3,
                            body_cells=None, **motion):
    """sphere_on_obstacle with the obstacle as an icosphere mesh (Engine.set_collision_mesh) instead of sphere_level_set: the field is built on
    the device.  motion: further fields of the object (trans_vel, omega, animate ...).  body_cells = (cx, 2, cz): the thrown body is a small
    lattice block resting on the obstacle's top instead of the sphere, its two node layers in y inside one particle block (with cx, cz = 2 the
    whole block is: a body on which the engine is deterministic)."""
    sc = sphere_on_obstacle(bits, radius_cells, obstacle_cells, boundary, friction, speed, material)
    col = {k: v for k, v in sc.pop("collision").items() if k not in ("sdf", "grad")}
    vertices, faces = icosphere((0.5, 0.34, 0.5), obstacle_cells / (1 << bits), subdivisions)
    sc["collision_mesh"] = {**col, **motion, "vertices": vertices, "faces": faces}
    sc["name"] += "_mesh"
    if body_cells is not None:
        n = 1 << bits
        j = int(np.ceil(0.34 * n + obstacle_cells))
        j += 1 if j % 4 == 1 else 0  # nodes j, j + 1 share a particle block (block_faces) unless j = 1 mod 4
        lo = [n // 2 - int(body_cells[0]) // 2, j, n // 2 - int(body_cells[2]) // 2]
        sc["models"][0]["xyz"] = lattice_box(bits, lo, [lo[0] + int(body_cells[0]), j + int(body_cells[1]), lo[2] + int(body_cells[2])])
    return sc


def mesh_drop(bits=6, radius_cells=9.0, center=(0.5, 0.3, 0.5), material=FIXED_COROTATED, subdivisions=3, margin=0.0):
    """sphere_drop with the body given as a triangle mesh: an icosphere of radius_cells about `center`, filled with lattice particles on the
    device (Engine.init_model_mesh) and dropped on the floor under gravity.  Same centre, radius, material and volume as
    sphere_drop(bits, radius_cells, center) - lattice_sphere's particles less the thin shell between the polyhedron and its sphere - so the
    two runs are directly comparable.  The model carries "mesh" instead of "xyz": its particle count is known once the engine has added it."""
    prm = {"volume": _vol(bits)} if material != SAND else {}
    vertices, faces = icosphere(center, radius_cells / (1 << bits), subdivisions)
    return {"name": "mesh_drop", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128},
            "models": [{"material": material, "mesh": {"vertices": vertices, "faces": faces, "margin": margin}, "v0": (0, 0, 0), "params": prm}]}


def two_paddles(bits=6, radius_cells=6.0, paddle_cells=(3.0, 10.0, 10.0), gap_cells=2.0, speed=1.0, boundary="slip", friction=0.3, spacing_cells=0.5, pad=2,
                material=FIXED_COROTATED, shape="box", subdivisions=2, dt=1e-4):
    """A sphere_drop-sized ball at rest between two mesh bodies - volumes in slots 0 and 1 (Engine.set_collision_volume_mesh), each built on
    the device from a box_mesh (shape="box") or an icosphere (shape="icosphere", radius paddle_cells[1] / 2) sampled spacing_cells dx apart -
    that move toward each other along x at +-speed on the one running clock: two mesh colliders in one context, each with its own trans_vel.
    The paddles start gap_cells dx off the ball; no gravity, so the material's x momentum comes from the paddles alone."""
    n = 1 << bits
    dx = 1.0 / n
    prm = {"volume": _vol(bits)} if material != SAND else {}
    c = np.array([0.5, 0.5, 0.5])
    half = np.asarray(paddle_cells, dtype=np.float64) * dx / 2
    off = (radius_cells + gap_cells) * dx + half[0]
    colliders = []
    for side in (-1.0, 1.0):
        centre = c + np.array([side * off, 0.0, 0.0])
        vertices, faces = box_mesh(centre - half, centre + half) if shape == "box" else icosphere(centre, half[1], subdivisions)
        colliders.append({"kind": "volume_mesh", "vertices": vertices, "faces": faces, "spacing": spacing_cells * dx, "pad": pad, "type": {"sticky": 0, "slip": 1, "separate": 2}[boundary],
                          "friction": friction, "trans_vel": (-side * speed, 0.0, 0.0), "animate": True})
    return {"name": "two_paddles", "bits": bits, "dt": dt, "config": {"max_ppc": 128, "gravity": 0.0},
            "models": [{"material": material, "xyz": lattice_sphere(bits, tuple(c), radius_cells), "v0": (0, 0, 0), "params": prm}], "colliders": colliders}


class Emitter:
    """A host-side particle source: a nozzle that turns into calls of Engine.emit (mpm_emit_particles), one lattice layer at a time.

    shape "box": lo, hi (world units) - the nozzle's cross-section is the box's extent on the two axes across the flow, its plane passes through
    the box's centre; shape "disc": center, radius, and a normal along the flow axis.  velocity: along one principal axis (the flow axis; a
    disc's normal must name the same axis).  The particles are the reference's lattice - 8 per cell, at node -+ 0.25 dx, i.e. the odd
    multiples of dx / 4 - cut by the cross-section, in the lattice plane nearest the nozzle's centre.  One layer is due every
    (dx / 2) / |v| seconds: t_k = start + k (dx / 2) / |v| for every t_k < end.  A layer due at t_k is handed out by the first due(t) with
    t >= t_k, at x + v (t - t_k): the stream is the same lattice whatever the substep sizes are.  The same rule in C++: host/emitter_rule.hpp."""

    def __init__(self, bits, shape, velocity, start=0.0, end=np.inf, model=0, lo=None, hi=None, center=None, radius=None, normal=None):
        v = np.asarray(velocity, dtype=np.float64).reshape(3)
        if np.count_nonzero(v) != 1 or not np.isfinite(v).all():
            raise ValueError(f"Emitter: velocity {tuple(v)} must be along one principal axis")
        self.bits, self.model, self.velocity = int(bits), int(model), v
        self.axis = int(np.flatnonzero(v)[0])
        self.start, self.end = float(start), float(end)
        n = 1 << self.bits
        h = 0.5 / n                                                  # the lattice spacing, dx / 2
        self.period = h / abs(v[self.axis])
        if shape == "disc":
            if center is None or radius is None:
                raise ValueError("Emitter: a disc needs center and radius")
            if normal is not None and (np.count_nonzero(normal) != 1 or int(np.flatnonzero(normal)[0]) != self.axis):
                raise ValueError("Emitter: a disc's normal must lie along the velocity's axis")
            c = np.asarray(center, dtype=np.float64).reshape(3)
        elif shape == "box":
            if lo is None or hi is None:
                raise ValueError("Emitter: a box needs lo and hi")
            lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
            c = (lo + hi) / 2
        else:
            raise ValueError(f"Emitter: unknown shape {shape!r} ('box' or 'disc')")
        j = int(min(max(np.floor(c[self.axis] / h), 0), 2 * n - 1))  # the lattice plane (j + 1/2) h nearest the centre; a tie goes to the lower one
        if j > 0 and c[self.axis] == j * h:
            j -= 1
        t = [d for d in range(3) if d != self.axis]
        coords = (np.arange(2 * n) + 0.5) * h
        A, B = np.meshgrid(coords, coords, indexing="ij")
        if shape == "disc":
            keep = (A - c[t[0]]) ** 2 + (B - c[t[1]]) ** 2 <= float(radius) ** 2
        else:
            keep = (A >= lo[t[0]]) & (A <= hi[t[0]]) & (B >= lo[t[1]]) & (B <= hi[t[1]])
        self.layer = np.empty((int(keep.sum()), 3), dtype=np.float64)
        self.layer[:, self.axis] = (j + 0.5) * h
        self.layer[:, t[0]], self.layer[:, t[1]] = A[keep], B[keep]
        self.next_layer = 0

    @classmethod
    def from_dict(cls, bits, d):
        """An entry of a scene's "emitters": {"model", "shape": "box" | "disc", "velocity", "start", "end", and lo / hi or center / radius / normal}."""
        keys = ("lo", "hi", "center", "radius", "normal")
        return cls(bits, d["shape"], d["velocity"], d.get("start", 0.0), d.get("end", np.inf), d.get("model", 0), **{k: d[k] for k in keys if k in d})

    def due(self, t):
        """The positions to emit at the substep boundary `t`, (m, 3) float32 - every layer that is due and has not been handed out - or an empty array."""
        out = []
        while True:
            tk = self.start + self.next_layer * self.period
            if not (tk < self.end and tk <= t):
                break
            out.append(self.layer + self.velocity[None, :] * (t - tk))
            self.next_layer += 1
        if not out:
            return np.zeros((0, 3), dtype=np.float32)
        return np.ascontiguousarray(np.concatenate(out), dtype=np.float32)


def faucet(bits=6, radius_cells=3.0, speed=2.0, height_cells=None, start=0.0, end=0.05, dt=1e-4):
    """A J-fluid jet into the unit box: the model starts EMPTY and a disc nozzle under the top wall zone pours it in, straight down at `speed`
    (scene key "emitters", Engine.main_loop serves them).  The nozzle sits height_cells above the floor (default: 10 cells under the top)."""
    n = 1 << bits
    dx = 1.0 / n
    y = (n - 10 if height_cells is None else height_cells) * dx
    return {"name": "faucet", "bits": bits, "dt": dt, "config": {"max_ppc": 16},
            "models": [{"material": J_FLUID, "xyz": np.zeros((0, 3), dtype=np.float32), "v0": (0.0, 0.0, 0.0), "params": {"volume": _vol(bits), "rho": 1e3}}],
            "emitters": [{"model": 0, "shape": "disc", "center": (0.5, y, 0.5), "normal": (0.0, -1.0, 0.0), "radius": radius_cells * dx,
                          "velocity": (0.0, -speed, 0.0), "start": start, "end": end}]}


def sand_pour(bits=6, radius_cells=2.5, speed=1.0, drop_cells=10.0, start=0.0, end=0.05, dt=1e-4):
    """Sand poured from a disc onto block_on_ramp's heightfield: the scene's elastic block is replaced by an empty sand model that a nozzle
    drop_cells above the terrain's centre fills."""
    sc = block_on_ramp(bits=bits, dt=dt)
    n = 1 << bits
    dx = 1.0 / n
    ground = float(sc["colliders"][0]["heights"][n // 2, n // 2])
    sc["name"] = "sand_pour"
    sc["config"] = {"max_ppc": 16}
    sc["models"] = [{"material": SAND, "xyz": np.zeros((0, 3), dtype=np.float32), "v0": (0.0, 0.0, 0.0), "params": {}}]
    sc["emitters"] = [{"model": 0, "shape": "disc", "center": (0.5, ground + drop_cells * dx, 0.5), "normal": (0.0, -1.0, 0.0), "radius": radius_cells * dx,
                       "velocity": (0.0, -speed, 0.0), "start": start, "end": end}]
    return sc


class Sink:
    """A host-side particle sink: a region that turns into calls of Engine.remove (mpm_remove_particles), one sweep at a time.

    region: one region dict of Engine.remove - set_collision_shape's keywords (kind, a, b, radius, inside_out) or the scene files' keys (point /
    normal, center, half_extents) -, in domain coordinates; model: the model it drains, -1 for all.  Sweep k is due at t_k = start + k period
    for every t_k < end; it is served by the first substep boundary t >= t_k, and several sweeps that are due at one boundary make one call
    (a second sweep of the same particles would find nothing).  A sweep that selects nothing costs one counting pass.  The same rule in C++:
    host/sink_rule.hpp."""

    def __init__(self, bits, region, model=-1, start=0.0, end=np.inf, period=None):
        if period is None or not (float(period) > 0.0) or not np.isfinite(float(period)):
            raise ValueError("Sink: period is required and must be > 0")
        if not isinstance(region, dict) or ("kind" not in region and "shape" not in region):
            raise ValueError("Sink: region must be a dict with a kind")
        self.bits, self.model, self.region = int(bits), int(model), dict(region)
        self.start, self.end, self.period = float(start), float(end), float(period)
        self.next_sweep = 0

    @classmethod
    def from_dict(cls, bits, d):
        """An entry of a scene's "sinks": the region's keys beside {"model", "start", "end", "period"}."""
        own = ("model", "start", "end", "period")
        return cls(bits, {k: v for k, v in d.items() if k not in own}, d.get("model", -1), d.get("start", 0.0), d.get("end", np.inf), d.get("period"))

    def due(self, t):
        """How many sweeps the substep boundary `t` serves: every sweep that is due and has not been served (0: no call)."""
        k = 0
        while True:
            tk = self.start + self.next_sweep * self.period
            if not (tk < self.end and tk <= t):
                break
            self.next_sweep += 1
            k += 1
        return k


def fountain(bits=6, radius_cells=3.0, speed=2.0, height_cells=None, sink_cells=4.0, period=None, start=0.0, end=0.05, dt=1e-4):
    """faucet with a drain: a sink box over the whole floor that reaches sink_cells above the floor's wall zone (8 cells, where the sticky wall
    holds the grid still and nothing would ever arrive), swept every `period` (default: the emitter's layer period, one sweep per emitted
    layer).  What the nozzle pours in leaves through the floor, so the particle count reaches a steady state (scene key "sinks")."""
    sc = faucet(bits=bits, radius_cells=radius_cells, speed=speed, height_cells=height_cells, start=start, end=end, dt=dt)
    dx = 1.0 / (1 << bits)
    top = (8.0 + sink_cells) * dx
    sc["name"] = "fountain"
    sc["sinks"] = [{"model": 0, "kind": "box", "center": (0.5, top / 2, 0.5), "half_extents": (0.5, top / 2, 0.5),
                    "start": start, "period": (dx / 2) / speed if period is None else period}]
    return sc


def drain(bits=6, block_cells=12, gap_cells=4.0, period=1e-3, dt=1e-4):
    """A J-fluid block that falls through a gap into a sink slab: the block hangs gap_cells above a half-space sink whose plane lies under it,
    and everything that sinks below the plane is taken out at the next sweep."""
    n = 1 << bits
    dx = 1.0 / n
    lo = n // 2 - block_cells // 2
    y0 = n // 3
    plane = (y0 - gap_cells) * dx
    return {"name": "drain", "bits": bits, "dt": dt, "config": {"max_ppc": 16},
            "models": [{"material": J_FLUID, "xyz": lattice_box(bits, (lo, y0, lo), (lo + block_cells, y0 + block_cells, lo + block_cells)), "v0": (0.0, 0.0, 0.0),
                        "params": {"volume": _vol(bits), "rho": 1e3}}],
            "sinks": [{"model": 0, "kind": "halfspace", "point": (0.5, plane, 0.5), "normal": (0.0, 1.0, 0.0), "period": period}]}


class ForceEntry:
    """A scene's force field with its lifetime: `field` holds Engine.set_force_field's keywords (kind, vec, centre, strength, swirl, pull, lift,
    soft, falloff, region, feather).  The rule: the entry is installed at the first substep boundary t where start <= t < end holds and removed
    at the first boundary where it no longer holds (start == end: never installed).  The same rule in C++: host/force_rule.hpp."""

    def __init__(self, field, start=0.0, end=np.inf):
        if not isinstance(field, dict) or "kind" not in field:
            raise ValueError("ForceEntry: field must be a dict with a kind")
        self.field, self.start, self.end = dict(field), float(start), float(end)
        self.installed = False

    @classmethod
    def from_dict(cls, d):
        """An entry of a scene's "forces": set_force_field's keywords beside {"start", "end"}."""
        return cls({k: v for k, v in d.items() if k not in ("start", "end")}, d.get("start", 0.0), d.get("end", np.inf))

    def due(self, t):
        """What the substep boundary `t` asks for: +1 install, -1 remove, 0 nothing."""
        want = self.start <= t < self.end
        act = int(want) - int(self.installed)
        self.installed = want
        return act


def sand_in_wind(bits=6, column_cells=(8, 16, 8), wind=(3.0, 0.0, 0.0), rate=50.0, feather_cells=2.0, start=0.0, end=np.inf, dt=1e-4):
    """A sand column under gravity with wind from the side: a DRAG field toward the horizontal velocity `wind` in a box over the upper half of
    the domain, its edge feathered over feather_cells (scene key "forces")."""
    n = 1 << bits
    dx = 1.0 / n
    lo = (n // 2 - column_cells[0] // 2, 8, n // 2 - column_cells[2] // 2)
    sc = {"name": "sand_in_wind", "bits": bits, "dt": dt, "config": {"max_ppc": 16},
          "models": [{"material": SAND, "xyz": lattice_box(bits, lo, tuple(lo[d] + column_cells[d] for d in range(3))), "v0": (0.0, 0.0, 0.0),
                      "params": {"volume": _vol(bits), "rho": 1e3}}],
          "forces": [{"kind": "drag", "vec": tuple(wind), "strength": rate, "feather": feather_cells * dx, "start": start, "end": end,
                      "region": {"kind": "box", "center": (0.5, (lo[1] + column_cells[1]) * dx, 0.5), "half_extents": (0.5, column_cells[1] * dx / 2, 0.5)}}]}
    return sc


def stirred_tank(bits=6, pool_cells=(24, 10, 24), swirl=40.0, pull=0.0, radius_cells=8.0, end=5e-3, dt=1e-4):
    """J-fluid in a box-shaped container (an inside-out box, slip), stirred: a VORTEX field about the vertical axis through the middle of the pool in a capsule region along
    that axis, switched off at `end` (scene keys "colliders", "forces")."""
    n = 1 << bits
    dx = 1.0 / n
    lo = (n // 2 - pool_cells[0] // 2, 10, n // 2 - pool_cells[2] // 2)
    top = (lo[1] + pool_cells[1]) * dx
    return {"name": "stirred_tank", "bits": bits, "dt": dt, "config": {"max_ppc": 16},
            "models": [{"material": J_FLUID, "xyz": lattice_box(bits, lo, tuple(lo[d] + pool_cells[d] for d in range(3))), "v0": (0.0, 0.0, 0.0),
                        "params": {"volume": _vol(bits), "rho": 1e3}}],
            "colliders": [{"kind": "box", "a": (0.5, 0.5, 0.5), "b": ((pool_cells[0] / 2 + 2) * dx, 0.5 - 9 * dx, (pool_cells[2] / 2 + 2) * dx), "inside_out": True,
                           "type": 1, "friction": 0.0}],
            "forces": [{"kind": "vortex", "vec": (0.0, 1.0, 0.0), "centre": (0.5, 0.0, 0.5), "swirl": swirl, "pull": pull, "start": 0.0, "end": end,
                        "region": {"kind": "capsule", "a": (0.5, lo[1] * dx, 0.5), "b": (0.5, top, 0.5), "radius": radius_cells * dx}}]}

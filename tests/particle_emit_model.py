"""What mpm_emit_particles promises, stated in NumPy (tests/test_particle_emit_model_cpu.py, tests/test_particle_emit_gpu.py), and the layer rule of
scenes.Emitter stated a second time, from its definition.

The emission adds particles to a context at a substep boundary.  Afterwards
  - the particle set of the model is the old set and the new particles, every one with the state it had or was given (merged_particles);
  - a grid node that no new particle's 27-node stencil reaches holds the bits it held (reached_nodes), a reached node holds the old value plus the
    set-up P2G of the new particles alone - particle_init_model's rasterisation (expected_grid);
  - the new particles' ids are old n .. old n + n - 1 in input order (new_ids), the model's n and its bucketed count grow by n (books_after).

Test infrastructure only."""
import itertools

import numpy as np

import particle_init_model as pim
from face_scenes import lround_half_away

U = pim.U


# ---- the particle set ----------------------------------------------------------------------------------------------------------------------------
def default_state9(material_is_fluid, n):
    """the stress-free state as mpm_retrieve_state returns it: b = I, or J = 1 in entry 0"""
    s = np.zeros((n, 9), np.float32)
    s[:, 0] = 1.0
    if not material_is_fluid:
        s[:, 4] = s[:, 8] = 1.0
    return s


def merged_particles(old, new):
    """old, new: dicts of "xyz" (n, 3), "state9" (n, 9), "logjp" (n,) float32 and optionally "ids" (n,): the model after the emission, old rows first"""
    out = {k: np.concatenate([np.asarray(old[k]), np.asarray(new[k])]) for k in ("xyz", "state9", "logjp")}
    if old.get("ids") is not None:
        out["ids"] = np.concatenate([np.asarray(old["ids"]), np.asarray(new["ids"])])
    return out


def sort_rows(p):
    """the rows of a particle dict ordered by position bits, ties by the state's bits: two dicts hold the same set iff their sorted rows are equal bit for bit"""
    x = np.ascontiguousarray(p["xyz"], np.float32).view(np.uint32)
    s = np.ascontiguousarray(p["state9"], np.float32).view(np.uint32)
    order = np.lexsort(tuple(s[:, c] for c in range(8, -1, -1)) + (x[:, 2], x[:, 1], x[:, 0]))
    return {k: np.ascontiguousarray(np.asarray(v)[order]) for k, v in p.items() if v is not None}


def same_set(a, b):
    a, b = sort_rows(a), sort_rows(b)
    return a.keys() == b.keys() and all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in ((a[k], b[k]) for k in a))


def new_ids(old_n, n):
    return np.arange(old_n, old_n + n, dtype=np.int32)


def books_after(books, model, n):
    """books: {"n": [...], "bucketed": [...], "lost", "dropped", "bias"} - only the emitted model's n and bucketed move"""
    out = {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in books.items()}
    out["n"][model] += n
    out["bucketed"][model] += n
    return out


def books_balance(books):
    return sum(books["bucketed"]) + books["lost"] + books["dropped"] + books["bias"] == sum(books["n"])


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------------
def grid_by_node(keys, blocks, bits):
    """A dumped grid (Engine.dump_grid) as (flat node numbers (K,) ascending, values (K, 4) float32): every node of every dumped block"""
    keys, blocks = np.asarray(keys, np.int64), np.asarray(blocks, np.float32)
    n = 1 << bits
    cell = np.arange(64)
    nd = np.stack([keys[:, None, 0] * 4 + (cell >> 4)[None, :], keys[:, None, 1] * 4 + ((cell >> 2) & 3)[None, :], keys[:, None, 2] * 4 + (cell & 3)[None, :]], axis=2).reshape(-1, 3)
    val = blocks.transpose(0, 2, 1).reshape(-1, 4)
    inside = np.all((nd >= 0) & (nd < n), axis=1)
    flat = ((nd[:, 0] * n + nd[:, 1]) * n + nd[:, 2])[inside]
    order = np.argsort(flat)
    return flat[order], val[inside][order]


def reached_nodes(xyz, bits):
    """flat numbers of the in-domain nodes of the 27-node stencils of the particles xyz (world units), ascending and unique"""
    n = 1 << bits
    p = np.asarray(xyz, np.float32).astype(np.float64) * n
    base = lround_half_away(p) - 1
    out = []
    for i, j, k in itertools.product(range(3), repeat=3):
        node = base + np.array([i, j, k])
        inside = np.all((node >= 0) & (node < n), axis=1)
        out.append(((node[:, 0] * n + node[:, 1]) * n + node[:, 2])[inside])
    return np.unique(np.concatenate(out))


def new_particle_scene(bits, material_params, xyz, v0=(0.0, 0.0, 0.0), velocity=None, affine=None):
    """the new particles alone as a scene particle_init_model rasterises"""
    return {"bits": bits, "models": [{"xyz": np.asarray(xyz, np.float32), "v0": v0, "velocity": velocity, "affine": affine, "params": dict(material_params)}]}


# Roundings of a reached node beyond pim's per-term count: the new particles' contributions arrive in up to 8 global atomics (one per contributing
# workgroup: a node belongs to the 8^3 cubes of at most 2 x 2 x 2 particle blocks), each one addition, on top of the old value (one more term).
EXTRA_TERMS = 8 + 1


def expected_grid(old_flat, old_val, scene_new):
    """-> (flat (K,), want (K, 4) float64, bound (K, 4)) over the nodes the new particles give mass to: old value + the new particles' set-up P2G, and
    what float32 may deviate by: (terms + EXTRA_TERMS + the rasteriser's per-term roundings) u times the sum of magnitudes, the old value's included"""
    g = pim.setup_nodes(scene_new)
    n = 1 << scene_new["bits"]
    flat = (g["nodes"][:, 0] * n + g["nodes"][:, 1]) * n + g["nodes"][:, 2]
    at = np.searchsorted(old_flat, flat)
    hit = (at < old_flat.size) & (old_flat[np.minimum(at, old_flat.size - 1)] == flat) if old_flat.size else np.zeros(flat.size, bool)
    old = np.zeros((flat.size, 4))
    old[hit] = old_val[at[hit]].astype(np.float64)
    k = g["count"].astype(np.float64) + EXTRA_TERMS
    mag = g["mag"] + np.abs(old)
    bound = np.empty_like(mag)
    bound[:, 0] = pim.gamma(k + pim.R_MASS) * mag[:, 0]
    bound[:, 1:] = pim.gamma(k + pim.R_MOMENTUM)[:, None] * mag[:, 1:]
    return flat, old + g["val"], bound + k[:, None] * 2.0 ** -126


# ---- the emitter's layer rule, from its definition --------------------------------------------------------------------------------------------------
def nozzle_lattice(bits, shape, axis, **geom):
    """The reference's particle lattice (8 per cell, at node -+ 0.25 dx) cut by the nozzle's cross-section, in the plane through the nozzle's centre
    snapped to the lattice: (m, 3) float64.  box: lo <= x <= hi on the two transverse axes; disc: distance to the centre in the plane <= radius."""
    n = 1 << bits
    dx = 1.0 / n
    coords = (np.arange(2 * n) + 0.5) * (dx / 2)                   # node -+ 0.25 dx: the odd multiples of dx / 4 inside the domain
    centre = np.asarray(geom["center"] if shape == "disc" else (np.asarray(geom["lo"], np.float64) + np.asarray(geom["hi"], np.float64)) / 2, np.float64)
    plane = coords[np.argmin(np.abs(coords - centre[axis]))]
    t = [d for d in range(3) if d != axis]
    A, B = np.meshgrid(coords, coords, indexing="ij")
    if shape == "disc":
        keep = (A - centre[t[0]]) ** 2 + (B - centre[t[1]]) ** 2 <= float(geom["radius"]) ** 2
    else:
        keep = (A >= geom["lo"][t[0]]) & (A <= geom["hi"][t[0]]) & (B >= geom["lo"][t[1]]) & (B <= geom["hi"][t[1]])
    pts = np.empty((int(keep.sum()), 3))
    pts[:, axis] = plane
    pts[:, t[0]], pts[:, t[1]] = A[keep], B[keep]
    return pts


def layer_times(bits, speed, start, end):
    """t_k = start + k (dx / 2) / |v| for every k >= 0 with t_k < end"""
    period = (0.5 / (1 << bits)) / speed
    out, k = [], 0
    while start + k * period < end:
        out.append(start + k * period)
        k += 1
    return np.array(out)


def expected_emissions(bits, shape, velocity, start, end, times, **geom):
    """What an emitter hands out at the substep boundaries `times` (ascending): per boundary the list of (layer number, points (m, 3) float64) -
    every layer once, at the first boundary with t >= t_k, moved on by v (t - t_k)."""
    v = np.asarray(velocity, np.float64)
    axis = int(np.argmax(np.abs(v)))
    lattice = nozzle_lattice(bits, shape, axis, **geom)
    tk = layer_times(bits, float(np.abs(v[axis])), start, end)
    out, nxt = [], 0
    for t in times:
        now = []
        while nxt < tk.size and tk[nxt] <= t:
            now.append((nxt, lattice + v[None, :] * (t - tk[nxt])))
            nxt += 1
        out.append(now)
    return out

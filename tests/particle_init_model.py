"""The set-up grid of a scene whose models carry per-particle initial conditions, in float64: face_scenes.reference_setup_grid generalised from
one v0 per model to a velocity and an APIC matrix per particle (tests/test_particle_init_model_cpu.py, tests/test_particle_init_gpu.py).

A particle p of mass m gives node i of its 27-node quadratic B-spline stencil
    m w_ip                            (mass)
    m w_ip (v_p + C_p (x_i - x_p))    (momentum; x_i - x_p in world units)
and a node outside [0, n)^3 receives nothing.  A model dict carries "velocity" (n, 3) and "affine" (n, 3, 3) with affine[p, r, c] = C_rc, or a
velocity field ("omega" / "velocity_gradient" / "pivot", scenes.model_velocity_field), or neither (v0 for every particle, C = 0).

Beside the sums the model returns what a float32 bound needs: per node and channel the sum of the terms' magnitudes and the number of terms.

Test infrastructure only."""
import itertools

import numpy as np

from claymore_amd import scenes
from face_scenes import bspline64, lround_half_away

U = 2.0 ** -24                       # unit roundoff of float32

# Roundings of ONE term as rasterize_particles_kernel forms it (claymore_amd/csrc/mpm_particle_init.hpp; the count is written above the kernel too):
#   momentum: d = (float) node - p per axis (1, relative to d), the three products and two additions of C d, + v_p (1)          7
#             w0 w1 w2 (2), mass * w (1), times the bracket (1)                                                               4
#             the three axis weights, at most 5 each (the square, 0.75 - square relative to w >= 0.5, and below node 1 of a lower
#             face p - base = p + 1, which rounds p)                                                                         15
#   mass:     the axis weights (15), w0 w1 w2 (2), mass * w (1)
R_MOMENTUM = 7 + 4 + 15
R_MASS = 15 + 2 + 1
# the velocity-field form computes v_p = v0 + G (x_p - pivot) in the kernel: x_p - pivot (1), three products, three additions
R_FIELD = 7


def gamma(k):
    """k roundings compounded: k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def model_particles(scene, m):
    """(p in cells (n, 3), mass, v (n, 3), C (n, 3, 3), vabs (n, 3)) of one model dict, float64.  vabs: the magnitude the velocity's own rounding is
    relative to - |v_p| for an array or a v0, |v0| + sum_c |G_rc (x - pivot)_c| for a field evaluated in the kernel.  The arrays are taken as they are
    given: float32 arrays are what the engine sees, a float64 array stands for itself."""
    bits = scene["bits"]
    x = np.asarray(m["xyz"], dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    prm = m.get("params", {})
    mass = float(np.float32(prm.get("volume", scenes._vol(bits))) * np.float32(prm.get("rho", 1e3)))
    field = scenes.model_velocity_field(m)
    if field is not None:
        assert m.get("velocity") is None and m.get("affine") is None, "a field and a velocity / affine array exclude each other"
        a, A = field
        v = a[None, :] + x @ A.T
        C = np.broadcast_to(A, (n, 3, 3)).copy()
        rel = x - np.asarray(m.get("pivot", (0, 0, 0)), dtype=np.float64)[None, :]
        vabs = np.abs(np.asarray(m.get("v0", (0, 0, 0)), dtype=np.float64))[None, :] + np.abs(rel) @ np.abs(A).T
    else:
        v0 = np.asarray(m.get("v0", (0, 0, 0)), dtype=np.float64)
        v = np.broadcast_to(v0, (n, 3)).copy() if m.get("velocity") is None else np.asarray(m["velocity"]).astype(np.float64).reshape(n, 3)
        C = np.zeros((n, 3, 3)) if m.get("affine") is None else np.asarray(m["affine"]).astype(np.float64).reshape(n, 3, 3)
        vabs = np.abs(v)
    return x * (1 << bits), mass, v, C, vabs


def setup_terms(scene):
    """Every in-domain (particle, node) term of the scene's set-up P2G, in the order reference_setup_grid adds them (models, then stencil offsets, then
    particles): nodes (T, 3) int64, val (T, 4) = {m w, m w (v + C d)}, mag (T, 4) = {m w, m w (vabs + sum_c |C_rc d_c|)}, block (T, 3) the
    particle's block key; and the mass that falls outside the domain, by face."""
    n = 1 << scene["bits"]
    dx = 1.0 / n
    nodes, val, mag, blk = [], [], [], []
    outside = {"lo": 0.0, "hi": 0.0}
    for m in scene["models"]:
        p, mass, v, C, vabs = model_particles(scene, m)
        base = lround_half_away(p) - 1
        w = bspline64(p - base)
        key = np.where(base - 1 < 0, -((-(base - 1)) // 4), (base - 1) // 4)                   # (N - 2) / 4, truncating (particle_block_key)
        for i, j, k in itertools.product(range(3), repeat=3):
            node = base + np.array([i, j, k])
            wm = mass * w[:, 0, i] * w[:, 1, j] * w[:, 2, k]
            inside = np.all((node >= 0) & (node < n), axis=1)
            outside["lo"] += float(wm[np.any(node < 0, axis=1)].sum())
            outside["hi"] += float(wm[np.any(node >= n, axis=1) & ~np.any(node < 0, axis=1)].sum())
            d = (node - p) * dx                                                                 # x_i - x_p, world units
            Cd = np.einsum("nrc,nc->nr", C, d)
            Cd_abs = np.einsum("nrc,nc->nr", np.abs(C), np.abs(d))
            nodes.append(node[inside])
            val.append(np.concatenate([wm[inside, None], wm[inside, None] * (v + Cd)[inside]], axis=1))
            mag.append(np.concatenate([wm[inside, None], wm[inside, None] * (vabs + Cd_abs)[inside]], axis=1))
            blk.append(key[inside])
    return np.concatenate(nodes), np.concatenate(val), np.concatenate(mag), np.concatenate(blk), outside


def setup_nodes(scene):
    """The set-up grid node by node: {"nodes" (K, 3) sorted, "val" (K, 4) float64 sums, "mag" (K, 4) sums of magnitudes, "count" (K,) terms with a
    non-zero weight, "outside"}; only nodes that receive mass."""
    nodes, val, mag, _, outside = setup_terms(scene)
    n = 1 << scene["bits"]
    flat = (nodes[:, 0] * n + nodes[:, 1]) * n + nodes[:, 2]
    uniq, inv = np.unique(flat, return_inverse=True)
    V, M = np.zeros((uniq.size, 4)), np.zeros((uniq.size, 4))
    np.add.at(V, inv, val)                                                                      # (unbuffered: the terms are added in their order)
    np.add.at(M, inv, mag)
    cnt = np.bincount(inv, weights=(val[:, 0] != 0).astype(np.float64), minlength=uniq.size).astype(np.int64)
    keep = V[:, 0] > 0
    un = np.stack([uniq // (n * n), (uniq // n) % n, uniq % n], axis=1)
    return {"nodes": un[keep], "val": V[keep], "mag": M[keep], "count": cnt[keep], "outside": outside}


def setup_grid(scene):
    """reference_setup_grid's return for a scene with per-particle velocities: ({node (3-tuple): [m, mv]}, outside)."""
    g = setup_nodes(scene)
    return {tuple(int(c) for c in nd): v for nd, v in zip(g["nodes"], g["val"])}, g["outside"]


def node_bounds(g, extra_momentum=0, extra_terms=0):
    """(K, 4): what the float32 grid may deviate from g["val"] by - (n + r) roundings compounded, times the sum of the terms' magnitudes: a sum of n
    terms in any order (LDS atomics, then one global atomic per contributing block; extra_terms: further partial sums, a group's ranks) carries at
    most n - 1 roundings per term, a term r.  A term below float32's normal range may be flushed: 2^-126 each."""
    k = g["count"].astype(np.float64) + extra_terms
    out = np.empty_like(g["mag"])
    out[:, 0] = gamma(k + R_MASS) * g["mag"][:, 0]
    out[:, 1:] = gamma(k + R_MOMENTUM + extra_momentum)[:, None] * g["mag"][:, 1:]
    return out + k[:, None] * 2.0 ** -126


def linear_field_bounds(g, nb, x, bits, a, A):
    """What retrieve_velocity may deviate from a linear field v = a + A x by at the particles x (n, 3), when the grid g (setup_nodes) holds that
    field's set-up P2G within nb (node_bounds): (bound on |v_p - (a + A x_p)| (n,), bound on |C_p - A| (n,)), per component.
    Node velocity v_i = p_i / m_i in float32: |v_i - want_i| <= e_i = (nb_p + |want_i| nb_m) / (m_i - nb_m) + u |want_i|.
    v_p = sum_i w_ip v_i over 27 nodes: the weights as above (3 x 5 + 2 roundings), one product, 27 additions -> gamma(45) sum_i w |v_i| <= gamma(45) max_i |v_i|,
    plus sum_i w e_i <= max_i e_i.  C_p = (4 / dx^2) sum_i w_ip v_i (x_i - x_p)^T with |x_i - x_p| <= 1.5 dx: one more product and the rounding of
    x_i - x_p -> (6 / dx) (max_i e_i + gamma(47) max_i |v_i|), then the two scalings (2 more roundings, folded into 49)."""
    n = 1 << bits
    want = a[None, :] + (g["nodes"] / float(n)) @ A.T
    wabs = np.abs(want).max(axis=1)
    m = g["val"][:, 0]
    e = (nb[:, 1:].max(axis=1) + wabs * nb[:, 0]) / (m - nb[:, 0]) + U * wabs
    flat = (g["nodes"][:, 0] * n + g["nodes"][:, 1]) * n + g["nodes"][:, 2]
    order = np.argsort(flat)
    p = np.asarray(x, dtype=np.float32).astype(np.float64) * n
    base = lround_half_away(p) - 1
    emax, vmax = np.zeros(p.shape[0]), np.zeros(p.shape[0])
    for i, j, k in itertools.product(range(3), repeat=3):
        node = base + np.array([i, j, k])
        f = (node[:, 0] * n + node[:, 1]) * n + node[:, 2]
        at = np.clip(np.searchsorted(flat[order], f), 0, flat.size - 1)
        hit = flat[order][at] == f                                   # (a stencil node without mass holds v_i = 0: no error)
        emax = np.maximum(emax, np.where(hit, e[order][at], 0.0))
        vmax = np.maximum(vmax, np.where(hit, wabs[order][at], 0.0))
    return emax + gamma(45) * vmax, 6.0 * n * (emax + gamma(49) * vmax)


def dumped_nodes(keys, blocks, bits):
    """A dumped grid (Engine.dump_grid) as (nodes (K, 3) sorted like setup_nodes', val (K, 4) float64): the nodes whose mass is not zero."""
    keys, blocks = np.asarray(keys, dtype=np.int64), np.asarray(blocks)
    n = 1 << bits
    b, cell = np.nonzero(blocks[:, 0, :] != 0)
    nd = np.stack([keys[b, 0] * 4 + (cell >> 4), keys[b, 1] * 4 + ((cell >> 2) & 3), keys[b, 2] * 4 + (cell & 3)], axis=1)
    order = np.argsort((nd[:, 0] * n + nd[:, 1]) * n + nd[:, 2])
    return nd[order], blocks[b, :, cell].astype(np.float64)[order]

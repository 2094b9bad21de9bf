"""NumPy model of the mesh-sampled model (include/claymore_amd.h "mpm_mesh_fill", claymore_amd/csrc/mpm_mesh_fill.hpp): the candidate lattice,
the clip rule, the order of the output, and inside(p) <=> sdis(p) < -margin with sdis from collision_mesh_model.Mesh's field rule.  Every
candidate is evaluated on its own: no tile is culled and nothing is taken from a tile's centre.  The one liberty is in the nearest-triangle
search, which skips triangles that provably cannot win (Mesh.nearest below); the rule and the four words are collision_mesh_model's.  `sample` also reports the
candidates whose sign collision_mesh_model.SIGN_MARGIN cannot vouch for: the tests place their meshes so that there are none."""
import numpy as np

import collision_mesh_model as mm

F32 = np.float32


def clip_range(bits, verts, box=None):
    """The nodes lo <= (i, j, k) < hi that are looked at: the box (default the domain) cut to floor(mn N) <= i < floor(mx N) + 2 per axis."""
    n = 1 << bits
    lo, hi = (np.zeros(3, dtype=np.int64), np.full(3, n, dtype=np.int64)) if box is None else (np.array(b, dtype=np.int64) for b in box)
    assert ((lo >= 0) & (lo <= n) & (hi >= 0) & (hi <= n)).all()
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    a, b = np.floor(v.min(axis=0) * n), np.floor(v.max(axis=0) * n) + 2
    lo = np.maximum(lo, np.clip(a, 0, n).astype(np.int64))
    hi = np.minimum(hi, np.clip(b, 0, n).astype(np.int64))
    return lo, np.maximum(hi, lo)


def candidates(bits, lo, hi):
    """The candidates of the nodes lo <= (i, j, k) < hi as (m, 3) float32 in the order of the contract: tiles of 4^3 nodes aligned to the
    domain, ascending with x slowest; nodes of a tile by (x 4 + y) 4 + z; candidates with a slowest, c fastest, -1 before +1."""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    if (hi <= lo).any():
        return np.zeros((0, 3), dtype=np.float32)
    grid = lambda axes: np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    tiles = grid([np.arange(lo[d] >> 2, (hi[d] + 3) >> 2) for d in range(3)])
    nodes = (4 * tiles[:, None, :] + grid([np.arange(4)] * 3)[None, :, :]).reshape(-1, 3)
    nodes = nodes[((nodes >= lo) & (nodes < hi)).all(axis=1)]
    signs = grid([np.array([-1, 1])] * 3).astype(np.float32)
    dx = F32(1.0 / (1 << bits))
    p = (nodes[:, None, :].astype(np.float32) + signs[None, :, :] * F32(0.25)) * dx
    assert p.dtype == np.float32
    return np.ascontiguousarray(p.reshape(-1, 3))


class Mesh(mm.Mesh):
    """collision_mesh_model.Mesh with a nearest-triangle search that leaves out the triangles that cannot win."""

    def nearest(self, p, chunk=512):
        """Mesh.nearest - the lowest index among the smallest float32 q - per chunk of points (they come tile by tile, so a chunk is compact).
        With g_t a triangle's centroid and R_t the largest distance of its corners from g_t, dist(p, t) lies in [|p - g_t| - R_t, |p - g_t|].
        A triangle whose lower bound exceeds the smallest upper bound by more than 2^-12 (coordinates are of order 1: the walk's float32
        error is a thousand times smaller) has a larger float32 q than the winner; it is dropped only if that holds for every point of the
        chunk.  The kept ones stay in index order, so argmin's first occurrence is still the lowest index."""
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        P = self.verts.astype(np.float64)[self.tris]
        g = P.mean(axis=1)
        R = np.linalg.norm(P - g[:, None, :], axis=2).max(axis=1)
        T = np.empty(len(p), dtype=np.int64)
        for s in range(0, len(p), chunk):
            x = p[s:s + chunk]
            d = np.linalg.norm(x.astype(np.float64)[:, None, :] - g[None, :, :], axis=2)
            keep = np.flatnonzero(((d - R[None, :]) <= d.min(axis=1)[:, None] + 2.0 ** -12).any(axis=0))
            q, _, _ = mm.walk(x[:, None, :], self.a[None, keep], self.ab[None, keep], self.ac[None, keep])
            assert not np.isnan(q).any()
            T[s:s + chunk] = keep[np.argmin(q, axis=1)]
        return T


def sample(bits, verts, tris, margin=0.0, box=None):
    """The sampler per point: dict(points (n, 3) float32 in the contract's order, candidates, inside (bool per candidate), undecided (indices
    of the candidates under the radial rule whose |(p - c) . m| / |m| is below SIGN_MARGIN), res (the field's result at every candidate))."""
    assert mm.validate(verts, tris)[0] == "ok"
    mesh = Mesh(verts, tris)
    lo, hi = clip_range(bits, mesh.verts, box)
    p = candidates(bits, lo, hi)
    if not len(p):
        return dict(points=p, candidates=p, inside=np.zeros(0, dtype=bool), undecided=np.zeros(0, dtype=np.int64), res=None)
    res = mesh.field(p)
    inside = res["out"][:, 0] < -F32(margin)
    undecided = np.flatnonzero(~res["plane"] & (res["margin"] < mm.SIGN_MARGIN))
    return dict(points=np.ascontiguousarray(p[inside]), candidates=p, inside=inside, undecided=undecided, res=res)


def l_prism(lo=(0.27, 0.31, 0.29), size=(0.36, 0.3, 0.22), notch=(0.17, 0.14)):
    """A non-convex closed mesh: the box lo .. lo + size with the corner x > lo + notch[0], y > lo + notch[1] cut away, extruded along z.
    8 triangles on the two L-shaped caps (a fan about the outer corner at lo) and 12 on the six sides, counter-clockwise seen from outside."""
    x0, y0, z0 = lo
    x1, y1, z1 = x0 + size[0], y0 + size[1], z0 + size[2]
    xm, ym = x0 + notch[0], y0 + notch[1]
    ring = [(x0, y0), (x1, y0), (x1, ym), (xm, ym), (xm, y1), (x0, y1)]  # counter-clockwise seen from +z
    v = np.array([(x, y, z) for z in (z0, z1) for x, y in ring], dtype=np.float32)
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 5)]  # a fan about ring[0]: convex from there (every diagonal stays inside the L)
    f = [(a, c, b) for a, b, c in cap] + [(6 + a, 6 + b, 6 + c) for a, b, c in cap]
    for i in range(6):
        j = (i + 1) % 6
        f += [(i, j, 6 + j), (i, 6 + j, 6 + i)]
    return v, np.array(f, dtype=np.int32)

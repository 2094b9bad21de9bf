"""NumPy model of the grid isosurface (mpm_grid_isosurface, claymore_amd/csrc/mpm_grid_isosurface.hpp): marching
tetrahedra over the mass channel of grid_field_model.GridField's dense array, padded with one node of zeros (the nodes -1 and N).

  cells      (i, j, k) in [-1, N - 1], corners (i, j, k) + {0, 1}^3; a node is inside iff f > iso_mass (a NaN is outside)
  tetrahedra the six Kuhn tetrahedra, one per permutation (a, b, c) of the axes: c0 = 0, c1 = e_a, c2 = e_a + e_b, c3 = (1, 1, 1)
  vertices   on an edge (A, B), A <= B componentwise, with exactly one end inside: t = (iso - f(A)) / (f(B) - f(A)), two float32 subtractions
             and one float32 division; node units A_d + t where B_d - A_d = 1 (one float32 add), A_d elsewhere; world = node units * dx
  triangles  one or three corners inside: one triangle; two: the quad P(I0,O0) P(I0,O1) P(I1,O1) P(I1,O0) split along P(I0,O0) - P(I1,O1).
             The winding comes from the corner coordinates alone (TABLES below): the normal points from the inside to the outside corners
  velocity   float64: ref = (p(A) + t (p(B) - p(A))) / iso with the float32 t, S = (|p(A)| + |p(B)|) / iso

Nothing here is typed in: the 16-case table is derived below from the rule, for each of the six tetrahedra."""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))      # (0,1,2) (0,2,1) (1,0,2) (1,2,0) (2,0,1) (2,1,0)


def tet_corners(perm):
    """(4, 3) ints: the corners c0 .. c3 of the Kuhn tetrahedron of the permutation."""
    a, b, _ = perm
    c = np.zeros((4, 3), dtype=np.int64)
    c[1, a] = 1
    c[2, a] = c[2, b] = 1
    c[3] = 1
    return c


def _det(u, v, w):
    return int(round(np.linalg.det(np.array([u, v, w], dtype=np.float64))))


def case_triangles(corners, mask):
    """The triangles of one tetrahedron for the 4-bit case `mask` (bit i: corner i inside): a list of triples of edges (i, j), i < j."""
    ins = [i for i in range(4) if mask >> i & 1]
    outs = [i for i in range(4) if not mask >> i & 1]
    e = lambda i, j: (min(i, j), max(i, j))                                      # noqa: E731
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        tri = [e(ins[0], o) for o in outs]
        keep = _det(*[corners[o] - corners[ins[0]] for o in outs]) > 0           # the normal runs along O - I
        return [tri if keep else [tri[0], tri[2], tri[1]]]
    if len(ins) == 3:
        tri = [e(i, outs[0]) for i in ins]
        keep = _det(*[corners[i] - corners[outs[0]] for i in ins]) < 0           # ... against I - O
        return [tri if keep else [tri[0], tri[2], tri[1]]]
    (i0, i1), (o0, o1) = ins, outs
    q = [e(i0, o0), e(i0, o1), e(i1, o1), e(i1, o0)]
    mid = [(corners[i] + corners[j]) / 2.0 for i, j in q]
    out_dir = (corners[o0] + corners[o1] - corners[i0] - corners[i1]) / 2.0
    s = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), out_dir))
    assert s != 0.0
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]] if s > 0 else [[q[0], q[2], q[1]], [q[0], q[3], q[2]]]


TABLES = [[case_triangles(tet_corners(p), m) for m in range(16)] for p in PERMS]


def perm_is_odd(perm):
    return _det(*np.eye(3, dtype=np.int64)[list(perm)]) < 0


def _lex_less(a, b):
    """Row-wise lexicographic a < b of two (n, k) unsigned arrays."""
    less = np.zeros(a.shape[0], dtype=bool)
    decided = np.zeros(a.shape[0], dtype=bool)
    for c in range(a.shape[1]):
        lt, gt = a[:, c] < b[:, c], a[:, c] > b[:, c]
        less |= ~decided & lt
        decided |= lt | gt
    return less


def canonical_order(tris):
    """tris (nt, 3, 3) float32 -> (order (nt,), rot (nt,)): the triangle at place q of the canonical form is tris[order[q]] with its vertices
    rotated left by rot[order[q]].  Each triangle is rotated cyclically so that its smallest vertex - by the bits of (x, y, z) as unsigned
    words; among equal ones the rotation with the smallest nine words - comes first, then the triangles are sorted by their nine words."""
    bits = np.ascontiguousarray(tris, dtype=np.float32).view(np.uint32).reshape(-1, 9)
    best, rot = bits.copy(), np.zeros(bits.shape[0], dtype=np.int64)
    for r in (1, 2):
        cand = np.roll(bits, -3 * r, axis=1)
        less = _lex_less(cand, best)
        best[less], rot[less] = cand[less], r
    order = np.lexsort(best.T[::-1])
    return order, rot


def canonical(tris):
    """(nt, 9) uint32: the canonical form of a triangle soup (see canonical_order)."""
    bits = np.ascontiguousarray(tris, dtype=np.float32).view(np.uint32).reshape(-1, 3, 3)
    order, rot = canonical_order(tris)
    idx = (np.arange(3)[None, :] + rot[order][:, None]) % 3
    return bits[order][np.arange(len(order))[:, None], idx].reshape(-1, 9)


def apply_order(values, order, rot):
    """Per-vertex values (nt, 3, ...) rearranged as canonical() rearranges the positions."""
    idx = (np.arange(3)[None, :] + rot[order][:, None]) % 3
    return values[order][np.arange(len(order))[:, None], idx]


class Surface:
    """tris (nt, 3, 3) float32 world positions; cell (nt, 3) the cell of each triangle; A, B (nt, 3, 3) the end nodes of each vertex's edge;
    t (nt, 3) float32; with velocity: ref, S (nt, 3, 3) float64."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def count(self):
        return self.tris.shape[0]

    def canonical(self):
        return canonical(self.tris)


def isosurface(dense, iso_mass, lo=None, hi=None, velocity=False, dx=None):
    """dense: GridField.dense - (4, N, N, N) uint32 bit patterns (or float32) - or a plain (N0, N1, N2) float32 mass field."""
    dense = np.asarray(dense)
    if dense.dtype == np.uint32:
        dense = dense.view(np.float32)
    if dense.ndim == 3:
        dense = dense[None]
    assert dense.dtype == np.float32 and dense.ndim == 4
    dims = np.array(dense.shape[1:])
    iso = np.float32(iso_mass)
    assert np.isfinite(iso) and iso > 0
    dx = np.float32(1.0 / dims[0] if dx is None else dx)
    F = np.zeros((dense.shape[0],) + tuple(dims + 2), dtype=np.float32)          # node n at index n + 1
    F[:, 1:-1, 1:-1, 1:-1] = dense
    with np.errstate(invalid="ignore"):
        inside = F[0] > iso
    n_in = np.zeros(tuple(dims + 1), dtype=np.int64)                             # cell c at index c + 1
    for d in itertools.product((0, 1), repeat=3):
        n_in += inside[d[0]:d[0] + dims[0] + 1, d[1]:d[1] + dims[1] + 1, d[2]:d[2] + dims[2] + 1]
    cells = np.argwhere((n_in > 0) & (n_in < 8)) - 1                             # low corner nodes of the mixed cells
    if (lo is None) != (hi is None):
        raise ValueError("one of lo / hi is None")
    if lo is not None:
        cells = cells[((cells >= np.asarray(lo)) & (cells < np.asarray(hi))).all(axis=1)]
    out = {k: [] for k in ("cell", "A", "B")}
    for perm, table in zip(PERMS, TABLES):
        corners = tet_corners(perm)
        node = cells[:, None, :] + corners[None]                                 # (nc, 4, 3)
        ins = inside[node[..., 0] + 1, node[..., 1] + 1, node[..., 2] + 1]
        mask = (ins * (1 << np.arange(4))).sum(axis=1)
        for m in range(1, 15):
            sel = mask == m
            if not sel.any():
                continue
            for tri in table[m]:
                out["cell"].append(cells[sel])
                out["A"].append(np.stack([node[sel, i] for i, _ in tri], axis=1))
                out["B"].append(np.stack([node[sel, j] for _, j in tri], axis=1))
    if not out["cell"]:
        z = np.zeros((0, 3, 3))
        return Surface(tris=z.astype(np.float32), cell=np.zeros((0, 3), np.int64), A=z.astype(np.int64), B=z.astype(np.int64), t=np.zeros((0, 3), np.float32),
                       ref=z.copy(), S=z.copy())
    cell, A, B = (np.concatenate(out[k]) for k in ("cell", "A", "B"))
    at = lambda c, n: F[c][n[..., 0] + 1, n[..., 1] + 1, n[..., 2] + 1]          # noqa: E731
    fA, fB = at(0, A), at(0, B)
    with np.errstate(all="ignore"):
        t = (iso - fA) / (fB - fA)                                               # float32 throughout
        node_units = A.astype(np.float32) + np.where(B - A == 1, t[..., None], np.float32(0))
        tris = node_units * dx
    s = Surface(tris=tris.astype(np.float32), cell=cell, A=A, B=B, t=t, ref=None, S=None)
    if velocity:
        pA = np.stack([at(c, A) for c in (1, 2, 3)], axis=-1).astype(np.float64)
        pB = np.stack([at(c, B) for c in (1, 2, 3)], axis=-1).astype(np.float64)
        with np.errstate(all="ignore"):
            s.ref = (pA + t.astype(np.float64)[..., None] * (pB - pA)) / float(iso)
            s.S = (np.abs(pA) + np.abs(pB)) / float(iso)
    return s


# ---- what the tests ask of a surface ----------------------------------------------------------------------------------------------------
def nondegenerate(tris):
    b = np.ascontiguousarray(tris, dtype=np.float32).view(np.uint32)
    same = lambda i, j: (b[:, i] == b[:, j]).all(axis=1)                         # noqa: E731
    return ~(same(0, 1) | same(1, 2) | same(0, 2))


def open_edges(tris):
    """The number of directed edges (welded on the position bits) of the non-degenerate triangles that are not matched by their reverse the
    same number of times: 0 for a closed surface."""
    tris = np.ascontiguousarray(tris, dtype=np.float32)[nondegenerate(tris)]
    if not len(tris):
        return 0
    _, inv = np.unique(tris.view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    f = inv.reshape(-1, 3).astype(np.int64)
    nv = int(f.max()) + 1
    fwd = np.concatenate([f[:, i] * nv + f[:, (i + 1) % 3] for i in range(3)])
    rev = np.concatenate([f[:, (i + 1) % 3] * nv + f[:, i] for i in range(3)])
    codes, cf = np.unique(fwd, return_counts=True)
    rcodes, cr = np.unique(rev, return_counts=True)
    if not np.array_equal(codes, rcodes):
        return int(len(np.setxor1d(codes, rcodes))) + int((cf[np.isin(codes, rcodes)] != cr[np.isin(rcodes, codes)]).sum())
    return int((cf != cr).sum())


def signed_volume(tris):
    t = np.asarray(tris, dtype=np.float64)
    return float(np.einsum("ni,ni->n", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def weld(tris, vel=None):
    """The welding of Engine.isosurface, restated: vertices unique on their position bits, triangles with two equal indices dropped."""
    pts = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 3)
    if not len(pts):
        return pts.copy(), np.zeros((0, 3), np.int32), (None if vel is None else np.zeros((0, 3), np.float32))
    _, first, inv = np.unique(pts.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    f = inv.reshape(-1, 3).astype(np.int32)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    return pts[first], f, (None if vel is None else np.asarray(vel, dtype=np.float32).reshape(-1, 3)[first])

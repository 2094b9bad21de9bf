"""NumPy model of the mesh-built collision field (include/claymore_amd.h, claymore_amd/csrc/mpm_collision_mesh.hpp): the per-triangle
records, the closest point of the Voronoi-region walk, q, the nearest triangle T, the plane / radial rule, |sdis| and g in float32 with the
kernel's operation order (every NumPy float32 operation is one IEEE operation, so nothing is contracted); the pseudonormals and the sign
in float64.  An independent float64 generalized winding number (van Oosterom & Strackee's solid angles / 4 pi) cross-checks the sign, and
`validate` restates the install's checks.  The model is evaluated on chosen node sets, never on a whole big grid."""
import numpy as np

F32 = np.float32
CORNER_A, CORNER_B, CORNER_C, EDGE_AB, EDGE_AC, EDGE_BC, FACE = range(7)
PLANE_Q = F32(2.0 ** -40)
SIGN_MARGIN = 2.0 ** -16  # the tests' condition on |(p - c) . m| / |m| at every radial-rule node they compare
MAX_TRIANGLES = MAX_VERTICES = 1 << 22


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def walk(p, a, ab, ac):
    """Closest point of the triangles (a, ab, ac) to the points p (float32 arrays that broadcast, last axis 3): q, c, feature."""
    assert p.dtype == a.dtype == ab.dtype == ac.dtype == np.float32
    with np.errstate(all="ignore"):
        ap = p - a
        bp = ap - ab
        cp = ap - ac
        d1, d2 = dot32(ab, ap), dot32(ac, ap)
        d3, d4 = dot32(ab, bp), dot32(ac, bp)
        d5, d6 = dot32(ab, cp), dot32(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        feature = np.select(conds, [CORNER_A, CORNER_B, EDGE_AB, CORNER_C, EDGE_AC, EDGE_BC], default=FACE)
        nv = np.select(conds, [zero, one, d1, zero, zero, zero], default=vb)
        nw = np.select(conds, [zero, zero, zero, one, d2, e43], default=vc)
        den = np.select(conds, [one, one, d1 - d3, one, d2 - d6, e43 + e56], default=(va + vb) + vc)
        assert nv.dtype == nw.dtype == den.dtype == np.float32
        w = nw / den
        v = np.where(feature == EDGE_BC, one - w, nv / den)
        c = (a + ab * v[..., None]) + ac * w[..., None]
        diff = p - c
        q = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    assert q.dtype == c.dtype == np.float32
    return q, c, feature


def validate(verts, tris):
    """The install's verdict as a tag - "ok", "few", "index", "nonfinite", "degenerate", "open", "volume" - with (closed, volume)."""
    v = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if len(t) < 4 or len(t) > MAX_TRIANGLES or len(v) > MAX_VERTICES:
        return "few", False, 0.0
    if (t < 0).any() or (t >= len(v)).any():
        return "index", False, 0.0
    if not np.isfinite(v).all():
        return "nonfinite", False, 0.0
    m = Mesh(v, t)
    with np.errstate(all="ignore"):
        nn = dot32(m.n, m.n)
    tag = "ok"
    if (~(nn > 0) | ~np.isfinite(nn)).any():
        tag = "degenerate"
    elif not m.closed:
        tag = "open"
    elif not m.volume > 0:
        tag = "volume"
    return tag, m.closed, m.volume


class Mesh:
    """The records of a mesh whose indices and vertices are usable (closed or not: a free edge's pseudonormal is its own triangle's n^)."""

    def __init__(self, verts, tris):
        self.verts = v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        self.tris = t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        self.a = v[t[:, 0]]
        self.ab = v[t[:, 1]] - self.a
        self.ac = v[t[:, 2]] - self.a
        ab, ac = self.ab, self.ac
        self.n = n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
        with np.errstate(all="ignore"):
            self.nh = n / np.sqrt(dot32(n, n))[:, None]
        assert self.nh.dtype == np.float32
        # float64: unit normals, volume, adjacency, pseudonormals
        P = v.astype(np.float64)[t]                                                               # (nt, 3 corners, 3)
        N = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        ln = np.linalg.norm(N, axis=1)
        self.nh64 = nh64 = np.where(ln[:, None] > 0, N / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
        self.volume = float(np.einsum("ni,ni->n", P[:, 0], np.cross(P[:, 1], P[:, 2])).sum() / 6.0)
        directed = {}
        for ti, (i, j, k) in enumerate(t.tolist()):
            for e in ((i, j), (j, k), (k, i)):
                directed.setdefault(e, []).append(ti)
        self.closed = all(len(o) == 1 and len(directed.get((e[1], e[0]), [])) == 1 for e, o in directed.items())
        vsum = np.zeros((len(v), 3))
        for k in range(3):
            x, y = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
            angle = np.arctan2(np.linalg.norm(np.cross(x, y), axis=1), np.einsum("ni,ni->n", x, y))
            np.add.at(vsum, t[:, k], angle[:, None] * nh64)
        self.pseudo = np.zeros((len(t), 6, 3))                                                    # [triangle, feature]
        for k in range(3):
            self.pseudo[:, k] = vsum[t[:, k]]
        for f, (u, w) in ((EDGE_AB, (0, 1)), (EDGE_AC, (2, 0)), (EDGE_BC, (1, 2))):
            for ti in range(len(t)):
                o = directed.get((int(t[ti, w]), int(t[ti, u])))
                self.pseudo[ti, f] = nh64[ti] + (nh64[o[0]] if o else 0.0)

    def nearest(self, p, chunk=2048):
        """T and q_T of the points p (n, 3) float32: the lowest index among the smallest q."""
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        T = np.empty(len(p), dtype=np.int64)
        for s in range(0, len(p), chunk):
            q, _, _ = walk(p[s:s + chunk, None, :], self.a[None], self.ab[None], self.ac[None])
            assert not np.isnan(q).any()
            T[s:s + chunk] = np.argmin(q, axis=1)                                                 # (the first occurrence of the minimum)
        return T

    def field(self, p, inside_out=False):
        """The four words at the points p (n, 3) float32 and what led to them: dict(out (n, 4) float32, T, feature, q, plane (bool), margin
        (|(p - c) . m| / |m| in float64; inf at plane-rule points), sign (float64 pseudonormal sign, +1 / -1; plane rule: that of sdis))."""
        p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 3)
        T = self.nearest(p)
        a, nh = self.a[T], self.nh[T]
        q, c, feature = walk(p, a, self.ab[T], self.ac[T])
        plane = (feature == FACE) | (q < PLANE_Q)
        out = np.empty((len(p), 4), dtype=np.float32)
        with np.errstate(all="ignore"):
            diff = p - c
            m = self.pseudo[T, np.minimum(feature, 5)]
            dotm = np.einsum("ni,ni->n", diff.astype(np.float64), m)
            s = np.where(dotm >= 0, F32(1), F32(-1)).astype(np.float32)
            d = np.sqrt(q)
            out[:, 0] = np.where(plane, dot32(p - a, nh), s * d)
            out[:, 1:] = np.where(plane[:, None], nh, (s[:, None] * diff) / d[:, None])
            margin = np.where(plane, np.inf, np.abs(dotm) / np.linalg.norm(m, axis=1))
        sign = np.where(plane, np.where(out[:, 0] >= 0, 1.0, -1.0), s.astype(np.float64))
        if inside_out:
            out = -out
        return dict(out=out, T=T, feature=feature, q=q, plane=plane, margin=margin, sign=sign)

    def winding(self, p, chunk=4096):
        """Generalized winding number of the points p in float64: 1 inside a closed outward-wound mesh, 0 outside."""
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        P = self.verts.astype(np.float64)[self.tris]
        w = np.empty(len(p))
        for s in range(0, len(p), chunk):
            A, B, Cc = (P[None, :, k] - p[s:s + chunk, None, :] for k in range(3))
            la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, Cc))
            num = np.einsum("pti,pti->pt", A, np.cross(B, Cc))
            den = la * lb * lc + np.einsum("pti,pti->pt", A, B) * lc + np.einsum("pti,pti->pt", B, Cc) * la + np.einsum("pti,pti->pt", Cc, A) * lb
            w[s:s + chunk] = (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)
        return w


def check_signs(mesh, res, p):
    """The tests' precondition on a compared node set: every radial-rule node is at least SIGN_MARGIN off its pseudonormal's zero plane, and
    the pseudonormal sign is the winding number's wherever the node is off the surface."""
    radial = ~res["plane"]
    assert (res["margin"][radial] >= SIGN_MARGIN).all(), float(res["margin"][radial].min())
    off = res["q"] >= PLANE_Q
    w = mesh.winding(p[off])
    assert (np.abs(w - np.round(w)) < 1e-9).all()
    assert np.array_equal(np.where(w > 0.5, -1.0, 1.0), res["sign"][off]), "pseudonormal sign != winding-number sign"


def grid_nodes(bits, lo=(0, 0, 0), shape=None):
    """The positions ((float) i dx ...) of the nodes lo + [0, shape) as (n, 3) float32, x slowest."""
    n = 1 << bits
    shape = [n - v for v in lo] if shape is None else shape
    g = np.stack(np.meshgrid(*[np.arange(lo[d], lo[d] + shape[d]) for d in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    return (g.astype(np.float32) * F32(1.0 / n)).astype(np.float32)


def write_obj(path, verts, tris):
    with open(path, "w") as f:
        for x in np.asarray(verts, dtype=np.float32).reshape(-1, 3):
            f.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in x))
        for t in np.asarray(tris).reshape(-1, 3):
            f.write("f %d %d %d\n" % tuple(int(i) + 1 for i in t))


# ---- the tests' meshes -------------------------------------------------------------------------------------------------------------------
def octahedron(centre=(0.47, 0.53, 0.51), radius=0.31):
    c = np.asarray(centre, dtype=np.float64)
    v = np.array([c + radius * np.array(d) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))], dtype=np.float32)
    f = np.array([(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)], dtype=np.int32)
    return v, f

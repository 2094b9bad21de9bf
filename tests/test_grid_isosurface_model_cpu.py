"""The model of the surface readout (tests/grid_isosurface_model.py) against what it has to be before it may judge the kernel: a closed,
outward-wound surface of the right volume on a smooth field, closed and on its edges on a rough one, independent of who asks for an edge,
clipped by cells; the welding of Engine.isosurface and the OBJ writer of the gmpm driver (claymore_amd/host/particle_io.hpp); the ABI
surface of mpm_grid_isosurface.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import grid_field_model as gfm
import grid_isosurface_model as im
from claymore_amd import _ffi
from claymore_amd.engine import weld_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
BITS = 6
N = 1 << BITS


@pytest.fixture(scope="module")
def hashed():
    """Blocks with values 2^[-20, 20): a cluster with holes, blocks at the domain's lower corner and upper faces."""
    rng = np.random.default_rng(5)
    keys = np.unique(np.concatenate([rng.integers(3, 8, (60, 3)), [[0, 0, 0], [0, 1, 0], [15, 15, 15], [15, 14, 15], [15, 3, 0]]]), axis=0)
    field = gfm.GridField(keys, gfm.hashed_blocks(len(keys), 23), BITS)
    return field, im.isosurface(field.dense, 1.0, velocity=True)


# ---- a smooth field -----------------------------------------------------------------------------------------------------------------------
def test_ball_is_closed_and_has_its_volume():
    n, centre = 40, np.array([19.3, 20.1, 18.7])
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1)
    f = np.maximum(0.0, 12.0 - np.linalg.norm(g - centre, axis=-1)).astype(np.float32)
    s = im.isosurface(f, 2.0, dx=1.0)
    vol, want = im.signed_volume(s.tris), 4.0 / 3.0 * np.pi * 10.0 ** 3
    print(f"ball: {s.count} triangles, {int((~im.nondegenerate(s.tris)).sum())} degenerate, volume {vol:.1f} of {want:.1f} ({100 * (vol / want - 1):+.2f} %)")
    assert s.count > 5000 and im.open_edges(s.tris) == 0
    assert vol > 0 and abs(vol - want) <= 0.01 * want                             # positive: the normals point out of the ball
    r = np.linalg.norm(s.tris.astype(np.float64) - centre, axis=-1)
    assert np.abs(r - 10.0).max() < 0.2                                           # linear interpolation of a distance field
    # every non-degenerate triangle's normal points away from the centre
    t = s.tris[im.nondegenerate(s.tris)].astype(np.float64)
    normal = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    assert (np.einsum("ni,ni->n", normal, t.mean(axis=1) - centre) > 0).all()


# ---- a rough field ------------------------------------------------------------------------------------------------------------------------
def test_hashed_field_is_closed_and_its_vertices_lie_on_their_edges(hashed):
    field, s = hashed
    deg = ~im.nondegenerate(s.tris)
    print(f"hashed: {s.count} triangles, {int(deg.sum())} degenerate, t in [{s.t.min()!r}, {s.t.max()!r}]")
    assert s.count > 20000 and im.open_edges(s.tris) == 0
    assert (s.t >= 0).all() and (s.t <= 1).all()
    d = s.B - s.A
    assert ((d >= 0) & (d <= 1)).all() and (d.sum(axis=-1) >= 1).all()            # A <= B componentwise, an edge of the cell
    assert (s.cell >= -1).all() and (s.cell <= N - 1).all() and (s.cell == -1).any() and (s.cell == N - 1).any()
    units = s.tris.astype(np.float64) * N                                         # (exact: dx is a power of two)
    off = units - s.A
    assert (off[d == 0] == 0).all()                                               # on the other axes: the node's own coordinate
    along = np.where(d == 1, off, np.nan)
    assert (np.nanmax(along, axis=-1) - np.nanmin(along, axis=-1) <= N * 2.0 ** -23).all()   # one t for the axes it moves along (each A_d + t rounds on its own)
    assert (np.abs(off[d == 1] - np.broadcast_to(s.t[..., None], d.shape)[d == 1]) <= N * 2.0 ** -24).all()
    assert (off[d == 1] >= 0).all() and (off[d == 1] <= 1).all()
    # exactly one end of every edge is inside, and the interpolated mass there is iso
    m = np.zeros((N + 2,) * 3, dtype=np.float32)
    m[1:-1, 1:-1, 1:-1] = field.values()[0]
    fa, fb = m[tuple((s.A + 1).transpose(2, 0, 1))], m[tuple((s.B + 1).transpose(2, 0, 1))]
    assert ((fa > 1) != (fb > 1)).all()
    mass = fa.astype(np.float64) + s.t.astype(np.float64) * (fb.astype(np.float64) - fa)
    assert (np.abs(mass - 1.0) <= 2.0 ** -22 * (np.abs(fa) + np.abs(fb))).all()


def test_a_vertex_depends_on_its_edge_only(hashed):
    """The same edge, asked for by different tetrahedra and cells, gives the same bits - and different edges different vertices (or a
    degenerate meeting at a node)."""
    _, s = hashed
    edge = np.concatenate([s.A.reshape(-1, 3), s.B.reshape(-1, 3)], axis=1)
    _, inv, counts = np.unique(edge, axis=0, return_inverse=True, return_counts=True)
    assert counts.min() >= 2 and counts.max() >= 6                                # every edge is shared; the main diagonal by six
    bits = s.tris.view(np.uint32).reshape(-1, 3)
    order = np.argsort(inv.reshape(-1), kind="stable")
    same_edge = inv.reshape(-1)[order][1:] == inv.reshape(-1)[order][:-1]
    assert (bits[order][1:][same_edge] == bits[order][:-1][same_edge]).all()


# ---- the decomposition --------------------------------------------------------------------------------------------------------------------
def test_the_six_tetrahedra_tile_the_cube_and_agree_across_faces():
    tets = [im.tet_corners(p) for p in im.PERMS]
    dets = [round(float(np.linalg.det((c[1:] - c[0]).astype(np.float64)))) for c in tets]
    assert sorted(dets) == [-1, -1, -1, 1, 1, 1] and sum(abs(d) for d in dets) / 6.0 == 1.0
    assert [d < 0 for d in dets] == [im.perm_is_odd(p) for p in im.PERMS]
    rng = np.random.default_rng(2)
    pts = rng.uniform(0, 1, (2000, 3))
    hits = np.zeros(len(pts), dtype=int)
    for c in tets:                                                                # barycentric coordinates all positive: inside
        lam = np.linalg.solve((c[1:] - c[0]).T.astype(np.float64), pts.T).T
        hits += ((lam > 0).all(axis=1) & (lam.sum(axis=1) < 1))
    assert (hits == 1).all()
    for c in tets:
        assert (np.diff(c, axis=0) >= 0).all()                                    # c0 <= c1 <= c2 <= c3 componentwise: every edge has its order
    edges = {(tuple(c[i]), tuple(c[j])) for c in tets for i in range(4) for j in range(i + 1, 4)}
    assert len(edges) == 19                                                       # 12 cube edges, 6 face diagonals, the main diagonal
    for axis in range(3):
        def diagonals(side):
            rest = [a for a in range(3) if a != axis]
            return {tuple((e[0][a], e[1][a]) for a in rest) for e in edges if e[0][axis] == side and e[1][axis] == side and all(e[0][a] != e[1][a] for a in rest)}
        assert diagonals(0) == diagonals(1) and len(diagonals(0)) == 1            # the face shared with the neighbour carries the same diagonal


def test_case_table_winds_outward_in_every_tetrahedron():
    """Real positions: for every tetrahedron and case, with random inside / outside values, the emitted normals point from the inside
    corners to the outside corners; odd permutations are the even table with the last two vertices exchanged."""
    rng = np.random.default_rng(4)
    for perm, table in zip(im.PERMS, im.TABLES):
        c = im.tet_corners(perm).astype(np.float64)
        for mask in range(1, 15):
            want = [[t[0], t[2], t[1]] for t in im.TABLES[0][mask]] if im.perm_is_odd(perm) else im.TABLES[0][mask]
            assert table[mask] == want
            assert len(table[mask]) == (2 if bin(mask).count("1") == 2 else 1)
            for _ in range(20):
                f = np.where([(mask >> i) & 1 for i in range(4)], rng.uniform(1.1, 3.0, 4), rng.uniform(0.0, 0.9, 4))
                ins = np.array([(mask >> i) & 1 for i in range(4)], dtype=bool)
                out_dir = c[~ins].mean(axis=0) - c[ins].mean(axis=0)
                for tri in table[mask]:
                    assert all(ins[i] != ins[j] and i < j for i, j in tri)
                    p = [c[i] + (1.0 - f[i]) / (f[j] - f[i]) * (c[j] - c[i]) for i, j in tri]
                    assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), out_dir) > 0, (perm, mask)


# ---- clipping -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", [((-1, -1, -1), (3, 6, 2)), ((13, 14, 12), (22, 15, 30)), ((0, 0, 0), (N, N, N)), ((-1, -1, -1), (N, N, N)), ((40, 40, 40), (50, 50, 50)),
                                 ((N - 1, 56, N - 2), (N + 7, N + 7, N + 7)), ((9, 9, 9), (3, 3, 3))])
def test_a_cell_box_returns_the_triangles_of_its_cells(hashed, box):
    field, whole = hashed
    lo, hi = np.array(box[0]), np.array(box[1])
    part = im.isosurface(field.dense, 1.0, lo=lo, hi=hi)
    sel = ((whole.cell >= lo) & (whole.cell < hi)).all(axis=1)
    assert part.count == int(sel.sum())
    assert np.array_equal(part.canonical(), im.canonical(whole.tris[sel]))
    if box == ((-1, -1, -1), (N, N, N)):
        assert part.count == whole.count
    if box[0] == (40, 40, 40) or box[0] == (9, 9, 9):
        assert part.count == 0
    with pytest.raises(ValueError):
        im.isosurface(field.dense, 1.0, lo=lo)


def test_canonical_form_ignores_order_and_rotation_only(hashed):
    _, s = hashed
    rng = np.random.default_rng(6)
    sub = s.tris[rng.permutation(s.count)[:3000]]
    rolled = np.stack([np.roll(t, int(r), axis=0) for t, r in zip(sub, rng.integers(0, 3, len(sub)))])[rng.permutation(len(sub))]
    assert np.array_equal(im.canonical(sub), im.canonical(rolled))
    flipped = sub.copy()
    flipped[0] = flipped[0][[0, 2, 1]]
    assert not np.array_equal(im.canonical(sub), im.canonical(flipped))           # a reversed winding is another surface
    order, rot = im.canonical_order(sub)
    assert np.array_equal(im.apply_order(sub, order, rot).view(np.uint32).reshape(-1, 9), im.canonical(sub))


# ---- welding and the OBJ file -------------------------------------------------------------------------------------------------------------
def synthetic_soup():
    """A tetrahedron's four faces (closed), a degenerate triangle on one of its vertices, and -0 beside +0 (different bits: not welded)."""
    p = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    faces = [(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)]
    tris = np.stack([p[list(f)] for f in faces] + [np.float32([p[1], p[1], p[2]]), np.float32([[-0.0, 0, 0], [0.5, 0.25, 0.125], [1 / 3, 2 / 3, 1e-20]])])
    vel = np.arange(tris.size, dtype=np.float32).reshape(tris.shape)
    return tris, vel


def test_weld_triangles():
    tris, vel = synthetic_soup()
    V, F, W = weld_triangles(tris, vel)
    assert V.dtype == np.float32 and F.dtype == np.int32 and W.dtype == np.float32
    assert V.shape == (7, 3) and F.shape == (5, 3) and W.shape == (7, 3)          # 4 corners, -0, and two more; the degenerate triangle is dropped
    rows = V.view(np.uint32)
    assert np.array_equal(rows, np.unique(rows, axis=0))                          # unique and sorted on the bits
    assert np.array_equal(V[F].view(np.uint32), tris[[0, 1, 2, 3, 5]].view(np.uint32))
    flat_p, flat_v = tris.reshape(-1, 3).view(np.uint32), vel.reshape(-1, 3)
    for v, w in zip(rows, W):
        first = int(np.argmax((flat_p == v).all(axis=1)))
        assert np.array_equal(w, flat_v[first])                                   # the velocity of the first occurrence
    V2, F2 = weld_triangles(tris)
    assert np.array_equal(V2, V) and np.array_equal(F2, F)
    assert im.open_edges(tris[:4]) == 0 and abs(im.signed_volume(tris[:4]) - 1 / 6) < 1e-12
    Vm, Fm, _ = im.weld(tris)
    assert np.array_equal(Vm, V) and np.array_equal(Fm, F)
    V0, F0, W0 = weld_triangles(np.zeros((0, 3, 3), np.float32), np.zeros((0, 3, 3), np.float32))
    assert V0.shape == (0, 3) and F0.shape == (0, 3) and W0.shape == (0, 3)


def parse_obj(path):
    v, f = [], []
    for line in open(path).read().splitlines():
        tag, *rest = line.split()
        assert tag in ("v", "f") and len(rest) == 3, line
        (v if tag == "v" else f).append([float(x) for x in rest] if tag == "v" else [int(x) for x in rest])
    return np.array(v, dtype=np.float64).reshape(-1, 3), np.array(f, dtype=np.int64).reshape(-1, 3)


def test_obj_writer_welds_like_the_wrapper(tmp_path):
    exe = tmp_path / "host_selftest"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(HOST, "host_selftest.cpp")])
    tris, _ = synthetic_soup()
    raw = tmp_path / "soup.f32"
    tris.tofile(raw)
    out = tmp_path / "surface_frame[0].obj"
    subprocess.check_call([str(exe), "--obj-from", str(raw), str(out)])
    text = open(out).read()
    assert text.startswith("v ") and text.endswith("\n") and text.index("f ") > text.rindex("v ")   # all the vertices, then all the faces
    v, f = parse_obj(out)
    V, F = weld_triangles(tris)
    assert np.array_equal(v.astype(np.float32).view(np.uint32), V.view(np.uint32))               # nine digits give the float32 back; -0 keeps its sign
    assert np.array_equal(f, F.astype(np.int64) + 1)                                              # 1-based
    # an empty soup is an empty file, a ragged one is refused
    np.zeros(0, np.float32).tofile(raw)
    subprocess.check_call([str(exe), "--obj-from", str(raw), str(out)])
    assert open(out).read() == ""
    np.zeros(10, np.float32).tofile(raw)
    assert subprocess.run([str(exe), "--obj-from", str(raw), str(out)]).returncode == 5


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ffi_table():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "claymore_amd.h")).read(), flags=re.S)
    lines = [" ".join(l.split()) for l in txt.splitlines()]
    decl = "int mpm_grid_isosurface(mpm_ctx* ctx, float iso_mass, const int lo[3], const int hi[3], float* tri_xyz, float* tri_vel, size_t* n);"
    assert lines.count(decl) == 1
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True).split()
    assert "mpm_grid_isosurface" in exported
    assert "grid_isosurface" in _ffi.HIP_ONLY and "grid_isosurface" not in _ffi.SIGNATURES       # HIP library only: the oracle has no counterpart
    hip = _ffi.load_hip()
    assert hip.build_info().decode().startswith("claymore_hip abi7 ")                             # an additive export does not bump the ABI
    assert hip.grid_isosurface(None, 1.0, None, None, None, None, None) == _ffi.MPM_ERR_NOT_READY  # a NULL context, without touching a device


def test_the_kernel_table_is_the_models():
    """The 16 words of iso_case_triangles (mpm_grid_isosurface.hpp) are the model's table of the identity permutation, four bits a vertex."""
    src = open(os.path.join(ROOT, "claymore_amd", "csrc", "mpm_grid_isosurface.hpp")).read()
    words = {int(m.group(1)): int(m.group(2), 16) for m in re.finditer(r"case (\d+): return 0x([0-9a-f]+)u;", src)}
    assert sorted(words) == list(range(1, 15))
    for mask in range(1, 15):
        want = 0
        for slot, (i, j) in enumerate(e for tri in im.TABLES[0][mask] for e in tri):
            want |= (i | (j << 2)) << (4 * slot)
        assert words[mask] == want, mask
    odd = int(re.search(r"kIsoOddPerms = 0x([0-9a-f]+)u", src).group(1), 16)
    assert [bool(odd >> p & 1) for p in range(6)] == [im.perm_is_odd(p) for p in im.PERMS]
    assert im.PERMS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]         # p = 2 a + (b is the larger of the other two)

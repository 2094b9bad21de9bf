"""The mesh-built collision field without a GPU: the x86 build of the kernel's own functions (claymore_amd/csrc/mpm_collision_mesh.hpp through
claymore_amd/host/host_selftest.cpp --mesh-closest / --mesh-check) against the NumPy model (tests/collision_mesh_model.py) bit for bit,
the install's validation, the OBJ reader of the gmpm driver, and the model against closed forms."""
import os
import subprocess

import numpy as np
import pytest

import collision_mesh_model as mm
import collision_shape_model as sm
from claymore_amd import scenes
from claymore_amd.engine import weld_triangles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
VERDICTS = {"ok": "ok", "few": "fewer than 4 triangles", "index": "index outside", "nonfinite": "not finite", "degenerate": "degenerate",
            "open": "not a closed, consistently oriented manifold", "volume": "signed volume"}


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh") / "host_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-o", exe, os.path.join(HOST, "host_selftest.cpp")])
    return exe


def closest(exe, tmp_path, verts, tris, pts):
    """host_selftest --mesh-closest: T, feature (int) and q, sdis, g (float32 from their printed bits)."""
    obj, raw = str(tmp_path / "m.obj"), str(tmp_path / "p.f32")
    mm.write_obj(obj, verts, tris)
    np.ascontiguousarray(pts, dtype=np.float32).tofile(raw)
    rows = [l.split() for l in subprocess.check_output([exe, "--mesh-closest", obj, raw], text=True).splitlines()]
    assert len(rows) == len(pts)
    words = np.array([[int(w, 16) for w in r[2:]] for r in rows], dtype=np.uint32).view(np.float32)
    return np.array([int(r[0]) for r in rows]), np.array([int(r[1]) for r in rows]), words[:, 0], words[:, 1:]


def check(exe, tmp_path, verts, tris, pts):
    """... equal to the model, bit for bit in q and the four words; returns the model's result."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    res = mm.Mesh(verts, tris).field(pts)
    T, feature, q, out = closest(exe, tmp_path, verts, tris, pts)
    assert np.array_equal(T, res["T"])
    assert np.array_equal(feature, res["feature"])
    assert np.array_equal(q.view(np.uint32), res["q"].view(np.uint32))
    assert np.array_equal(out.view(np.uint32), res["out"].view(np.uint32))
    return res


def mesh_check(exe, tmp_path, verts, tris, name="c.obj"):
    obj = str(tmp_path / name)
    mm.write_obj(obj, verts, tris)
    return dict(l.split(" ", 1) for l in subprocess.check_output([exe, "--mesh-check", obj], text=True).splitlines())


# ---- single triangles: all seven features ---------------------------------------------------------------------------------------------------
def test_single_triangle_features(selftest, tmp_path):
    v = np.array([(0.2, 0.3, 0.4), (0.7, 0.35, 0.45), (0.3, 0.8, 0.5)], dtype=np.float32)
    a, b, c = v.astype(np.float64)
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    centroid = (a + b + c) / 3
    pts = [a, b, c]                                                                                # exactly on a vertex
    pts += [0.5 * (a + b), 0.5 * (a + c), 0.5 * (b + c)]                                           # on (or a rounding off) an edge
    for corner in (a, b, c):                                                                       # beyond each corner, either side
        pts += [corner + 0.2 * (corner - centroid) + s * 0.05 * n for s in (1, -1)]
    for u, w in ((a, b), (a, c), (b, c)):                                                          # off each edge, either side
        mid = 0.5 * (u + w)
        pts += [mid + 0.3 * (mid - centroid) + s * 0.07 * n for s in (1, -1)]
    pts += [centroid + s * 0.1 * n for s in (1, -1)] + [centroid]                                  # over, under and on the face
    res = check(selftest, tmp_path, v, [(0, 1, 2)], np.array(pts))
    assert set(res["feature"].tolist()) == set(range(7))
    radial = ~res["plane"]
    assert (res["margin"][radial] >= mm.SIGN_MARGIN).all()
    assert (res["q"][:3] == 0).all() and res["plane"][:3].all()                                    # on a vertex: the plane rule
    assert np.array_equal(res["feature"][:3], [mm.CORNER_A, mm.CORNER_B, mm.CORNER_C])


def test_in_plane_points_and_ties(selftest, tmp_path):
    # a triangle in the plane z = 0.25 (all coordinates dyadic): in-plane points outside it have (p - c) . m = 0 exactly - the sign is +
    v = np.array([(0.25, 0.25, 0.25), (0.75, 0.25, 0.25), (0.25, 0.75, 0.25)], dtype=np.float32)
    pts = np.array([(0.125, 0.125, 0.25), (0.5, 0.125, 0.25), (0.875, 0.125, 0.25), (0.75, 0.75, 0.25), (0.125, 0.5, 0.25), (0.125, 0.875, 0.25),
                    (0.5, 0.25, 0.25), (0.375, 0.375, 0.25)], dtype=np.float32)
    res = check(selftest, tmp_path, v, [(0, 1, 2)], pts)
    out = res["out"]
    assert (out[:6, 0] > 0).all() and (out[:6, 3] == 0).all() and not res["plane"][:6].any()
    assert (out[6:, 0] == 0).all() and res["plane"][6:].all()
    # two mirror-image triangles and the same triangle twice: the points of the mirror plane are equidistant - the lowest index wins
    v2 = np.array([(0.25, 0.25, 0.25), (0.25, 0.75, 0.25), (0.25, 0.25, 0.75), (0.75, 0.25, 0.25), (0.75, 0.75, 0.25), (0.75, 0.25, 0.75)], dtype=np.float32)
    t2 = [(3, 4, 5), (0, 1, 2), (3, 4, 5)]
    pts2 = np.array([(0.5, 0.375, 0.375), (0.5, 0.125, 0.5), (0.5, 0.875, 0.875), (0.875, 0.375, 0.375)], dtype=np.float32)
    m = mm.Mesh(v2, t2)
    q, _, _ = mm.walk(pts2[:3, None, :], m.a[None], m.ab[None], m.ac[None])
    assert (q[:, 0] == q[:, 1]).all() and (q[:, 0] == q[:, 2]).all()
    res = check(selftest, tmp_path, v2, t2, pts2)
    assert (res["T"] == 0).all()


# ---- the meshes of the GPU tests, seeded points ---------------------------------------------------------------------------------------------
MESHES = {"octahedron": lambda: mm.octahedron(), "box": lambda: scenes.box_mesh((0.21, 0.33, 0.27), (0.71, 0.62, 0.79)),
          "on-grid box": lambda: scenes.box_mesh((0.25,) * 3, (0.75,) * 3), "icosphere 2": lambda: scenes.icosphere((0.5, 0.34, 0.5), 6.0 / 64, 2)}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_seeded_points_match_bit_for_bit(selftest, tmp_path, name):
    verts, tris = MESHES[name]()
    rng = np.random.default_rng(11)
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    span = (hi - lo).max()
    wide = rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (1500, 3))                                 # around the mesh, inside and outside
    tv = verts.astype(np.float64)[tris[rng.integers(0, len(tris), 1500)]]
    bary = rng.dirichlet((1, 1, 1), 1500)
    near = np.einsum("nk,nkd->nd", bary, tv) + rng.normal(0, 0.02 * span, (1500, 3))               # close to the surface
    pts = np.concatenate([wide, near]).astype(np.float32)
    mesh = mm.Mesh(verts, tris)
    assert mm.validate(verts, tris)[0] == "ok"
    res = check(selftest, tmp_path, verts, tris, pts)
    mm.check_signs(mesh, res, pts)
    assert (~res["plane"]).sum() > 100 and res["plane"].sum() > 100
    assert len(set(res["feature"].tolist())) >= 5


# ---- validation -----------------------------------------------------------------------------------------------------------------------------
def broken_meshes():
    v, f = scenes.box_mesh((0.21, 0.33, 0.27), (0.71, 0.62, 0.79))
    flipped = f.copy()
    flipped[5] = flipped[5, ::-1]
    degenerate = np.concatenate([f, [(0, 1, 1), (0, 1, 1)]]).astype(np.int32)
    return {"sound": (v, f, "ok"), "open": (v, f[:-1], "open"), "one triangle flipped": (v, flipped, "open"), "wound inward": (v, f[:, ::-1], "volume"),
            "degenerate triangle": (v, degenerate, "degenerate"), "duplicated triangle": (v, np.concatenate([f, f[:1]]), "open"),
            "three triangles": (v, f[:3], "few")}


@pytest.mark.parametrize("name", sorted(broken_meshes()))
def test_mesh_check_agrees_with_the_model(selftest, tmp_path, name):
    v, f, want = broken_meshes()[name]
    tag, closed, volume = mm.validate(v, f)
    assert tag == want
    rep = mesh_check(selftest, tmp_path, v, f)
    assert int(rep["nv"]) == len(v) and int(rep["nt"]) == len(f)
    assert VERDICTS[tag] in rep["verdict"], rep
    if tag != "few":
        assert int(rep["closed"]) == int(closed)
        assert float(rep["volume"]) == pytest.approx(volume, rel=1e-12, abs=1e-15)
    if tag == "volume":
        assert "flip the winding" in rep["verdict"] and "inside_out" in rep["verdict"]


# ---- the OBJ reader ---------------------------------------------------------------------------------------------------------------------------
def test_obj_reader_round_trips_the_surface_writer(selftest, tmp_path):
    verts, tris = scenes.icosphere((0.4, 0.5, 0.6), 0.2, 1)
    soup = verts[tris]                                                                             # (nt, 3, 3): what mpm_grid_isosurface hands out
    raw, obj = str(tmp_path / "soup.f32"), str(tmp_path / "soup.obj")
    soup.tofile(raw)
    subprocess.check_call([selftest, "--obj-from", raw, obj])
    V, F = weld_triangles(soup)
    rep = dict(l.split(" ", 1) for l in subprocess.check_output([selftest, "--mesh-check", obj], text=True).splitlines())
    assert (int(rep["nv"]), int(rep["nt"]), rep["verdict"]) == (len(V), len(F), "ok")
    assert float(rep["volume"]) == pytest.approx(mm.Mesh(V, F).volume, rel=1e-12)
    # every vertex came back with its bits: it lies on the mesh that was read, at distance exactly zero
    V.tofile(str(tmp_path / "v.f32"))
    rows = subprocess.check_output([selftest, "--mesh-closest", obj, str(tmp_path / "v.f32")], text=True).splitlines()
    assert len(rows) == len(V) and all(r.split()[2] == "00000000" for r in rows)


def test_obj_reader_reads_quads_suffixes_and_negative_indices(selftest, tmp_path):
    v, f = scenes.box_mesh((0.25, 0.25, 0.25), (0.5, 0.75, 0.625))
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    obj = str(tmp_path / "quads.obj")
    with open(obj, "w") as fh:
        fh.write("# a box\nvn 0 0 1\nvt 0.5 0.5\n")
        for x in v:
            fh.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in x))
        fh.write("g sides\n")
        for k, q in enumerate(quads):
            if k % 3 == 0:
                fh.write("f " + " ".join(str(i + 1) for i in q) + "\n")
            elif k % 3 == 1:
                fh.write("f " + " ".join("%d/1/1" % (i + 1) for i in q) + "\n")
            else:
                fh.write("f " + " ".join("%d//1" % (i - 8) for i in q) + "\n")                      # -8 .. -1: relative to the vertices read so far
    rep = dict(l.split(" ", 1) for l in subprocess.check_output([selftest, "--mesh-check", obj], text=True).splitlines())
    assert (int(rep["nv"]), int(rep["nt"]), int(rep["closed"]), rep["verdict"]) == (8, 12, 1, "ok")
    assert float(rep["volume"]) == pytest.approx(mm.Mesh(v, f).volume, rel=1e-12)


# ---- the model against closed forms -----------------------------------------------------------------------------------------------------------
def test_box_field_is_the_closed_form_box():
    """Bound: the coordinates are below 1, so every float32 operation of the walk rounds by at most 2^-24 absolute; the longest chain (an
    edge: three subtractions, two dot products of three terms, a division by |edge|^2 >= 0.08, the point, the difference, q, sqrtf) stays
    below 24 such roundings after the division's amplification; the shape model's float32 centre and half extent add 2 x 2^-25.  32 x 2^-24."""
    lo, hi = (0.21, 0.33, 0.27), (0.71, 0.62, 0.79)
    verts, tris = scenes.box_mesh(lo, hi)
    v64 = verts.astype(np.float64)
    c = sm.collider("box", a=0.5 * (v64[0] + v64[7]), b=0.5 * (v64[7] - v64[0]))
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.uniform(0, 1, (3000, 3)), mm.grid_nodes(4)]).astype(np.float32)
    mesh = mm.Mesh(verts, tris)
    res = mesh.field(pts)
    mm.check_signs(mesh, res, pts)
    want, _ = sm.closed_form(c, pts)
    err = np.abs(res["out"][:, 0].astype(np.float64) - want).max()
    print(f"box: max |sdis - closed form| = {err:.3e} (bound {32 * 2.0 ** -24:.3e})")
    assert err <= 32 * 2.0 ** -24
    assert np.allclose(np.linalg.norm(res["out"][:, 1:].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_icosphere_field_lies_between_its_spheres():
    centre, radius = np.array((0.5, 0.34, 0.5)), 6.0 / 64
    verts, tris = scenes.icosphere(centre, radius, 2)
    mesh = mm.Mesh(verts, tris)
    P = verts.astype(np.float64)[tris]
    inscribed = np.abs(np.einsum("ni,ni->n", mesh.nh64, P[:, 0] - centre)).min()
    circumscribed = np.linalg.norm(verts.astype(np.float64) - centre, axis=1).max()
    rng = np.random.default_rng(4)
    pts = rng.uniform(centre - 2 * radius, centre + 2 * radius, (3000, 3)).astype(np.float32)
    res = mesh.field(pts)
    mm.check_signs(mesh, res, pts)
    rho = np.linalg.norm(pts.astype(np.float64) - centre, axis=1)
    sdis = res["out"][:, 0].astype(np.float64)
    assert 0.9 * radius < inscribed < circumscribed < radius * (1 + 1e-6)
    assert (sdis >= rho - circumscribed - 32 * 2.0 ** -24).all() and (sdis <= rho - inscribed + 32 * 2.0 ** -24).all()


def test_scene_meshes_are_closed_and_outward():
    for verts, tris in (scenes.box_mesh((0.1, 0.2, 0.3), (0.4, 0.6, 0.9)), scenes.icosphere((0.5, 0.5, 0.5), 0.25, 3), mm.octahedron()):
        assert mm.validate(verts, tris)[0] == "ok"
    v, f = scenes.icosphere((0.5, 0.5, 0.5), 0.25, 3)
    assert len(f) == 1280 and len(v) == 642
    assert len(scenes.box_mesh((0, 0, 0), (1, 1, 1))[1]) == 12
    assert mm.Mesh(v, f).volume == pytest.approx(4 / 3 * np.pi * 0.25 ** 3, rel=0.02)
    sc = scenes.sphere_on_obstacle_mesh()
    assert "collision" not in sc and sc["collision_mesh"]["faces"].shape == (1280, 3) and sc["collision_mesh"]["type"] == 1

"""The mesh-sampled model without a GPU: the per-point host restatement (claymore_amd/csrc/mpm_mesh_fill.hpp's mesh_fill_host through
claymore_amd/host/host_selftest.cpp --mesh-fill) against the NumPy model (tests/mesh_fill_model.py) bit for bit in set and order, the model
against scenes.lattice_box and scenes.lattice_sphere, the refusals, and the binding.  domain_bits 6."""
import os
import subprocess

import numpy as np
import pytest

import collision_mesh_model as mm
import mesh_fill_model as fm
from claymore_amd import _ffi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "claymore_amd", "host")
BITS = 6
N = 1 << BITS
DX = 1.0 / N

# The tests' meshes, placed so that no candidate's sign is in doubt (asserted wherever they are used).  The box's faces are at half-cell
# positions: every candidate is a quarter cell off them.
BOX = ((20.5 * DX, 17.5 * DX, 22.5 * DX), (33.5 * DX, 30.5 * DX, 29.5 * DX))
MESHES = {"box": lambda: scenes.box_mesh(*BOX), "octahedron": lambda: mm.octahedron((0.47, 0.53, 0.51), 0.13),
          "icosphere 2": lambda: scenes.icosphere((0.5, 0.34, 0.5), 6.0 / 64, 2), "L prism": fm.l_prism}


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fill") / "host_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-o", exe, os.path.join(HOST, "host_selftest.cpp")])
    return exe


def host_fill(exe, tmp_path, verts, tris, bits=BITS, margin=None, box=None):
    """host_selftest --mesh-fill: the points as (n, 3) uint32 position bits, or the refusal's text."""
    obj = str(tmp_path / "m.obj")
    mm.write_obj(obj, verts, tris)
    cmd = [exe, "--mesh-fill", obj, str(bits)]
    if margin is not None or box is not None:
        cmd.append(repr(float(margin or 0.0)))
    if box is not None:
        cmd += [str(int(v)) for v in list(box[0]) + list(box[1])]
    lines = subprocess.check_output(cmd, text=True).splitlines()
    head = lines[0].split(" ", 1)
    if head[0] == "refused":
        return head[1]
    pts = np.array([[int(w, 16) for w in l.split()] for l in lines[1:]], dtype=np.uint32).reshape(-1, 3)
    assert head[0] == "count" and int(head[1]) == len(pts)
    return pts


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sorted_bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
    return a[np.lexsort(a.T[::-1])].view(np.uint32)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_host_restatement_equals_the_model_in_set_and_order(selftest, tmp_path, name):
    verts, tris = MESHES[name]()
    want = fm.sample(BITS, verts, tris)
    assert len(want["undecided"]) == 0, (name, len(want["undecided"]))                             # the test's condition on the placement
    got = host_fill(selftest, tmp_path, verts, tris)
    print(f"{name}: {len(got)} points of {len(want['candidates'])} candidates")
    assert len(got) > 500 and np.array_equal(got, bits_of(want["points"]))
    margin = 0.75 * DX
    want_m = fm.sample(BITS, verts, tris, margin=margin)
    got_m = host_fill(selftest, tmp_path, verts, tris, margin=margin)
    assert 0 < len(got_m) < len(got) and np.array_equal(got_m, bits_of(want_m["points"]))


def test_clip_box_through_a_tile_and_empty_results(selftest, tmp_path):
    verts, tris = MESHES["octahedron"]()
    box = ((0, 30, 0), (N, 39, 35))                                                                # cuts tiles 28 .. 31 and 36 .. 39 in y, 32 .. 35 in z
    want = fm.sample(BITS, verts, tris, box=box)
    got = host_fill(selftest, tmp_path, verts, tris, box=box)
    assert len(got) > 100 and np.array_equal(got, bits_of(want["points"]))
    whole = fm.sample(BITS, verts, tris)["points"]
    node = np.rint(whole.astype(np.float64) * N).astype(int)
    keep = ((node >= box[0]) & (node < box[1])).all(axis=1)
    assert np.array_equal(bits_of(whole[keep]), got)                                               # tiles are the domain's: the order does not depend on the box
    assert len(host_fill(selftest, tmp_path, verts, tris, box=((10, 10, 10), (10, 40, 40)))) == 0  # hi <= lo on an axis
    tiny = scenes.box_mesh((0.505, 0.505, 0.505), (0.510, 0.510, 0.510))                          # holds no candidate
    assert len(host_fill(selftest, tmp_path, *tiny)) == 0 and len(fm.sample(BITS, *tiny)["points"]) == 0


def test_box_mesh_gives_exactly_the_lattice_box():
    got = fm.sample(BITS, *MESHES["box"]())
    assert len(got["undecided"]) == 0
    want = scenes.lattice_box(BITS, (21, 18, 23), (34, 31, 30))                                   # the nodes the faces at .5 enclose
    assert np.array_equal(sorted_bits(got["points"]), sorted_bits(want))


def test_icosphere_count_is_within_the_shell_bound_of_the_lattice_sphere():
    """With r_in the polyhedron's inradius and r_out its circumradius about the centre, ball(r_in) < polyhedron < ball(r_out): the mesh's count
    lies between the lattice's counts at those two radii, lattice_sphere's own count (at the nominal radius = r_out up to float32 rounding of
    the vertices) included in the same interval."""
    centre, radius = np.array((0.5, 0.34, 0.5)), 6.0 / 64
    verts, tris = scenes.icosphere(centre, radius, 2)
    mesh = mm.Mesh(verts, tris)
    P = verts.astype(np.float64)[tris]
    r_in = np.abs(np.einsum("ni,ni->n", mesh.nh64, P[:, 0] - centre)).min()
    r_out = np.linalg.norm(verts.astype(np.float64) - centre, axis=1).max()
    n_mesh = len(fm.sample(BITS, verts, tris)["points"])
    n_in = len(scenes.lattice_sphere(BITS, centre, (r_in - 1e-6) / DX))
    n_out = len(scenes.lattice_sphere(BITS, centre, (r_out + 1e-6) / DX))
    n_sphere = len(scenes.lattice_sphere(BITS, centre, radius / DX))
    print(f"icosphere: {n_mesh} points; lattice spheres {n_in} (r_in = {r_in / DX:.3f} dx) .. {n_out} (r_out = {r_out / DX:.3f} dx), nominal {n_sphere}")
    assert n_in <= n_mesh <= n_out and n_in <= n_sphere <= n_out
    assert abs(n_mesh - n_sphere) <= n_out - n_in


def test_mesh_drop_scene_is_sphere_drop_with_a_mesh_body():
    sc, ref = scenes.mesh_drop(bits=BITS, radius_cells=6.0), scenes.sphere_drop(bits=BITS, radius_cells=6.0, center=(0.5, 0.3, 0.5))
    model, = sc["models"]
    assert "xyz" not in model and mm.validate(model["mesh"]["vertices"], model["mesh"]["faces"])[0] == "ok" and len(model["mesh"]["faces"]) == 1280
    assert (sc["bits"], sc["dt"], sc["config"], model["material"], model["params"]) == (ref["bits"], ref["dt"], ref["config"], ref["models"][0]["material"], ref["models"][0]["params"])
    got = fm.sample(BITS, model["mesh"]["vertices"], model["mesh"]["faces"], margin=model["mesh"]["margin"])
    sphere = set(map(bytes, bits_of(ref["models"][0]["xyz"])))
    assert len(got["undecided"]) == 0 and set(map(bytes, bits_of(got["points"]))) <= sphere and len(got["points"]) > 0.9 * len(sphere)


def test_refusals(selftest, tmp_path):
    v, f = MESHES["box"]()
    assert "not a closed" in host_fill(selftest, tmp_path, v, f[:-1])
    assert "signed volume" in host_fill(selftest, tmp_path, v, f[:, ::-1])
    assert "margin" in host_fill(selftest, tmp_path, v, f, margin=-0.01)
    assert "margin" in host_fill(selftest, tmp_path, v, f, margin=float("nan"))
    assert "lo / hi" in host_fill(selftest, tmp_path, v, f, box=((0, 0, -1), (N, N, N)))
    assert "lo / hi" in host_fill(selftest, tmp_path, v, f, box=((0, 0, 0), (N, N + 1, N)))


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True).split()
    for name in ("sample_mesh", "add_model_mesh", "test_mesh_fill"):
        assert "mpm_" + name + "(" in header and "mpm_" + name in exported
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES                               # HIP library only: the oracle has no counterpart
    import ctypes as C
    assert C.sizeof(_ffi.MeshFill) == 4 * (1 + 3 + 3 + 1 + 8)

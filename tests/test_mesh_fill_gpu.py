"""The mesh-sampled model on the device (mpm_sample_mesh, mpm_add_model_mesh; claymore_amd/csrc/mpm_mesh_fill.hpp) against the per-point NumPy
model (tests/mesh_fill_model.py), bit for bit in set and order; the order through the product path (track_ids); the equivalence with the same
array given to mpm_add_model; several models in one context; the refusals; the gmpm driver's "file": "name.obj".  domain_bits 6 unless noted.
Every compared mesh is placed so that the model finds no candidate whose sign is in doubt, and that is asserted."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import collision_mesh_model as mm
import mesh_fill_model as fm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError
from test_mesh_fill_model_cpu import BITS, DX, MESHES, N, bits_of, sorted_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRM = {"volume": scenes._vol(BITS), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
# name -> (mesh, margin, box).  Every mesh's bounding box is off the tiles' faces (the box mesh's is 20.5 .. 33.5 cells).  The octahedron (8)
# and the box (12) have fewer triangles than a wave has lanes; every tile near the 1280-triangle icosphere of radius 6 dx sees all of it
# within D + 2 r (2 r = 6.06 dx): ten chunks of candidates.
CASES = {name: (mesh, 0.0, None) for name, mesh in MESHES.items()}
CASES.update({name + ", margin": (mesh, 0.75 * DX, None) for name, mesh in MESHES.items()})
CASES["icosphere 3"] = (lambda: scenes.icosphere((0.47, 0.53, 0.51), 6.0 / 64, 3), 0.0, None)
# 80 triangles, no multiple of 64: the walk's last sweep is partly filled (the bound's lanes clamped to nt - 1, the candidate test's excluded)
CASES["icosphere 1, 80 triangles"] = (lambda: scenes.icosphere((0.47, 0.52, 0.55), 0.21, 1), 0.0, None)
CASES["octahedron, box through tiles"] = (MESHES["octahedron"], 0.0, ((0, 30, 0), (N, 39, 35)))
CASES["L prism, box and margin"] = (MESHES["L prism"], 0.3 * DX, ((19, 0, 21), (38, N, 30)))
TINY = ((0.505, 0.505, 0.505), (0.510, 0.510, 0.510))                                              # between two candidates: holds none


def modelled(bits, verts, tris, margin=0.0, box=None):
    want = fm.sample(bits, verts, tris, margin=margin, box=box)
    assert len(want["undecided"]) == 0, len(want["undecided"])                                     # the test's condition on the placement
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_sample_mesh_equals_the_model_in_set_and_order(name):
    mesh, margin, box = CASES[name]
    verts, tris = mesh()
    want = modelled(BITS, verts, tris, margin, box)
    got = Engine.sample_mesh(BITS, verts, tris, margin=margin, box=box)
    print(f"{name}: {len(got)} points (model {len(want['points'])}) of {len(want['candidates'])} candidates, {len(tris)} triangles")
    assert got.shape == want["points"].shape and len(got) > 100
    assert np.array_equal(bits_of(got), bits_of(want["points"]))


def test_empty_results_and_the_count_first_protocol():
    tiny = scenes.box_mesh(*TINY)
    assert Engine.sample_mesh(BITS, *tiny).shape == (0, 3)
    verts, tris = MESHES["octahedron"]()
    assert Engine.sample_mesh(BITS, verts, tris, box=((10, 10, 10), (10, 40, 40))).shape == (0, 3)  # hi <= lo on an axis
    api = _ffi.load_hip()
    n = C.c_size_t(0)
    args = (BITS, verts.ctypes.data, len(verts), tris.ctypes.data, len(tris), None)
    assert api.sample_mesh(*args, None, C.byref(n), 0) == _ffi.MPM_OK                             # count
    total = n.value
    assert total == len(fm.sample(BITS, verts, tris)["points"])
    short = np.full((total - 1, 3), -7.0, dtype=np.float32)
    n = C.c_size_t(total - 1)
    assert api.sample_mesh(*args, short.ctypes.data, C.byref(n), 0) == _ffi.MPM_ERR_CAPACITY and n.value == total
    assert (short == -7.0).all()                                                                    # nothing written
    roomy = np.full((total + 5, 3), -7.0, dtype=np.float32)
    n = C.c_size_t(total + 5)
    assert api.sample_mesh(*args, roomy.ctypes.data, C.byref(n), 0) == _ffi.MPM_OK and n.value == total
    assert (roomy[total:] == -7.0).all() and np.array_equal(bits_of(roomy[:total]), bits_of(Engine.sample_mesh(BITS, verts, tris)))
    for bad in (dict(margin=-0.01), dict(margin=float("nan")), dict(box=((0, 0, -1), (N, N, N))), dict(box=((0, 0, 0), (N, N + 1, N)))):
        with pytest.raises(EngineError) as err:
            Engine.sample_mesh(BITS, verts, tris, **bad)
        assert err.value.code == _ffi.MPM_ERR_INVALID
    with pytest.raises(EngineError):
        Engine.sample_mesh(BITS, verts, tris[:-1])                                                  # open
    with pytest.raises(EngineError):
        Engine.sample_mesh(BITS, verts, tris[:, ::-1])                                              # wound inward


def test_bits_7_sphere_most_tiles_decided_from_their_centre():
    """The icosphere of radius 0.3 at domain_bits 7: 38 cells of radius, so most tiles of its bounding box are farther than r + margin from
    the surface and take their answer from the centre.  Per point against the model in a slab of four node layers through the centre - it
    crosses the surface at every angle in its plane and holds interior, shell and outside tiles -; the whole sampling holds the slab's points
    in the slab's order, every lattice point within the inradius and none beyond the circumradius."""
    bits, n = 7, 128
    centre, radius = np.array((0.5, 0.5, 0.5)), 0.3
    verts, tris = scenes.icosphere(centre, radius, 2)
    slab = ((0, 0, 62), (n, n, 66))
    want = modelled(bits, verts, tris, box=slab)
    got = Engine.sample_mesh(bits, verts, tris, box=slab)
    mismatches = -1 if got.shape != want["points"].shape else int((bits_of(got) != bits_of(want["points"])).any(axis=1).sum())
    print(f"slab: {len(got)} points (model {len(want['points'])}) of {len(want['candidates'])} candidates, {mismatches} mismatches")
    assert mismatches == 0
    stats = (C.c_double * 8)()
    api = _ffi.load_hip()
    assert api.test_mesh_fill(bits, verts.ctypes.data, len(verts), tris.ctypes.data, len(tris), None, stats, 0) == _ffi.MPM_OK
    whole = Engine.sample_mesh(bits, verts, tris)
    print(f"whole: {len(whole)} points, {int(stats[2])} of {int(stats[1])} tiles decided from their centre")
    assert int(stats[0]) == len(whole) and stats[2] > 0.5 * stats[1]
    node = np.rint(whole.astype(np.float64) * n).astype(int)
    assert np.array_equal(bits_of(whole[((node >= slab[0]) & (node < slab[1])).all(axis=1)]), bits_of(got))
    mesh = mm.Mesh(verts, tris)
    P = verts.astype(np.float64)[tris]
    r_in = np.abs(np.einsum("ni,ni->n", mesh.nh64, P[:, 0] - centre)).min()
    r_out = np.linalg.norm(verts.astype(np.float64) - centre, axis=1).max()
    rho = np.linalg.norm(whole.astype(np.float64) - centre, axis=1)
    assert rho.max() <= r_out + 1e-6
    core = scenes.lattice_sphere(bits, centre, (r_in - 1e-6) * n)
    assert len(core) == int((rho <= r_in - 1e-6).sum())                                             # distinct lattice points: equal counts, equal sets
    assert len(np.unique(whole.view(np.uint32), axis=0)) == len(whole)


@pytest.fixture(scope="module")
def ico():
    return scenes.icosphere((0.5, 0.34, 0.5), 6.0 / 64, 2)


def test_ids_follow_the_order_of_sample_mesh(ico):
    pts = Engine.sample_mesh(BITS, *ico)
    e = Engine(domain_bits=BITS, max_ppc=128, track_ids=True)
    mid = e.init_model_mesh(_ffi.FIXED_COROTATED, *ico, v0=(0.0, -0.5, 0.0), **PRM)
    assert mid == 0 and e.models[0]["n"] == len(pts)
    e.initial_setup()
    xyz, ids = e.retrieve_ids(0)
    assert sorted(ids.tolist()) == list(range(len(pts)))
    assert np.array_equal(bits_of(xyz[np.argsort(ids)]), bits_of(pts))
    assert np.array_equal(sorted_bits(e.retrieve_positions(0)), sorted_bits(pts))
    buf = e.save_checkpoint()                                                                       # the paths behind mpm_add_model work unchanged
    e.run_fixed(3, 1e-4)
    e.load_checkpoint(buf)
    assert np.array_equal(sorted_bits(e.retrieve_positions(0)), sorted_bits(pts))
    e.close()


def test_mesh_model_equals_the_array_model():
    """init_model_mesh against init_model on sample_mesh's array, 20 substeps: positions joined on the ids and mpm_grid_totals bit for bit.  The
    body is a box mesh around the 2 x 2 x 2 nodes 30, 31 (faces at 29.5 and 31.5 cells: 64 particles inside one particle block, whose faces
    are at 4 k + 1.5 cells), on which the engine is deterministic - a dense body differs in the last bits between two runs of one
    configuration (float atomics in P2G), and there would be nothing to compare."""
    verts, tris = scenes.box_mesh((29.5 * DX,) * 3, (31.5 * DX,) * 3)
    pts = Engine.sample_mesh(BITS, verts, tris)
    assert np.array_equal(sorted_bits(pts), sorted_bits(scenes.lattice_box(BITS, (30, 30, 30), (32, 32, 32))))
    out = []
    for how in ("mesh", "array", "mesh"):
        e = Engine(domain_bits=BITS, max_ppc=128, track_ids=True)
        if how == "mesh":
            e.init_model_mesh(_ffi.FIXED_COROTATED, verts, tris, v0=(0.3, -0.5, 0.1), **PRM)
        else:
            e.init_model(_ffi.FIXED_COROTATED, pts, (0.3, -0.5, 0.1), **PRM)
        e.initial_setup()
        e.run_fixed(20, 1e-4)
        xyz, ids = e.retrieve_ids(0)
        assert e.diagnostics().lost_particles == 0 and len(ids) == 64
        out.append((bits_of(xyz[np.argsort(ids)]), e.grid_totals().view(np.uint64)))
        e.close()
    assert not np.array_equal(out[0][0], bits_of(pts)), "nothing moved"
    for k in range(2):
        assert np.array_equal(out[0][k], out[1][k]), k
        assert np.array_equal(out[0][k], out[2][k]), k


def test_two_mesh_models_and_an_array_model_in_one_context(ico):
    octa = mm.octahedron((0.47, 0.7, 0.51), 0.13)                                                   # above the icosphere, clear of it
    block = scenes.lattice_box(BITS, (8, 40, 8), (14, 46, 14))
    e = Engine(domain_bits=BITS, max_ppc=128, track_ids=True)
    a = e.init_model_mesh(_ffi.FIXED_COROTATED, *ico, v0=(0.0, 0.5, 0.0), **PRM)
    b = e.init_model(_ffi.FIXED_COROTATED, block, (0.0, -0.5, 0.0), **PRM)
    c = e.init_model_mesh(_ffi.J_FLUID, *octa, margin=0.75 * DX)
    assert (a, b, c) == (0, 1, 2)
    want = [Engine.sample_mesh(BITS, *ico), block, Engine.sample_mesh(BITS, *octa, margin=0.75 * DX)]
    assert [m["n"] for m in e.models] == [len(w) for w in want]
    e.initial_setup()
    for m, w in enumerate(want):
        xyz, ids = e.retrieve_ids(m)
        assert np.array_equal(bits_of(xyz[np.argsort(ids)]), bits_of(w)), m
    e.run_fixed(5, 1e-4)
    cnt = e.counts()
    assert [int(cnt.particles[m]) for m in range(3)] == [len(w) for w in want] and e.diagnostics().lost_particles == 0
    e.close()


def test_mesh_drop_scene_runs_beside_sphere_drop():
    """scenes.mesh_drop through build_engine: the icosphere's particles are sphere_drop's less the shell between the polyhedron and its
    sphere, and after a few substeps under gravity both bodies have fallen alike."""
    from claymore_amd.engine import build_engine
    mesh_sc, sphere_sc = scenes.mesh_drop(bits=BITS, radius_cells=6.0), scenes.sphere_drop(bits=BITS, radius_cells=6.0, center=(0.5, 0.3, 0.5))
    ys = []
    for sc in (mesh_sc, sphere_sc):
        e = build_engine(sc)
        e.initial_setup()
        start = e.retrieve_positions(0)
        e.run_fixed(10, sc["dt"])
        ys.append((len(start), float(e.retrieve_positions(0)[:, 1].astype(np.float64).mean() - start[:, 1].astype(np.float64).mean())))
        assert e.diagnostics().lost_particles == 0
        e.close()
    sphere = set(map(bytes, bits_of(sphere_sc["models"][0]["xyz"])))
    filled = Engine.sample_mesh(BITS, **{k: mesh_sc["models"][0]["mesh"][k] for k in ("vertices", "faces")})
    assert ys[0][0] == len(filled) and set(map(bytes, bits_of(filled))) <= sphere and 0.9 * len(sphere) < len(filled) <= len(sphere)
    assert ys[0][1] < 0 and ys[0][1] == pytest.approx(ys[1][1], rel=0.05)


def test_refusals_leave_the_context_as_it_was(ico):
    e = Engine(domain_bits=BITS, max_ppc=128)
    verts, tris = ico
    for bad, why in ((dict(faces=tris[:-1]), "not a closed"), (dict(faces=tris[:, ::-1]), "flip the winding"), (dict(margin=-1.0), "margin"),
                     (dict(box=((0, 0, 0), (N, N, N + 1))), "lo / hi")):
        with pytest.raises(EngineError) as err:
            e.init_model_mesh(_ffi.FIXED_COROTATED, **{**dict(vertices=verts, faces=tris), **bad}, **PRM)
        assert err.value.code == _ffi.MPM_ERR_INVALID and why in str(err.value), (why, str(err.value))
    assert e.models == []
    assert e.init_model_mesh(_ffi.FIXED_COROTATED, *scenes.box_mesh(*TINY), **PRM) == 0 and e.models[0]["n"] == 0    # an empty model is legal
    assert e.init_model_mesh(_ffi.FIXED_COROTATED, verts, tris, **PRM) == 1
    e.initial_setup()
    with pytest.raises(EngineError) as err:
        e.init_model_mesh(_ffi.FIXED_COROTATED, verts, tris, **PRM)
    assert err.value.code == _ffi.MPM_ERR_INVALID and "before mpm_initial_setup" in str(err.value)
    assert len(e.models) == 2 and e.counts().model_count == 2
    e.run_fixed(3, 1e-4)                                                                            # the context still runs
    assert len(e.retrieve_positions(1)) == e.models[1]["n"] and len(e.retrieve_positions(0)) == 0
    e.close()


def test_gmpm_model_from_an_obj_file(tmp_path):
    """A gmpm model with "file": "body.obj": the mesh's bounding box scaled uniformly into `span` and moved to `offset` - v' = (v - mn) s + offset
    per axis in float32, s = min over the axes of span / (mx - mn) -, then the mesh fill with the model's "margin".  Frame 0 holds the model's
    points under that placement."""
    import __graft_entry__ as g
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    v, f = mm.octahedron((3.0, -2.0, 5.0), 4.0)                                                    # in units of its own
    mm.write_obj(str(tmp_path / "body.obj"), v, f)
    offset, span, margin = [0.31, 0.42, 0.36], [0.26, 0.3, 0.28], 0.3 * DX
    model = dict(PRM, file="body.obj", constitutive="fixed_corotated", offset=offset, span=span, velocity=[0, 0, 0], margin=margin)
    sim = {"gpuid": 0, "fps": 500, "frames": 1, "default_dt": 1e-4, "domain_bits": BITS, "output_dir": str(tmp_path)}
    (tmp_path / "scene.json").write_text(json.dumps({"simulation": sim, "models": [model]}))
    log = subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(tmp_path / "scene.json")], text=True, timeout=300)
    mn, mx = v.min(axis=0), v.max(axis=0)
    s = (np.asarray(span, dtype=np.float32) / (mx - mn)).min()
    placed = (v - mn) * s + np.asarray(offset, dtype=np.float32)
    assert placed.dtype == np.float32 and s.dtype == np.float32
    want = modelled(BITS, placed, f, margin=float(np.float32(margin)))
    got = read_bgeo_attrs(tmp_path / "model_id[0]_frame[0].bgeo")[0]
    print(f"gmpm: {len(got)} points, model {len(want['points'])}")
    assert f"init 0-th model with {len(want['points'])} particles" in log
    assert len(got) > 1000 and np.array_equal(sorted_bits(got), sorted_bits(want["points"]))
    last = read_bgeo_attrs(tmp_path / "model_id[0]_frame[1].bgeo")[0]
    assert len(last) == len(got)

"""The mesh-built collision field on the device (mpm_set_collision_mesh, claymore_amd/csrc/mpm_collision_mesh.hpp) against the NumPy model
(tests/collision_mesh_model.py), bit for bit in all four words and read through mpm_get_collision_field; the refusals, which change nothing;
removal and re-install; the equivalence with the same field installed through mpm_set_collision_object; the engine's own iso-surface as
input; the gmpm driver's "collision_mesh" key.  domain_bits 6 throughout."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import collision_mesh_model as mm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError, build_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = 6
N = 1 << BITS
DX = 1.0 / N


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sorted_rows(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x[np.lexsort(x.T[::-1])].view(np.uint32)


def two_boxes():
    v0, f0 = scenes.box_mesh((0.13, 0.21, 0.17), (0.41, 0.52, 0.45))
    v1, f1 = scenes.box_mesh((0.58, 0.47, 0.55), (0.86, 0.9, 0.81))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + 8]).astype(np.int32)


WHOLE_GRID = {"on-grid box": lambda: scenes.box_mesh((0.25,) * 3, (0.75,) * 3), "box": lambda: scenes.box_mesh((0.21, 0.33, 0.27), (0.71, 0.62, 0.79)),
              "octahedron": mm.octahedron, "two boxes": two_boxes}
ICO = dict(centre=(0.47, 0.53, 0.51), radius=0.2, subdivisions=3)


@pytest.fixture(scope="module")
def eng():
    e = Engine(domain_bits=BITS)
    yield e
    e.close()


def modelled(verts, tris, nodes):
    """The model's four words at `nodes`, after the tests' precondition on the sign (collision_mesh_model.check_signs)."""
    mesh = mm.Mesh(verts, tris)
    assert mm.validate(verts, tris)[0] == "ok"
    res = mesh.field(nodes)
    mm.check_signs(mesh, res, nodes)
    return res


@pytest.mark.parametrize("name", sorted(WHOLE_GRID))
def test_whole_grid_equals_the_model(eng, name):
    verts, tris = WHOLE_GRID[name]()
    eng.set_collision_mesh(verts, tris)
    got = eng.collision_field()
    assert got.shape == (N, N, N, 4)
    nodes = mm.grid_nodes(BITS)
    res = modelled(verts, tris, nodes)
    want = res["out"].reshape(N, N, N, 4)
    bad = (bits(got) != bits(want)).any(axis=-1)
    print(f"{name}: {int(bad.sum())} of {N ** 3} nodes differ; plane rule at {int(res['plane'].sum())}, on the surface {int((res['q'] < mm.PLANE_Q).sum())}")
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    assert np.isfinite(got).all()
    if name == "on-grid box":  # the nodes the q < 2^-40 clause exists for: on faces, and on edges, face diagonals and corners (features other than the face)
        on = res["q"] < mm.PLANE_Q
        off_face = on & (res["feature"] != mm.FACE)
        corners = on & (res["feature"] <= mm.CORNER_C)
        print(f"on the surface: {int(on.sum())}, of them not by the face region: {int(off_face.sum())}, corners: {int(corners.sum())}")
        assert on.sum() >= 6 * 31 * 31 and off_face.sum() >= 134 and corners.sum() >= 8
        assert (res["out"][on, 0] == 0).all()
    if name == "two boxes":
        T = res["T"]
        assert (T < 12).any() and (T >= 12).any()
    # inside_out: every word is the negation
    eng.set_collision_mesh(verts, tris, inside_out=True)
    assert np.array_equal(bits(eng.collision_field()), bits(got) ^ np.uint32(0x80000000))


def test_icosphere_straddling_box_centre_tile_and_far_nodes(eng):
    verts, tris = scenes.icosphere(ICO["centre"], ICO["radius"], ICO["subdivisions"])
    assert len(tris) == 1280
    eng.set_collision_mesh(verts, tris)
    lattice = np.stack(np.meshgrid(*[np.arange(0, N, 9)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)        # 8^3 nodes all over the domain
    whole = eng.collision_field()
    boxes = {"20^3 across the surface": ((33, 24, 23), (20, 20, 20)), "the tile at the centre": ((28, 32, 32), (4, 4, 4))}
    for name, (lo, shape) in boxes.items():
        got = eng.collision_field(lo, shape)
        assert np.array_equal(bits(got), bits(whole[lo[0]:lo[0] + shape[0], lo[1]:lo[1] + shape[1], lo[2]:lo[2] + shape[2]])), name
        nodes = mm.grid_nodes(BITS, lo, shape)
        res = modelled(verts, tris, nodes)
        bad = (bits(got).reshape(-1, 4) != bits(res["out"])).any(axis=-1)
        print(f"{name}: {int(bad.sum())} of {len(nodes)} nodes differ, sdis in [{got[..., 0].min():.4f}, {got[..., 0].max():.4f}], {len(set(res['T'].tolist()))} triangles win")
        assert not bad.any(), (name, np.argwhere(bad)[:5])
        if "surface" in name:
            assert got[..., 0].min() < -2 * DX and got[..., 0].max() > 2 * DX
    # the centre tile sees every triangle as a candidate (D + 2 r reaches them all): several chunks are consumed
    c = (np.array((28, 32, 32)) + 1.5) * DX
    d = np.linalg.norm(verts.astype(np.float64) - c, axis=1)
    assert d.max() < d.min() + 2 * 2.598 * DX
    nodes = (lattice.astype(np.float32) * np.float32(DX)).astype(np.float32)
    res = modelled(verts, tris, nodes)
    got = whole[lattice[:, 0], lattice[:, 1], lattice[:, 2]]
    assert np.array_equal(bits(got), bits(res["out"]))
    assert np.abs(got[:, 0]).max() > 0.4


def test_icosphere_of_80_triangles_the_last_sweep_partly_filled(eng):
    """80 triangles, no multiple of 64: in the walk's second sweep over the triangles 16 lanes hold one and 48 hold none - in the bound they
    repeat triangle 79, in the candidate test they are excluded.  A 20^3 box of nodes across the surface against the model, bit for bit."""
    verts, tris = scenes.icosphere((0.47, 0.52, 0.55), 0.21, 1)
    assert len(tris) == 80
    eng.set_collision_mesh(verts, tris)
    lo, shape = (20, 22, 24), (20, 20, 20)
    got = eng.collision_field(lo, shape)
    nodes = mm.grid_nodes(BITS, lo, shape)
    res = modelled(verts, tris, nodes)
    bad = (bits(got).reshape(-1, 4) != bits(res["out"])).any(axis=-1)
    print(f"{int(bad.sum())} of {len(nodes)} nodes differ, sdis in [{got[..., 0].min():.4f}, {got[..., 0].max():.4f}], {len(set(res['T'].tolist()))} triangles win")
    assert not bad.any(), np.argwhere(bad)[:5]
    assert got[..., 0].min() < -2 * DX and got[..., 0].max() > 2 * DX and (res["T"] >= 64).any() and (res["T"] < 64).any()


def test_refusals_change_nothing(eng):
    verts, tris = scenes.box_mesh((0.21, 0.33, 0.27), (0.71, 0.62, 0.79))
    eng.set_collision_mesh(verts, tris, time=0.25)
    before = eng.collision_field().copy()
    api, ctx = eng.api, eng.ctx
    obj = _ffi.CollisionObject()
    api.default_collision_object(C.byref(obj))

    def install(v, f, o=obj, nv=None, nt=None, null=()):
        v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
        rc = api.set_collision_mesh(ctx, C.byref(o) if o is not None else None, None, None if "verts" in null else v.ctypes.data, len(v) if nv is None else nv,
                                    None if "tris" in null else f.ctypes.data, len(f) if nt is None else nt)
        return rc, api.last_error(ctx).decode()

    bad_type = _ffi.CollisionObject()
    api.default_collision_object(C.byref(bad_type))
    bad_type.type = 3
    flipped = tris.copy()
    flipped[4] = flipped[4, ::-1]
    nan = verts.copy()
    nan[3, 1] = np.nan
    inf = verts.copy()
    inf[5, 2] = np.inf
    far = tris.copy()
    far[7, 2] = 8
    negative = tris.copy()
    negative[0, 0] = -1
    cases = {"NULL obj": (install(verts, tris, o=None), "NULL obj"), "NULL verts": (install(verts, tris, null=("verts",)), "NULL verts or tris"),
             "NULL tris": (install(verts, tris, null=("tris",)), "NULL verts or tris"), "boundary type": (install(verts, tris, o=bad_type), "boundary type outside 0..2"),
             "three triangles": (install(verts, tris[:3]), "fewer than 4 triangles"), "too many triangles": (install(verts, tris, nt=_ffi.MESH_MAX_TRIANGLES + 1), "triangles"),
             "too many vertices": (install(verts, tris, nv=_ffi.MESH_MAX_VERTICES + 1), "vertices"), "index past nv": (install(verts, far), "index outside [0, nv)"),
             "negative index": (install(verts, negative), "index outside [0, nv)"), "NaN vertex": (install(nan, tris), "vertex 3 is not finite"),
             "inf vertex": (install(inf, tris), "vertex 5 is not finite"),
             "degenerate": (install(verts, np.concatenate([tris, [(0, 1, 1), (0, 1, 1)]])), "degenerate"), "open": (install(verts, tris[:-1]), "not a closed"),
             "flipped triangle": (install(verts, flipped), "not a closed"), "duplicated triangle": (install(verts, np.concatenate([tris, tris[:1]])), "not a closed"),
             "wound inward": (install(verts, tris[:, ::-1]), "flip the winding")}
    for name, ((rc, msg), want) in cases.items():
        assert rc == _ffi.MPM_ERR_INVALID and want in msg, (name, rc, msg)
    assert "inside_out" in cases["wound inward"][0][1]
    assert api.set_collision_mesh(None, C.byref(obj), None, verts.ctypes.data, 8, tris.ctypes.data, 12) == _ffi.MPM_ERR_INVALID
    assert np.array_equal(bits(eng.collision_field()), bits(before)), "a refused install changed the field"
    assert eng.collision_time() == 0.25 and not eng.collision_clock_running()
    with pytest.raises(EngineError):
        eng.set_collision_mesh(verts, tris[:-1])


def test_removal_reinstall_and_the_readouts_refusals(eng):
    verts, tris = mm.octahedron()
    eng.set_collision_mesh(verts, tris, time=0.5, animate=True)
    assert eng.collision_time() == 0.5 and eng.collision_clock_running()
    first = eng.collision_field((10, 20, 30), (5, 6, 7)).copy()
    api, ctx = eng.api, eng.ctx
    out = np.zeros(4 * N ** 3, dtype=np.float32)

    def read(lo, dims, dst=out):
        rc = api.get_collision_field(ctx, (C.c_int * 3)(*lo) if lo is not None else None, (C.c_int * 3)(*dims) if dims is not None else None,
                                     dst.ctypes.data if dst is not None else None)
        return rc, api.last_error(ctx).decode()

    for lo, dims, dst, want in (((0, 0, 0), (0, 1, 1), out, "dims entry < 1"), ((0, 0, 0), (1, -2, 1), out, "dims entry < 1"), ((-1, 0, 0), (2, 2, 2), out, "leaves [0, N)^3"),
                                ((60, 0, 0), (5, 1, 1), out, "leaves [0, N)^3"), ((0, 0, N), (1, 1, 1), out, "leaves [0, N)^3"), (None, (1, 1, 1), out, "NULL"),
                                ((0, 0, 0), None, out, "NULL"), ((0, 0, 0), (1, 1, 1), None, "NULL")):
        rc, msg = read(lo, dims, dst)
        assert rc == _ffi.MPM_ERR_INVALID and want in msg, (lo, dims, rc, msg)
    assert read((60, 0, 0), (4, 64, 64))[0] == _ffi.MPM_OK
    # a mesh install replaces a host-array install and the other way round; the readout serves both
    sdf, grad = scenes.sphere_level_set(BITS, (0.5, 0.34, 0.5), 6 * DX)
    eng.set_collision_object(sdf, grad)
    assert not eng.collision_clock_running()
    f = eng.collision_field()
    assert np.array_equal(bits(f[..., 0]), bits(sdf)) and np.array_equal(bits(np.moveaxis(f[..., 1:], -1, 0)), bits(grad))
    eng.set_collision_mesh(verts, tris)
    assert np.array_equal(bits(eng.collision_field((10, 20, 30), (5, 6, 7))), bits(first))
    eng.set_collision_object()                                                                      # removal
    rc, msg = read((0, 0, 0), (1, 1, 1))
    assert rc == _ffi.MPM_ERR_INVALID and "no level-set collision object" in msg
    with pytest.raises(EngineError):
        eng.collision_time()
    eng.set_collision_mesh(verts, tris)
    assert np.array_equal(bits(eng.collision_field((10, 20, 30), (5, 6, 7))), bits(first))


STEPS = 40


def test_mesh_object_equals_the_level_set_object_of_its_own_field():
    """scenes.sphere_on_obstacle_mesh for 40 substeps with the clock running and a translating, rotating object, against a second context on
    which the field read back from the first (mpm_get_collision_field, split into sdf / grad) is installed through mpm_set_collision_object:
    positions and mpm_dump_grid bit for bit.  The thrown body is the scene's 2 x 2 x 2-cell block (64 particles inside one particle block): on
    a dense sphere two runs of ONE configuration already differ in the last bits (float atomics of P2G), and there would be nothing to compare."""
    motion = dict(trans_vel=(0.3, 0.2, 0.0), omega=(0.0, 0.0, 2.0), animate=True)
    sc = scenes.sphere_on_obstacle_mesh(bits=BITS, speed=2.0, body_cells=(2, 2, 2), **motion)
    probe = build_engine(sc)
    field = probe.collision_field()
    probe.close()
    col = {k: v for k, v in sc["collision_mesh"].items() if k not in ("vertices", "faces")}
    level = {k: v for k, v in sc.items() if k != "collision_mesh"}
    level["collision"] = dict(col, sdf=field[..., 0].copy(), grad=np.ascontiguousarray(np.moveaxis(field[..., 1:], -1, 0)))
    free = {k: v for k, v in sc.items() if k != "collision_mesh"}
    out = {}
    for name, s in (("mesh", sc), ("mesh again", sc), ("level set", level), ("free", free)):
        e = build_engine(s)
        e.initial_setup()
        e.run_fixed(STEPS, s["dt"])
        keys, blocks = e.dump_grid()
        order = np.lexsort(keys.T[::-1])
        x = e.retrieve_positions(0)
        assert len(x) == 64 and e.diagnostics().lost_particles == 0
        out[name] = sorted_rows(x), keys[order], bits(blocks[order]), (e.collision_time(), e.collision_clock_running()) if name != "free" else None
        e.close()
    assert all(np.array_equal(a, b) for a, b in zip(out["mesh"][:3], out["mesh again"][:3])), "the scene is not deterministic: nothing to compare"
    for k in range(3):
        assert np.array_equal(out["mesh"][k], out["level set"][k]), k
    assert out["mesh"][3] == out["level set"][3] and out["mesh"][3][1] and out["mesh"][3][0] > 0.9 * STEPS * sc["dt"]
    assert not np.array_equal(out["mesh"][0], out["free"][0]), "the obstacle touched nothing"


def test_the_engines_own_isosurface_installs():
    """Engine.isosurface(weld=True) of a small resting block is closed and outward by construction: it installs, and the sign of the field agrees
    with mass > iso_mass at every node farther than one cell from the surface."""
    e = Engine(domain_bits=BITS, max_ppc=128, gravity=0.0)
    lo, hi = (24, 26, 22), (34, 33, 36)
    prm = {"volume": scenes._vol(BITS), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    e.init_model(_ffi.FIXED_COROTATED, scenes.lattice_box(BITS, lo, hi), (0.0, 0.0, 0.0), **prm)
    e.initial_setup()
    iso = np.float32(500.0 * DX ** 3)
    V, F = e.isosurface(iso_mass=float(iso))
    mass = e.grid_volume()[0]
    assert mm.validate(V, F)[0] == "ok"
    e.set_collision_mesh(V, F)
    f = e.collision_field()
    e.close()
    far = np.abs(f[..., 0]) > DX
    inside = mass > iso
    print(f"{len(F)} triangles; {int(far.sum())} nodes farther than a cell, {int((inside & far).sum())} of them inside")
    assert (inside & far).sum() > 100 and (~inside & far).sum() > 100000
    assert np.array_equal(f[..., 0][far] < 0, inside[far])
    assert np.allclose(np.linalg.norm(f[..., 1:].astype(np.float64), axis=-1), 1.0, atol=1e-5)


def test_gmpm_collision_mesh_scene_equals_the_engine(tmp_path):
    """The "collision_mesh" key of the gmpm driver on a written OBJ file (a box in cell units, scaled and offset under the first body of
    tests/test_gmpm_stress_gpu.py's two single-block bodies, on which the engine is deterministic), three frames: frame 0 holds the sampled
    particles, and every later frame equals, bit for bit, the Python engine's with the same mesh."""
    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS as GB, DT_DEFAULT, FC, FPS, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    frames = 3
    v, f = scenes.box_mesh((0.0, 0.0, 0.0), (8.0, 4.25, 7.0))
    scale, offset = 1.0 / 64, (4.0 / 64, 14.0 / 64, 16.0 / 64)
    mm.write_obj(str(tmp_path / "body.obj"), v, f)
    mesh = {"file": "body.obj", "type": "slip", "friction": 0.2, "scale": scale, "offset": list(offset)}
    sim = {"gpuid": 0, "fps": FPS, "frames": frames, "default_dt": DT_DEFAULT, "domain_bits": GB, "output_dir": str(tmp_path)}
    (tmp_path / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "collision_mesh": mesh}))
    log = subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(tmp_path / "scene.json")], text=True, timeout=300)
    assert "has a collision mesh of 12 triangles" in log
    start = [read_bgeo_attrs(frame(tmp_path, m, 0))[0] for m in range(len(MODELS))]
    placed = (v * np.float32(scale) + np.asarray(offset, dtype=np.float32)).astype(np.float32)

    def drive(with_mesh):
        models = []
        for mod, xyz in zip(MODELS, start):
            mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
            models.append({"material": mat, "xyz": xyz, "v0": mod["velocity"], "params": ({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {})})
        sc = {"bits": GB, "config": {"max_ppc": 128}, "models": models}
        if with_mesh:
            sc["collision_mesh"] = {"vertices": placed, "faces": f, "type": 1, "friction": 0.2}
        e = build_engine(sc)
        spf = np.float32(1.0) / np.float32(FPS)
        max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in MODELS)
        dt = e.compute_dt(max_v0, 0.0, float(spf), DT_DEFAULT)
        e.initial_setup()
        res = []
        for _ in range(frames):
            t = np.float32(0.0)
            while t < spf:
                next_dt, _ = e.substep(dt, float(t), float(spf), DT_DEFAULT)
                t = np.float32(t + np.float32(dt))
                dt = next_dt
            res.append([sorted_rows(e.retrieve_positions(m)) for m in range(len(MODELS))])
        e.close()
        return res

    want, free = drive(True), drive(False)
    for fr in range(1, frames + 1):
        for m in range(len(MODELS)):
            got = sorted_rows(read_bgeo_attrs(frame(tmp_path, m, fr))[0])
            assert np.array_equal(got, want[fr - 1][m]), (fr, m)
    assert not np.array_equal(want[-1][0], free[-1][0]), "the mesh touched nothing"

"""Per-particle initial conditions without a GPU: the two entry points' surface (header, export, _ffi), the float64 set-up model of
tests/particle_init_model.py against the uniform-v0 model it generalises and against a linear field, and the index option of the scene
splitters."""
import os
import re
import subprocess

import numpy as np

import face_scenes as fs
import particle_init_model as pim
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine

ROOT = _ffi.repo_root()


def test_library_exports_the_two_entry_points_and_header_declares_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    for sym in ("mpm_add_model_particles", "mpm_set_model_velocity_field"):
        assert re.search(r"\bT %s$" % sym, out, re.M), sym + " is not exported"
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert "typedef struct mpm_particle_init {" in hdr and "} mpm_particle_init;" in hdr
    assert re.search(r"int mpm_add_model_particles\(mpm_ctx\* ctx, int material, const mpm_material_params\* params, const float\* xyz, size_t n, const float v0\[3\],\s*"
                     r"const mpm_particle_init\* init /\* NULL == mpm_add_model \*/, int\* model_id\);", hdr)
    assert "int mpm_set_model_velocity_field(mpm_ctx* ctx, int model, const float v0[3], const float grad9[9] /* column-major */, const float pivot[3]);" in hdr
    assert "affine9[9*i + 3*c + r] = C_rc" in hdr.split("typedef struct mpm_particle_init {")[1].split("} mpm_particle_init;")[0], "the header names the affine layout"
    for name, nargs in (("add_model_particles", 8), ("set_model_velocity_field", 5)):
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES          # (the oracle stays as it is)
        fn = getattr(_ffi.load_hip(), name)
        assert fn.restype is _ffi.C.c_int and len(fn.argtypes) == nargs
    assert _ffi.C.sizeof(_ffi.ParticleInit) == 4 * _ffi.C.sizeof(_ffi.C.c_void_p) + 16
    assert callable(Engine.set_model_velocity_field) and callable(Engine.snapshot_models)
    assert _ffi.load_hip().build_info().decode().startswith("claymore_hip abi7 ")


def test_model_with_a_constant_velocity_is_the_uniform_model():
    sc = fs.setup_slab_scene()
    want, want_out = fs.reference_setup_grid(sc)
    m = sc["models"][0]
    n = m["xyz"].shape[0]
    per = dict(sc, models=[dict(m, v0=(9.0, 9.0, 9.0), velocity=np.tile(np.float32(m["v0"]), (n, 1)), affine=np.zeros((n, 3, 3), np.float32))])
    for scene in (sc, per):
        got, got_out = pim.setup_grid(scene)
        massed = {k: v for k, v in want.items() if v[0] > 0}
        assert set(got) == set(massed)
        for k, v in massed.items():
            assert np.array_equal(got[k], v), (k, got[k], v)
        assert got_out == want_out


def test_a_linear_field_is_reproduced_at_every_massed_node():
    rng = np.random.default_rng(7)
    a, A = rng.uniform(-2, 2, 3), rng.uniform(-50, 50, (3, 3))
    sc = fs.setup_slab_scene()
    m = sc["models"][0]
    x = m["xyz"].astype(np.float64)
    v = a[None, :] + x @ A.T                                            # float64 arrays: the model takes them as they are
    per = dict(sc, models=[dict(m, velocity=v, affine=np.broadcast_to(A, (x.shape[0], 3, 3)))])
    g = pim.setup_nodes(per)
    xi = g["nodes"] / float(1 << sc["bits"])
    want = a[None, :] + xi @ A.T
    got = g["val"][:, 1:] / g["val"][:, :1]
    assert g["nodes"].shape[0] > 1000
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    # and the same through the model's own field form
    fld = dict(sc, models=[dict(m, v0=tuple(a), velocity_gradient=A.ravel().tolist(), pivot=(0.0, 0.0, 0.0))])
    g2 = pim.setup_nodes(fld)
    assert np.array_equal(g2["nodes"], g["nodes"]) and np.abs(g2["val"] - g["val"]).max() <= 1e-12 * np.abs(g["val"]).max()
    # with the affine term dropped the field is NOT reproduced: the check above can tell
    g3 = pim.setup_nodes(dict(sc, models=[dict(m, velocity=v)]))
    assert np.abs(g3["val"][:, 1:] / g3["val"][:, :1] - want).max() > 1e-3


def test_split_slabs_returns_indices_that_reproduce_the_parts():
    rng = np.random.default_rng(3)
    lattice = scenes.lattice_sphere(6, (0.5, 0.5, 0.5), 6.0)
    shuffled = lattice[rng.permutation(lattice.shape[0])]
    for xyz in (lattice, shuffled):
        for kw in (dict(parts=3, axis=0), dict(parts=2, axis=1, block=scenes.block_faces(6)), dict(parts=4, axis=2)):
            plain = scenes.split_slabs(xyz, **kw)
            parts, index = scenes.split_slabs(xyz, return_index=True, **kw)
            assert isinstance(plain, list) and len(plain) == len(parts) == len(index) == kw["parts"]
            for a, b, idx in zip(plain, parts, index):
                assert np.array_equal(a, b) and np.array_equal(xyz[idx], b)
            assert np.array_equal(np.sort(np.concatenate(index)), np.arange(xyz.shape[0]))
        plain = scenes.split_boxes(xyz, (2, 1, 2), block=scenes.block_faces(6))
        parts, index = scenes.split_boxes(xyz, (2, 1, 2), block=scenes.block_faces(6), return_index=True)
        assert len(plain) == len(parts) == 4
        for a, b, idx in zip(plain, parts, index):
            assert np.array_equal(a, b) and np.array_equal(xyz[idx], b)
        assert np.array_equal(np.sort(np.concatenate(index)), np.arange(xyz.shape[0]))


def test_new_scenes_carry_a_velocity_field():
    for sc in (scenes.spinning_ball(), scenes.sheared_block()):
        m = sc["models"][0]
        a, A = scenes.model_velocity_field(m)
        assert sc["config"]["gravity"] == 0.0 and np.abs(A).max() > 0
        c = np.asarray(m["pivot"])
        assert np.allclose(a + A @ c, m["v0"])
        x = m["xyz"].astype(np.float64)
        assert np.abs(x.mean(axis=0) - c).max() < 1e-9, "the pivot is the body's centre"
    assert np.allclose(scenes.model_velocity_field(scenes.spinning_ball(omega=(0, 0, 2.0))["models"][0])[1] @ [1.0, 0.0, 0.0], [0.0, 2.0, 0.0])
    assert scenes.model_velocity_field(scenes.two_spheres(bits=5)["models"][0]) is None


def test_host_selftest_parses_a_model_with_a_velocity_field(tmp_path):
    exe = tmp_path / "host_selftest"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", str(exe), os.path.join(ROOT, "claymore_amd", "host", "host_selftest.cpp")])

    def run(model):
        out = subprocess.check_output([str(exe), "--model-field", model], text=True).split()
        return out[0], np.array([float(x) for x in out[1:]])

    kind, f = run('{"velocity": [1, 0, 0], "omega": [0, 0, 2], "pivot": [0.5, 0.5, 0.5]}')
    assert kind == "field" and np.array_equal(f[:3], [1, 0, 0]) and np.array_equal(f[12:15], [0.5, 0.5, 0.5])
    G = f[3:12].reshape(3, 3).T                                           # column-major -> G[r, c]
    assert np.array_equal(G, [[0, -2, 0], [2, 0, 0], [0, 0, 0]])
    assert np.allclose(f[15:18], np.array([1, 0, 0]) + np.cross([0, 0, 2], np.array([1, 2, 3]) - 0.5))
    kind, f = run('{"velocity": [0, 0, 0], "velocity_gradient": [0, 1, 2, 3, 4, 5, 6, 7, 8]}')
    assert kind == "field" and np.array_equal(f[3:12].reshape(3, 3).T, np.arange(9).reshape(3, 3))       # row-major in the file
    kind, f = run('{"velocity": [1, 2, 3]}')
    assert kind == "none" and np.array_equal(f[:3], [1, 2, 3]) and not f[3:12].any()
    assert subprocess.run([str(exe), "--model-field", '{"velocity": [0, 0, 0], "velocity_gradient": [1, 2]}'], capture_output=True).returncode == 1

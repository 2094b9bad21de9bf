"""Per-particle velocity output (mpm_retrieve_velocity, claymore_amd/csrc/mpm_readout.hpp) on the GPU.  The reference has no velocity readout
and neither has the oracle: the expected values are computed here in float64 from a dumped grid (HIP's own, or the oracle's) at the
returned positions, with G2P's stencil, weights, tie rule and face rule (gather64)."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

import face_scenes as F
from claymore_amd import _ffi, scenes
from claymore_amd.engine import build_engine
from oracle_ffi import oracle_api
from parity_util import match

pytestmark = pytest.mark.gpu
V0 = (0.3, -0.7, 1.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------------------
def node_velocities(keys, blocks, bits):
    """Dense (n + 8)^3 x 3 node velocity array of a dumped grid: p / m where m > 0, zero elsewhere - and zero for every node of a block
    that is not in the dump and for nodes at or beyond n (the padding)."""
    n = 1 << bits
    V = np.zeros((n + 8, n + 8, n + 8, 3))
    cell = np.arange(64)
    cx, cy, cz = cell >> 4, (cell >> 2) & 3, cell & 3
    for key, blk in zip(keys, blocks):
        m = blk[0].astype(np.float64)
        v = np.where(m > 0, blk[1:].astype(np.float64) / np.where(m > 0, m, 1.0), 0.0)      # (3, 64)
        V[4 * key[0] + cx, 4 * key[1] + cy, 4 * key[2] + cz] = v.T
    return V


def gather64(xyz, V, bits):
    """(v_p, C_p) of particles at world positions xyz from node velocities V: base node N - 1 with N = lround(x / dx) (ties away from zero),
    B-spline weights of x / dx - base, the stencil placed in the particle block's node cube as G2P places it - cube base ((base - 1) & 3) + 1
    from the block's first node 4 * ((N - 2) / 4) (truncating), which wraps the stencils of cells -2 / -1 -; C = 4 / dx^2 sum w v (x_i - x_p)^T."""
    n = 1 << bits
    p = xyz.astype(np.float64) * n
    N, base, key, _ = F.kernel_axis(xyz.astype(np.float32) * np.float32(n))
    fd = p - base
    w = F.bspline64(fd)                                         # (P, 3 axes, 3 nodes)
    n0 = 4 * key + ((base - 1) & 3) + 1                         # (P, 3)
    v = np.zeros((xyz.shape[0], 3))
    A = np.zeros((xyz.shape[0], 3, 3))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                W = w[:, 0, i] * w[:, 1, j] * w[:, 2, k]
                vi = V[n0[:, 0] + i, n0[:, 1] + j, n0[:, 2] + k]
                r = np.array([i, j, k], dtype=np.float64)[None, :] - fd
                v += W[:, None] * vi
                A += (W[:, None] * vi)[:, :, None] * r[:, None, :]
    return v, 4.0 * n * A                                       # (A in cells: C = D^-1 A dx = 4 / dx * A)


def sort_rows(*arrs):
    key = np.concatenate([np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1) for a in arrs], axis=1)
    order = np.lexsort(key.T[::-1])
    return [a[order] for a in arrs]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------
def four_material_bodies(bits=6, v0=V0):
    """One sphere per material, well inside the domain and apart, all with the same initial velocity."""
    n = 1 << bits
    models = []
    for mat, c in zip(range(4), ((0.3, 0.3, 0.3), (0.7, 0.3, 0.3), (0.3, 0.7, 0.7), (0.7, 0.7, 0.5))):
        prm = {"volume": scenes._vol(bits), "rho": 1e3} if mat in (_ffi.J_FLUID, _ffi.FIXED_COROTATED, _ffi.NACC) else {}
        models.append({"material": mat, "xyz": scenes.lattice_sphere(bits, c, 0.08 * n), "v0": tuple(v0), "params": prm})
    return {"name": "four_bodies", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128}, "models": models}


IMPACTS = {
    # four materials against the three lower faces: sand and J-fluid yield there, particles in the wall zone and in cells -2 / -1
    "lower_faces": lambda: F.lower_face_materials_scene(5),
    # a body in the x = 0 wall zone (from cell -2) falling onto a level-set sphere in the x = 0 / y = 0 edge
    "collision_object": lambda: F.corner_obstacle_scene(5, "slip"),
}


def readout_all(eng, nmodels):
    return [eng.retrieve_velocity(m, affine=True) for m in range(nmodels)]


# ---- uniform fields ---------------------------------------------------------------------------------------------------------------------------------
def test_uniform_translation_after_setup_all_materials():
    """After set-up every node holds m v0 / m: v_p = v0 to rounding (sum w = 1), C_p = 0 to rounding (APIC keeps affine fields)."""
    sc = four_material_bodies()
    eng = build_engine(sc)
    eng.initial_setup()
    v0 = np.array(V0)
    dx = 1.0 / (1 << sc["bits"])
    for m, mod in enumerate(sc["models"]):
        xyz, v, Cm = eng.retrieve_velocity(m, affine=True)
        assert xyz.shape == (mod["xyz"].shape[0], 3) and v.shape == xyz.shape and Cm.shape == (xyz.shape[0], 3, 3)
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(Cm))
        err = np.linalg.norm(v.astype(np.float64) - v0, axis=1).max()
        assert err <= 1e-6 * np.linalg.norm(v0), (m, err)
        assert np.abs(Cm).max() <= 1e-5 * np.linalg.norm(v0) / dx, (m, np.abs(Cm).max())
        xs = eng.retrieve_positions(m)
        a, b = sort_rows(xyz)[0], sort_rows(xs)[0]
        assert np.array_equal(a, b)                              # the same particle set as retrieve_positions
    eng.close()


@pytest.mark.parametrize("driver", ["run_fixed", "substep"])
def test_free_fall(driver):
    """20 fixed substeps of bodies far from every wall: each grid update adds g dt, so v_p = v0 + (0, 20 g dt, 0); the kinetic energy is
    1/2 M |v|^2."""
    sc = four_material_bodies()
    eng = build_engine(sc)
    eng.initial_setup()
    dt, steps = 1e-4, 20
    if driver == "run_fixed":
        eng.run_fixed(steps, dt)
    else:
        t = 0.0
        for _ in range(steps):
            eng.substep(dt, t, 1.0, dt)
            t += dt
    want = np.array(V0, dtype=np.float64) + np.array([0.0, steps * dt * float(np.float32(eng.cfg.gravity)), 0.0])
    mass_total = 0.0
    for m in range(len(sc["models"])):
        _, v = eng.retrieve_velocity(m)
        err = np.abs(v.astype(np.float64) - want).max()
        assert err <= 2e-6 * np.linalg.norm(want), (m, err)
        mass_total += eng.model_mass(m) * v.shape[0]
    ke = eng.kinetic_energy()
    ke_want = 0.5 * mass_total * float(want @ want)
    assert abs(ke - ke_want) <= 1e-5 * ke_want, (ke, ke_want)
    assert abs(eng.kinetic_energy(0) - 0.5 * eng.model_mass(0) * sc["models"][0]["xyz"].shape[0] * float(want @ want)) <= 1e-5 * ke_want
    eng.close()


# ---- against a float64 gather ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", sorted(IMPACTS))
def test_against_a_float64_gather_of_the_own_grid(scene):
    """Impacts at the domain's faces (tests/face_scenes.py), 50 substeps: v_p and C_p against the float64 gather from mpm_dump_grid at the
    returned positions.  Runs with whichever G2P2G layout the process uses (test_both_list_layouts forces each)."""
    sc = IMPACTS[scene]()
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(50, sc["dt"])
    out = readout_all(eng, len(sc["models"]))
    cnt = eng.counts()
    assert [o[0].shape[0] for o in out] == [cnt.particles[m] for m in range(len(out))]     # every bucketed particle, once
    keys, blocks = eng.dump_grid()
    V = node_velocities(keys, blocks, sc["bits"])
    xs_all, vs_all, vr_all, cs_all, cr_all = [], [], [], [], []
    wall_or_wrapped = 0
    for xyz, v, Cm in out:
        vr, cr = gather64(xyz, V, sc["bits"])
        xs_all.append(xyz), vs_all.append(v), vr_all.append(vr), cs_all.append(Cm), cr_all.append(cr)
        cells = np.floor(xyz.astype(np.float64) * (1 << sc["bits"]))
        wall_or_wrapped += int(np.sum(np.any(cells < 8, axis=1)))
    vs, vr, cs, cr = (np.concatenate(a) for a in (vs_all, vr_all, cs_all, cr_all))
    assert wall_or_wrapped > 100                               # the scene does put particles in the wall zone
    vmax, cmax = np.abs(vr).max(), np.abs(cr).max()
    assert vmax > 0.01 and cmax > 0.0                          # (the wall zone's slip walls stop the lower-face bodies: |v| ~ 0.05)
    dv = np.abs(vs - vr).max()
    dc = np.abs(cs - cr).max()
    print(f"{scene}: max |dv| {dv:.3g} of max |v| {vmax:.3g}, max |dC| {dc:.3g} of max |C| {cmax:.3g}")
    assert dv <= 2e-6 * vmax, (dv, vmax)
    assert dc <= 2e-6 * cmax, (dc, cmax)
    eng.close()


def test_wrapped_stencil_of_cells_minus_two_and_minus_one():
    """Particles of cells -2 / -1 right after set-up: the readout uses G2P's wrapped cube base, not the particle's true stencil."""
    bits = 5
    xyz = F.to_world(F.face_box_cells(bits, 1, "lo", depth=8, width=8), bits)
    sc = {"name": "floor_box", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128},
          "models": [{"material": _ffi.FIXED_COROTATED, "xyz": xyz, "v0": (0.25, -1.0, 0.5), "params": {"volume": scenes._vol(bits), "rho": 1e3}}]}
    eng = build_engine(sc)
    eng.initial_setup()
    x, v, Cm = eng.retrieve_velocity(0, affine=True)
    keys, blocks = eng.dump_grid()
    vr, cr = gather64(x, node_velocities(keys, blocks, bits), bits)
    low = np.floor(x[:, 1].astype(np.float64) * (1 << bits)) < 1
    assert low.sum() >= 64
    assert np.abs(v - vr).max() <= 2e-6 * np.abs(vr).max()
    assert np.abs(Cm - cr).max() <= 2e-6 * max(np.abs(cr).max(), 1.0)
    eng.close()


@pytest.mark.parametrize("scene", sorted(IMPACTS))
def test_against_the_oracle(scene):
    """The HIP readout against the float64 gather from the ORACLE's grid at the oracle's positions, particles matched by position: 1e-5 of the
    largest |v| for every body but the sand body yielding against z = 0 in "lower_faces".  There the two engines' GRIDS already differ by more
    (tests/test_domain_faces_gpu.py: 1.3e-4 node by node after 40 substeps, the rounding amplification of sand's return mapping), so the readout
    is held to 1e-5 beyond what the same float64 gather from HIP's own grid at the same positions deviates: it adds no error of its own."""
    sc = IMPACTS[scene]()
    nm = len(sc["models"])
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(50, sc["dt"])
    hip = readout_all(eng, nm)
    Vh = node_velocities(*eng.dump_grid(), sc["bits"])
    eng.close()
    ora = build_engine(sc, api=oracle_api())
    ora.initial_setup()
    ora.run_fixed(50, sc["dt"])
    xo = [ora.retrieve_positions(m) for m in range(nm)]
    ko, bo = ora.dump_grid()
    ora.close()
    V = node_velocities(ko, bo, sc["bits"])
    res = []
    for (xh, vh, _), x in zip(hip, xo):
        assert xh.shape == x.shape
        idx, _ = match(x.astype(np.float64), xh.astype(np.float64))
        vr, _ = gather64(x, V, sc["bits"])
        vg, _ = gather64(x, Vh, sc["bits"])
        res.append((float(np.abs(vh[idx] - vr).max()), float(np.abs(vg - vr).max()), float(np.abs(vr).max())))
    vmax = max(r[2] for r in res)
    for m, (dv, dgrid, _) in enumerate(res):
        print(f"{scene} vs oracle, model {m}: max |dv| {dv:.3g}, grids alone {dgrid:.3g}, of max |v| {vmax:.3g}")
        if scene == "lower_faces" and sc["models"][m]["material"] == _ffi.SAND:
            assert dv <= dgrid + 1e-5 * vmax, (m, dv, dgrid, vmax)
        else:
            assert dv <= 1e-5 * vmax, (m, dv, vmax)


@pytest.mark.parametrize("mask", ["0", "0xF"])
def test_both_list_layouts(mask):
    """test_against_a_float64_gather_of_the_own_grid with the G2P2G kernel forced per process (MPM_G2P2G_PAIRS, read once by the library):
    the sliced list layout with its holes ("0") and the pair layout ("0xF")."""
    env = dict(os.environ, MPM_G2P2G_PAIRS=mask)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_against_a_float64_gather_of_the_own_grid"], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and "2 passed" in tail and "failed" not in tail, (mask, tail, r.stderr[-1500:])


# ---- consistency ----------------------------------------------------------------------------------------------------------------------------------------
def test_consistency_with_retrieve_state_repeat_and_checkpoint():
    sc = IMPACTS["lower_faces"]()
    nm = len(sc["models"])
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(30, sc["dt"])
    first = readout_all(eng, nm)
    for m, (x, v, Cm) in enumerate(first):
        xs, _, _ = eng.retrieve_state(m)
        assert np.array_equal(sort_rows(x)[0], sort_rows(xs)[0])              # the same positions, as a set
        x2, v2, C2 = eng.retrieve_velocity(m, affine=True)
        a, b = sort_rows(x, v, Cm.reshape(-1, 9)), sort_rows(x2, v2, C2.reshape(-1, 9))
        assert all(np.array_equal(p, q) for p, q in zip(a, b))               # the same (x, v, C) triples, as a set
        x3, v3 = eng.retrieve_velocity(m)                                      # affine=False: the same (x, v) pairs
        assert all(np.array_equal(p, q) for p, q in zip(sort_rows(x, v), sort_rows(x3, v3)))
    buf = eng.save_checkpoint()
    eng.run_fixed(5, sc["dt"])
    eng.load_checkpoint(buf)
    for (x, v, Cm), (x2, v2, C2) in zip(first, readout_all(eng, nm)):
        a, b = sort_rows(x, v, Cm.reshape(-1, 9)), sort_rows(x2, v2, C2.reshape(-1, 9))
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
    eng.close()


def test_error_codes():
    sc = four_material_bodies(bits=6)
    eng = build_engine(sc)
    api, ctx = eng.api, eng.ctx
    n0 = sc["models"][0]["xyz"].shape[0]
    xyz = np.empty((n0, 3), np.float32)
    vel = np.empty((n0, 3), np.float32)
    aff = np.empty((n0, 9), np.float32)
    pX, pV, pA = (a.ctypes.data_as(C.c_void_p) for a in (xyz, vel, aff))
    n = C.c_size_t(n0)
    assert api.retrieve_velocity(ctx, 0, pX, pV, pA, C.byref(n)) == _ffi.MPM_ERR_NOT_READY       # before set-up
    eng.initial_setup()
    for bad in (-1, 4):
        n = C.c_size_t(n0)
        assert api.retrieve_velocity(ctx, bad, pX, pV, pA, C.byref(n)) == _ffi.MPM_ERR_INVALID
    n = C.c_size_t(n0)
    assert api.retrieve_velocity(ctx, 0, None, pV, pA, C.byref(n)) == _ffi.MPM_ERR_INVALID
    assert api.retrieve_velocity(ctx, 0, pX, None, pA, C.byref(n)) == _ffi.MPM_ERR_INVALID
    assert api.retrieve_velocity(ctx, 0, pX, pV, pA, None) == _ffi.MPM_ERR_INVALID
    n = C.c_size_t(10)
    assert api.retrieve_velocity(ctx, 0, pX, pV, pA, C.byref(n)) == _ffi.MPM_ERR_CAPACITY
    assert n.value == 10
    assert np.all(np.isfinite(vel[:10])) and np.abs(vel[:10].astype(np.float64) - np.array(V0)).max() <= 1e-6 * np.linalg.norm(V0)
    n = C.c_size_t(n0)
    assert api.retrieve_velocity(ctx, 0, pX, pV, None, C.byref(n)) == _ffi.MPM_OK and n.value == n0       # affine9 may be NULL
    # a context inside an in-process group: refused while the group exists
    other = build_engine(sc)
    other.initial_setup()
    ctxs = (C.c_void_p * 2)(eng.ctx.value, other.ctx.value)
    groups = (C.c_void_p * 2)()
    assert api.group_create_local(ctxs, 2, groups) == _ffi.MPM_OK
    try:
        n = C.c_size_t(n0)
        assert api.retrieve_velocity(ctx, 0, pX, pV, pA, C.byref(n)) == _ffi.MPM_ERR_INVALID
        assert "group" in api.last_error(ctx).decode()
    finally:
        for g in groups:
            api.group_destroy(g)
    n = C.c_size_t(n0)
    assert api.retrieve_velocity(ctx, 0, pX, pV, pA, C.byref(n)) == _ffi.MPM_OK      # (no group substep ran: its grid is whole again)
    other.close()
    eng.close()


def test_refused_while_the_grid_holds_velocities():
    """The phase-level calls: mpm_grid_update turns grid[0]'s momenta into velocities in place, and they stay there through mpm_g2p2g until
    mpm_rebuild_partition carries the next P2G over.  In between the readout is refused (a gather of v_i / m_i would be off by the node mass);
    a checkpoint saved in that state says so, and one saved after the rebuild reads out as before."""
    sc = four_material_bodies()
    eng = build_engine(sc)
    eng.initial_setup()
    api, ctx = eng.api, eng.ctx
    n0 = sc["models"][0]["xyz"].shape[0]
    xyz, vel = np.empty((n0, 3), np.float32), np.empty((n0, 3), np.float32)

    def call():
        n = C.c_size_t(n0)
        return api.retrieve_velocity(ctx, 0, xyz.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p), None, C.byref(n))

    dt = 1e-4
    assert call() == _ffi.MPM_OK
    eng.grid_update(dt)
    assert call() == _ffi.MPM_ERR_INVALID
    assert "holds velocities" in api.last_error(ctx).decode()
    mid = eng.save_checkpoint()                               # (allowed: a checkpoint may be taken between the phases)
    eng.g2p2g(dt, dt)
    assert call() == _ffi.MPM_ERR_INVALID
    eng.rebuild_partition()
    assert call() == _ffi.MPM_OK
    want = np.array(V0) + np.array([0.0, dt * float(np.float32(eng.cfg.gravity)), 0.0])
    assert np.abs(vel.astype(np.float64) - want).max() <= 2e-6 * np.linalg.norm(want)
    done = eng.save_checkpoint()
    eng.load_checkpoint(mid)
    assert call() == _ffi.MPM_ERR_INVALID                     # the grid of `mid` holds velocities
    eng.g2p2g(dt, dt)
    eng.rebuild_partition()
    assert call() == _ffi.MPM_OK
    assert np.abs(vel.astype(np.float64) - want).max() <= 2e-6 * np.linalg.norm(want)
    eng.load_checkpoint(done)
    assert call() == _ffi.MPM_OK
    eng.run_fixed(3, dt)                                      # (every whole-substep driver ends with momenta in the grid)
    assert call() == _ffi.MPM_OK
    eng.close()


# ---- the state readout (readout_kernel<kReadState>: the same list walk and slot rule, no grid) ----------------------------------------------------
STATE_SCENES = {"sand": _ffi.SAND, "fluid": _ffi.J_FLUID}


@pytest.mark.parametrize("material", sorted(STATE_SCENES))
def test_retrieve_state_whatever_the_grid_holds_and_with_short_arrays(material):
    """mpm_retrieve_state reads records and rows only.  Taken right after mpm_grid_update (grid[0] holds velocities) it equals, as a matched set,
    the readout after the rebuild of a substep of dt = 0 (x += v * 0: no particle moves; the rebuild re-sorts the lists).  With an output array
    of n // 3 it returns MPM_ERR_CAPACITY and n // 3 distinct particles of the full readout.  Runs with whichever G2P2G layout the process uses
    (test_retrieve_state_in_both_list_layouts forces each)."""
    sc = F.wall_zone_scene(5, "out", material=STATE_SCENES[material])
    nm = len(sc["models"])
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(20, sc["dt"])
    eng.grid_update(sc["dt"])
    before = [eng.retrieve_state(m) for m in range(nm)]
    eng.g2p2g(0.0, sc["dt"])
    eng.rebuild_partition()
    after = [eng.retrieve_state(m) for m in range(nm)]
    for (xa, sa, la), (xb, sb, lb) in zip(before, after):
        assert xa.shape == xb.shape and xa.shape[0] > 100
        idx, d = match(xa.astype(np.float64), xb.astype(np.float64))
        assert d.max() <= 1e-6, d.max()
        assert np.abs(sb[idx].astype(np.float64) - sa).max() <= 1e-5 * max(1.0, float(np.abs(sa).max()))
        assert np.abs(lb[idx].astype(np.float64) - la).max() <= 1e-5
    api, ctx = eng.api, eng.ctx
    for m, (x, st, lj) in enumerate(after):
        k = x.shape[0] // 3
        xs, ss, ls = np.full((k, 3), np.nan, np.float32), np.full((k, 9), np.nan, np.float32), np.full(k, np.nan, np.float32)
        n = C.c_size_t(k)
        assert api.retrieve_state(ctx, m, *(a.ctypes.data_as(C.c_void_p) for a in (xs, ss, ls)), C.byref(n)) == _ffi.MPM_ERR_CAPACITY
        assert n.value == k
        idx, d = match(xs.astype(np.float64), x.astype(np.float64))     # (asserts k distinct particles)
        assert d.max() == 0.0
        assert np.array_equal(ss, st[idx]) and np.array_equal(ls, lj[idx])
    eng.close()


@pytest.mark.parametrize("mask", ["0", "0xF"])
def test_retrieve_state_in_both_list_layouts(mask):
    """test_retrieve_state_whatever_the_grid_holds_and_with_short_arrays with the G2P2G kernel forced per process, as test_both_list_layouts."""
    env = dict(os.environ, MPM_G2P2G_PAIRS=mask)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_retrieve_state_whatever_the_grid_holds"], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and "2 passed" in tail and "failed" not in tail, (mask, tail, r.stderr[-1500:])


# ---- the gmpm driver's frames -------------------------------------------------------------------------------------------------------------------------
def _read_bgeo_any(path):
    raw = open(path, "rb").read()
    npoints = struct.unpack(">I", raw[9:13])[0]
    nattr = struct.unpack(">7I", raw[13:41])[3]
    if nattr == 0:
        assert len(raw) == 41 + 16 * npoints + 2
        return np.frombuffer(raw[41:41 + 16 * npoints], dtype=">f4").reshape(npoints, 4)[:, :3].astype(np.float32), None
    from test_particle_velocity_cpu import read_bgeo_v
    return read_bgeo_v(path)


def test_gmpm_output_velocity(tmp_path):
    """gmpm with simulation.output_velocity writes every frame with the "v" attribute (frame 0: the model's v0; later frames: the readout);
    without the key the frames are the position-only ones."""
    import __graft_entry__ as g
    g.build_host()
    frames = 2
    models = [{"file": "sphere", "constitutive": "fixed_corotated", "rho": 1e3, "volume": float(np.float32((1 / 64) ** 3 / 8)),
               "youngs_modulus": 5e3, "poisson_ratio": 0.4, "offset": [0.34375, 0.421875, 0.421875], "span": [0.15625] * 3, "velocity": [0.5, 0, 0]},
              {"file": "sphere", "constitutive": "sand", "offset": [0.53125, 0.421875, 0.421875], "span": [0.15625] * 3, "velocity": [-0.5, 0, 0]}]
    runs = {}
    for flag in (False, True):
        d = tmp_path / ("v" if flag else "plain")
        d.mkdir()
        sim = {"gpuid": 0, "fps": 500, "frames": frames, "default_dt": 1e-4, "domain_bits": 6, "output_dir": str(d)}
        if flag:
            sim["output_velocity"] = True
        fn = d / "scene.json"
        fn.write_text(json.dumps({"simulation": sim, "models": models}))
        subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(fn)], text=True, timeout=300)
        runs[flag] = d
    for mi, mod in enumerate(models):
        for f in range(frames + 1):
            name = f"model_id[{mi}]_frame[{f}].bgeo"
            xp, vp = _read_bgeo_any(runs[False] / name)
            xv, vv = _read_bgeo_any(runs[True] / name)
            assert vp is None and vv is not None and xp.shape == xv.shape
            assert np.all(np.isfinite(vv))
            if f == 0:
                raw_plain = open(runs[False] / name, "rb").read()
                assert np.array_equal(xp, xv)
                assert np.array_equal(vv, np.tile(np.float32(mod["velocity"]), (xv.shape[0], 1)))
                assert len(raw_plain) == 41 + 16 * xp.shape[0] + 2
            else:
                assert np.abs(vv.mean(axis=0) - np.float32(mod["velocity"])).max() < 0.2      # a body still moving roughly with its v0


# ---- C3 at full size ---------------------------------------------------------------------------------------------------------------------------------
def test_c3_full_size_readout_in_free_fall():
    """The 40.1 M-particle sand column after bench.py's warm-up (10 substeps of 1e-4): every particle is read out, all values finite, and the
    column, still falling freely (its floor is 4 cells above the wall zone), has v_y = g t."""
    sc = scenes.sand_column(9)
    total = sc["models"][0]["xyz"].shape[0]
    eng = build_engine(sc)
    eng.initial_setup()
    steps = 10
    eng.run_fixed(steps, sc["dt"])
    t0 = time.perf_counter()
    xyz, v = eng.retrieve_velocity(0)
    took = time.perf_counter() - t0
    assert xyz.shape[0] == total == 128 * 306 * 128 * 8
    assert np.all(np.isfinite(xyz)) and np.all(np.isfinite(v))
    gy = steps * sc["dt"] * float(np.float32(eng.cfg.gravity))
    assert np.abs(v[:, 1].astype(np.float64) - gy).max() <= 1e-5 * abs(gy), np.abs(v[:, 1] - gy).max()
    assert np.abs(v[:, [0, 2]]).max() <= 1e-5 * abs(gy)
    assert took < 60.0, took
    eng.close()

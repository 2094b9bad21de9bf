"""Force fields on the GPU (claymore_amd/csrc/mpm_force_field.hpp: grid_force_kernel ahead of every applied grid update, force_cell inside the
load readouts; mpm_set_force_field, mpm_get_force_field, mpm_test_force_field) against tests/force_field_model.py, which
tests/test_force_field_model_cpu.py judges on the CPU.  The grids are injected through the checkpoint port of
tests/test_grid_update_kernels_gpu.py: grid_update_model's 28-particle scene at bits 6 with 222 neighbour blocks in all 27 wall classes.  The
expected grid is the existing model of the update composed with the new one - gm.plain(force_model(pattern)) - compared on uint32 bit patterns
with check_cells' convention for v1; the regions are collision_shape_model's, whose faces cut through blocks and pass exactly through nodes."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import ckpt_format as cf
import collision_shape_model as sm
import face_scenes as fs
import force_field_model as fm
import grid_update_model as gm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from test_force_field_model_cpu import CASES, FOUR, ffi_fields, host_cell, host_forces  # noqa: F401  (host_forces: the x86 build's fixture)
from test_grid_update_kernels_gpu import check_cells, grid_rows, sorted_rows, state_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = gm.G_BLOCKS
N = 1 << gm.BITS
DX = fm.DX
DT = 1e-4
GRAVITY = -9.8
SEEDS = (1, 2, 3)
U = 2.0 ** -24


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def scene(gravity, boundary):
    prm = {"volume": scenes._vol(gm.BITS), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "force_field_cells", "bits": gm.BITS, "dt": DT, "config": {"max_ppc": 128, "gravity": gravity, "boundary_blocks": boundary},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": fs.to_world(gm.scene_cells(), gm.BITS), "v0": (0.5, -1.0, 0.25), "params": prm}]}


def set_fields(eng, fields):
    """Slots 0 .. 3 from model fields (None: empty)."""
    fields = list(fields) + [None] * (4 - len(fields))
    for slot, f in enumerate(fields):
        eng.set_force_field(slot, None) if f is None else eng.set_force_field(slot, **fm.engine_kwargs(f))


class Ctx:
    """One context of the scene, checkpointed right after set-up; fields and colliders come and go, the injected grid comes from the checkpoint."""

    def __init__(self, gravity=GRAVITY, boundary=2):
        self.gravity, self.boundary = gravity, boundary
        self.eng = build_engine(scene(gravity, boundary))
        self.eng.initial_setup()
        self.ckpt = self.eng.save_checkpoint().copy()
        self.keys, _ = self.eng.dump_grid()
        self.nbc = len(self.keys)

    def load(self, pattern):
        self.eng.load_checkpoint(cf.with_grid(self.ckpt, pattern))

    def update(self, pattern, dt=DT):
        self.load(pattern)
        mv = np.float32(self.eng.grid_update(dt))
        keys, blocks = self.eng.dump_grid()
        assert np.array_equal(keys, self.keys)
        return mv, blocks


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(boundary=2):
        if boundary not in made:
            made[boundary] = Ctx(GRAVITY, boundary)
            assert made[boundary].nbc == 222 and sorted(map(tuple, made[boundary].keys.tolist())) == sorted(map(tuple, gm.scene_keys().tolist()))
        return made[boundary]
    yield get
    for c in made.values():
        c.eng.close()


def expected(c, fields, pat, dt):
    """The existing model composed with the new one: -> live, strict, fused, forced grid, acted."""
    forced, acted = fm.force_model(c.keys, fields, dt, pat.view(np.float32))
    live, strict, fused = gm.plain(c.keys, G, c.boundary, c.gravity, dt, forced)
    return live, strict, fused, forced, acted


def check_forced_update(c, fields, pat, dt, want_some=True):
    mv, out = c.update(pat, dt)
    live, strict, fused, forced, acted = expected(c, fields, pat, dt)
    assert np.array_equal(gm.bits(forced[:, 0]), pat[:, 0])
    taken = check_cells(pat, out, live, strict, fused)          # (mass channel and m <= 0 cells: the pattern's bits)
    assert taken in (None, "strict"), taken
    # a live cell no field acted on (w == 0 in every slot) is the plain update of the pattern itself
    _, plain_strict, _ = gm.plain(c.keys, G, c.boundary, c.gravity, dt, pat.view(np.float32))
    idle = live & ~acted
    for ch in (1, 2, 3):
        assert np.array_equal(gm.canon(out[:, ch])[idle], gm.canon(plain_strict[:, ch])[idle]), ch
    if want_some and dt:
        assert (acted & live).sum() > 50 and (gm.canon(strict[:, 1:]) != gm.canon(plain_strict[:, 1:])).any(), "the field changed nothing"
    return out, acted & live


# ---- 1. cell by cell --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", [2, 1])
@pytest.mark.parametrize("name,f", CASES, ids=[c[0] for c in CASES])
def test_cell_by_cell(ctxs, name, f, boundary):
    """grid_force_kernel + grid_update_kernel on injected grids of the finite and the full tier, seeds 1-3, dt 1e-4 and 0: every kind and falloff,
    without a region and in each of the four region shapes, inside out and feathered (force_field_model.case_list)."""
    c = ctxs(boundary)
    set_fields(c.eng, [f])
    try:
        for tier in ("finite", "full"):
            for seed in SEEDS:
                pat = gm.generate(c.nbc, seed, tier)[0]
                for dt in (DT, 0.0):
                    _, acted = check_forced_update(c, [f], pat, dt)
                    if f["region"] is not None:                  # the region's face cuts through the grid: both kinds of live cell
                        assert acted.sum() > 50 and (~acted).sum() > 50
    finally:
        set_fields(c.eng, [])


# ---- 2. four slots, and order -------------------------------------------------------------------------------------------------------------------
def test_four_slots_and_their_order(ctxs):
    c = ctxs()
    try:
        for fields in (FOUR, [FOUR[1], None, None, FOUR[0]], [None, FOUR[3]]):
            set_fields(c.eng, fields)
            got = c.eng.force_fields()
            assert [g is not None for g in got] == [f is not None for f in list(fields) + [None] * (4 - len(fields))]
            for seed in SEEDS:
                check_forced_update(c, fields, gm.generate(c.nbc, seed, "finite")[0], DT)
            check_forced_update(c, fields, gm.generate(c.nbc, 1, "full")[0], DT)
        # a DRAG and a UNIFORM slot swapped: the bits change the way the model says
        d, u = fm.make("drag"), fm.make("uniform")
        pat = gm.generate(c.nbc, 2, "finite")[0]
        outs = []
        for fields in ([d, u], [u, d]):
            set_fields(c.eng, fields)
            outs.append(check_forced_update(c, fields, pat, DT)[0])
        assert (gm.bits(outs[0]) != gm.bits(outs[1])).sum() > 1000
    finally:
        set_fields(c.eng, [])


# ---- 3. with colliders ----------------------------------------------------------------------------------------------------------------------------
def test_field_with_a_slip_half_space_and_with_the_level_set_object(ctxs):
    """The collider kernels' result on forced momenta equals the collider model on force_model(pattern)."""
    from test_collision_shapes_gpu import assert_grid
    c = ctxs()
    eng = c.eng
    fields = [fm.make("drag", "box", feather=fm.FEATHER), fm.make("uniform", vec=(4.0, 2.0, -3.0))]
    set_fields(eng, fields)
    try:
        hs = sm.make("halfspace", type=1, friction=0.3)
        eng.set_collision_shape(0, **sm.engine_kwargs(hs))
        eng.set_collision_clock(False, 0.0)
        for seed in SEEDS:
            pat = gm.generate(c.nbc, seed, "finite")[0]
            mv, out = c.update(pat)
            forced, acted = fm.force_model(c.keys, fields, DT, pat.view(np.float32))
            live, want, mx, hits = sm.grid_update(c.keys, G, c.boundary, c.gravity, DT, forced, [hs], 0.0, DX)
            assert hits[0].sum() > 500 and (hits[0] & acted).sum() > 200
            assert_grid(pat, out, live, want)
            assert gm.bits(mv) == gm.bits(mx)
        eng.set_collision_shape(0, None)
        # the level-set object: a STICKY half-space along y whose surface cuts the central blocks (test_collision_kernel_node_mapping's)
        idx = np.arange(N, dtype=np.float64)
        sdf = np.broadcast_to(((idx + 0.5 - 30.0) / N).reshape(1, N, 1), (N, N, N)).astype(np.float32)
        grad = np.zeros((3, N, N, N), np.float32)
        grad[1] = 1.0
        eng.set_collision_object(sdf=sdf, grad=grad, type=0)
        pat = gm.generate(c.nbc, 2, "finite")[0]
        mv, out = c.update(pat)
        forced, _ = fm.force_model(c.keys, fields, DT, pat.view(np.float32))
        live, want, mx = gm.collision(c.keys, G, c.boundary, c.gravity, DT, forced, sticky_sdf=sdf)
        assert np.array_equal(gm.bits(out), gm.bits(want)), np.argwhere(gm.bits(out) != gm.bits(want))[:4].tolist()
        assert gm.bits(mv) == gm.bits(mx)
    finally:
        eng.set_collision_object(None)
        eng.set_collision_shape(0, None)
        set_fields(eng, [])


def rows_array(d):
    return np.array([[d[n]["count"], *d[n]["impulse"], *d[n]["angular_impulse"], d[n]["mass"]] for n in _ffi.LOAD_ROW_NAMES], dtype=np.float64)


def test_load_readouts_see_the_forced_momenta(ctxs):
    """mpm_collider_loads, the read-only readout of the coming update, equals the gauge's reading after mpm_grid_update bit for bit with fields
    installed (the gauge reads behind the fields' pass, the readout applies the fields to its register copy); the contact map holds the same nodes;
    both differ from the readings without the fields."""
    c = ctxs()
    eng = c.eng
    fields = [fm.make("uniform", "sphere", vec=(0.0, -400.0, 0.0)), fm.make("drag", "box", feather=fm.FEATHER)]
    hs = sm.make("halfspace", type=2, friction=0.3)                           # SEPARATE: what it touches depends on the velocity's sign
    eng.set_collision_shape(0, **sm.engine_kwargs(hs))
    eng.set_collision_clock(False, 0.0)
    try:
        pat = gm.generate(c.nbc, 3, "finite")[0]
        c.load(pat)
        bare = rows_array(eng.collider_loads(DT))
        set_fields(eng, fields)
        read = rows_array(eng.collider_loads(DT))
        nodes, rows, mass, dv, va = eng.collider_contacts(DT)
        keys, blocks = eng.dump_grid()
        assert np.array_equal(gm.bits(blocks), pat), "a readout wrote the grid"
        eng.load_gauge(True)
        eng.grid_update(DT)
        gauge, elapsed, updates = eng.read_load_gauge()
        gauge = rows_array(gauge)
        eng.load_gauge(False)
        assert updates == 1
        assert np.array_equal(read.view(np.uint64), gauge.view(np.uint64)), (read, gauge)
        assert read[1, 0] > 100 and int(read[:, 0].sum()) == len(nodes)
        assert not np.array_equal(read[1], bare[1]), "the fields changed nothing at the collider"
        # the contact map's velocities are those of the model on the forced momenta
        forced, _ = fm.force_model(c.keys, fields, DT, pat.view(np.float32))
        live, want, mx, hits = sm.grid_update(c.keys, G, c.boundary, c.gravity, DT, forced, [hs], 0.0, DX)
        on0 = rows == 1
        nd = gm.node_coords(c.keys)
        lut = {tuple(nd[b, :, k]): (b, k) for b in range(c.nbc) for k in range(64)}
        got_v = np.stack([va[i] for i in np.flatnonzero(on0)])
        want_v = np.stack([want[lut[tuple(nodes[i])][0], 1:4, lut[tuple(nodes[i])][1]] for i in np.flatnonzero(on0)])
        assert np.array_equal(gm.canon(got_v), gm.canon(want_v))
    finally:
        eng.set_collision_shape(0, None)
        set_fields(eng, [])


def test_rigid_body_sees_forced_momenta_and_feels_no_field(ctxs):
    """A body in slot 0 plus a UNIFORM field: the body's state and the grid after one update equal those of a run without the field whose grid had
    the forced momenta injected directly - the fields' pass comes first, and the field acts on the material alone."""
    c = ctxs()
    eng = c.eng
    sp = sm.make("sphere", type=1, friction=0.3)
    f = fm.make("uniform", vec=(30.0, -20.0, 10.0))
    pat = gm.generate(c.nbc, 1, "finite")[0]
    forced, _ = fm.force_model(c.keys, [f], DT, pat.view(np.float32))
    states, grids = [], []
    try:
        for fields, grid in (([f], pat), ([], gm.bits(forced))):
            eng.set_collision_shape(0, **sm.engine_kwargs(sp))
            eng.set_collision_clock(False, 0.0)
            eng.set_collider_body(0, mass=5.0, inertia=(0.3, 0.2, 0.25, 0.01, -0.02, 0.015), com=tuple(float(v) for v in sp["a"]))
            set_fields(eng, fields)
            _, out = c.update(grid)
            st = eng.collider_body(0)
            assert st["updates"] == 1 and st["last_touched_nodes"] > 100
            states.append(st)
            grids.append(gm.bits(out))
        for k in ("position", "orientation", "velocity", "omega", "angular_momentum", "last_impulse", "last_angular_impulse"):
            assert np.array_equal(states[0][k].view(np.uint64), states[1][k].view(np.uint64)), k
        assert states[0]["last_touched_mass"] == states[1]["last_touched_mass"] and states[0]["last_touched_nodes"] == states[1]["last_touched_nodes"]
        assert np.array_equal(grids[0], grids[1])
        # ... and the field mattered: without it the impulse is another one
        eng.set_collision_shape(0, **sm.engine_kwargs(sp))
        eng.set_collision_clock(False, 0.0)
        eng.set_collider_body(0, mass=5.0, inertia=(0.3, 0.2, 0.25, 0.01, -0.02, 0.015), com=tuple(float(v) for v in sp["a"]))
        c.update(pat)
        assert not np.array_equal(eng.collider_body(0)["last_impulse"], states[0]["last_impulse"])
    finally:
        eng.set_collision_shape(0, None)
        set_fields(eng, [])


# ---- 4. the function-level entry point -----------------------------------------------------------------------------------------------------------
def device_cell(fields, dt, X, mp4):
    X, mp4 = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(mp4, dtype=np.float32)
    out = np.empty_like(mp4)
    assert _ffi.load_hip().test_force_field(ffi_fields(fields), len(fields), float(dt), DX, ptr(X), ptr(mp4), len(X), ptr(out), 0) == 0
    return out


@pytest.mark.parametrize("name,f", CASES, ids=[c[0] for c in CASES])
def test_device_equals_the_x86_build_equals_the_model(host_forces, name, f):
    """mpm_test_force_field on the hostcheck's point set: device = x86 = model on bit patterns (computed NaNs as NaNs)."""
    X, mp4 = fm.adversarial_points([f], 3)
    for dt in (DT, 0.0):
        want, acted = fm.force_cell([f], X, dt, mp4)
        dev, host = device_cell([f], dt, X, mp4), host_cell(host_forces, [f], dt, X, mp4)
        assert np.array_equal(gm.bits(dev[:, 0]), gm.bits(mp4[:, 0])) and np.array_equal(gm.bits(dev[~acted]), gm.bits(mp4[~acted]))
        for got in (dev, host):
            bad = gm.canon(got) != gm.canon(want)
            assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_device_four_slots(host_forces):
    X, mp4 = fm.adversarial_points(FOUR, 5)
    want, acted = fm.force_cell(FOUR, X, DT, mp4)
    dev = device_cell(FOUR, DT, X, mp4)
    assert np.array_equal(gm.canon(dev), gm.canon(want)) and np.array_equal(gm.bits(dev[~acted]), gm.bits(mp4[~acted]))
    assert np.array_equal(gm.canon(host_cell(host_forces, FOUR, DT, X, mp4)), gm.canon(want))


# ---- 5. the drivers -----------------------------------------------------------------------------------------------------------------------------
def sparse(sync_interval=None):
    from test_collision_clock_gpu import sparse_scene
    sc = sparse_scene()
    sc["collision"] = None
    sc["config"]["gravity"] = GRAVITY
    if sync_interval is not None:
        sc["config"]["sync_interval"] = sync_interval
    return sc


def snapshot(eng):
    return (sorted_rows(eng.retrieve_positions(0)), state_rows(eng)) + grid_rows(eng)


def assert_same(a, b, what=""):
    for name, x, y in zip(("positions", "state", "grid keys", "grid"), a, b):
        assert x.shape == y.shape and np.array_equal(x, y), (what, name, int((x != y).sum()) if x.shape == y.shape else (x.shape, y.shape))


DRIVER_FIELDS = [fm.make("drag", "box", feather=fm.FEATHER, strength=50.0), None, fm.make("vortex", centre=(0.5, 0.25, 0.5), swirl=30.0, pull=4.0, lift=-1.5)]


@pytest.mark.parametrize("sync_interval", [1, None])
def test_run_fixed_equals_the_phase_level_loop_with_fields(sync_interval):
    """mpm_run_fixed(12) with two fields installed - every grid update a launch of its own behind the fields' pass - against grid update, g2p2g,
    rebuild phase by phase on the deterministic sparse scene: positions, state and the grid the run leaves behind bit for bit; and the fields
    did something (the run without them ends elsewhere)."""
    sc = sparse(sync_interval)
    runs = []
    for how in ("phase", "phase", "fixed", "bare"):
        eng = build_engine(sc)
        eng.initial_setup()
        if how != "bare":
            set_fields(eng, DRIVER_FIELDS)
        if how == "phase":
            for _ in range(12):
                eng.grid_update(sc["dt"])
                eng.g2p2g(sc["dt"], sc["dt"])
                eng.rebuild_partition()
        else:
            eng.run_fixed(12, sc["dt"])
        runs.append(snapshot(eng))
        eng.close()
    assert_same(runs[0], runs[1], "the scene is not deterministic: nothing to compare")
    assert runs[0][0].shape == (48, 3)
    assert_same(runs[2], runs[0], "run_fixed against the phase-level loop")
    assert not np.array_equal(runs[3][0], runs[0][0]), "the fields changed nothing"


def test_a_field_removed_mid_run_and_empty_slots_cost_nothing():
    """Six substeps with fields, then the fields are removed: from the checkpoint taken there, the context goes on (fusing again) exactly as a
    context that never had a field and was fed the same checkpoint.  A context whose slots were filled and emptied before the run gives the bits
    of one that never heard of fields."""
    sc = sparse()
    a, b, never = build_engine(sc), build_engine(sc), build_engine(sc)
    try:
        for e in (a, b, never):
            e.initial_setup()
        set_fields(a, DRIVER_FIELDS)
        a.run_fixed(6, sc["dt"])
        set_fields(a, [])
        assert a.force_fields() == [None] * 4
        ck = a.save_checkpoint().copy()
        a.run_fixed(6, sc["dt"])
        b.load_checkpoint(ck)
        b.run_fixed(6, sc["dt"])
        assert_same(snapshot(a), snapshot(b), "after the removal")
        # all slots empty: the parent's path
        set_fields(b, FOUR)
        set_fields(b, [])
        b.load_checkpoint(never.save_checkpoint().copy())
        b.run_fixed(12, sc["dt"])
        never.run_fixed(12, sc["dt"])
        assert_same(snapshot(b), snapshot(never), "empty slots")
    finally:
        for e in (a, b, never):
            e.close()


# ---- 6. physics ---------------------------------------------------------------------------------------------------------------------------------
STEPS = 20


def block_scene(gravity, v0=(0.0, 0.0, 0.0), material=_ffi.FIXED_COROTATED):
    """A lattice block of 12 x 12 x 12 cells (13 824 particles) in the interior of the bits-6 domain."""
    lo = (26, 30, 26)
    prm = {"volume": scenes._vol(6), "rho": 1e3}
    return {"name": "force_block", "bits": 6, "dt": DT, "config": {"max_ppc": 16, "gravity": gravity},
            "models": [{"material": material, "xyz": scenes.lattice_box(6, lo, tuple(x + 12 for x in lo)), "v0": v0, "params": prm}]}


def free_fall_deviation(eng, y0, g):
    """Largest deviation of a particle from the discrete closed form of free fall after STEPS substeps (v_n = n g dt, y_n = y_0 + g dt^2 n (n + 1) / 2,
    dt the float32 step) in float64: (velocity, relative to v_n; height, relative to the distance fallen - every particle falls the same distance,
    so the sorted heights pair up)."""
    dt = float(np.float32(DT))
    xyz, vel = eng.retrieve_velocity(0)[:2]
    v_n, fall = STEPS * g * dt, g * dt * dt * STEPS * (STEPS + 1) / 2
    dv = np.abs(vel.astype(np.float64) - np.array([0.0, v_n, 0.0])).max() / abs(v_n)
    dy = np.abs(np.sort(xyz[:, 1].astype(np.float64)) - np.sort(y0.astype(np.float64) + fall)).max() / abs(fall)
    return dv, dy


def test_free_fall_under_a_uniform_field_equals_free_fall_under_gravity():
    """gravity = 0 plus UNIFORM (0, g, 0), and gravity = g with no field, both against the float64 discrete closed form of free fall.  The field
    run's deviation may be at most twice what the existing gravity shows in this same test (the yardstick is the parent's path)."""
    g = -9.8
    dev = {}
    for how in ("gravity", "field"):
        sc = block_scene(g if how == "gravity" else 0.0)
        eng = build_engine(sc)
        eng.initial_setup()
        y0 = eng.retrieve_positions(0)[:, 1].copy()
        if how == "field":
            eng.set_force_field(0, "uniform", vec=(0.0, g, 0.0))
        eng.run_fixed(STEPS, DT)
        dev[how] = free_fall_deviation(eng, y0, g)
        eng.close()
    print(f"free fall after {STEPS} substeps, deviation (velocity, height): under gravity {dev['gravity'][0]:.3e}, {dev['gravity'][1]:.3e}; "
          f"under the UNIFORM field {dev['field'][0]:.3e}, {dev['field'][1]:.3e}")
    assert dev["gravity"][0] < 1e-4 and dev["gravity"][1] < 1e-1            # (the yardstick itself is in free fall: heights carry ulp(0.5) / fall = 3e-4 a step)
    assert dev["field"][0] <= 2.0 * dev["gravity"][0] and dev["field"][1] <= 2.0 * dev["gravity"][1], dev


def test_drag_decays_momentum_as_implicit_euler_says():
    """DRAG toward rest everywhere, no gravity, the block moving with v0: particle_momentum() after n substeps against p0 / (1 + k dt)^n in float64.
    Margin: twice the relative momentum drift the same block shows with no field over the same steps, plus the statement's roundings - per substep
    and node k dt (1), 1 + s (1), the quotient (1): 3 n U."""
    k, v0 = 400.0, (0.6, -0.3, 0.45)
    mom = {}
    for how in ("bare", "drag"):
        eng = build_engine(block_scene(0.0, v0))
        eng.initial_setup()
        p0 = eng.particle_momentum()["momentum"]
        if how == "drag":
            eng.set_force_field(0, "drag", vec=(0.0, 0.0, 0.0), strength=k)
        eng.run_fixed(STEPS, DT)
        mom[how] = (p0, eng.particle_momentum()["momentum"])
        eng.close()
    drift = np.abs(mom["bare"][1] - mom["bare"][0]).max() / np.abs(mom["bare"][0]).max()
    s = float(np.float32(np.float32(k) * np.float32(DT)))
    want = mom["drag"][0] / (1.0 + s) ** STEPS
    err = np.abs(mom["drag"][1] - want).max() / np.abs(want).max()
    margin = 2.0 * drift + 3 * STEPS * U
    print(f"drag over {STEPS} substeps: momentum / closed form - 1 = {err:.3e}; drift without a field {drift:.3e}, margin {margin:.3e}; decay factor {(1 + s) ** -STEPS:.4f}")
    assert (1 + s) ** -STEPS < 0.5
    assert err <= margin, (err, margin)


def test_vortex_angular_impulse():
    """A block at rest, no gravity, one update under a VORTEX about the vertical axis through its middle: the angular momentum about the axis the
    update leaves on the grid, sum m (rp x v) . n, has the sign and the magnitude of sum m swirl |rp|^2 dt.  Bound per node, counted as in
    test_model_against_the_float64_closed_forms (p = 0 before: no cancellation against an old momentum): U m dt (E_a + 4 A) for the momentum, 2 U |p'|
    for the division by the mass and back; summed with the lever arm |rp|."""
    swirl, pull, lift = 25.0, 3.0, -2.0
    centre = np.array([0.5, 0.0, 0.5])
    eng = build_engine(block_scene(0.0))
    eng.initial_setup()
    keys, before = eng.dump_grid()
    eng.set_force_field(0, "vortex", vec=(0.0, 1.0, 0.0), centre=tuple(centre), swirl=swirl, pull=pull, lift=lift)
    eng.grid_update(DT)
    keys2, after = eng.dump_grid()
    eng.close()
    assert np.array_equal(keys, keys2)
    dt = float(np.float32(DT))
    X = (gm.node_coords(keys).astype(np.float32) * np.float32(DX)).astype(np.float64)          # (nbc, 3, 64)
    m = before[:, 0].astype(np.float64)
    live = m > 0
    assert live.sum() > 1000 and not before[:, 1:][np.broadcast_to(live[:, None], before[:, 1:].shape)].any()
    r = X - centre[None, :, None]
    rp = r.copy()
    rp[:, 1] = 0.0
    v = after[:, 1:4].astype(np.float64)
    L = (m * (rp[:, 2] * v[:, 0] - rp[:, 0] * v[:, 2]))[live].sum()                             # (rp x v) . y
    want = (m * swirl * (rp[:, 0] ** 2 + rp[:, 2] ** 2) * dt)[live].sum()
    rho = np.abs(r).sum(axis=1)
    A = 4 * swirl * rho + 2 * pull * rho + abs(lift)
    Ea = 36 * swirl * rho + 14 * pull * rho + 2 * abs(lift)
    per_node = U * m * dt * (Ea + 4 * A) + 2 * U * m * dt * A
    bound = 1.01 * (per_node * (np.abs(rp[:, 0]) + np.abs(rp[:, 2])))[live].sum()
    print(f"vortex: angular impulse {L:.9e}, closed form {want:.9e}, |difference| {abs(L - want):.3e}, bound {bound:.3e}")
    assert L > 0 and want > 0
    assert abs(L - want) <= bound, (L, want, bound)


# ---- 7. refusals and scenes ---------------------------------------------------------------------------------------------------------------------
def test_a_grouped_context_is_refused_and_a_group_refuses_a_field():
    from test_collision_shapes_gpu import sparse_analytic
    sc = sparse_analytic(boundary="slip")
    world = 2
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    lg.create()
    errors = []

    def work(r):
        try:
            ranks[r].initial_setup()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    try:
        assert not errors, errors
        with pytest.raises(EngineError) as e:
            ranks[0].eng.set_force_field(0, "uniform", vec=(0.0, -1.0, 0.0))
        assert e.value.code == _ffi.MPM_ERR_INVALID and "group" in str(e.value)
        assert ranks[0].eng.force_fields() == [None] * 4
    finally:
        for r in ranks:
            r.close()
    eng = build_engine(sc)
    eng.initial_setup()
    eng.set_force_field(1, "uniform", vec=(0.0, -1.0, 0.0))
    handles = (C.c_void_p * 1)()
    ctxs_ = (C.c_void_p * 1)(eng.ctx)
    assert eng.api.group_create_local(ctxs_, 1, handles) == _ffi.MPM_ERR_INVALID and b"force field" in eng.api.last_error(eng.ctx)
    eng.run_fixed(2, sc["dt"])                                                              # (the context itself goes on)
    eng.close()


def test_an_invalid_field_leaves_the_slots_as_they_were(ctxs):
    eng = ctxs().eng
    set_fields(eng, FOUR)
    before = eng.force_fields()
    try:
        assert all(b is not None for b in before)
        axis = np.array(before[2]["vec"], np.float64)
        assert abs(np.linalg.norm(axis) - 1.0) < 4 * U and np.array_equal(np.float32(before[2]["vec"]), FOUR[2]["vec"])      # the unit axis, the model's bits
        assert np.array_equal(np.float32(before[3]["region"]["b"]), FOUR[3]["region"]["b"])                                  # the unit region normal
        nan = float("nan")
        bad = [dict(kind=5), dict(kind="point", falloff=3), dict(kind="uniform", vec=(nan, 0, 0)), dict(kind="vortex", vec=(0, 0, 0)),
               dict(kind="drag", strength=-1.0), dict(kind="point", soft=-1.0), dict(kind="uniform", feather=-1.0), dict(kind="uniform", strength=float("inf")),
               dict(kind="uniform", region=dict(kind="box", a=(0.5, 0.5, 0.5), b=(0.1, 0.0, 0.1))), dict(kind="uniform", region=dict(kind="sphere", a=(0.5, 0.5, 0.5), radius=0.0))]
        for slot in range(4):
            for kw in bad:
                with pytest.raises(EngineError) as e:
                    eng.set_force_field(slot, **kw)
                assert e.value.code == _ffi.MPM_ERR_INVALID and "mpm_set_force_field" in str(e.value), (kw, str(e.value))
        for slot in (-1, 4):
            with pytest.raises(EngineError) as e:
                eng.set_force_field(slot, "uniform", vec=(0, -1, 0))
            assert e.value.code == _ffi.MPM_ERR_INVALID and "slot" in str(e.value)
        assert eng.force_fields() == before
        # a checkpoint load leaves the installed fields in place
        c = ctxs()
        c.load(gm.generate(c.nbc, 1, "finite")[0])
        assert eng.force_fields() == before
    finally:
        set_fields(eng, [])


@pytest.mark.parametrize("name", ["sand_in_wind", "stirred_tank"])
def test_new_scenes_through_main_loop(name):
    """Two frames of 2 ms: the entry is installed from 0.5 ms on and removed at 3 ms - force_fields() shows it at the end of frame 1 and not at the
    end of frame 2 - and it moved the material."""
    sc = getattr(scenes, name)()
    sc["forces"][0]["start"], sc["forces"][0]["end"] = 0.0005, 0.003
    eng = build_engine(sc)
    seen = []
    def spin(e):                                                   # angular momentum per unit particle mass about the vertical axis through the middle
        xyz, vel = e.retrieve_velocity(0)[:2]
        x, z = xyz[:, 0].astype(np.float64) - 0.5, xyz[:, 2].astype(np.float64) - 0.5
        return float((z * vel[:, 0] - x * vel[:, 2]).sum())
    eng.main_loop(2, 500, 1e-4, on_frame=lambda frame, e: seen.append((e.cur_time, e.force_fields()[0], e.particle_momentum()["momentum"].copy(), spin(e))))
    d = eng.diagnostics()
    eng.close()
    print(name, [(t, None if f is None else f["kind"], p, L) for t, f, p, L in seen])
    assert (int(d.lost_particles), int(d.dropped_particles)) == (0, 0)
    assert seen[0][1] is not None and seen[0][1]["kind"] == sc["forces"][0]["kind"] and seen[1][1] is None
    bare = dict(sc)
    bare.pop("forces")
    ref = build_engine(bare)
    ref.main_loop(1, 500, 1e-4)
    p_ref, spin_ref = ref.particle_momentum()["momentum"], spin(ref)
    ref.close()
    print(name, "without the field:", p_ref, spin_ref)
    if name == "sand_in_wind":
        assert seen[0][2][0] > 0 and seen[0][2][0] > 100 * abs(p_ref[0])                       # the wind pushed the sand along +x
    else:
        assert seen[0][3] > 0 and seen[0][3] > 100 * abs(spin_ref)                             # swirl > 0 about +y: (r x v) . y > 0


def test_gmpm_forces_scene_equals_the_engine(tmp_path):
    """A "forces" scene - a feathered DRAG box switched off mid-run and a UNIFORM field switched on mid-run - through the gmpm driver for two
    frames: its positions are those of the same scene driven through Engine with scenes.ForceEntry, bit for bit (tests/test_gmpm_stress_gpu.py's
    two single-block bodies, on which the engine is deterministic)."""
    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS, DT_DEFAULT, FC, FPS, FRAMES, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    forces = [{"kind": "drag", "vec": [2.0, 0.5, 0.0], "strength": 300.0, "feather": 2 / 64, "start": 0.0, "end": 0.00213,
               "region": {"shape": "box", "center": [8 / 64, 25 / 64, 25 / 64], "half_extents": [6 / 64, 12 / 64, 12 / 64]}},
              {"kind": "uniform", "vec": [0.0, 0.0, 25.0], "start": 0.00107}]
    d = tmp_path / "forces"
    d.mkdir()
    sim = {"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d)}
    (d / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "forces": forces}))
    log = subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(d / "scene.json")], text=True, timeout=300)
    assert "has 2 forces" in log
    start = [read_bgeo_attrs(frame(d, m, 0))[0] for m in range(len(MODELS))]

    def drive(with_forces):
        eng = Engine(domain_bits=BITS, max_ppc=128)
        for mod, xyz in zip(MODELS, start):
            mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
            eng.init_model(mat, xyz, mod["velocity"], **({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {}))
        entries = []
        if with_forces:
            for f in forces:
                f = dict(f)
                if "region" in f:
                    r = f["region"]
                    f["region"] = {"kind": r["shape"], "center": r["center"], "half_extents": r["half_extents"]}
                entries.append(scenes.ForceEntry.from_dict(f))

        def serve(t):
            for slot, fe in enumerate(entries):
                act = fe.due(t)
                if act > 0:
                    eng.set_force_field(slot, **fe.field)
                elif act < 0:
                    eng.set_force_field(slot, None)
        spf = np.float32(1.0) / np.float32(FPS)
        max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in MODELS)
        dt = eng.compute_dt(max_v0, 0.0, float(spf), DT_DEFAULT)
        eng.initial_setup()
        cur = np.float32(0.0)
        serve(0.0)
        frames, log_ = [], []
        for _ in range(FRAMES):
            t = np.float32(0.0)
            while t < spf:
                next_dt, _ = eng.substep(dt, float(t), float(spf), DT_DEFAULT)
                t = np.float32(t + np.float32(dt))
                cur = np.float32(cur + np.float32(dt))
                dt = next_dt
                serve(float(cur))
            frames.append([sorted_rows(eng.retrieve_positions(m)) for m in range(len(MODELS))])
            log_.append([f is not None for f in eng.force_fields()[:2]])
        eng.close()
        return frames, log_

    (want, installed), (free, _) = drive(True), drive(False)
    assert installed == [[True, True], [False, True]], installed
    for f in range(1, FRAMES + 1):
        for m in range(len(MODELS)):
            got = sorted_rows(read_bgeo_attrs(frame(d, m, f))[0])
            assert np.array_equal(got, want[f - 1][m]), (f, m)
    for m in range(len(MODELS)):
        assert not np.array_equal(want[-1][m], free[-1][m]), f"the forces did not move model {m}"

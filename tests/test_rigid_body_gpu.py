"""Rigid bodies on the GPU (claymore_amd/csrc/mpm_rigid_body.hpp: grid_update_body_kernel, body_step_kernel; mpm_set_collider_body,
mpm_get_collider_body, mpm_set_collider_body_state) against tests/rigid_body_model.py, which tests/test_rigid_body_cpu.py judges on the CPU.
The injected grids are tests/test_collider_loads_gpu.py's: VolumeCtx at bits 6, 222 neighbour blocks in all 27 wall classes, the generator's
finite tier.  Velocities, contacts, the state and the impulses are compared on bit patterns; the totals against math.fsum within the existing
bound 4 n 2^-53 sum |terms|."""
import copy
import threading

import numpy as np
import pytest

import ckpt_format as cf
import collider_load_model as lm
import collision_shape_model as sm
import collision_volume_model as vm
import grid_update_model as gm
import heightfield_model as hm
import rigid_body_model as bm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from test_collider_loads_gpu import assert_totals, rows_array
from test_collision_shapes_gpu import BOUNDARY, DT, DX, G, GRAVITY, N, sorted_rows, sparse_analytic
from test_collision_volume_gpu import VolumeCtx

pytestmark = pytest.mark.gpu
H, G64 = float(np.float32(DT)), float(np.float32(GRAVITY))
INERTIA = (0.3, 0.2, 0.25, 0.01, -0.02, 0.015)


@pytest.fixture(scope="module")
def ctx():
    c = VolumeCtx()
    assert c.nbc == 222
    yield c
    c.eng.close()


def install_bodies(ctx, cols, bodies, field=None, t=0.0):
    """cols as VolumeCtx.install takes them; bodies: {slot: dict(mass, inertia, com[, gravity, lock, force, torque])}.  -> {slot: (constants, start state)},
    the start state read from the device and checked against the model's on bits."""
    ctx.install(cols, field=field, t=t)
    out = {}
    for slot, b in bodies.items():
        ctx.eng.set_collider_body(slot, **b)
        c = bm.constants(**b)
        got = bm.state_of(ctx.eng.collider_body(slot))
        assert np.array_equal(bm.state_words(got), bm.state_words(bm.start(cols[slot], c, t))), slot
        out[slot] = (c, got)
    return out


def check_update(ctx, seed, cols, bodies, field=None, dt=DT):
    """One update on an injected grid: contacts, totals, every node's velocity, the maximum, the impulses and the new state against the model."""
    eng = ctx.eng
    start = install_bodies(ctx, cols, bodies, field=field)
    pat = gm.generate(ctx.nbc, seed, "finite")[0]
    eng.load_checkpoint(cf.with_grid(ctx.ckpt, pat))
    for slot, (c, s0) in start.items():                                                    # (a checkpoint load leaves a body as it is)
        assert np.array_equal(bm.state_words(bm.state_of(eng.collider_body(slot))), bm.state_words(s0))
    spec = {slot: (c["com"], bm.pose_of(s0)) for slot, (c, s0) in start.items()}
    nr = bm.node_rows(ctx.keys, G, BOUNDARY, GRAVITY, dt, pat.view(np.float32), cols, 0.0, DX, field=field, bodies=spec)
    got_nr, got_rec = lm.sort_contacts(*eng.collider_contacts(dt))
    want_nr, want_rec = lm.contacts(nr)
    assert np.array_equal(got_nr, want_nr), (len(got_nr), len(want_nr))
    assert not (gm.canon(got_rec) != gm.canon(want_rec)).any()
    loads = rows_array(eng.collider_loads(dt))
    piv = lm.default_pivots([None if s in bodies else c for s, c in enumerate(cols)], 0.0, field=field)
    for slot, (c, s0) in start.items():
        piv[1 + slot] = s0["x"]                                                             # a body row's default pivot: its x
    want, mag = lm.totals(nr, piv)
    assert_totals(loads, want, mag, "body rows about x")
    mv = np.float32(eng.grid_update(dt))
    keys, out = eng.dump_grid()
    assert np.array_equal(keys, ctx.keys) and np.array_equal(gm.bits(out[:, 0]), pat[:, 0])
    vel = np.ascontiguousarray(out[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    lv = nr["live"]
    bad = (gm.canon(vel[lv]) != gm.canon(nr["v_final"][lv])).any(axis=1)
    assert not bad.any(), (int(bad.sum()), nr["nodes"][lv][bad][:4].tolist())
    assert np.array_equal(gm.bits(vel[~lv]), pat[:, 1:4].transpose(0, 2, 1).reshape(-1, 3)[~lv]), "a massless cell changed"
    vf = nr["v_final"][lv]
    assert gm.bits(mv) == gm.bits(gm.collision_q32(vf[:, 0], vf[:, 1], vf[:, 2]).max()), float(mv)
    for slot, (c, s0) in start.items():
        d = eng.collider_body(slot)
        row = loads[1 + slot]
        assert np.array_equal(d["last_impulse"].view(np.uint64), row[1:4].view(np.uint64)) and np.array_equal(d["last_angular_impulse"].view(np.uint64), row[4:7].view(np.uint64))
        assert d["last_touched_nodes"] == row[0] and d["last_touched_mass"] == row[7] and d["updates"] == 1
        s = copy.deepcopy(s0)
        assert bm.body_step(s, c, row[1:4], row[4:7], row[0], row[7], H, G64)
        assert np.array_equal(bm.state_words(bm.state_of(d)), bm.state_words(s)), (slot, d)
        assert d["max_mass_ratio"] == row[7] * c["inv_mass"]
    return nr, loads


def body(com, **kw):
    return dict(mass=5.0, inertia=INERTIA, com=tuple(float(v) for v in com), **kw)


# ---- 1. one update on an injected grid ------------------------------------------------------------------------------------------------------
def test_two_bodies_a_prescribed_collider_the_field_and_the_walls(ctx):
    f = sm.make("box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    sdf, grad = sm.sample_field(f, N, DX)
    a = sm.make("sphere", type=1, friction=0.3, trans_vel=(0.2, -0.1, 0.3), omega=(1.0, 2.0, -1.0))
    p = sm.make("capsule", type=2, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    b = sm.make("box", type=2, friction=0.25, trans=(0.5, 0.5, 0.5), rot_mat=sm.TILT, trans_vel=(-0.3, 0.2, 0.1), omega=(0.5, -1.5, 1.0))
    bodies = {0: body(a["a"]), 3: body(b["a"], gravity=False, force=(0.5, 0.0, -0.25), torque=(0.0, 0.1, 0.0))}
    nr, loads = check_update(ctx, 11, [a, p, None, b], bodies, field=(f, sdf, grad))
    assert nr["used"] == [lm.WALLS, 0, 1, 2, 4] and (loads[[0, 1, 2, 4, 5], 0] > 100).all(), loads[:, 0]
    assert (nr["touched"][1] & nr["touched"][4]).sum() > 20                                # slot 3 acts on what slot 0 left


def test_two_bodies_around_a_prescribed_heightfield_and_a_prescribed_volume(ctx):
    """Every kind of the slot dispatch in one walk with bodies installed: a sphere body, tests/test_collision_volume_gpu.py's mixed-slots heightfield
    (it cuts the block), a prescribed volume, a tilted box body."""
    a = sm.make("sphere", type=1, friction=0.3, trans_vel=(0.2, -0.1, 0.3), omega=(1.0, 2.0, -1.0))
    h = hm.make("65x65", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    v = vm.sphere_volume(shape="box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    b = sm.make("box", type=2, friction=0.25, trans=(0.5, 0.5, 0.5), rot_mat=sm.TILT, trans_vel=(-0.3, 0.2, 0.1), omega=(0.5, -1.5, 1.0))
    nr, loads = check_update(ctx, 16, [a, h, v, b], {0: body(a["a"]), 3: body(b["a"], gravity=False)})
    assert nr["used"] == [lm.WALLS, 1, 2, 3, 4] and (loads[[1, 2, 3, 4, 5], 0] > 0).all(), loads[:, 0]


def test_capsule_body_and_mesh_built_volume_body(ctx):
    eng = ctx.eng
    c = sm.make("capsule", type=0, trans=(0.45, 0.5, 0.5), rot_mat=sm.TILT, trans_vel=(0.1, 0.3, -0.2), omega=(-1.0, 0.5, 2.0))
    mid = 0.5 * (c["a"].astype(np.float64) + c["b"].astype(np.float64))
    # the volume: built on the device from an icosphere; the model reads the table back
    v, f = scenes.icosphere((0.47, 0.52, 0.55), 0.21, 2)
    kw = dict(type=1, friction=0.3, trans=(0.5, 0.5, 0.5), trans_vel=(0.0, -0.25, 0.5), omega=(0.0, 0.5, 0.0))
    ctx.install([])
    eng.set_collision_volume_mesh(2, v, f, spacing=0.037, **kw)
    desc, table = eng.collision_volume(2)
    vol = vm.volume(table, origin=desc["origin"], spacing=desc["spacing"], **kw)
    m, i6, com = eng.mesh_mass_properties(v, f, 40.0)

    class Keep(VolumeCtx):                                                                  # (install the mesh-built volume again where the model's table would go)
        def __init__(self, base):
            self.__dict__.update(base.__dict__)

        def install(self, colliders=(), field=None, t=0.0):
            VolumeCtx.install(self, [colliders[0], None], field=field, t=t)
            self.eng.set_collision_volume_mesh(2, v, f, spacing=0.037, **kw)
            self.eng.set_collision_clock(False, float(t))

    nr, loads = check_update(Keep(ctx), 12, [c, None, vol], {0: body(mid, lock="rx"), 2: dict(mass=m, inertia=i6, com=com)})
    assert (loads[[1, 3], 0] > 50).all(), loads[:, 0]
    eng.set_collision_volume_mesh(2, v, f, spacing=0.037, **kw)
    eng.set_collider_body(2, density=40.0)                                                  # density=: the mesh the slot was given
    d = eng.collider_body(2)
    assert d["mass"] == float(np.float32(m)) and np.array_equal(d["inertia"], i6) and np.array_equal(d["com"], com)


# ---- 2. degenerate equalities -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,typ", [("sphere", 0), ("box", 1), ("capsule", 2)])
def test_body_at_rest_leaves_the_prescribed_colliders_bits(ctx, name, typ):
    c = sm.make(name, type=typ, friction=0.3)
    c = {**c, "trans": c["a"].copy()}                                                       # com == obj.trans, identity rot_mat, v = omega = 0
    pat = gm.generate(ctx.nbc, 13, "finite")[0]
    ctx.install([None, c])
    mv0, prescribed = ctx.update(pat)
    install_bodies(ctx, [None, c], {1: body(c["a"], gravity=False)})
    mv1, as_body = ctx.update(pat)
    assert np.array_equal(gm.bits(as_body), gm.bits(prescribed)) and gm.bits(mv0) == gm.bits(mv1)
    assert ctx.eng.collider_body(1)["last_touched_nodes"] > 100


def test_body_that_touches_nothing_leaves_every_bit(ctx):
    far = sm.collider("sphere", a=(2.0, 2.0, 2.0), radius=0.05, type=0, trans_vel=(0.3, -0.2, 0.1), omega=(1.0, 2.0, 3.0))
    a = sm.make("box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    pat = gm.generate(ctx.nbc, 14, "finite")[0]
    ctx.install([a])
    mv0, without = ctx.update(pat)
    install_bodies(ctx, [a, None, far], {2: body(far["a"])})
    mv1, with_body = ctx.update(pat)
    assert np.array_equal(gm.bits(with_body), gm.bits(without)) and gm.bits(mv0) == gm.bits(mv1)
    d = ctx.eng.collider_body(2)
    assert d["last_touched_nodes"] == 0 and not d["last_impulse"].any() and d["updates"] == 1


# ---- 3. the protocol -------------------------------------------------------------------------------------------------------------------------------
def test_free_fall_locks_round_trip_and_removal(ctx):
    eng = ctx.eng
    far = sm.collider("sphere", a=(2.0, 2.0, 2.0), radius=0.05, type=0, omega=(0.0, 0.0, 2.0))
    install_bodies(ctx, [far, far], {0: body(far["a"]), 1: body(far["a"], lock="x y z rx ry rz", force=(1.0, 1.0, 1.0), torque=(0.5, 0.5, 0.5))})
    n = 12
    for _ in range(n):
        eng.load_checkpoint(ctx.ckpt)                                                       # (a grid with the last P2G's momenta; the bodies touch none of it)
        eng.grid_update(DT)
    d0, d1 = eng.collider_body(0), eng.collider_body(1)
    v, y = n * G64 * H, 2.0 + G64 * H * H * n * (n + 1) / 2
    assert d0["updates"] == n and abs(d0["velocity"][1] - v) <= 4 * n * 2.0 ** -53 * abs(v) and abs(d0["position"][1] - y) <= 4 * n * 2.0 ** -53 * abs(y)
    assert d0["position"][0] == 2.0 and d0["orientation"][3] != 0.0
    assert not d1["velocity"].any() and np.array_equal(d1["position"], [2.0, 2.0, 2.0]) and not d1["omega"].any() and list(d1["orientation"]) == [1.0, 0.0, 0.0, 0.0]
    assert d1["lock"] == 63 and d1["mass"] == 5.0 and d1["updates"] == n
    # new constants for a body in motion: the float64 state stays, word for word (the centre of mass is the same, so x stays too)
    eng.set_collider_body(0, **{**body(far["a"]), "mass": 7.0})
    d = eng.collider_body(0)
    for key in ("position", "orientation", "velocity", "last_impulse", "last_angular_impulse"):
        assert np.array_equal(d[key].view(np.uint64), d0[key].view(np.uint64)), key
    assert d["mass"] == 7.0 and d["updates"] == n and np.abs(d["omega"] - d0["omega"]).max() <= 8 * 2.0 ** -53 * np.abs(d0["omega"]).max()
    moved = np.array(far["a"], np.float64) + [0.25, 0.0, 0.0]
    eng.set_collider_body(0, **body(moved))                                                 # the centre of mass a quarter to the right in material coordinates
    q = d["orientation"]
    want = d["position"] + np.array(bm.rotation(q)).reshape(3, 3) @ np.array([0.25, 0.0, 0.0])
    assert np.abs(eng.collider_body(0)["position"] - want).max() <= 4 * 2.0 ** -53 * 2.25
    eng.set_collider_body(0, **body(far["a"]))
    eng.set_collider_body_state(0, position=d0["position"], orientation=d0["orientation"], velocity=d0["velocity"], omega=d0["omega"])
    # a restart, and what comes back, on bits
    x, q, w = [0.3, 0.4000000000000001, 0.5], np.array([0.5, -0.5, 0.5, 0.5]), [0.1, -0.2, 0.3]
    eng.set_collider_body_state(0, position=x, orientation=q, velocity=[1.0, 2.0, 3.0], omega=w)
    d = eng.collider_body(0)
    assert d["position"].tolist() == x and d["orientation"].tolist() == q.tolist() and d["velocity"].tolist() == [1.0, 2.0, 3.0] and d["updates"] == n
    s = bm.state_of(d0)
    s["q"], s["l"] = q.tolist(), bm.world_apply(bm.rotation(q), bm.constants(**body(far["a"]))["Ib"], w)
    bm.omega_of(s, bm.constants(**body(far["a"])))
    assert d["omega"].tolist() == s["omega"] and d["angular_momentum"].tolist() == s["l"]
    eng.set_collider_body_state(0, velocity=[0.0, 0.0, 0.0])                                # NULLs keep
    d2 = eng.collider_body(0)
    assert d2["position"].tolist() == x and d2["omega"].tolist() == s["omega"] and not d2["velocity"].any()
    # removal: by a re-install, by emptying the slot, and back to a prescribed collider
    eng.set_collision_shape(0, **sm.engine_kwargs(far))
    with pytest.raises(EngineError) as e:
        eng.collider_body(0)
    assert e.value.code == _ffi.MPM_ERR_INVALID and "no rigid body" in str(e.value)
    eng.set_collision_shape(1, None)
    with pytest.raises(EngineError):
        eng.collider_body(1)
    eng.set_collider_body(0, **body(far["a"]))
    eng.load_checkpoint(ctx.ckpt)
    keys, grid = eng.dump_grid()
    blk, cell = (int(v) for v in np.argwhere(grid[:, 0] > 0)[0])
    node = keys[blk] * 4 + np.array([cell >> 4, (cell >> 2) & 3, cell & 3])
    eng.set_collider_body_state(0, position=(node * DX).tolist())                           # onto a massed node
    eng.set_collider_body(0)                                                                # prescribed again, where it stands
    with pytest.raises(EngineError):
        eng.collider_body(0)
    assert eng.collider_loads(DT)["slot0"]["count"] > 0                                     # (at rest there: the sticky sphere stops the node it sits on)


def test_refusals(ctx):
    eng = ctx.eng
    ok = sm.make("sphere", type=1)
    ctx.install([ok, sm.make("halfspace"), None, {**ok, "scale": np.float32(1.125)}])
    eng.set_collision_heightfield(2, np.zeros((4, 4), np.float32), spacing=0.25)
    good = body(ok["a"])

    def refused(slot, word, **kw):
        with pytest.raises(EngineError) as e:
            eng.set_collider_body(slot, **{**good, **kw})
        assert e.value.code == _ffi.MPM_ERR_INVALID and word in str(e.value), str(e.value)

    refused(1, "unbounded")
    refused(2, "unbounded")
    refused(3, "scale")
    refused(4, "slot")
    refused(0, "mass", mass=0.0)
    refused(0, "mass", mass=float("inf"))
    refused(0, "positive definite", inertia=(0.3, 0.2, 0.25, 0.4, 0.0, 0.0))
    refused(0, "NaN", com=(float("nan"), 0.0, 0.0))
    eng.set_collision_shape(3, None)
    refused(3, "empty")
    for bad, word in ((dict(dsdt=0.5), "dsdt"), (dict(rot_mat=np.eye(3, dtype=np.float32).ravel() * 1.01), "rotation"), (dict(rot_mat=np.diag([1.0, -1.0, 1.0]).ravel()), "reflection")):
        eng.set_collision_shape(3, **{**sm.engine_kwargs(ok), **bad})
        refused(3, word)
    b = _ffi.RigidBody()
    b.mass, b.inertia[0], b.inertia[1], b.inertia[2], b.reserved[3] = 1.0, 1.0, 1.0, 1.0, 7
    import ctypes as C
    assert eng.api.set_collider_body(eng.ctx, 0, C.byref(b)) == _ffi.MPM_ERR_INVALID and b"reserved" in eng.api.last_error(eng.ctx)
    with pytest.raises(EngineError):                                                        # nothing was installed by any of the refused calls
        eng.collider_body(0)
    with pytest.raises(EngineError):
        eng.set_collider_body_state(0, position=[0, 0, 0])
    with pytest.raises(EngineError):
        eng.set_collider_body(0)
    eng.set_collider_body(0, **good)
    with pytest.raises(EngineError) as e:                                                   # mass forgotten: not a silent release
        eng.set_collider_body(0, inertia=INERTIA, com=good["com"])
    assert "mass" in str(e.value) and eng.collider_body(0)["mass"] == 5.0
    with pytest.raises(EngineError) as e:
        eng.set_collider_body_state(0, orientation=[0.0, 0.0, 0.0, 0.0])
    assert e.value.code == _ffi.MPM_ERR_INVALID
    ctx.install([])


def test_a_grouped_context_is_refused_and_a_group_refuses_a_body():
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
            ranks[0].eng.set_collider_body(0, **body(sc["colliders"][0]["a"]))
        assert e.value.code == _ffi.MPM_ERR_INVALID and "group" in str(e.value)
    finally:
        for r in ranks:
            r.close()
    # the other way round: a context with a body is not adopted
    import ctypes as C
    eng = build_engine(sc)
    eng.initial_setup()
    eng.set_collider_body(0, **body(sc["colliders"][0]["a"]))
    handles = (C.c_void_p * 1)()
    ctxs = (C.c_void_p * 1)(eng.ctx)
    assert eng.api.group_create_local(ctxs, 1, handles) == _ffi.MPM_ERR_INVALID and b"rigid body" in eng.api.last_error(eng.ctx)
    eng.run_fixed(2, sc["dt"])                                                              # (the context itself goes on)
    assert eng.collider_body(0)["updates"] == 2
    eng.close()


def test_nan_in_a_touched_node_is_nonfinite(ctx):
    eng = ctx.eng
    c = sm.make("sphere", type=1, friction=0.3)
    install_bodies(ctx, [c], {0: body(c["a"])})
    pat = gm.generate(ctx.nbc, 15, "finite")[0].copy()
    nr = bm.node_rows(ctx.keys, G, BOUNDARY, GRAVITY, DT, pat.view(np.float32), [c], 0.0, DX, bodies={0: (body(c["a"])["com"], bm.pose_of(bm.state_of(eng.collider_body(0))))})
    interior = np.repeat(np.all(gm.wall_class(ctx.keys, G, BOUNDARY) == 1, axis=1), 64)    # (a wall zeroes its component whatever the momentum holds)
    node = int(np.flatnonzero(nr["touched"][1] & interior)[0])
    pat[node // 64, 1, node % 64] = np.float32(np.nan).view(np.uint32)
    eng.load_checkpoint(cf.with_grid(ctx.ckpt, pat))
    with pytest.raises(EngineError) as e:
        eng.substep(DT, 0.0, 1.0, DT)
    assert e.value.code == _ffi.MPM_ERR_NONFINITE
    d = eng.collider_body(0)
    assert d["updates"] == 1 and np.isnan(d["last_impulse"][0]) and np.isnan(d["velocity"][0])
    ctx.install([])


# ---- 4. the loops ------------------------------------------------------------------------------------------------------------------------------------
STEPS = 16


def sparse_body_scene():
    """The sparse 48-particle scene (deterministic: no two particles on one node) with its slip sphere, in contact from the first substep, as a
    body five times the material's mass: gravity off, v0 = the sphere's velocity."""
    sc = sparse_analytic(boundary="slip")
    col = sc["colliders"][0]
    col["animate"] = False
    col["body"] = dict(mass=0.1, inertia=(2e-4, 2e-4, 2e-4, 0.0, 0.0, 0.0), com=col["a"], gravity=False)
    return sc


def phase_run(sc, gauge=False):
    eng = build_engine(sc)
    eng.initial_setup()
    if gauge:
        eng.load_gauge(True)
    acc = np.zeros(8)
    for _ in range(STEPS):
        eng.grid_update(sc["dt"])
        d = eng.collider_body(0)
        acc = acc + np.array([d["last_touched_nodes"], *d["last_impulse"], *d["last_angular_impulse"], d["last_touched_mass"]])
        eng.g2p2g(sc["dt"], sc["dt"])
        eng.rebuild_partition()
    out = (eng.collider_body(0), sorted_rows(eng.retrieve_positions(0)), acc, rows_array(eng.read_load_gauge()[0]) if gauge else None)
    eng.close()
    return out


@pytest.fixture(scope="module")
def phase_runs():
    sc = sparse_body_scene()
    return sc, phase_run(sc, gauge=True), phase_run(sc)


def test_gauge_beside_a_body(phase_runs):
    """Inside one phase-level run the gauge's body row is the host's running sum of the per-update last_impulse / last_angular_impulse, bit for bit:
    the gauge's kernels and the update's read the same grid, the same pose and the same pivot, in the same order."""
    _, (d, _, acc, rows), _ = phase_runs
    assert d["updates"] == STEPS and acc[0] > 0 and np.abs(acc[1:4]).max() > 0
    assert np.array_equal(rows[1].view(np.uint64), acc.view(np.uint64)), (rows[1], acc)


def test_run_fixed_equals_the_phase_level_loop(phase_runs):
    """mpm_run_fixed(n, dt) with a body - every update a kernel of its own - against the phase-level loop: updates == n, and the state within 4 x
    what two phase-level runs show between themselves, with a floor of 4 x 2^-24 of the state's scale (one float32 rounding flip of a pose word;
    the scale of x, v, omega, l: the largest magnitude of that vector over the three runs, of q: 1)."""
    sc, (p1, x1, _, _), (p2, x2, _, _) = phase_runs
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(STEPS, sc["dt"])
    f, xf = eng.collider_body(0), sorted_rows(eng.retrieve_positions(0))
    eng.close()
    assert f["updates"] == STEPS == p1["updates"]
    worst = 0.0
    for name in ("position", "orientation", "velocity", "omega", "angular_momentum"):
        scale = 1.0 if name == "orientation" else max(np.abs(r[name]).max() for r in (f, p1, p2))
        between, err = np.abs(p1[name] - p2[name]).max(), np.abs(f[name] - p1[name]).max()
        print(name, "run_fixed - phase", err, "phase - phase", between, "scale", scale)
        worst = max(worst, err / scale if scale else err)
        assert err <= max(4 * between, 4 * 2.0 ** -24 * scale), (name, err, between, scale)
    print("run_fixed against the phase-level loop: largest |difference| / scale", worst)
    assert np.abs(p1["velocity"] - [1.0, 0.0, 0.0]).max() > 1e-4                            # (the material did push back)
    assert np.array_equal(x1, x2) and xf.shape == x1.shape


def positions_rel(xb, xp):
    """parity_util.match_and_compare's pos_rel of two runs of one scene."""
    from parity_util import match
    idx, _ = match(xp, xb)
    return (np.abs(xb[idx] - xp).max(axis=1) / np.abs(xp).max(axis=1)).max()


def test_heavy_body_is_the_prescribed_collider():
    """Mass 1e12, v0 given, gravity off: 20 substeps of sphere_on_obstacle_analytic at bits 6 against the same sphere prescribed with trans_vel = v0
    on a running clock; particle positions agree to the project's parity bound (1e-5 relative).  Measured on an MI355X: pos_rel 0.0 - in that
    scene the obstacle and the lowest massed node are 1.3 cells apart, 20 substeps close 0.2 of them, and no node is touched in either run
    (printed).  Closing the gap within the 20 substeps takes v0 = 20 m/s, and then the two runs do NOT agree: a prescribed collider's response
    adds trans_vel twice (collision_respond: rot^T (omega x radius + trans_vel) scale + trans_vel, the reference's statement), so a translating
    prescribed sphere drives the material at 2 v0 while its pose moves at v0; a body drives it at its true velocity.  The limit with contact is
    therefore taken at rest, where both statements give 0: test_heavy_body_at_rest_in_contact."""
    v0 = (0.0, 0.5, 0.0)

    def run(as_body):
        sc = scenes.sphere_on_obstacle_analytic(bits=6)
        col = sc["colliders"][0]
        col["trans_vel"], col["animate"] = v0, not as_body
        if as_body:
            col["body"] = dict(mass=1e12, inertia=(1e12, 1e12, 1e12, 0.0, 0.0, 0.0), com=col["a"], gravity=False)
        eng = build_engine(sc)
        eng.initial_setup()
        eng.run_fixed(20, sc["dt"])
        x = eng.retrieve_positions(0).astype(np.float64)
        d = eng.collider_body(0) if as_body else None
        pose = d["position"] if as_body else np.float64(col["a"]) + np.float64(v0) * eng.collision_time()
        eng.close()
        return x, d, pose

    (xb, d, pb), (xp, _, pp) = run(True), run(False)
    rel = positions_rel(xb, xp)
    print("heavy body against the prescribed sphere: pos_rel", rel, "touched nodes", d["last_touched_nodes"], "centres", pb, pp)
    assert rel < 1e-5 and d["updates"] == 20 and np.abs(d["velocity"] - v0).max() < 1e-9
    assert d["last_touched_nodes"] == 0 and d["max_mass_ratio"] == 0.0                      # what this scene is: no contact within the 20 substeps (see above)
    assert np.abs(pb - pp).max() < 1e-6                                                     # the two spheres did move alike


def test_heavy_body_at_rest_in_contact():
    """The heavy-body limit with contact: a fixed-corotated block thrown at 1 m/s against a slip sphere that overlaps it by a cell, the sphere
    once a body of mass 1e12 at rest (gravity off) and once prescribed at rest, 20 substeps: positions to 1e-5 relative, with nodes touched in every update (78 in the last one, pos_rel 1.2e-7 on an MI355X)."""
    def run(as_body):
        sc = scenes.sphere_through_block_analytic(bits=6, block_cells=(12, 8, 12), radius_cells=5.0, gap_cells=-1.0, speed=0.0, boundary="slip", dt=1e-4, animate=False)
        sc["models"][0]["v0"] = (-1.0, 0.0, 0.0)
        col = sc["colliders"][0]
        if as_body:
            col["body"] = dict(mass=1e12, inertia=(1e12, 1e12, 1e12, 0.0, 0.0, 0.0), com=col["a"], gravity=False)
        eng = build_engine(sc)
        eng.initial_setup()
        eng.run_fixed(20, sc["dt"])
        x = eng.retrieve_positions(0).astype(np.float64)
        d = eng.collider_body(0) if as_body else None
        eng.close()
        return x, d

    (xb, d), (xp, _) = run(True), run(False)
    rel = positions_rel(xb, xp)
    print("heavy body at rest against the prescribed sphere at rest: pos_rel", rel, "touched nodes", d["last_touched_nodes"], "body velocity", d["velocity"])
    assert rel < 1e-5 and d["updates"] == 20 and d["last_touched_nodes"] > 50 and np.abs(d["velocity"]).max() < 1e-9


def test_closed_system_keeps_its_momentum():
    """cfg.gravity = 0, a sticky sphere body flying into a fixed-corotated block clear of the walls, 40 substeps: sum m v of the particles plus
    mass v of the body keeps its start value within 4 x the relative drift the same block shows flying freely, with no collider, over the same
    40 substeps (both printed)."""
    speed, mass, n = 1.0, 8.0, 40
    sc = scenes.sphere_through_block_analytic(bits=6, block_cells=(12, 8, 12), radius_cells=5.0, gap_cells=-1.0, speed=speed, boundary="sticky", dt=4e-4, animate=False)
    assert sc["config"]["gravity"] == 0.0
    free = copy.deepcopy(sc)
    free["colliders"] = None
    free["models"][0]["v0"] = (speed, 0.0, 0.0)
    eng = build_engine(free)
    eng.initial_setup()
    p0 = eng.particle_momentum()["momentum"]
    eng.run_fixed(n, free["dt"])
    p1 = eng.particle_momentum()["momentum"]
    eng.close()
    drift_free = np.abs(p1 - p0).max() / np.abs(p0).max()
    col = sc["colliders"][0]
    col["body"] = dict(mass=mass, inertia=(0.01, 0.01, 0.01, 0.0, 0.0, 0.0), com=col["a"], gravity=False)
    eng = build_engine(sc)
    eng.initial_setup()
    start = eng.particle_momentum()["momentum"] + mass * eng.collider_body(0)["velocity"]
    eng.run_fixed(n, sc["dt"])
    d = eng.collider_body(0)
    end = eng.particle_momentum()["momentum"] + mass * d["velocity"]
    eng.close()
    drift = np.abs(end - start).max() / np.abs(start).max()
    print("closed system: relative drift", drift, "free flight", drift_free, "max mass ratio", d["max_mass_ratio"], "body velocity", d["velocity"])
    assert d["velocity"][0] < speed - 1e-3 and d["max_mass_ratio"] < 1.0                    # momentum did go over, and the coupling was in its stable range
    assert drift <= 4 * drift_free, (drift, drift_free)


# ---- 5. scenes and the gmpm driver --------------------------------------------------------------------------------------------------------------------
def test_scenes_ball_into_sand_and_floating_box():
    """The two demonstration scenes through build_engine ("body": {...} in a collider's dict) at a size that runs in a second, each body thrown
    down at 1 m/s so that 40 substeps show the material pushing back: both end slower than 40 substeps of free fall from that speed would leave them."""
    sc = scenes.ball_into_sand(bed_cells=(24, 8, 24), drop_cells=0.0, speed=1.0)
    eng = build_engine(sc)
    eng.initial_setup()
    m, i6, com = eng.shape_mass_properties("sphere", 8e3, a=sc["colliders"][0]["a"], radius=sc["colliders"][0]["radius"], api=eng.api)
    d0 = eng.collider_body(0)
    assert d0["mass"] == m and d0["gravity"] and np.array_equal(d0["position"], np.float32(sc["colliders"][0]["a"]).astype(np.float64))
    eng.run_fixed(40, sc["dt"])
    d = eng.collider_body(0)
    free = -1.0 + 40 * G64 * H
    print("ball_into_sand: v_y", d["velocity"][1], "free fall", free, "max mass ratio", d["max_mass_ratio"])
    assert d["updates"] == 40 and free < d["velocity"][1] < 0 and d["last_touched_nodes"] > 0 and d["max_mass_ratio"] < 0.5
    eng.close()
    sc = scenes.floating_box(pool_cells=(24, 20, 24), speed=1.0)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(40, sc["dt"])
    d = eng.collider_body(0)
    print("floating_box: v_y", d["velocity"][1], "free fall", free, "max mass ratio", d["max_mass_ratio"])
    assert d["updates"] == 40 and d["velocity"][1] > free and d["last_impulse"][1] > 0 and d["max_mass_ratio"] < 0.5
    eng.close()


def test_gmpm_body_and_output_bodies(tmp_path):
    """A "body" inside a "colliders" entry and simulation.output_bodies through the gmpm driver: bodies_frame[f].json holds the state the engine
    reaches when it is driven through the same substeps (the two single-block boxes of tests/test_gmpm_stress_gpu.py: deterministic)."""
    import json
    import os
    import subprocess
    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS, DT_DEFAULT, FC, FPS, FRAMES, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    from claymore_amd.engine import Engine
    g.build_host()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    col = {"shape": "sphere", "center": [10.5 / 64, 31.5 / 64, 31.5 / 64], "radius": 1.5 / 64, "type": "slip", "friction": 0.2, "velocity": [-2.0, 0.0, 0.0],
           "body": {"density": 4000.0, "gravity": False, "lock": "y rz"}}
    d = tmp_path / "bodies"
    d.mkdir()
    sim = {"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d), "output_bodies": True}
    (d / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "colliders": [col]}))
    subprocess.check_output([os.path.join(root, "claymore_amd", "host", "gmpm"), "-f", str(d / "scene.json")], text=True, timeout=300)
    start = [read_bgeo_attrs(frame(d, m, 0))[0] for m in range(len(MODELS))]
    eng = Engine(domain_bits=BITS, max_ppc=128)
    for mod, xyz in zip(MODELS, start):
        mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
        eng.init_model(mat, xyz, mod["velocity"], **({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {}))
    eng.set_collision_shape(0, "sphere", a=col["center"], radius=col["radius"], type=1, friction=0.2, trans_vel=col["velocity"])
    eng.set_collision_clock(True, 0.0)
    eng.set_collider_body(0, density=4000.0, gravity=False, lock="y rz")
    spf = np.float32(1.0) / np.float32(FPS)
    max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in MODELS)
    dt = eng.compute_dt(max_v0, 0.0, float(spf), DT_DEFAULT)
    eng.initial_setup()
    touched = 0
    for f in range(1, FRAMES + 1):
        t = np.float32(0.0)
        while t < spf:
            next_dt, _ = eng.substep(dt, float(t), float(spf), DT_DEFAULT)
            t = np.float32(t + np.float32(dt))
            dt = next_dt
        want = eng.collider_body(0)
        doc = json.loads((d / f"bodies_frame[{f}].json").read_text())
        got = doc["bodies"]["slot0"]
        assert doc["frame"] == f and got["updates"] == want["updates"] > 0 and got["last_touched_nodes"] == want["last_touched_nodes"]
        for key in ("position", "orientation", "velocity", "omega", "angular_momentum", "last_impulse", "last_angular_impulse"):
            assert np.array_equal(np.array(got[key]), want[key]), (f, key, got[key], want[key])
        assert got["velocity"][1] == 0.0 and got["omega"][2] == 0.0
        touched += want["last_touched_nodes"]
    eng.close()
    assert touched > 0                                                                      # (the body did meet material)

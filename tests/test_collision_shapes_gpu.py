"""Analytic collision shapes on the GPU (claymore_amd/csrc/mpm_collision_shapes.hpp; grid_update_collider_kernel<ShapeArgs>, carry_grid_kernel<true, ShapeArgs>,
mpm_test_collision_shape) against tests/collision_shape_model.py, which tests/test_collision_shapes_cpu.py judges on the CPU.  The grids are
injected through the checkpoint port of tests/test_grid_update_kernels_gpu.py: grid_update_model's 28-particle scene at bits 6 with 222
neighbour blocks in all 27 wall classes, the generator's finite tier.  Every comparison with the model is on uint32 bit patterns; computed
NaNs compare as NaNs (grid_update_model.canon), masses and skipped cells on their raw bits.

Mutations (built in a scratch copy, not committed) and the test that catches each.  The four in mpm_collision_shapes.hpp were run against
tests/test_collision_shapes_cpu.py::test_host_build_equals_the_float32_model_bit_for_bit on the x86 build, which failed for each; the same
statements run in test_device_query_equals_the_model and test_cell_by_cell here.  The two above the header were NOT run on an MI355X; the
tests named are the ones expected to fail, from reading the code:
  `inside_out` ignored (shape_query)                         ..._bit_for_bit[*-True] on the CPU; here test_device_query_equals_the_model[container]
  capsule clamp dropped (shape_capsule)                      ..._bit_for_bit[capsule-*] (the special points beyond both ends); test_cell_by_cell[capsule-*]
  box tie rule `>` -> `>=` (shape_box)                       ..._bit_for_bit[box-*] (nodes with |y - 32| == |z - 32|: the normal's axis); test_cell_by_cell[box-slip-*]
  `sdis < 0` instead of `<=` (shape_resolve)                 ..._bit_for_bit[halfspace-False-*], [box-False-*] (nodes ON the surface); test_cell_by_cell[halfspace-*-identity]
  slot order reversed (grid_cell(ShapeArgs))                 test_slots_act_in_order (the two orders give the model's two different grids)
  the clock advanced once per collider (with_collider)       test_run_fixed_equals_the_phase_level_loop (clock == the float32 sum of n dt) and
                                                             test_errors_and_the_clocks_book_keeping (two shapes, one grid update: T + dt)"""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest
from scipy.spatial import cKDTree

import ckpt_format as cf
import collision_shape_model as sm
import face_scenes as fs
import grid_update_model as gm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from parity_util import match

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, N, DX, DT = gm.G_BLOCKS, 1 << gm.BITS, sm.DX, 1e-4
GRAVITY, BOUNDARY = -9.8, 2
TYPES = {"sticky": 0, "slip": 1, "separate": 2}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def scene():
    prm = {"volume": scenes._vol(gm.BITS), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "collision_shape_cells", "bits": gm.BITS, "dt": DT, "config": {"max_ppc": 128, "gravity": GRAVITY, "boundary_blocks": BOUNDARY},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": fs.to_world(gm.scene_cells(), gm.BITS), "v0": (0.5, -1.0, 0.25), "params": prm}]}


class ShapeCtx:
    """One context of the scene, checkpointed right after set-up; colliders come and go, the injected grid comes from the checkpoint."""

    def __init__(self):
        self.eng = build_engine(scene())
        self.eng.initial_setup()
        self.ckpt = self.eng.save_checkpoint().copy()
        self.keys, _ = self.eng.dump_grid()
        self.nbc = len(self.keys)

    def install(self, colliders=(), field=None, t=0.0):
        """colliders: up to four model colliders or None (an empty slot); field: (collider, sdf, grad) or None.  The clock is left stopped at t."""
        if field is None:
            self.eng.set_collision_object(None)
        else:
            kw = sm.engine_kwargs(field[0])
            self.eng.set_collision_object(sdf=field[1], grad=field[2], **{k: kw[k] for k in ("type", "friction", "scale", "dsdt", "trans", "trans_vel", "omega", "rot_mat", "time")})
        cols = list(colliders) + [None] * (4 - len(colliders))
        for slot, c in enumerate(cols):
            self.eng.set_collision_shape(slot, None) if c is None else self.eng.set_collision_shape(slot, **sm.engine_kwargs(c))
        if field is not None or any(c is not None for c in cols):
            self.eng.set_collision_clock(False, float(t))

    def update(self, pattern, dt=DT):
        self.eng.load_checkpoint(cf.with_grid(self.ckpt, pattern))
        mv = np.float32(self.eng.grid_update(dt))
        keys, blocks = self.eng.dump_grid()
        assert np.array_equal(keys, self.keys)
        return mv, blocks

    def model(self, pattern, colliders, t=0.0, field=None, dt=DT):
        return sm.grid_update(self.keys, G, BOUNDARY, GRAVITY, dt, pattern.view(np.float32), colliders, t, DX, field=field)


@pytest.fixture(scope="module")
def ctx():
    c = ShapeCtx()
    assert c.nbc == 222 and sorted(map(tuple, c.keys.tolist())) == sorted(map(tuple, gm.scene_keys().tolist()))
    yield c
    c.eng.close()


def assert_grid(pat, out, live, want):
    ob = gm.bits(out)
    assert np.array_equal(ob[:, 0], pat[:, 0]), "mass channel changed"
    for ch in range(4):
        assert np.array_equal(ob[:, ch][~live], pat[:, ch][~live]), f"a skipped cell's channel {ch} changed"
    for ch in (1, 2, 3):
        bad = (gm.canon(out[:, ch]) != gm.canon(want[:, ch])) & live
        assert not bad.any(), (ch, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- 1. mpm_test_collision_shape -----------------------------------------------------------------------------------------------------------
def device_query(c, t, X):
    from test_collision_shapes_cpu import ffi_pair
    obj, sh = ffi_pair(c)
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(X), 4), np.float32)
    assert _ffi.load_hip().test_collision_shape(C.byref(obj), C.byref(sh), float(t), DX, ptr(X), len(X), ptr(out), 0) == 0
    return out[:, 0], out[:, 1:]


@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("name", sorted(sm.SHAPES))
def test_device_query_equals_the_model(name, moved):
    """sdis and n on the device, bit for bit, on the points of the CPU test: 4096 seeded domain points and the special points (n = 0, sdis == 0,
    box ties and centre, the capsule's clamp at both ends, NaN), identity pose and the moved, turned, scaled, growing pose at T = 0.37; the
    `container` is the inside_out case."""
    from test_collision_shapes_cpu import domain_points_of
    c = sm.make(name, moved)
    t = sm.T_MOVED if moved else 0.0
    sp = sm.special_points(c)
    X = np.concatenate([sm.seeded_points(7), sp if not moved else domain_points_of(c, t, sp)])
    sd, n = device_query(c, t, X)
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    sdm, nm = sm.query(c, xm)
    assert np.array_equal(gm.canon(sd), gm.canon(sdm)), np.argwhere(gm.canon(sd) != gm.canon(sdm))[:4].tolist()
    assert np.array_equal(gm.canon(n), gm.canon(nm)), np.argwhere(gm.canon(n) != gm.canon(nm))[:4].tolist()
    assert 0.02 < (sdm <= 0).mean() < 0.98 and np.isnan(sdm[-3:]).all()


# ---- 2. cell by cell -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("typ", sorted(TYPES))
@pytest.mark.parametrize("name", sm.KIND_CASES)
def test_cell_by_cell(ctx, name, typ, moved):
    """grid_update_collider_kernel<ShapeArgs> with one shape on a generated grid: every velocity and the returned (doubled) maximum equal the model bit for
    bit; the shape cuts interior and wall-zone blocks and touches between 10 % and 90 % of the live cells (checked on the model)."""
    c = sm.make(name, moved, type=TYPES[typ], friction=0.3)
    t = sm.T_MOVED if moved else 0.0
    ctx.install([c], t=t)
    for seed in (1, 2):
        pat = gm.generate(ctx.nbc, seed, "finite")[0]
        live, want, mx, hits = ctx.model(pat, [c], t)
        share = hits[0].sum() / live.sum()
        cut = hits[0].any(axis=1) & (live & ~hits[0]).any(axis=1)
        interior = np.all(gm.wall_class(ctx.keys, G, BOUNDARY) == 1, axis=1)
        assert 0.10 <= share <= 0.90 and (cut & interior).any() and (cut & ~interior).any(), (share, int((cut & interior).sum()), int((cut & ~interior).sum()))
        mv, out = ctx.update(pat)
        assert_grid(pat, out, live, want)
        assert gm.bits(mv) == gm.bits(mx) == gm.bits(gm.collision_q32(want[:, 1], want[:, 2], want[:, 3])[live].max()), (float(mv), float(mx))
        assert ctx.eng.collision_time() == float(np.float32(t))                    # (a stopped clock stays)


# ---- 3. against the level-set kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", sorted(TYPES))
@pytest.mark.parametrize("name", ["halfspace", "box"])
def test_shape_kernel_equals_the_level_set_kernel(ctx, name, typ):
    """The axis half-space and the box at identity pose on one injected grid: through mpm_set_collision_object with the field sampled from the
    model (grid_update_collider_kernel<CollisionArgs>) and through the shape (grid_update_collider_kernel<ShapeArgs>).  Bit-identical at the nodes inside query_sdf's box;
    outside it the level set acts on nothing, the shape on every node - those cells equal the model."""
    c = sm.make(name, type=TYPES[typ], friction=0.3, trans_vel=(0.25, -0.5, 0.125), omega=(0.5, 1.0, -0.25))
    sdf, grad = sm.sample_field(c, N, DX)
    pat = gm.generate(ctx.nbc, 3, "finite")[0]
    ctx.install([], field=(c, sdf, grad))
    _, via_field = ctx.update(pat)
    ctx.install([c])
    _, via_shape = ctx.update(pat)
    live, want, _, hits = ctx.model(pat, [c])
    nd = gm.node_coords(ctx.keys)
    inbox = np.all((nd >= 4 * BOUNDARY) & (nd < 4 * (G - BOUNDARY)), axis=1)
    assert (hits[0] & inbox).sum() > 100 and (hits[0] & ~inbox).sum() > 100
    for ch in range(4):
        assert np.array_equal(gm.bits(via_field[:, ch])[inbox], gm.bits(via_shape[:, ch])[inbox]), ch
    assert_grid(pat, via_shape, live, want)
    assert (gm.bits(via_field[:, 1:]) != gm.bits(via_shape[:, 1:])).any(axis=1)[hits[0] & ~inbox].any()


# ---- 4. slots -----------------------------------------------------------------------------------------------------------------------------------
def test_slots_act_in_order(ctx):
    """Two overlapping shapes in both orders give the model's two different grids; a shape beside a level-set object applies the field first;
    emptying a slot restores the one-collider grid, emptying all of them the plain kernel's bits and maximum."""
    a = sm.make("halfspace_tilted", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    b = sm.make("sphere", type=2, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    pat = gm.generate(ctx.nbc, 4, "finite")[0]
    ctx.install([])
    mv_plain, plain = ctx.update(pat)
    got, want = {}, {}
    for order, cols in (("ab", [a, b]), ("ba", [b, a]), ("a-b", [a, None, None, b]), ("a", [a]), ("-b", [None, b])):
        ctx.install(cols)
        mv, out = ctx.update(pat)
        live, w, mx, hits = ctx.model(pat, cols)
        assert_grid(pat, out, live, w)
        assert gm.bits(mv) == gm.bits(mx)
        got[order], want[order] = gm.bits(out), gm.bits(w)
    both = (want["ab"] != want["ba"]).any(axis=1)
    assert both.sum() > 100 and np.array_equal(got["ab"], got["a-b"]) and not np.array_equal(got["ab"], got["a"]) and not np.array_equal(got["ab"], got["-b"])
    # a level-set object beside a shape: the field first
    f = sm.make("box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    sdf, grad = sm.sample_field(f, N, DX)
    ctx.install([b], field=(f, sdf, grad))
    mv, out = ctx.update(pat)
    live, w, mx, hits = ctx.model(pat, [b], field=(f, sdf, grad))
    assert (hits[0] & hits[1]).sum() > 100
    assert_grid(pat, out, live, w)
    assert gm.bits(mv) == gm.bits(mx)
    # (the other order is another grid: the model with the sphere in front of the box, compared inside query_sdf's box where field and shape agree)
    _, rev, _, _ = ctx.model(pat, [b, f])
    nd = gm.node_coords(ctx.keys)
    inbox = np.all((nd >= 4 * BOUNDARY) & (nd < 4 * (G - BOUNDARY)), axis=1)
    assert ((gm.bits(rev[:, 1:]) != gm.bits(w[:, 1:])).any(axis=1) & inbox).sum() > 50
    # emptying
    ctx.eng.set_collision_object(None)
    _, out = ctx.update(pat)
    assert np.array_equal(gm.bits(out), got["-b"])                               # (the field gone: the sphere alone, whatever its slot)
    ctx.install([a, b])
    ctx.eng.set_collision_shape(1, None)
    ctx.eng.set_collision_clock(False, 0.0)
    _, out = ctx.update(pat)
    assert np.array_equal(gm.bits(out), got["a"])
    ctx.eng.set_collision_shape(0, None)
    mv, out = ctx.update(pat)
    assert np.array_equal(gm.bits(out), gm.bits(plain)) and gm.bits(mv) == gm.bits(mv_plain)
    with pytest.raises(EngineError):
        ctx.eng.collision_time()                                                 # nothing installed any more


# ---- 5. / 6. the carry-over and the physics ---------------------------------------------------------------------------------------------------------
from test_collision_clock_cpu import SCENE, STEPS  # noqa: E402  (the dense scene and its substep count, chosen on the oracle's level-set run)

MOTION = {"omega": (10.0, -5.0, 15.0), "dsdt": 2.0, "rot_mat": sm.TILT}
# The sparse twin is in contact from the first substep (gap -3 cells).  The substep count comes from the oracle's level-set run of the same scene
# (CPU, slip, this motion): the particles whose position differs from the free run's number 9 / 9 / 16 / 20 / 22 after 10 / 20 / 40 / 60 / 90
# substeps - by 60 the sphere has reached nearly all it ever reaches (and tests/test_collision_clock_gpu.py runs the level-set original that long).
SPARSE_STEPS = 60


def sparse_analytic(**kw):
    """tests/test_collision_clock_gpu.py's sparse_scene (48 particles, no two on one grid node: the engine is deterministic on it) with the
    sphere as a shape."""
    sc = scenes.sphere_through_block_analytic(**{**SCENE, "block_cells": (16, 12, 16), "gap_cells": -3.0}, **kw)
    q = np.rint(sc["models"][0]["xyz"].astype(np.float64) * 64 * 4).astype(np.int64)
    sc["models"][0]["xyz"] = np.ascontiguousarray(sc["models"][0]["xyz"][(q % 16 == 15).all(axis=1)])
    sc["models"][0]["v0"] = (-0.5, 0.25, -0.125)
    assert sc["models"][0]["xyz"].shape == (48, 3)
    return sc


def f32_sum(t0, dts):
    t = np.float32(t0)
    for d in dts:
        t = np.float32(t + np.float32(d))
    return float(t)


def sorted_rows(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x[np.lexsort(x.T[::-1])].view(np.uint32)


def grid_rows(eng):
    keys, blocks = eng.dump_grid()
    order = np.lexsort(keys.T[::-1])
    return keys[order], gm.bits(blocks[order])


def run(sc, n, how):
    eng = build_engine(sc)
    eng.initial_setup()
    if how == "fused":
        eng.run_fixed(n, sc["dt"])
    else:
        for _ in range(n):
            eng.grid_update(sc["dt"])
            eng.g2p2g(sc["dt"], sc["dt"])
            eng.rebuild_partition()
    out = (sorted_rows(eng.retrieve_positions(0)),) + grid_rows(eng) + (eng.collision_time() if sc.get("colliders") else None,)
    eng.close()
    return out


@pytest.mark.parametrize("sync_interval", [1, 8])
@pytest.mark.parametrize("boundary", ["slip", "separate"])
def test_run_fixed_equals_the_phase_level_loop(boundary, sync_interval):
    """mpm_run_fixed(n) - every grid update but the first rides on carry_grid_kernel<true, ShapeArgs> - against grid update, g2p2g, rebuild phase by phase
    (grid_update_collider_kernel<ShapeArgs>) with a moving, turning, growing analytic sphere and a running clock: positions, the grid the run leaves behind
    and the clock bit for bit."""
    sc = sparse_analytic(boundary=boundary, **MOTION)
    sc["config"]["sync_interval"] = sync_interval
    p1, p2, fused = run(sc, SPARSE_STEPS, "phase"), run(sc, SPARSE_STEPS, "phase"), run(sc, SPARSE_STEPS, "fused")
    for a, b in zip(p1[:3], p2[:3]):
        assert np.array_equal(a, b), "the scene is not deterministic: nothing to compare"
    free = run({**sc, "colliders": None}, SPARSE_STEPS, "phase")
    moved = len({tuple(r) for r in p1[0].tolist()} - {tuple(r) for r in free[0].tolist()})
    assert moved >= 12, moved                                                    # (the sphere acted on a quarter of the particles at least)
    assert fused[3] == p1[3] == f32_sum(0.0, [sc["dt"]] * SPARSE_STEPS)
    for what, f, p in zip(("positions", "grid keys", "grid"), fused[:3], p1[:3]):
        assert f.shape == p.shape and np.array_equal(f, p), (what, int((f != p).sum()) if f.shape == p.shape else (f.shape, p.shape))


@pytest.mark.parametrize("boundary", ["sticky", "slip", "separate"])
def test_moving_analytic_sphere_displaces_the_block(boundary):
    """tests/test_collision_clock_cpu.py's dense scene and substep count with the sphere as a shape, through mpm_run_fixed: no particle ends deeper
    than 1.25 dx inside the moved sphere, and at least 10 % of the particles lie farther than one cell from every particle of the held-clock
    run (the rule and measure of test_oracle_moving_sphere_displaces_the_block)."""
    sc = scenes.sphere_through_block_analytic(boundary=boundary, **SCENE)
    held = scenes.sphere_through_block_analytic(boundary=boundary, animate=False, **SCENE)
    out = {}
    for name, s in (("moving", sc), ("held", held)):
        eng = build_engine(s)
        eng.initial_setup()
        eng.run_fixed(STEPS, s["dt"])
        out[name] = (eng.retrieve_positions(0).astype(np.float64), eng.collision_time())
        eng.close()
    (xm, T), (xh, Th) = out["moving"], out["held"]
    assert Th == 0.0 and T == f32_sum(0.0, [sc["dt"]] * STEPS)
    col = sc["colliders"][0]
    centre = np.array(col["a"], dtype=np.float64) + np.array(col["trans_vel"], dtype=np.float64) * T
    depth = SCENE["radius_cells"] * DX - np.linalg.norm(xm - centre, axis=1)
    away = cKDTree(xh).query(xm)[0] / DX
    print(boundary, "deepest particle / dx:", depth.max() / DX, "share farther than one cell:", (away > 1.0).mean())
    assert depth.max() < 1.25 * DX, depth.max() / DX
    assert (away > 1.0).mean() >= 0.10, (away > 1.0).mean()


# ---- 7. a group of two ------------------------------------------------------------------------------------------------------------------------------
def test_group_of_two_equals_one_context_with_a_moving_shape():
    """Two ranks (mpm_group_run_fixed, in-process transport, the same colliders and clock on both) against one context holding the whole block:
    1e-6 relative, the bound of test_group_of_two_equals_one_context_with_a_moving_object's docstring (the oracle that test also compares with
    knows no shapes); the clocks agree exactly and the ranks did exchange halo blocks."""
    sc = sparse_analytic(boundary="slip", **MOTION)
    one = build_engine(sc)
    one.initial_setup()
    one.run_fixed(SPARSE_STEPS, sc["dt"])
    x1, t1 = one.retrieve_positions(0), one.collision_time()
    one.close()
    world = 2
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            ranks[r].initial_setup()
            ranks[r].run_fixed(SPARSE_STEPS, sc["dt"])
            out[r] = (ranks[r].eng.retrieve_positions(0), ranks[r].eng.collision_time(), sum(ranks[r].send_counts))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    for r in ranks:
        r.close()
    assert not errors, errors
    assert all(o[1] == t1 for o in out) and min(o[2] for o in out) > 0
    xg = np.concatenate([o[0] for o in out])
    idx, _ = match(x1.astype(np.float64), xg.astype(np.float64))
    rel = (np.abs(xg[idx].astype(np.float64) - x1).max(axis=1) / np.abs(x1).max(axis=1)).max()
    print("group vs single", rel)
    assert rel < 1e-6, rel


# ---- 8. errors and the clock's book-keeping -------------------------------------------------------------------------------------------------------
def test_errors_and_the_clocks_book_keeping(ctx):
    eng = ctx.eng
    ctx.install([])
    ok = dict(kind="sphere", a=(0.5, 0.5, 0.5), radius=0.1)
    nan = float("nan")
    bad = [dict(ok, slot=-1), dict(ok, slot=4), dict(ok, kind=0), dict(ok, kind=5), dict(ok, type=-1), dict(ok, type=3), dict(ok, radius=0.0), dict(ok, radius=-1.0),
           dict(ok, radius=float("inf")), dict(ok, radius=nan), dict(ok, a=(nan, 0.5, 0.5)),
           dict(kind="capsule", a=(0.5, 0.5, 0.5), b=(0.5, 0.5, 0.5), radius=0.1), dict(kind="capsule", a=(0.1, 0.5, 0.5), b=(0.5, 0.5, 0.5), radius=0.0),
           dict(kind="capsule", a=(0.1, 0.5, 0.5), b=(0.5, nan, 0.5), radius=0.1),
           dict(kind="box", a=(0.5, 0.5, 0.5), b=(0.1, 0.0, 0.1)), dict(kind="box", a=(0.5, 0.5, 0.5), b=(0.1, -0.1, 0.1)), dict(kind="box", a=(0.5, 0.5, 0.5), b=(0.1, float("inf"), 0.1)),
           dict(kind="box", a=(0.5, 0.5, 0.5), b=(0.1, nan, 0.1)),
           dict(kind="halfspace", a=(0.5, 0.5, 0.5), b=(0.0, 0.0, 0.0)), dict(kind="halfspace", a=(0.5, 0.5, 0.5), b=(0.0, float("inf"), 0.0)),
           dict(kind="halfspace", a=(0.5, 0.5, 0.5), b=(0.0, nan, 1.0))]
    for kw in bad:
        kw = dict(kw)
        slot = kw.pop("slot", 0)
        with pytest.raises(EngineError) as e:
            eng.set_collision_shape(slot, **kw)
        assert e.value.code == _ffi.MPM_ERR_INVALID and "collision shape" in str(e.value), (kw, str(e.value))
    for kw, word in ((dict(ok, radius=0.0), "radius"), (dict(kind="box", a=(0, 0, 0), b=(1, 0, 1)), "half extents"), (dict(kind="halfspace", b=(0, 0, 0)), "normal"),
                     (dict(ok, type=7), "boundary type"), (dict(ok, kind=9), "kind"), (dict(ok, a=(nan, 0, 0)), "NaN in a"),
                     (dict(kind="capsule", a=(0.5, 0.5, 0.5), b=(0.5, 0.5, 0.5), radius=0.1), "coincide")):
        with pytest.raises(EngineError) as e:
            eng.set_collision_shape(0, **kw)
        assert word in str(e.value), (word, str(e.value))
    # nothing installed (every call above failed): the clock has no owner
    with pytest.raises(EngineError) as e:
        eng.set_collision_clock(True, 0.0)
    assert e.value.code == _ffi.MPM_ERR_INVALID
    # install sets the clock to obj->time, stopped; a second install does so again; a removal stops it
    eng.set_collision_shape(0, **dict(ok, time=0.25))
    assert eng.collision_time() == 0.25 and not eng.collision_clock_running()
    eng.set_collision_clock(True, 0.5)
    eng.set_collision_shape(2, **dict(ok, a=(0.25, 0.5, 0.5), time=0.125))
    assert eng.collision_time() == 0.125 and not eng.collision_clock_running()
    eng.set_collision_clock(True, 0.5)
    # one clock, advanced once per grid update whatever the number of colliders; a checkpoint load keeps the shapes and the clock
    pat = gm.generate(ctx.nbc, 9, "finite")[0]
    mv, out = ctx.update(pat)
    assert eng.collision_time() == f32_sum(0.5, [DT]) and eng.collision_clock_running()
    cols = [sm.collider(**dict(ok, time=0.0)), None, sm.collider(**dict(ok, a=(0.25, 0.5, 0.5)))]
    live, want, mx, _ = ctx.model(pat, cols, t=0.5)
    assert_grid(pat, out, live, want)
    eng.set_collision_shape(2, None)
    assert not eng.collision_clock_running() and eng.collision_time() == f32_sum(0.5, [DT])
    eng.set_collision_shape(0, None)
    with pytest.raises(EngineError):
        eng.collision_time()


# ---- 9. the gmpm driver ---------------------------------------------------------------------------------------------------------------------------
def test_gmpm_colliders_scene_equals_the_engine(tmp_path):
    """A "colliders" scene - a sticky box and a moving slip sphere - through the gmpm driver for two frames: its positions are the ones of the same
    scene driven through Engine, bit for bit (tests/test_gmpm_stress_gpu.py's two single-block bodies, on which the engine is deterministic)."""
    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS, DT_DEFAULT, FC, FPS, FRAMES, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    cols = [{"shape": "box", "center": [8 / 64, 19.5 / 64, 19.5 / 64], "half_extents": [0.75 / 64, 3 / 64, 3 / 64], "type": "sticky"},
            {"shape": "sphere", "center": [10.5 / 64, 31.5 / 64, 31.5 / 64], "radius": 1.5 / 64, "type": "slip", "friction": 0.2, "velocity": [-2.0, 0.0, 0.0]}]
    d = tmp_path / "colliders"
    d.mkdir()
    sim = {"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d)}
    (d / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "colliders": cols}))
    log = subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(d / "scene.json")], text=True, timeout=300)
    assert "has 2 colliders, clock running" in log
    start = [read_bgeo_attrs(frame(d, m, 0))[0] for m in range(len(MODELS))]

    def drive(colliders):
        eng = Engine(domain_bits=BITS, max_ppc=128)
        for mod, xyz in zip(MODELS, start):
            mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
            eng.init_model(mat, xyz, mod["velocity"], **({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {}))
        if colliders:
            eng.set_collision_shape(0, "box", a=cols[0]["center"], b=cols[0]["half_extents"], type=0, trans=cols[0]["center"])
            eng.set_collision_shape(1, "sphere", a=cols[1]["center"], radius=cols[1]["radius"], type=1, friction=0.2, trans=cols[1]["center"], trans_vel=cols[1]["velocity"])
            eng.set_collision_clock(True, 0.0)
        spf = np.float32(1.0) / np.float32(FPS)
        max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in MODELS)
        dt = eng.compute_dt(max_v0, 0.0, float(spf), DT_DEFAULT)
        eng.initial_setup()
        frames = []
        for _ in range(FRAMES):
            t = np.float32(0.0)
            while t < spf:
                next_dt, _ = eng.substep(dt, float(t), float(spf), DT_DEFAULT)
                t = np.float32(t + np.float32(dt))
                dt = next_dt
            frames.append([sorted_rows(eng.retrieve_positions(m)) for m in range(len(MODELS))])
        eng.close()
        return frames

    want, free = drive(True), drive(False)
    for f in range(1, FRAMES + 1):
        for m in range(len(MODELS)):
            got = sorted_rows(read_bgeo_attrs(frame(d, m, f))[0])
            assert np.array_equal(got, want[f - 1][m]), (f, m)
    for m in range(len(MODELS)):
        assert not np.array_equal(want[-1][m], free[-1][m]), f"the collider of model {m} touched nothing"

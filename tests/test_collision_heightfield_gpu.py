"""The heightfield collider on the GPU (claymore_amd/csrc/mpm_collision_heightfield.hpp; grid_update_collider_kernel<TerrainArgs>, carry_grid_kernel<true, TerrainArgs>,
mpm_test_collision_heightfield) against tests/heightfield_model.py, which tests/test_collision_heightfield_cpu.py judges on the CPU.  The grids
are injected through the checkpoint port of tests/test_collision_shapes_gpu.py (its ShapeCtx): grid_update_model's 28-particle scene at bits 6
with 222 neighbour blocks in all 27 wall classes, the generator's finite tier.  Every comparison with the model is on uint32 bit patterns;
computed NaNs compare as NaNs (grid_update_model.canon).  No test leaves the table's footprint unguarded: the out-of-footprint and NaN points
are answered by the query's own range check before any load (proved on the CPU, tests 2 and 5 there)."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import collision_shape_model as sm
import grid_update_model as gm
import heightfield_model as hm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from parity_util import match
from test_collision_clock_cpu import STEPS
from test_collision_shapes_gpu import BOUNDARY, DT, DX, G, GRAVITY, N, TYPES, ShapeCtx, assert_grid, f32_sum, grid_rows, ptr, sorted_rows, sparse_analytic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TerrainCtx(ShapeCtx):
    """ShapeCtx whose slots take shape and heightfield colliders alike, with heightfield_model.grid_update as the model."""

    def install(self, colliders=(), field=None, t=0.0):
        if field is None:
            self.eng.set_collision_object(None)
        else:
            kw = sm.engine_kwargs(field[0]) if field[0]["kind"] != "heightfield" else hm.engine_kwargs(field[0])
            self.eng.set_collision_object(sdf=field[1], grad=field[2], **{k: kw[k] for k in ("type", "friction", "scale", "dsdt", "trans", "trans_vel", "omega", "rot_mat", "time")})
        cols = list(colliders) + [None] * (4 - len(colliders))
        for slot, c in enumerate(cols):
            if c is None:
                self.eng.set_collision_shape(slot, None)
            elif c["kind"] == "heightfield":
                self.eng.set_collision_heightfield(slot, **hm.engine_kwargs(c))
            else:
                self.eng.set_collision_shape(slot, **sm.engine_kwargs(c))
        if field is not None or any(c is not None for c in cols):
            self.eng.set_collision_clock(False, float(t))

    def model(self, pattern, colliders, t=0.0, field=None, dt=DT):
        return hm.grid_update(self.keys, G, BOUNDARY, GRAVITY, dt, pattern.view(np.float32), colliders, t, DX, field=field)


@pytest.fixture(scope="module")
def ctx():
    c = TerrainCtx()
    assert c.nbc == 222 and sorted(map(tuple, c.keys.tolist())) == sorted(map(tuple, gm.scene_keys().tolist()))
    yield c
    c.eng.close()


def wide_terrain(moved=False, **kw):
    """81 x 81 samples 0.013 apart from (-0.02, -0.02): a table whose cells are no multiple of dx, wider than the domain."""
    o = (-0.02, -0.02)
    return hm.heightfield(hm.terrain(81, 81, 3, 0.013, origin=o), origin=o, spacing=0.013, **{**(sm.MOVED if moved else {}), **kw})


TERRAINS = {"dx": lambda moved=False, **kw: hm.make("65x65", moved, **kw), "0.013": wide_terrain}


def inbox_nodes(keys):
    nd = gm.node_coords(keys)
    return np.all((nd >= 4 * BOUNDARY) & (nd < 4 * (G - BOUNDARY)), axis=1)


# ---- 1. mpm_test_collision_heightfield ---------------------------------------------------------------------------------------------------------
def device_query(c, t, X):
    from test_collision_heightfield_cpu import ffi_triple
    obj, hf, H = ffi_triple(c)
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(X), 4), np.float32)
    assert _ffi.load_hip().test_collision_heightfield(C.byref(obj), C.byref(hf), ptr(H), float(t), ptr(X), len(X), ptr(out), 0) == 0
    return out[:, 0], out[:, 1:]


@pytest.mark.parametrize("inside_out", [False, True], ids=["floor", "ceiling"])
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("name", ["2x2", "5x3", "65x65", "33x17"])
def test_device_query_equals_the_model(name, moved, inside_out):
    """sdis and n on the device, bit for bit, on the points of the CPU test: 4096 seeded domain points and the special points (on samples, on
    cell edges, u = 0 and u = nx - 1 and one float outside each, on the surface, NaN), identity pose and the moved pose at T = 0.37."""
    from test_collision_heightfield_cpu import query_points
    c = hm.make(name, moved, inside_out=inside_out)
    t = sm.T_MOVED if moved else 0.0
    X = query_points(c, t, moved)
    sd, n = device_query(c, t, X)
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    sdm, nm = hm.query(c, xm)
    assert np.array_equal(gm.canon(sd), gm.canon(sdm)), np.argwhere(gm.canon(sd) != gm.canon(sdm))[:4].tolist()
    assert np.array_equal(gm.canon(n), gm.canon(nm)), np.argwhere(gm.canon(n) != gm.canon(nm))[:4].tolist()
    assert 0.02 < (sdm <= 0).mean() < 0.98 and np.isnan(sdm[-3:]).all()


# ---- 2. cell by cell -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("typ", sorted(TYPES))
@pytest.mark.parametrize("name", sorted(TERRAINS))
def test_cell_by_cell(ctx, name, typ, moved):
    """grid_update_collider_kernel<TerrainArgs> with one heightfield (a seeded ramp plus bumps: 65 x 65 at spacing dx, and 81 x 81 at spacing 0.013) on a
    generated grid: every velocity and the returned (doubled) maximum equal the model bit for bit.  On the model alone: the surface touches
    between 10 % and 90 % of the live cells and cuts interior and wall-zone blocks."""
    c = TERRAINS[name](moved, type=TYPES[typ], friction=0.3)
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
        assert ctx.eng.collision_time() == float(np.float32(t))


# ---- 3. against the level-set kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_heightfield_kernel_equals_the_level_set_kernel(ctx, typ):
    """The 65 x 65 terrain at identity pose (origin 0, spacing dx: its samples sit on the nodes) on one injected grid: through
    mpm_set_collision_object with the field sampled from the model (heightfield_model.sample_field) and through the heightfield.  Bit-identical
    at the nodes inside query_sdf's box; the remaining cells equal the model."""
    c = hm.make("65x65", type=TYPES[typ], friction=0.3, trans_vel=(0.25, -0.5, 0.125), omega=(0.5, 1.0, -0.25))
    sdf, grad = hm.sample_field(c, N, DX)
    pat = gm.generate(ctx.nbc, 3, "finite")[0]
    ctx.install([], field=(c, sdf, grad))
    _, via_field = ctx.update(pat)
    ctx.install([c])
    _, via_hf = ctx.update(pat)
    live, want, _, hits = ctx.model(pat, [c])
    inbox = inbox_nodes(ctx.keys)
    assert (hits[0] & inbox).sum() > 100 and (hits[0] & ~inbox).sum() > 100
    for ch in range(4):
        assert np.array_equal(gm.bits(via_field[:, ch])[inbox], gm.bits(via_hf[:, ch])[inbox]), ch
    assert_grid(pat, via_hf, live, want)
    assert (gm.bits(via_field[:, 1:]) != gm.bits(via_hf[:, 1:])).any(axis=1)[hits[0] & ~inbox].any()


# ---- 4. a flat table is the half-space ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", sorted(TYPES))
@pytest.mark.parametrize("case", ["65x65-identity", "9x9-moved"])
def test_flat_table_equals_the_halfspace_shape_kernel(ctx, case, typ):
    """A table of constant height 32 dx against the shape halfspace(a = (., 32 dx, .), b = +y) on the whole grid: grid_update_collider_kernel<TerrainArgs> and
    grid_update_collider_kernel<ShapeArgs> leave the same bits in every channel and return the same maximum.  65 x 65 samples on the nodes at identity
    pose; 9 x 9 samples one unit apart about the domain at the moved pose (every node's material point lies in its footprint)."""
    cst, moved = np.float32(32 * DX), case.endswith("moved")
    mv = sm.MOVED if moved else {}
    t = sm.T_MOVED if moved else 0.0
    kw = dict(type=TYPES[typ], friction=0.3, **mv)
    hf = hm.heightfield(np.full((9, 9), cst, np.float32), origin=(-4.0, -4.0), spacing=1.0, **kw) if moved else hm.heightfield(np.full((65, 65), cst, np.float32), spacing=DX, **kw)
    hs = sm.collider("halfspace", a=(0.25, cst, 0.75), b=(0.0, 1.0, 0.0), **kw)
    pat = gm.generate(ctx.nbc, 5, "finite")[0]
    live, want, mx, hits = ctx.model(pat, [hf], t)
    assert 0.10 <= hits[0].sum() / live.sum() <= 0.90
    ctx.install([hf], t=t)
    mv_hf, out_hf = ctx.update(pat)
    ctx.install([hs], t=t)
    mv_hs, out_hs = ctx.update(pat)
    assert np.array_equal(gm.bits(out_hf), gm.bits(out_hs)) and gm.bits(mv_hf) == gm.bits(mv_hs) == gm.bits(mx)
    assert_grid(pat, out_hf, live, want)


# ---- 5. slots -----------------------------------------------------------------------------------------------------------------------------------
def test_slots_mix_shapes_and_heightfields_in_order(ctx):
    """Sphere, heightfield, box in slots 0, 1, 2 and with the outer two exchanged: each order gives the model's grid for that order, and the two
    differ.  Two heightfields in two slots.  A shape installed over a heightfield and back again.  A level-set object beside a heightfield: the
    field first.  Emptying every slot restores the plain kernel's bits and maximum."""
    s = sm.make("sphere", type=2, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    b = sm.make("box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    h = hm.make("65x65", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    h2 = wide_terrain(type=2, friction=0.1, inside_out=True, trans_vel=(0.0, -0.25, 0.0))
    pat = gm.generate(ctx.nbc, 4, "finite")[0]
    ctx.install([])
    mv_plain, plain = ctx.update(pat)

    def check(cols, field=None):
        ctx.install(cols, field=field)
        mv, out = ctx.update(pat)
        live, w, mx, hits = ctx.model(pat, cols, field=field)
        assert_grid(pat, out, live, w)
        assert gm.bits(mv) == gm.bits(mx)
        return gm.bits(out), gm.bits(w), hits

    shb, w_shb, hits = check([s, h, b])
    bhs, w_bhs, _ = check([b, h, s])
    assert (hits[0] & hits[1]).sum() > 50 and (hits[1] & hits[2]).sum() > 50
    assert (w_shb != w_bhs).any(axis=1).sum() > 50 and not np.array_equal(shb, bhs)
    hh, _, hits = check([h, None, None, h2])
    assert (hits[0] & hits[1]).sum() > 50
    h2h, _, _ = check([h2, h])
    assert not np.array_equal(hh, h2h)
    # a shape over a heightfield and back again (slot 1)
    ctx.install([s, h, b])
    ctx.eng.set_collision_shape(1, **sm.engine_kwargs(b))
    ctx.eng.set_collision_clock(False, 0.0)
    _, out = ctx.update(pat)
    live, w, _, _ = ctx.model(pat, [s, b, b])
    assert_grid(pat, out, live, w)
    ctx.eng.set_collision_heightfield(1, **hm.engine_kwargs(h))
    ctx.eng.set_collision_clock(False, 0.0)
    _, out = ctx.update(pat)
    assert np.array_equal(gm.bits(out), shb)
    # a level-set object beside a heightfield: the field first
    f = sm.make("box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    sdf, grad = sm.sample_field(f, N, DX)
    _, _, hits = check([None, h], field=(f, sdf, grad))
    assert (hits[0] & hits[1]).sum() > 50
    # emptying: the field, then every slot (a heightfield slot through mpm_set_collision_shape(NULL) too)
    ctx.eng.set_collision_object(None)
    ctx.eng.set_collision_shape(1, None)
    mv, out = ctx.update(pat)
    assert np.array_equal(gm.bits(out), gm.bits(plain)) and gm.bits(mv) == gm.bits(mv_plain)
    with pytest.raises(EngineError):
        ctx.eng.collision_time()                                                 # nothing installed any more


# ---- 6. the carry-over --------------------------------------------------------------------------------------------------------------------------
def sparse_terrain(boundary="slip", **kw):
    """tests/test_collision_shapes_gpu.py's sparse twin of test_collision_clock_cpu's SCENE (48 particles every fourth cell, no two on one grid
    node: the engine is deterministic while that lasts) with the sphere replaced by a terrain under the block's LOWEST particle layer only:
    the float atomics of P2G make a denser contact, which drives particles onto shared nodes, irreproducible from run to run.
    The layers sit at y = 27.75, 31.75 and 35.75 cells and fly at v0 = (-0.5, 0.25, -0.125); the surface lies between 27.5 and 29.5 cells
    under the block - node row 27 of every lowest-layer particle is below it, node rows 31 .. 33 of the next layer are above - and rises with
    the clock at the layers' own 0.25, so the lowest layer slides on it for the whole run while the others never touch it.  A slip surface
    that is nearly tangent to the relative velocity changes a velocity by a few hundredths: over STEPS substeps (0.16 s) no two particles
    come closer than three cells on every axis, no node ever receives two contributions, and the float atomics of P2G have nothing to reorder."""
    sc = sparse_analytic(boundary=boundary)
    X, Z = np.meshgrid(np.arange(N + 1) * DX, np.arange(N + 1) * DX, indexing="ij")
    heights = (28.5 * DX + 0.04 * (X - 0.5) + 0.025 * (Z - 0.5) + 0.5 * DX * np.sin(9 * X + 1.0) * np.cos(7 * Z + 2.0)).astype(np.float32)
    x = sc["models"][0]["xyz"].astype(np.float64) / DX
    assert sorted(set(np.round(x[:, 1], 2))) == [27.75, 31.75, 35.75]
    under = heights[int(x[:, 0].min()) - 8:int(x[:, 0].max()) + 4, int(x[:, 2].min()) - 5:int(x[:, 2].max()) + 4] / DX      # (the block drifts 5.1 cells along -x, 1.3 along -z)
    assert 27.25 < under.min() and under.max() < 29.75, (under.min(), under.max())
    sc["colliders"] = [dict(kind="heightfield", heights=heights, origin=(0.0, 0.0), spacing=DX, type=TYPES[boundary], friction=0.3, trans_vel=(0.05, 0.25, -0.05),
                            animate=True, **kw)]
    return sc


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
def test_run_fixed_equals_the_phase_level_loop(sync_interval):
    """mpm_run_fixed(n) - every grid update but the first rides on carry_grid_kernel<true, TerrainArgs> - against grid update, g2p2g, rebuild phase by
    phase (grid_update_collider_kernel<TerrainArgs>) with a moving terrain and a running clock, on the sparse scene and step count of
    test_collision_clock_cpu: positions, the grid the run leaves behind and the clock bit for bit."""
    sc = sparse_terrain("slip")
    sc["config"]["sync_interval"] = sync_interval
    p1, p2, fused = run(sc, STEPS, "phase"), run(sc, STEPS, "phase"), run(sc, STEPS, "fused")
    for a, b in zip(p1[:3], p2[:3]):
        assert np.array_equal(a, b), "the scene is not deterministic: nothing to compare"
    free = run({**sc, "colliders": None}, STEPS, "phase")
    moved = len({tuple(r) for r in p1[0].tolist()} - {tuple(r) for r in free[0].tolist()})
    assert moved >= 12, moved                                                    # (the terrain acted on a quarter of the particles at least)
    assert fused[3] == p1[3] == f32_sum(0.0, [sc["dt"]] * STEPS)
    for what, f, p in zip(("positions", "grid keys", "grid"), fused[:3], p1[:3]):
        assert f.shape == p.shape and np.array_equal(f, p), (what, int((f != p).sum()) if f.shape == p.shape else (f.shape, p.shape))


# ---- 7. the scene -------------------------------------------------------------------------------------------------------------------------------
RAMP_STEPS = 40


def test_block_on_ramp_equals_its_level_set_and_slides_downhill():
    """scenes.block_on_ramp with a 2 x 2 x 2-cell block (64 particles inside one particle block, on which the engine is deterministic) for 40
    substeps: the heightfield run equals, bit for bit in positions, the run with the level set sampled from the model of the same table; no
    particle is lost; the block stays out of the wall-zone blocks (key sets, before and after) where the level set would not act; the centre
    of mass moves downhill (-x: the ramp rises along +x; a free fall has no x displacement at all)."""
    sc = scenes.block_on_ramp(bits=6, block_cells=(2, 2, 2), speed=2.0)
    col = sc["colliders"][0]
    c = hm.heightfield(col["heights"], origin=col["origin"], spacing=col["spacing"], type=col["type"], friction=col["friction"])
    assert np.float32(col["spacing"]) == np.float32(DX)
    sdf, grad = hm.sample_field(c, N, DX)
    level = {k: v for k, v in sc.items() if k != "colliders"}
    level["collision"] = {"sdf": sdf, "grad": grad, "type": col["type"], "friction": col["friction"]}
    x0 = sc["models"][0]["xyz"].astype(np.float64)
    out = {}
    for name, s in (("heightfield", sc), ("heightfield again", sc), ("level set", level), ("free", {**level, "collision": None})):
        eng = build_engine(s)
        eng.initial_setup()
        keys0, _ = eng.dump_grid()
        eng.run_fixed(RAMP_STEPS, s["dt"])
        keys1, _ = eng.dump_grid()
        for keys in (keys0, keys1):
            assert (keys >= BOUNDARY).all() and (keys < G - BOUNDARY).all(), "the block reached a wall-zone block"
        x = eng.retrieve_positions(0)
        assert len(x) == len(x0) and eng.diagnostics().lost_particles == 0 and eng.diagnostics().discarded_p2g == 0
        out[name] = sorted_rows(x), x.astype(np.float64).mean(axis=0)
        eng.close()
    assert np.array_equal(out["heightfield"][0], out["heightfield again"][0]), "the scene is not deterministic: nothing to compare"
    assert np.array_equal(out["heightfield"][0], out["level set"][0])
    assert not np.array_equal(out["heightfield"][0], out["free"][0])
    shift, free = out["heightfield"][1] - x0.mean(axis=0), out["free"][1] - x0.mean(axis=0)
    print("centre of mass / dx: on the ramp", shift / DX, "free", free / DX)
    assert abs(free[0]) < 1e-7 and shift[0] < -1e-3 * DX and shift[1] > free[1], (shift, free)


# ---- 8. a group of two --------------------------------------------------------------------------------------------------------------------------
GROUP_STEPS = 60


def test_group_of_two_equals_one_context_with_a_moving_heightfield():
    """Two ranks (mpm_group_run_fixed, in-process transport, the same heightfield and clock on both) against one context holding the whole
    block, as test_group_of_two_equals_one_context_with_a_moving_shape does: 1e-6 relative, the clocks agree exactly and the ranks did
    exchange halo blocks."""
    sc = sparse_terrain("slip")
    one = build_engine(sc)
    one.initial_setup()
    one.run_fixed(GROUP_STEPS, sc["dt"])
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
            ranks[r].run_fixed(GROUP_STEPS, sc["dt"])
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
    assert all(o[1] == t1 for o in out) and t1 == f32_sum(0.0, [sc["dt"]] * GROUP_STEPS) and min(o[2] for o in out) > 0
    xg = np.concatenate([o[0] for o in out])
    idx, _ = match(x1.astype(np.float64), xg.astype(np.float64))
    rel = (np.abs(xg[idx].astype(np.float64) - x1).max(axis=1) / np.abs(x1).max(axis=1)).max()
    print("group vs single", rel)
    assert rel < 1e-6, rel


# ---- 9. errors and book-keeping -----------------------------------------------------------------------------------------------------------------
def test_errors_and_the_clocks_book_keeping(ctx):
    eng = ctx.eng
    ctx.install([])
    H = hm.make("5x3")["heights"]
    ok = dict(heights=H, origin=(0.1, 0.2), spacing=0.2)
    nan, inf = float("nan"), float("inf")
    bad_h, inf_h, big = H.copy(), H.copy(), H.copy()
    bad_h[2, 1], inf_h[0, 0] = nan, inf
    big[1, 1], big[3, 1] = 3e38, -3e38                                          # finite heights whose central difference overflows
    cases = [(dict(ok, slot=-1), "slot"), (dict(ok, slot=4), "slot"), (dict(ok, heights=np.zeros((1, 3), np.float32)), "nx"), (dict(ok, heights=np.zeros((3, 1), np.float32)), "nz"),
             (dict(ok, heights=np.zeros((4097, 2), np.float32)), "nx"), (dict(ok, heights=np.zeros((2, 4097), np.float32)), "nz"), (dict(ok, spacing=0.0), "spacing"),
             (dict(ok, spacing=-0.5), "spacing"), (dict(ok, spacing=inf), "spacing"), (dict(ok, spacing=nan), "spacing"), (dict(ok, origin=(nan, 0.0)), "origin"),
             (dict(ok, origin=(0.0, nan)), "origin"), (dict(ok, type=-1), "boundary type"), (dict(ok, type=3), "boundary type"), (dict(ok, heights=bad_h), "not finite"),
             (dict(ok, heights=inf_h), "not finite"), (dict(ok, heights=big), "not finite")]
    for kw, word in cases:
        kw = dict(kw)
        slot = kw.pop("slot", 0)
        with pytest.raises(EngineError) as e:
            eng.set_collision_heightfield(slot, **kw)
        assert e.value.code == _ffi.MPM_ERR_INVALID and "heightfield" in str(e.value) and word in str(e.value), (word, str(e.value))
    api, obj, hf = eng.api, _ffi.CollisionObject(), _ffi.Heightfield()
    assert api.default_collision_object(C.byref(obj)) == 0
    hf.nx, hf.nz, hf.spacing = 5, 3, 0.2
    for args, word in (((C.byref(obj), None, ptr(H)), "hf"), ((C.byref(obj), C.byref(hf), None), "heights")):
        assert api.set_collision_heightfield(eng.ctx, 0, *args) == _ffi.MPM_ERR_INVALID and word in api.last_error(eng.ctx).decode()
    # the internal kind number is not accepted from mpm_collision_shape
    with pytest.raises(EngineError) as e:
        eng.set_collision_shape(0, 5, a=(0.5, 0.5, 0.5), radius=0.1)
    assert "kind" in str(e.value)
    # nothing installed (every call above failed): the clock has no owner
    with pytest.raises(EngineError) as e:
        eng.set_collision_clock(True, 0.0)
    assert e.value.code == _ffi.MPM_ERR_INVALID
    # install sets the clock to obj->time, stopped; it succeeds with only a heightfield installed; a second install of either kind resets it
    h = hm.make("65x65", type=1, friction=0.3, trans_vel=(0.0, 0.25, 0.0))
    eng.set_collision_heightfield(1, **{**hm.engine_kwargs(h), "time": 0.25})
    assert eng.collision_time() == 0.25 and not eng.collision_clock_running()
    eng.set_collision_clock(True, 0.5)
    eng.set_collision_shape(2, "sphere", a=(0.25, 0.5, 0.5), radius=0.1, time=0.125)
    assert eng.collision_time() == 0.125 and not eng.collision_clock_running()
    eng.set_collision_shape(2, None)
    # a refused install leaves the old occupant acting (and the clock alone)
    eng.set_collision_clock(True, 0.5)
    for kw in (dict(ok, spacing=0.0), dict(ok, heights=bad_h)):
        with pytest.raises(EngineError):
            eng.set_collision_heightfield(1, **kw)
    with pytest.raises(EngineError):
        eng.set_collision_shape(1, 9)
    assert eng.collision_clock_running() and eng.collision_time() == 0.5
    pat = gm.generate(ctx.nbc, 9, "finite")[0]
    mv, out = ctx.update(pat)
    assert eng.collision_time() == f32_sum(0.5, [DT]) and eng.collision_clock_running()       # one clock, advanced once per grid update
    live, want, mx, hits = ctx.model(pat, [None, h], t=0.5)
    assert hits[0].sum() > 100
    assert_grid(pat, out, live, want)
    assert gm.bits(mv) == gm.bits(mx)
    eng.set_collision_heightfield(1, None)
    with pytest.raises(EngineError):
        eng.collision_time()


# ---- 10. the gmpm driver ------------------------------------------------------------------------------------------------------------------------
def test_gmpm_heightfield_scene_equals_the_engine(tmp_path):
    """A "colliders" scene with one heightfield under tests/test_gmpm_stress_gpu.py's first body (two single-block bodies, on which the engine
    is deterministic), given inline ("heights") and as a raw float32 file ("file", relative to the scene), through the gmpm driver for two
    frames: both write the positions of build_engine on the same collider dict, bit for bit."""
    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS, DT_DEFAULT, FC, FPS, FRAMES, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    nx, nz, sp, origin = 5, 6, 4 / 64, (4 / 64, 10 / 64)
    ii, kk = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    H = ((18.3 + 0.25 * ii - 0.1 * kk) / 64).astype(np.float32)
    col = {"shape": "heightfield", "nx": nx, "nz": nz, "origin": list(origin), "spacing": sp, "type": "slip", "friction": 0.2}
    runs = {}
    for how in ("inline", "file"):
        d = tmp_path / how
        d.mkdir()
        c = dict(col, heights=[float(v) for v in H.ravel()]) if how == "inline" else dict(col, file="ground.f32")
        if how == "file":
            H.astype("<f4").tofile(str(d / "ground.f32"))
        sim = {"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d)}
        (d / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "colliders": [c]}))
        log = subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(d / "scene.json")], text=True, timeout=300)
        assert "has 1 colliders" in log
        runs[how] = d
    start = [read_bgeo_attrs(frame(runs["inline"], m, 0))[0] for m in range(len(MODELS))]

    def drive(colliders):
        models = []
        for mod, xyz in zip(MODELS, start):
            mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
            models.append({"material": mat, "xyz": xyz, "v0": mod["velocity"], "params": ({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {})})
        eng = build_engine({"bits": BITS, "config": {"max_ppc": 128}, "models": models, "colliders": colliders})
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

    want = drive([{"kind": "heightfield", "heights": H, "origin": origin, "spacing": sp, "type": 1, "friction": 0.2, "trans": (origin[0], 0.0, origin[1])}])
    free = drive([])
    for how, d in runs.items():
        for f in range(1, FRAMES + 1):
            for m in range(len(MODELS)):
                got = sorted_rows(read_bgeo_attrs(frame(d, m, f))[0])
                assert np.array_equal(got, want[f - 1][m]), (how, f, m)
    assert not np.array_equal(want[-1][0], free[-1][0]), "the heightfield touched nothing"

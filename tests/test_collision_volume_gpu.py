"""The volume collider on the GPU (claymore_amd/csrc/mpm_collision_volume.hpp; grid_update_collider_kernel<VolumeColliderArgs>,
carry_grid_kernel<true, VolumeColliderArgs>, collision_mesh_table_kernel, mpm_test_collision_volume) against tests/collision_volume_model.py,
which tests/test_collision_volume_cpu.py judges on the CPU.  The grids are injected through the checkpoint port of
tests/test_collision_shapes_gpu.py (its ShapeCtx): grid_update_model's 28-particle scene at bits 6 with 222 neighbour blocks in all 27 wall
classes, the generator's finite tier.  Every comparison with the model is on uint32 bit patterns; computed NaNs compare as NaNs
(grid_update_model.canon).  No test leaves a table's footprint unguarded: the out-of-footprint and NaN points are answered by the query's own
range check before any load (proved on the CPU, tests 3 and 4 there)."""
import ctypes as C
import threading

import numpy as np
import pytest

import collision_mesh_model as cm
import collision_shape_model as sm
import collision_volume_model as vm
import grid_update_model as gm
import heightfield_model as hm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from parity_util import match
from test_collision_clock_cpu import STEPS
from test_collision_shapes_gpu import BOUNDARY, DT, DX, G, GRAVITY, N, TYPES, ShapeCtx, assert_grid, f32_sum, grid_rows, ptr, sorted_rows, sparse_analytic

pytestmark = pytest.mark.gpu


class VolumeCtx(ShapeCtx):
    """ShapeCtx whose slots take shape, heightfield and volume colliders alike, with collision_volume_model.grid_update as the model."""

    def install(self, colliders=(), field=None, t=0.0):
        if field is None:
            self.eng.set_collision_object(None)
        else:
            kw = sm.engine_kwargs(field[0]) if field[0]["kind"] not in ("volume", "heightfield") else vm.engine_kwargs(field[0])
            self.eng.set_collision_object(sdf=field[1], grad=field[2], **{k: kw[k] for k in ("type", "friction", "scale", "dsdt", "trans", "trans_vel", "omega", "rot_mat", "time")})
        cols = list(colliders) + [None] * (4 - len(colliders))
        for slot, c in enumerate(cols):
            if c is None:
                self.eng.set_collision_shape(slot, None)
            elif c["kind"] == "volume":
                self.eng.set_collision_volume(slot, **vm.engine_kwargs(c))
            elif c["kind"] == "heightfield":
                self.eng.set_collision_heightfield(slot, **hm.engine_kwargs(c))
            else:
                self.eng.set_collision_shape(slot, **sm.engine_kwargs(c))
        if field is not None or any(c is not None for c in cols):
            self.eng.set_collision_clock(False, float(t))

    def model(self, pattern, colliders, t=0.0, field=None, dt=DT):
        return vm.grid_update(self.keys, G, BOUNDARY, GRAVITY, dt, pattern.view(np.float32), colliders, t, DX, field=field)


@pytest.fixture(scope="module")
def ctx():
    c = VolumeCtx()
    assert c.nbc == 222 and sorted(map(tuple, c.keys.tolist())) == sorted(map(tuple, gm.scene_keys().tolist()))
    yield c
    c.eng.close()


# ---- 1. mpm_test_collision_volume ----------------------------------------------------------------------------------------------------------------
def device_query(c, t, X):
    from test_collision_volume_cpu import ffi_triple
    obj, vol, T = ffi_triple(c)
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(X), 4), np.float32)
    assert _ffi.load_hip().test_collision_volume(C.byref(obj), C.byref(vol), ptr(T), float(t), ptr(X), len(X), ptr(out), 0) == 0
    return out[:, 0], out[:, 1:]


@pytest.mark.parametrize("inside_out", [False, True], ids=["outward", "inside_out"])
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("name", ["ico", "2x2x2"])
def test_device_query_equals_the_model(name, moved, inside_out):
    """sdis and n on the device, bit for bit, on the points of the CPU test: 4096 seeded domain points and the special points (on samples, on
    cell edges, u = 0 and u = dims - 1 and one float outside each, NaN), on the 13 x 9 x 18 table of an icosphere's field 0.037 apart and on
    a 2 x 2 x 2 table, identity pose and the moved pose at T = 0.37, both values of inside_out."""
    c = vm.make(name, moved, inside_out=inside_out)
    t = sm.T_MOVED if moved else 0.0
    X = vm.query_points(c, t, moved)
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    sdm, nm = vm.query(c, xm)
    assert 0.02 < (sdm <= 0).mean() < 0.98 and np.isnan(sdm[~vm.footprint(c, xm)]).all() and np.isnan(sdm[-3:]).all()
    sd, n = device_query(c, t, X)
    assert np.array_equal(gm.canon(sd), gm.canon(sdm)), np.argwhere(gm.canon(sd) != gm.canon(sdm))[:4].tolist()
    assert np.array_equal(gm.canon(n), gm.canon(nm)), np.argwhere(gm.canon(n) != gm.canon(nm))[:4].tolist()


# ---- 2. cell by cell -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_cell_by_cell(ctx, typ, moved):
    """grid_update_collider_kernel<VolumeColliderArgs> with one volume - the field of collision_shape_model's sphere on 45^3 samples 0.041
    apart (no multiple of dx) from -0.4, wider than the domain at both poses - on a generated grid: every velocity and the returned
    (doubled) maximum equal the model bit for bit.  On the model alone: the surface touches between 10 % and 90 % of the live cells and
    cuts interior and wall-zone blocks."""
    c = vm.sphere_volume(moved=moved, type=TYPES[typ], friction=0.3)
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
def node_volume(shape, **kw):
    """A shape's field sampled at the nodes (collision_shape_model.sample_field) as a volume with origin 0, spacing dx, dims N, and as the
    level-set object's (sdf, grad)."""
    sdf, grad = sm.sample_field(sm.make(shape), N, DX)
    T = np.concatenate([sdf[..., None], np.moveaxis(grad, 0, -1)], axis=-1).astype(np.float32)
    return vm.volume(T, origin=(0.0, 0.0, 0.0), spacing=DX, **kw), sdf, grad


@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("typ", sorted(TYPES))
def test_volume_kernel_equals_the_level_set_kernel(ctx, typ, moved):
    """origin = 0, spacing = dx, dims = N (64^3, 4 MiB): the same samples through mpm_set_collision_object (grid_update_collider_kernel<CollisionArgs>)
    and through the volume, at identity pose with a moving surface and at the moved pose (material points between the samples: both kernels
    interpolate).  All four channels are bit-identical at the cells whose material point lies inside query_sdf's box; every cell of the volume's
    run equals the model; outside the box the level set acts on nothing, the volume wherever its footprint is - at least one such cell differs."""
    kw = sm.MOVED if moved else dict(trans_vel=(0.25, -0.5, 0.125), omega=(0.5, 1.0, -0.25))
    t = sm.T_MOVED if moved else 0.0
    c, sdf, grad = node_volume("sphere", type=TYPES[typ], friction=0.3, **kw)
    pat = gm.generate(ctx.nbc, 3, "finite")[0]
    live, want, _, hits = ctx.model(pat, [c], t)
    X = (gm.node_coords(ctx.keys).transpose(0, 2, 1).reshape(-1, 3).astype(np.float32) * np.float32(DX)).astype(np.float32)
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    lo, hi = np.float32(np.float32(np.float32(BOUNDARY) * np.float32(DX)) * np.float32(4)), np.float32(np.float32(np.float32(G - BOUNDARY) * np.float32(4)) * np.float32(DX))
    inbox = ((xm >= lo) & (xm < hi)).all(axis=1).reshape(live.shape)
    assert (hits[0] & inbox).sum() > 100 and (hits[0] & ~inbox).sum() > 100
    ctx.install([], field=(c, sdf, grad), t=t)
    _, via_field = ctx.update(pat)
    ctx.install([c], t=t)
    _, via_vol = ctx.update(pat)
    for ch in range(4):
        a, b = gm.bits(via_field[:, ch]), gm.bits(via_vol[:, ch])
        assert np.array_equal(a[inbox], b[inbox]), (ch, int((a != b)[inbox].sum()))
    assert_grid(pat, via_vol, live, want)
    assert (gm.bits(via_field[:, 1:]) != gm.bits(via_vol[:, 1:])).any(axis=1)[hits[0] & ~inbox].any()


# ---- 4. the mesh build --------------------------------------------------------------------------------------------------------------------------
BOX = ((0.31, 0.42, 0.29), (0.52, 0.57, 0.71))
MESHES = {
    # 12 triangles on 13 x 9 x 18 samples: partial tiles on every axis
    "box": dict(mesh=lambda: scenes.box_mesh(*BOX), origin=(0.2331, 0.3517, 0.1823), spacing=0.0371, dims=(13, 9, 18)),
    # 320 triangles: more than one kMeshChunk flush per tile
    "icosphere": dict(mesh=lambda: scenes.icosphere((0.47, 0.52, 0.55), 0.21, 2), origin=(0.2231, 0.2617, 0.2923), spacing=0.0271, dims=(19, 20, 21)),
    # 80 triangles, no multiple of 64: the walk's last sweep is partly filled (the bound's lanes clamped to nt - 1, the candidate test's excluded)
    "icosphere80": dict(mesh=lambda: scenes.icosphere((0.47, 0.52, 0.55), 0.21, 1), origin=(0.2231, 0.2617, 0.2923), spacing=0.0471, dims=(10, 11, 9)),
    # dims = 0: the box is the host's
    "auto": dict(mesh=lambda: scenes.icosphere((0.47, 0.52, 0.55), 0.11, 2), origin=None, spacing=0.0171, dims=None),
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_mesh_built_table_equals_the_model(ctx, name):
    """mpm_set_collision_volume_mesh followed by mpm_get_collision_volume against collision_mesh_model's field value at the samples
    origin + (float) i * spacing, bit for bit (precondition, on the model: every radial-rule sample is clear of its pseudonormal's zero plane
    and the sign is the winding number's - collision_mesh_model.check_signs); the descriptor read back is the one given, or the host's
    auto-sizing rule; a sub-box read back equals the same samples."""
    m = MESHES[name]
    v, f = m["mesh"]()
    mesh = cm.Mesh(v, f)
    if m["dims"] is None:
        origin, dims, ok = vm.autosize(v, m["spacing"], 2)
        assert ok
    else:
        origin, dims = np.asarray(m["origin"], np.float32), list(m["dims"])
    want, res, p = vm.mesh_table(mesh, origin, m["spacing"], dims)
    cm.check_signs(mesh, res, p)
    assert (want[..., 0] < 0).any() and (want[..., 0] > 0).any() and (~res["plane"]).any() and res["plane"].any()
    ctx.install([])
    ctx.eng.set_collision_volume_mesh(2, v, f, spacing=m["spacing"], origin=m["origin"], dims=m["dims"], pad=0 if m["dims"] is None else 3, inside_out=True, type=1)
    desc, got = ctx.eng.collision_volume(2)
    assert list(desc["dims"]) == list(dims) and np.array_equal(np.asarray(desc["origin"], np.float32).view(np.uint32), origin.view(np.uint32))
    assert desc["spacing"] == np.float32(m["spacing"]) and desc["inside_out"] and desc["pad"] == (2 if m["dims"] is None else 3)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())
    _, sub = ctx.eng.collision_volume(2, lo=(1, 2, 3), shape=(5, 4, 6))
    assert np.array_equal(sub.view(np.uint32), want[1:6, 2:6, 3:9].view(np.uint32))
    ctx.eng.set_collision_volume(2, None)


def test_mesh_built_volume_on_the_nodes_equals_the_mesh_built_level_set_and_survives_a_round_trip(ctx):
    """With origin = 0, spacing = dx and dims = N the table is what mpm_set_collision_mesh followed by mpm_get_collision_field gives, bit for
    bit.  A volume read back and installed again through mpm_set_collision_volume leaves the same grid as the mesh-built one."""
    v, f = scenes.icosphere((0.47, 0.52, 0.55), 0.21, 2)
    ctx.install([])
    ctx.eng.set_collision_mesh(v, f, type=1)
    field = ctx.eng.collision_field()
    ctx.eng.set_collision_object(None)
    kw = dict(type=1, friction=0.3, trans_vel=(0.25, -0.5, 0.125))
    ctx.eng.set_collision_volume_mesh(0, v, f, spacing=DX, origin=(0.0, 0.0, 0.0), dims=(N, N, N), **kw)
    desc, table = ctx.eng.collision_volume(0)
    assert table.shape == field.shape == (N, N, N, 4) and np.array_equal(table.view(np.uint32), field.view(np.uint32))
    pat = gm.generate(ctx.nbc, 6, "finite")[0]
    ctx.eng.set_collision_clock(False, 0.0)
    mv0, out0 = ctx.update(pat)
    ctx.eng.set_collision_volume(0, table, origin=desc["origin"], spacing=desc["spacing"], inside_out=desc["inside_out"], **kw)
    ctx.eng.set_collision_clock(False, 0.0)
    mv1, out1 = ctx.update(pat)
    assert np.array_equal(gm.bits(out0), gm.bits(out1)) and gm.bits(mv0) == gm.bits(mv1)
    live, want, mx, hits = ctx.model(pat, [vm.volume(table, spacing=DX, **kw)])
    assert hits[0].sum() > 100
    assert_grid(pat, out1, live, want)
    ctx.eng.set_collision_volume(0, None)


# ---- 5. slots -----------------------------------------------------------------------------------------------------------------------------------
def test_slots_mix_every_kind_in_order(ctx):
    """Field object, a sphere shape, a heightfield and two volumes with different poses and types; then permuted; then one removed.  Each result
    equals the model for that order, and the order matters."""
    s = sm.make("sphere", type=2, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    h = hm.make("65x65", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    v1 = vm.sphere_volume(shape="box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    v2 = vm.make("ico", type=0, trans=(0.03, -0.02, 0.01), trans_vel=(0.0, -0.25, 0.5), omega=(0.0, 0.5, 0.0))
    f = sm.make("halfspace_tilted", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    sdf, grad = sm.sample_field(f, N, DX)
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

    a, wa, hits = check([s, h, v1, v2], field=(f, sdf, grad))
    assert all(x.sum() > 50 for x in hits) and (hits[3] & hits[4]).sum() > 20 and (hits[1] & hits[3]).sum() > 20
    b, wb, _ = check([v2, v1, h, s], field=(f, sdf, grad))
    assert (wa != wb).any(axis=1).sum() > 50 and not np.array_equal(a, b)
    c, wc, _ = check([s, h, None, v2], field=(f, sdf, grad))
    assert not np.array_equal(a, c)
    d, _, _ = check([v1, v2])
    e, _, _ = check([v2, v1])
    assert not np.array_equal(d, e)
    # any kind over any other, and back
    ctx.install([s, h, v1, v2], field=(f, sdf, grad))
    ctx.eng.set_collision_shape(2, **sm.engine_kwargs(s))
    ctx.eng.set_collision_heightfield(3, **hm.engine_kwargs(h))
    ctx.eng.set_collision_volume(1, **vm.engine_kwargs(v1))
    ctx.eng.set_collision_clock(False, 0.0)
    _, out = ctx.update(pat)
    live, w, _, _ = ctx.model(pat, [s, v1, s, h], field=(f, sdf, grad))
    assert_grid(pat, out, live, w)
    ctx.install([])
    mv, out = ctx.update(pat)
    assert np.array_equal(gm.bits(out), gm.bits(plain)) and gm.bits(mv) == gm.bits(mv_plain)


# ---- 6. the carry-over --------------------------------------------------------------------------------------------------------------------------
def sparse_volume(boundary="slip", **kw):
    """tests/test_collision_heightfield_gpu.py's sparse_terrain with the terrain given as a volume: the heightfield model's field - tangent-plane
    distance and (-gx, 1, -gz) - sampled on the nodes 8 .. 56 x 18 .. 42 x 8 .. 56 (49 x 25 x 49 samples dx apart), under the block's lowest
    particle layer only and rising with the clock at the layers' own 0.25, so that the lowest layer slides on it for the whole run while the
    others never touch it (its docstring carries the argument for the scene's determinism)."""
    from test_collision_heightfield_gpu import sparse_terrain
    sc = sparse_terrain(boundary)
    col = sc["colliders"][0]
    h = hm.heightfield(col["heights"], origin=col["origin"], spacing=col["spacing"])
    lo, dims = (8, 18, 8), (49, 25, 49)
    p = vm.sample_points(tuple(np.float32(v) * np.float32(DX) for v in lo), DX, dims)
    assert np.array_equal(p, (np.stack(np.meshgrid(*[np.arange(lo[d], lo[d] + dims[d]) for d in range(3)], indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(DX)))
    sd, _ = hm.query(h, p)
    T = h["table"][lo[0]:lo[0] + dims[0], lo[2]:lo[2] + dims[2]]
    g = np.stack([np.broadcast_to(-T[:, None, :, 1], dims), np.ones(dims, np.float32), np.broadcast_to(-T[:, None, :, 2], dims)], axis=-1)
    field4 = np.concatenate([sd.reshape(dims)[..., None], g], axis=-1).astype(np.float32)
    sc["colliders"] = [dict(kind="volume", field4=field4, origin=tuple(float(np.float32(v) * np.float32(DX)) for v in lo), spacing=DX, type=TYPES[boundary], friction=0.3,
                            trans_vel=col["trans_vel"], animate=True, **kw)]
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
    """mpm_run_fixed(n) - every grid update but the first rides on carry_grid_kernel<true, VolumeColliderArgs> - against grid update, g2p2g, rebuild
    phase by phase (grid_update_collider_kernel<VolumeColliderArgs>) with a moving volume and a running clock, on the sparse scene and step count
    of test_collision_clock_cpu: positions, the grid the run leaves behind and the clock bit for bit."""
    sc = sparse_volume("slip")
    sc["config"]["sync_interval"] = sync_interval
    p1, p2, fused = run(sc, STEPS, "phase"), run(sc, STEPS, "phase"), run(sc, STEPS, "fused")
    for a, b in zip(p1[:3], p2[:3]):
        assert np.array_equal(a, b), "the scene is not deterministic: nothing to compare"
    free = run({**sc, "colliders": None}, STEPS, "phase")
    moved = len({tuple(r) for r in p1[0].tolist()} - {tuple(r) for r in free[0].tolist()})
    assert moved >= 12, moved                                                    # (the volume acted on a quarter of the particles at least)
    assert fused[3] == p1[3] == f32_sum(0.0, [sc["dt"]] * STEPS)
    for what, f, p in zip(("positions", "grid keys", "grid"), fused[:3], p1[:3]):
        assert f.shape == p.shape and np.array_equal(f, p), (what, int((f != p).sum()) if f.shape == p.shape else (f.shape, p.shape))


# ---- 7. a group of two --------------------------------------------------------------------------------------------------------------------------
GROUP_STEPS = 60


def test_group_of_two_equals_one_context_with_a_moving_volume():
    """Two ranks (mpm_group_run_fixed, in-process transport, the same volume and clock on both) against one context holding the whole block, as
    test_group_of_two_equals_one_context_with_a_moving_heightfield does: 1e-6 relative, the clocks agree exactly and the ranks did exchange
    halo blocks."""
    sc = sparse_volume("slip")
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


# ---- 8. errors and book-keeping -----------------------------------------------------------------------------------------------------------------
def test_errors_and_the_clocks_book_keeping(ctx):
    import torch
    eng = ctx.eng
    ctx.install([])
    nan, inf = float("nan"), float("inf")
    T = vm.make("ico")["table"]
    ok = dict(field4=T, origin=(0.26, 0.37, 0.21), spacing=0.037)
    bad_t, inf_t = T.copy(), T.copy()
    bad_t[3, 2, 1, 0], inf_t[0, 0, 0, 3] = nan, inf
    # nothing installed: the clock has no owner
    with pytest.raises(EngineError) as e:
        eng.set_collision_clock(True, 0.0)
    assert e.value.code == _ffi.MPM_ERR_INVALID
    # an occupant whose action and clock every refusal below must leave alone
    occ = vm.sphere_volume(type=1, friction=0.3, trans_vel=(0.0, 0.25, 0.0))
    eng.set_collision_volume(1, **{**vm.engine_kwargs(occ), "time": 0.25})
    assert eng.collision_time() == 0.25 and not eng.collision_clock_running()
    eng.set_collision_clock(True, 0.5)
    cases = [(dict(ok, slot=-1), "slot"), (dict(ok, slot=4), "slot"), (dict(ok, field4=np.zeros((1, 3, 3, 4), np.float32)), "dims"), (dict(ok, field4=np.zeros((2, 2, 1025, 4), np.float32)), "dims"),
             (dict(ok, spacing=0.0), "spacing"), (dict(ok, spacing=-0.5), "spacing"), (dict(ok, spacing=inf), "spacing"), (dict(ok, spacing=nan), "spacing"),
             (dict(ok, origin=(nan, 0.0, 0.0)), "origin"), (dict(ok, origin=(0.0, 0.0, nan)), "origin"), (dict(ok, type=-1), "boundary type"), (dict(ok, type=3), "boundary type"),
             (dict(ok, field4=bad_t), "not finite"), (dict(ok, field4=inf_t), "not finite")]
    for kw, word in cases:
        kw = dict(kw)
        slot = kw.pop("slot", 1)
        with pytest.raises(EngineError) as e:
            eng.set_collision_volume(slot, **kw)
        assert e.value.code == _ffi.MPM_ERR_INVALID and "status 1: collision volume:" in str(e.value) and word in str(e.value), (word, str(e.value))
    v, f = scenes.box_mesh((0.3, 0.3, 0.3), (0.6, 0.5, 0.7))
    mesh_ok = dict(vertices=v, faces=f, spacing=0.03)
    mesh_cases = [(dict(mesh_ok, pad=-1), "pad"), (dict(mesh_ok, spacing=1e-5), "dims"), (dict(mesh_ok, faces=f[:-1]), "closed"), (dict(mesh_ok, faces=f[:, ::-1]), "signed volume"),
                  (dict(mesh_ok, faces=f[:3]), "fewer than 4"), (dict(mesh_ok, origin=(0.0, 0.0, 0.0), dims=(1, 4, 4)), "dims"), (dict(mesh_ok, type=5), "boundary type")]
    for kw, word in mesh_cases:
        with pytest.raises(EngineError) as e:
            eng.set_collision_volume_mesh(1, **kw)
        assert e.value.code == _ffi.MPM_ERR_INVALID and "status 1: collision volume:" in str(e.value) and word in str(e.value), (word, str(e.value))
    api, obj, vol = eng.api, _ffi.CollisionObject(), _ffi.CollisionVolume()
    assert api.default_collision_object(C.byref(obj)) == 0
    vol.dims[0], vol.dims[1], vol.dims[2], vol.spacing = 13, 9, 18, 0.037
    for args, word in (((C.byref(obj), None, ptr(T)), "vol"), ((C.byref(obj), C.byref(vol), None), "field4")):
        assert api.set_collision_volume(eng.ctx, 1, *args) == _ffi.MPM_ERR_INVALID and word in api.last_error(eng.ctx).decode()
    vol.dims[0] = vol.dims[1] = vol.dims[2] = 0
    assert api.set_collision_volume(eng.ctx, 1, C.byref(obj), C.byref(vol), ptr(T)) == _ffi.MPM_ERR_INVALID and "zero" in api.last_error(eng.ctx).decode()
    # reading back: a slot without a volume, a box that leaves the table
    for slot, kw, word in ((0, {}, "no volume"), (5, {}, "slot"), (1, dict(lo=(0, 0, 40), shape=(2, 2, 6)), "leaves the table"), (1, dict(lo=(0, -1, 0), shape=(2, 2, 2)), "leaves the table")):
        with pytest.raises(EngineError) as e:
            eng.collision_volume(slot, **kw)
        assert e.value.code == _ffi.MPM_ERR_INVALID and word in str(e.value), str(e.value)
    # the internal kind number is not accepted from mpm_collision_shape
    with pytest.raises(EngineError) as e:
        eng.set_collision_shape(1, 6, a=(0.5, 0.5, 0.5), radius=0.1)
    assert "kind" in str(e.value)
    # every refusal left the occupant acting and the clock alone: one grid update at T = 0.5, then T + dt
    assert eng.collision_clock_running() and eng.collision_time() == 0.5
    pat = gm.generate(ctx.nbc, 9, "finite")[0]
    mv, out = ctx.update(pat)
    assert eng.collision_time() == f32_sum(0.5, [DT]) and eng.collision_clock_running()
    live, want, mx, hits = ctx.model(pat, [None, occ], t=0.5)
    assert hits[0].sum() > 100
    assert_grid(pat, out, live, want)
    assert gm.bits(mv) == gm.bits(mx)
    # a second install of any kind resets the clock, stopped
    eng.set_collision_shape(2, "sphere", a=(0.25, 0.5, 0.5), radius=0.1, time=0.125)
    assert eng.collision_time() == 0.125 and not eng.collision_clock_running()
    eng.set_collision_shape(2, None)
    # a replace frees the old table: 128^3 samples (32 MiB) installed, then replaced three times - at most one table's worth of free memory may go
    big = np.zeros((128, 128, 128, 4), np.float32)
    big[..., 0], big[..., 2] = 1.0, 1.0
    eng.set_collision_volume(1, big, origin=(0.0, 0.0, 0.0), spacing=1.0 / 127)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        eng.set_collision_volume(1, big, origin=(0.0, 0.0, 0.0), spacing=1.0 / 127)
    free1 = torch.cuda.mem_get_info()[0]
    print("free device memory before / after three replaces", free0, free1)
    assert free0 - free1 <= big.nbytes, (free0, free1)
    # removing the last collider leaves the clock without an owner
    eng.set_collision_volume(1, None)
    with pytest.raises(EngineError):
        eng.collision_time()


# ---- 9. the scene -------------------------------------------------------------------------------------------------------------------------------
def test_two_paddles_squeeze_the_ball():
    """scenes.two_paddles - two mesh-built volumes in slots 0 and 1 that move toward each other - for 20 substeps: both tables are there with
    their own boxes, the clock ran, no particle is lost, and the material's x momentum changes sign between the paddles: the half of the
    ball next to the left paddle is pushed toward +x, the other half toward -x."""
    sc = scenes.two_paddles(bits=6, gap_cells=0.5, speed=2.0)
    eng = build_engine(sc)
    d0, t0 = eng.collision_volume(0)
    d1, t1 = eng.collision_volume(1)
    assert d0["dims"] == d1["dims"] and d0["origin"][0] < 0.5 < d1["origin"][0] and (t0[..., 0] < 0).any() and (t1[..., 0] < 0).any()
    eng.initial_setup()
    eng.run_fixed(20, sc["dt"])
    assert eng.collision_time() == f32_sum(0.0, [sc["dt"]] * 20) and eng.diagnostics().lost_particles == 0
    x, v = eng.retrieve_velocity(0)
    eng.close()
    left, right = x[:, 0] < 0.5 - 2 * DX, x[:, 0] > 0.5 + 2 * DX
    px_left, px_right = float(v[left, 0].astype(np.float64).sum()), float(v[right, 0].astype(np.float64).sum())
    print("x momentum / mass: left half", px_left, "right half", px_right)
    assert px_left > 0 > px_right and (np.abs(v[:, 0]) > 0.1).sum() > 50


# ---- 10. the gmpm driver ------------------------------------------------------------------------------------------------------------------------
def test_gmpm_mesh_and_volume_scene_equals_the_engine(tmp_path):
    """A "colliders" scene with a "mesh" collider (an OBJ box under tests/test_gmpm_stress_gpu.py's first body) and a "volume" collider (a raw
    float32 table of a plane's field under its second body) - two single-block bodies, on which the engine is deterministic - through the gmpm
    driver for two frames: it writes the positions of build_engine on the same data, bit for bit, and both colliders acted."""
    import json
    import os
    import subprocess

    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS, DT_DEFAULT, FC, FPS, FRAMES, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    v, f = scenes.box_mesh((4 / 64, 14 / 64, 16 / 64), (12 / 64, 18.3 / 64, 23 / 64))
    cm.write_obj(str(tmp_path / "body.obj"), v, f)
    origin, sp, dims = (4 / 64, 26 / 64, 26 / 64), 2 / 64, (6, 6, 6)
    p = vm.sample_points(origin, sp, dims)
    T = np.concatenate([(p[:, 1:2] - np.float32(30.3 / 64)).astype(np.float32), np.broadcast_to(np.array([0, 1, 0], np.float32), (len(p), 3))], axis=1).reshape(dims + (4,))
    T.astype("<f4").tofile(str(tmp_path / "plane.f32"))
    cols = [{"shape": "mesh", "file": "body.obj", "spacing": 0.75 / 64, "pad": 3, "type": "slip", "friction": 0.2},
            {"shape": "volume", "file": "plane.f32", "dims": list(dims), "origin": list(origin), "spacing": sp, "type": "sticky"}]
    sim = {"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(tmp_path)}
    (tmp_path / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "colliders": cols}))
    log = subprocess.check_output([os.path.join(root, "claymore_amd", "host", "gmpm"), "-f", str(tmp_path / "scene.json")], text=True, timeout=300)
    assert "has 2 colliders" in log
    start = [read_bgeo_attrs(frame(tmp_path, m, 0))[0] for m in range(len(MODELS))]

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

    want = drive([{"kind": "volume_mesh", "vertices": v, "faces": f, "spacing": 0.75 / 64, "pad": 3, "type": 1, "friction": 0.2},
                  {"kind": "volume", "field4": T, "origin": origin, "spacing": sp, "type": 0}])
    free = drive([])
    for fr in range(1, FRAMES + 1):
        for m in range(len(MODELS)):
            got = sorted_rows(read_bgeo_attrs(frame(tmp_path, m, fr))[0])
            assert np.array_equal(got, want[fr - 1][m]), (fr, m)
    for m in range(len(MODELS)):
        assert not np.array_equal(want[-1][m], free[-1][m]), f"collider {m} touched nothing"

"""Particle removal on the GPU (mpm_count_particles_in, mpm_remove_particles, Engine.count_in / Engine.remove;
claymore_amd/csrc/mpm_particle_remove.hpp) against the NumPy statement of its contract (tests/particle_remove_model.py): after every removal the
selected particles - the model's float32 predicate on the positions read back, bit-exact - are gone and listed, the survivors hold the bits they
had; a grid node no removed stencil reaches has the bits it had, a reached node holds the survivors' set-up mass and its old velocity within a
bound counted from the roundings, exact zeros where nobody is left; the table checks, the counts follow, n and the cumulative counters stay, the
totals fall by what the call reports.  A refused call and a call that selects nothing leave the checkpoint byte for byte as it was.  No bound
here was fitted to what the kernels return."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ckpt_format as cf  # noqa: E402,F401
import face_scenes as fs  # noqa: E402
import g2p2g_bench as gb  # noqa: E402
import g2p2g_model as gm  # noqa: E402
import particle_emit_model as pem  # noqa: E402
import particle_init_model as pim  # noqa: E402
import particle_remove_model as prm  # noqa: E402
from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import EngineError, build_engine  # noqa: E402
from test_particle_emit_gpu import assert_unchanged, model_dict, read_particles, scene_of, set_up, snapshot, state9_of  # noqa: E402

pytestmark = pytest.mark.gpu

BITS, MAX_PPC = gm.BITS, gm.MAX_PPC
DX = np.float32(0.5 ** BITS)
U = pim.U
V0 = (0.3, -0.2, 0.1)


def block_box(key, shrink=0.0):
    """the box that holds the particles gm.block_particles puts into block `key`: cells [4k + 1.5, 4k + 5.5], as a region in world units"""
    c = (4.0 * np.asarray(key, np.float64) + 3.5) * float(DX)
    return {"kind": "box", "center": tuple(c), "half_extents": (float(DX) * (2.0 - shrink),) * 3}


def rows_of(xyz, ids, model):
    """removed rows as a sorted structured array: position bits, id, model"""
    x = np.ascontiguousarray(xyz, np.float32).view(np.uint32).reshape(-1, 3)
    r = np.empty(x.shape[0], dtype=[("x", np.uint32), ("y", np.uint32), ("z", np.uint32), ("id", np.int32), ("m", np.int32)])
    r["x"], r["y"], r["z"], r["id"], r["m"] = x[:, 0], x[:, 1], x[:, 2], ids, model
    return np.sort(r, order=["x", "y", "z", "id", "m"])


def remove_checked(eng, regions=None, ids=None, model=-1, tag=""):
    """Engine.remove, then everything the contract says, against particle_remove_model.  Returns the call's result."""
    nm = len(eng.models)
    regions = [] if regions is None else ([regions] if isinstance(regions, dict) else list(regions))
    before = [read_particles(eng, m) for m in range(nm)]
    flat0, val0 = pem.grid_by_node(*eng.dump_grid(), BITS)
    cnt0, d0, tot0, cap0 = eng.counts(), eng.diagnostics(), eng.grid_totals(), eng.capacity()
    n0, rem0 = [m["n"] for m in eng.models], [m["removed"] for m in eng.models]
    gone = [prm.selected(before[m]["xyz"], regions, before[m]["ids"], ids if (ids is not None and m == model) else ()) if model in (-1, m) else np.zeros(before[m]["xyz"].shape[0], bool)
            for m in range(nm)]
    want_removed = [int(g.sum()) for g in gone]
    if regions and ids is None:
        assert eng.count_in(regions, model) == want_removed, (tag, "count_in")
    res = eng.remove(regions=regions, ids=ids, model=model, return_removed=True)
    assert res["removed"] == want_removed, (tag, res["removed"], want_removed)
    assert res["relaid"] == (sum(want_removed) > 0)
    assert eng.api.check_table(eng.ctx) == 0
    # the particles: survivors and removed rows, bit for bit, as sets
    split = [prm.split(before[m], gone[m]) for m in range(nm)]
    for m in range(nm):
        assert pem.same_set(read_particles(eng, m), split[m][0]), (tag, "survivors of model", m)
    want_rows = np.concatenate([rows_of(split[m][1]["xyz"], split[m][1]["ids"] if eng.track_ids else -1, m) for m in range(nm)])
    assert np.array_equal(rows_of(res["xyz"], res["ids"], res["model"]), np.sort(want_rows, order=["x", "y", "z", "id", "m"])), (tag, "the removed rows")
    # the grid, node by node
    flat1, val1 = pem.grid_by_node(*eng.dump_grid(), BITS)
    removed_xyz = np.concatenate([split[m][1]["xyz"] for m in range(nm)])
    params = [{"volume": eng.models[m]["params"].volume, "rho": eng.models[m]["params"].rho} for m in range(nm)]
    worst = prm.check_grid(flat0, val0, flat1, val1, removed_xyz, prm.survivor_scene(BITS, [(params[m], split[m][0]["xyz"]) for m in range(nm)]))
    print(f"{tag}: {sum(want_removed)} particles removed {want_removed}, {flat1.size} nodes of {flat0.size} left; worst error / bound per channel {worst}")
    # counts, n, counters, totals, capacities
    cnt1, d1, tot1 = eng.counts(), eng.diagnostics(), eng.grid_totals()
    for m in range(nm):
        assert int(cnt1.particles[m]) == int(cnt0.particles[m]) - want_removed[m]
        assert eng.models[m]["n"] == n0[m] and eng.models[m]["removed"] == rem0[m] + want_removed[m]
    assert (int(d1.lost_particles), int(d1.discarded_p2g), int(d1.dropped_particles)) == (int(d0.lost_particles), int(d0.discarded_p2g), int(d0.dropped_particles))
    # the float64 totals are sums of K float32 values in an unspecified order: (K - 1) 2^-53 of the sum of magnitudes each, four of them in play
    slack = 4 * max(flat0.size, 1) * 2.0 ** -53 * np.abs(val0).astype(np.float64).sum(axis=0)
    out = np.concatenate([[res["mass"]], res["momentum"]])
    assert (np.abs((tot0 - tot1) - out) <= slack).all(), (tag, tot0 - tot1, out)
    assert eng.particle_momentum()["count"] == sum(int(cnt1.particles[m]) for m in range(nm))
    assert eng.capacity() == cap0, "capacities neither shrink nor grow"
    return res


def moving_cluster(material=gm.FC, track_ids=False, steps=3, **extra):
    """the cluster with a velocity, a few substeps on: the grid holds momenta that differ from node to node, the lists carry neighbour tags"""
    eng = set_up(scene_of([model_dict(material, gm.scene_cluster(), v0=V0)], track_ids=track_ids, **extra))
    if steps:
        eng.run_fixed(steps, 1e-4)
    return eng


# ---- regions and counts ------------------------------------------------------------------------------------------------------------------------------
C0 = (4.0 * np.asarray(gm.CLUSTER[0], np.float64) + 5.5) * float(DX)          # the corner the eight blocks of the cluster share
REGIONS = {
    "halfspace": {"kind": "halfspace", "point": tuple(C0), "normal": (1.0, 2.0, -0.5)},
    "sphere": {"kind": "sphere", "center": tuple(C0), "radius": 2.3 * float(DX)},
    "box": {"kind": "box", "center": tuple(C0 + 0.4 * float(DX)), "half_extents": (1.7 * float(DX), 3.1 * float(DX), 0.9 * float(DX))},
    "capsule": {"kind": "capsule", "a": tuple(C0 - 2.5 * float(DX)), "b": tuple(C0 + 2.5 * float(DX)), "radius": 1.2 * float(DX)},
    "inside_out sphere": {"kind": "sphere", "center": tuple(C0), "radius": 3.0 * float(DX), "inside_out": True},
}


@pytest.mark.parametrize("kind", sorted(REGIONS))
def test_each_shape_kind_and_inside_out(kind):
    eng = moving_cluster()
    res = remove_checked(eng, REGIONS[kind], tag=kind)
    assert 0 < res["removed"][0] < eng.models[0]["n"]
    eng.run_fixed(3, 1e-5)
    assert int(eng.counts().particles[0]) == eng.models[0]["n"] - res["removed"][0] and eng.api.check_table(eng.ctx) == 0
    eng.close()


def test_two_regions_that_overlap_count_a_particle_once():
    eng = moving_cluster()
    x = eng.retrieve_positions(0)
    a, b = prm.selected(x, [REGIONS["sphere"]]), prm.selected(x, [REGIONS["box"]])
    assert (a & b).sum() > 0 and (a & ~b).sum() > 0 and (b & ~a).sum() > 0
    res = remove_checked(eng, [REGIONS["sphere"], REGIONS["box"]], tag="two regions")
    assert res["removed"][0] == int((a | b).sum())
    eng.close()


# ---- where the removed particles sit --------------------------------------------------------------------------------------------------------------------
def test_one_particle_a_whole_block_and_all_eight_blocks():
    eng = moving_cluster()
    x = eng.retrieve_positions(0)
    one = x[np.argmin(np.abs(x.astype(np.float64) - C0).sum(axis=1))].astype(np.float64)
    res = remove_checked(eng, {"kind": "sphere", "center": tuple(one), "radius": 1e-4 * float(DX)}, tag="one particle")
    assert res["removed"] == [1]
    eng.close()
    eng = moving_cluster(steps=0)                                       # (at rest in their blocks: the box is the block)
    blocks0 = eng.counts().particle_blocks
    res = remove_checked(eng, block_box(gm.CLUSTER[3]), tag="a whole block")
    assert res["removed"][0] >= 185 and eng.counts().particle_blocks == blocks0 - 1
    res = remove_checked(eng, {"kind": "sphere", "center": (0.5, 0.5, 0.5), "radius": 1.0}, tag="all eight blocks")
    c = eng.counts()
    assert (int(c.particles[0]), c.particle_blocks, c.neighbor_blocks) == (0, 0, 0) and eng.models[0]["removed"] == eng.models[0]["n"]
    assert np.array_equal(eng.grid_totals(), np.zeros(4))
    eng.run_fixed(2, 1e-5)
    assert int(eng.counts().particles[0]) == 0
    eng.close()


def test_particles_in_the_outermost_cells_of_the_six_faces():
    """face_scenes' slabs - cells -2 / -1 of the lower faces, the top cells, corners and edges - set up beside the cluster and removed: node -1 has
    no cell to mark and the blocks beyond the upper faces do not exist"""
    slab = fs.setup_slab_cells(BITS)
    eng = set_up(scene_of([model_dict(gm.FC, np.concatenate([gm.scene_cluster(), slab]), v0=V0)]))
    res = remove_checked(eng, {"kind": "box", "center": (0.5, 0.5, 0.5), "half_extents": (0.5 - 4 * float(DX),) * 3, "inside_out": True}, tag="six faces")
    assert res["removed"] == [slab.shape[0]]
    eng.close()


def test_half_of_a_full_block_and_one_cell_down_to_one():
    """1024 = max_ppc * 64 records in one block, half of them removed: the walk crosses the 512-record chunk and the merged tail; 513 particles in
    one cell, all but one removed"""
    rng = np.random.default_rng(21)
    key = gm.SITES[13]
    full = gm.block_particles(key, MAX_PPC * 64, rng)
    eng = set_up(scene_of([model_dict(gm.SAND, np.concatenate([full, gm.scene_one_cell()]), v0=V0)]))
    half = {"kind": "halfspace", "point": tuple((4.0 * np.asarray(key, np.float64) + 3.5) * float(DX)), "normal": (0.0, 0.0, 1.0)}
    assert 300 < int(prm.selected(full * DX, [half]).sum()) < 724
    remove_checked(eng, half, model=0, tag="half of a 1024-particle block")
    eng.close()
    cell = gm.scene_one_cell()[:513]
    eng = set_up(scene_of([model_dict(gm.J_FLUID, cell, v0=V0)]))
    keep = (cell[7] * DX).astype(np.float64)
    res = remove_checked(eng, {"kind": "sphere", "center": tuple(keep), "radius": 1e-4 * float(DX), "inside_out": True}, tag="513 in one cell down to 1")
    assert res["removed"] == [512] and int(eng.counts().particles[0]) == 1
    eng.close()


# ---- materials, models and ids ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS, ids=[gm.NAMES[m] for m in gm.MATERIALS])
def test_every_material_keeps_its_state(material):
    pos, st = gm.scene_state("cluster", material)
    eng = set_up(scene_of([model_dict(material, pos, state=state9_of(material, st), logjp=st["logjp"], v0=V0)]))
    remove_checked(eng, REGIONS["halfspace"], tag=gm.NAMES[material])
    remove_checked(eng, REGIONS["sphere"], tag=gm.NAMES[material] + ", a second removal")
    eng.close()


def two_models():
    pa, pb = gm.scene_cluster(), gm.EXTRA_SCENES["cluster_b"]()
    sa, sb = gm.make_state(gm.SAND, pa.shape[0], 81), gm.make_state(gm.J_FLUID, pb.shape[0], 82)
    return set_up(scene_of([model_dict(gm.SAND, pa, state=state9_of(gm.SAND, sa), logjp=sa["logjp"], v0=V0), model_dict(gm.J_FLUID, pb, state=state9_of(gm.J_FLUID, sb), v0=(0.0, -1.0, 0.0))]))


def test_two_models_sharing_blocks_all_of_them_and_one():
    eng = two_models()
    eng.run_fixed(2, 1e-4)
    res = remove_checked(eng, REGIONS["box"], model=-1, tag="two models, model = -1")
    assert res["removed"][0] > 0 and res["removed"][1] > 0 and set(res["model"].tolist()) == {0, 1}
    res = remove_checked(eng, REGIONS["halfspace"], model=1, tag="two models, model = 1")
    assert res["removed"][0] == 0 and res["removed"][1] > 0
    eng.close()


def test_a_model_emptied_and_emitted_into_again_continues_its_ids():
    from test_particle_emit_gpu import emit_checked
    pa, pb = gm.scene_cluster(), gm.EXTRA_SCENES["cluster_b"]()
    eng = set_up(scene_of([model_dict(gm.FC, pa, v0=V0), model_dict(gm.J_FLUID, pb)], track_ids=True))
    res = remove_checked(eng, {"kind": "sphere", "center": (0.5, 0.5, 0.5), "radius": 1.0}, model=1, tag="a model emptied")
    assert res["removed"] == [0, pb.shape[0]] and int(eng.counts().particles[1]) == 0 and eng.models[1]["n"] == pb.shape[0]
    new = gm.block_particles(gm.CLUSTER[2], 50, np.random.default_rng(22))
    assert emit_checked(eng, 1, new, v0=(0.0, -1.0, 0.0), tag="emitted into again") == pb.shape[0]
    ids = np.sort(eng.retrieve_ids(1)[1])
    assert np.array_equal(ids, np.arange(pb.shape[0], pb.shape[0] + 50)), "the ids continue from n: a removed id does not return"
    eng.run_fixed(3, 1e-4)
    assert np.array_equal(np.sort(eng.retrieve_ids(1)[1]), ids) and int(eng.counts().particles[0]) == pa.shape[0]
    eng.close()


def test_tracked_ids_alone_with_a_region_stale_and_duplicate():
    eng = moving_cluster(track_ids=True)
    n = eng.models[0]["n"]
    pick = np.arange(5, n, 7, dtype=np.int32)
    res = remove_checked(eng, ids=pick, model=0, tag="ids alone")
    assert res["removed"] == [pick.size] and np.array_equal(np.sort(res["ids"]), pick)
    again = np.concatenate([pick[:10], pick[:10], np.int32([6, 6, 13])])            # stale (gone already), duplicates, and two that live
    res = remove_checked(eng, ids=again, model=0, tag="stale and duplicate ids")
    assert res["removed"] == [2] and np.array_equal(np.sort(res["ids"]), [6, 13])
    res = remove_checked(eng, REGIONS["sphere"], ids=np.arange(0, n, 11, dtype=np.int32), model=0, tag="ids and a region")
    assert res["removed"][0] > 0
    before = snapshot(eng)
    res = eng.remove(ids=pick, model=0)
    assert res["removed"] == [0] and not res["relaid"]
    assert_unchanged(eng, before, "only stale ids: nothing selected")
    eng.close()


# ---- nothing selected ------------------------------------------------------------------------------------------------------------------------------------
FAR = {"kind": "sphere", "center": (0.2, 0.2, 0.2), "radius": 2.0 * float(DX)}


def test_nothing_selected_changes_nothing_and_keeps_the_still_path_on_offer():
    """nothing moves (no gravity, stress-free, at rest): of a 64-substep window's rebuilds all but the first take the still path after set-up; a
    removal that selects nothing leaves the checkpoint byte for byte and the next window takes the still path from its first rebuild on - the check of
    test_still_path_is_not_offered_to_the_first_rebuild_after_an_emission, reversed; after a real removal the first rebuild is not offered it"""
    eng = set_up(scene_of([model_dict(gm.FC, gm.scene_cluster())], config={"gravity": 0.0, "sync_interval": 64}))
    s0 = int(eng.diagnostics().still_rebuilds)
    eng.run_fixed(64, 1e-5)
    s1 = int(eng.diagnostics().still_rebuilds)
    before = snapshot(eng)
    assert eng.count_in(FAR) == [0]
    res = eng.remove(regions=FAR, return_removed=True)
    assert res["removed"] == [0] and not res["relaid"] and res["mass"] == 0.0 and res["xyz"].shape == (0, 3)
    assert_unchanged(eng, before, "nothing selected")
    eng.run_fixed(64, 1e-5)
    s2 = int(eng.diagnostics().still_rebuilds)
    assert remove_checked(eng, block_box(gm.CLUSTER[5]), tag="a real removal")["relaid"]
    eng.run_fixed(64, 1e-5)
    s3 = int(eng.diagnostics().still_rebuilds)
    eng.close()
    assert (s1 - s0, s2 - s1, s3 - s2) == (63, 64, 63)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def refused(eng, code, word, **kw):
    before = snapshot(eng)
    with pytest.raises(EngineError) as e:
        eng.remove(**kw)
    assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
    assert_unchanged(eng, before, word)


def test_every_refusal_changes_nothing():
    eng = build_engine(scene_of([model_dict(gm.SAND, gm.scene_cluster(), v0=V0)], track_ids=True))
    with pytest.raises(EngineError) as e:
        eng.remove(regions=REGIONS["sphere"])
    assert e.value.code == _ffi.MPM_ERR_NOT_READY
    with pytest.raises(EngineError) as e:
        eng.count_in(REGIONS["sphere"])
    assert e.value.code == _ffi.MPM_ERR_NOT_READY
    eng.initial_setup()
    eng.run_fixed(2, 1e-5)
    INV, n = _ffi.MPM_ERR_INVALID, eng.models[0]["n"]
    sph = REGIONS["sphere"]
    refused(eng, INV, "no model", regions=sph, model=1)
    refused(eng, INV, "no model", regions=sph, model=-2)
    for bad, word in (({"kind": 7}, "unknown kind"), ({"kind": "sphere", "center": (0.5, 0.5, 0.5), "radius": 0.0}, "radius"), ({"kind": "sphere", "center": (np.nan, 0.5, 0.5), "radius": 0.1}, "NaN"),
                      ({"kind": "halfspace", "point": (0.5, 0.5, 0.5), "normal": (0.0, 0.0, 0.0)}, "normal"), ({"kind": "box", "center": (0.5, 0.5, 0.5), "half_extents": (0.1, -0.1, 0.1)}, "half extents"),
                      ({"kind": "capsule", "a": (0.5, 0.5, 0.5), "b": (0.5, 0.5, 0.5), "radius": 0.1}, "coincide")):
        refused(eng, INV, word, regions=[sph, bad])
        before = snapshot(eng)
        with pytest.raises(EngineError) as e:
            eng.count_in([bad])
        assert e.value.code == INV and word in str(e.value)
        assert_unchanged(eng, before, word)
    refused(eng, INV, "nregions", regions=[sph] * 9)
    refused(eng, INV, "model >= 0", ids=[1, 2], model=-1)
    refused(eng, INV, "outside 0..", ids=[1, n], model=0)
    refused(eng, INV, "outside 0..", ids=[-1], model=0)
    before = snapshot(eng)
    what, res = _ffi.Removal(), _ffi.RemovalResult()
    arr, k = eng._sink_regions("test", [sph])
    what.regions, what.nregions = arr, k
    what.reserved[2] = 1
    assert eng.api.remove_particles(eng.ctx, 0, C.byref(what), C.byref(res)) == INV
    assert eng.api.remove_particles(eng.ctx, 0, None, C.byref(res)) == INV
    what.reserved[2], what.regions = 0, None
    assert eng.api.remove_particles(eng.ctx, 0, C.byref(what), C.byref(res)) == INV          # regions missing
    # capacity one short: refused with the true counts
    sel = int(prm.selected(eng.retrieve_positions(0), [sph]).sum())
    buf = np.empty((sel, 3), np.float32)
    what.regions, what.removed_xyz, what.capacity = arr, buf.ctypes.data, sel - 1
    assert eng.api.remove_particles(eng.ctx, 0, C.byref(what), C.byref(res)) == _ffi.MPM_ERR_CAPACITY and int(res.removed[0]) == sel and res.relaid == 0
    assert_unchanged(eng, before, "a reserved word, a NULL removal, NULL regions, capacity one short")
    # between mpm_grid_update and mpm_rebuild_partition the grid holds velocities
    eng.grid_update(1e-5)
    refused(eng, INV, "holds velocities", regions=sph)
    eng.g2p2g(1e-5, 1e-5)
    refused(eng, INV, "holds velocities", regions=sph)
    eng.rebuild_partition()
    # ids that are not valid: a tracked context between load_checkpoint and load_particle_ids
    ck, ids = eng.save_checkpoint().copy(), eng.save_particle_ids().copy()
    eng.load_checkpoint(ck)
    with pytest.raises(EngineError) as e:
        eng.remove(regions=sph)
    assert e.value.code == INV and "ids" in str(e.value) and np.array_equal(eng.save_checkpoint(), ck)
    eng.load_particle_ids(ids)
    sel = int(prm.selected(eng.retrieve_positions(0), [sph]).sum())         # (the substep in between has moved the particles)
    assert remove_checked(eng, sph, tag="after the refusals the same call is accepted")["removed"] == [sel] and sel > 0
    # a context that has been through the halo tagging
    assert eng.api.halo_tag_begin(eng.ctx) == 0 and eng.api.halo_tag_end(eng.ctx, C.byref(C.c_int(0)), (C.c_int * 32)()) == 0
    refused(eng, INV, "group", regions=sph)
    eng.close()
    eng = set_up(scene_of([model_dict(gm.FC, gm.scene_cluster())]))
    refused(eng, INV, "tracked context", ids=[1, 2], model=0)
    eng.close()


# ---- the re-laid state is one the substep kernels accept ---------------------------------------------------------------------------------------------------
def test_one_substep_from_the_relaid_state_against_the_model_and_the_books():
    """remove from the bench's context; then one substep from the state READ BACK after the removal, with an injected velocity field, against
    g2p2g_model - every particle and every node, under test_g2p2g_blocks_gpu's bounds - and the books verifier, as emission's test of this name does"""
    from test_g2p2g_blocks_gpu import check
    from test_rebuild_books_gpu import books
    material = gm.FC
    pos, st = gm.scene_state("cluster", material)
    bench = gb.Bench([(material, pos)])
    try:
        bench.inject([st], lambda keys: gm.grid_of(keys, "rest"))
        bench.eng.g2p2g(gm.DT, gm.NEW_DT)
        bench.eng.rebuild_partition()                              # the lists now carry neighbour tags: both walks follow them
        p0 = bench.read(0)
        gone = prm.selected(p0["pos"] * DX, [REGIONS["sphere"]])
        res = bench.eng.remove(regions=REGIONS["sphere"])
        assert res["removed"] == [int(gone.sum())] and 0 < gone.sum() < gone.size
        bench.parts = [(material, p0["pos"][~gone])]
        back = bench.read(0)
        ck = bench.eng.save_checkpoint().copy()
        for seed in range(1, 65):                                 # (the field is re-drawn until no particle sits on the brink of a branch, as test_second_substep does)
            m2 = gm.step(bench.consts[0], back["pos"], gm.gather_field(back["pos"], "flow", seed), b6=back["b6"], reflected=back["reflected"], logjp=None, J=None)
            if not m2["unstable"].any():
                break
        bench.load(ck, lambda keys: gm.grid_of(keys, "flow", seed=seed))
        out = bench.step()
        bench.parts = [(material, back["pos"])]
        check(bench, out, [m2], "flow", "one substep after a removal")
        _, _, found = books(bench.eng, 1)
        assert not found, found[:10]
    finally:
        bench.close()


def test_a_checkpoint_saved_after_a_removal_loads_and_both_run_on_identically():
    """a context sized by n - what the models were ever given - loads the checkpoint; what was loaded is there bit for bit, its books balance over
    the run that follows, and the same window in both contexts agrees within tests/test_checkpoint_gpu.py's 2e-6 (two runs of one context differ
    in the last bits too: the P2G sums with float atomics)"""
    pos = gm.scene_cluster()
    sc = scene_of([model_dict(gm.SAND, pos, v0=(0.2, 0.0, 0.1))], track_ids=True)
    a = set_up(sc)
    a.run_fixed(4, 1e-4)
    k = a.remove(regions=REGIONS["box"])["removed"][0]
    ck, ids = a.save_checkpoint().copy(), a.save_particle_ids().copy()
    b = set_up(sc)
    b.load_checkpoint(ck)
    b.load_particle_ids(ids)
    pa, pb = read_particles(a, 0), read_particles(b, 0)
    ga, gb_ = pem.grid_by_node(*a.dump_grid(), BITS), pem.grid_by_node(*b.dump_grid(), BITS)
    assert pem.same_set(pa, pb) and np.array_equal(pa["ids"], pb["ids"]) and pa["ids"].shape[0] == pos.shape[0] - k
    assert np.array_equal(ga[0], gb_[0]) and np.array_equal(ga[1].view(np.uint32), gb_[1].view(np.uint32))
    for eng in (a, b):
        eng.run_fixed(16, 1e-4)
        assert int(eng.counts().particles[0]) == pos.shape[0] - k
    pa, pb = read_particles(a, 0), read_particles(b, 0)
    a.close()
    b.close()
    assert np.array_equal(pa["ids"], pb["ids"])
    xa, xb = pa["xyz"].astype(np.float64), pb["xyz"].astype(np.float64)
    rel = (np.abs(xa - xb).max(axis=1) / np.abs(xb).max(axis=1)).max()
    print(f"after 16 substeps in both contexts: positions within {rel:.3g} (relative)")
    assert rel < 2e-6


def test_removal_after_particles_were_lost_keeps_the_books():
    """test_emission_after_particles_were_lost_keeps_the_books' bench: particles leave through the upper x face and are counted as lost; a removal
    then re-lays fewer particles than the model was given, and every host synchronisation of the run that follows balances the books"""
    pos = np.concatenate([gm.scene_cluster(), gm.block_particles((15, 6, 6), 60, np.random.default_rng(15))])
    st = gm.make_state(gm.FC, pos.shape[0], 40)
    out_x = np.float32(3.9 * float(DX) / gm.DT)
    bench = gb.Bench([(gm.FC, pos)])
    try:
        bench.inject([st], lambda keys: np.tile(np.float32([out_x, 0, 0])[None, :, None], (keys.shape[0], 1, 64)))
        bench.eng.g2p2g(gm.DT, gm.NEW_DT)
        bench.eng.rebuild_partition()
        eng = bench.eng
        lost, held = int(eng.diagnostics().lost_particles), int(eng.counts().particles[0])
        assert lost > 0 and held + lost + int(eng.diagnostics().dropped_particles) == pos.shape[0]
        x = eng.retrieve_positions(0)
        region = {"kind": "halfspace", "point": tuple(np.median(x.astype(np.float64), axis=0)), "normal": (0.0, 1.0, 0.0)}
        k = eng.remove(regions=region)["removed"][0]
        assert k == int(prm.selected(x, [region]).sum()) and 0 < k < held
        assert int(eng.counts().particles[0]) == held - k and int(eng.diagnostics().lost_particles) == lost
        eng.run_fixed(16, 1e-5)
        d = eng.diagnostics()
        assert int(eng.counts().particles[0]) + int(d.lost_particles) + int(d.dropped_particles) + k == pos.shape[0]
    finally:
        bench.close()


# ---- the velocity field carries over ----------------------------------------------------------------------------------------------------------------------
def test_the_survivors_stay_in_the_velocity_field_they_were_in():
    """a stress-free blob at gravity 0 with one v0, half of it removed: the rescaled nodes keep p / m, so retrieve_velocity returns v0 within
    test_uniform_translation_after_setup_all_materials' bound (1e-6 |v0|), and k substeps move every survivor by k dt v0 within that bound per
    step plus the rounding of a stored position (cell units below 2^6: 2^-24 of the domain per step, and once more for the readout)"""
    bits, k, dt = BITS, 10, 1e-4
    v0 = np.array((0.3, -0.7, 1.1))
    blob = scenes.lattice_sphere(bits, (0.5, 0.5, 0.5), 6.0)
    sc = {"name": "remove_field", "bits": bits, "dt": dt, "config": {"max_ppc": MAX_PPC, "gravity": 0.0},
          "models": [{"material": _ffi.FIXED_COROTATED, "xyz": blob, "v0": tuple(v0), "params": {"volume": scenes._vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}],
          "track_ids": True}
    eng = set_up(sc)
    res = remove_checked(eng, {"kind": "halfspace", "point": (0.5, 0.5, 0.5), "normal": (1.0, 0.3, 0.0)}, tag="half a blob")
    assert blob.shape[0] // 3 < res["removed"][0] < 2 * blob.shape[0] // 3
    x, v = eng.retrieve_velocity(0)
    ids0, x = eng.order_by_id(0, x)
    err = np.linalg.norm(v.astype(np.float64) - v0, axis=1).max()
    bound = 1e-6 * np.linalg.norm(v0)
    print(f"survivors' v_p: {err / bound:.3f} of the readout test's bound")
    assert err <= bound
    eng.run_fixed(k, dt)
    ids1, x1 = eng.order_by_id(0, eng.retrieve_positions(0))
    eng.close()
    assert np.array_equal(ids0, ids1)
    moved = np.abs(x1.astype(np.float64) - (x.astype(np.float64) + k * dt * v0)).max()
    print(f"after {k} substeps: {moved:.3g}, bound {k * (dt * bound + 2.0 ** -24) + 2.0 ** -24:.3g}")
    assert moved <= k * (dt * bound + 2.0 ** -24) + 2.0 ** -24


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------------------------
def test_a_blob_flies_on_as_the_oracle_flies_it_alone_after_its_neighbour_was_removed():
    """two blobs with no common grid node, under gravity: K substeps, blob 1 removed whole, L more; blob 2 against the oracle flying blob 2 alone
    for K + L = 20 substeps, under test_an_emitted_blob_flies_as_the_oracle_flies_it_from_set_up's bound for its 20 substeps"""
    from parity_util import match, run_engine
    from oracle_ffi import oracle_api
    bits, K, L, dt = 6, 5, 15, 1e-4
    prm_ = {"volume": scenes._vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    one = scenes.lattice_sphere(bits, (0.3, 0.6, 0.5), 4.0)
    two = scenes.lattice_box(bits, (40, 20, 28), (46, 26, 34))
    v0 = (1.0, 0.5, -0.25)
    sc = {"name": "remove_flight", "bits": bits, "dt": dt, "config": {"max_ppc": 16},
          "models": [{"material": _ffi.FIXED_COROTATED, "xyz": one, "v0": (0, 0, 0), "params": dict(prm_)},
                     {"material": _ffi.FIXED_COROTATED, "xyz": two, "v0": v0, "params": dict(prm_)}]}
    assert not np.isin(pem.reached_nodes(one, bits), pem.reached_nodes(two, bits)).any()
    eng = set_up(sc)
    eng.run_fixed(K, dt)
    g0 = pem.grid_by_node(*eng.dump_grid(), bits)
    res = remove_checked(eng, {"kind": "sphere", "center": (0.3, 0.6, 0.5), "radius": 8.0 * float(DX)}, tag="blob 1 whole")
    assert res["removed"] == [one.shape[0], 0]
    g1 = pem.grid_by_node(*eng.dump_grid(), bits)
    keep = np.isin(g0[0], g1[0])
    assert np.array_equal(g0[1][keep].view(np.uint32), g1[1].view(np.uint32)), "blob 2's nodes are untouched bit for bit"
    eng.run_fixed(L, dt)
    xh = eng.retrieve_positions(1)
    eng.close()
    alone = dict(sc, models=[sc["models"][1]])
    xo = run_engine(alone, K + L, dt, api=oracle_api())["state"][0][0]
    idx, _ = match(xo.astype(np.float64), xh.astype(np.float64))
    rel = (np.abs(xh[idx].astype(np.float64) - xo).max(axis=1) / np.abs(xo).max(axis=1)).max()
    print(f"blob 2 after {K} + {L} substeps: positions within {rel:.3g} (relative) of the oracle's run alone")
    assert xh.shape == xo.shape and rel < 1e-5                 # parity_util's position bound (smoke(): pos_rel < 1e-5)


# ---- scenes and drivers ---------------------------------------------------------------------------------------------------------------------------------------
def test_fountain_through_main_loop_reaches_a_steady_state():
    """the faucet with a sink box over the floor: the live count stops growing - its last-frame count is not above its count at two thirds of the
    run plus one emitted layer - and everything emitted is either live or removed"""
    sc = scenes.fountain(bits=BITS, radius_cells=2.0, speed=8.0, height_cells=16, sink_cells=4.0, end=1.0)
    eng = build_engine(sc)
    layer = scenes.Emitter.from_dict(BITS, sc["emitters"][0]).layer.shape[0]
    seen = []

    def on_frame(frame, e):
        seen.append((e.cur_time, int(e.counts().particles[0]), e.models[0]["n"], e.models[0]["removed"]))
    eng.main_loop(6, 250, 1e-4, on_frame=on_frame)
    d = eng.diagnostics()
    eng.close()
    print("fountain frames (time, live, emitted, removed):", seen)
    assert all(live + removed == n for _, live, n, removed in seen) and (int(d.lost_particles), int(d.dropped_particles)) == (0, 0)
    assert seen[-1][3] > 0 and seen[-1][2] > seen[3][2], "the tap still runs and the drain drains"
    assert seen[-1][1] <= seen[3][1] + layer


def test_gmpm_serves_the_sinks_of_a_scene_file(tmp_path):
    """gmpm on a falling J-fluid block with a half-space sink under it: the frames' point counts shrink, and removed_frame*.json sums to the
    difference between frame 0 and the last frame"""
    import __graft_entry__ as g
    from bgeo_reader import read_bgeo
    g.build_host()
    model = {"file": "box", "constitutive": "jfluid", "rho": 1e3, "volume": float(np.float32((1 / 64) ** 3 / 8)), "offset": [0.4, 0.3, 0.4], "span": [0.2, 0.2, 0.2], "velocity": [0, -4.0, 0]}
    sim = {"gpuid": 0, "fps": 100, "frames": 3, "default_dt": 1e-4, "domain_bits": BITS, "max_ppc": 16, "output_dir": str(tmp_path), "output_removed": True}
    sinks = [{"shape": "halfspace", "point": [0.5, 0.3, 0.5], "normal": [0, 1, 0], "model": 0, "start": 0.0, "period": 2e-3}]
    (tmp_path / "scene.json").write_text(json.dumps({"simulation": sim, "models": [model], "sinks": sinks}))
    out = subprocess.check_output([os.path.join(os.path.dirname(HERE), "claymore_amd", "host", "gmpm"), "-f", str(tmp_path / "scene.json")], text=True, timeout=300)
    counts = [read_bgeo(tmp_path / f"model_id[0]_frame[{f}].bgeo")[0].shape[0] for f in (0, 1, 2, 3)]
    removed = [json.loads((tmp_path / f"removed_frame[{f}].json").read_text()) for f in (1, 2, 3)]
    print("gmpm frames:", counts, [r["removed"] for r in removed], out[-300:])
    assert counts[0] > counts[1] > counts[2] > counts[3] > 0
    assert [r["removed"][0] for r in removed] == [counts[f] - counts[f + 1] for f in range(3)]
    assert all(r["mass"] > 0 and r["momentum"][1] < 0 for r in removed)


# ---- both list layouts ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_sliced_layout_passes_too():
    """Everything above runs with the list layout this process was given (default: the pair layout for all four materials).  The region, site,
    material, model and id tests run once more in a fresh child process with MPM_G2P2G_PAIRS=0 - every model in the sliced layout, whose lists
    have holes that the walks skip - as emission's last test does; a child that ends on a signal or at its time limit fails the test, and nothing
    is tried again."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "shape_kind or overlap or whole_block or full_block or every_material or two_models or tracked"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

"""Particle emission on the GPU (mpm_emit_particles, Engine.emit; claymore_amd/csrc/mpm_particle_emit.hpp) against the NumPy statement of its
contract (tests/particle_emit_model.py): after every emission the model holds the old particles and the new ones, each with the bits it had or
was given; a grid node no new stencil reaches has the bits it had; a reached node holds the old value plus the new particles' set-up P2G within
a bound counted from the roundings (particle_init_model's per-term count, plus one addition per contributing workgroup - at most 8 - and one
for the old value, relative to the sum of magnitudes); the table checks, the counts follow, the cumulative counters stay.  A refused call leaves
the checkpoint byte for byte as it was.  No bound here was fitted to what the kernels return."""
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

import ckpt_format as cf  # noqa: E402
import face_scenes as fs  # noqa: E402
import g2p2g_bench as gb  # noqa: E402
import g2p2g_model as gm  # noqa: E402
import particle_emit_model as pem  # noqa: E402
import particle_init_model as pim  # noqa: E402
from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import EngineError, build_engine  # noqa: E402

pytestmark = pytest.mark.gpu

BITS, MAX_PPC = gm.BITS, gm.MAX_PPC
DX = np.float32(0.5 ** BITS)
U = pim.U


def model_dict(material, pos_cells, **extra):
    return dict({"material": material, "xyz": np.ascontiguousarray(pos_cells, np.float32).reshape(-1, 3) * DX, "v0": (0.0, 0.0, 0.0),
                 "params": dict(gm.material_overrides(material))}, **extra)


def scene_of(models, bits=BITS, max_ppc=MAX_PPC, config=None, **extra):
    return dict({"name": "particle_emit", "bits": bits, "dt": gm.DT, "config": dict({"max_ppc": max_ppc}, **(config or {})), "models": models}, **extra)


def set_up(sc):
    eng = build_engine(sc)
    eng.initial_setup()
    return eng


def state9_of(material, st):
    if material == gm.J_FLUID:
        s = np.zeros((st["J"].shape[0], 9), np.float32)
        s[:, 0] = st["J"]
        return s
    b = st["b6"]
    s = np.stack([np.where(st["reflected"], -b[:, 0], b[:, 0]), b[:, 3], b[:, 4], b[:, 3], b[:, 1], b[:, 5], b[:, 4], b[:, 5], b[:, 2]], axis=1)
    return np.ascontiguousarray(s, np.float32)


def read_particles(eng, m):
    """model m as a particle dict of particle_emit_model: xyz, state9, logjp (+ ids in a tracked engine)"""
    x, s9, lj = eng.retrieve_state(m)
    if not eng.track_ids:
        return {"xyz": x.copy(), "state9": s9.copy(), "logjp": lj.copy(), "ids": None}
    ids, x, s9, lj = eng.order_by_id(m, x, s9, lj)
    return {"xyz": x, "state9": s9, "logjp": lj, "ids": ids.astype(np.int32)}


def snapshot(eng):
    """what a refused call must leave as it was"""
    out = {"ckpt": eng.save_checkpoint().copy(), "capacity": eng.capacity(), "n": [m["n"] for m in eng.models]}
    if eng.track_ids:
        out["ids"] = eng.save_particle_ids().copy()
    d = eng.diagnostics()
    out["diag"] = (int(d.lost_particles), int(d.discarded_p2g), int(d.dropped_particles), int(d.overflow_flags), int(d.still_rebuilds))
    return out


def assert_unchanged(eng, before, why):
    after = snapshot(eng)
    assert np.array_equal(after["ckpt"], before["ckpt"]), f"{why}: the checkpoint changed"
    assert after["capacity"] == before["capacity"] and after["n"] == before["n"] and after["diag"] == before["diag"], why
    if "ids" in before:
        assert np.array_equal(after["ids"], before["ids"]), why


def refused(eng, code, word, model, xyz, **kw):
    before = snapshot(eng)
    with pytest.raises(EngineError) as e:
        eng.emit(model, xyz, **kw)
    assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
    assert_unchanged(eng, before, word)


def emit_checked(eng, model, new_cells, v0=(0.0, 0.0, 0.0), velocity=None, affine=None, state=None, logjp=None, tag=""):
    """Engine.emit, then everything the contract says, against particle_emit_model.  state: state_kind "b".  Returns first_id."""
    nm = len(eng.models)
    material = eng.models[model]["material"]
    prm = eng.models[model]["params"]
    xyz = np.ascontiguousarray(new_cells, np.float32).reshape(-1, 3) * DX
    n = xyz.shape[0]
    before = [read_particles(eng, m) for m in range(nm)]
    flat0, val0 = pem.grid_by_node(*eng.dump_grid(), BITS)
    cnt0, d0, tot0, old_n = eng.counts(), eng.diagnostics(), eng.grid_totals(), eng.models[model]["n"]
    cap0 = eng.capacity()
    first = eng.emit(model, xyz, v0=v0, velocity=velocity, affine=affine, state=state, logjp=logjp)
    assert first == old_n and eng.models[model]["n"] == old_n + n
    assert eng.api.check_table(eng.ctx) == 0
    # the particles: old and new, bit for bit, as sets
    has_lj = material in (gm.SAND, gm.NACC)
    new = {"xyz": xyz, "state9": pem.default_state9(material == gm.J_FLUID, n) if state is None else np.ascontiguousarray(state, np.float32).reshape(n, 9),
           "logjp": np.full(n, np.float32(prm.log_jp0) if has_lj else np.float32(0), np.float32) if (logjp is None or not has_lj) else np.asarray(logjp, np.float32),
           "ids": pem.new_ids(old_n, n) if eng.track_ids else None}
    for m in range(nm):
        want = pem.merged_particles(before[m], new) if m == model else before[m]
        if not eng.track_ids:
            want = dict(want, ids=None)
        assert pem.same_set(read_particles(eng, m), want), (tag, "particles of model", m)
    # the grid, node by node
    flat1, val1 = pem.grid_by_node(*eng.dump_grid(), BITS)
    assert np.isin(flat0, flat1).all(), "a node of the old grid is gone"
    old1 = np.zeros_like(val1)
    old1[np.searchsorted(flat1, flat0)] = val0
    reached = np.isin(flat1, pem.reached_nodes(xyz, BITS))
    assert np.array_equal(val1[~reached].view(np.uint32), old1[~reached].view(np.uint32)), (tag, "an untouched node changed (or a new block does not start at zero)")
    sc_new = pem.new_particle_scene(BITS, {"volume": prm.volume, "rho": prm.rho}, xyz, v0, velocity, affine)
    flat_w, want, bound = pem.expected_grid(flat0, val0, sc_new)
    assert np.isin(flat_w, flat1).all(), "a node that receives mass lies in no registered block"
    at = np.searchsorted(flat1, flat_w)
    err = np.abs(val1[at].astype(np.float64) - want)
    print(f"{tag}: {n} particles into model {model}, {flat_w.size} reached nodes of {flat1.size}; worst error / bound per channel {(err / bound).max(axis=0)}")
    assert (err <= bound).all(), (tag, np.argwhere(err > bound)[:5])
    massless = reached.copy()
    massless[at] = False
    assert np.array_equal(val1[massless].view(np.uint32), old1[massless].view(np.uint32))
    # counts, totals, counters, capacities
    cnt1, d1, tot1 = eng.counts(), eng.diagnostics(), eng.grid_totals()
    for m in range(nm):
        assert int(cnt1.particles[m]) == int(cnt0.particles[m]) + (n if m == model else 0)
    assert (int(d1.lost_particles), int(d1.discarded_p2g), int(d1.dropped_particles)) == (int(d0.lost_particles), int(d0.discarded_p2g), int(d0.dropped_particles))
    added = (want - old1[at].astype(np.float64)).sum(axis=0)
    slack = 8 * U * np.abs(val1).astype(np.float64).sum(axis=0) * 2.0 ** -29          # (the float64 totals' own additions)
    assert (np.abs(tot1 - (tot0 + added)) <= bound.sum(axis=0) + slack).all(), (tot1, tot0 + added)
    assert eng.particle_momentum()["count"] == sum(int(cnt1.particles[m]) for m in range(nm))
    assert eng.capacity()[2] >= cap0[2]
    return first


# ---- where the new particles land ----------------------------------------------------------------------------------------------------------------
LANDINGS = {"a cell that holds particles": gm.CLUSTER[0], "a neighbour-tier block": (8, 6, 6), "an exterior-tier block": (5, 6, 6), "a block nobody registered": (12, 12, 12)}


@pytest.mark.parametrize("where", sorted(LANDINGS))
def test_new_particles_land(where):
    rng = np.random.default_rng(5)
    eng = set_up(scene_of([model_dict(gm.FC, gm.scene_cluster())]))
    new = gm.block_particles(LANDINGS[where], 40, rng)
    v, Cm = rng.uniform(-2.0, 2.0, (40, 3)).astype(np.float32), rng.uniform(-50.0, 50.0, (40, 3, 3)).astype(np.float32)
    emit_checked(eng, 0, new, velocity=v, affine=Cm, tag=where)
    eng.run_fixed(3, 1e-5)
    assert int(eng.counts().particles[0]) == eng.models[0]["n"] and eng.api.check_table(eng.ctx) == 0
    eng.close()


def test_new_particles_land_in_the_outermost_cells_of_the_six_faces():
    """face_scenes' slabs - cells -2 / -1 of the lower faces, the top cells, corners and edges - emitted beside the cluster: node -1 is dropped and
    the blocks beyond the upper faces do not exist, as at set-up"""
    eng = set_up(scene_of([model_dict(gm.FC, gm.scene_cluster())]))
    new = fs.setup_slab_cells(BITS)
    rng = np.random.default_rng(6)
    v, Cm = rng.uniform(-2.0, 2.0, (new.shape[0], 3)).astype(np.float32), rng.uniform(-50.0, 50.0, (new.shape[0], 3, 3)).astype(np.float32)
    emit_checked(eng, 0, new, velocity=v, affine=Cm, tag="six faces")
    g = pim.setup_nodes(pem.new_particle_scene(BITS, {}, new * DX))
    assert g["outside"]["lo"] > 0 and g["outside"]["hi"] > 0
    eng.close()


# ---- sizes that cross a boundary of the layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", [gm.SAND, gm.J_FLUID], ids=["sand", "jfluid"])
def test_sizes_that_cross_a_boundary_of_the_layout(material):
    """63 -> 64 -> 65 records (the bin edge), 511 -> 513 and 768 -> 769 (the pair layout's chunk and tail rule), 1023 -> 1024 = max_ppc * 64
    (accepted) and one more (refused, nothing changed), n = 1 all along, and n = 0"""
    rng = np.random.default_rng(7)
    full = MAX_PPC * 64
    sites = {63: gm.SITES[0], 511: gm.SITES[5], 768: gm.SITES[10], full - 1: gm.SITES[15]}
    pools = {k: gm.block_particles(key, k + 2, rng) for k, key in sites.items()}
    eng = set_up(scene_of([model_dict(material, np.concatenate([pools[k][:k] for k in sites]))]))
    emit_checked(eng, 0, pools[63][63:64], tag="63 -> 64")
    emit_checked(eng, 0, pools[63][64:65], tag="64 -> 65")
    emit_checked(eng, 0, pools[511][511:513], tag="511 -> 513")
    emit_checked(eng, 0, pools[768][768:769], tag="768 -> 769")
    emit_checked(eng, 0, pools[full - 1][full - 1:full], tag="a block filled to max_ppc * 64")
    refused(eng, _ffi.MPM_ERR_CAPACITY, "max_ppc*64", 0, pools[full - 1][full:full + 1] * DX)
    before = snapshot(eng)
    assert eng.emit(0, np.zeros((0, 3), np.float32)) == eng.models[0]["n"]
    assert_unchanged(eng, before, "n = 0")
    eng.run_fixed(2, 1e-5)
    assert int(eng.counts().particles[0]) == eng.models[0]["n"] == sum(sites) + 6
    eng.close()


# ---- materials, models, arrays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS, ids=[gm.NAMES[m] for m in gm.MATERIALS])
def test_every_material_with_and_without_the_arrays(material):
    """into the cluster's own blocks: a deformed state, log Jp, velocities and APIC matrices; then - without a substep between - plain particles,
    which start stress-free at log_jp0 with v0"""
    pos, st = gm.scene_state("cluster", material)
    eng = set_up(scene_of([model_dict(material, pos, state=state9_of(material, st), logjp=st["logjp"])]))
    extra = gm.EXTRA_SCENES["cluster_b"]()
    se = gm.make_state(material, extra.shape[0], 31)
    rng = np.random.default_rng(8)
    v, Cm = rng.uniform(-2.0, 2.0, (extra.shape[0], 3)).astype(np.float32), rng.uniform(-50.0, 50.0, (extra.shape[0], 3, 3)).astype(np.float32)
    emit_checked(eng, 0, extra, velocity=v, affine=Cm, state=state9_of(material, se), logjp=se["logjp"], tag=f"{gm.NAMES[material]} with arrays")
    emit_checked(eng, 0, gm.block_particles(gm.CLUSTER[3], 20, rng), v0=(0.5, -1.0, 0.25), tag=f"{gm.NAMES[material]} plain")
    emit_checked(eng, 0, gm.block_particles(gm.CLUSTER[5], 20, rng), velocity=v[:20], tag=f"{gm.NAMES[material]} velocity only")
    emit_checked(eng, 0, gm.block_particles(gm.CLUSTER[6], 20, rng), affine=Cm[:20], v0=(0.0, 1.0, 0.0), state=state9_of(material, se)[:20], tag=f"{gm.NAMES[material]} affine and state")
    eng.close()


def test_state_given_as_deformation_gradients():
    pos = gm.scene_cluster()
    eng = set_up(scene_of([model_dict(gm.FC, pos)]))
    extra = gm.EXTRA_SCENES["cluster_b"]()[:200]
    st = gm.make_state(gm.FC, extra.shape[0], 32)
    eng.emit(0, extra * DX, state=st["F32"], state_kind="f")
    x, s9, _ = eng.retrieve_state(0)
    eng.close()
    keys = {tuple(r) for r in (extra * DX).view(np.uint32).tolist()}
    new = np.array([tuple(r) in keys for r in x.view(np.uint32).tolist()])
    assert new.sum() == extra.shape[0]
    og, ow = gb.by_position_bits(x[new]), gb.by_position_bits(extra * DX)
    F = st["F32"].astype(np.float64)[ow]
    want = F @ F.transpose(0, 2, 1)
    bound = (3 + 2) * U * (np.abs(F) @ np.abs(F).transpose(0, 2, 1))      # three products and two additions, as test_particle_init_gpu counts them
    got = s9[new][og].astype(np.float64).reshape(-1, 3, 3)
    refl = np.signbit(got[:, 0, 0])
    got[:, 0, 0] = np.abs(got[:, 0, 0])
    assert (np.abs(got - want) <= bound).all() and np.array_equal(refl, np.linalg.det(F) < 0)


def test_two_models_sharing_blocks_an_empty_model_and_an_all_empty_context():
    pa, pb = gm.scene_cluster(), gm.EXTRA_SCENES["cluster_b"]()
    half = pb.shape[0] // 2
    sa, sb = gm.make_state(gm.SAND, pa.shape[0], 81), gm.make_state(gm.J_FLUID, pb.shape[0], 82)
    eng = set_up(scene_of([model_dict(gm.SAND, pa, state=state9_of(gm.SAND, sa), logjp=sa["logjp"]), model_dict(gm.J_FLUID, pb[:half], state=state9_of(gm.J_FLUID, sb)[:half]),
                           model_dict(gm.NACC, np.zeros((0, 3), np.float32))]))
    emit_checked(eng, 1, pb[half:], state=state9_of(gm.J_FLUID, sb)[half:], v0=(0.0, -1.0, 0.0), tag="the second of two models sharing blocks")
    pc = gm.scene_isolated()
    lj = np.linspace(-0.02, 0.005, pc.shape[0]).astype(np.float32)
    emit_checked(eng, 2, pc, logjp=lj, tag="a model that was added empty")
    eng.run_fixed(3, 1e-5)
    cnt = eng.counts()
    assert [int(cnt.particles[m]) for m in range(3)] == [pa.shape[0], pb.shape[0], pc.shape[0]]
    eng.close()
    eng = set_up(scene_of([model_dict(gm.FC, np.zeros((0, 3), np.float32)), model_dict(gm.J_FLUID, np.zeros((0, 3), np.float32))]))
    assert eng.counts().particle_blocks == 0
    emit_checked(eng, 1, pb, v0=(0.0, -1.0, 0.0), tag="a context whose models are all empty")
    eng.run_fixed(3, 1e-5)
    assert int(eng.counts().particles[1]) == pb.shape[0] and int(eng.counts().particles[0]) == 0
    eng.close()


def test_linear_field_of_a_lone_emitted_blob_is_reproduced_by_the_readout():
    """test_linear_field_is_reproduced_by_grid_and_readout's ball, emitted into an empty model with its field as per-particle arrays: the grid is
    the set-up grid's and retrieve_velocity returns the field, under that test's bounds (0 + x is exact: the old value adds no rounding)"""
    sc = scenes.spinning_ball(bits=6)
    sc["config"] = dict(sc["config"], max_ppc=16)
    m = sc["models"][0]
    a, A = scenes.model_velocity_field(m)
    x64 = m["xyz"].astype(np.float64)
    vel = (a[None, :] + x64 @ A.T).astype(np.float32)
    aff = np.broadcast_to(A.astype(np.float32), (x64.shape[0], 3, 3)).copy()
    g = pim.setup_nodes(sc)
    nb = pim.node_bounds(g, extra_momentum=pim.R_FIELD)
    empty = {k: v for k, v in m.items() if k not in ("omega", "velocity_gradient", "pivot")}
    empty["xyz"] = np.zeros((0, 3), np.float32)
    eng = set_up(dict(sc, models=[empty]))
    eng.emit(0, m["xyz"], velocity=vel, affine=aff)
    nodes, val = pim.dumped_nodes(*eng.dump_grid(), 6)
    assert np.array_equal(nodes, g["nodes"]) and (np.abs(val - g["val"]) <= nb).all()
    x, v, Cp = eng.retrieve_velocity(0, affine=True)
    eng.close()
    want = a[None, :] + x.astype(np.float64) @ A.T
    ev, ec = np.abs(v - want).max(axis=1), np.abs(Cp.astype(np.float64) - A[None]).max(axis=(1, 2))
    bv, bc = pim.linear_field_bounds(g, nb, x, 6, a, A)
    print(f"emitted ball: v_p error {(ev / bv).max():.3f}, C_p error {(ec / bc).max():.3f} of their bounds")
    assert x.shape[0] == m["xyz"].shape[0] and (ev <= bv).all() and (ec <= bc).all()


# ---- tracked ids -----------------------------------------------------------------------------------------------------------------------------------
def test_tracked_ids_old_unchanged_new_contiguous_two_emissions_in_a_row():
    rng = np.random.default_rng(9)
    pos = gm.scene_block_sizes()
    eng = set_up(scene_of([model_dict(gm.FC, pos, v0=(0.3, 0.0, -0.2))], track_ids=True))
    eng.run_fixed(3, 1e-4)                                        # the ids have been through G2P2G: they no longer sit where set-up put them
    n0 = pos.shape[0]
    a, b = gm.block_particles(gm.SITES[3], 70, rng), gm.block_particles((12, 12, 9), 5, rng)
    assert emit_checked(eng, 0, a, v0=(0.0, -1.0, 0.0), tag="tracked, first") == n0
    assert emit_checked(eng, 0, b, tag="tracked, second") == n0 + 70
    ids, x = eng.order_by_id(0, eng.retrieve_positions(0))
    assert np.array_equal(ids, np.arange(n0 + 75))
    assert np.array_equal(x[n0:].view(np.uint32), (np.concatenate([a, b]) * DX).view(np.uint32)), "row old n + i of the model is input row i"
    eng.run_fixed(3, 1e-4)
    assert np.array_equal(np.sort(eng.retrieve_ids(0)[1]), np.arange(n0 + 75))
    eng.close()


# ---- capacity --------------------------------------------------------------------------------------------------------------------------------------
def test_block_and_bin_capacities_refuse_with_grow_0_and_grow_with_grow_1():
    rng = np.random.default_rng(10)
    pos = gm.scene_cluster()
    far = gm.block_particles((12, 12, 12), 10, rng)
    many = np.concatenate([gm.block_particles(k, 800, rng) for k in gm.CLUSTER])       # 8 x ~1000 particles: 8 x 16 bins, more than n / 64 + 64 + 1
    eng = set_up(scene_of([model_dict(gm.FC, pos)], config={"max_blocks": 64, "grow": 0}))
    assert eng.counts().exterior_blocks == 64
    refused(eng, _ffi.MPM_ERR_CAPACITY, "block capacity", 0, far * DX)
    refused(eng, _ffi.MPM_ERR_CAPACITY, "bin capacity", 0, many * DX)
    emit_checked(eng, 0, gm.block_particles(gm.CLUSTER[2], 30, rng), tag="what fits is accepted with grow = 0")
    assert eng.capacity()[2] == 0
    eng.close()
    eng = set_up(scene_of([model_dict(gm.FC, pos)], config={"max_blocks": 64, "grow": 1}))
    emit_checked(eng, 0, far, tag="blocks grow")
    blocks, bins, events = eng.capacity()
    assert blocks > 64 and events >= 1
    emit_checked(eng, 0, many, tag="bins grow")
    assert eng.capacity()[2] > events and eng.capacity()[1][0] >= int(eng.counts().bins[0])
    eng.run_fixed(2, 1e-5)
    assert int(eng.counts().particles[0]) == eng.models[0]["n"]
    eng.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_changes_nothing():
    rng = np.random.default_rng(11)
    pos = gm.scene_cluster()
    new = gm.block_particles((9, 9, 9), 6, rng) * DX
    eng = build_engine(scene_of([model_dict(gm.SAND, pos)], track_ids=True))
    with pytest.raises(EngineError) as e:
        eng.emit(0, new)
    assert e.value.code == _ffi.MPM_ERR_NOT_READY
    eng.initial_setup()
    eng.run_fixed(2, 1e-5)
    INV = _ffi.MPM_ERR_INVALID
    refused(eng, INV, "no model", 1, new)
    refused(eng, INV, "no model", -1, new)
    before = snapshot(eng)
    assert eng.api.emit_particles(eng.ctx, 0, None, 3, None, None, None) == INV
    init = _ffi.ParticleInit()
    init.reserved[1] = 1
    assert eng.api.emit_particles(eng.ctx, 0, new.ctypes.data, new.shape[0], None, C.byref(init), None) == INV
    init, ident = _ffi.ParticleInit(), np.tile(np.eye(3, dtype=np.float32).ravel(), (6, 1))
    init.state9, init.state_kind = ident.ctypes.data, 7
    assert eng.api.emit_particles(eng.ctx, 0, new.ctypes.data, new.shape[0], None, C.byref(init), None) == INV
    assert_unchanged(eng, before, "NULL xyz, a reserved word, an unknown state_kind")
    good = {"velocity": np.zeros((6, 3), np.float32), "affine": np.zeros((6, 3, 3), np.float32), "state": np.tile(np.eye(3, dtype=np.float32).ravel(), (6, 1)), "logjp": np.zeros(6, np.float32)}
    for k, arr in good.items():
        for bad in (np.nan, np.inf):
            a = arr.copy()
            a.reshape(-1)[a.size // 2] = bad
            refused(eng, INV, "not finite", 0, new, **{k: a})
    for entry, value in ((0, 0.0), (4, 0.0), (4, -1.0), (8, -1.0)):
        a = good["state"].copy()
        a[5, entry] = value
        refused(eng, INV, "strictly positive", 0, new, state=a)
    bad = new.copy()
    bad[2, 1] = np.nan
    refused(eng, INV, "not finite", 0, bad)
    refused(eng, INV, "v0 is not finite", 0, new, v0=(0.0, np.inf, 0.0))
    n = 1 << BITS
    for cell in (-2.6, n + 1.6):                                 # what set-up counts as outside: a block key below 0 or beyond the last block
        out = new.copy()
        out[4, 2] = np.float32(cell) * DX
        refused(eng, INV, "outside the domain", 0, out)
    # between mpm_grid_update and mpm_rebuild_partition the grid holds velocities
    eng.grid_update(1e-5)
    refused(eng, INV, "holds velocities", 0, new)
    eng.g2p2g(1e-5, 1e-5)
    refused(eng, INV, "holds velocities", 0, new)
    eng.rebuild_partition()
    # ids that are not valid: a tracked context between load_checkpoint and load_particle_ids
    ck, ids = eng.save_checkpoint().copy(), eng.save_particle_ids().copy()
    eng.load_checkpoint(ck)
    with pytest.raises(EngineError) as e:
        eng.emit(0, new)
    assert e.value.code == INV and "ids" in str(e.value) and np.array_equal(eng.save_checkpoint(), ck)
    eng.load_particle_ids(ids)
    emit_checked(eng, 0, new / DX, tag="after the refusals the same call is accepted")
    # a context that has been through the halo tagging
    assert eng.api.halo_tag_begin(eng.ctx) == 0 and eng.api.halo_tag_end(eng.ctx, C.byref(C.c_int(0)), (C.c_int * 32)()) == 0
    refused(eng, INV, "group", 0, new)
    eng.close()


# ---- after particles were lost ---------------------------------------------------------------------------------------------------------------------
def test_emission_after_particles_were_lost_keeps_the_books():
    """The injection bench of the torn tests with a block against the upper x face and a grid that moves everything 3.9 cells outward in one
    substep (less than a block, so every destination is a neighbour; the nodes beyond the face do not exist and give the outermost particles
    nothing, the ones a cell or two further in get most of it): those leave the domain and are counted as lost; an emission then re-lays fewer
    particles than the model was given, and every host synchronisation of the run that follows balances the books (no MPM_ERR_INTERNAL)"""
    pos = np.concatenate([gm.scene_cluster(), gm.block_particles((15, 6, 6), 60, np.random.default_rng(15))])
    st = gm.make_state(gm.FC, pos.shape[0], 40)
    out_x = np.float32(3.9 * float(DX) / gm.DT)
    bench = gb.Bench([(gm.FC, pos)])
    try:
        bench.inject([st], lambda keys: np.tile(np.float32([out_x, 0, 0])[None, :, None], (keys.shape[0], 1, 64)))
        bench.eng.g2p2g(gm.DT, gm.NEW_DT)
        bench.eng.rebuild_partition()
        eng = bench.eng
        lost = int(eng.diagnostics().lost_particles)
        held = int(eng.counts().particles[0])
        print("lost before the emission:", lost, "held:", held)
        assert lost > 0 and held + lost + int(eng.diagnostics().dropped_particles) == pos.shape[0]
        new = gm.block_particles((9, 3, 3), 50, np.random.default_rng(12)) * DX
        assert eng.emit(0, new) == pos.shape[0]
        assert int(eng.counts().particles[0]) == held + 50 and int(eng.diagnostics().lost_particles) == lost
        eng.run_fixed(16, 1e-5)
        d = eng.diagnostics()
        assert int(eng.counts().particles[0]) + int(d.lost_particles) + int(d.dropped_particles) == pos.shape[0] + 50
    finally:
        bench.close()


# ---- the re-laid state is one the substep kernels accept ---------------------------------------------------------------------------------------------
def test_one_substep_from_the_relaid_state_against_the_model_and_the_books():
    """emit into the bench's context; one G2P2G + rebuild with the books verifier (rebuild_books.check_books, as test_rebuild_books_gpu calls it); then
    one substep from the state READ BACK after the emission, with an injected velocity field, against g2p2g_model - every particle and every node,
    under test_g2p2g_blocks_gpu's bounds"""
    from test_g2p2g_blocks_gpu import check
    from test_rebuild_books_gpu import books
    material = gm.FC
    pos, st = gm.scene_state("cluster", material)
    extra = gm.EXTRA_SCENES["cluster_b"]()
    se = gm.make_state(material, extra.shape[0], 33)
    bench = gb.Bench([(material, pos)])
    try:
        bench.inject([st], lambda keys: gm.grid_of(keys, "rest"))
        bench.eng.g2p2g(gm.DT, gm.NEW_DT)
        bench.eng.rebuild_partition()                              # the lists now carry neighbour tags: the gather follows them
        p0 = bench.read(0)
        bench.eng.emit(0, extra * DX, state=state9_of(material, se))
        merged = np.concatenate([p0["pos"], extra])
        bench.parts = [(material, merged)]
        back = bench.read(0)
        ck = bench.eng.save_checkpoint().copy()
        for seed in range(1, 65):                                 # (the field is re-drawn until no particle sits on the brink of a branch, as test_second_substep does)
            m2 = gm.step(bench.consts[0], back["pos"], gm.gather_field(back["pos"], "flow", seed), b6=back["b6"], reflected=back["reflected"], logjp=None, J=None)
            if not m2["unstable"].any():
                break
        bench.load(ck, lambda keys: gm.grid_of(keys, "flow", seed=seed))
        res = bench.step()
        bench.parts = [(material, back["pos"])]
        check(bench, res, [m2], "flow", "one substep after an emission")
        _, _, found = books(bench.eng, 1)
        assert not found, found[:10]
    finally:
        bench.close()


def test_still_path_is_not_offered_to_the_first_rebuild_after_an_emission():
    """nothing moves (no gravity, stress-free, at rest): of a 64-substep window's rebuilds all but the first take the still path - after set-up, and
    again after an emission"""
    eng = set_up(scene_of([model_dict(gm.FC, gm.scene_cluster())], config={"gravity": 0.0, "sync_interval": 64}))
    s0 = int(eng.diagnostics().still_rebuilds)
    eng.run_fixed(64, 1e-5)
    s1 = int(eng.diagnostics().still_rebuilds)
    eng.emit(0, gm.block_particles((9, 9, 9), 30, np.random.default_rng(13)) * DX)
    eng.run_fixed(64, 1e-5)
    s2 = int(eng.diagnostics().still_rebuilds)
    eng.run_fixed(64, 1e-5)
    s3 = int(eng.diagnostics().still_rebuilds)
    eng.close()
    assert (s1 - s0, s2 - s1, s3 - s2) == (63, 63, 64)


# ---- trajectory ------------------------------------------------------------------------------------------------------------------------------------
def test_an_emitted_blob_flies_as_the_oracle_flies_it_from_set_up():
    from parity_util import match, run_engine
    from oracle_ffi import oracle_api
    bits, k, dt = 6, 20, 1e-4
    prm = {"volume": scenes._vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    blob = scenes.lattice_sphere(bits, (0.3, 0.6, 0.5), 4.0)
    body = scenes.lattice_box(bits, (40, 20, 28), (46, 26, 34))
    v0 = (1.0, 0.5, -0.25)
    sc = {"name": "emit_flight", "bits": bits, "dt": dt, "config": {"max_ppc": 16, "gravity": 0.0},
          "models": [{"material": _ffi.FIXED_COROTATED, "xyz": body, "v0": (0, 0, 0), "params": dict(prm)},
                     {"material": _ffi.FIXED_COROTATED, "xyz": np.zeros((0, 3), np.float32), "v0": (0, 0, 0), "params": dict(prm)}]}
    eng = set_up(sc)
    eng.run_fixed(5, dt)
    eng.emit(1, blob, v0=v0)
    eng.run_fixed(k, dt)
    xh = eng.retrieve_positions(1)
    eng.close()
    alone = dict(sc, models=[dict(sc["models"][1], xyz=blob, v0=v0)])
    xo = run_engine(alone, k, dt, api=oracle_api())["state"][0][0]
    idx, _ = match(xo.astype(np.float64), xh.astype(np.float64))
    rel = (np.abs(xh[idx].astype(np.float64) - xo) .max(axis=1) / np.abs(xo).max(axis=1)).max()
    print(f"emitted blob after {k} substeps: positions within {rel:.3g} (relative) of the oracle's run from set-up")
    assert xh.shape == xo.shape and rel < 1e-5                 # parity_util's position bound (smoke(): pos_rel < 1e-5)


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_saved_after_an_emission_loads_into_a_context_sized_by_the_grown_n():
    """the recipe of include/claymore_amd.h: add the models with as many particles as the checkpoint carries (any positions: they only size the
    context), set up, load the checkpoint and the ids.  Held as tests/test_checkpoint_gpu.py holds a restart: what was loaded is there bit for
    bit - particles, ids, grid -, and the same window run in both contexts agrees within that file's 2e-6 (two runs of ONE context differ in the
    last bits too: the P2G sums with float atomics, whose order is free).  Measured: after the window the ids agree exactly and 1 of 1 699
    positions differs, by 6e-8 relative."""
    rng = np.random.default_rng(14)
    pos = gm.scene_cluster()
    new = gm.block_particles((8, 7, 6), 120, rng)
    sc = scene_of([model_dict(gm.SAND, pos, v0=(0.2, 0.0, 0.1))], track_ids=True)
    a = set_up(sc)
    a.run_fixed(4, 1e-4)
    a.emit(0, new * DX, v0=(0.0, -1.0, 0.0))
    ck, ids = a.save_checkpoint().copy(), a.save_particle_ids().copy()
    assert cf.parse(ck)["models"][0]["n"] == pos.shape[0] + 120
    sizing = rng.permutation(np.concatenate([pos, new]))          # (positions that only size the context)
    b = set_up(scene_of([model_dict(gm.SAND, sizing)], track_ids=True))
    b.load_checkpoint(ck)
    b.load_particle_ids(ids)
    pa, pb = read_particles(a, 0), read_particles(b, 0)
    ga, gb_ = pem.grid_by_node(*a.dump_grid(), BITS), pem.grid_by_node(*b.dump_grid(), BITS)
    assert pem.same_set(pa, pb) and np.array_equal(pa["ids"], pb["ids"]) and pa["ids"].shape[0] == pos.shape[0] + 120
    assert np.array_equal(ga[0], gb_[0]) and np.array_equal(ga[1].view(np.uint32), gb_[1].view(np.uint32))
    for eng in (a, b):
        eng.run_fixed(16, 1e-4)
    pa, pb = read_particles(a, 0), read_particles(b, 0)                 # (rows in id order: row k is the same particle in both)
    a.close()
    b.close()
    assert np.array_equal(pa["ids"], pb["ids"])
    xa, xb = pa["xyz"].astype(np.float64), pb["xyz"].astype(np.float64)
    rel = (np.abs(xa - xb).max(axis=1) / np.abs(xb).max(axis=1)).max()
    print(f"after 16 substeps in both contexts: positions within {rel:.3g} (relative), {int((pa['xyz'] != pb['xyz']).any(axis=1).sum())} of {xa.shape[0]} rows differ in a bit")
    assert rel < 2e-6


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------------------
def emitter_count(sc, t):
    """how many particles the scene's emitters have handed out by time t, from the model's statement of the layer rule"""
    total = 0
    for e in sc["emitters"]:
        geom = {k: e[k] for k in ("lo", "hi", "center", "radius") if k in e}
        v = np.asarray(e["velocity"], np.float64)
        axis = int(np.argmax(np.abs(v)))
        layers = (pem.layer_times(sc["bits"], float(np.abs(v[axis])), e.get("start", 0.0), e.get("end", np.inf)) <= t).sum()
        total += int(layers) * pem.nozzle_lattice(sc["bits"], e["shape"], axis, **geom).shape[0]
    return total


def test_faucet_through_main_loop():
    sc = scenes.faucet(bits=BITS, radius_cells=2.0, speed=8.0, end=0.0055)
    eng = build_engine(sc)
    seen = []

    def on_frame(frame, e):
        seen.append((e.cur_time, int(e.counts().particles[0]), e.models[0]["n"]))
    eng.main_loop(3, 500, 1e-4, on_frame=on_frame)
    d = eng.diagnostics()
    tot = eng.grid_totals()
    mass = eng.model_mass(0)
    eng.close()
    print("faucet frames (time, particles, n):", seen)
    assert [s[1] for s in seen] == [s[2] for s in seen] == [emitter_count(sc, s[0]) for s in seen]
    assert seen[0][1] > 0 and seen[-1][1] > seen[0][1]
    assert (int(d.lost_particles), int(d.dropped_particles)) == (0, 0)
    # every node is a float32 sum of at most 8 blocks' max_ppc * 64 terms, each weight product a few roundings: (8 max_ppc 64 + R_MASS) u of the mass
    assert abs(tot[0] - seen[-1][1] * mass) <= pim.gamma(8 * 16 * 64 + pim.R_MASS) * seen[-1][1] * mass


def test_gmpm_serves_the_emitters_of_a_scene_file(tmp_path):
    """gmpm on the faucet as a scene file: the frames carry growing point counts - the emitter model's - and with output_ids the ids are ascending
    and stable: the points a frame shares with the one before are its first rows, in the same id order"""
    import __graft_entry__ as g
    from bgeo_reader import read_bgeo
    g.build_host()
    sc = scenes.faucet(bits=BITS, radius_cells=2.0, speed=8.0, end=0.0055)
    e = sc["emitters"][0]
    model = {"file": "box", "constitutive": "jfluid", "rho": 1e3, "volume": float(np.float32((1 / 64) ** 3 / 8)), "offset": [0.5, 0.5, 0.5], "span": [0.0, 0.0, 0.0], "velocity": [0, 0, 0]}
    sim = {"gpuid": 0, "fps": 500, "frames": 3, "default_dt": 1e-4, "domain_bits": BITS, "max_ppc": 16, "output_dir": str(tmp_path), "output_ids": True}
    emitters = [{"model": 0, "shape": "disc", "center": list(e["center"]), "normal": list(e["normal"]), "radius": e["radius"], "velocity": list(e["velocity"]), "start": e["start"], "end": e["end"]}]
    (tmp_path / "scene.json").write_text(json.dumps({"simulation": sim, "models": [model], "emitters": emitters}))
    out = subprocess.check_output([os.path.join(os.path.dirname(HERE), "claymore_amd", "host", "gmpm"), "-f", str(tmp_path / "scene.json")], text=True, timeout=300)
    counts = []
    for f in (1, 2, 3):
        x, attrs, _ = read_bgeo(tmp_path / f"model_id[0]_frame[{f}].bgeo")
        assert np.array_equal(attrs["id"].ravel(), np.arange(x.shape[0])), "ids ascending, the new ones the largest"
        counts.append(x.shape[0])
    print("gmpm frames:", counts, out[-300:])
    assert 0 < counts[0] < counts[1] <= counts[2]
    assert counts[2] == emitter_count(sc, np.inf)                 # the emitter ends at 5.5 ms, the run at 6 ms


# ---- both list layouts -----------------------------------------------------------------------------------------------------------------------------
def test_the_sliced_layout_passes_too():
    """Everything above runs with the list layout this process was given (default: the pair layout for all four materials).  The landing, size,
    material, model and id tests run once more in a fresh child process with MPM_G2P2G_PAIRS=0 - every model in the sliced layout - selected the
    way test_model_slots_gpu selects it; a child that ends on a signal or at its time limit fails the test, and nothing is tried again."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "land or sizes or every_material or two_models or tracked"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

"""The collider-load readout on the GPU (claymore_amd/csrc/mpm_collider_loads.hpp: collider_loads_kernel, collider_loads_reduce_kernel,
collider_contacts_kernel; mpm_collider_loads, mpm_collider_contacts, mpm_load_gauge, mpm_load_gauge_read) against tests/collider_load_model.py,
which tests/test_collider_loads_cpu.py judges on the CPU.  The grids are injected through the checkpoint port of
tests/test_collision_shapes_gpu.py: grid_update_model's 28-particle scene at bits 6 with 222 neighbour blocks in all 27 wall classes, the
generator's finite tier.  Contacts are compared on uint32 bit patterns; totals within 4 n 2^-53 sum |terms| per component, n the row's touched
nodes: the per-node terms are the model's bits (float64 products of float32 values without contraction), so the device's sum and math.fsum
differ by the rounding of at most n - 1 additions, each at most 2^-53 of a partial sum that never exceeds sum |terms|.

The gauge.  A comparison of two RUNS needs a scene on which the engine is deterministic (a dense body differs in the last bits from run to run:
float atomics in P2G), so the run-against-run case uses the sparse 48-particle twin of tests/test_collision_shapes_gpu.py, in contact with its
moving sphere from the first substep - and even there two runs number their blocks differently, so the sums agree to the summation's bound and
not on bits (test_gauge_in_run_fixed_equals_the_phase_level_readouts).  Bit for bit is asserted where it can hold: between the gauge and the
host's running sum of mpm_collider_loads inside ONE run, where both read the same grids under the same numbering - on that scene and on the dense
one, a 2 048-particle block over a slip half-space."""
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import ckpt_format as cf
import collider_load_model as lm
import collision_shape_model as sm
import collision_volume_model as vm
import grid_update_model as gm
import heightfield_model as hm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from test_collision_shapes_gpu import BOUNDARY, DT, DX, G, GRAVITY, MOTION, N, TYPES, sorted_rows, sparse_analytic
from test_collision_volume_gpu import VolumeCtx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    c = VolumeCtx()
    assert c.nbc == 222 and sorted(map(tuple, c.keys.tolist())) == sorted(map(tuple, gm.scene_keys().tolist()))
    yield c
    c.eng.close()


def rows_array(d):
    """Engine.collider_loads' dict as the ABI's (6, 8) float64 rows."""
    return np.array([[d[n]["count"], *d[n]["impulse"], *d[n]["angular_impulse"], d[n]["mass"]] for n in _ffi.LOAD_ROW_NAMES], dtype=np.float64)


def assert_totals(got, want, mag, what=""):
    assert np.array_equal(got[:, 0], want[:, 0]), (what, got[:, 0], want[:, 0])
    bound = 4 * want[:, :1] * U * mag[:, 1:]
    err = np.abs(got[:, 1:] - want[:, 1:])
    print(what, "totals: largest error / bound", float(np.nanmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
    assert (err <= bound).all(), (what, err, bound)


def flat_index(nr, nodes):
    code = lambda a: (a[:, 0].astype(np.int64) * 4 * G + a[:, 1]) * 4 * G + a[:, 2]  # noqa: E731
    all_codes = code(nr["nodes"])
    order = np.argsort(all_codes)
    at = np.searchsorted(all_codes[order], code(nodes))
    return order[at]


def check_readout(ctx, seed, cols, field=None, t=0.0, dt=DT):
    """One injected grid through contacts, totals (twice), a caller pivot, the grid and clock untouched, then the real grid update."""
    eng = ctx.eng
    ctx.install(cols, field=field, t=t)
    pat = gm.generate(ctx.nbc, seed, "finite")[0]
    eng.load_checkpoint(cf.with_grid(ctx.ckpt, pat))
    installed = field is not None or any(c is not None for c in cols)
    keys0, grid0 = eng.dump_grid()
    clock0 = eng.collision_time() if installed else None
    got_nr, got_rec = lm.sort_contacts(*eng.collider_contacts(dt))
    first, second = rows_array(eng.collider_loads(dt)), rows_array(eng.collider_loads(dt))
    # a caller pivot on every row
    c2 = np.array([[0.3 + 0.05 * r, 0.6 - 0.04 * r, 0.45 + 0.03 * r] for r in range(6)], dtype=np.float32)
    moved = rows_array(eng.collider_loads(dt, pivots={r: c2[r] for r in range(6)}))
    keys1, grid1 = eng.dump_grid()
    assert np.array_equal(keys0, keys1) and np.array_equal(gm.bits(grid0), gm.bits(grid1)) and np.array_equal(gm.bits(grid0), pat), "the readout wrote the grid"
    assert (eng.collision_time() if installed else None) == clock0 == (float(np.float32(t)) if installed else None), "the readout moved the clock"
    # the model
    nr = lm.node_rows(ctx.keys, G, BOUNDARY, GRAVITY, dt, pat.view(np.float32), cols, t, DX, field=field)
    want_nr, want_rec = lm.contacts(nr)
    assert np.array_equal(got_nr, want_nr), (len(got_nr), len(want_nr))
    bad = gm.canon(got_rec) != gm.canon(want_rec)
    assert not bad.any(), (int(bad.any(axis=1).sum()), got_nr[bad.any(axis=1)][:4].tolist())
    piv = lm.default_pivots(cols, t, field=field)
    want, mag = lm.totals(nr, piv)
    assert_totals(first, want, mag, "default pivots")
    assert np.array_equal(first.view(np.uint64), second.view(np.uint64)), "two calls on one state differ"
    want2, mag2 = lm.totals(nr, c2.astype(np.float64))
    assert_totals(moved, want2, mag2, "caller pivots")
    # L' = L + (c - c') x J: each of the three sums carries its own summation error
    d = piv - c2.astype(np.float64)
    shift = np.cross(d, first[:, 1:4])
    ad, aj = np.abs(d), mag[:, 1:4]
    abs_cross = np.stack([ad[:, 1] * aj[:, 2] + ad[:, 2] * aj[:, 1], ad[:, 2] * aj[:, 0] + ad[:, 0] * aj[:, 2], ad[:, 0] * aj[:, 1] + ad[:, 1] * aj[:, 0]], axis=1)
    bound = 4 * want[:, :1] * U * (mag[:, 4:7] + mag2[:, 4:7] + abs_cross)
    assert (np.abs(moved[:, 4:7] - (first[:, 4:7] + shift)) <= bound).all(), (moved[:, 4:7] - first[:, 4:7] - shift, bound)
    assert np.array_equal(moved[:, :4], first[:, :4]) and np.array_equal(moved[:, 7], first[:, 7])      # (the impulses know no pivot)
    # the update itself: every node's last record holds the velocity the real kernel writes
    eng.grid_update(dt)
    keys2, out = eng.dump_grid()
    assert np.array_equal(keys2, ctx.keys)
    vel = np.ascontiguousarray(out[:, 1:4].transpose(0, 2, 1).reshape(-1, 3))
    rank = np.where(got_nr[:, 3] == lm.WALLS, 0, got_nr[:, 3] + 1)
    idx = flat_index(nr, got_nr[:, :3])
    order = np.lexsort((rank, idx))
    last = order[np.append(np.diff(idx[order]) != 0, True)] if len(order) else order
    # (on bits, but for the sign of a zero: a collider that turns -0 into +0 - `v - v_obj + v_obj` with v_obj = 0 - has dv == 0 and, by the definition, no record)
    unsigned_zero = lambda a: np.where(a == 0, np.float32(0.0), a)  # noqa: E731
    differ = (gm.canon(unsigned_zero(got_rec[last, 4:7])) != gm.canon(unsigned_zero(vel[idx[last]]))).any(axis=1)
    assert not differ.any(), ("a node's last record is not the velocity the update wrote", int(differ.sum()), got_nr[last][differ][:4].tolist(),
                              got_rec[last][differ][:4].tolist(), vel[idx[last]][differ][:4].tolist())
    lv = nr["live"]
    assert np.array_equal(gm.canon(vel[lv]), gm.canon(nr["v_final"][lv]))
    with pytest.raises(EngineError) as e:                                           # the grid holds velocities now
        eng.collider_loads(dt)
    assert e.value.code == _ffi.MPM_ERR_INVALID and "velocities" in str(e.value)
    return nr, first


# ---- 1. contacts, totals, the update ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("typ", sorted(TYPES))
@pytest.mark.parametrize("name", sm.KIND_CASES)
def test_analytic_shapes(ctx, name, typ, moved):
    c = sm.make(name, moved, type=TYPES[typ], friction=0.3)
    nr, tot = check_readout(ctx, 1, [None, c], t=sm.T_MOVED if moved else 0.0)      # (slot 1: row 2)
    assert nr["used"] == [lm.WALLS, 2] and tot[2, 0] > 200 and tot[1, 0] == 0, tot[:, 0]


def test_heightfield(ctx):
    h = hm.make("65x65", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    nr, tot = check_readout(ctx, 2, [h])
    assert tot[1, 0] > 200


def test_volume(ctx):
    v = vm.make("ico", type=0, trans=(0.03, -0.02, 0.01), trans_vel=(0.0, -0.25, 0.5), omega=(0.0, 0.5, 0.0))
    nr, tot = check_readout(ctx, 3, [None, None, v, vm.sphere_volume(shape="box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))])
    assert tot[3, 0] > 50 and tot[4, 0] > 200, tot[:, 0]


def test_level_set_object_with_two_slots(ctx):
    f = sm.make("box", type=1, friction=0.3, trans_vel=(0.0, 0.5, 0.0))
    sdf, grad = sm.sample_field(f, N, DX)
    a = sm.make("halfspace_tilted", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    b = sm.make("sphere", type=2, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    nr, tot = check_readout(ctx, 4, [a, None, None, b], field=(f, sdf, grad))
    assert nr["used"] == [lm.WALLS, 0, 1, 4] and (tot[[0, 1, 4, 5], 0] > 200).all() and (nr["touched"][0] & nr["touched"][4]).sum() > 20
    # the level-set object alone: grid_update_collider_kernel<CollisionArgs>'s twin
    nr, tot = check_readout(ctx, 5, [], field=(f, sdf, grad))
    assert nr["used"] == [lm.WALLS, 0] and tot[0, 0] > 200


def test_walls_alone_in_all_27_classes(ctx):
    nr, tot = check_readout(ctx, 6, [])
    assert nr["used"] == [lm.WALLS] and (tot[:5] == 0).all()
    wc = np.repeat(gm.wall_class(ctx.keys, G, BOUNDARY), 64, axis=0)
    seen = {tuple(r) for r in wc[nr["touched"][lm.WALLS]].tolist()}
    assert len(seen) == 26 and (1, 1, 1) not in seen                                 # every class with a wall; the interior has no row


def test_slot_order_changes_the_rows(ctx):
    a = sm.make("halfspace_tilted", type=1, friction=0.3, trans_vel=(0.5, 0.0, 0.0))
    b = sm.make("sphere", type=2, friction=0.2, trans_vel=(0.0, 0.0, -0.75))
    _, ab = check_readout(ctx, 4, [a, b])
    _, ba = check_readout(ctx, 4, [b, a])
    assert not np.array_equal(ab[1, 1:4], ba[2, 1:4]) and not np.array_equal(ab[2, 1:4], ba[1, 1:4]) and np.array_equal(ab[5], ba[5])


# ---- 2. the protocol and the refusals -------------------------------------------------------------------------------------------------------------
def test_count_then_fetch_and_refusals(ctx):
    eng, api = ctx.eng, ctx.eng.api
    c = sm.make("sphere", type=1, friction=0.3)
    ctx.install([c])
    eng.load_checkpoint(cf.with_grid(ctx.ckpt, gm.generate(ctx.nbc, 7, "finite")[0]))
    n = C.c_size_t(0)
    assert api.collider_contacts(eng.ctx, DT, None, None, C.byref(n)) == _ffi.MPM_OK and n.value > 1000
    true = n.value
    short = true // 3
    nr, rec = np.full((short + 1, 4), -7, np.int32), np.full((short + 1, 8), -7.0, np.float32)
    n = C.c_size_t(short)
    assert api.collider_contacts(eng.ctx, DT, nr.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p), C.byref(n)) == _ffi.MPM_ERR_CAPACITY and n.value == true
    assert (nr[short] == -7).all() and (rec[short] == -7).all() and (nr[:short, 3] >= 0).all()        # `short` records written, nothing behind them
    want, _ = lm.sort_contacts(*eng.collider_contacts(DT))
    have = {tuple(r) for r in want.tolist()}
    assert all(tuple(r) in have for r in nr[:short].tolist())                       # (some `short` of the true records)
    out = (C.c_double * 8 * 6)()
    for dt in (0.0, -1e-4, float("nan")):
        assert api.collider_loads(eng.ctx, dt, None, out) == _ffi.MPM_ERR_INVALID and b"dt" in api.last_error(eng.ctx)
        assert api.collider_contacts(eng.ctx, dt, None, None, C.byref(n)) == _ffi.MPM_ERR_INVALID
    assert api.collider_loads(eng.ctx, DT, None, None) == _ffi.MPM_ERR_INVALID and api.collider_contacts(eng.ctx, DT, None, None, None) == _ffi.MPM_ERR_INVALID
    assert api.collider_contacts(eng.ctx, DT, nr.ctypes.data_as(C.c_void_p), None, C.byref(n)) == _ffi.MPM_ERR_INVALID
    with pytest.raises(EngineError) as e:
        eng.read_load_gauge()                                                       # the gauge is off
    assert e.value.code == _ffi.MPM_ERR_INVALID
    # velocities in the grid: refused, and a gauge that is on stays as it was
    eng.load_gauge(True)
    eng.grid_update(DT)
    _, _, updates = eng.read_load_gauge(reset=False)
    assert updates == 1
    for call in (lambda: eng.collider_loads(DT), lambda: eng.collider_contacts(DT)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.code == _ffi.MPM_ERR_INVALID
    rows, elapsed, updates = eng.read_load_gauge(reset=True)
    assert updates == 1 and elapsed == float(np.float32(DT)) and rows["slot0"]["count"] > 500
    assert eng.read_load_gauge()[2] == 0
    eng.load_gauge(False)
    with pytest.raises(EngineError):
        eng.read_load_gauge()
    # before set-up
    fresh = build_engine(sparse_analytic(boundary="slip", **MOTION))
    for call in (lambda: fresh.collider_loads(DT), lambda: fresh.collider_contacts(DT), lambda: fresh.load_gauge(True), lambda: fresh.read_load_gauge()):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.code == _ffi.MPM_ERR_NOT_READY
    fresh.close()


def test_a_grouped_context_is_refused():
    sc = sparse_analytic(boundary="slip", **MOTION)
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
        eng = ranks[0].eng
        for call in (lambda: eng.collider_loads(DT), lambda: eng.collider_contacts(DT), lambda: eng.load_gauge(True)):
            with pytest.raises(EngineError) as e:
                call()
            assert e.value.code == _ffi.MPM_ERR_INVALID and "group" in str(e.value)
        with pytest.raises(EngineError):
            eng.read_load_gauge()                                                   # (still off)
    finally:
        for r in ranks:
            r.close()


# ---- 3. the gauge -----------------------------------------------------------------------------------------------------------------------------------
STEPS = 16


def f64_sum(dts):
    t = 0.0
    for d in dts:
        t += float(np.float32(d))
    return t


def test_gauge_in_run_fixed_equals_the_phase_level_readouts():
    """16 substeps of mpm_run_fixed with the gauge on against the phase-level loop that calls mpm_collider_loads before each mpm_grid_update (the
    sparse deterministic scene, a moving, turning, growing slip sphere, the clock running).  Inside the phase-level run the gauge's accumulators
    ARE the host's running float64 sum of the per-call totals, added in the same order, bit for bit.  Between the two runs only the node values
    are the same: a rebuild numbers its blocks in the order its atomics land (mpm_kernels.hpp), the fixed order of the sums is an order of block
    numbers, and `the same state gives the same bits` cannot reach across two numberings (on an MI355X the comparison of the two runs on bits
    failed while every comparison inside one run held).  Across the runs the bound is therefore the summation's: per substep 4 n 2^-53 sum |terms|, n the touched nodes, plus one rounding
    of the running sum per substep, with |r x j| <= |j_a| + |j_b| per component (arm and pivot inside the unit domain).  The touched-node count,
    16 updates, the float64 sum of the dts and the particles' end positions (gauge on, off, phase loop) are
    equalities."""
    sc = sparse_analytic(boundary="slip", **MOTION)
    dt = sc["dt"]
    gauged = build_engine(sc)
    gauged.initial_setup()
    gauged.load_gauge(True)
    gauged.run_fixed(STEPS, dt)
    rows, elapsed, updates = gauged.read_load_gauge(reset=False)
    x_gauged, clock = sorted_rows(gauged.retrieve_positions(0)), gauged.collision_time()
    gauged.close()

    phase = build_engine(sc)
    phase.initial_setup()
    phase.load_gauge(True)                                                          # (mpm_grid_update feeds it too)
    acc, bound = np.zeros((6, 8)), np.zeros((6, 8))
    for _ in range(STEPS):
        tot = rows_array(phase.collider_loads(dt))
        _, crow, cm, cdv, _ = phase.collider_contacts(dt)
        for r in range(6):
            sel = crow == r
            mj = (cm[sel, None].astype(np.float64) * np.abs(cdv[sel].astype(np.float64))).sum(axis=0)
            mag = np.array([0.0, *mj, mj[1] + mj[2], mj[2] + mj[0], mj[0] + mj[1], cm[sel].astype(np.float64).sum()])
            assert sel.sum() == tot[r, 0]
            bound[r] += (4 * sel.sum() + 1) * U * mag * 1.001
        acc = acc + tot
        phase.grid_update(dt)
        phase.g2p2g(dt, dt)
        phase.rebuild_partition()
    rows_p, elapsed_p, updates_p = phase.read_load_gauge()
    x_phase = sorted_rows(phase.retrieve_positions(0))
    phase.close()

    plain = build_engine(sc)
    plain.initial_setup()
    plain.run_fixed(STEPS, dt)
    x_plain = sorted_rows(plain.retrieve_positions(0))
    assert plain.collision_time() == clock
    plain.close()

    assert updates == updates_p == STEPS and elapsed == elapsed_p == f64_sum([dt] * STEPS)
    assert acc[1, 0] > 0 and np.abs(acc[1, 1:4]).max() > 0, acc[1]               # (the sphere did load the material)
    got_p, got = rows_array(rows_p), rows_array(rows)
    assert np.array_equal(got_p.view(np.uint64), acc.view(np.uint64)), ("phase loop", got_p - acc)
    print("run_fixed against the phase loop: |difference|", np.abs(got - acc).max(axis=0), "bound", bound.max(axis=0))
    assert np.array_equal(got[:, 0], acc[:, 0]) and (np.abs(got - acc) <= bound).all(), (got - acc, bound)
    with np.errstate(all="ignore"):
        assert np.array_equal(rows["slot0"]["force"], got[1, 1:4] / elapsed) and np.array_equal(rows["slot0"]["torque"], got[1, 4:7] / elapsed)
    assert np.array_equal(x_gauged, x_plain) and np.array_equal(x_gauged, x_phase)


def block_over_half_space():
    """An 8 x 4 x 8-cell block (2 048 particles) falling at 1 m/s onto a slip half-space whose surface lies half a cell above its lowest nodes, bits 6."""
    bits, n = 6, 64
    lo, hi = [n // 2 - 4, n // 2, n // 2 - 4], [n // 2 + 4, n // 2 + 4, n // 2 + 4]
    dx = 1.0 / n
    return {"name": "block_over_half_space", "bits": bits, "dt": 1e-4, "config": {},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": scenes.lattice_box(bits, lo, hi), "v0": (0.25, -1.0, 0.0),
                        "params": {"volume": scenes._vol(bits), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}],
            "colliders": [{"kind": "halfspace", "a": (0.5, (lo[1] + 0.5) * dx, 0.5), "b": (0.0, 1.0, 0.0), "type": 1, "friction": 0.3}]}


def test_gauge_on_a_dense_block_every_driver_feeds_it():
    """The 2 048-particle block over a slip half-space: inside one run the gauge and the host's running sum of mpm_collider_loads read the same
    grids, so they agree bit for bit although the scene is dense; mpm_run_fixed and mpm_substep then add their updates to the same accumulators.
    The half-space carries the block: its vertical load is upwards on the material, downwards (negative y) on the collider."""
    sc = block_over_half_space()
    assert len(sc["models"][0]["xyz"]) == 2048
    dt = sc["dt"]
    eng = build_engine(sc)
    eng.initial_setup()
    eng.load_gauge(True)
    acc = np.zeros((6, 8))
    for _ in range(8):
        acc = acc + rows_array(eng.collider_loads(dt))
        eng.grid_update(dt)
        eng.g2p2g(dt, dt)
        eng.rebuild_partition()
    rows, elapsed, updates = eng.read_load_gauge(reset=False)
    got = rows_array(rows)
    assert updates == 8 and elapsed == f64_sum([dt] * 8) and np.array_equal(got.view(np.uint64), acc.view(np.uint64)), got - acc
    assert acc[1, 0] > 8 * 50 and acc[1, 2] < 0 and rows["slot0"]["force"][1] < 0, acc[1]
    eng.run_fixed(8, dt)
    assert eng.read_load_gauge(reset=False)[2] == 16
    next_dt, _ = eng.substep(dt, 0.0, 1.0, dt)
    rows, elapsed, updates = eng.read_load_gauge(reset=True)
    assert updates == 17 and elapsed == f64_sum([dt] * 17) and rows["slot0"]["count"] > got[1, 0]
    assert eng.read_load_gauge()[1:] == (0.0, 0)
    eng.load_checkpoint(eng.save_checkpoint())                                      # (no part of a checkpoint: a load starts it over)
    eng.grid_update(dt)
    ck = eng.save_checkpoint()
    assert eng.read_load_gauge(reset=False)[2] == 1
    eng.load_checkpoint(ck)
    assert eng.read_load_gauge(reset=False)[2] == 0
    eng.close()


# ---- 4. the gmpm driver -----------------------------------------------------------------------------------------------------------------------------
def test_gmpm_output_loads_equals_the_engines_gauge(tmp_path):
    """tests/test_collision_shapes_gpu.py's "colliders" scene (two single-block bodies, a sticky box and a moving slip sphere: deterministic) through
    the gmpm driver with simulation.output_loads: every loads_frame[f].json holds the numbers Engine.read_load_gauge returns for that frame."""
    import __graft_entry__ as g
    from test_gmpm_stress_gpu import BITS, DT_DEFAULT, FC, FPS, FRAMES, MODELS, frame
    from test_particle_stress_cpu import read_bgeo_attrs
    g.build_host()
    cols = [{"shape": "box", "center": [8 / 64, 19.5 / 64, 19.5 / 64], "half_extents": [0.75 / 64, 3 / 64, 3 / 64], "type": "sticky"},
            {"shape": "sphere", "center": [10.5 / 64, 31.5 / 64, 31.5 / 64], "radius": 1.5 / 64, "type": "slip", "friction": 0.2, "velocity": [-2.0, 0.0, 0.0]}]
    d = tmp_path / "loads"
    d.mkdir()
    sim = {"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d), "output_loads": True}
    (d / "scene.json").write_text(json.dumps({"simulation": sim, "models": MODELS, "colliders": cols}))
    subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(d / "scene.json")], text=True, timeout=300)
    start = [read_bgeo_attrs(frame(d, m, 0))[0] for m in range(len(MODELS))]
    eng = Engine(domain_bits=BITS, max_ppc=128)
    for mod, xyz in zip(MODELS, start):
        mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
        eng.init_model(mat, xyz, mod["velocity"], **({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {}))
    eng.set_collision_shape(0, "box", a=cols[0]["center"], b=cols[0]["half_extents"], type=0, trans=cols[0]["center"])
    eng.set_collision_shape(1, "sphere", a=cols[1]["center"], radius=cols[1]["radius"], type=1, friction=0.2, trans=cols[1]["center"], trans_vel=cols[1]["velocity"])
    eng.set_collision_clock(True, 0.0)
    spf = np.float32(1.0) / np.float32(FPS)
    max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in MODELS)
    dt = eng.compute_dt(max_v0, 0.0, float(spf), DT_DEFAULT)
    eng.initial_setup()
    eng.load_gauge(True)
    loaded = 0
    for f in range(1, FRAMES + 1):
        t = np.float32(0.0)
        while t < spf:
            next_dt, _ = eng.substep(dt, float(t), float(spf), DT_DEFAULT)
            t = np.float32(t + np.float32(dt))
            dt = next_dt
        rows, elapsed, updates = eng.read_load_gauge(reset=True)
        doc = json.loads((d / f"loads_frame[{f}].json").read_text())
        assert doc["frame"] == f and doc["updates"] == updates > 0 and doc["elapsed"] == elapsed
        for name in _ffi.LOAD_ROW_NAMES:
            r, w = doc["rows"][name], rows[name]
            assert r["count"] == w["count"] and r["mass"] == w["mass"], (f, name)
            for key in ("impulse", "angular_impulse", "force", "torque"):
                assert np.array_equal(np.array(r[key]), w[key]), (f, name, key, r[key], w[key])
        loaded += rows["slot0"]["count"] + rows["slot1"]["count"]
    assert loaded > 0                                                               # (a collider was touched)
    eng.close()

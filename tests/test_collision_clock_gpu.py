"""Moving collision object on the GPU: the HIP engine with its clock running against the oracle driven step by step, the fused loop
against the phase-level one, the clock's book-keeping, restart, and a two-rank group against one context."""
import ctypes as C
import threading

import numpy as np
import pytest

from claymore_amd import _ffi, scenes
from claymore_amd.engine import EngineError, build_engine
from claymore_amd.mgsp import LocalGroup, MgspGroupRank
from parity_util import match
from test_collision_clock_cpu import SCENE, STEPS, drive_oracle

pytestmark = pytest.mark.gpu

# (b): translation + rotation + growth from a tilted start orientation: Rz(0.3) Rx(0.2) in the reference's [3 i + j] storage; the angles reach
# 1.6 / 0.8 / 2.4 rad and the sphere grows by 32 % over the 400 substeps
_cz, _sz, _cx, _sx = np.cos(0.3), np.sin(0.3), np.cos(0.2), np.sin(0.2)
TILT = (np.array([[_cz, -_sz, 0], [_sz, _cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, _cx, -_sx], [0, _sx, _cx]])).astype(np.float32).ravel()
MOTIONS = {"translation": {}, "full": {"omega": (10.0, -5.0, 15.0), "dsdt": 2.0, "rot_mat": TILT}}


def rel_dev(x, ref):
    idx, _ = match(ref.astype(np.float64), x.astype(np.float64))
    return (np.abs(x[idx].astype(np.float64) - ref) .max(axis=1) / np.abs(ref).max(axis=1)).max(), idx


def phase_run(sc, steps, hook=None):
    """The phase-level loop on the HIP engine; the scene's `animate` starts the clock.  Returns positions, max-velocity series, totals, time."""
    eng = build_engine(sc)
    eng.initial_setup()
    mv = []
    for k in range(steps):
        if hook:
            hook(eng, k)
        mv.append(eng.grid_update(sc["dt"]))
        eng.g2p2g(sc["dt"], sc["dt"])
        eng.rebuild_partition()
    out = eng.retrieve_positions(0), np.array(mv), eng.grid_totals(), eng.collision_time()
    eng.close()
    return out


def f32_sum(t0, dts):
    t = np.float32(t0)
    for d in dts:
        t = np.float32(t + np.float32(d))
    return float(t)


@pytest.mark.parametrize("motion", sorted(MOTIONS))
@pytest.mark.parametrize("boundary", ["sticky", "slip", "separate"])
def test_hip_matches_oracle_with_a_moving_object(boundary, motion):
    """Phase-level loop, clock running, against the oracle with time = T_k installed before every grid update: positions within the
    project's standing 1e-5 relative, max-velocity series and grid mass as test_hip_matches_oracle_with_collision_object has them.
    Measured (MI355X): positions slip 1.8e-6 / 1.6e-6 (full / translation), separate 2.6e-6 / 1.6e-6, two HIP runs against each other
    3-8e-7; the oracle against itself in another summation order: 1e-6 (test_collision_clock_cpu.SCENE)."""
    sc = scenes.sphere_through_block(boundary=boundary, **SCENE, **MOTIONS[motion])
    xo, mvo, to, T = drive_oracle(sc, STEPS)
    xh, mvh, th, Th = phase_run(sc, STEPS)
    assert xh.shape == xo.shape
    rel, _ = rel_dev(xh, xo)
    print(boundary, motion, "pos_rel", rel, "max-velocity rel", np.abs(mvh - mvo).max() / np.abs(mvo).max(), "mass rel", abs(th[0] - to[0]) / abs(to[0]))
    assert Th == T == f32_sum(0.0, [sc["dt"]] * STEPS)
    assert rel < 1e-5, rel
    assert np.allclose(mvh, mvo, rtol=2e-4, atol=1e-9)
    assert abs(th[0] - to[0]) <= 1e-6 * abs(to[0])


def sparse_scene(**kw):
    """One particle every fourth cell of a 16 x 12 x 16-cell block (48 particles, each given a velocity), the sphere overlapping the block from
    the start.  The 3 x 3 x 3 stencils of two particles share no node, so every grid node receives one contribution per substep and the float
    atomics of P2G have nothing to reorder (two contributions would still commute): the engine is deterministic on this scene, which is what
    a bit-for-bit comparison of two code paths needs."""
    sc = scenes.sphere_through_block(**{**SCENE, "block_cells": (16, 12, 16), "gap_cells": -3.0}, **kw)
    q = np.rint(sc["models"][0]["xyz"].astype(np.float64) * 64 * 4).astype(np.int64)              # quarter cells: 4 node - 1 or 4 node + 1
    sc["models"][0]["xyz"] = np.ascontiguousarray(sc["models"][0]["xyz"][(q % 16 == 15).all(axis=1)])
    sc["models"][0]["v0"] = (-0.5, 0.25, -0.125)
    assert sc["models"][0]["xyz"].shape == (48, 3)
    return sc


SPARSE_STEPS = 60


@pytest.mark.parametrize("sync_interval", [1, None])
@pytest.mark.parametrize("boundary", ["slip", "separate"])
def test_run_fixed_equals_the_phase_level_loop_bit_for_bit(boundary, sync_interval):
    """mpm_run_fixed(n) - every grid update but the first rides on the carry-over (carry_grid_kernel<true, CollisionArgs>), windowed - against the
    same n substeps phase by phase (grid_update_collider_kernel<CollisionArgs>), moving + turning + growing object: the same statements on the same data,
    positions equal bit for bit after matching.  The data are the same only where the engine is deterministic: on the dense block two
    phase-level runs of one scene already differ from each other in the last bits (float atomics in P2G; measured 3-8e-7), so the comparison runs on sparse_scene, whose two phase-level runs are
    required to be identical first; the dense block is compared below under the bound two runs of one scene have to meet."""
    sc = sparse_scene(boundary=boundary, **MOTIONS["full"])
    if sync_interval is not None:
        sc["config"]["sync_interval"] = sync_interval
    xp, _, _, Tp = phase_run(sc, SPARSE_STEPS)
    xq, _, _, _ = phase_run(sc, SPARSE_STEPS)
    assert np.array_equal(np.sort(xp.view("f4,f4,f4"), axis=0), np.sort(xq.view("f4,f4,f4"), axis=0)), "the scene is not deterministic: nothing to compare"
    free = {**sc, "collision": None}
    xfree, _, _, _ = phase_run_free(free, SPARSE_STEPS)
    rows = lambda x: {tuple(r) for r in x.tolist()}
    moved = len(rows(xp) - rows(xfree))
    assert moved >= 12, moved                                    # (the object did act on a quarter of the particles at least)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(SPARSE_STEPS, sc["dt"])
    xf, Tf = eng.retrieve_positions(0), eng.collision_time()
    eng.close()
    rel, idx = rel_dev(xf, xp)
    print(boundary, "sync_interval", sync_interval, "fused vs phase-level pos_rel", rel, "| particles the object moved:", moved)
    assert Tf == Tp == f32_sum(0.0, [sc["dt"]] * SPARSE_STEPS)
    assert np.array_equal(xf[idx].view(np.uint32), xp.view(np.uint32)), rel


def phase_run_free(sc, steps):
    eng = build_engine(sc)
    eng.initial_setup()
    for _ in range(steps):
        eng.grid_update(sc["dt"])
        eng.g2p2g(sc["dt"], sc["dt"])
        eng.rebuild_partition()
    out = eng.retrieve_positions(0), None, None, None
    eng.close()
    return out


@pytest.mark.parametrize("sync_interval", [1, None])
def test_run_fixed_follows_the_phase_level_loop_on_the_dense_block(sync_interval):
    """The dense block, fused against phase-level, under the project's standing 1e-5 relative; the phase-level loop against itself is printed
    beside it (measured 3-8e-7)."""
    sc = scenes.sphere_through_block(boundary="slip", **SCENE, **MOTIONS["full"])
    if sync_interval is not None:
        sc["config"]["sync_interval"] = sync_interval
    xp, _, _, Tp = phase_run(sc, STEPS)
    xq, _, _, _ = phase_run(sc, STEPS)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(STEPS, sc["dt"])
    xf, Tf = eng.retrieve_positions(0), eng.collision_time()
    d = eng.diagnostics()
    eng.close()
    rel, _ = rel_dev(xf, xp)
    rel_self, _ = rel_dev(xq, xp)
    print("sync_interval", sync_interval, "fused vs phase-level pos_rel", rel, "| phase-level against itself", rel_self)
    assert Tf == Tp and d.lost_particles == 0 and d.discarded_p2g == 0
    assert rel < 1e-5, (rel, rel_self)


def test_clock_book_keeping():
    """collision_time() after n fixed and n adaptive substeps is the float32 accumulation of the dts used; a stopped clock reproduces the
    static run; no clock without an object; removing (or re-installing) the object stops the clock."""
    sc = scenes.sphere_through_block(boundary="sticky", **SCENE)
    col = {k: v for k, v in sc["collision"].items() if k != "animate"}
    eng = build_engine(sc)
    eng.initial_setup()
    assert eng.collision_time() == 0.0 and eng.collision_clock_running()
    eng.run_fixed(37, sc["dt"])
    assert eng.collision_time() == f32_sum(0.0, [sc["dt"]] * 37)
    eng.set_collision_clock(True, 0.25)
    dts, dt, t = [], 1e-4, 0.0
    for _ in range(25):                                          # adaptive: the dt each substep actually used
        nd, _ = eng.substep(dt, t, 1.0 / 24, 2e-3)
        dts.append(dt)
        t += dt
        dt = nd
    assert len(set(dts)) > 1                                     # (the dt did adapt)
    assert eng.collision_time() == f32_sum(0.25, dts)
    eng.set_collision_clock(False, 0.5)
    eng.run_fixed(5, sc["dt"])
    eng.grid_update(sc["dt"])
    assert eng.collision_time() == 0.5 and not eng.collision_clock_running()
    eng.set_collision_clock(True, 0.5)
    eng.set_collision_object(**col)                              # installing an object: its own time, stopped
    assert eng.collision_time() == 0.0 and not eng.collision_clock_running()
    eng.set_collision_clock(True, 0.0)
    eng.set_collision_object(None)
    with pytest.raises(EngineError) as e:
        eng.set_collision_clock(True, 0.0)
    assert e.value.code == _ffi.MPM_ERR_INVALID
    with pytest.raises(EngineError):
        eng.collision_time()
    eng.close()


def test_stopped_clock_is_the_static_object():
    """A clock stopped at T reproduces the run of an object installed with time = T bit for bit (on sparse_scene, where the engine is
    deterministic), and differs from the run with the clock started at T."""
    T, runs = 0.01, {}
    for how in ("stopped", "installed", "running"):
        sc = sparse_scene(boundary="slip", **MOTIONS["full"])
        sc["collision"]["animate"] = False
        if how == "installed":
            sc["collision"]["time"] = T
        eng = build_engine(sc)
        if how != "installed":
            eng.set_collision_clock(how == "running", T)
        eng.initial_setup()
        eng.run_fixed(SPARSE_STEPS, sc["dt"])
        assert eng.collision_time() == (float(np.float32(T)) if how != "running" else f32_sum(T, [sc["dt"]] * SPARSE_STEPS))
        runs[how] = np.sort(eng.retrieve_positions(0).view("f4,f4,f4"), axis=0)
        eng.close()
    assert np.array_equal(runs["stopped"], runs["installed"])
    assert not np.array_equal(runs["stopped"], runs["running"])


def test_restart_with_a_moving_object():
    """Checkpoint + collision_time() mid-run, a fresh context, object and clock installed again, continue: against the uninterrupted run and
    against the oracle's, under test_restart_follows_the_uninterrupted_run's bounds (2e-6 between two HIP runs, 1e-5 to the oracle).  On
    sparse_scene, where the engine is deterministic: the restarted run then has to equal the uninterrupted one bit for bit."""
    sc, STEPS = sparse_scene(boundary="separate", **MOTIONS["full"]), SPARSE_STEPS
    half = STEPS // 2
    ref = build_engine(sc)
    ref.initial_setup()
    ref.run_fixed(half, sc["dt"])
    ckpt, t_save = ref.save_checkpoint().copy(), ref.collision_time()
    ref.run_fixed(STEPS - half, sc["dt"])
    want, t_end = ref.retrieve_positions(0), ref.collision_time()
    ref.close()
    xo, _, _, T = drive_oracle(sc, STEPS)
    assert t_save == f32_sum(0.0, [sc["dt"]] * half) and t_end == T
    eng = build_engine({**sc, "collision": {**sc["collision"], "animate": False}})
    eng.initial_setup()
    eng.load_checkpoint(ckpt)
    assert eng.collision_time() == 0.0 and not eng.collision_clock_running()      # neither object nor clock travels in a checkpoint
    eng.set_collision_clock(True, t_save)
    eng.run_fixed(STEPS - half, sc["dt"])
    got = eng.retrieve_positions(0)
    assert eng.collision_time() == t_end
    eng.close()
    a, _ = rel_dev(got, want)
    b, _ = rel_dev(got, xo)
    c, _ = rel_dev(want, xo)
    print("restart vs uninterrupted", a, "| restart vs oracle", b, "| uninterrupted vs oracle", c)
    assert c < 1e-5 and a < 2e-6 and b < 1e-5, (a, b, c)


def test_group_of_two_equals_one_context_with_a_moving_object():
    """Two ranks (mpm_group_run_fixed, in-process transport, the same moving object and clock on both) against one context holding the
    whole block: 1e-6 relative as in test_cpp_group_equals_single_engine; both against the oracle under 1e-5.  On sparse_scene, where
    a single context is deterministic, so that what the partition changes is all there is to see (measured: 6e-8)."""
    sc, STEPS = sparse_scene(boundary="slip", **MOTIONS["full"]), SPARSE_STEPS
    one = build_engine(sc)
    one.initial_setup()
    one.run_fixed(STEPS, sc["dt"])
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
            ranks[r].run_fixed(STEPS, sc["dt"])
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
    xo, _, _, T = drive_oracle(sc, STEPS)
    assert T == t1
    g1, _ = rel_dev(xg, x1)
    go, _ = rel_dev(xg, xo)
    so, _ = rel_dev(x1, xo)
    print("group vs single", g1, "| group vs oracle", go, "| single vs oracle", so)
    assert go < 1e-5 and so < 1e-5, (go, so)
    assert g1 < 1e-6, g1

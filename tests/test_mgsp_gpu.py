"""The HIP halo path (mark / split / collect / reduce kernels, halo-first G2P2G, two-stream ordering) on ONE GPU:
N engine contexts share the device, one Python thread per "rank", and a thread-barrier communicator stands in for
RCCL (a single GPU cannot host several RCCL ranks).  Everything else is the product code path of claymore_amd.mgsp.
The N-rank result must match the single-rank CPU oracle."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

from claymore_amd import _ffi, scenes
from claymore_amd.mgsp import LocalGroup, MgspGroupRank, MgspRank
from parity_util import match, run_engine, to_b
from oracle_ffi import oracle_api

pytestmark = pytest.mark.gpu


class ThreadComm:
    """all_reduce(max) / all_gather / all_to_all_v between threads of one process (device-to-device copies)."""

    def __init__(self, world):
        self.world = world
        self.bar = threading.Barrier(world)
        self.slots = [None] * world

    def view(self, rank):
        return _RankComm(self, rank)


class _RankComm:
    def __init__(self, g, rank):
        self.g, self.rank = g, rank

    def _publish(self, obj):
        torch.cuda.synchronize()
        self.g.slots[self.rank] = obj
        self.g.bar.wait()

    def _done(self):
        torch.cuda.synchronize()
        self.g.bar.wait()

    def all_reduce_max(self, t):
        self._publish(t.clone())
        m = torch.stack([x.to(t.device) for x in self.g.slots]).max(dim=0).values
        self._done()
        t.copy_(m)

    def all_gather(self, out, inp):
        self._publish(inp)
        n = inp.shape[0]
        for p, x in enumerate(self.g.slots):
            out[p * n:(p + 1) * n].copy_(x)
        self._done()

    def all_to_all(self, recv, send, splits):
        offs = np.concatenate([[0], np.cumsum(splits)]).astype(int)
        self._publish((send, offs))
        for p, (psend, poffs) in enumerate(self.g.slots):
            # what p sends to me sits in p's segment [rank]; symmetric counts: it has my splits[p] elements
            seg = psend[poffs[self.rank]:poffs[self.rank + 1]]
            assert seg.numel() == splits[p]
            recv[offs[p]:offs[p + 1]].copy_(seg)
        self._done()


def _run_threads(scene, world, nsteps, dt, phased=False):
    group = ThreadComm(world)
    results, errors = [None] * world, []

    def work(rank):
        try:
            sim = MgspRank(scene, rank, world, device=0, comm=group.view(rank))
            sim.initial_setup()
            shared = 0
            for _ in range(nsteps):
                (sim.substep_phased if phased else sim.substep)(dt, dt)
                shared = max(shared, sum(sim.send_counts))
            results[rank] = (sim.local_state(), shared, sim.n_halo_blocks)
            sim.close()
        except Exception as e:  # noqa: BLE001
            errors.append(e)
            group.bar.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    return results


@pytest.mark.parametrize("world,kind,phased", [(2, "collide", False), (4, "collide", False), (2, "sand", False), (2, "collide", True)])
def test_multi_context_equals_oracle(world, kind, phased):
    if kind == "collide":
        sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
        nsteps = 60
    else:
        sc = scenes.sphere_drop(bits=6, radius_cells=6.0, center=(0.5, 0.3, 0.5), material=_ffi.SAND)
        sc["models"][0]["params"] = {}
        nsteps = 30
    res = _run_threads(sc, world, nsteps, 1e-4, phased)
    assert max(r[1] for r in res) > 0          # halo blocks were exchanged
    assert max(r[2] for r in res) > 0          # and some particle blocks went through the halo-first pass
    ora = run_engine(sc, nsteps, 1e-4, api=oracle_api())
    for m in range(len(sc["models"])):
        xm = np.concatenate([r[0][m][0] for r in res])
        sm = np.concatenate([r[0][m][1] for r in res])
        xo, so, _ = ora["state"][m]
        assert xm.shape == xo.shape
        idx, _ = match(xo.astype(np.float64), xm.astype(np.float64))
        rel = np.abs(xm[idx].astype(np.float64) - xo).max(axis=1) / np.abs(xo).max(axis=1)
        assert rel.max() < 1e-5, rel.max()
        assert np.abs(to_b(sm, True)[idx] - to_b(so, False)).max() < 1e-4


# ---- the C++ group driver (claymore_amd/csrc/mpm_group.inc) -----------------------------------------------------------
def _run_group_threads(scene, world, nsteps, dt, adaptive=None, local_scenes=None, fixed=False):
    """`world` engine contexts on one GPU, one thread per rank, every substep inside mpm_group_substep (in-process
    transport: device-to-device copies; the RCCL transport needs one GPU per rank).  local_scenes: a partition made by
    the caller (one scene per rank) instead of the equal-count slabs of `scene`."""
    lg = LocalGroup(world)
    if local_scenes is not None:
        ranks = [MgspGroupRank(local_scenes[r], r, world, device=0, local_group=lg, prepartitioned=True) for r in range(world)]
    else:
        ranks = [MgspGroupRank(scene, r, world, device=0, local_group=lg) for r in range(world)]
    lg.create()
    results, errors = [None] * world, []

    def work(rank):
        try:
            sim = ranks[rank]
            sim.initial_setup()
            shared = 0
            if adaptive is None and fixed:      # mpm_group_run_fixed: the whole loop inside the library
                sim.run_fixed(nsteps, dt)
                shared, steps = sum(sim.send_counts), nsteps
            elif adaptive is None:
                for _ in range(nsteps):
                    sim.substep(dt, dt)
                    shared = max(shared, sum(sim.send_counts))
                steps = nsteps
            else:
                steps = sim.main_loop(*adaptive)
                shared = sum(sim.send_counts)
            results[rank] = (sim.local_state(), shared, sim.n_halo_blocks, steps)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    for r in ranks:
        r.close()
    assert not errors, errors
    return results


def _compare_with_oracle(sc, res, nsteps, dt, tol=1e-5):
    ora = run_engine(sc, nsteps, dt, api=oracle_api())
    for m in range(len(sc["models"])):
        xm = np.concatenate([r[0][m][0] for r in res])
        sm = np.concatenate([r[0][m][1] for r in res])
        xo, so, _ = ora["state"][m]
        assert xm.shape == xo.shape
        idx, _ = match(xo.astype(np.float64), xm.astype(np.float64))
        rel = np.abs(xm[idx].astype(np.float64) - xo).max(axis=1) / np.abs(xo).max(axis=1)
        assert rel.max() < tol, rel.max()
        assert np.abs(to_b(sm, True)[idx] - to_b(so, False)).max() < 1e-4


@pytest.mark.parametrize("world,kind", [(2, "collide"), (4, "collide"), (3, "sand")])
def test_cpp_group_equals_oracle(world, kind):
    if kind == "collide":
        sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
        nsteps = 60
    else:
        sc = scenes.sphere_drop(bits=6, radius_cells=6.0, center=(0.5, 0.3, 0.5), material=_ffi.SAND)
        sc["models"][0]["params"] = {}
        nsteps = 30
    res = _run_group_threads(sc, world, nsteps, 1e-4)
    assert max(r[1] for r in res) > 0 and max(r[2] for r in res) > 0
    _compare_with_oracle(sc, res, nsteps, 1e-4)


def test_cpp_group_c5_shaped_fluid_dam_8_ranks():
    """BASELINE config 5 in miniature: a weakly compressible J-fluid dam break (box in a corner of the domain, reference
    fluid defaults) at bits 8, cut into 8 equal-count slabs, one engine context per rank, all substeps in the C++ driver."""
    sc = scenes.fluid_dam(bits=8, size_cells=(48, 36, 40), min_corner=(12, 12, 12))
    nsteps = 40
    res = _run_group_threads(sc, 8, nsteps, 1e-4)
    assert sum(r[1] for r in res) > 0 and max(r[2] for r in res) > 0
    _compare_with_oracle(sc, res, nsteps, 1e-4)


def test_cpp_group_weak_scaling_layout_one_column_per_rank():
    """bench.py's weak-scaling workload in miniature: 4 touching sand columns (2 x 2 on the floor), one per rank, each rank
    building only its own column; the union must evolve like the single-engine oracle run of all four columns."""
    size, world = (8, 14, 8), 4
    parts = [scenes.sand_columns_rank(r, world, bits=6, size_cells=size) for r in range(world)]
    whole = dict(parts[0])
    whole["models"] = [dict(parts[0]["models"][0], xyz=np.concatenate([p["models"][0]["xyz"] for p in parts]))]
    nsteps = 30
    res = _run_group_threads(None, world, nsteps, 1e-4, local_scenes=parts, fixed=True)
    assert min(r[1] for r in res) > 0 and min(r[2] for r in res) > 0  # every rank shares faces: halo blocks everywhere
    _compare_with_oracle(whole, res, nsteps, 1e-4)


def test_rccl_transport_single_rank_equals_plain_engine():
    """The RCCL code path itself (communicator, ncclAllGather, grouped send / recv, all-reduce) with the one rank a single
    GPU can host: the result must be the plain single-GPU engine's."""
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
    sim = MgspGroupRank(sc, 0, 1, device=0)
    sim.initial_setup()
    sim.run_fixed(30, 1e-4)
    got = sim.local_state()
    sim.close()
    ref = run_engine(sc, 30, 1e-4)
    for m in range(2):
        xo = ref["state"][m][0]
        idx, _ = match(xo.astype(np.float64), got[m][0].astype(np.float64))
        assert np.abs(got[m][0][idx] - xo).max() < 2e-6


def test_cpp_group_compute_dt_equals_the_reference_golden():
    """mpm_group_compute_dt - the dt rule inside mpm_group_main_loop - against the outputs of the MGSP project's own compute_dt
    (Projects/MGSP/utility_funcs.hpp:32-55; tests/golden/g12_mgsp_dt_*, generated by tests/golden/gen/gen_golden_mgsp.sh): bit for bit.
    The reference's grid is 256^3 (Projects/MGSP/settings.h: DOMAIN_BITS = 8), so is the context's."""
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    rows = np.fromfile(os.path.join(g, "g12_mgsp_dt_in.f32"), dtype=np.float32).reshape(-1, 4)
    want = np.fromfile(os.path.join(g, "g12_mgsp_dt_out.f32"), dtype=np.float32)
    sc = scenes.two_spheres(bits=8, radius_cells=4.0, gap_cells=3.0)
    sim = MgspGroupRank(sc, 0, 1, device=0)
    try:
        for (mv, cur, nxt, dtd), w in zip(rows, want):
            got = np.float32(sim.api.group_compute_dt(sim.grp, float(mv), float(cur), float(nxt), float(dtd)))
            assert got.view(np.uint32) == np.float32(w).view(np.uint32), (mv, cur, nxt, dtd, got, w)
    finally:
        sim.close()


def test_cpp_group_adaptive_main_loop_matches_frames():
    """mpm_group_main_loop: MGSP's compute_dt (CFL 0.3, 0.51 rule) from the maximum velocity over all ranks; two frames."""
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
    res = _run_group_threads(sc, 2, 0, 0.0, adaptive=(2, 240, 1e-4))
    steps = [r[3] for r in res]
    assert steps[0] == steps[1] and steps[0] >= 2 * int(round((1 / 240) / 1e-4))
    n = sum(m["xyz"].shape[0] for m in sc["models"])
    assert sum(r[0][m][0].shape[0] for r in res for m in range(2)) == n
    for r in res:
        for m in range(2):
            assert np.isfinite(r[0][m][0]).all()


def _oracle_mgsp_main_loop(sc, frames, fps, dt_default, threads=8):
    """MgspBenchmark::main_loop (mgsp_benchmark.cuh:361-559) on the single-rank CPU oracle: the same adaptive loop the C++ group
    driver runs (MGSP's compute_dt - CFL 0.3, 0.51 frame-remainder rule, Projects/MGSP/utility_funcs.hpp:32-55 - from the maximum
    grid velocity, per-frame clock), phase by phase through the oracle's C ABI."""
    from claymore_amd.engine import build_engine
    api = oracle_api()
    eng = build_engine(sc, api=api)
    eng.initial_setup()
    api.raw.mpmo_set_threads(eng.ctx, threads)
    # the dt rule is the ORACLE's restatement of Projects/MGSP/utility_funcs.hpp:32-55 (pinned to the reference's outputs by
    # tests/golden/g12_mgsp_dt_*), not the product package's: the C++ driver is compared with the checker, not with a sibling
    dx = float(eng.dx)

    def rule(mv, cur, nxt, dtd):
        return float(api.raw.mpmo_fn_compute_dt_mgsp(float(mv), float(cur), float(nxt), float(dtd), dx))

    spf = float(np.float32(1.0) / np.float32(fps))
    nd = rule(0.0, 0.0, spf, dt_default)
    steps = 0
    for _ in range(frames):
        t = np.float32(0.0)
        while t < np.float32(spf):
            dt = nd
            assert dt > 0.0
            mv = float(np.sqrt(np.float32(eng.grid_update(dt))))
            nd = rule(mv, float(np.float32(t + np.float32(dt))), spf, dt_default)
            if not nd > 0.0:
                nd = rule(mv, 0.0, spf, dt_default)
            eng.g2p2g(dt, nd)
            eng.rebuild_partition()
            t = np.float32(t + np.float32(dt))
            steps += 1
    state = [eng.retrieve_state(m) for m in range(len(sc["models"]))]
    eng.close()
    return state, steps


def test_cpp_group_adaptive_main_loop_equals_oracle():
    """mpm_group_main_loop (adaptive dt from the maximum velocity over all ranks, CFL 0.3 / 0.51 rule, per-frame clock) against the
    oracle driven through the same loop: same number of substeps, positions within 1e-5 relative."""
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
    frames, fps, dt_default = 2, 240, 1e-4
    res = _run_group_threads(sc, 2, 0, 0.0, adaptive=(frames, fps, dt_default))
    want, steps = _oracle_mgsp_main_loop(sc, frames, fps, dt_default)
    assert [r[3] for r in res] == [steps, steps], ([r[3] for r in res], steps)
    for m in range(len(sc["models"])):
        xm = np.concatenate([r[0][m][0] for r in res])
        xo = want[m][0]
        assert xm.shape == xo.shape
        idx, _ = match(xo.astype(np.float64), xm.astype(np.float64))
        rel = np.abs(xm[idx].astype(np.float64) - xo).max(axis=1) / np.abs(xo).max(axis=1)
        assert rel.max() < 1e-5, rel.max()


def test_full_size_c4_two_spheres_4_ranks():
    """BASELINE config 4 at size: two fixed-corotated spheres of R = 84 dx (2 x 19.9 M particles) on the 512^3 grid, MGSP static
    particle partition over 4 ranks - here 4 engine contexts on the one GPU, the C++ group driver on its in-process transport.
    20 substeps; every particle accounted for on its rank, nothing lost or discarded, halo blocks exchanged, and the spheres move
    as free bodies do (they do not touch yet): x by +-1 m/s, y by g t^2 / 2."""
    sc = scenes.two_spheres_c4()
    n_models = [m["xyz"].shape[0] for m in sc["models"]]
    assert 19.5e6 < n_models[0] < 20.5e6 and n_models[0] == n_models[1]
    world, nsteps, dt = 4, 20, 1e-4
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    x0 = [m["xyz"][:, :2].astype(np.float64).mean(axis=0) for m in sc["models"]]
    del sc
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            sim = ranks[r]
            sim.initial_setup()
            sim.run_fixed(nsteps, dt)
            c, d = sim.eng.counts(), sim.eng.diagnostics()
            sums = []
            for m in range(2):
                x = sim.eng.retrieve_positions(m)
                assert np.isfinite(x).all()
                sums.append((x.shape[0], x[:, :2].astype(np.float64).sum(axis=0)))
            out[r] = dict(particles=[int(c.particles[m]) for m in range(2)], lost=int(d.lost_particles), disc=int(d.discarded_p2g),
                          sent=sum(sim.send_counts), halo=sim.n_halo_blocks, n_local=sim.n_local, sums=sums)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=900)
    for r in ranks:
        r.close()
    assert not errors, errors
    assert sum(o["lost"] for o in out) == 0 and sum(o["disc"] for o in out) == 0
    assert all(sum(o["particles"]) == o["n_local"] for o in out)
    assert min(o["sent"] for o in out) > 0 and min(o["halo"] for o in out) > 0      # every rank shares a slab interface
    t = nsteps * dt
    for m, sign in ((0, 1.0), (1, -1.0)):
        n = sum(o["sums"][m][0] for o in out)
        assert n == n_models[m]
        mean = sum(o["sums"][m][1] for o in out) / n
        assert abs((mean[0] - x0[m][0]) - sign * 1.0 * t) < 2e-2 * t                 # x: +-1 m/s
        fall = -9.8 * dt * dt * nsteps * (nsteps + 1) / 2                              # symplectic Euler: v_k = -g k dt, x += v_k dt
        assert abs((mean[1] - x0[m][1]) - fall) < 5e-2 * abs(fall) + 1e-7


def test_full_size_c5_fluid_dam_8_ranks():
    """BASELINE config 5 at size: the weakly compressible J-fluid dam of 256 x 192 x 256 cells (100.7 M particles) on the 1024^3 grid,
    MGSP static particle partition over 8 ranks - here 8 engine contexts on the one GPU, the C++ group driver on its in-process
    transport.  12 substeps at the scene's acoustic-CFL time step; every particle accounted for on its rank, nothing lost or discarded,
    every rank shares a slab interface and exchanges halo blocks, positions finite, and the dam - four cells above the wall zone - falls
    freely: y by g t^2 / 2 (symplectic Euler), no net motion in x and z."""
    sc = scenes.fluid_dam(10, (256, 192, 256))
    n_total = scenes.total_particles(sc)
    assert n_total == 256 * 192 * 256 * 8
    world, nsteps, dt = 8, 12, sc["dt"]
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    com0 = sc["models"][0]["xyz"].mean(axis=0, dtype=np.float64)
    del sc
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            sim = ranks[r]
            sim.initial_setup()
            sim.run_fixed(nsteps, dt)
            c, d = sim.eng.counts(), sim.eng.diagnostics()
            x = sim.eng.retrieve_positions(0)
            assert np.isfinite(x).all()
            out[r] = dict(particles=int(c.particles[0]), lost=int(d.lost_particles), disc=int(d.discarded_p2g), flags=int(d.overflow_flags),
                          sent=sum(sim.send_counts), halo=sim.n_halo_blocks, n_local=sim.n_local, n=x.shape[0], s=x.astype(np.float64).sum(axis=0))
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=1200)
    for r in ranks:
        r.close()
    assert not errors, errors
    assert sum(o["lost"] for o in out) == 0 and sum(o["disc"] for o in out) == 0 and all(o["flags"] == 0 for o in out)
    assert all(o["particles"] == o["n_local"] == o["n"] for o in out) and sum(o["n"] for o in out) == n_total
    assert min(o["sent"] for o in out) > 0 and min(o["halo"] for o in out) > 0      # every rank shares a slab interface
    com = sum(o["s"] for o in out) / n_total
    fall = -9.8 * dt * dt * nsteps * (nsteps + 1) / 2                                  # symplectic Euler: v_k = -g k dt, x += v_k dt
    assert abs((com[1] - com0[1]) - fall) < 5e-2 * abs(fall) + 2e-8, (com - com0, fall)
    assert abs(com[0] - com0[0]) < 2e-8 and abs(com[2] - com0[2]) < 2e-8


@pytest.mark.parametrize("material,transport", [(_ffi.SAND, "in-process"), (_ffi.FIXED_COROTATED, "in-process"), (_ffi.SAND, "peer"), (_ffi.SAND, "peer-tightpad")])
def test_cpp_group_equals_single_engine(material, transport, monkeypatch):
    """("peer-tightpad", ADVICE r5: the recovery of a truncated key list - re-tag behind the two G2P2G passes, collect again - on the hub's ASYNCHRONOUS
    exchange and key all-gather, where the ev_done / ev_kdone ordering matters as well; until now only the rccl double ran it.)
    ("peer": the peer-direct transport's code path - hipMemcpyPeerAsync behind the peer's event on the comm stream, no host
    synchronisation in the exchange or the key all-gather - with all contexts on the one GPU; MPM_GROUP_TRANSPORT is read when the group is made.)
    N ranks against ONE rank of the same engine: the static particle partition changes block numbering, sort order and the
    order of the float additions on shared grid blocks, and nothing else - every per-particle decision (Jacobi sweeps included: the
    convergence mask is per lane) depends on the particle alone.  150 substeps of two colliding bodies, 2 and 3 ranks: positions within
    1e-6 relative of the single-engine run (measured 2-3e-7, i.e. float-atomic noise; tools/nrank_vs_one.py)."""
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4, material=material)
    if material == _ffi.SAND:
        for m in sc["models"]:
            m["params"] = {}
    if transport.startswith("peer"):
        monkeypatch.setenv("MPM_GROUP_TRANSPORT", "peer")
    else:
        monkeypatch.delenv("MPM_GROUP_TRANSPORT", raising=False)
    if transport.endswith("tightpad"):
        monkeypatch.setenv("MPM_GROUP_PAD_TIGHT", "1")
    else:
        monkeypatch.delenv("MPM_GROUP_PAD_TIGHT", raising=False)
    nsteps = 150
    one = run_engine(sc, nsteps, 1e-4)
    for world in (2, 3):
        res = _run_group_threads(sc, world, nsteps, 1e-4, fixed=True)
        for m in range(len(sc["models"])):
            xm = np.concatenate([r[0][m][0] for r in res])
            xo = one["state"][m][0]
            idx, _ = match(xo.astype(np.float64), xm.astype(np.float64))
            rel = np.abs(xm[idx].astype(np.float64) - xo).max(axis=1) / np.abs(xo).max(axis=1)
            assert rel.max() < 1e-6, (world, m, rel.max())


def test_group_substep_reports_this_ranks_max_velocity():
    """mpm_group_substep returns the rank's max |v|^2 after its grid update (the input of MGSP's compute_dt, mgsp_benchmark.cuh:410-418),
    whether the grid update ran as its own kernel (phase by phase) or rode on the previous rebuild's carry-over (mpm_group_run_fixed)."""
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=3.0, speed=2.0)
    world = 2
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            sim = ranks[r]
            sim.initial_setup()
            mv = [sim.substep(1e-4, 1e-4) for _ in range(3)]        # separate grid-update kernel
            sim.run_fixed(4, 1e-4)                                  # fused into the carry-over
            mv.append(sim.substep(1e-4, 1e-4))
            out[r] = mv
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for r in ranks:
        r.close()
    assert not errors, errors
    for mv in out:
        assert all(3.9 < v < 4.2 for v in mv), mv                   # |v|^2 = 2^2 (+ a few mm/s of gravity)


def _run_growth_ranks(parts, calls, per_call, dt):
    """One in-process group over the per-rank scenes `parts`, `calls` x run_fixed(per_call).  Per rank: the exterior block count at set-up,
    its peak at the calls' ends, capacity() after set-up and at the end, the diagnostics, the positions per model."""
    world = len(parts)
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(parts[r], r, world, device=0, local_group=lg, prepartitioned=True) for r in range(world)]
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            sim = ranks[r]
            sim.initial_setup()
            ebc0 = peak = sim.eng.counts().exterior_blocks
            cap0 = sim.eng.capacity()
            for _ in range(calls):
                sim.run_fixed(per_call, dt)
                peak = max(peak, sim.eng.counts().exterior_blocks)
            d = sim.eng.diagnostics()
            out[r] = {"ebc0": ebc0, "peak": peak, "cap0": cap0, "cap1": sim.eng.capacity(), "lost": d.lost_particles, "dropped": d.dropped_particles,
                      "xyz": [sim.eng.retrieve_positions(m) for m in range(len(sim.eng.models))]}
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for r in ranks:
        r.close()
    assert not errors, errors
    return out


def test_a_grouped_rank_grows_its_block_capacity_inside_run_fixed():
    """Block-capacity growth of a grouped context: besides the arrays every context has it regrows the halo lists (overlap marks, halo and
    interior lists) and the per-peer send lists.  The scene of test_capacity_grows_inside_a_long_run_between_windows (two touching spheres
    flying apart: about 40 % more exterior blocks over 300 substeps) cut for 2 ranks, every rank 70 % full at set-up - below the 3/4 mark - in
    one mpm_group_run_fixed call; same trajectory as the same group with room to spare."""
    from claymore_amd.mgsp import partition_scene
    world, nsteps = 2, 300
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=-3.0)
    nm = len(sc["models"])

    def parts(max_blocks=None):
        ps = [partition_scene(sc, r, world) for r in range(world)]
        for r, p in enumerate(ps):
            p["config"] = dict(sc["config"], **({"max_blocks": max_blocks[r]} if max_blocks else {}))
        return ps
    roomy = _run_growth_ranks(parts(), 30, nsteps // 30, sc["dt"])
    tight = _run_growth_ranks(parts([int(o["ebc0"] / 0.70) for o in roomy]), 1, nsteps, sc["dt"])
    print("grouped growth: roomy (ebc0, peak) %s; tight capacity (blocks, bins, events) at set-up %s, at the end %s" % (
        [(o["ebc0"], o["peak"]) for o in roomy], [o["cap0"] for o in tight], [o["cap1"] for o in tight]))
    must = [r for r in range(world) if roomy[r]["peak"] > tight[r]["cap0"][0] * 3 // 4]      # these ranks will have to grow
    assert all(o["cap0"][2] == 0 for o in tight) and must, [(o["ebc0"], o["peak"]) for o in roomy]
    for r in must:
        assert tight[r]["cap1"][2] >= 1 and tight[r]["cap1"][0] > tight[r]["cap0"][0], (r, tight[r]["cap0"], tight[r]["cap1"])
    assert all(o["lost"] == 0 and o["dropped"] == 0 for o in roomy + tight)
    for m in range(nm):
        want = np.concatenate([o["xyz"][m] for o in roomy]).astype(np.float64)
        got = np.concatenate([o["xyz"][m] for o in tight]).astype(np.float64)
        assert got.shape == want.shape
        idx, _ = match(want, got)
        rel = np.abs(got[idx] - want).max(axis=1) / np.abs(want).max(axis=1)
        assert rel.max() < 2e-6, (m, rel.max())


@pytest.fixture(scope="session")
def rccl_double_library(tmp_path_factory):
    """Build tests/rccl_double/rccl_double.cpp (an in-process double of the RCCL calls the group driver binds) with hipcc, once per session."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("rccl_double") / "librccl_double.so"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_double", "rccl_double.cpp")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(out), src, "-lpthread"], check=True, capture_output=True, timeout=600)
    return str(out)


@pytest.mark.parametrize("world,kind", [(2, "fixed"), (3, "substeps"), (4, "fixed"), (2, "adaptive"), (3, "fixed-nodefer"), (4, "fixed-big"), (8, "fixed-big"), (4, "fixed-big-sync"), (8, "fixed-big-sync"), (2, "plate"), (2, "plate-fall"), (3, "resume"),
                                        (4, "fixed-big-tightpad"), (4, "fixed-big-tightpad-nodefer"), (4, "fixed-big-overlaptag")])
def test_rccl_transport_with_several_ranks_through_the_rccl_double(world, kind, rccl_double_library):
    """The RCCL branch of the group driver with world > 1 (RCCL itself cannot host two ranks on one device, the box has one GPU):
    every rank a thread with its own context, mpm_group_create with a unique id, the grouped ncclSend / ncclRecv of the halo exchange,
    the ncclAllGather of the keys and the ncclAllReduce of the maximum velocity served by an in-process double loaded through
    MPM_RCCL_LIBRARY (tests/rccl_double/).  The double is STREAM-ORDERED like the real library (copies enqueued behind the peer's event,
    nothing synchronises the host), so a stream dependency the driver forgot is a race here too; "fixed-big" runs 4.2 M particles in contact,
    launches long enough for such a race to show, against the plain single-GPU engine; "plate" is the regression scene of the windowed loop's
    stale interior-block count (a rank whose blocks are all halo blocks at first, all interior 20 substeps later: it used to lose half its
    particles without a flag).  Runs in a subprocess (the library binds its
    collective library once per process)."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPM_RCCL_LIBRARY=rccl_double_library)
    if kind.endswith("-overlaptag"):   # the optional overlap of the tagging chain with the rebuild's last kernel (MPM_GROUP_OVERLAP_TAG=1) ran in no test
        env["MPM_GROUP_OVERLAP_TAG"] = "1"
        kind = kind[:-11]
    if kind.endswith("-sync"):    # the double's other mode: every call synchronises the host (a mutant of the driver without the comm stream's wait for the
        env["RCCL_DOUBLE_SYNC"] = "1"   # collect kernel fails here at once, in the stream-ordered mode only sometimes: profiles/r04_double_mutants.txt)
        kind = kind[:-5]
    if kind.endswith("-nodefer") and kind != "fixed-nodefer":
        env["MPM_GROUP_DEFER"] = "0"
        kind = kind[:-8]
    tight = "-tightpad" in kind
    if tight:
        # The key lists of the tagging all-gather travel WITHOUT slack (MPM_GROUP_PAD_TIGHT=1): every substep in which a rank's block count grows
        # truncates its list.  The windowed loop then repeats the tagging behind the two G2P2G passes that already ran on the incomplete one and
        # collects again (round 4 gave up with MPM_ERR_CAPACITY there: ADVICE r4); the loop that waits per substep tags again at once.  Same physics.
        env["MPM_GROUP_PAD_TIGHT"] = "1"
        env["MPM_GROUP_VERBOSE"] = "1"
        kind = kind.replace("-tightpad", "")
    if kind == "fixed-nodefer":   # the same loop with the host waiting at the end of every substep (what "fixed" defers behind the next halo-first launch)
        env["MPM_GROUP_DEFER"] = "0"
        kind = "fixed"
    r = subprocess.run([sys.executable, os.path.join(here, "rccl_double", "run_group.py"), str(world), kind], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "OK world" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    if tight:
        import re
        retags = [int(m) for m in re.findall(r"(\d+) key-list re-tags", r.stderr)]
        assert len(retags) == world and max(retags) > 0, ("the scene never outgrew a key list: the recovery did not run", r.stderr[-2000:])


@pytest.fixture(scope="session")
def stale_interior_mutant(tmp_path_factory):
    """The engine library with round 4's windowed-loop bug put back (-DMPM_EXPERIMENT -DMPM_HACK_STALE_INTERIOR: the interior G2P2G pass is
    skipped on a block count the host has not seen yet), built once per session."""
    import shutil
    import subprocess
    import __graft_entry__ as ge
    hipcc = shutil.which("hipcc") or ge.HIPCC
    out = tmp_path_factory.mktemp("mutant") / "libclaymore_stale.so"
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "claymore_amd", "csrc", "claymore_hip.hip")
    subprocess.run([hipcc] + ge.HIP_FLAGS + ["-DMPM_EXPERIMENT", "-DMPM_HACK_STALE_INTERIOR", "-o", str(out), src, "-ldl", "-lpthread"], check=True, capture_output=True, timeout=900)
    return str(out)


def test_the_librarys_books_catch_the_windowed_loops_particle_loss(rccl_double_library, stale_interior_mutant):
    """VERDICT r4 #4c: round 4's windowed group loop lost the particles of a few blocks with nothing counted as lost, and only bench.py's
    end-of-run self-check noticed.  With the bug put back (a mutant build) on the regression scene, the library's own books - particles
    bucketed + lost + dropped == particles added, checked at every host synchronisation and, on the device, in every rank's status word -
    stop the run with MPM_ERR_INTERNAL on the rank that lost them AND on its peer in the same substep (gmpm_simulator.cuh:617 only prints the total)."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPM_RCCL_LIBRARY=rccl_double_library, RUN_GROUP_LIBRARY=stale_interior_mutant)
    r = subprocess.run([sys.executable, os.path.join(here, "rccl_double", "run_group.py"), "2", "plate-stale"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK world 2 plate-stale" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("world", [2, 3])
def test_a_failing_rank_fails_every_rank_and_nobody_hangs(world, rccl_double_library):
    """Error propagation of the group driver on the RCCL branch: one rank outgrows its block capacity inside mpm_group_run_fixed.  Its
    status word travels in row 0 of the padded key all-gather, so every rank sees it at the same read-back and returns MPM_ERR_CAPACITY;
    without that the peers would sit in the next ncclRecv forever (the subprocess would hit its timeout)."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MPM_RCCL_LIBRARY=rccl_double_library)
    r = subprocess.run([sys.executable, os.path.join(here, "rccl_double", "run_group.py"), str(world), "fail"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK world" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.fixture(scope="session")
def rccl_double_mp_library(tmp_path_factory):
    """Build tests/rccl_double/rccl_double_mp.cpp (the MULTI-PROCESS double of the RCCL calls: data staged through a shared mapping) once per session."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("rccl_double_mp") / "librccl_double_mp.so"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rccl_double", "rccl_double_mp.cpp")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(out), src, "-lpthread"], check=True, capture_output=True, timeout=600)
    return str(out)


@pytest.mark.parametrize("world", [2, 4])
def test_the_drivers_multi_process_bench_launch_on_one_gpu(world, rccl_double_mp_library, tmp_path):
    """The launch the driver uses for its scaling curve - python -m torch.distributed.run --nproc-per-node N bench.py --gpus N - with N
    PROCESSES sharing the one GPU (bench.py --oversubscribe) and the collectives served by the multi-process double (MPM_RCCL_LIBRARY):
    gloo rendez-vous, the unique id broadcast from rank 0, ncclCommInitRank in every process, the rank's slab of the column, the C++ group
    loop, bench.py's self-check over all ranks (every particle bucketed, nothing lost or discarded), the max over ranks and the ONE JSON
    line on rank 0's stdout.  What it cannot show is RCCL itself and the timing."""
    import json
    import socket
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    frac = 1.0 / 32.0
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "6", "--warmup", "3", "--oversubscribe", "--watchdog", "500"]
    cmd += ["--fraction", str(frac)]   # (strong scaling, BASELINE's metric: the one column cut into `world` slabs on particle-block faces)
    env = dict(os.environ, MPM_RCCL_LIBRARY=rccl_double_mp_library, RCCL_DOUBLE_DIR=str(tmp_path), RCCL_DOUBLE_TIMEOUT_S="200", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-6000:])
    rec = json.loads(lines[0])
    assert rec.get("error") is None, rec
    assert rec["n_gpus"] == world and rec["steps"] == 6 and rec["warmup"] == 3 and rec["scaling"] == "strong" and rec["value"] > 0
    assert f"x{world}" in rec["config"]["parallelism"] and "oversubscribed" in rec["config"]
    assert "block-aligned" in rec["config"]["parallelism"]
    assert rec["roofline"]["particles_per_launch"] * world == pytest.approx(rec["config"]["particles"], rel=0.11)   # block-aligned slabs: within 10 % of the equal share (scenes.split_slabs)
    assert "collective library" in r.stderr and "rccl_double_mp" in r.stderr                                        # the library says what it loaded


def test_bench_two_ranks_on_real_rccl_when_the_box_has_two_gpus():
    """The same launch on the real library: skipped on the one-GPU boxes this suite usually runs on; on a box with two or more GPUs it is
    the first place RCCL carries the halo exchange between two devices (strong scaling of a 1/32-scale column, bench.py's self-check)."""
    import json
    import socket
    import subprocess
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5", "--fraction", str(1.0 / 32.0), "--watchdog", "500"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MPM_RCCL_LIBRARY", None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-2000:], r.stderr[-6000:])
    rec = json.loads(lines[0])
    assert rec.get("error") is None and rec["n_gpus"] == 2 and rec["value"] > 0, rec
    assert rec["config"]["self_check"]["lost_particles"] == 0 and rec["config"]["self_check"]["particles_bucketed"] == rec["config"]["particles"]

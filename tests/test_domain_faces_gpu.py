"""Parity with the oracle in the outer shell of the domain: particles in the wall zone of all six faces, in cells -2 / -1 of the lower faces
(node index 0 / 1, truncated into block 0 and wrapped by the G2P2G sort key), in the top cells of every axis (stencils that reach block G, which
has no table entry) and at exact rounding ties.  Scenes: tests/face_scenes.py.  Tolerances are the suite's (tests/test_parity_gpu.py)."""
import os

import numpy as np
import pytest

import face_scenes as F
from claymore_amd.engine import build_engine
from oracle_ffi import oracle_api
from parity_util import grid_compare, grid_velocity_compare, match_and_compare, run_pair

pytestmark = pytest.mark.gpu
POS_TOL = 1e-5


def _setup_only(scene, api):
    eng = build_engine(scene, api=api)
    eng.initial_setup()
    out = {"counts0": eng.counts(), "totals0": eng.grid_totals(), "grid": eng.dump_grid()}
    if api is None:
        out["diag"] = eng.diagnostics()
    eng.close()
    return out


def _no_extra_hip_blocks(res):
    """The converse of grid_compare's check: every non-empty HIP block is a block of the oracle's grid too."""
    kh, bh = res["hip"]["grid"]
    ko = {tuple(k) for k in res["oracle"]["grid"][0]}
    for k, b in zip(kh, bh):
        assert tuple(k) in ko or not np.any(b), ("HIP has a non-empty grid block the oracle lacks", tuple(k))


def _books(res, counts="counts"):
    """Both engines hold the same blocks and keep the same particles; HIP's lost + dropped counters account for exactly the particles the
    oracle does not keep (the oracle has no counters: a particle it loses is missing from its buckets)."""
    ch, co = res["hip"][counts], res["oracle"][counts]
    assert (ch.particle_blocks, ch.neighbor_blocks, ch.exterior_blocks) == (co.particle_blocks, co.neighbor_blocks, co.exterior_blocks), \
        ((ch.particle_blocks, ch.neighbor_blocks, ch.exterior_blocks), (co.particle_blocks, co.neighbor_blocks, co.exterior_blocks))
    nm = len(res["scene"]["models"])
    kept_h, kept_o = [ch.particles[i] for i in range(nm)], [co.particles[i] for i in range(nm)]
    assert kept_h == kept_o, (kept_h, kept_o)
    added = sum(m["xyz"].shape[0] for m in res["scene"]["models"])
    d = res["hip"]["diag"]
    assert d.lost_particles + d.dropped_particles == added - sum(kept_o), (d.lost_particles, d.dropped_particles, added, sum(kept_o))


def test_setup_grid_at_the_six_faces_node_by_node():
    """The rasterized grid after set-up (rasterize_blocks_kernel) against the oracle and against the float64 restatement, node by node: slabs
    at cell offsets 0 .. 3.5 from every face (n - 0.01 .. n - 3.5 at the upper ones), exact ties at even and odd k, the eight corners and the
    twelve edges.  Particles with x / dx < 0.5 put mass on node -1, which lies below the block's LDS node cube: the kernel must drop it, as the
    oracle does (tests/test_rasterize_faces_model.py); the stencils of the top cells reach block G, which has no table entry."""
    sc = F.setup_slab_scene(5)
    res = {"hip": _setup_only(sc, None), "oracle": _setup_only(sc, oracle_api()), "scene": sc}
    _books(res, "counts0")
    assert res["hip"]["diag"].lost_particles == 0 and res["hip"]["diag"].dropped_particles == 0
    assert grid_compare(res) < 1e-5, grid_compare(res)
    _no_extra_hip_blocks(res)
    th, to = res["hip"]["totals0"], res["oracle"]["totals0"]
    assert abs(th[0] - to[0]) < 1e-5 * abs(to[0]), (th, to)
    assert np.abs(th[1:] - to[1:]).max() < 1e-5 * abs(to[0]), (th, to)       # (|v0| ~ 1: momentum on the mass scale)
    ref, _ = F.reference_setup_grid(sc)
    ref = {nd: v for nd, v in ref.items() if v[0] > 0}
    got = F.grid_to_nodes(*res["hip"]["grid"])
    assert set(got) == set(ref), (sorted(set(got) ^ set(ref))[:8])
    scale = max(v[0] for v in ref.values())
    worst = max(float(np.abs(got[nd] - ref[nd]).max()) for nd in ref) / scale
    assert worst < 1e-5, worst


@pytest.mark.parametrize("direction", ["out", "in"])
def test_wall_zone_bodies_at_all_six_faces(direction):
    """One elastic body per face, 12 cells deep from the outer two cells through the 8-cell wall zone, thrown out of the domain or into it: the slip
    walls of grid_update_kernel and of the fused carry_grid_kernel<true> on all six faces.  Grid and grid velocities node by node after 1 and
    10 substeps, particles (position, b) after 60."""
    sc = F.wall_zone_scene(5, direction)
    for nsteps in (1, 10):
        res = run_pair(sc, nsteps, 1e-4, collect_grid=True)
        _books(res, "counts0")
        _books(res)
        g, v = grid_compare(res), grid_velocity_compare(res)
        assert g < 1e-5 and v < 1e-5, (nsteps, g, v)
        _no_extra_hip_blocks(res)
    res = run_pair(sc, 60, 1e-4)
    _books(res)
    err = match_and_compare(res)
    assert err["pos_rel"] < POS_TOL, err
    assert err["state_rel"] < 1e-4 and err["logjp_abs"] < 1e-4, err
    assert err["grid_mass_rel"] < 1e-5, err


def test_lower_face_materials_parity():
    """J-fluid, fixed-corotated, sand and NACC bodies against the three lower faces, moving toward them: particles of cells -2 / -1 are
    bucketed into block 0 and the G2P2G sort key wraps them ((cx & 3) + 1, like the oracle).  Positions, b and log Jp after 40 substeps (b and
    log Jp measured 3.0e-5 / 2.2e-5: the sand body yields against z = 0 and its return mapping amplifies rounding, as in
    test_parity_gpu.py::test_long_run_sand_stays_close_to_the_oracle; the grid is compared block by block, not node by node, for that reason)."""
    sc = F.lower_face_materials_scene(5)
    res = run_pair(sc, 40, 1e-4, collect_grid=True)
    _books(res, "counts0")
    _books(res)
    err = match_and_compare(res)
    assert err["pos_rel"] < POS_TOL, err
    assert err["state_rel"] < 1e-4 and err["logjp_abs"] < 1e-4, err
    assert err["grid_mass_rel"] < 1e-5, err
    _no_extra_hip_blocks(res)


@pytest.mark.parametrize("mask", ["0", "0xF"])
def test_lower_face_materials_with_both_g2p2g_kernels(mask):
    """test_lower_face_materials_parity with the G2P2G kernel forced per process (MPM_G2P2G_PAIRS, read once by the library): one particle per
    lane for every material ("0") and two per lane for all four ("0xF")."""
    import subprocess
    import sys
    env = dict(os.environ, MPM_G2P2G_PAIRS=mask)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_lower_face_materials_parity"], env=env, capture_output=True, text=True, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and "1 passed" in tail and "failed" not in tail, (mask, tail, r.stderr[-1500:])


@pytest.mark.parametrize("boundary", ["sticky", "slip", "separate"])
def test_collision_object_in_a_wall_zone_corner(boundary):
    """A level-set sphere in the x = 0 / y = 0 edge, a body against x = 0 falling onto it: grid_update_collider_kernel<CollisionArgs> sees object nodes in
    wall-zone blocks (left to the slip walls) and next to them (resolved).  Positions after 80 substeps, the grid and its velocities node by
    node (velocities: the suite's bound beyond 10 substeps, test_parity_gpu.py::test_grid_velocity_parity_over_many_substeps)."""
    sc = F.corner_obstacle_scene(5, boundary)
    res = run_pair(sc, 80, 1e-4, collect_grid=True)
    _books(res, "counts0")
    _books(res)
    err = match_and_compare(res)
    assert err["pos_rel"] < POS_TOL, err
    assert err["state_rel"] < 1e-4, err
    g, v = grid_compare(res), grid_velocity_compare(res)
    assert g < 1e-5 and v < 2.4e-5, (g, v)
    _no_extra_hip_blocks(res)

"""No driver's offer leaks into the next call.  What one substep's launches are offered - the fused carry-over, the still path, the phase stamps, the
lean events - is a value the driver fills per substep (claymore_hip.hip: SubstepPlan), so drivers can follow one another on one context in any order
and compute what one driver alone computes.

(a) Single context, the deterministic sparse scene of tests/test_collision_clock_gpu.py as tests/test_grid_update_kernels_gpu.py runs it (no object,
gravity): mpm_run_fixed(6), two mpm_substep calls, two phase-level substeps, mpm_run_fixed(6) against sixteen mpm_run_fixed(1) calls - positions,
material state and the grid bit for bit, as that file compares its drivers.  Again with MPM_PHASE_TIMERS=events and with MPM_STILL_LAUNCH=thin:2,
which a context reads at its creation: each in a child process.
(b) A two-rank in-process group on the two colliding spheres of tests/test_mgsp_gpu.py: mpm_group_run_fixed(4), two mpm_group_substep calls,
mpm_group_run_fixed(4) against one mpm_group_run_fixed(10), within the 1e-6 relative that file allows between two runs of that scene (float atomics).
Every call checks the particle books itself and fails with MPM_ERR_INTERNAL if they do not balance."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)                                         # (the child runs start this file as a script)
from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import build_engine  # noqa: E402
from claymore_amd.mgsp import LocalGroup, MgspGroupRank  # noqa: E402
from parity_util import match  # noqa: E402

pytestmark = pytest.mark.gpu

WHAT = ("positions", "state", "grid keys", "grid")


def sparse():
    from test_collision_clock_gpu import sparse_scene
    sc = sparse_scene(material=_ffi.FIXED_COROTATED)
    sc["collision"] = None
    sc["config"]["gravity"] = -9.8
    return sc


def single_runs():
    """[mixed drivers, sixteen mpm_run_fixed(1)] -> (positions, state, grid keys, grid bits) each, rows in the canonical order."""
    from test_grid_update_kernels_gpu import grid_rows, sorted_rows, state_rows
    sc = sparse()
    dt = sc["dt"]
    runs = []
    for how in ("mixed", "one by one"):
        eng = build_engine(sc)
        eng.initial_setup()
        if how == "mixed":
            eng.run_fixed(6, dt)
            for _ in range(2):
                nd, _ = eng.substep(dt, 0.0, 1.0, dt)
                assert nd == np.float32(dt), (nd, dt)               # (the scene is slow: compute_dt returns dt_default)
            for _ in range(2):
                eng.grid_update(dt)
                eng.g2p2g(dt, dt)
                eng.rebuild_partition()
            eng.run_fixed(6, dt)
        else:
            for _ in range(16):
                eng.run_fixed(1, dt)
        d = eng.diagnostics()
        assert int(d.lost_particles) == 0
        runs.append((sorted_rows(eng.retrieve_positions(0)), state_rows(eng)) + grid_rows(eng))
        eng.close()
    return runs


def assert_same_bits(runs):
    assert runs[0][0].shape == (48, 3) and runs[0][1].shape == (48, 13)
    for what, a, b in zip(WHAT, runs[0], runs[1]):
        assert a.shape == b.shape and np.array_equal(a, b), (what, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))


def test_drivers_in_turn_on_one_context():
    assert "MPM_PHASE_TIMERS" not in os.environ and "MPM_STILL_LAUNCH" not in os.environ, "this case is the default: run it without the switches"
    assert_same_bits(single_runs())


@pytest.mark.parametrize("switch", ["MPM_PHASE_TIMERS=events", "MPM_STILL_LAUNCH=thin:2"])
def test_drivers_in_turn_on_one_context_under_a_switch(switch, tmp_path):
    path = str(tmp_path / "runs.npz")
    name, value = switch.split("=")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    z = np.load(path)
    assert_same_bits([[z[f"{k}_{i}"] for i in range(4)] for k in ("mixed", "ones")])


def group_run(sc, calls):
    """Two ranks on one GPU, one thread each; calls: what every rank issues, ("fixed", n) or ("substep", n).  -> per model the ranks' positions in one array."""
    world, dt = 2, 1e-4
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            sim = ranks[r]
            sim.initial_setup()
            for kind, n in calls:
                if kind == "fixed":
                    sim.run_fixed(n, dt)
                else:
                    for _ in range(n):
                        sim.substep(dt, dt)
            out[r] = sim.local_state()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    for r in ranks:
        r.close()
    assert not errors, errors                                      # (unbalanced books are an error of the call that finds them)
    return [np.concatenate([out[r][m][0] for r in range(world)]) for m in range(len(sc["models"]))]


def test_group_drivers_in_turn():
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
    mixed = group_run(sc, [("fixed", 4), ("substep", 2), ("fixed", 4)])
    one = group_run(sc, [("fixed", 10)])
    for m, (xm, xo) in enumerate(zip(mixed, one)):
        assert xm.shape == xo.shape
        idx, _ = match(xo.astype(np.float64), xm.astype(np.float64))
        rel = np.abs(xm[idx].astype(np.float64) - xo).max(axis=1) / np.abs(xo).max(axis=1)
        print("model", m, "mixed group drivers vs one run_fixed(10): pos_rel", rel.max())
        assert rel.max() < 1e-6, (m, rel.max())


if __name__ == "__main__":
    mixed, ones = single_runs()
    np.savez(sys.argv[1], **{f"mixed_{i}": a for i, a in enumerate(mixed)}, **{f"ones_{i}": a for i, a in enumerate(ones)})

"""The phase timers of mpm_run_fixed from the stamps its kernels write (mpm_kernels.hpp: phase_stamp) against the HIP events they replace
(MPM_PHASE_TIMERS=events, read when a context is created: the events runs are a child process).

Scene: C1 (scenes.two_spheres(): two models, 48 840 particles, 128^3), 16 substeps in ONE mpm_run_fixed call, with sync_interval 8 (two full windows) and 3
(five full windows and a short one: the closing launch and the row hand-over between windows six times).  The call's first substep launches the stand-alone
grid update and keeps its events in both modes; the other fifteen are stamped.

Measured on an MI355X (profiles/substep_fixed_cost.txt, section 6): grid_update_ms 0.00408, g2p2g_ms 0.04920, partition_ms 0.01661, total_ms 0.06989 at
sync_interval 8 (0.00433 / 0.04913 / 0.01652 / 0.06998 at 3), the call's wall time 1.17 ms for 16 x 0.0699 = 1.12 ms of device time."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)                                         # (the events runs start this file as a script)
from claymore_amd import scenes  # noqa: E402
from claymore_amd.engine import build_engine  # noqa: E402
from parity_util import match  # noqa: E402

pytestmark = pytest.mark.gpu

STEPS, DT = 16, 1e-4
REPEATS = 3
# two runs of the engine differ in the order of their float atomics (P2G sums): test_still_rebuild_gpu.RUN_TOL, the bound of
# test_parity_gpu.test_run_fixed_is_independent_of_the_sync_interval
RUN_TOL = 2e-6


def c1(sync_interval):
    sc = scenes.two_spheres()
    sc["config"] = dict(sc["config"], sync_interval=sync_interval)
    return sc


def run(sync_interval, books=False):
    """One call of 16 substeps on a fresh context: timers, the host's wall time of the call, counts, the states of both models."""
    sc = c1(sync_interval)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.api.sync(eng.ctx)
    t0 = time.perf_counter()
    eng.run_fixed(STEPS, DT)
    wall_ms = 1e3 * (time.perf_counter() - t0)
    tm = eng.timers()
    cnt = eng.counts()
    out = {"grid": float(tm.grid_update_ms), "g2p2g": float(tm.g2p2g_ms), "part": float(tm.partition_ms), "total": float(tm.total_ms), "wall_ms": wall_ms,
           "last_g2p2g": float(eng.last_g2p2g_ms()), "blocks": [cnt.particle_blocks, cnt.neighbor_blocks, cnt.exterior_blocks],
           "particles": [int(cnt.particles[i]) for i in range(cnt.model_count)], "still": int(eng.diagnostics().still_rebuilds),
           "lost": int(eng.diagnostics().lost_particles)}
    state = [eng.retrieve_state(m)[0] for m in range(2)]
    if books:
        import rebuild_books
        assert eng.api.check_table(eng.ctx) == 0
        out["findings"] = rebuild_books.check_books(eng.save_checkpoint().copy(), [eng.dump_block_rows(m) for m in range(2)], sc["bits"], eng.cfg.max_ppc,
                                                    counts=out["particles"])
    eng.close()
    return out, state


def rel_dev(x, ref):
    """Largest relative position difference after bringing both runs' particles into one order (parity_util.match: particle order is unspecified, and a
    lexicographic sort of float positions that differ in their last bits would pair the wrong ones)."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    idx, _ = match(ref, x)
    return float((np.abs(x[idx] - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def child_main(path):
    """MPM_PHASE_TIMERS=events is in this process's environment: a warm-up run, REPEATS runs at sync_interval 8 (their spread), one at 3."""
    run(8)
    reps = [run(8, books=(i == 0)) for i in range(REPEATS)]
    three = run(3)
    np.savez(path, s8_0=reps[0][1][0], s8_1=reps[0][1][1], s3_0=three[1][0], s3_1=three[1][1])
    reps[0][0]["findings"] = [repr(f) for f in reps[0][0]["findings"]]
    print("RESULT " + json.dumps({"reps": [r[0] for r in reps], "three": three[0]}))


@pytest.fixture(scope="module")
def events(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("events") / "state.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, MPM_PHASE_TIMERS="events"), capture_output=True, text=True,
                       timeout=300, cwd=os.path.dirname(os.path.abspath(__file__)))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    res = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    res["state"] = dict(np.load(path))
    return res


@pytest.fixture(scope="module")
def stamps():
    assert os.environ.get("MPM_PHASE_TIMERS") != "events", "this module compares the default with the events: run it without the switch"
    run(8)                                                       # (warm-up: code objects, the allocator)
    return {8: run(8, books=True), 3: run(3, books=True)}


@pytest.mark.parametrize("k", [8, 3])
def test_the_phases_add_up_and_fit_into_the_call(stamps, k):
    t = stamps[k][0]
    print(k, t)
    assert t["grid"] > 0 and t["g2p2g"] > 0 and t["part"] > 0 and t["total"] > 0
    # Float rounding: a substep's three phase times and its total are float32 roundings of exact tick differences that add up (stamps), or four float32
    # values of the runtime's own subtraction of timestamps that add up (the call's first substep: events) - half an ulp of at most the substep's time each,
    # summed in float64 -, and the four averages are rounded to float32 once more: 4 x 2^-24 + 2 x 2^-24 of the total, rounded up to 4 ulp.
    assert abs(t["grid"] + t["g2p2g"] + t["part"] - t["total"]) <= 4 * 2.0 ** -23 * t["total"], t
    assert t["total"] * STEPS <= t["wall_ms"], t
    assert t["last_g2p2g"] > 0 and t["last_g2p2g"] < t["total"] * STEPS
    assert t["lost"] == 0 and not t["findings"], t["findings"][:5]


def test_stamps_do_not_exceed_the_events(stamps, events):
    """g2p2g_ms of the stamped run against the events run's, both sync_interval 8: the stamps' value may exceed the events' median by no more than the
    events runs' own spread (max - min of three repeats).

    Measured (profiles/substep_fixed_cost.txt, section 6): events 0.05164 / 0.05189 / 0.05232 ms (spread 0.00068), stamps 0.04920 ms - 0.0034 ms inside the
    bound, 0.0027 ms below the events' median (an event interval holds G2P2G's dispatch behind a barrier packet; the stamps run from its first workgroup to
    the compaction's).  At sync_interval 3: events 0.05179, stamps 0.04913."""
    ev = sorted(r["g2p2g"] for r in events["reps"])
    spread = ev[-1] - ev[0]
    print("events g2p2g_ms", ev, "spread", spread, "stamps", stamps[8][0]["g2p2g"], "stamps k=3", stamps[3][0]["g2p2g"], "events k=3", events["three"]["g2p2g"])
    assert stamps[8][0]["g2p2g"] <= ev[1] + spread
    for r in events["reps"] + [events["three"]]:
        assert r["grid"] > 0 and r["g2p2g"] > 0 and r["part"] > 0 and r["total"] * STEPS <= r["wall_ms"]


@pytest.mark.parametrize("k", [8, 3])
def test_both_modes_compute_the_same(stamps, events, k):
    """Counts and still rebuilds equal; books verified in both (tests/rebuild_books.py); the particle state equal particle by particle, to the bound two runs
    of one mode are held to (RUN_TOL: the order of the P2G atomics is not fixed)."""
    mine, state = stamps[k]
    theirs = events["reps"][0] if k == 8 else events["three"]
    for key in ("blocks", "particles", "still", "lost"):
        assert mine[key] == theirs[key], (key, mine[key], theirs[key])
    assert not events["reps"][0]["findings"]
    for m in range(2):
        assert state[m].shape == events["state"][f"s{k}_{m}"].shape
        rel = rel_dev(state[m], events["state"][f"s{k}_{m}"])
        print("model", m, "max relative position difference", rel)
        assert rel < RUN_TOL, rel


if __name__ == "__main__":
    child_main(sys.argv[1])

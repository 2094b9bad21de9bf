"""The still path of the partition rebuild (mpm_config.still_rebuild, mpm_diagnostics.still_rebuilds) on the GPU: a substep of mpm_run_fixed in
which no particle changed its block keeps the partition - same blocks, same numbers - instead of rebuilding it.  Every test states when the path
must be taken and when it must not, from particle positions (the oracle's, or the engine's own read back between substeps), and compares what the
run computes with the switched-off run and with the oracle.

A particle's block is a function of its position, (lround(x / dx) - 2) >> 2 per axis; particle order is unspecified on both sides, so "somebody
changed block in this substep" is read off the per-block particle counts before and after it (in these scenes no two particles can swap blocks)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from claymore_amd import _ffi, scenes
from claymore_amd.engine import build_engine
from oracle_ffi import oracle_api
from parity_util import match, match_and_compare

pytestmark = pytest.mark.gpu

POS_TOL = 1e-5      # test_parity_gpu.POS_TOL
RUN_TOL = 2e-6      # two runs of the engine against each other: test_run_fixed_is_independent_of_the_sync_interval
BITS, DX = 6, 1.0 / 64
STEPS, DT = 100, 1e-4


def falling_box(**config):
    """16^3 cells of sand at bits 6 (32 768 particles), eight cells clear of the wall zone on every side, thrown downwards at 0.5: a rigid
    free fall.  The lower particle of every node (node - 0.25 dx) leaves its cell after 0.25 dx, and for the node layers j = 2 mod 4 that cell
    face is a block face: 0.5 t + 4.9 t^2 = dx / 4 at t = 7.3e-3, in the eighth decade of the 100 substeps."""
    lo = np.array([24, 30, 24])
    xyz = scenes.lattice_box(BITS, lo, lo + 16)
    assert xyz.shape[0] == 32768
    return {"name": "falling_box", "bits": BITS, "dt": DT, "config": dict(config),
            "models": [{"material": _ffi.SAND, "xyz": xyz, "v0": (0.0, -0.5, 0.0), "params": {}}]}


def block_census(x):
    """per-block particle counts as a dict {block key: count}"""
    b = (np.rint(np.asarray(x, dtype=np.float64) / DX).astype(np.int64) - 2) >> 2
    keys, cnt = np.unique(b, axis=0, return_counts=True)
    return {tuple(int(v) for v in k): int(c) for k, c in zip(keys, cnt)}


def face_margin(x):
    """smallest distance of any coordinate to a cell face (cells are centred on the nodes), in dx"""
    g = np.asarray(x, dtype=np.float64) / DX - 0.5
    return float(np.abs(g - np.rint(g)).min())


def rel_dev(x, ref):
    idx, _ = match(ref.astype(np.float64), x.astype(np.float64))
    return float((np.abs(x[idx].astype(np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def still_count(eng):
    return int(eng.diagnostics().still_rebuilds)


def triple(c):
    return (c.particle_blocks, c.neighbor_blocks, c.exterior_blocks)


@pytest.fixture(scope="module")
def oracle_fall():
    """The oracle's trajectory of the falling box, substep by substep: which substeps move a particle to another block, and its final state."""
    sc = falling_box()
    api = oracle_api()
    ora = build_engine(sc, api=api)
    ora.initial_setup()
    api.raw.mpmo_set_threads(ora.ctx, 8)
    out = {"counts0": ora.counts(), "totals0": ora.grid_totals()}
    census = [block_census(ora.retrieve_positions(0))]
    margins = []
    for _ in range(STEPS):
        ora.run_fixed(1, DT)
        x = ora.retrieve_positions(0)
        census.append(block_census(x))
        margins.append(face_margin(x))
    out.update(counts=ora.counts(), totals=ora.grid_totals(), state=[ora.retrieve_state(0)])
    ora.close()
    crossing = [s for s in range(1, STEPS + 1) if census[s] != census[s - 1]]      # 1-based: substep s takes the state s - 1 to the state s
    return {"res": out, "crossing": crossing, "margins": margins, "census": census[-1]}


def book_findings(eng):
    """tests/rebuild_books.check_books on the context as it stands: everything the last rebuild wrote, the look-up rows included"""
    import rebuild_books
    assert eng.api.check_table(eng.ctx) == 0
    cnt = eng.counts()
    return rebuild_books.check_books(eng.save_checkpoint().copy(), [eng.dump_block_rows(0)], BITS, eng.cfg.max_ppc, counts=[int(cnt.particles[0])])


def hip_fall(still, stops=(), sync_interval=0, track_ids=False, steps=STEPS, books=False):
    """The falling box on the HIP engine.  stops: substep numbers after which the run is interrupted to read the counter and the positions.
    Returns the parity_util-style result, the readings {substep: (still_rebuilds, census)} and the engine's own block sets.  books: the books
    and look-up rows are verified (book_findings) at the first stop, which lies in a still streak of two or more, at the first stop whose
    substep moved a particle to another block, and at the first stop after that whose substep moved nobody (a streak of one); the readings
    {what: (substep, growth of still_rebuilds in it, findings)} come back as out["books"]."""
    from test_parity_gpu import _hip_block_sets
    cfg = {"still_rebuild": still}
    if sync_interval:
        cfg["sync_interval"] = sync_interval
    sc = falling_box(**cfg)
    sc["track_ids"] = track_ids
    eng = build_engine(sc)
    eng.initial_setup()
    out = {"counts0": eng.counts(), "totals0": eng.grid_totals()}
    seen, done = {}, 0
    for s in sorted(set(stops) | {steps}):
        eng.run_fixed(s - done, DT)
        done = s
        seen[s] = (still_count(eng), block_census(eng.retrieve_positions(0)))
        if books:
            checked = out.setdefault("books", {})
            what = None
            if not checked:
                what = "streak"
            elif s - 1 in seen:
                moved = seen[s][1] != seen[s - 1][1]
                if moved and "crossing" not in checked:
                    what = "crossing"
                elif not moved and "crossing" in checked and "streak of one" not in checked:
                    what = "streak of one"
            if what:
                checked[what] = (s, seen[s][0] - seen[s - 1][0] if s - 1 in seen else None, book_findings(eng))
    out.update(counts=eng.counts(), totals=eng.grid_totals(), state=[eng.retrieve_state(0)], diag=eng.diagnostics())
    assert eng.api.check_table(eng.ctx) == 0
    assert out["diag"].lost_particles == 0 and out["diag"].discarded_p2g == 0 and out["diag"].dropped_particles == 0
    if track_ids:
        xyz, ids = eng.retrieve_ids(0)
        out["by_id"] = xyz[np.argsort(ids, kind="stable")]
    sets, counts, _ = _hip_block_sets(eng, 10, 128 * 64, DX)
    assert counts == triple(out["counts"])
    eng.close()
    return out, seen, {k: len(v) for k, v in sets.items()}


def test_still_then_crossing_then_still(oracle_fall):
    """Test 1 of the issue.  The oracle says in which substeps particles change block: a short burst (the lower particles of four node layers
    cross a block face together, within rounding of each other), the first of them where the free fall puts it.  The engine is stopped around
    the burst: a substep in which one of ITS particles changed block must not count as still, every other one must (the first rebuild after
    set-up excepted: it is never offered the path).  Switched off the counter stays 0, and both runs agree with each other and with the oracle."""
    cross = oracle_fall["crossing"]
    t = (-0.5 + np.sqrt(0.25 + 4 * 4.9 * 0.25 * DX)) / 9.8            # 0.5 t + 4.9 t^2 = dx / 4
    assert cross and abs(cross[0] - t / DT) <= 2 and cross[-1] - cross[0] <= 3, (cross, t / DT)
    first = cross[0]
    # the final state decides nothing by a rounding tie: no coordinate within 1e-3 dx of a cell face (a substep moves a particle by 3.7e-3 dx)
    assert oracle_fall["margins"][STEPS - 1] > 1e-3, oracle_fall["margins"][STEPS - 1]
    window = range(first - 3, cross[-1] + 4)
    on, seen, sets_on = hip_fall(0, stops=window, books=True)
    off, seen_off, sets_off = hip_fall(-1)
    assert seen_off[STEPS][0] == 0
    slow = []
    for s in window[1:]:
        moved = seen[s][1] != seen[s - 1][1]
        grew = seen[s][0] - seen[s - 1][0]
        assert grew == (0 if moved else 1), (s, moved, grew)
        if moved:
            slow.append(s)
    print("oracle crossing substeps", cross, "engine", slow, "still_rebuilds", seen[STEPS][0], "oracle face margin", oracle_fall["margins"][first - 1])
    # the engine's first crossing is the oracle's, unless the oracle's own decision there hangs on less than 1e-4 dx (30 times the two sides' distance)
    assert slow and (slow[0] == first or oracle_fall["margins"][first - 1] < 1e-4 or oracle_fall["margins"][first - 2] < 1e-4), (slow, cross)
    assert seen[window[0]][0] == window[0] - 1                       # every substep before the burst but the first
    assert seen[STEPS][0] == STEPS - 1 - len(slow)                   # ... and every one after it
    assert 0.8 * STEPS <= seen[STEPS][0] < STEPS
    assert triple(on["counts"]) == triple(off["counts"]) == triple(oracle_fall["res"]["counts"])
    assert rel_dev(on["state"][0][0], off["state"][0][0]) < RUN_TOL
    for run in (on, off):
        err = match_and_compare({"hip": run, "oracle": oracle_fall["res"]})
        print(err)
        assert err["n"] == 32768 and err["pos_rel"] < POS_TOL, err
    assert sets_on == sets_off == oracle_fall["census"]
    # the books and look-up rows the rebuild left (tests/rebuild_books.py): in a still streak of two or more (rows passed over), after a full
    # rebuild (the crossing), and after the first still rebuild behind it (rows derived from the ones that stand)
    bk = on["books"]
    print("books verified at", {k: v[:2] for k, v in bk.items()})
    assert set(bk) == {"streak", "crossing", "streak of one"} and bk["streak"][0] == window[0] >= 3 and bk["crossing"][1] == 0 and bk["streak of one"][1] == 1
    assert all(not v[2] for v in bk.values()), {k: v[2][:5] for k, v in bk.items()}


def test_sync_interval(oracle_fall):
    """Test 2: the decision is taken on the device, so the window between two host synchronisations does not enter it."""
    runs = {k: hip_fall(0, sync_interval=k) for k in (1, 8, 64)}
    for k in (8, 64):
        assert triple(runs[k][0]["counts"]) == triple(runs[1][0]["counts"]) == triple(oracle_fall["res"]["counts"])
        assert runs[k][1][STEPS][0] == runs[1][1][STEPS][0] >= 0.8 * STEPS
        assert rel_dev(runs[k][0]["state"][0][0], runs[1][0]["state"][0][0]) < RUN_TOL


def test_material_at_rest_until_a_collider_arrives():
    """Test 3: scenes.sphere_through_block as the collision-clock tests run it (their SCENE: the smallest the project uses) - a block at rest
    without gravity, a sticky sphere that starts two cells clear of it and reaches the first particles' stencils after some 40 substeps.  Before
    that every rebuild but the first is still.  From then on particles move, and the counter grows exactly in the substeps in which none of them
    changed block (a pushed lattice crosses block faces in bursts, not in every substep): the run is stopped after every substep of the contact
    phase to see both.  Against the oracle driven with the same clock: the bound of test_collision_parity."""
    from test_collision_clock_cpu import SCENE, drive_oracle
    sc = scenes.sphere_through_block(boundary="sticky", **SCENE)
    steps, calm = 160, 30
    xo = drive_oracle(sc, steps)[0]
    eng = build_engine(sc)
    eng.initial_setup()
    x0 = eng.retrieve_positions(0)
    eng.run_fixed(calm, sc["dt"])
    assert still_count(eng) == calm - 1 > 0
    assert np.array_equal(np.sort(eng.retrieve_positions(0), axis=0), np.sort(x0, axis=0))        # nobody has moved yet
    prev, last = block_census(x0), still_count(eng)
    moved_steps = 0
    for s in range(calm + 1, steps + 1):
        eng.run_fixed(1, sc["dt"])
        cen, cnt = block_census(eng.retrieve_positions(0)), still_count(eng)
        moved = cen != prev
        assert cnt - last == (0 if moved else 1), (s, moved, cnt - last)
        moved_steps += moved
        prev, last = cen, cnt
    print("substeps with a block change:", moved_steps, "of", steps - calm, "still_rebuilds", last)
    assert moved_steps > 0 and last == steps - 1 - moved_steps
    xh = eng.retrieve_positions(0)
    assert eng.api.check_table(eng.ctx) == 0 and eng.diagnostics().lost_particles == 0
    eng.close()
    assert rel_dev(xh, xo) < POS_TOL


def _cloud(seed, lo, cells, per_cell=8):
    """particles at seeded random positions in a box of `cells`^3 cells: at a steady drift some of them change block in EVERY substep (a lattice
    body crosses its block faces layer by layer, once in dozens of substeps)"""
    rng = np.random.default_rng(seed)
    n = per_cell * cells ** 3
    return ((np.asarray(lo, dtype=np.float64) + rng.random((n, 3)) * cells) * DX).astype(np.float32)


def _two_models(v0, v1):
    prm = {"volume": float(np.float32(DX ** 3 / 8)), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "two_models", "bits": BITS, "dt": DT, "config": {"gravity": 0.0},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": _cloud(7, (14, 26, 26), 10), "v0": v0, "params": dict(prm)},
                       {"material": _ffi.FIXED_COROTATED, "xyz": _cloud(11, (38, 27, 27), 8), "v0": v1, "params": dict(prm)}]}


@pytest.mark.parametrize("case", ["first_moves", "second_moves", "both_rest"])
def test_two_models_one_at_rest_one_moving(case):
    """Test 4: two models on one grid, apart, no gravity (undeformed fixed-corotated material: a model given no velocity stays exactly where
    it is, a model given one drifts rigidly).  One flag serves both: while either model has a particle that changes block the counter stays 0 -
    the drifting cloud loses particles to other blocks in every substep, which is checked on the engine's own positions -, with both at rest
    every rebuild but the first is still.  One moving case against the oracle as in test_mixed_materials_share_one_grid_parity."""
    rest = (0.0, 0.0, 0.0)
    v = {"first_moves": ((1.0, 0.0, 0.0), rest), "second_moves": (rest, (0.0, -1.0, 0.6)), "both_rest": (rest, rest)}[case]
    mover = 0 if case == "first_moves" else 1
    sc = _two_models(*v)
    steps = 30
    eng = build_engine(sc)
    eng.initial_setup()
    if case == "both_rest":
        eng.run_fixed(steps, DT)
        assert still_count(eng) == steps - 1
    else:
        prev = [block_census(eng.retrieve_positions(m)) for m in range(2)]
        for s in range(steps):
            eng.run_fixed(1, DT)
            cen = [block_census(eng.retrieve_positions(m)) for m in range(2)]
            assert cen != prev, f"substep {s + 1}: nobody changed block - the scene does not test what it is meant to"
            assert cen[mover] != prev[mover] and cen[1 - mover] == prev[1 - mover]      # (the other model rests)
            prev = cen
        assert still_count(eng) == 0
    hip = {"state": [eng.retrieve_state(m) for m in range(2)], "totals": eng.grid_totals(), "counts": eng.counts()}
    assert eng.api.check_table(eng.ctx) == 0 and eng.diagnostics().lost_particles == 0
    eng.close()
    if case == "first_moves":
        ora = build_engine(sc, api=oracle_api())
        ora.initial_setup()
        ora.run_fixed(steps, DT)
        res = {"hip": hip, "oracle": {"state": [ora.retrieve_state(m) for m in range(2)], "totals": ora.grid_totals(), "counts": ora.counts()}}
        ora.close()
        err = match_and_compare(res)
        assert err["n"] == sum(m["xyz"].shape[0] for m in sc["models"]) and err["pos_rel"] < POS_TOL, err
        assert [hip["counts"].particles[i] for i in range(2)] == [res["oracle"]["counts"].particles[i] for i in range(2)]


def test_checkpoint_in_the_middle_of_a_streak():
    """Test 5: a checkpoint taken 20 substeps into a still streak, loaded into a fresh context: its first rebuild is not offered the path (the data
    was laid out by the host), the ones after it are, and the trajectory is the uninterrupted one."""
    sc = falling_box()
    a = build_engine(sc)
    a.initial_setup()
    a.run_fixed(20, DT)
    assert still_count(a) == 19
    buf = a.save_checkpoint().copy()
    a.run_fixed(21, DT)
    xa = a.retrieve_positions(0)
    a.close()
    b = build_engine(sc)
    b.initial_setup()
    b.load_checkpoint(buf)
    b.run_fixed(1, DT)
    assert still_count(b) == 0
    b.run_fixed(20, DT)
    assert still_count(b) == 20
    xb = b.retrieve_positions(0)
    assert b.api.check_table(b.ctx) == 0
    b.close()
    assert rel_dev(xb, xa) < RUN_TOL


def test_particle_ids_follow_through_still_rebuilds(oracle_fall):
    """Test 6: the side array of a tracked context is moved by the rows prepare leaves behind, on the still path those of the standing partition:
    30 still substeps, then on through the crossing; position by id against the switched-off run."""
    first = oracle_fall["crossing"][0]
    assert first > 31
    on, seen, _ = hip_fall(0, stops=(30,), track_ids=True)
    off, _, _ = hip_fall(-1, track_ids=True)
    assert seen[30][0] == 29 and seen[STEPS][0] < STEPS - 1
    assert on["by_id"].shape == off["by_id"].shape == (32768, 3)
    rel = np.abs(on["by_id"].astype(np.float64) - off["by_id"]).max(axis=1) / np.abs(off["by_id"]).max(axis=1)
    assert rel.max() < RUN_TOL, rel.max()


def test_one_particle_kernel_sets_the_flag_too():
    """Test 7: test 1 with the one-particle-per-lane kernel (MPM_G2P2G_PAIRS=0 is read once per process: a process of its own)."""
    if os.environ.get("MPM_G2P2G_PAIRS") == "0":
        pytest.skip("this is the inner run")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "test_still_then_crossing_then_still"], env=dict(os.environ, MPM_G2P2G_PAIRS="0"), capture_output=True, text=True, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0 and "1 passed" in tail and "failed" not in tail, (tail, r.stderr[-1500:])

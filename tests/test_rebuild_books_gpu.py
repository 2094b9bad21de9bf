"""The partition rebuild (claymore_amd/csrc/mpm_kernels.hpp: compact_blocks_kernel, both register_blocks_kernel phases, carry_grid_kernel's
numbering, prepare_blocks_kernel<SORT>) field by field: known particles in a known velocity field (injected through a checkpoint as
tests/test_g2p2g_blocks_gpu.py injects them), ONE mpm_g2p2g + mpm_rebuild_partition, then a checkpoint and mpm_dump_block_rows, and
tests/rebuild_books.check_books over everything the rebuild wrote - tiers, sizes, row_of, bins, every record, the list layout, the pair
counts, all 64 lanes of every look-up row - plus the one thing the books cannot say of themselves: every record's SORT KEY is the prediction of
the float64 model (g2p2g_model.step: per axis clamp(((narena - 1) & 3) + rint(nfd + vel new_dt / dx), 0, 5), y * 36 + x * 6 + z).  A particle is
left out of that comparison only when some axis' rint argument lies within 2 bound("pos") + 2^-20 of a half-integer, at most 1 % of a scene
(tests/test_rebuild_books_cpu.py asserts the cap for every generator on the model alone).  The scenes are those of tests/rebuild_scenes.py: bits 6,
max_ppc 16.  tests/test_still_rebuild_gpu.py calls check_books on the still path (streak 1, streak >= 2, after a crossing).

Both list layouts: the file runs in process with the default G2P2G mask (all materials in the pair layout) and, from
test_the_sliced_layout_passes_too, once more in a child process with MPM_G2P2G_PAIRS=0.

Stale launches (test_stale_launches): see its docstring for the thresholds crossed and the ones the public API does not reach.

Kernel mutations (value-only, each built in a scratch copy of mpm_kernels.hpp and never committed; each run ONCE on an MI355X against this file with
the default mask, without test_stale_launches - 64 unchecked substeps on wrong books - and without the child run; what failed, and the first finding):
  1 still path: the mirror index (53 - lane) & 63 -> (52 - lane) & 63      test_still_rebuild_rows at its first still rebuild: "row: source lane" (run alone: the other
                                                                           tests never take the still path).  tests/test_still_rebuild_gpu.py makes the same check at
                                                                           its "streak of one" stop: not run there; expected: test_still_then_crossing_then_still
  2 lanes 27-53: table_query at key + dir where key - dir belongs           all 11 tests run: "row: destination lane" in every block (test_drop_overflow: the dropped
                                                                           count first - the particles went to the wrong neighbour)
  3 nbins = c / kBin without the round-up                                  10 of 11: "bin ranges do not tile [0, bincount)" (test_drop_overflow passes: 1024 = 16 bins)
  4 register_blocks_kernel: `bound` not rounded up to whole workgroups     left out: lanes past `total` would leave the loop while their workgroup's other waves wait at
                                                                           block_append's barriers - reading the code, a hang, not a wrong value
  5 pairinfo written for chunk0 / kPrepChunk + 1                           9 of 11: "two singles of one key" / "pairs and singles do not add up to the key counts" /
                                                                           "mismatched slots"; test_sizes and test_all_keys fail earlier, at the injection: the loader
                                                                           refuses the pair counts set-up left ("corrupt pair counts"); test_tiers passes (one record
                                                                           per block: no pair either way)
  6 the arena rule of a single dropped (arena = lane parity for all)       8 of 11: "arena rule of a single"; test_tiers and test_one_cell pass (no key with a pair
                                                                           slot and a single in one slice)
  7 compaction: rm.row_of[m][nb] = nb                                      test_migration, test_two_models, test_settled_blocks_keep_their_lists, test_drop_overflow:
                                                                           "row_of", and with it the tiers and every record of the misplaced lists; the 7 tests whose
                                                                           blocks keep their numbers through the compaction (one workgroup, nobody leaves) pass"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
from scipy.spatial import cKDTree

import ckpt_format as cf
import g2p2g_model as gm
import rebuild_books as rb
import rebuild_scenes as rs
from claymore_amd.engine import build_engine
from g2p2g_bench import Bench

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BITS, MAX_PPC = rs.BITS, rs.MAX_PPC
PAIRS = os.environ.get("MPM_G2P2G_PAIRS", "") not in ("0", "0x0")          # the layout this process's library sorts into


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.time()
    yield
    print(f"wall time {request.node.name}: {time.time() - t0:.2f} s")


def books(eng, nmodels):
    """(checkpoint, rows per model, findings) of a context right after a rebuild"""
    assert eng.api.check_table(eng.ctx) == 0
    ck = eng.save_checkpoint().copy()
    rows = [eng.dump_block_rows(m) for m in range(nmodels)]
    cnt = eng.counts()
    found = rb.check_books(ck, rows, eng.cfg.domain_bits, eng.cfg.max_ppc, counts=[int(cnt.particles[m]) for m in range(nmodels)])
    return ck, rows, found


def sort_key_findings(ck, sc, models, parts=None, subset=False):
    """Every record's key field against the model's prediction, the records matched to the model's particles by their new position (nearest
    neighbour, asserted one-to-one and closer than 1e-3 cells).  subset: the context holds fewer particles than the model (dropped ones)."""
    out = []
    parts = sc["parts"] if parts is None else parts
    for m, ((mat, pos), mod) in enumerate(zip(parts, models)):
        r = cf.list_records(ck, m)
        got = cf.record_positions(ck, m, r).astype(np.float64)
        assert r["ok"].all() and (subset or got.shape[0] == pos.shape[0]), (got.shape[0], pos.shape[0])
        d, idx = cKDTree(mod["pos"]).query(got)
        assert d.max(initial=0.0) < 1e-3 and np.unique(idx).size == idx.size, (float(d.max(initial=0.0)), idx.size - np.unique(idx).size)
        dec = rs.decided(mod, sc["tier"], mat)
        left_out = int((~dec).sum())
        wrong = np.flatnonzero((r["key"] != mod["sort_key"][idx]) & dec[idx])
        print(f"{sc['name']} {gm.NAMES[mat]}: {got.shape[0]} records, {left_out} particles on a rounding tie, {wrong.size} keys differ, "
              f"{int((r['tag'] != 13).sum())} records with a neighbour tag, keys in use {np.unique(r['key']).size}")
        if left_out > rs.TIE_CAP * pos.shape[0]:
            out.append(("too many particles on a tie", m, left_out))
        if wrong.size:
            out.append(("sort key", m, wrong.size, wrong[:4].tolist(), r["key"][wrong[:4]].tolist(), mod["sort_key"][idx][wrong[:4]].tolist()))
        tag_wrong = np.flatnonzero(r["tag"] != mod["dirtag"][idx])
        if tag_wrong.size:
            out.append(("direction tag", m, tag_wrong.size, tag_wrong[:4].tolist()))
    return out


def step_and_books(eng, nmodels):
    """mpm_g2p2g(DT, NEW_DT) + mpm_rebuild_partition, then the books - BEFORE any particle readout walks the new lists: (checkpoint, rows,
    findings, counts, particles lost in the step)"""
    lost0 = int(eng.diagnostics().lost_particles)
    eng.g2p2g(gm.DT, gm.NEW_DT)
    cnt = eng.rebuild_partition()
    ck, rows, found = books(eng, nmodels)
    return ck, rows, found, cnt, int(eng.diagnostics().lost_particles) - lost0


def run(sc):
    """One bench, one injection, one g2p2g + rebuild, the books and the sort keys: (checkpoint, rows, models)"""
    bench = Bench(sc["parts"])
    try:
        bench.inject(sc["states"], lambda keys: rs.grid_of(keys, sc["field"]))
        ck, rows, found, cnt, lost = step_and_books(bench.eng, len(sc["parts"]))
        assert not found, found[:10]
        models = rs.model(sc)
        found = sort_key_findings(ck, sc, models)
        h = cf.parse(ck)
        assert all(bool(M["layout"]) == PAIRS for M in h["models"]), "the list layout is not the one this process was asked for"
        print(f"{sc['name']}: blocks {h['pbc']} / {h['nbc']} / {h['ebc']} (previous {h['prev_pbc']} / {h['prev_count']}), lost {lost}, findings {len(found)}")
        assert (cnt.particle_blocks, cnt.neighbor_blocks, cnt.exterior_blocks) == (h["pbc"], h["nbc"], h["ebc"])
        assert lost == 0
        assert not found, found[:10]
        return ck, rows, models
    finally:
        bench.close()


# ---- tiers -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["rest", "flow"])
def test_tiers(tier):
    """One particle per block on isolated sites and at faces, edges and corners of the domain (-1 lanes on up to three sides of a row)."""
    ck, rows, _ = run(rs.scene_tiers(tier))
    h = cf.parse(ck)
    assert h["pbc"] == 26 and (rows[0][:, 27:62] == -1).any()


# ---- sizes and keys -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", [gm.J_FLUID, gm.SAND])
def test_sizes(material):
    """One block per size in {1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 767, 768, 769, 1023, 1024}: the chunk and slice boundaries of both layouts."""
    ck, rows, _ = run(rs.scene_sizes(material))
    h = cf.parse(ck)
    assert sorted(cf.section(ck, h, ("size", 0), np.int32)[:h["pbc"]].tolist()) == sorted(rs.SIZES)


def test_one_cell():
    """Every record of a block carries the same key (513 in one block; 257 + 256 on two keys in another)."""
    ck, rows, _ = run(rs.scene_one_cell())
    assert sorted(np.unique(k).size for k in rb.record_keys(ck, 0).values()) == [1, 2]


def test_all_keys_in_equal_numbers():
    """One block whose records carry each of the 216 keys four times."""
    ck, rows, _ = run(rs.scene_all_keys())
    (keys,) = rb.record_keys(ck, 0).values()
    assert np.array_equal(np.bincount(keys, minlength=216), [4] * 216)


def test_every_key_an_odd_count():
    """One block whose records carry every key 1, 3 or 5 times: 216 singles in 648 records (mismatched slots in the pair layout)."""
    ck, rows, _ = run(rs.scene_odd_keys())
    (keys,) = rb.record_keys(ck, 0).values()
    assert (np.bincount(keys, minlength=216) % 2 == 1).all() and keys.size == 648


# ---- migration -------------------------------------------------------------------------------------------------------------------------------
def test_migration():
    """A block emptied through all 26 of its borders (19 of the receiving blocks were exterior blocks only), two neighbours that swap all their
    particles; nobody is lost."""
    sc = rs.scene_migration()
    ck, rows, models = run(sc)
    h = cf.parse(ck)
    cur = set(map(tuple, cf.cur_keys(ck)[:h["pbc"]].tolist()))
    prev = cf.section(ck, h, "prev_keys", np.int32).reshape(-1, 3)
    prev_tier = {tuple(k): (0 if i < h["prev_pbc"] else 1) for i, k in enumerate(prev.tolist())}
    ring = [tuple(int(v) for v in np.array(rs.BURST) + d) for d in gm.OFFS - 1 if d.any()]
    assert rs.BURST not in cur and all(k in cur for k in ring) and all(prev_tier[k] == 1 for k in ring)
    assert (h["prev_pbc"], h["pbc"]) == (3, 28)
    r = cf.list_records(ck, 0)
    assert (r["tag"] != 13).all() and np.unique(r["tag"]).size == 26


# ---- two models ------------------------------------------------------------------------------------------------------------------------------
def test_two_models():
    """Blocks that hold both models and blocks that hold one of them (size 0, bin offset 0 in the other): the rows of both."""
    ck, rows, _ = run(rs.scene_two_models())
    h = cf.parse(ck)
    s = [cf.section(ck, h, ("size", m), np.int32)[:h["pbc"]] for m in range(2)]
    assert ((s[0] > 0) & (s[1] > 0)).sum() >= 8 and ((s[0] > 0) & (s[1] == 0)).sum() >= 3 and ((s[0] == 0) & (s[1] > 0)).sum() >= 3
    assert np.array_equal(rows[0][:, 27:], rows[1][:, 27:]) and not np.array_equal(rows[0][:, :27], rows[1][:, :27])


# ---- settled blocks ----------------------------------------------------------------------------------------------------------------------------
def test_settled_blocks_keep_their_lists():
    """Step 1 on the cluster (flow tier).  Step 2 under a ZERO field: nobody moves, but every record's key becomes the prediction at rest, which
    differs from the one step 1 made with the flow's velocity for the particles it expected to change cell - so step 2 still sorts (the figure
    is printed).  Step 3 under a zero field finds every block settled (every particle stayed with an unchanged key): prepare_blocks_kernel skips
    the sort and hands the pair counts on under the block's new number.  Books and rows verify after each step; after step 3 every block's record
    key sequence is what it was after step 2, bit for bit, and every position is unchanged."""
    sc = rs.scene_cluster()
    bench = Bench(sc["parts"])
    try:
        bench.inject(sc["states"], lambda keys: rs.grid_of(keys, sc["field"]))
        ck, _, found, _, lost = step_and_books(bench.eng, 1)
        assert not found and lost == 0, found[:10]
        seqs = [rb.record_keys(ck, 0)]
        for step in (2, 3):
            pos = cf.record_positions(ck, 0)
            bench.load(ck, lambda keys: rs.grid_of(keys, rs.zero_field))
            ck, _, found, _, lost = step_and_books(bench.eng, 1)
            st = {k: None for k in ("b6", "reflected", "logjp")}
            st["J"] = np.ones(pos.shape[0], np.float32)
            mod = rs.model(sc, parts=[(gm.J_FLUID, pos)], states=[st], field=rs.zero_field)
            found += sort_key_findings(ck, dict(sc, name=f"cluster, step {step}", tier="rest"), mod, parts=[(gm.J_FLUID, pos)])
            assert not found, (step, found[:10])
            assert lost == 0 and (cf.list_records(ck, 0)["tag"] == 13).all()
            assert np.array_equal(np.sort(cf.record_positions(ck, 0).view(np.uint32), axis=0), np.sort(pos.view(np.uint32), axis=0))
            seqs.append(rb.record_keys(ck, 0))
        changed = sum(not np.array_equal(seqs[0].get(k, ()), v) for k, v in seqs[1].items())
        print(f"blocks whose key sequence changed from step 1 to step 2: {changed} of {len(seqs[1])}")
        assert seqs[1].keys() == seqs[2].keys() and all(np.array_equal(seqs[1][k], seqs[2][k]) for k in seqs[1])
    finally:
        bench.close()


# ---- drop --------------------------------------------------------------------------------------------------------------------------------------
def test_drop_overflow():
    """Two adjacent blocks of 600; one moves wholly into the other under drop_overflow = 1: the destination holds 1024, exactly 176 particles are
    dropped, the emptied block is no particle block any more, and the books verify for what is left."""
    sc = rs.scene_drop()
    (mat, pos), = sc["parts"]
    dx = 0.5 ** BITS
    eng = build_engine({"name": "drop", "bits": BITS, "dt": gm.DT, "config": {"max_ppc": MAX_PPC, "drop_overflow": 1},
                        "models": [{"material": mat, "xyz": pos * np.float32(dx), "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(mat, BITS))}]})
    try:
        eng.initial_setup()
        buf = eng.save_checkpoint().copy()
        g = cf.grid(buf).copy()
        g[:, 1:4] = rs.grid_of(cf.cur_keys(buf)[:g.shape[0]], sc["field"])
        eng.load_checkpoint(cf.with_grid(buf, g))
        d0 = eng.diagnostics()
        eng.g2p2g(gm.DT, gm.NEW_DT)
        cnt = eng.rebuild_partition()
        d1 = eng.diagnostics()
        ck, rows, found = books(eng, 1)
        h = cf.parse(ck)
        print("dropped", d1.dropped_particles - d0.dropped_particles, "lost", d1.lost_particles - d0.lost_particles, "particles", int(cnt.particles[0]))
        assert d1.dropped_particles - d0.dropped_particles == 176 and d1.lost_particles == d0.lost_particles
        assert h["pbc"] == 1 and tuple(cf.cur_keys(ck)[0].tolist()) == rs.DROP[1]
        assert int(cf.section(ck, h, ("size", 0), np.int32)[0]) == 1024 == int(cnt.particles[0])
        assert not found, found[:10]
        found = sort_key_findings(ck, sc, rs.model(sc), subset=True)
        assert not found, found[:10]
    finally:
        eng.close()


# ---- the still path ------------------------------------------------------------------------------------------------------------------------------
def test_still_rebuild_rows():
    """The two-model scene at rest without gravity (undeformed material: nobody moves), three substeps of mpm_run_fixed one by one: a full rebuild,
    a still rebuild (rows derived from the rows that stand: lane l < 27 from lane 53 - l) and a second still rebuild in a row (settled blocks are
    passed over).  The books are verified after each - before the next G2P2G reads the rows."""
    sc = rs.scene_two_models()
    dx = 0.5 ** BITS
    eng = build_engine({"name": "at_rest", "bits": BITS, "dt": gm.DT, "config": {"max_ppc": MAX_PPC, "gravity": 0.0},
                        "models": [{"material": m, "xyz": p * np.float32(dx), "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(m, BITS))} for m, p in sc["parts"]]})
    try:
        eng.initial_setup()
        for step, want_still in ((1, 0), (2, 1), (3, 2)):
            eng.run_fixed(1, gm.DT)
            assert int(eng.diagnostics().still_rebuilds) == want_still, (step, int(eng.diagnostics().still_rebuilds))
            ck, rows, found = books(eng, 2)
            assert not found, (step, found[:10])
            for m, (_, p) in enumerate(sc["parts"]):
                assert np.array_equal(np.sort(cf.record_positions(ck, m).view(np.uint32), axis=0), np.sort(p.view(np.uint32), axis=0)), "somebody moved"
    finally:
        eng.close()


# ---- stale launches ----------------------------------------------------------------------------------------------------------------------------
def test_stale_launches():
    """One window of mpm_run_fixed (sync_interval 64, 64 substeps, bits 8) in which the block counts outgrow what the window's launches were sized
    for, so that the rebuild kernels take further trips through their loops: a ball of 40 000 J-fluid particles (no stiffness to speak of, no
    gravity) of radius 10.6 cells, given the velocity field v = k (x - c), k = 300 / s, through the grid of its set-up checkpoint - every particle
    then flies on at its own velocity, the ball grows by 3 % of its first radius per substep and thins out to ~20 particles per block.

    Launch sizes of the window, from the counts (P0, N0, E0) of the synchronisation before it (claymore_hip.hip: launch_rebuild, launch_prepare,
    hint_blocks), E' = E0 + E0 / 16 + 1024:
      compact_blocks_kernel        ceil(E' / 1024) workgroups of 1024: a second trip when the old exterior count exceeds  1024 ceil(E' / 1024)
      register_blocks_kernel<0,1>  ceil(8 E' / 256) workgroups, 8 lanes per block:  when the particle block count exceeds   32 ceil(8 E' / 256)
      register_blocks_kernel<-1,1> ceil(32 E' / 256) workgroups, 32 lanes per block: when it exceeds                          8 ceil(32 E' / 256)
      prepare_blocks_kernel        E' + E' / 16 + 64 workgroups, one per block:      when it exceeds that
      G2P2G (hint_blocks)          P0 + P0 / 16 + 64 rounded up to 8, one per block: when it exceeds that
    All five are asserted crossed, from mpm_get_counts before and after the window (the counts grow monotonically, by under 3 % per substep at the
    end: a threshold passed by 10 % at the end was passed several substeps before it, and the compaction reads the count of the substep before).
    NOT crossed: carry_grid_kernel (2048 workgroups x 4 blocks: a second trip needs more than 8192 neighbour blocks) - the block capacity set-up
    gives this scene is E0 3 / 2 + 4096 = 4736, and a context whose exterior count passes its capacity inside a window ends the run with
    MPM_ERR_CAPACITY; a scene that starts above 8192 neighbour blocks has E' > 9700 and its register / prepare launches then cover a growth of
    1024 blocks and more, which 64 substeps below the CFL limit do not produce from a body that size within a few seconds of test time.  The same
    holds for the caps of the register launches (4096 and 8192 workgroups: 131 072 and 65 536 particle blocks).

    Afterwards: nobody lost, the table consistent, and check_books over everything the last rebuild of the window wrote (not the sort keys: the
    model does not follow 64 substeps)."""
    bits, n, r0, k = 8, 40000, 10.6, 300.0
    dx = 0.5 ** bits
    rng = np.random.default_rng(31)
    c = np.array([128.3, 127.1, 128.6])
    u = rng.normal(size=(n, 3))
    pos = (c + u / np.linalg.norm(u, axis=1)[:, None] * r0 * rng.random(n)[:, None] ** (1.0 / 3.0)).astype(np.float32)
    vol = float(np.float32(dx ** 3 / 8.0))
    eng = build_engine({"name": "burst", "bits": bits, "dt": gm.DT, "config": {"max_ppc": MAX_PPC, "gravity": 0.0, "sync_interval": 64},
                        "models": [{"material": gm.J_FLUID, "xyz": pos * np.float32(dx), "v0": (0.0, 0.0, 0.0),
                                    "params": dict(rho=1e3, volume=vol, bulk=1e-3, gamma=7.15, viscosity=0.0)}]})
    try:
        eng.initial_setup()
        buf = eng.save_checkpoint().copy()
        g = cf.grid(buf).copy()
        keys = cf.cur_keys(buf)[:g.shape[0]].astype(np.int64)
        cell = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)])
        v = (k * dx * ((4 * keys[:, None, :] + cell[None, :, :]) - c[None, None, :])).astype(np.float32)          # (nbc, 64, 3) m/s
        g[:, 1:4] = g[:, 0:1] * v.transpose(0, 2, 1)                                                                   # momenta: the run starts with a grid update
        eng.load_checkpoint(cf.with_grid(buf, g))
        c0 = eng.counts()
        P0, E0 = int(c0.particle_blocks), int(c0.exterior_blocks)
        cap = eng.capacity()[0]
        Ee = min(cap, E0 + E0 // 16 + 1024)
        cdiv = lambda a, b: -(-a // b)
        limits = {"compact_blocks_kernel (old exterior blocks)": 1024 * cdiv(Ee, 1024), "register_blocks_kernel<0,1>": 32 * min(4096, cdiv(8 * Ee, 256)),
                  "register_blocks_kernel<-1,1>": 8 * min(8192, cdiv(32 * Ee, 256)), "prepare_blocks_kernel": min(cap, Ee + Ee // 16 + 64),
                  "G2P2G": (min(P0 + P0 // 16 + 64, max(cap, 8)) + 7) & ~7}
        eng.run_fixed(64, gm.DT)
        c1 = eng.counts()
        d = eng.diagnostics()
        P1, E1 = int(c1.particle_blocks), int(c1.exterior_blocks)
        print(f"stale launches: blocks {P0} / {int(c0.neighbor_blocks)} / {E0} -> {P1} / {int(c1.neighbor_blocks)} / {E1}, capacity {cap}, limits {limits}")
        assert eng.capacity()[0] == cap or E1 * 4 > cap * 3, "the capacity grew inside the window"
        for name, lim in limits.items():
            have = E1 if name.startswith("compact") else P1
            assert have > 1.1 * lim, (name, have, lim)
        assert d.lost_particles == 0 and d.dropped_particles == 0 and int(c1.particles[0]) == n
        ck, rows, found = books(eng, 1)
        assert not found, found[:10]
    finally:
        eng.close()


# ---- the other layout --------------------------------------------------------------------------------------------------------------------------
def test_the_sliced_layout_passes_too():
    """Everything above ran with the default mask (pair layout).  This test runs the file again in a fresh child process with MPM_G2P2G_PAIRS=0 -
    the one-particle-per-lane kernel, the sliced list layout and its sort - under a time limit, deselecting itself and the window test there."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not test_the_sliced_layout_passes_too and not test_stale_launches"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

"""All eight model slots on the GPU (kMaxModels = 8: CkptHeader::models[8], mpm_counts::particles[8], the eight status words behind each of ST_BINS0,
ST_PART0 and ST_BINSPREV, PrepareModels / RebuildModels / ClearArgs, the threadIdx.x < kMaxModels lanes): the scenes of tests/model_slot_scenes.py
put particles into slots 4 .. 7, empty models into slots 0, 3 and 7, leave model 0 out of occupied blocks, and - in the child processes of
test_mixed_layouts_in_child_processes - give the models of one context different list layouts (MPM_G2P2G_PAIRS = 0x5, 0xA; 0 for the sliced
layout alone).  The tools are the existing ones: the injection bench (tests/g2p2g_bench.py), check() of tests/test_g2p2g_blocks_gpu.py, check_books
(tests/rebuild_books.py) with books() and sort_key_findings() of tests/test_rebuild_books_gpu.py, run_pair / match_and_compare for the pipeline.
Every bound is one the project has: g2p2g_model.bound, rebuild_scenes.TIE_CAP / tie_margin, POS_TOL, and the readout bound of
tests/test_particle_velocity_gpu.py.  tests/test_model_slots_cpu.py licenses the scenes and shows check() rejecting faults in the high slots.

mpm_particle_momentum and mpm_stress_totals document model -1 as "all models": test_per_model_calls_refuse_a_model_that_is_not_there asks them
for model -2 instead, every other call for -1, all of them for 8.

A context that has just loaded a checkpoint holds block b's list in row b (unpack_lists_kernel writes row_of[b] = b): the checkpoint test tells
check_books so (loaded=True), everything else it checks as after a rebuild.

Wall time on an MI355X (every test prints its own): the 22 in-process tests take 2.6 s together - none more than 0.7 s: the first injected step
(with the scene's generation), the two pipeline runs with their oracle - and the file 6 s with its imports; each of the three child processes
runs those 22 tests once more in 6 to 8 s: 30 s in all.

Kernel mutations (value-only): not run - read closely, none of the three examples is value-only for the calls this file makes.  Expected from reading:
  ST_PART0 + (threadIdx.x & 3) in the compaction's total          counts.particles[4 .. 7] read 0 and slots 0 .. 3 hold the sums: test_one_injected_step (eight), at check()'s
                                                                  particle count.  Not run: M.bucketed is read back from those words and sizes the packed list buffer of
                                                                  mpm_checkpoint_save, which pack_lists_kernel then fills by the blocks' sizes - past its end for slots 4 .. 7
  keep0 used for every m in prepare_blocks_kernel                 a block settled for model 0 skips the sort of the others: test_books_of_all_eight_rows (flow), the layout
                                                                  findings and the sort keys of slots 1 .. 7.  Not run: stale pair counts then shape G2P2G's iterations
  pm.pairinfo[0] deciding the layout for all models               the child processes with masks 0x5 and 0xA: test_books_of_all_eight_rows, "pair slot of two keys" or
                                                                  "sliced layout: keys not in key-major order" for the models whose layout differs from model 0's.  Not run:
                                                                  with model 0 in the pair layout the sort would write pair counts through another model's null pairinfo"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ckpt_format as cf
import g2p2g_model as gm
import model_slot_scenes as ms
import rebuild_books as rb
import rebuild_scenes as rs
from claymore_amd import _ffi, scenes
from claymore_amd.engine import EngineError, build_engine
from g2p2g_bench import Bench, by_position_bits
from parity_util import match_and_compare, run_pair
from test_g2p2g_blocks_gpu import check
from test_parity_gpu import POS_TOL
from test_particle_ids_gpu import IdBench
from test_particle_velocity_gpu import gather64, node_velocities
from test_rebuild_books_gpu import books, sort_key_findings

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BITS, MAX_PPC, N = ms.BITS, ms.MAX_PPC, ms.NSLOTS
_MASK = os.environ.get("MPM_G2P2G_PAIRS", "")
PAIR_MASK = (int(_MASK, 0) if _MASK else 0xF) & 0xF                    # the per-material mask this process's library reads (claymore_hip.hip: pair_mask)
CASES = [(name, tier) for name in ms.NAMES for tier in ms.TIERS]


def layout_of(material):
    return (PAIR_MASK >> material) & 1


@pytest.fixture(autouse=True)
def wall_time(request):
    t0 = time.time()
    yield
    print(f"wall time {request.node.name}: {time.time() - t0:.2f} s")


def grid_injector(sc):
    return lambda keys: rs.grid_of(keys, sc["field"])


def step_with_books(bench):
    """mpm_g2p2g + mpm_rebuild_partition on an injected bench; the books first (before any readout walks the new lists), then what Bench.step returns."""
    eng = bench.eng
    d0 = eng.diagnostics()
    eng.g2p2g(gm.DT, gm.NEW_DT)
    cnt = eng.rebuild_partition()
    ck, rows, found = books(eng, len(bench.parts))
    d1 = eng.diagnostics()
    res = dict(counts=cnt, lost=int(d1.lost_particles) - int(d0.lost_particles), discarded=int(d1.discarded_p2g) - int(d0.discarded_p2g), grid=eng.dump_grid(),
               state=[bench.read(i) for i in range(len(bench.parts))])
    return res, ck, rows, found


_STEPPED = {}


def stepped(name, tier):
    """One bench, one injection, one step of scene `name` on `tier`, shared by the tests that look at it: {scene, parts, res, ck, rows, found, models}"""
    if (name, tier) not in _STEPPED:
        sc = ms.scene(name, tier)
        bench = Bench(sc["parts"])
        try:
            bench.inject(sc["states"], grid_injector(sc))
            res, ck, rows, found = step_with_books(bench)
            _STEPPED[name, tier] = dict(scene=sc, parts=bench.parts, res=res, ck=ck, rows=rows, found=found, models=ms.models(sc))
        finally:
            bench.close()
    return _STEPPED[name, tier]


def bins_of(pos_cells):
    """Bins a model needs for the particles at pos_cells: ceil(size / 64) summed over its blocks"""
    if pos_cells.shape[0] == 0:
        return 0
    _, c = np.unique(gm.block_keys(pos_cells), axis=0, return_counts=True)
    return int(((c + cf.K_BIN - 1) // cf.K_BIN).sum())


def check_counts(cnt, parts, state):
    assert cnt.model_count == N
    for m, (_, p) in enumerate(parts):
        assert int(cnt.particles[m]) == p.shape[0], ("counts.particles", m, int(cnt.particles[m]), p.shape[0])
        assert int(cnt.bins[m]) == bins_of(state[m]["pos"]), ("counts.bins", m, int(cnt.bins[m]), bins_of(state[m]["pos"]))
        if p.shape[0] == 0:
            assert int(cnt.particles[m]) == 0 and int(cnt.bins[m]) == 0 and state[m]["pos"].shape[0] == 0


class View:
    """What check() reads of a bench"""

    def __init__(self, parts):
        self.parts, self.bits = parts, BITS


# ---- 1. one injected step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tier", CASES)
def test_one_injected_step(name, tier):
    """Inject, one mpm_g2p2g + mpm_rebuild_partition, check(): every model's particles, the shared grid node by node, total mass, lost, discarded;
    and the eight count words."""
    s = stepped(name, tier)
    check(View(s["parts"]), s["res"], s["models"], tier, name)
    check_counts(s["res"]["counts"], s["parts"], s["res"]["state"])
    assert s["res"]["lost"] == 0


# ---- 2. the books -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tier", CASES)
def test_books_of_all_eight_rows(name, tier):
    """check_books, the sort keys and mpm_check_table (books()) on the same steps, over all eight models; lanes 27 .. 63 of the rows are the same
    for every model; size and bin offset are 0 wherever a model is absent from a block; every model's layout word is the mask bit of its material."""
    s = stepped(name, tier)
    ck, rows = s["ck"], s["rows"]
    assert not s["found"], s["found"][:10]
    found = sort_key_findings(ck, s["scene"], s["models"])
    assert not found, found[:10]
    h = cf.parse(ck)
    assert h["nmodels"] == N and len(rows) == N
    for m, (mat, p) in enumerate(s["parts"]):
        M = h["models"][m]
        assert M["material"] == mat and bool(M["layout"]) == bool(layout_of(mat)), ("layout word", m, M, PAIR_MASK)
        assert h["sections"]["pairinfo", m][1] == (4 * h["pbc"] * cf.K_PAIR_CHUNKS if layout_of(mat) else 0)
        assert rows[m].shape == (h["pbc"], 64) and np.array_equal(rows[m][:, 27:], rows[0][:, 27:]), ("lanes 27 .. 63 differ between models", m)
        size = cf.section(ck, h, ("size", m), np.int32)[:h["pbc"]]
        bdst = cf.section(ck, h, ("binoff_dst", m), np.int32)[:h["pbc"]]
        have = set(map(tuple, gm.block_keys(s["res"]["state"][m]["pos"]).tolist()))
        absent = np.array([tuple(k) not in have for k in cf.cur_keys(ck)[:h["pbc"]].tolist()], bool)
        assert (size[absent] == 0).all() and (bdst[absent] == 0).all() and (size[~absent] > 0).all(), ("size / bin offset of absent blocks", m)
        assert int(size.sum()) == p.shape[0] == M["bucketed"] == M["n"]
    if name == "eight":
        sz = np.stack([cf.section(ck, h, ("size", m), np.int32)[:h["pbc"]] for m in range(N)])
        assert ((sz > 0).sum(axis=0) >= 3).sum() >= 8 and (sz[0] == 0).sum() >= 3 and all(((sz[m] > 0) & (np.delete(sz, m, axis=0) == 0).all(axis=0)).any() for m in range(N))


# ---- 3. the still path with slot 0 absent -------------------------------------------------------------------------------------------------------------
def sorted_state(eng, m):
    x, st, lj = eng.retrieve_state(m)
    o = by_position_bits(x)
    return np.concatenate([np.ascontiguousarray(a[o], np.float32).view(np.uint32) for a in (x, st, lj[:, None])], axis=1)


@pytest.mark.parametrize("name", ["holes", "eight"])
def test_still_path_with_slot_0_absent(name):
    """The scene's positions at rest without gravity (undeformed material, a zero velocity field: nobody moves), four substeps of mpm_run_fixed one by
    one: a full rebuild, then still rebuilds in streaks of 1 (rows mirrored from the standing row, read from blockinfo[0] for all models), 2 and 3
    (prepare_blocks_kernel's skip path) - with model 0 empty (`holes`) or absent from seven occupied blocks (`eight`).  The books verify after each,
    and every model's readout - positions with their state rows - comes back bit for bit from the step before.  Stillness needs undeformed
    material, so all particles of a model carry the SAME state (b = I, one log Jp, J = 1): the comparison sees a particle that moved, went
    missing or came back with a damaged row, not states exchanged between two particles of one model (the injected steps, whose states are
    all different, see those)."""
    sc = ms.scene(name, "rest")
    dx = 0.5 ** BITS
    eng = build_engine({"name": "slots_at_rest", "bits": BITS, "dt": gm.DT, "config": {"max_ppc": MAX_PPC, "gravity": 0.0},
                        "models": [{"material": m, "xyz": p * np.float32(dx), "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(m, BITS))} for m, p in sc["parts"]]})
    try:
        eng.initial_setup()
        before = [sorted_state(eng, m) for m in range(N)]
        for step, want_still in ((1, 0), (2, 1), (3, 2), (4, 3)):
            eng.run_fixed(1, gm.DT)
            assert int(eng.diagnostics().still_rebuilds) == want_still, (step, int(eng.diagnostics().still_rebuilds))
            ck, rows, found = books(eng, N)
            assert not found, (step, found[:10])
            cnt = eng.counts()
            assert cnt.model_count == N and [int(cnt.particles[m]) for m in range(N)] == [p.shape[0] for _, p in sc["parts"]]
            h = cf.parse(ck)
            for m, (mat, p) in enumerate(sc["parts"]):
                assert bool(h["models"][m]["layout"]) == bool(layout_of(mat))
                assert np.array_equal(rows[m][:, 27:], rows[0][:, 27:])
                assert np.array_equal(np.sort(cf.record_positions(ck, m).view(np.uint32), axis=0), np.sort(p.view(np.uint32), axis=0)), ("somebody moved", step, m)
                now = sorted_state(eng, m)
                assert np.array_equal(now, before[m]), ("the state changed in a substep at rest", step, m, int((now != before[m]).any(axis=1).sum()))
                before[m] = now
        d = eng.diagnostics()
        assert d.lost_particles == 0 and d.dropped_particles == 0
    finally:
        eng.close()


# ---- 4. mixed layouts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["0x5", "0xA", "0"])
def test_mixed_layouts_in_child_processes(mask):
    """Everything else in this file runs in process with the mask the process was given (default: all four materials in the pair layout).  This test
    runs the file once more in a fresh child process per mask - 0x5: J-fluid and sand in the pair layout, fixed-corotated and NACC sliced; 0xA: the
    other way round; 0: all sliced - under a time limit, deselecting itself there.  A child that ends on a signal or at its time limit fails the
    test, and nothing is tried again."""
    env = dict(os.environ, MPM_G2P2G_PAIRS=mask)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not test_mixed_layouts_in_child_processes"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", mask, r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail and "skipped" not in tail, (mask, r.returncode, tail, r.stderr[-1500:])


# ---- 5. a checkpoint in a mixed context ---------------------------------------------------------------------------------------------------------------
def check_ids(eng, parts, rows_of_id, predicted, tier, tag):
    """Ids of slot m are a permutation of 0 .. n_m - 1, and the particle that carries id i is where the model puts the particle that carried it before
    the step: predicted[m][rows_of_id[m][i]] (cells), inside the position bound."""
    for m, (mat, p) in enumerate(parts):
        xyz, ids = eng.retrieve_ids(m)
        assert ids.shape == (p.shape[0],) and np.array_equal(np.sort(ids), np.arange(p.shape[0])), (tag, m, "the ids are no permutation of 0 .. n - 1")
        if p.shape[0] == 0:
            continue
        got = xyz.astype(np.float64) * 2.0 ** BITS
        e = gm.err_pos(got, predicted[m][rows_of_id[m][ids]])
        print(f"{tag} slot {m} {gm.NAMES[mat]}: {ids.size} ids, worst position error by id {float(e.max()):.3g} (bound {gm.bound('pos', tier, mat):.3g})")
        assert e.max() <= gm.bound("pos", tier, mat), (tag, m, float(e.max()))


def id_pairs(eng, m):
    xyz, ids = eng.retrieve_ids(m)
    o = by_position_bits(xyz)
    return np.concatenate([xyz[o].view(np.uint32), ids[o].view(np.uint32)[:, None]], axis=1)


@pytest.mark.parametrize("name", ["eight", "holes"])
def test_checkpoint_in_a_mixed_context(name):
    """A tracked context: inject, one step, check(); the checkpoint and the ids blob saved there and loaded into a FRESH eight-model context: its books
    are clean, mpm_retrieve_state and mpm_retrieve_ids of every slot return what the saving context returns, bit for bit, and a second injected
    step - a new field, the model fed the state read back - passes check().  Through both steps the ids follow their particles."""
    tier = "flow"
    sc = ms.scene(name, tier)
    a = IdBench(sc["parts"])
    b = None
    try:
        a.inject(sc["states"], grid_injector(sc))
        a.eng.load_particle_ids(a.ids0)
        res1 = a.step()
        models1 = ms.models(sc)
        check(a, res1, models1, tier, name + ", step 1")
        check_counts(res1["counts"], a.parts, res1["state"])
        check_ids(a.eng, a.parts, [np.arange(p.shape[0]) for _, p in a.parts], [m["pos"] for m in models1], tier, name + ", step 1")
        ck, blob = a.eng.save_checkpoint().copy(), a.eng.save_particle_ids().copy()
        h = cf.parse(ck)
        assert [bool(M["layout"]) for M in h["models"]] == [bool(layout_of(m)) for m in ms.MATERIALS]
        want_state = [sorted_state(a.eng, m) for m in range(N)]
        want_ids = [id_pairs(a.eng, m) for m in range(N)]
        b = IdBench(sc["parts"])
        b.eng.load_checkpoint(ck)
        b.eng.load_particle_ids(blob)
        assert b.eng.api.check_table(b.eng.ctx) == 0                # (books() of test_rebuild_books_gpu.py, with check_books told that this is a loaded state)
        cnt = b.eng.counts()
        found = rb.check_books(b.eng.save_checkpoint().copy(), [b.eng.dump_block_rows(m) for m in range(N)], BITS, MAX_PPC, counts=[int(cnt.particles[m]) for m in range(N)], loaded=True)
        assert not found, found[:10]
        for m in range(N):
            assert np.array_equal(sorted_state(b.eng, m), want_state[m]), ("retrieve_state after the load", m)
            assert np.array_equal(id_pairs(b.eng, m), want_ids[m]), ("retrieve_ids after the load", m)
        # step 2: the first field seed under which no particle of the state READ BACK sits on the brink of a branch (test_second_substep)
        back = res1["state"]
        parts2 = [(mat, back[m]["pos"]) for m, (mat, _) in enumerate(sc["parts"])]
        states2 = [dict(b6=None if mat == gm.J_FLUID else back[m]["b6"], reflected=None if mat == gm.J_FLUID else back[m]["reflected"],
                        logjp=back[m]["logjp"] if mat in (gm.SAND, gm.NACC) else None, J=back[m]["J"] if mat == gm.J_FLUID else None) for m, (mat, _) in enumerate(sc["parts"])]
        for seed in range(1, 65):
            sc2 = dict(sc, field=rs.tier_field(tier, seed))
            models2 = ms.models(sc2, parts=parts2, states=states2)
            if not any(m["unstable"].any() for m in models2):
                break
        print("field of step 2: seed", seed)
        assert not any(m["unstable"].any() for m in models2)
        b.load(ck, grid_injector(sc2))
        b.eng.load_particle_ids(blob)
        rows_of_id = []
        for m, (_, p1) in enumerate(parts2):                       # which row of the read-back state carries which id
            xyz, ids = b.eng.retrieve_ids(m)
            og, ow = by_position_bits(xyz), by_position_bits(p1 * np.float32(0.5 ** BITS))
            assert np.array_equal(xyz[og].view(np.uint32), (p1 * np.float32(0.5 ** BITS))[ow].view(np.uint32))
            r = np.empty(p1.shape[0], np.int64)
            r[ids[og]] = ow
            rows_of_id.append(r)
        b.parts = parts2
        res2, _, _, found = step_with_books(b)                       # (a rebuild has run: the ordinary row_of rule holds again)
        assert not found, found[:10]
        check(b, res2, models2, tier, name + ", step 2")
        check_counts(res2["counts"], parts2, res2["state"])
        check_ids(b.eng, parts2, rows_of_id, [m["pos"] for m in models2], tier, name + ", step 2")
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- 6. readouts on every slot -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eight", "holes"])
def test_readouts_on_every_slot(name):
    """After an injected step (flow tier; the grid holds the P2G's momenta): mpm_retrieve_velocity of every slot against the float64 gather of the
    context's own grid (the bound of test_against_a_float64_gather_of_the_own_grid), mpm_retrieve_stress and mpm_retrieve_positions with n_m rows
    whose position bits are those of mpm_retrieve_state, the totals' counts; an empty slot returns 0 rows and MPM_OK."""
    sc = ms.scene(name, "flow")
    bench = Bench(sc["parts"])
    try:
        bench.inject(sc["states"], grid_injector(sc))
        bench.eng.g2p2g(gm.DT, gm.NEW_DT)
        bench.eng.rebuild_partition()
        eng = bench.eng
        V = node_velocities(*eng.dump_grid(), BITS)
        out, ref = [], []
        for m, (mat, p) in enumerate(sc["parts"]):
            n = p.shape[0]
            xs = eng.retrieve_state(m)[0]
            xv, v, Cm = eng.retrieve_velocity(m, affine=True)
            xq, s6, s3 = eng.retrieve_stress(m)
            xp = eng.retrieve_positions(m)
            assert xs.shape == xv.shape == xq.shape == xp.shape == v.shape == (n, 3) and Cm.shape == (n, 3, 3) and s6.shape == (n, 6) and s3.shape == (n, 3), (m, n)
            want = xs[by_position_bits(xs)].view(np.uint32)
            for got in (xv, xq, xp):
                assert np.array_equal(got[by_position_bits(got)].view(np.uint32), want), ("position bits of a readout", m)
            assert np.isfinite(s6).all() and np.isfinite(s3).all() and np.isfinite(v).all() and np.isfinite(Cm).all()
            assert eng.particle_momentum(m)["count"] == n and eng.stress_totals(m)["count"] == n
            out.append((v, Cm))
            ref.append(gather64(xv, V, BITS) if n else (np.zeros((0, 3)), np.zeros((0, 3, 3))))
        vmax, cmax = max(np.abs(r[0]).max(initial=0.0) for r in ref), max(np.abs(r[1]).max(initial=0.0) for r in ref)
        assert vmax > 1.0 and cmax > 0.0
        for m, ((v, Cm), (vr, cr)) in enumerate(zip(out, ref)):
            dv, dc = np.abs(v - vr).max(initial=0.0), np.abs(Cm - cr).max(initial=0.0)
            print(f"{name} slot {m}: {v.shape[0]} rows, max |dv| {dv:.3g} of max |v| {vmax:.3g}, max |dC| {dc:.3g} of max |C| {cmax:.3g}")
            assert dv <= 2e-6 * vmax and dc <= 2e-6 * cmax, (m, dv, vmax, dc, cmax)
        assert eng.particle_momentum()["count"] == eng.stress_totals()["count"] == sum(p.shape[0] for _, p in sc["parts"])
    finally:
        bench.close()


# ---- 7. pipeline parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eight", "holes"])
def test_pipeline_parity_on_eight_models(name):
    """The pipeline forms through mpm_run_fixed (windows, fused carry-over) and the oracle: 60 substeps, positions inside POS_TOL, the eight count
    words equal.  The oracle takes the empty models as they are; match_and_compare is given the occupied slots (an empty set has no nearest
    neighbour), after both sides were seen to return no row for the empty ones."""
    sc = ms.pipeline(name)
    res = run_pair(sc, ms.PIPELINE_STEPS, ms.PIPELINE_DT)
    n = [m["xyz"].shape[0] for m in sc["models"]]
    ch, co = res["hip"]["counts"], res["oracle"]["counts"]
    assert ch.model_count == co.model_count == N
    assert [int(ch.particles[i]) for i in range(N)] == [int(co.particles[i]) for i in range(N)] == n
    for side in ("hip", "oracle"):
        assert [s[0].shape[0] for s in res[side]["state"]] == n
    occ = [i for i in range(N) if n[i]]
    assert tuple(occ) == ms.occupied(name)
    part = {side: dict(res[side], state=[res[side]["state"][i] for i in occ]) for side in ("hip", "oracle")}
    err = match_and_compare(part)
    print(name, err)
    assert err["n"] == sum(n) and err["pos_rel"] < POS_TOL, err
    d = res["hip"]["diag"]
    assert d.lost_particles == 0 and d.dropped_particles == 0


# ---- 8. limits -----------------------------------------------------------------------------------------------------------------------------------------
class NinthBench(Bench):
    """The injection bench on a context that was asked for a ninth model, both ways, before set-up."""

    def __init__(self, parts):
        self.bits, self.dx = BITS, 0.5 ** BITS
        self.parts = [(m, np.ascontiguousarray(p, np.float32)) for m, p in parts]
        self.over = [gm.material_overrides(m, BITS) for m, _ in self.parts]
        sc = {"name": "ninth", "bits": BITS, "dt": gm.DT, "config": {"max_ppc": MAX_PPC},
              "models": [{"material": m, "xyz": p * np.float32(self.dx), "v0": (0.0, 0.0, 0.0), "params": dict(o)} for (m, p), o in zip(self.parts, self.over)]}
        self.eng = build_engine(sc)
        self.refused = []
        extra = self.parts[0][1][:5] * np.float32(self.dx)
        for add in (lambda: self.eng.init_model(gm.FC, extra, **gm.material_overrides(gm.FC, BITS)),
                    lambda: self.eng.init_model_mesh(gm.FC, *scenes.box_mesh((0.4, 0.4, 0.4), (0.5, 0.5, 0.5)), **gm.material_overrides(gm.FC, BITS))):
            with pytest.raises(EngineError) as e:
                add()
            self.refused.append(e.value.code)
        self.eng.initial_setup()
        self.ckpt = self.eng.save_checkpoint().copy()
        self.consts = [gm.constants(m, o) for (m, _), o in zip(self.parts, self.over)]


def test_a_ninth_model_is_refused_and_the_context_lives_on():
    """A ninth mpm_add_model and a ninth mpm_add_model_mesh return MPM_ERR_CAPACITY; the context then sets up with its eight and passes test 1."""
    sc = ms.scene("eight", "flow")
    bench = NinthBench(sc["parts"])
    try:
        assert bench.refused == [_ffi.MPM_ERR_CAPACITY, _ffi.MPM_ERR_CAPACITY] and len(bench.eng.models) == N
        assert bench.eng.counts().model_count == N
        bench.inject(sc["states"], grid_injector(sc))
        res = bench.step()
        check(bench, res, ms.models(sc), "flow", "eight, after a refused ninth")
        check_counts(res["counts"], bench.parts, res["state"])
    finally:
        bench.close()


def test_per_model_calls_refuse_a_model_that_is_not_there():
    """Every per-model call - mpm_retrieve_positions / _state / _velocity / _stress / _ids, mpm_dump_block_rows, mpm_particle_momentum,
    mpm_stress_totals - refuses model 8, model 108 and model -1 (the two totals, for which -1 means all models: -2) with MPM_ERR_INVALID, the code
    include/claymore_amd.h documents for a bad model, and writes nothing: the caller's arrays keep their canaries and *n its value.  The context
    tracks ids and they are valid (set-up, no load since), so mpm_retrieve_ids refuses for the model alone; for model 1 every call works and writes."""
    sc = ms.scene("holes", "rest")
    bench = IdBench(sc["parts"])
    try:
        eng = bench.eng
        api, ctx = eng.api, eng.ctx
        cap = 1024

        def canary(*shape):
            return np.full(shape, np.float32(-77.25), np.float32)

        def arrays_and_call(which, model):
            n = C.c_size_t(cap)
            if which == "retrieve_positions":
                arrs = [canary(cap, 3)]
                rc = api.retrieve_positions(ctx, model, arrs[0].ctypes.data, C.byref(n))
            elif which == "retrieve_state":
                arrs = [canary(cap, 3), canary(cap, 9), canary(cap)]
                rc = api.retrieve_state(ctx, model, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, C.byref(n))
            elif which == "retrieve_velocity":
                arrs = [canary(cap, 3), canary(cap, 3), canary(cap, 9)]
                rc = api.retrieve_velocity(ctx, model, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, C.byref(n))
            elif which == "retrieve_stress":
                arrs = [canary(cap, 3), canary(cap, 6), canary(cap, 3)]
                rc = api.retrieve_stress(ctx, model, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, C.byref(n))
            elif which == "retrieve_ids":
                arrs = [canary(cap, 3), np.full(cap, -77, np.int32)]
                rc = api.retrieve_ids(ctx, model, arrs[0].ctypes.data, arrs[1].ctypes.data, C.byref(n))
            elif which == "dump_block_rows":
                arrs = [np.full((cap, 64), -77, np.int32)]
                rc = api.dump_block_rows(ctx, model, arrs[0].ctypes.data, C.byref(n))
            else:
                out = (C.c_double * 8)(*([-77.25] * 8))
                rc = getattr(api, which)(ctx, model, out)
                arrs = [np.array(out[:])]
            return rc, arrs, n.value
        for which in ("retrieve_positions", "retrieve_state", "retrieve_velocity", "retrieve_stress", "retrieve_ids", "dump_block_rows", "particle_momentum", "stress_totals"):
            rc, clean, _ = arrays_and_call(which, 1)                                     # (a model that is there: the call works, and writes every array)
            assert rc == _ffi.MPM_OK and all((a != -77.25).any() if a.dtype != np.int32 else (a != -77).any() for a in clean), which
            for model in (N, -2 if which in ("particle_momentum", "stress_totals") else -1, N + 100):
                rc, arrs, n = arrays_and_call(which, model)
                assert rc == _ffi.MPM_ERR_INVALID, (which, model, rc)
                assert all((a == (-77 if a.dtype == np.int32 else -77.25)).all() for a in arrs), (which, model, "the call wrote to the caller's arrays")
                assert n == cap, (which, model, n)
        # the context is none the worse for it
        assert eng.retrieve_state(1)[0].shape[0] == sc["parts"][1][1].shape[0] and eng.retrieve_state(0)[0].shape[0] == 0
    finally:
        bench.close()

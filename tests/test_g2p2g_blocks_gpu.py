"""The fused G2P2G kernels (claymore_amd/csrc/mpm_g2p2g.hpp, mpm_g2p2g_pair.hpp) block by block: ONE substep of the real kernels on known,
deformed particle state in populated blocks, against the float64 model of tests/g2p2g_model.py (which tests/test_g2p2g_model_cpu.py judges
against the oracle and the golden rows).  The injection port is the checkpoint: mpm_checkpoint_load copies the bins and the grid verbatim, so a
checkpoint saved after set-up with the state slots of its particles (tests/ckpt_format.with_particle_state: positions untouched, so lists, sizes
and pair counts stay valid) and the velocity channels of its grid (with_grid) overwritten puts every particle of every block into a chosen state
inside a chosen velocity field; mpm_g2p2g + mpm_rebuild_partition, then mpm_retrieve_state / mpm_dump_grid / mpm_get_diagnostics / mpm_get_counts
show what the kernel made of it.  No new ABI, no switch.

All scenes: bits 6, max_ppc 16 (1024 particles per block: two 512-record chunks and the merged tail), dt 1e-4, new_dt 7.5e-5.

Bounds.  Per particle, against the model on the injected float32 values: max(the project's bound for the undeformed one-particle rows, 3 x Y),
Y = the float32 reference side's own deviation from the model for the same quantity, tier and material (g2p2g_model.Y).  Per grid node, derived:
|got - sum_p c_p| <= sum_p E_p + (n_g + 1) 2^-23 sum_p |c_p| over the union of expected and returned nodes, E_p = the per-particle stencil bound x
that particle's largest mass / momentum entry, no exception: the scenes hold no particle on the brink of a sand branch / NACC case (the generator
re-draws those, g2p2g_model.scene_state; check() asserts it, also for the state a first substep leaves behind).  Exact: particle
counts, the number of particle blocks (= distinct block keys of the returned positions), lost = 0, discarded = the model's count.

Kernel mutations (value-only, built in a scratch copy, never committed).  NOT RUN on an MI355X - the column says which test is EXPECTED to fail,
from reading the code, to be replaced by what a run shows:
  1 the scatter uses the old fd for the new weights           not run; expected: every grid comparison (isolated, flow tier upwards)
  2 contrib uses dt where new_dt belongs                      not run; expected: the grid comparisons of the solid models (stress term x 4/3)
  3 the B member of a pair slot takes A's b21                 not run; expected: test_block_sizes / test_neighbour_blocks (b of the B members), default mask only
  4 the shell path's atomics skip the mass channel            not run; expected: test_neighbour_blocks (fast), test_torn, the total-mass check
  5 log Jp is stored un-updated for slots >= 64               not run; expected: test_block_sizes (sand, NACC: sizes 65 upwards)
  6 the reflected bit is dropped on store                     not run; expected: the reflected-mark comparison of every FC scene
  7 the second scatter arena's sum is added twice for singles not run; expected: test_block_sizes / test_one_cell (nodes of odd-lane particles)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ckpt_format as cf
import g2p2g_model as gm
from g2p2g_bench import Bench, by_position_bits, st9_to_b6  # noqa: F401  (other test files take them from here)
from parity_util import match

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DX = 0.5 ** gm.BITS


def check_particles(bench, res, models, tier, tag, fails, bound_of=None):
    """The per-particle half of check(): counts, state and position of every particle of every model against `models`, and the books (particle
    blocks, lost, discarded).  Appends to `fails`; returns the per-model stencil bounds the grid comparison needs.  bound_of(i, quantity, tier,
    material): the bound of model i (default: g2p2g_model.bound for every model)."""
    if bound_of is None:
        bound_of = lambda i, q, t, mat: gm.bound(q, t, mat)
    blocks = set()
    n_disc = 0
    sbs = []
    for i, ((material, p), m, got) in enumerate(zip(bench.parts, models, res["state"])):
        name = gm.NAMES[material]
        n = p.shape[0]
        assert int(res["counts"].particles[i]) == n, (tag, name, "particle count", int(res["counts"].particles[i]), n)
        fin = m["finite"]
        assert fin.all() or tier in ("torn", "golden_violent"), "non-finite model rows below the torn tier"
        idx, _ = match(m["pos"][fin], got["pos"].astype(np.float64))          # (nearest neighbour, asserted one-to-one: final positions are >= 1e-3 cell apart)
        assert not m["unstable"].any(), (tag, name, "a row on the brink of a branch: the scenes hold none (g2p2g_model.scene_state)", np.flatnonzero(m["unstable"])[:5].tolist())
        rows = np.flatnonzero(fin)
        keep = np.ones(rows.size, bool)
        figs = {"pos": gm.err_pos(got["pos"][idx].astype(np.float64), m["pos"][rows])}
        if material == gm.J_FLUID:
            figs["J"] = gm.err_J(got["J"][idx].astype(np.float64), m["J"][rows])[keep]
        else:
            figs["b"] = gm.err_b(got["b6"][idx].astype(np.float64), m["b6"][rows])[keep]
            wrong = (got["reflected"][idx] != m["reflected"][rows]) & keep
            if wrong.any():
                fails.append((name, "reflected mark", int(wrong.sum()), rows[wrong][:5].tolist()))
            if material != gm.FC:
                figs["logjp"] = np.abs(got["logjp"][idx].astype(np.float64) - m["logjp"][rows])[keep]
        for q, e in figs.items():
            bnd = bound_of(i, q, tier, material)
            worst = float(e.max()) if e.size else 0.0
            print(f"{tag} {name} {tier} {q}: worst {worst:.3g} bound {bnd:.3g} (Y {gm.Y[q, tier, name]:.3g}) over {e.size} particles")
            if not worst <= bnd:
                fails.append((name, q, worst, bnd, int((e > bnd).sum())))
        blocks.update(map(tuple, gm.block_keys(got["pos"]).tolist()))
        n_disc += int(m["discarded"][fin].sum())
        sbs.append(bound_of(i, "stencil", tier, material))
    # the books
    print(f"{tag} {tier}: particle blocks {res['counts'].particle_blocks} (positions say {len(blocks)}), lost {res['lost']}, discarded {res['discarded']} (model {n_disc})")
    if res["counts"].particle_blocks != len(blocks):
        fails.append(("particle_blocks", int(res["counts"].particle_blocks), len(blocks)))
    if res["lost"] != 0 or res["discarded"] != n_disc:
        fails.append(("books", res["lost"], res["discarded"], n_disc))
    return sbs


def check_grid(exp, grid, tier, tag, fails):
    """The grid half of check(): the dumped grid against the assembled expectation `exp` (g2p2g_model.assemble) node by node over the union of
    expected and returned nodes, and the total mass.  Appends to `fails`."""
    gk, gv = gm.grid_nodes(*grid)
    ratio, bad, what = gm.compare_grid(exp, gk, gv)
    print(f"{tag} {tier} grid: {exp['key'].size} expected nodes, {gk.size} returned, up to {int(exp['n'].max())} contributions per node, worst |diff| / bound {ratio:.3g} at {what}")
    if bad:
        fails.append(("grid nodes beyond their bound", bad, ratio, what))
    mass_bound = float(((exp["n"] + 1) * 2.0 ** -23 * exp["abs"][:, 0]).sum())          # the summation term alone: a particle's 27 weights add up to its mass whatever its position
    if not abs(gv[:, 0].sum() - exp["sum"][:, 0].sum()) <= mass_bound:
        fails.append(("total mass", float(gv[:, 0].sum()), float(exp["sum"][:, 0].sum()), mass_bound))


def check(bench, res, models, tier, tag="", grid_extra=None, bound_of=None):
    """The step's result against the model outputs `models` (one step() dict per model of the bench).  Prints every figure before it asserts.
    grid_extra: (packed node keys, (k, 4) values) that something other than the models' particles has added to the grid, once per node
    (g2p2g_model.add_contribution); default: nothing.  bound_of: see check_particles."""
    fails = []
    sbs = check_particles(bench, res, models, tier, tag, fails, bound_of)
    exp = gm.assemble(models, sbs)
    if grid_extra is not None:
        exp = gm.add_contribution(exp, *grid_extra)
    check_grid(exp, res["grid"], tier, tag, fails)
    assert not fails, (tag, tier, fails)


def run(parts_states, tier, seed=0, tag=""):
    """One bench, one injection, one step, one check: parts_states = [(material, pos_cells, state)]"""
    bench = Bench([(m, p) for m, p, _ in parts_states])
    try:
        bench.inject([st for _, _, st in parts_states], lambda keys: gm.grid_of(keys, tier, seed))
        res = bench.step()
        models = [gm.step(c, p, gm.gather_field(p, tier, seed), b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"]) for c, (m, p, st) in zip(bench.consts, parts_states)]
        check(bench, res, models, tier, tag)
        return res, models
    finally:
        bench.close()


# ---- isolated: 48 sites, one particle each, every tier and material ------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS)
def test_isolated_particles_on_every_tier(material):
    """One particle per block on 48 sites, each in its own state inside its own cube of the field; eight of them planted on tie values and on the
    bounds of the block's first and last cell (the last eight sites).  One context, re-loaded per tier."""
    pos, st = gm.scene_state("isolated", material)
    bench = Bench([(material, pos)])
    try:
        for tier in gm.TIERS:
            bench.inject([st], lambda keys: gm.grid_of(keys, tier))
            res = bench.step()
            m = gm.model_scene(material, pos, st, tier)
            check(bench, res, [m], tier, "isolated")
    finally:
        bench.close()


# ---- block sizes: 1 .. 1024 particles per block ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material,tier", [(gm.FC, "flow"), (gm.SAND, "flow"), (gm.J_FLUID, "rest"), (gm.NACC, "rest")])
def test_block_sizes(material, tier):
    """One block per size in {1, 2, 3, 64, 65, 127, 128, 129, 511, 512, 513, 768, 769, 1024} in one scene: partial and several 64-lane iterations,
    one and two 512-record chunks, the merged tail of up to 768 records, slots beyond a block's first bin ({b21, log Jp} rows, the b record)."""
    pos, st = gm.scene_state("block_sizes", material)
    run([(material, pos, st)], tier, tag="block sizes")


# ---- one cell: all-equal sort keys ---------------------------------------------------------------------------------------------------------
def test_one_cell():
    """513 particles in a single cell, and 257 + 256 in two cells of one block: every lane of an iteration holds the same stencil base, so the owner
    table hands one lane per arena to the chain and everything else goes through the serial path (fixed-corotated, flow tier)."""
    pos, st = gm.scene_state("one_cell", gm.FC)
    run([(gm.FC, pos, st)], "flow", tag="one cell")


# ---- neighbours: blocks that share grid blocks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["flow", "fast"])
@pytest.mark.parametrize("material", gm.MATERIALS)
def test_neighbour_blocks(material, tier):
    """A 2 x 2 x 2 cluster of adjacent particle blocks with about 200 particles each: eight workgroups add into shared grid blocks, particles cross
    between them (the shell path's global atomics), and the rebuild buckets them in blocks that were neighbours a step ago."""
    pos, st = gm.scene_state("cluster", material)
    res, models = run([(material, pos, st)], tier, tag="cluster")
    assert (models[0]["dirtag"] != 13).sum() >= 0.03 * pos.shape[0]


def test_mixed_materials_in_the_same_blocks():
    """Fixed-corotated and J-fluid particles in the same blocks of the cluster: one grid, two launches."""
    pos_a, st_a = gm.scene_state("cluster", gm.FC)
    pos_b = gm.scene_cluster(seed=44, lo=90, hi=110)
    st_b = gm.make_state(gm.J_FLUID, pos_b.shape[0], 44)
    run([(gm.FC, pos_a, st_a), (gm.J_FLUID, pos_b, st_b)], "flow", tag="mixed")


# ---- a second substep: records that say "came from neighbour t" ----------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS)
def test_second_substep(material):
    """Step 1 on the cluster (flow tier); a checkpoint of what it left; a NEW velocity field patched into that; step 2 against the model fed the
    positions and state READ BACK after step 1 (so errors do not compound).  The lists of step 2 carry neighbour tags, their source bins lie in
    other blocks, and the pair layout is the one the rebuild has just sorted."""
    pos, st = gm.scene_state("cluster", material)
    bench = Bench([(material, pos)])
    try:
        bench.inject([st], lambda keys: gm.grid_of(keys, "flow"))
        res1 = bench.step()
        check(bench, res1, [gm.model_scene(material, pos, st, "flow")], "flow", "second substep, step 1")
        ck = bench.eng.save_checkpoint().copy()
        h = cf.parse(ck)
        ppb = cf.K_BIN * h["max_ppc"]
        tags = (cf.section(ck, h, ("lists", 0), np.int32).view(np.uint32) >> np.uint32(ppb.bit_length() - 1 + cf.K_KEY_BITS)) & np.uint32(31)
        moved = int((tags != 13).sum())
        print("records with a neighbour tag:", moved, "of", tags.size)
        assert moved >= 0.03 * tags.size
        back = res1["state"][0]
        p1 = back["pos"]
        solid = material != gm.J_FLUID
        # the new field: the first seed for which no particle of the state READ BACK sits on the brink of a sand branch / NACC case (the state a
        # return mapping leaves lies ON the yield surface, so with a given field one particle or two of 1 579 usually do: the field is re-drawn as
        # the generator re-draws states, and check() then holds every particle to its bound)
        for seed in range(1, 65):
            m2 = gm.step(bench.consts[0], p1, gm.gather_field(p1, "flow", seed), b6=back["b6"] if solid else None, reflected=back["reflected"] if solid else None,
                         logjp=back["logjp"] if material in (gm.SAND, gm.NACC) else None, J=back["J"] if not solid else None)
            if not m2["unstable"].any():
                break
        print("field of step 2: seed", seed)
        bench.load(ck, lambda keys: gm.grid_of(keys, "flow", seed=seed))
        again = bench.read(0)
        og, ow = by_position_bits(again["pos"]), by_position_bits(back["pos"])
        for k in ("pos", "J") if material == gm.J_FLUID else ("pos", "b6", "reflected", "logjp"):
            assert np.array_equal(np.ascontiguousarray(again[k][og]).view(np.uint8), np.ascontiguousarray(back[k][ow]).view(np.uint8)), k
        res2 = bench.step()
        bench.parts = [(material, p1)]
        check(bench, res2, [m2], "flow", "second substep, step 2")
    finally:
        bench.close()


# ---- torn: the discard path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS)
def test_torn(material):
    """The isolated scene and one block of 129 particles in a field that moves a particle over one cell per substep (:877-885): the number of
    discarded contributions is the model's and the oracle's on the same rows, nothing is lost, a discarded particle leaves nothing on the grid
    and is still bucketed with its state stored (check() compares every particle, discarded or not)."""
    pos, st = gm.scene_state("torn", material)
    res, models = run([(material, pos, st)], "torn", tag="torn")
    of, oi = gm.oracle_scene(material, pos, st, "torn")
    n_model, n_oracle = int(models[0]["discarded"].sum()), int((oi[:, 13] != 0).sum())
    print("discarded: kernel", res["discarded"], "model", n_model, "oracle", n_oracle)
    assert res["discarded"] == n_model == n_oracle and n_model >= 1
    assert res["lost"] == 0


# ---- the golden rows with a deformed F ---------------------------------------------------------------------------------------------------
GOLDEN_STRIDE = 1


@pytest.mark.parametrize("material", gm.MATERIALS)
def test_deformed_golden_rows_through_the_real_kernel(material):
    """The golden rows of arenas 0 .. 2 (the ones that abide by the CFL condition) that carry a deformed F and a non-trivial log Jp - 84 per material,
    which the existing one-particle test cannot replay for want of a per-particle initial state in the ABI - as one-particle scenes through the real
    kernel: state in through with_particle_state as b = fl32(F F^T), the row's velocity arena through with_grid.  Stride 1: all 84 rows per material
    (about a second).  Bounds: those of this file with Y measured on the golden rows themselves."""
    P, arenas, rin, wf, wi = gm.golden_rows()
    bits = int(P["bits"])
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32) if material != gm.J_FLUID else np.array([1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    plain = np.all(rin[:, 5:14] == eye, axis=1) & (rin[:, 14] == np.float32(-0.01 if material == gm.NACC else 0.0))
    rows = np.flatnonzero((rin[:, 0] == material) & (rin[:, 1] < 3) & ~plain)
    assert rows.size == 84
    rows = rows[::GOLDEN_STRIDE]
    over = gm.golden_overrides(P, material)
    model = gm.golden_model(material, P, arenas, rin[rows])
    state = gm.golden_state(material, rin[rows])
    assert model["finite"].all() and not model["unstable"].any()
    crossed = 0
    for j, r in enumerate(rows):
        pos = (rin[r, 2:5].astype(np.float64) * 2.0 ** bits).astype(np.float32).reshape(1, 3)
        arena = arenas[int(rin[r, 1])]
        origin = 4 * gm.block_keys(pos)[0]

        def vgrid(keys, arena=arena, origin=origin):
            out = np.zeros((len(keys), 3, 64), np.float32)
            for i, k in enumerate(np.asarray(keys).astype(np.int64)):
                o = 4 * k - origin
                if ((o >= 0) & (o <= 4)).all():
                    out[i] = arena[:, o[0]:o[0] + 4, o[1]:o[1] + 4, o[2]:o[2] + 4].reshape(3, 64)
            return out
        bench = Bench([(material, pos)], bits=bits, max_ppc=8, overrides=[over])
        try:
            one = {k: (v[j:j + 1] if v is not None else None) for k, v in state.items()}
            bench.inject([one], vgrid)
            d0 = bench.eng.diagnostics()
            before = (int(d0.lost_particles), int(d0.discarded_p2g))
            bench.eng.g2p2g(P["dt"], P["new_dt"])
            cnt = bench.eng.rebuild_partition()
            d1 = bench.eng.diagnostics()
            res = dict(counts=cnt, lost=int(d1.lost_particles) - before[0], discarded=int(d1.discarded_p2g) - before[1], grid=bench.eng.dump_grid(), state=[bench.read(0)])
            check(bench, res, [{k: v[j:j + 1] for k, v in model.items()}], "golden", f"golden row {r}")
        finally:
            bench.close()
        crossed += int(model["dirtag"][j] != 13)
    print("rows:", rows.size, "changed block:", crossed)


# ---- both kernels ----------------------------------------------------------------------------------------------------------------------------
def test_both_kernels_pass_this_file():
    """Everything above runs in process with the default mask (all four materials on the pair kernel).  This test runs the file again in a fresh
    child process with MPM_G2P2G_PAIRS=0 - the one-particle-per-lane kernel and the sliced list layout - under a time limit, deselecting itself
    there.  A child that ends on a signal fails the test, and nothing else is started."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not test_both_kernels_pass_this_file"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

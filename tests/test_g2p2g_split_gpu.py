"""The split G2P2G passes of the multi-GPU path - mpm_g2p2g_halo / mpm_mgsp_begin over the compacted halo block list, mpm_g2p2g_interior over all
blocks with the `only_flag` skip - against the float64 block model of tests/g2p2g_model.py, on injected deformed state (the checkpoint port of
tests/test_g2p2g_blocks_gpu.py, the phase-level halo calls of tests/test_halo_kernels_gpu.py).  Three facts are stated directly:
  1 exactly once: every particle block is processed by one of the two launches (a block taken twice adds its mass again, one taken by neither
    loses its particles);
  2 complete after the halo pass: what mpm_halo_collect(gid = 1) ships between the two launches already holds every contribution this rank will
    ever make to a shared grid block;
  3 launch-shape independence: a particle's new position and state do not depend on which launch handled it (bit for bit against plain
    mpm_g2p2g, and between the phased and the fused entry).
Part 1 drives ONE context with synthetic peer key lists (free inputs of mpm_halo_tag_peer: they select any subset of blocks as halo; particle
block k touches the grid blocks k + {0, 1}^3).  Part 2 cuts the slab scene (g2p2g_model.scene_slab, licensed on the CPU by
tests/test_g2p2g_model_cpu.py) between two MgspRank contexts on one GPU with the thread communicator of tests/test_mgsp_gpu.py; the cut is
partition_scene's with its planes on block faces (mgsp.ALIGN_TO_BLOCKS): the equal-count cut leaves ten particles of the x = 6 layer on rank 1,
and rank 0 then has no interior block at all.

All scenes: bits 6, max_ppc 16, dt / new_dt of g2p2g_model, the velocity field g2p2g_model.grid_of (a pure function of the node: any two contexts
agree on it).  mpm_checkpoint_load clears the tagging: every test tags AFTER the load.

Bounds: those of tests/test_g2p2g_blocks_gpu.py and nothing else - per particle g2p2g_model.bound(), per node compare_grid()'s derived bound.  A
block that mpm_halo_reduce adds to counts as one more contribution per node with E = 0 (g2p2g_model.add_contribution).  The bit-for-bit
comparisons rest on DESIGN.md's statement that a per-particle result depends on the particle alone.

Kernel mutations (value-only, built in a scratch copy, never committed) run on an MI355X against the cluster and isolated tests of this file
(blocks of at most 215 particles: every_block, shared_blocks, mixed, identities, fused_entry; default mask, i.e. the pair kernel in process; both
G2P2G kernels carried the mutation), and the tests that failed, each with ordinary assertion failures or the library's own error return:
  `block_list ? block_list[bid] : bid` -> `bid` (both G2P2G kernels)     all 14: the rebuild's books ("1558 bucketed of 1579 added": the listed blocks are taken by
                                                                          neither launch), particle matching not one-to-one (isolated), ids not a permutation
  the `flag == 0` skip dropped from both G2P2G kernels                   all 14: the rebuild's books ("49 bucketed of 48 added", "2370 bucketed of 1579 added")
  the same skip dropped from move_ids_kernel                             none: equivalent.  The interior launch then moves the halo blocks' ids once more, from the
                                                                          same source slots to the same destination slots - the same values written twice
  `halo = true` only for i == 0 in halo_split_kernel                     10: the halo count of the tagging (1 where 2, 2 where 4 blocks touch the key) in
                                                                          shared_blocks (all 5), mixed, identities[cluster], fused_entry (all 3); the isolated
                                                                          tests pass (their keys are the blocks' own, i = j = k = 0)
  `ctx->grid[gid]` -> `ctx->grid[0]` in halo_collect                     5: shared_blocks (all): 64 nodes beyond their bound, velocities of 20 m/s where the
                                                                          P2G sums belong
  MPM_HACK_STALE_INTERIOR (-DMPM_EXPERIMENT)                             none: equivalent here.  The hack differs only where the host has not seen the counts
                                                                          (the windowed group loop, tests/test_mgsp_gpu.py); every call of this file has
(the slab, block_sizes and torn tests were left out of the mutation runs)

Wall time of the whole file on an MI355X: 17.9 s for its 31 tests, the MPM_G2P2G_PAIRS=0 child included (7.8 s for the 30 in process); the
slowest single test, the child apart, takes 0.4 s."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import ckpt_format as cf
import g2p2g_model as gm
import halo_model as hm
import particle_ids_model as pim
from claymore_amd import mgsp
from claymore_amd.mgsp import MgspRank
from test_g2p2g_blocks_gpu import Bench, by_position_bits, check, check_particles
from test_halo_kernels_gpu import CANARY, HipRank, _dev, _ptr
from test_mgsp_gpu import ThreadComm
from test_particle_ids_gpu import IdBench
from test_particle_ids_gpu import inject as inject_with_ids

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PEER = 5
HALO_COUNTS = (0, 1, 7, 8, 9, 47, 48)
CELL = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)])


# ---- helpers -------------------------------------------------------------------------------------------------------------------------------
def halo_port(eng):
    """tests/test_halo_kernels_gpu.HipRank's phase-level calls on an existing engine"""
    hr = HipRank.__new__(HipRank)
    hr.eng, hr.api, hr.ctx = eng, eng.api, eng.ctx
    return hr


def keys_array(keys):
    return np.asarray(list(keys), dtype=np.int32).reshape(-1, 3)


def tag(hr, lists, tag_=""):
    """Tag with the peer lists {peer: keys}; asserts through mpm_halo_dump that the halo list and the interior flags are the set-level model's
    (tests/halo_model.py), duplicate-free and complementary.  -> (model, tagging, send counts)"""
    m = hr.model()
    lists = {p: keys_array(k) for p, k in lists.items()}
    t = m.tag(lists)
    nh, sc = hr.tag(lists)
    ov, hl, fl = hr.dump(m)
    print(f"{tag_}: {m.pbc} particle blocks, {nh} halo, {int(fl.sum())} interior, send counts {[(p, c) for p, c in enumerate(sc) if c]}")
    assert nh == len(t.halo_blocks) == hl.size and sc == t.send_counts
    assert len(set(hl.tolist())) == hl.size and {m.keys[b] for b in hl} == t.halo_blocks
    assert set(fl.tolist()) <= {0, 1} and fl.size == m.pbc
    assert np.array_equal(np.flatnonzero(fl == 0), np.sort(hl)), "the interior flags are not the complement of the halo list"
    return m, t, sc


def split_step(bench, between=None, after=None):
    """Bench.step() with the two launches in place of mpm_g2p2g: mpm_g2p2g_halo, between(), mpm_g2p2g_interior, after(), mpm_rebuild_partition"""
    eng = bench.eng
    d0 = eng.diagnostics()
    before = (int(d0.lost_particles), int(d0.discarded_p2g))
    eng._check(eng.api.g2p2g_halo(eng.ctx, gm.DT, gm.NEW_DT))
    if between:
        between()
    eng._check(eng.api.g2p2g_interior(eng.ctx, gm.DT, gm.NEW_DT))
    if after:
        after()
    cnt = eng.rebuild_partition()
    d1 = eng.diagnostics()
    gk, gb = eng.dump_grid()
    return dict(counts=cnt, lost=int(d1.lost_particles) - before[0], discarded=int(d1.discarded_p2g) - before[1], grid=(gk, gb),
                state=[bench.read(i) for i in range(len(bench.parts))])


def state_keys(material):
    return ("pos", "J") if material == gm.J_FLUID else ("pos", "b6", "reflected") + (("logjp",) if material != gm.FC else ())


def assert_same_bits(material, got, want, what):
    """Two retrieve_state readouts hold the same particles bit for bit (rows ordered by position bits)"""
    assert got["pos"].shape == want["pos"].shape, (what, got["pos"].shape, want["pos"].shape)
    og, ow = by_position_bits(got["pos"]), by_position_bits(want["pos"])
    for k in state_keys(material):
        a, b = np.ascontiguousarray(got[k][og]), np.ascontiguousarray(want[k][ow])
        differ = np.flatnonzero((a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)).any(axis=1))
        worst = float(np.abs(a[differ].astype(np.float64) - b[differ].astype(np.float64)).max()) if differ.size and k != "reflected" else 0.0
        print(f"{what} {gm.NAMES[material]} {k}: {differ.size} of {a.shape[0]} rows differ (largest difference {worst:.3g})")
        assert differ.size == 0, (what, k, differ[:5].tolist(), worst)


def models_of(bench, parts_states, tier):
    return [gm.step(c, p, gm.gather_field(p, tier), b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"]) for c, (m, p, st) in zip(bench.consts, parts_states)]


def every_other_block(m):
    return {PEER: [m.keys[b] for b in range(0, m.pbc, 2)]}


def run_split(parts_states, tier, lists_of, tag_):
    """One bench, one injection, tagging with lists_of(halo model), the two launches, check() -> (res, models, tagging)"""
    bench = Bench([(m, p) for m, p, _ in parts_states])
    try:
        bench.inject([st for _, _, st in parts_states], lambda keys: gm.grid_of(keys, tier))
        hr = halo_port(bench.eng)
        m, t, _ = tag(hr, lists_of(hr.model()), tag_)
        assert t.halo_blocks and t.interior_blocks, "the scene is meant to give both launches something to do"
        res = split_step(bench)
        models = models_of(bench, parts_states, tier)
        check(bench, res, models, tier, tag_)
        return res, models, t
    finally:
        bench.close()


# ---- 1a: exactly once, for every halo count --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", [gm.FC, gm.SAND])
def test_every_block_exactly_once_for_every_halo_count(material):
    """The isolated scene (48 blocks, one particle each, keys three apart: grid block k belongs to particle block k alone), flow tier.  For
    h in HALO_COUNTS one peer lists the keys of h blocks drawn with a seeded rng - never the first h of the numbering, so a kernel that ignored
    its list would take other blocks -: 0 and 48 leave one launch empty, 1, 7, 8, 9 and 47 deal the list over the 8 XCD shares with and without a
    remainder.  The split step passes check() with the unsplit bounds and returns every particle bit for bit as plain mpm_g2p2g does."""
    pos, st = gm.scene_state("isolated", material)
    model = gm.model_scene(material, pos, st, "flow")
    vgrid = lambda keys: gm.grid_of(keys, "flow")
    bench = Bench([(material, pos)])
    try:
        hr = halo_port(bench.eng)
        bench.inject([st], vgrid)
        plain = bench.step()
        check(bench, plain, [model], "flow", "isolated, one launch")
        rng = np.random.default_rng(48)
        for h in HALO_COUNTS:
            bench.inject([st], vgrid)
            m = hr.model()
            assert m.pbc == 48
            while True:
                pick = np.sort(rng.permutation(48)[:h])
                if h in (0, 48) or pick.tolist() != list(range(h)):
                    break
            listed = [m.keys[b] for b in rng.permutation(pick)]
            _, t, sc = tag(hr, {PEER: listed}, f"isolated h = {h}")
            ov, hl, fl = hr.dump(m)
            assert hl.size == h and np.array_equal(np.sort(hl), pick) and sc[PEER] == h
            assert np.array_equal(np.flatnonzero(fl == 1), np.setdiff1d(np.arange(48), pick))
            res = split_step(bench)
            check(bench, res, [model], "flow", f"isolated h = {h}")
            assert res["lost"] == 0 and int(res["counts"].particles[0]) == 48
            assert res["counts"].particle_blocks == plain["counts"].particle_blocks == len(set(map(tuple, gm.block_keys(res["state"][0]["pos"]).tolist())))
            assert_same_bits(material, res["state"][0], plain["state"][0], f"isolated h = {h}: split against one launch,")
    finally:
        bench.close()


# ---- 1b: shared blocks are complete after the halo pass ------------------------------------------------------------------------------------
SHARED = {"1 block": ({PEER: [(6, 6, 6)]}, 1), "2 blocks": ({PEER: [(7, 6, 6)]}, 2), "4 blocks": ({PEER: [(7, 7, 6)]}, 4), "8 blocks": ({PEER: [(7, 7, 7)]}, 8),
          "two peers": ({0: [(6, 6, 6)], 31: [(8, 8, 8)]}, 2)}


def fabricated(keys, particle_mass):
    """What a peer might send for the grid blocks `keys`: hashed noise of the node, positive mass.  -> (blocks (n, 256), packed nodes, (64 n, 4))"""
    keys = keys_array(keys).astype(np.int64)
    nodes = 4 * keys[:, None, :] + CELL[None, :, :]
    v = gm.field(nodes, "flow", seed=77)
    u = gm.field(nodes, "rest", seed=78)[..., 0]                          # [-0.1, 0.9)
    mass = (np.float32(particle_mass) * (np.float32(1.0) + np.float32(0.5) * u)).astype(np.float32)
    assert (mass > 0).all()
    blocks = np.empty((len(keys), 4, 64), np.float32)
    blocks[:, 0] = mass
    blocks[:, 1:4] = (v * mass[..., None]).transpose(0, 2, 1)
    return blocks.reshape(len(keys), 256), gm.pack_nodes(nodes).reshape(-1), blocks.transpose(0, 2, 1).reshape(-1, 4).astype(np.float64)


@pytest.mark.parametrize("material,tier", [(m, "flow") for m in gm.MATERIALS] + [(gm.SAND, "fast")])
def test_shared_blocks_are_complete_after_the_halo_pass(material, tier):
    """The cluster with one shared grid key touched by 1, 2, 4 and 8 particle blocks, and two peers with one key each.  After mpm_g2p2g_halo and
    BEFORE the interior launch mpm_halo_collect(gid = 1) returns exactly the shared keys, and every node of those blocks already agrees with the
    WHOLE scene's model sum (compare_grid's bound, restricted to the blocks) - the interior launch adds nothing to them; the canaries around the
    buffers are intact.  Then the interior launch and mpm_halo_reduce(gid = 1) with a fabricated block per shared key: after the rebuild the
    grid is the model's plus that one addition per node, over the union of nodes, and the particles pass check()."""
    pos, st = gm.scene_state("cluster", material)
    model = gm.model_scene(material, pos, st, tier)
    exp = gm.assemble([model], [gm.bound("stencil", tier, material)])
    bench = Bench([(material, pos)])
    try:
        hr = halo_port(bench.eng)
        for name, (lists, n_halo) in SHARED.items():
            what = f"cluster {gm.NAMES[material]} {tier}, {name}"
            bench.inject([st], lambda keys: gm.grid_of(keys, tier))
            m, t, sc = tag(hr, lists, what)
            assert len(t.halo_blocks) == n_halo and len(t.interior_blocks) == 8 - n_halo
            sent = {}

            def between():
                for p, ks in lists.items():
                    n = sc[p]
                    rc, ns, keys, blocks = hr.collect(p, n, gid=1)
                    assert rc == 0 and ns == n == len(ks), (what, p, rc, ns, n)
                    assert (keys[0] == CANARY).all() and (keys[1 + n:] == CANARY).all() and (blocks[0] == CANARY).all() and (blocks[1 + n:] == CANARY).all(), (what, p, "a canary was overwritten")
                    sent[p] = (keys[1:1 + n].copy(), blocks[1:1 + n].copy())

            extra = {}

            def after():
                for p, ks in lists.items():
                    blocks, nodes, vals = fabricated(ks, bench.consts[0]["mass"])
                    hr.reduce(keys_array(ks), blocks, gid=1)
                    extra[p] = (nodes, vals)

            res = split_step(bench, between, after)
            for p, ks in lists.items():
                keys, blocks = sent[p]
                assert sorted(hm.as_keys(keys)) == sorted(tuple(k) for k in ks), (what, p)
                gk, gv = gm.grid_nodes(keys, blocks.reshape(-1, 4, 64))
                e = gm.restrict(exp, gm.in_blocks(exp["key"], keys))
                ratio, bad, worst = gm.compare_grid(e, gk, gv)
                print(f"{what}: peer {p} collected {len(keys)} block(s) after the halo pass: {e['key'].size} expected nodes, {gk.size} returned, worst |diff| / bound {ratio:.3g} at {worst}")
                assert e["key"].size > 0, "nobody contributes to the shared block: nothing to compare"
                assert bad == 0, (what, p, bad, ratio, worst)
            check(bench, res, [model], tier, what, grid_extra=(np.concatenate([extra[p][0] for p in lists]), np.concatenate([extra[p][1] for p in lists])))
    finally:
        bench.close()


# ---- 1c: large blocks and two models -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material,tier", [(gm.SAND, "flow"), (gm.J_FLUID, "rest")])
def test_block_sizes_with_every_other_block_halo(material, tier):
    """Blocks of 1 .. 1024 particles, every other one listed: multi-chunk blocks and the merged tail through the list path and through the flag path."""
    pos, st = gm.scene_state("block_sizes", material)
    res, _, t = run_split([(material, pos, st)], tier, every_other_block, "block sizes, every other block halo")
    assert len(t.halo_blocks) == 7 and res["lost"] == 0


def test_mixed_materials_share_one_list_and_one_flag_array():
    """Fixed-corotated and J-fluid particles in the same blocks of the cluster, the key (7, 7, 6) shared: two launches per pass read one list and
    one flag array."""
    pos_a, st_a = gm.scene_state("cluster", gm.FC)
    pos_b = gm.scene_cluster(seed=44, lo=90, hi=110)
    st_b = gm.make_state(gm.J_FLUID, pos_b.shape[0], 44)
    res, _, t = run_split([(gm.FC, pos_a, st_a), (gm.J_FLUID, pos_b, st_b)], "flow", lambda m: {PEER: [(7, 7, 6)]}, "mixed, (7, 7, 6) shared")
    assert len(t.halo_blocks) == 4 and res["lost"] == 0


# ---- 1d: discards add up ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS)
def test_torn_discards_add_up_over_the_two_launches(material):
    """The torn scene, every other block listed: the two launches together discard what the model discards, nothing is lost, and check() compares
    every particle, discarded or not."""
    pos, st = gm.scene_state("torn", material)
    res, models, _ = run_split([(material, pos, st)], "torn", every_other_block, "torn, every other block halo")
    n_model = int(models[0]["discarded"][models[0]["finite"]].sum())
    print("discarded: the two launches", res["discarded"], "model", n_model)
    assert res["discarded"] == n_model >= 1 and res["lost"] == 0


# ---- 1e: identities ------------------------------------------------------------------------------------------------------------------------
def isolated_list(h):
    def lists(m):
        rng = np.random.default_rng(480 + h)
        while True:
            pick = np.sort(rng.permutation(m.pbc)[:h])
            if pick.tolist() != list(range(h)):
                return {PEER: [m.keys[b] for b in pick]}
    return lists


@pytest.mark.parametrize("shape", ["isolated h = 1", "isolated h = 9", "cluster (7, 7, 6)"])
def test_identities_follow_the_two_launches(shape):
    """move_ids_kernel with the halo list and with the interior flags: after the split step the id blob holds what tests/particle_ids_model.py
    predicts from the checkpoint and blob before it in every live slot, and mpm_retrieve_ids returns a permutation."""
    if shape.startswith("isolated"):
        parts, tier, lists_of = [(gm.FC, gm.scene_isolated())], "flow", isolated_list(int(shape.split("=")[1]))
    else:
        parts, tier, lists_of = [(gm.SAND, gm.scene_cluster())], "fast", lambda m: {PEER: [(7, 7, 6)]}
    bench = IdBench(parts)
    try:
        eng = bench.eng
        inject_with_ids(bench, [gm.make_state(m, p.shape[0], 7 + i) for i, (m, p) in enumerate(parts)], tier, as_momentum=False)
        hr = halo_port(eng)
        _, t, _ = tag(hr, lists_of(hr.model()), shape)
        assert t.halo_blocks and t.interior_blocks
        ck, blob = eng.save_checkpoint().copy(), eng.save_particle_ids().copy()
        d0 = eng.diagnostics()
        eng._check(eng.api.g2p2g_halo(eng.ctx, gm.DT, gm.NEW_DT))
        eng._check(eng.api.g2p2g_interior(eng.ctx, gm.DT, gm.NEW_DT))
        eng.rebuild_partition()
        d1 = eng.diagnostics()
        assert int(d1.lost_particles) + int(d1.dropped_particles) == int(d0.lost_particles) + int(d0.dropped_particles)
        after = pim.unpack(eng.save_particle_ids())
        for mi, (_, p) in enumerate(parts):
            exp, live = pim.expected_blob_slots(ck, blob, mi)
            n_after, got = after[mi]
            assert n_after == p.shape[0] and got.size == exp.size
            wrong = np.flatnonzero(got[live] != exp[live])
            print(f"{shape} model {mi}: {int(live.sum())} live slots, {wrong.size} wrong")
            assert wrong.size == 0, (shape, wrong[:8].tolist(), got[live][wrong[:8]].tolist(), exp[live][wrong[:8]].tolist())
            xyz, ids = eng.retrieve_ids(mi)
            assert np.array_equal(np.sort(ids), np.arange(p.shape[0])), "mpm_retrieve_ids does not return a permutation"
    finally:
        bench.close()


# ---- 1f: the fused entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", [gm.J_FLUID, gm.FC, gm.SAND])
def test_fused_entry_equals_the_phased_one(material):
    """The cluster with momenta injected (velocity x the node's saved mass) and (7, 7, 6) shared with a synthetic peer, twice from one load: phased
    (mpm_grid_update, halo, interior, rebuild) and fused (mpm_mgsp_begin, interior, mpm_mgsp_rebuild_export, mpm_mgsp_tag, mpm_mgsp_end; the peer's
    padded key rows as the phantom peers of tests/test_halo_kernels_gpu.py have them).  The particles, the counts and the diagnostics are equal
    bit for bit; each path's grid and particles pass check() against the model fed the velocities mpm_dump_grid returns right after the phased
    run's grid update."""
    pos, st = gm.scene_state("cluster", material)
    shared = [(7, 7, 6)]
    bench = Bench([(material, pos)])
    try:
        eng, api, ctx = bench.eng, bench.eng.api, bench.eng.ctx
        hr = halo_port(eng)
        buf = cf.with_particle_state(bench.ckpt, 0, pos, J=st["J"]) if material == gm.J_FLUID else cf.with_particle_state(bench.ckpt, 0, pos, b=st["b6"], logjp=st["logjp"], reflected=st["reflected"])
        g = cf.grid(buf).copy()
        g[:, 1:4] = gm.grid_of(cf.cur_keys(buf)[:g.shape[0]], "flow") * g[:, 0:1]
        buf = cf.with_grid(buf, g)
        # phased
        eng.load_checkpoint(buf)
        _, t, _ = tag(hr, {1: shared}, "fused entry, phased run")
        assert len(t.halo_blocks) == 4
        eng.grid_update(gm.DT)
        vk, vb = eng.dump_grid()
        vk, vb = vk.copy(), vb.copy()
        phased = split_step(bench)
        c = bench.consts[0]
        model = gm.step(c, pos, gm.gather_grid(pos, vk, vb), b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"])
        check(bench, phased, [model], "flow", "fused entry, phased run")
        # fused
        eng.load_checkpoint(buf)
        tag(hr, {1: shared}, "fused entry, fused run")
        d0 = eng.diagnostics()
        before = (int(d0.lost_particles), int(d0.discarded_p2g))
        pad = 4 * eng.counts().neighbor_blocks + 8
        mine = torch.full((pad, 3), CANARY, dtype=torch.int32, device="cuda")
        allk = _dev(hm.padded_rows(2, pad, {1: keys_array(shared)}).reshape(-1, 3))
        torch.cuda.synchronize()
        eng._check(api.mgsp_begin(ctx, gm.DT, gm.NEW_DT))
        eng._check(api.g2p2g_interior(ctx, gm.DT, gm.NEW_DT))
        eng._check(api.mgsp_rebuild_export(ctx, _ptr(mine), pad))
        eng._check(api.mgsp_tag(ctx, _ptr(allk), pad, 2, 0))
        sc, nh, mx, mv = (C.c_int * 32)(), C.c_int(-1), C.c_int(-1), C.c_float(0)
        eng._check(api.mgsp_end(ctx, sc, C.byref(nh), C.byref(mx), C.byref(mv)))
        d1 = eng.diagnostics()
        fused = dict(counts=eng.counts(), lost=int(d1.lost_particles) - before[0], discarded=int(d1.discarded_p2g) - before[1], grid=eng.dump_grid(), state=[bench.read(0)])
        check(bench, fused, [model], "flow", "fused entry, fused run")
        m2 = hr.model()
        t2 = m2.tag({1: keys_array(shared)})
        assert nh.value == len(t2.halo_blocks) and list(sc) == t2.send_counts and mx.value == 2, (nh.value, list(sc)[:2], mx.value)      # (the peer's row holds one key)
        assert mine.cpu().numpy()[0].tolist() == [m2.nbc, 0, 0]
        # the two paths
        assert_same_bits(material, fused["state"][0], phased["state"][0], "fused against phased,")
        for f in ("particle_blocks", "neighbor_blocks", "exterior_blocks"):
            assert getattr(fused["counts"], f) == getattr(phased["counts"], f), f
        assert int(fused["counts"].particles[0]) == int(phased["counts"].particles[0]) == pos.shape[0]
        assert (fused["lost"], fused["discarded"]) == (phased["lost"], phased["discarded"]) == (0, 0)
    finally:
        bench.close()


# ---- 2: two real contexts ------------------------------------------------------------------------------------------------------------------
def rows_in(whole, part):
    """Index of every row of `part` in `whole`, by position bits (every one found exactly once)"""
    where = {tuple(k): i for i, k in enumerate(np.ascontiguousarray(whole, np.float32).view(np.uint32).tolist())}
    assert len(where) == whole.shape[0]
    return np.array([where[tuple(k)] for k in np.ascontiguousarray(part, np.float32).view(np.uint32).tolist()], np.int64)


_TWO_RANKS = {}


def two_ranks(material, tier):
    """The slab cut between two MgspRanks on one GPU; on each rank the set-up checkpoint patched with its own particles' state and the field,
    _tag(), _advance(DT, NEW_DT): the halo launch, the exchange with gid 1 beside the interior launch, the rebuild and the tagging.  Run once per
    (material, tier) and shared between the tests.  -> per rank a dict of what came out, all numpy."""
    if (material, tier) in _TWO_RANKS:
        return _TWO_RANKS[material, tier]
    pos, st = gm.scene_state("slab", material)
    sc = {"name": "g2p2g_split_slab", "bits": gm.BITS, "dt": gm.DT, "config": {"max_ppc": gm.MAX_PPC},
          "models": [{"material": material, "xyz": pos * np.float32(0.5 ** gm.BITS), "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(material))}]}
    world, group = 2, ThreadComm(2)
    out, errors = [None] * world, []
    align = mgsp.ALIGN_TO_BLOCKS
    mgsp.ALIGN_TO_BLOCKS = True                  # partition_scene's cut planes on block faces (see the module docstring)

    def work(rank):
        sim = None
        try:
            sim = MgspRank(sc, rank, world, device=0, comm=group.view(rank))
            sim.initial_setup()
            own = sim.eng.retrieve_state(0)[0] * np.float32(2.0 ** gm.BITS)
            idx = rows_in(pos, own)
            bench = Bench.__new__(Bench)
            bench.bits, bench.dx, bench.eng = gm.BITS, 0.5 ** gm.BITS, sim.eng
            bench.parts = [(material, pos[idx])]
            bench.over = [gm.material_overrides(material)]
            bench.consts = [gm.constants(material, bench.over[0])]
            bench.ckpt = sim.eng.save_checkpoint().copy()
            bench.inject([{k: (v[idx] if v is not None else None) for k, v in st.items()}], lambda keys: gm.grid_of(keys, tier))
            hr = halo_port(sim.eng)
            m = hr.model()
            sim._tag()
            ov, hl, fl = hr.dump(m)
            d0 = sim.eng.diagnostics()
            sends, n_halo = list(sim.send_counts), sim.n_halo_blocks
            sim._advance(gm.DT, gm.NEW_DT)
            sim._check(sim.api.sync(sim.ctx))
            d1 = sim.eng.diagnostics()
            gk, gb = sim.eng.dump_grid()
            out[rank] = dict(idx=idx, bench=bench, keys=m.keys, pbc=m.pbc, halo=sorted(m.keys[b] for b in hl), interior=sorted(m.keys[b] for b in np.flatnonzero(fl == 1)),
                             sends=sends, n_halo=n_halo, counts=sim.eng.counts(), lost=int(d1.lost_particles) - int(d0.lost_particles),
                             discarded=int(d1.discarded_p2g) - int(d0.discarded_p2g), grid=(gk.copy(), gb.copy()), state=[bench.read(0)])
        except BaseException as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            group.bar.abort()
        finally:
            if sim is not None:
                sim.close()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
    finally:
        mgsp.ALIGN_TO_BLOCKS = align
    assert not errors and all(o is not None for o in out), errors
    _TWO_RANKS[material, tier] = out
    return out


TWO_RANK_CASES = [(m, "flow") for m in gm.MATERIALS] + [(gm.SAND, "fast")]


@pytest.mark.parametrize("material,tier", TWO_RANK_CASES)
def test_two_ranks_against_the_whole_scene_model(material, tier):
    """2a.  What the cut gave is asserted, not assumed.  Each rank's particles against the whole-scene model rows of its own particles
    (check()'s per-particle bounds and books); each rank's grid against the whole-scene sums with one more addition per node, at the nodes it
    returns; the union of returned nodes covers every expected node and nothing appears elsewhere; the nodes of blocks shared before the step carry
    identical bits on both ranks (world 2: fl(a + b) = fl(b + a))."""
    pos, st = gm.scene_state("slab", material)
    model = gm.model_scene(material, pos, st, tier)
    ranks = two_ranks(material, tier)
    what = f"slab {gm.NAMES[material]} {tier}"
    # the cut
    assert np.array_equal(np.sort(np.concatenate([r["idx"] for r in ranks])), np.arange(pos.shape[0])), "the ranks' particles are not a partition of the scene"
    for r, o in enumerate(ranks):
        pkeys = sorted(set(map(tuple, gm.block_keys(pos[o["idx"]]).tolist())))
        print(f"{what} rank {r}: {o['idx'].size} particles in blocks {pkeys}; halo {o['halo']}; interior {o['interior']}; send counts {[(p, c) for p, c in enumerate(o['sends']) if c]}")
        assert sorted(o["keys"][:o["pbc"]]) == pkeys
        assert len(o["halo"]) >= 1 and len(o["interior"]) >= 1 and o["n_halo"] == len(o["halo"])
        assert sorted(o["halo"] + o["interior"]) == pkeys
    assert {k[0] for k in ranks[0]["keys"][:ranks[0]["pbc"]]} == {5, 6} and {k[0] for k in ranks[1]["keys"][:ranks[1]["pbc"]]} == {7, 8}
    shared = set(ranks[0]["keys"]) & set(ranks[1]["keys"])
    assert ranks[0]["sends"][1] == ranks[1]["sends"][0] == len(shared) > 0
    new_x = gm.block_keys(model["pos"])[:, 0]
    crossing = int((new_x[ranks[0]["idx"]] >= 7).sum() + (new_x[ranks[1]["idx"]] <= 6).sum())
    print(f"{what}: {len(shared)} shared grid blocks, {crossing} model particles cross the cut")
    assert crossing >= 10
    # particles and books, rank by rank
    fails = []
    for r, o in enumerate(ranks):
        rows = {k: v[o["idx"]] for k, v in model.items()}
        check_particles(o["bench"], o, [rows], tier, f"{what} rank {r}", fails)
    assert sum(int(o["counts"].particles[0]) for o in ranks) == pos.shape[0] and all(o["lost"] == 0 for o in ranks)
    # grids
    exp = gm.assemble([model], [gm.bound("stencil", tier, material)])
    seen = []
    for r, o in enumerate(ranks):
        gk, gv = gm.grid_nodes(*o["grid"])
        stray = int((~np.isin(gk, exp["key"])).sum())
        e = gm.restrict(exp, np.isin(exp["key"], gk))
        e["n"] = e["n"] + 1
        ratio, bad, worst = gm.compare_grid(e, gk, gv)
        print(f"{what} rank {r} grid: {gk.size} nodes returned of {exp['key'].size} expected in the scene, {stray} nobody contributes to, worst |diff| / bound {ratio:.3g} at {worst}")
        if stray or bad:
            fails.append(("grid", r, stray, bad, ratio, worst))
        seen.append(gk)
    missing = np.setdiff1d(exp["key"], np.concatenate(seen))
    if missing.size:
        fails.append(("expected nodes that no rank returns", missing.size, gm.unpack_nodes(missing[:3]).tolist()))
    g0, g1 = hm.grid_dict(*ranks[0]["grid"]), hm.grid_dict(*ranks[1]["grid"])
    both = [k for k in sorted(shared) if k in g0 and k in g1]
    differ = [k for k in both if not np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32))]
    filled = sum(bool(np.any(g0[k])) for k in both)
    print(f"{what}: {len(both)} of {len(shared)} shared blocks held by both ranks after the step, {filled} of them non-zero, {len(differ)} differ in their bits")
    assert filled >= 1
    if differ:
        fails.append(("shared blocks whose bits differ between the ranks", differ[:4]))
    assert not fails, (what, fails)


@pytest.mark.parametrize("material,tier", TWO_RANK_CASES)
def test_two_ranks_equal_one_context_bit_for_bit(material, tier):
    """2b.  The union of both ranks' particles equals, bit for bit, the whole slab stepped in one context with plain mpm_g2p2g."""
    pos, st = gm.scene_state("slab", material)
    ranks = two_ranks(material, tier)
    bench = Bench([(material, pos)])
    try:
        bench.inject([st], lambda keys: gm.grid_of(keys, tier))
        plain = bench.step()
    finally:
        bench.close()
    union = {k: np.concatenate([o["state"][0][k] for o in ranks]) for k in state_keys(material)}
    assert_same_bits(material, union, plain["state"][0], f"slab {tier}: two ranks against one context,")


# ---- both kernels ----------------------------------------------------------------------------------------------------------------------------
def test_both_kernels_pass_this_file():
    """Everything above runs in process with the default mask (the pair kernel).  This test runs the file again in a fresh child process with
    MPM_G2P2G_PAIRS=0 - the one-particle-per-lane kernel and the sliced list layout - under a time limit, deselecting itself there.  A child
    that ends on a signal or at its limit fails the test, and nothing else is started."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not test_both_kernels_pass_this_file"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

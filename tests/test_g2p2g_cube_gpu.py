"""The node cube of a particle block against its eight grid blocks, both ways, through the real kernels: the staging of the grid velocities into the gather arena
and the write-back of the scatter arenas to the next grid (claymore_amd/csrc/mpm_g2p2g.hpp: cube_stage_load / cube_stage_store / cube_writeback, two octants per
wave-instruction by the lane mapping of mpm_cube_lane.hpp, which tests/test_cube_lane_model.py checks on the CPU).

ONE substep through the ABI per scene, injected as tests/test_g2p2g_blocks_gpu.py injects (its Bench / check / run are used as they are): every node of the P2G
grid against the float64 assembler of tests/g2p2g_model.py at the per-node summation bound derived there, every particle's position and state against the model at
the existing per-particle bounds; nodes the model leaves untouched must be bit-zero.  J-fluid (four waves, no serial queue) and sand (three waves, queue) each:
  (a) one block with one particle in each of its eight corner cells: all eight octants, all 216 arena nodes receive something, one contribution each
  (b) the same scene twice: a lone block has one writer per node, so the two grids are bit-identical
  (c) two face-adjacent blocks and a 2 x 2 x 2 group with a particle in every corner cell: shared nodes with two to eight writers
  (d) a block column in the wall zone of each low face (tests/face_scenes.face_box_cells; the layers with lround(p) >= 2, for which the model defines the block key)
  (e) two models on one grid
  (f) the gather side: the hashed node-velocity field of the flow tier - each of the 216 staged nodes distinct - and the particles' positions and state after the step
  (g) the whole file once more in a child process with MPM_G2P2G_PAIRS=0 (the one-particle kernel uses the same helpers)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import face_scenes as fs
import g2p2g_model as gm
import test_g2p2g_blocks_gpu as tb

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MATERIALS = (gm.J_FLUID, gm.SAND)
KEY = (6, 6, 6)
PAIR = [(3, 3, 3), (4, 3, 3)]                                  # two face-adjacent blocks, clear of the group
GROUP = gm.CLUSTER


def corner_particles(key, rng, jitter=0.3):
    """One particle in each of the eight corner cells of particle block `key` (cells): lround(p) = 4 k + 2 or 4 k + 5 per axis, so the eight stencils
    (bases 4 k + 1 and 4 k + 4) tile nodes 1 .. 6 of the block's node cube: 8 x 27 = 216 distinct nodes, 27 per octant."""
    c = np.array([(x, y, z) for x in (2, 5) for y in (2, 5) for z in (2, 5)], np.float64)
    p = (4.0 * np.asarray(key, np.float64)[None, :] + c + rng.uniform(-jitter, jitter, (8, 3))).astype(np.float32)
    assert (gm.block_keys(p) == np.asarray(key)[None, :]).all()
    return p


def state_for(material, pos, seed, tiers):
    """make_state with the rows that are ill-posed on one of `tiers` re-drawn, as g2p2g_model.scene_state does for its scenes."""
    st = gm.make_state(material, pos.shape[0], seed)
    for draw in range(1, 12):
        bad = gm.ill_posed(material, pos, st, tiers=tiers)
        if not bad.any():
            break
        new = gm.make_state(material, pos.shape[0], seed + 100 * draw)
        for k in ("F32", "b6", "reflected", "logjp"):
            if st[k] is not None:
                st[k][bad] = new[k][bad]
    assert not gm.ill_posed(material, pos, st, tiers=tiers).any()
    return st


def expected(parts_states, models, tier):
    return gm.assemble(models, [gm.bound("stencil", tier, m) for m, _, _ in parts_states])


def assert_untouched_nodes_are_bit_zero(res, exp):
    gk, gb = res["grid"]
    gk, gb = np.asarray(gk).astype(np.int64), np.ascontiguousarray(gb, np.float32)
    cell = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)])
    nodes = gm.pack_nodes(4 * gk[:, None, :] + cell[None, :, :])                      # (blocks, 64)
    untouched = ~np.isin(nodes, exp["key"])
    bits = gb.view(np.uint32).transpose(0, 2, 1)[untouched]                            # (untouched nodes, 4 channels)
    print("grid blocks returned:", gk.shape[0], "untouched nodes in them:", int(untouched.sum()), "not bit-zero:", int((bits != 0).any(axis=1).sum()))
    assert not (bits != 0).any()


def writers_per_node(parts_states, models):
    """Per expected node: the number of particle blocks that contribute to it (each block is one workgroup, one writer)"""
    node, blk = [], []
    for (_, p, _), m in zip(parts_states, models):
        keep = ~m["discarded"] & m["finite"]
        node.append(gm.pack_nodes(m["nodes"][keep]).reshape(-1))
        blk.append(np.repeat(gm.pack_nodes(gm.block_keys(p)[keep]), 27))
    pairs = np.unique(np.stack([np.concatenate(node), np.concatenate(blk)], axis=1), axis=0)
    _, count = np.unique(pairs[:, 0], return_counts=True)
    return count


def run_checked(parts_states, tier, tag):
    res, models = tb.run(parts_states, tier, tag=tag)
    exp = expected(parts_states, models, tier)
    assert_untouched_nodes_are_bit_zero(res, exp)
    return res, models, exp


def corner_scene(material, tier, seed=21):
    pos = corner_particles(KEY, np.random.default_rng(seed))
    return [(material, pos, state_for(material, pos, seed, (tier,)))]


# ---- (a) + (b): one block, eight corner cells ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", MATERIALS)
def test_one_block_fills_all_216_nodes_and_does_so_bit_for_bit_twice(material):
    ps = corner_scene(material, "rest")
    res, models, exp = run_checked(ps, "rest", "corners")
    assert exp["key"].size == 216 and (exp["n"] == 1).all()                            # rest tier: nobody changes its stencil base, every arena node gets one contribution
    lo = 4 * np.asarray(KEY) + 1
    assert (gm.unpack_nodes(exp["key"]).min(axis=0) == lo).all() and (gm.unpack_nodes(exp["key"]).max(axis=0) == lo + 5).all()
    gk, gv = gm.grid_nodes(*res["grid"])
    assert gk.size == 216 and (gv[:, 0] != 0).all()                                    # all 216 nodes carry mass: eight grid blocks, 27 cells each
    assert np.unique(np.asarray(res["grid"][0]).astype(np.int64), axis=0).shape[0] >= 8
    res2, _, _ = run_checked(ps, "rest", "corners again")
    k1, b1 = res["grid"]
    k2, b2 = res2["grid"]
    o1, o2 = np.lexsort(np.asarray(k1).T[::-1]), np.lexsort(np.asarray(k2).T[::-1])
    assert np.array_equal(np.asarray(k1)[o1], np.asarray(k2)[o2])
    assert np.array_equal(np.ascontiguousarray(b1, np.float32)[o1].view(np.uint32), np.ascontiguousarray(b2, np.float32)[o2].view(np.uint32)), "one writer per node: the grids must agree bit for bit"


# ---- (c): shared nodes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", MATERIALS)
def test_two_to_eight_blocks_write_a_node(material):
    rng = np.random.default_rng(22)
    pos = np.concatenate([corner_particles(k, rng) for k in PAIR + GROUP] + [gm.block_particles(k, 24, rng) for k in PAIR + GROUP])
    ps = [(material, pos, state_for(material, pos, 22, ("rest",)))]
    res, models, exp = run_checked(ps, "rest", "pair + group")
    w = writers_per_node(ps, models)
    print("nodes by number of writing blocks:", {int(k): int((w == k).sum()) for k in np.unique(w)})
    assert {2, 4, 8} <= set(w.tolist())


# ---- (d): the low faces ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", MATERIALS)
def test_blocks_against_the_low_faces(material):
    """face_box_cells against x = 0, y = 0, z = 0: the layers from p = 1.75 on (lround(p) >= 2: block 0 along the normal, whose node cube starts at the
    domain's first node), a 6 x 6-cell patch in the middle of the face."""
    boxes = []
    for axis in range(3):
        b = fs.face_box_cells(gm.BITS, axis, "lo", depth=12, width=12)
        boxes.append(b[b[:, axis] >= 1.5])
    pos = np.concatenate(boxes).astype(np.float32)
    assert (gm.block_keys(pos).min(axis=0) == 0).all()
    ps = [(material, pos, state_for(material, pos, 23, ("rest",)))]
    run_checked(ps, "rest", "low faces")


# ---- (e): two models, one grid --------------------------------------------------------------------------------------------------------------
def test_two_models_on_one_grid():
    pa = corner_particles(KEY, np.random.default_rng(24))
    pb = corner_particles(KEY, np.random.default_rng(25))
    ps = [(gm.J_FLUID, pa, state_for(gm.J_FLUID, pa, 24, ("rest",))), (gm.SAND, pb, state_for(gm.SAND, pb, 25, ("rest",)))]
    res, models, exp = run_checked(ps, "rest", "two models")
    assert exp["key"].size == 216 and (exp["n"] == 2).all()


# ---- (f): the gather side ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", MATERIALS)
def test_every_staged_node_reaches_its_particle(material):
    """The flow tier's field: 20 m/s of drift and 5 m/s of per-node noise, so each of the 216 staged nodes holds its own three values and a node staged into the
    wrong arena slot, or from the wrong cell or grid block, moves a particle by ~1e-2 cell against a bound of ~1e-6.  tb.check compares positions and state."""
    ps = corner_scene(material, "flow", seed=26)
    v = gm.gather_field(ps[0][1], "flow")
    flat = v.reshape(-1, 3)
    assert np.unique(flat, axis=0).shape[0] == 216                                     # 8 particles x 27 nodes, all distinct
    run_checked(ps, "flow", "gather")


# ---- (g): both kernels ------------------------------------------------------------------------------------------------------------------------
def test_both_kernels_pass_this_file():
    """Everything above runs in process with the default mask (the pair kernels).  Once more in a fresh child process with MPM_G2P2G_PAIRS=0 - the
    one-particle-per-lane kernel -, under a time limit, deselecting itself there.  A child that ends on a signal fails the test, and nothing else is started."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not test_both_kernels_pass_this_file"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

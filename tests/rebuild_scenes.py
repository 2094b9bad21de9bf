"""The scenes of tests/test_rebuild_books_gpu.py: particle positions (cells), a node-velocity field, and what the float64 model
(tests/g2p2g_model.step) makes of them - new positions, direction tags and the PREDICTED SORT KEY every record must carry.  A scene is a dict
{"name", "tier" (whose position bound the sort-key margin takes), "parts": [(material, pos_cells (n, 3) float32)], "states": [make_state dicts],
"field": nodes (..., 3) int -> (..., 3) float32 m/s}.  tests/test_rebuild_books_cpu.py runs every generator on the model alone (the cap on
particles whose key is decided by a rounding tie, the migrations each scene promises); the GPU test runs the kernels on them.

All scenes: bits 6, max_ppc 16, dt / new_dt of g2p2g_model.

Test infrastructure only."""
import numpy as np

import g2p2g_model as gm

BITS, MAX_PPC = gm.BITS, gm.MAX_PPC
G = 1 << (BITS - 2)
DX = 0.5 ** BITS
SIZES = (1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 767, 768, 769, 1023, 1024)
CELL_PER_STEP = DX / gm.DT                     # m/s that move a particle one cell per substep (640)
TIE_CAP = 0.01                                 # at most this share of a scene's particles may be left out of the sort-key comparison


def tier_field(tier, seed=0):
    return lambda nodes: gm.field(nodes, tier, seed)


def zero_field(nodes):
    return np.zeros(np.asarray(nodes).shape[:-1] + (3,), np.float32)


def grid_of(keys, f):
    """Channels 1 .. 3 of the grid blocks `keys` (n, 3) under the field f: (n, 3, 64) float32, cell = 16 x + 4 y + z (g2p2g_model.grid_of)."""
    keys = np.asarray(keys).astype(np.int64)
    cell = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)])
    return np.ascontiguousarray(np.asarray(f(4 * keys[:, None, :] + cell[None, :, :]), np.float32).transpose(0, 2, 1))


def gather(pos_cells, f):
    """vn of g2p2g_model.step from the field f."""
    return np.asarray(f(gm.stencil_base(pos_cells)[:, None, :] + gm.OFFS[None, :, :]), np.float32)


def model(scene, parts=None, states=None, field=None):
    """g2p2g_model.step per model of the scene (or of the given parts / states / field: a later substep)."""
    parts = scene["parts"] if parts is None else parts
    states = scene["states"] if states is None else states
    f = scene["field"] if field is None else field
    out = []
    for (mat, pos), st in zip(parts, states):
        c = gm.constants(mat, gm.material_overrides(mat, BITS))
        out.append(gm.step(c, pos, gather(pos, f), b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"], bits=BITS))
    return out


def tie_margin(tier, material):
    """A particle is left out of the sort-key comparison only when some axis' rint argument lies this close to a half-integer: the model's own
    position bound, twice, plus the float32 rounding of a value below 8."""
    return 2.0 * gm.bound("pos", tier, material) + 2.0 ** -20


def decided(m, tier, material):
    """Mask over the particles of a step() result: the predicted sort key hangs on no rounding tie."""
    a = m["sort_arg"]
    return (np.abs(a - np.floor(a) - 0.5) >= tie_margin(tier, material)).all(axis=1)


def _scene(name, tier, parts, field, seed):
    return dict(name=name, tier=tier, parts=[(m, np.ascontiguousarray(p, np.float32)) for m, p in parts], field=field,
                states=[gm.make_state(m, p.shape[0], seed + 7 * i) for i, (m, p) in enumerate(parts)])


def _in_block(key, lo, hi, n, rng):
    """n positions in block `key` at offsets [lo, hi) (cells, per axis) from the block's lower bound 4 key + 1.5"""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    p = (4.0 * np.asarray(key, np.float64) + 1.5 + rng.uniform(lo, hi, (n, 3))).astype(np.float32)
    assert (gm.block_keys(p) == np.asarray(key)[None, :]).all()
    return p


# ---- tiers: one particle per block, isolated and at a face, an edge and a corner of the domain --------------------------------------------
FACE_KEYS = [(0, 7, 7), (G - 1, 7, 10), (7, 0, 4), (4, G - 1, 7), (10, 4, 0), (7, 10, G - 1),           # faces
             (0, 0, 10), (G - 1, G - 1, 4), (0, 11, G - 1), (11, 0, G - 1),                               # edges
             (0, 0, 0), (G - 1, G - 1, G - 1), (0, G - 1, 0), (G - 1, 0, G - 1)]                           # corners


def scene_tiers(tier, seed=21):
    """One particle per block on 12 isolated sites and on 14 blocks at faces, edges and corners of the domain.  Along an axis on which its block
    touches the upper face a particle sits in [4 G - 2.3, 4 G - 1.8) - its stencil and the one it will have stay inside the domain -, on the
    lower face in [2, 5): positions that set-up accepts (tests/face_scenes.py goes further out)."""
    rng = np.random.default_rng(seed)
    pts = [_in_block(k, 0.5, 3.5, 1, rng) for k in gm.SITES[:12]]
    for k in FACE_KEYS:
        lo = [0.2 if v == G - 1 else 0.5 for v in k]
        hi = [0.7 if v == G - 1 else 3.5 for v in k]
        pts.append(_in_block(k, lo, hi, 1, rng))
    return _scene(f"tiers_{tier}", tier, [(gm.FC, np.concatenate(pts))], tier_field(tier, seed), seed)


# ---- sizes and keys ---------------------------------------------------------------------------------------------------------------------------
def scene_sizes(material, seed=22):
    """One block per size of SIZES on the first 15 sites, the particles 0.2 cells clear of the block's bounds: under the flow tier (0.17 cells per
    substep at most) nobody leaves, the sizes after the step are SIZES."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([_in_block(k, 0.2, 3.8, n, rng) for k, n in zip(gm.SITES, SIZES)])
    return _scene(f"sizes_{gm.NAMES[material]}", "flow", [(material, pos)], tier_field("flow", seed), seed)


def scene_one_cell(seed=23):
    """g2p2g_model.scene_one_cell: every record of a block has the same key (rest tier: nobody leaves its cell's prediction)."""
    return _scene("one_cell", "rest", [(gm.FC, gm.scene_one_cell())], tier_field("rest", seed), seed)


KEY_BLOCK = (6, 9, 6)
KEY_SPEED = 0.45 * DX / gm.NEW_DT              # the prediction reaches 0.45 cells beyond the position


def key_field(nodes):
    """Diverging from the middle of KEY_BLOCK's node cube along every axis: the particles of its first cells are predicted one cell further down
    (cube coordinate 0), those of its last cells one further up (5) - all 216 keys occur among particles that stay in the block."""
    n = np.asarray(nodes).astype(np.int64)
    mid = 4 * np.asarray(KEY_BLOCK) + 3.5
    return (np.where(n < mid, -KEY_SPEED, KEY_SPEED)).astype(np.float32)


def scene_keys(counts, seed=24, name="keys"):
    """A block whose records carry key k exactly counts[k] times (216 entries): candidates drawn over the block, stepped through the model under
    key_field, and for every key the first counts[k] of those that stay in the block and whose key hangs on no tie.  (Particles do not interact
    within a substep under an injected grid: a subset keeps its keys.)"""
    rng = np.random.default_rng(seed)
    cand = _in_block(KEY_BLOCK, 0.02, 3.98, 60000, rng)
    sc = _scene(name, "fast", [(gm.J_FLUID, cand)], key_field, seed)
    m = model(sc)[0]
    ok = (m["dirtag"] == 13) & decided(m, "fast", gm.J_FLUID) & ~m["discarded"]
    pick = []
    for k, c in enumerate(counts):
        idx = np.flatnonzero(ok & (m["sort_key"] == k))[:c]
        assert idx.size == c, (k, idx.size, c)
        pick.append(idx)
    pick = np.sort(np.concatenate(pick))
    sc["parts"] = [(gm.J_FLUID, cand[pick])]
    sc["states"] = [{k: (v[pick] if v is not None else None) for k, v in sc["states"][0].items()}]
    return sc


def scene_all_keys():
    return scene_keys([4] * 216, name="all_keys")


def scene_odd_keys():
    return scene_keys([(1, 3, 5)[k % 3] for k in range(216)], name="odd_keys")


# ---- migration --------------------------------------------------------------------------------------------------------------------------------
BURST = (6, 6, 6)                              # its particles leave through all 26 borders
SWAP = ((10, 10, 10), (11, 10, 10))            # neighbours along x that swap all their particles
BURST_SPEED = 0.5 * CELL_PER_STEP
SWAP_SPEED = 4.0 * CELL_PER_STEP


def _box(n, lo, hi):
    return ((n >= np.asarray(lo)) & (n <= np.asarray(hi))).all(axis=-1)


def migration_field(nodes):
    n = np.asarray(nodes).astype(np.int64)
    v = np.zeros(n.shape[:-1] + (3,), np.float32)
    # around BURST: per axis -V on its first two node layers and below, +V on its last two and above, 0 on the two in the middle
    o = 4 * np.asarray(BURST)
    near = _box(n, o - 3, o + 10)
    for ax in range(3):
        a = n[..., ax] - o[ax]
        v[..., ax] = np.where(near, np.where(a <= 2, -BURST_SPEED, np.where(a >= 5, BURST_SPEED, 0.0)), 0.0)
    # SWAP: +4 cells per substep on the nodes up to 4 k + 5 of the lower block, -4 cells from 4 k + 6 on
    o = 4 * np.asarray(SWAP[0])
    near = _box(n, o, o + np.array([10, 7, 7]))
    v[..., 0] = np.where(near, np.where(n[..., 0] <= o[0] + 5, SWAP_SPEED, -SWAP_SPEED), v[..., 0])
    return v


def scene_migration(seed=25):
    """BURST: four particles near each of its 26 borders (per axis in the first 0.4 cells, in the block's middle or in the last 0.4 cells), moving
    outward at half a cell per substep: the block is left empty, its 26 neighbours - 19 of them exterior blocks until now - become particle blocks.
    SWAP: 300 particles in the lower three cells of one block, 300 in the upper three of its x-neighbour, displaced by exactly four cells towards
    each other (their stencils see one velocity only): every particle changes block, both blocks stay."""
    rng = np.random.default_rng(seed)
    band = {-1: (0.05, 0.4), 0: (1.6, 2.4), 1: (3.6, 3.95)}
    pts = []
    for d in gm.OFFS - 1:
        if (d == 0).all():
            continue
        lo, hi = zip(*[band[int(c)] for c in d])
        pts.append(_in_block(BURST, lo, hi, 4, rng))
    pts.append(_in_block(SWAP[0], (0.1, 0.1, 0.1), (2.9, 3.9, 3.9), 300, rng))
    pts.append(_in_block(SWAP[1], (1.1, 0.1, 0.1), (3.9, 3.9, 3.9), 300, rng))
    return _scene("migration", "torn", [(gm.J_FLUID, np.concatenate(pts))], migration_field, seed)


# ---- two models -------------------------------------------------------------------------------------------------------------------------------
def scene_two_models(seed=26):
    """The cluster with fixed-corotated and J-fluid particles in the same blocks (flow tier), three isolated blocks that hold only the first model
    and three that hold only the second."""
    rng = np.random.default_rng(seed)
    a = np.concatenate([gm.scene_cluster(seed=seed, lo=150, hi=170)] + [gm.block_particles(k, 70, rng) for k in gm.SITES[:3]])
    b = np.concatenate([gm.scene_cluster(seed=seed + 1, lo=90, hi=110)] + [gm.block_particles(k, 70, rng) for k in gm.SITES[60:63]])
    return _scene("two_models", "flow", [(gm.FC, a), (gm.J_FLUID, b)], tier_field("flow", seed), seed)


def scene_cluster(seed=27):
    """The cluster, J-fluid, flow tier: the first of the substeps of the settled-blocks test."""
    return _scene("cluster", "flow", [(gm.J_FLUID, gm.scene_cluster(seed=seed))], tier_field("flow", seed), seed)


# ---- drop -------------------------------------------------------------------------------------------------------------------------------------
DROP = ((4, 11, 4), (5, 11, 4))


def drop_field(nodes):
    n = np.asarray(nodes).astype(np.int64)
    v = np.zeros(n.shape[:-1] + (3,), np.float32)
    o = 4 * np.asarray(DROP[0])
    v[..., 0] = np.where(_box(n, o, o + np.array([5, 7, 7])), SWAP_SPEED, 0.0)
    return v


def scene_drop(seed=28):
    """Two x-neighbours of 600 particles each; the lower one is displaced by exactly four cells into the upper one, which rests: 1200 arrivals for
    1024 list slots."""
    rng = np.random.default_rng(seed)
    a = _in_block(DROP[0], (0.1, 0.1, 0.1), (2.9, 3.9, 3.9), 600, rng)
    b = _in_block(DROP[1], (1.1, 0.1, 0.1), (3.9, 3.9, 3.9), 600, rng)
    return _scene("drop", "torn", [(gm.J_FLUID, np.concatenate([a, b]))], drop_field, seed)


GENERATORS = {
    "tiers_rest": lambda: scene_tiers("rest"), "tiers_flow": lambda: scene_tiers("flow"),
    "sizes_jfluid": lambda: scene_sizes(gm.J_FLUID), "sizes_sand": lambda: scene_sizes(gm.SAND),
    "one_cell": scene_one_cell, "all_keys": scene_all_keys, "odd_keys": scene_odd_keys,
    "migration": scene_migration, "two_models": scene_two_models, "cluster": scene_cluster, "drop": scene_drop,
}

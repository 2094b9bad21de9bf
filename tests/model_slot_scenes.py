"""The scenes of tests/test_model_slots_cpu.py and tests/test_model_slots_gpu.py: contexts that use all eight model slots (kMaxModels), with
particles in slots 4 .. 7, with empty models in front of, between and behind occupied ones, and with model 0 absent from occupied blocks.

Injected form (scene(name, tier)): a dict like those of tests/rebuild_scenes.py - {"name", "tier", "seed", "parts": [(material, pos_cells (n, 3)
float32)] x 8, "states": [g2p2g_model.make_state dicts] x 8, "field": nodes -> m/s} -, bits 6, max_ppc 16, dt / new_dt of g2p2g_model.
  eight      materials by slot MATERIALS = [FC, SAND, NACC, J_FLUID, J_FLUID, NACC, SAND, FC]: every material's kernel runs once in slots 0 .. 3 and
             once in slots 4 .. 7.  Every model is a cluster of its own seed and size over the 2 x 2 x 2 blocks of g2p2g_model.CLUSTER (all eight
             blocks hold all eight models) plus one private block on its own g2p2g_model.SITES entry, where the other seven have size 0 and bin
             offset 0 - so slot 0 is absent from seven occupied blocks.
  holes      `eight` with slots 0, 3 and 7 empty (n = 0): the first slot, a middle slot and the last slot.
  last_only  seven empty models, particles only in slot 7.
As g2p2g_model.scene_state does, the state of a row that is ill-posed on the rest or the flow tier (on the brink of a sand branch / NACC case, or
with a trial F the reference's SVD does not decompose) is re-drawn until none is left.

Pipeline form (pipeline(name)): a scene dict for claymore_amd.engine.build_engine with the same eight material slots (and for `holes` the same three
empty slots) as small lattice spheres and boxes, thrown at each other in pairs (slots 0-1, 2-3, 4-5, 6-7) under gravity, 4 256 particles in
all.  The second FC (slot 7) and the second SAND (slot 6) have non-default parameters: a kernel that picked up the other slot's MaterialConst
would move their particles differently.

Test infrastructure only."""
import numpy as np

import g2p2g_model as gm
import rebuild_scenes as rs
from claymore_amd import scenes

BITS, MAX_PPC = gm.BITS, gm.MAX_PPC
NSLOTS = 8
MATERIALS = [gm.FC, gm.SAND, gm.NACC, gm.J_FLUID, gm.J_FLUID, gm.NACC, gm.SAND, gm.FC]
HOLES = (0, 3, 7)
TIERS = ("rest", "flow")
SEED = 0                                                        # of the velocity field: the one test_g2p2g_model_cpu.oracle_as_engine runs the oracle in
PRIVATE = [k for k in gm.SITES if k[0] in (3, 12)][:NSLOTS]     # one private block per slot, clear of the cluster's node cubes (keys 6 .. 7, nodes 24 .. 35)
PRIVATE_SIZE = (70, 5, 64, 65, 33, 1, 129, 17)                 # one, two and three bins; a full bin; a single particle
NAMES = ("eight", "holes", "last_only")


def _positions(slot):
    """Slot `slot` of `eight`: a cluster of 12 + 4 slot .. 18 + 4 slot particles per block, and its private block."""
    rng = np.random.default_rng(900 + slot)
    return np.concatenate([gm.scene_cluster(seed=70 + slot, lo=12 + 4 * slot, hi=18 + 4 * slot), rs._in_block(PRIVATE[slot], 0.2, 3.8, PRIVATE_SIZE[slot], rng)])


def occupied(name):
    return {"eight": tuple(range(NSLOTS)), "holes": tuple(s for s in range(NSLOTS) if s not in HOLES), "last_only": (NSLOTS - 1,)}[name]


def _state(material, pos, seed):
    """g2p2g_model.scene_state's rule on given positions: rows ill-posed on a tier of TIERS get the state of a further draw."""
    st = gm.make_state(material, pos.shape[0], seed)
    if pos.shape[0] == 0 or material == gm.J_FLUID:
        return st
    for draw in range(1, 12):
        bad = gm.ill_posed(material, pos, st, tiers=TIERS, seed=SEED)
        if not bad.any():
            break
        new = gm.make_state(material, pos.shape[0], seed + 100 * draw)
        for k in ("F32", "b6", "reflected", "logjp"):
            if st[k] is not None:
                st[k][bad] = new[k][bad]
    assert not gm.ill_posed(material, pos, st, tiers=TIERS, seed=SEED).any()
    return st


_CACHE = {}


def scene(name, tier):
    """The injected form of scene `name` under the field of `tier` (one fixed draw per scene: the tiers share positions and states)."""
    assert name in NAMES and tier in TIERS
    if name not in _CACHE:
        base = scene("eight", tier) if name != "eight" else None    # `holes` and `last_only` are `eight` with models taken out
        parts, states = [], []
        for slot, mat in enumerate(MATERIALS):
            if slot in occupied(name):
                if base is not None:
                    parts.append((mat, base["parts"][slot][1].copy()))
                    states.append({k: (v.copy() if v is not None else None) for k, v in base["states"][slot].items()})
                else:
                    pos = _positions(slot)
                    parts.append((mat, pos))
                    states.append(_state(mat, pos, 300 + 7 * slot))
            else:
                parts.append((mat, np.zeros((0, 3), np.float32)))
                states.append(gm.make_state(mat, 0, 300 + 7 * slot))
        _CACHE[name] = (parts, states)
    parts, states = _CACHE[name]
    return dict(name=name, tier=tier, seed=SEED, field=rs.tier_field(tier, SEED), parts=[(m, p.copy()) for m, p in parts],
                states=[{k: (v.copy() if v is not None else None) for k, v in st.items()} for st in states])


def census(sc):
    """{block key: [particles of slot 0 .. 7]} of a scene's positions"""
    out = {}
    for slot, (_, pos) in enumerate(sc["parts"]):
        for k in map(tuple, gm.block_keys(pos).tolist()):
            out.setdefault(k, [0] * NSLOTS)[slot] += 1
    return out


def models(sc, parts=None, states=None):
    """g2p2g_model.step per slot of the scene at the scenes' default parameters (rebuild_scenes.model).  An empty slot gets the rows [:0] of a
    one-particle result: every array of step() with its dtype and trailing shape, and no row."""
    parts = sc["parts"] if parts is None else parts
    states = sc["states"] if states is None else states
    out = []
    for (mat, pos), st in zip(parts, states):
        if pos.shape[0]:
            out.append(rs.model(sc, parts=[(mat, pos)], states=[st])[0])
        else:
            one = rs._in_block(gm.SITES[0], 1.0, 3.0, 1, np.random.default_rng(0))
            m = rs.model(sc, parts=[(mat, one)], states=[gm.make_state(mat, 1, 0)])[0]
            out.append({k: v[:0] for k, v in m.items()})
    return out


# ---- the pipeline form ----------------------------------------------------------------------------------------------------------------------------
PAIR_SITES = ((20, 22), (20, 44), (44, 22), (44, 44))           # (y, z) of the four pairs, in cells
PAIR_SPEED = 2.0                                                # m/s towards each other: 0.77 cells each in 60 substeps of 1e-4, the gap is 1.25 cells
PIPELINE_DT = 1e-4
PIPELINE_STEPS = 60
SECOND_FC = dict(youngs_modulus=2e4, poisson_ratio=0.3, rho=2e3)
SECOND_SAND = dict(youngs_modulus=2e4, poisson_ratio=0.3, cohesion=0.05, beta=0.5, yield_surface=0.21012822)    # material_variants S3: friction angle 20 degrees


def pipeline(name):
    """Eight bodies in four pairs along x, a sphere of radius 2.5 cells (552 particles) on the left and a box of 4^3 nodes (512 particles) on the
    right of each, 1.25 cells apart, thrown at each other at PAIR_SPEED under the default gravity."""
    assert name in ("eight", "holes")
    dx = 0.5 ** BITS
    vol = scenes._vol(BITS)
    out = []
    for slot, mat in enumerate(MATERIALS):
        y, z = PAIR_SITES[slot // 2]
        if slot % 2 == 0:
            xyz = scenes.lattice_sphere(BITS, ((32 - 3.0) * dx, y * dx, z * dx), 2.5)
        else:
            xyz = scenes.lattice_box(BITS, np.array([33, y - 2, z - 2]), np.array([37, y + 2, z + 2]))
        if slot not in occupied(name):
            xyz = xyz[:0]
        prm = {"volume": vol}
        if mat == gm.FC:
            prm.update(youngs_modulus=5e3, poisson_ratio=0.4, rho=1e3)
        if slot == 7:
            prm.update(SECOND_FC)
        if slot == 6:
            prm.update(SECOND_SAND)
        out.append({"material": mat, "xyz": np.ascontiguousarray(xyz, np.float32), "v0": (PAIR_SPEED if slot % 2 == 0 else -PAIR_SPEED, 0.0, 0.0), "params": prm})
    return {"name": "model_slots_" + name, "bits": BITS, "dt": PIPELINE_DT, "config": {}, "models": out}

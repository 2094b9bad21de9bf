"""Persistent particle identities on the GPU (claymore_amd/csrc/mpm_particle_ids.hpp, mpm_track_particle_ids / mpm_retrieve_ids /
mpm_particle_ids_save / _load): an id is the particle's index in the array its model was added with, and it follows the particle through
set-up, every G2P2G path, capacity growth and a checkpoint.  Every identity check is exact integer equality.

Three independent witnesses:
  * set-up: the id readout's positions against the input array, bit for bit;
  * one substep against the host model (tests/particle_ids_model.py), which predicts the next id blob from ONE checkpoint and its blob alone,
    on the block shapes at which the list walk can go wrong, with deformed state injected through the checkpoint;
  * a rigidly translating lattice, whose sites are recovered from the final positions by rounding - a ground truth that uses no list at all."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import ckpt_format as cf
import g2p2g_model as gm
import particle_ids_model as pim
from claymore_amd import _ffi
from claymore_amd.engine import Engine, EngineError, build_engine, join_by_position
from claymore_amd.mgsp import MgspRank, partition_scene
from test_g2p2g_blocks_gpu import Bench

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MATERIALS = (_ffi.J_FLUID, _ffi.FIXED_COROTATED, _ffi.SAND, _ffi.NACC)         # nch 4, 9, 10, 10


def bits_of(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def sorted_rows(a):
    a = np.ascontiguousarray(a)
    flat = a.reshape(a.shape[0], -1).view(np.uint32)
    return flat[np.lexsort(flat.T[::-1])]


# ---- 1. set-up -----------------------------------------------------------------------------------------------------------------------------
def check_setup(eng, inputs):
    for m, xyz_in in enumerate(inputs):
        n = xyz_in.shape[0]
        xyz, ids = eng.retrieve_ids(m)
        assert ids.dtype == np.int32 and xyz.shape == (n, 3)
        assert np.array_equal(np.sort(ids), np.arange(n)), "the ids after set-up are not exactly 0 .. n-1"
        xs, _, _ = eng.retrieve_state(m)
        # retrieve_state's position of input particle j: found by its bits among the state readout's rows (the set-up stores x / dx and the
        # readout multiplies by dx, both exact)
        assert np.array_equal(sorted_rows(xs), sorted_rows(xyz_in)), "retrieve_state does not return the input positions bit for bit"
        assert np.array_equal(bits_of(xyz), bits_of(xyz_in[ids])), "xyz[k] is not the position of input particle ids[k]"


@pytest.mark.parametrize("material", MATERIALS)
def test_setup_ids_index_the_input_array(material):
    """Blocks of 1 .. 1024 particles (several bins per block, the last one partial), every material's record format."""
    pos = gm.scene_block_sizes()
    xyz = pos * np.float32(0.5 ** gm.BITS)
    sc = {"name": "ids_setup", "bits": gm.BITS, "dt": gm.DT, "config": {"max_ppc": gm.MAX_PPC}, "track_ids": True,
          "models": [{"material": material, "xyz": xyz, "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(material))}]}
    eng = build_engine(sc)
    try:
        eng.initial_setup()
        check_setup(eng, [xyz])
    finally:
        eng.close()


def test_setup_two_models_on_one_grid():
    a = gm.scene_cluster() * np.float32(0.5 ** gm.BITS)
    b = gm.scene_cluster(seed=44, lo=90, hi=110) * np.float32(0.5 ** gm.BITS)
    sc = {"name": "ids_setup2", "bits": gm.BITS, "dt": gm.DT, "config": {"max_ppc": gm.MAX_PPC}, "track_ids": True,
          "models": [{"material": _ffi.FIXED_COROTATED, "xyz": a, "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(_ffi.FIXED_COROTATED))},
                     {"material": _ffi.J_FLUID, "xyz": b, "v0": (0.0, 0.0, 0.0), "params": dict(gm.material_overrides(_ffi.J_FLUID))}]}
    eng = build_engine(sc)
    try:
        eng.initial_setup()
        check_setup(eng, [a, b])
    finally:
        eng.close()


# ---- 2. one substep against the host model ---------------------------------------------------------------------------------------------------
class IdBench(Bench):
    """tests/test_g2p2g_blocks_gpu.Bench on a context that tracks ids."""

    def __init__(self, parts, bits=gm.BITS, max_ppc=gm.MAX_PPC):
        self.bits, self.dx = bits, 0.5 ** bits
        self.parts = [(m, np.ascontiguousarray(p, np.float32)) for m, p in parts]
        self.over = [gm.material_overrides(m, bits) for m, _ in self.parts]
        sc = {"name": "ids_blocks", "bits": bits, "dt": gm.DT, "config": {"max_ppc": max_ppc}, "track_ids": True,
              "models": [{"material": m, "xyz": p * np.float32(self.dx), "v0": (0.0, 0.0, 0.0), "params": dict(o)} for (m, p), o in zip(self.parts, self.over)]}
        self.eng = build_engine(sc)
        self.eng.initial_setup()
        self.ckpt = self.eng.save_checkpoint().copy()
        self.ids0 = self.eng.save_particle_ids().copy()


def scene_id_sizes(seed=21):
    """One block each of 1, 63, 64, 65 (the bin boundary) and 1024 particles (two 512-record chunks / the merged 256-record tail)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([gm.block_particles(k, n, rng) for k, n in zip(gm.SITES, (1, 63, 64, 65, 1024))])


SHAPES = {
    "sizes": lambda: ([(gm.FC, scene_id_sizes())], "flow"),
    "one_cell": lambda: ([(gm.FC, gm.scene_one_cell())], "flow"),                       # 513 in one cell: all-equal sort keys
    "cluster_sand": lambda: ([(gm.SAND, gm.scene_cluster())], "fast"),                  # 2 x 2 x 2 blocks, particles that change block
    "cluster_nacc": lambda: ([(gm.NACC, gm.scene_cluster())], "flow"),
    "mixed": lambda: ([(gm.FC, gm.scene_cluster()), (gm.J_FLUID, gm.scene_cluster(seed=44, lo=90, hi=110))], "flow"),   # two materials, one grid
    "torn": lambda: ([(gm.J_FLUID, gm.scene_torn())], "torn"),                          # particles leave; the discard path
}


def inject(bench, states, tier, as_momentum):
    """The set-up checkpoint with deformed state patched in (positions, and so every list, untouched) and the tier's velocity field in the grid
    - as velocities for a bare mpm_g2p2g, as momenta (velocity x the node's mass) for a run that starts with a grid update -, loaded; then its ids."""
    buf = bench.ckpt
    for i, ((m, p), st) in enumerate(zip(bench.parts, states)):
        buf = cf.with_particle_state(buf, i, p, J=st["J"]) if m == gm.J_FLUID else cf.with_particle_state(buf, i, p, b=st["b6"], logjp=st["logjp"], reflected=st["reflected"])
    g = cf.grid(buf).copy()
    v = gm.grid_of(cf.cur_keys(buf)[:g.shape[0]], tier)
    g[:, 1:4] = v * g[:, 0:1] if as_momentum else v
    bench.eng.load_checkpoint(cf.with_grid(buf, g))
    with pytest.raises(EngineError) as e:
        bench.eng.retrieve_ids(0)
    assert e.value.code == _ffi.MPM_ERR_INVALID
    with pytest.raises(EngineError):
        bench.eng.save_particle_ids()
    bench.eng.load_particle_ids(bench.ids0)


@pytest.mark.parametrize("mode", ["phases", "run_fixed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_substep_against_the_host_model(shape, mode):
    """Checkpoint and id blob at step k, one substep, the blob at k + 1: every slot the model names holds the id the model predicts.  Three
    substeps, each predicted from the state read back; phase-level calls (mpm_g2p2g + mpm_rebuild_partition) and mpm_run_fixed(1)."""
    parts, tier = SHAPES[shape]()
    bench = IdBench(parts)
    try:
        states = [gm.make_state(m, p.shape[0], 7 + i) for i, (m, p) in enumerate(parts)]
        inject(bench, states, tier, as_momentum=mode == "run_fixed")
        eng = bench.eng
        moved = 0
        for k in range(3):
            ck, blob = eng.save_checkpoint().copy(), eng.save_particle_ids().copy()
            d0 = eng.diagnostics()
            lost0, disc0 = int(d0.lost_particles) + int(d0.dropped_particles), int(d0.discarded_p2g)
            if mode == "run_fixed":
                eng.run_fixed(1, gm.DT)
            else:
                if k:
                    eng.grid_update(gm.DT)
                eng.g2p2g(gm.DT, gm.NEW_DT)
                eng.rebuild_partition()
            d1 = eng.diagnostics()
            lost = int(d1.lost_particles) + int(d1.dropped_particles) - lost0
            after = pim.unpack(eng.save_particle_ids())
            h = cf.parse(ck)
            ppb = cf.K_BIN * h["max_ppc"]
            for m, (_, p) in enumerate(parts):
                exp, live = pim.expected_blob_slots(ck, blob, m)
                n_after, got = after[m]
                assert n_after == p.shape[0] and got.size == exp.size, (shape, mode, k, m, got.size, exp.size)
                wrong = np.flatnonzero(got[live] != exp[live])
                print(f"{shape} {mode} step {k} model {m}: {int(live.sum())} live slots, {wrong.size} wrong, lost {lost}, discarded {int(d1.discarded_p2g) - disc0}")
                assert wrong.size == 0, (shape, mode, k, m, wrong[:8].tolist(), got[live][wrong[:8]].tolist(), exp[live][wrong[:8]].tolist())
                tags = (cf.section(ck, h, ("lists", m), np.int32).view(np.uint32) >> np.uint32(ppb.bit_length() - 1 + cf.K_KEY_BITS)) & np.uint32(31)
                moved += int((tags != 13).sum())
                xyz, ids = eng.retrieve_ids(m)
                assert ids.size == int(eng.counts().particles[m]) and np.unique(ids).size == ids.size
                if lost == 0:
                    assert np.array_equal(np.sort(ids), np.sort(pim.live_ids(ck, blob, m)))
            if shape == "torn" and k == 0:
                assert int(d1.discarded_p2g) - disc0 >= 1, "the torn tier discards contributions"
        if shape in ("cluster_sand", "cluster_nacc", "mixed", "torn"):
            assert moved > 0, "no record of steps 2 and 3 carried a neighbour tag: no particle changed block"
    finally:
        bench.close()


# ---- 3. rigid translation --------------------------------------------------------------------------------------------------------------------
BITS = 7
DX = 0.5 ** BITS
CELLS = 20
SITES_PER_AXIS = 2 * CELLS
FIRST = np.array([40.3, 60.1, 50.7]) + 0.25               # the first lattice site, in cells
V0 = (0.9, -1.3, 0.6)
DT = 1e-4
RESIDUAL = 0.05                                           # cells; half the lattice spacing is 0.25, the oracle's largest residual 1e-4


def lattice_scene(material, track=True, stride=1, **config):
    """A 20^3-cell block, two particles per cell and axis (stride 1: 64 000); id = (i * 40 + j) * 40 + k of site (i, j, k)."""
    s = np.arange(0, SITES_PER_AXIS, stride)
    ijk = np.stack(np.meshgrid(s, s, s, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz = ((FIRST[None, :] + 0.5 * ijk) * DX).astype(np.float32)
    return {"name": "ids_lattice", "bits": BITS, "dt": DT, "config": dict(config), "track_ids": track,
            "models": [{"material": material, "xyz": xyz, "v0": V0, "params": {}}]}, ijk


def check_sites(xyz0, xyz, ids, tag=""):
    """After subtracting the mean displacement every particle's lattice site is recovered by rounding and must be the site of input particle
    ids[k]; the ids are a full permutation."""
    n = xyz0.shape[0]
    assert ids.size == n and np.array_equal(np.sort(ids), np.arange(n)), (tag, "the ids are not a permutation of the input indices")
    x0 = xyz0.astype(np.float64) / DX
    x = xyz.astype(np.float64) / DX
    disp = x.mean(axis=0) - x0.mean(axis=0)
    site = (x - disp[None, :] - FIRST[None, :]) / 0.5
    residual = float(np.abs(site - np.rint(site)).max() * 0.5)
    want = np.rint((x0[ids] - FIRST[None, :]) / 0.5).astype(np.int64)
    wrong = int((np.rint(site).astype(np.int64) != want).any(axis=1).sum())
    print(f"{tag}: displacement {disp.round(3).tolist()} cells, residual {residual:.3g} cell, {wrong} of {n} ids name another site")
    assert residual < RESIDUAL, (tag, residual)
    assert wrong == 0, (tag, wrong)
    return disp


def run_lattice(material, nsteps=400, window=50, **config):
    sc, _ = lattice_scene(material, **config)
    eng = build_engine(sc)
    try:
        eng.initial_setup()
        for _ in range(nsteps // window):
            eng.run_fixed(window, DT)
        xyz, ids = eng.retrieve_ids(0)
        return sc["models"][0]["xyz"], xyz, ids, eng.capacity()
    finally:
        eng.close()


@pytest.mark.parametrize("material", MATERIALS)
def test_rigid_translation_ids_name_their_lattice_sites(material):
    """400 substeps of free fall with v0 = (0.9, -1.3, 0.6): the block moves (4.6, -7.7, 3.1) cells and crosses block faces on every axis."""
    xyz0, xyz, ids, _ = run_lattice(material)
    disp = check_sites(xyz0, xyz, ids, f"material {material}")
    assert np.abs(disp - np.array([4.6, -7.7, 3.1])).max() < 0.1, disp


def test_rigid_translation_with_the_sliced_list_layout():
    """The same in a fresh child process with MPM_G2P2G_PAIRS=0 (read once per process): the one-particle kernel and the sliced lists."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "pytest", os.path.abspath(__file__) + "::test_rigid_translation_ids_name_their_lattice_sites[%d]" % _ffi.SAND,
                        "-m", "gpu", "-q", "-x", "-s", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, cwd=ROOT)
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and "1 passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])


# ---- 4. capacity growth ---------------------------------------------------------------------------------------------------------------------
def test_ids_survive_capacity_growth():
    """The same scene with max_blocks just above the exterior block count of the set-up: the context passes the 3/4 mark, the block arrays and
    with them the bins - and the id arrays - are reallocated during the run."""
    sc, _ = lattice_scene(_ffi.FIXED_COROTATED)
    probe = build_engine(sc)
    probe.initial_setup()
    ebc = probe.counts().exterior_blocks
    probe.close()
    xyz0, xyz, ids, cap = run_lattice(_ffi.FIXED_COROTATED, max_blocks=ebc + ebc // 8)
    print("capacity:", cap, "exterior blocks at set-up:", ebc)
    assert cap[2] >= 1, "no growth event: the scene does not test what it is meant to"
    check_sites(xyz0, xyz, ids, "growth")


# ---- 5. tracking changes nothing else ------------------------------------------------------------------------------------------------------
def run_observables(track, nsteps=50):
    # one particle every fourth cell: no two stencils share a node, the float atomics of P2G have nothing to reorder and the engine is
    # deterministic (tests/test_collision_clock_gpu.py), which a bit-for-bit comparison of two runs needs - two runs of the dense lattice differ
    # from each other in the last bits with or without tracking
    sc, _ = lattice_scene(_ffi.FIXED_COROTATED, track=track, stride=8)
    eng = build_engine(sc)
    try:
        eng.initial_setup()
        eng.run_fixed(nsteps, DT)
        x, st, lj = eng.retrieve_state(0)
        keys, blocks = eng.dump_grid()
        c = eng.counts()
        rows = np.concatenate([x, st, lj[:, None]], axis=1)
        grid = np.concatenate([keys.astype(np.float32).view(np.uint32).reshape(len(keys), -1), blocks.reshape(len(keys), -1).view(np.uint32)], axis=1)
        return sorted_rows(rows), grid[np.lexsort(keys.T[::-1])], (c.particle_blocks, c.neighbor_blocks, c.exterior_blocks, int(c.particles[0]), int(c.bins[0]))
    finally:
        eng.close()


def test_tracking_changes_no_other_output():
    a, b, t = run_observables(False), run_observables(False), run_observables(True)
    assert a[0].shape[0] == 125
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], "the scene is not deterministic: nothing to compare"
    assert np.array_equal(a[0], t[0]), "retrieve_state differs with tracking on"
    assert np.array_equal(a[1], t[1]), "the grid differs with tracking on"
    assert a[2] == t[2], (a[2], t[2])


# ---- 6. groups -----------------------------------------------------------------------------------------------------------------------------
def check_rank_sites(sc, world, results, tag):
    total = 0
    for r, (xyz, ids) in enumerate(results):
        xyz0 = partition_scene(sc, r, world)["models"][0]["xyz"]
        assert xyz0.shape[0] > 0
        check_sites(xyz0, xyz, ids, f"{tag} rank {r}")
        total += ids.size
    assert total == sc["models"][0]["xyz"].shape[0]


def test_group_ranks_carry_rank_local_ids():
    """LocalGroup(2) on one GPU, the lattice cut across x (the block crosses the cut), 200 substeps through MgspGroupRank.run_fixed."""
    from test_group_velocity_gpu import run_group
    sc, _ = lattice_scene(_ffi.FIXED_COROTATED)

    def script(sim):
        sim.initial_setup()
        for _ in range(4):
            sim.run_fixed(50, DT)
        return sim.retrieve_ids(0)
    check_rank_sites(sc, 2, run_group(sc, 2, script), "group")


def test_phase_level_halo_and_interior_passes_move_the_ids():
    """Two contexts on one GPU driven phase by phase (mpm_g2p2g_halo with its exact block list, mpm_g2p2g_interior with its flags) and through the
    fused substep (mpm_mgsp_begin): the thread communicator of tests/test_mgsp_gpu.py stands in for RCCL."""
    from test_mgsp_gpu import ThreadComm
    sc, _ = lattice_scene(_ffi.FIXED_COROTATED)
    world, group = 2, ThreadComm(2)
    results, errors, halo = [None] * world, [], [0] * world

    def work(rank):
        try:
            sim = MgspRank(sc, rank, world, device=0, comm=group.view(rank))
            sim.initial_setup()
            for k in range(60):
                (sim.substep_phased if k < 40 else sim.substep)(DT, DT)
                halo[rank] = max(halo[rank], sim.n_halo_blocks)
            results[rank] = sim.eng.retrieve_ids(0)
            sim.close()
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))
            group.bar.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errors, errors
    assert min(halo) > 0, "no particle block went through the halo-first pass"
    check_rank_sites(sc, world, results, "phased")


# ---- 7. the checkpoint rule and the errors ----------------------------------------------------------------------------------------------------
def test_checkpoint_rule_and_errors():
    sc, _ = lattice_scene(_ffi.FIXED_COROTATED, stride=2)                 # 8 000 particles
    plain = build_engine(dict(sc, track_ids=False))
    eng = build_engine(sc)
    ref = build_engine(sc)
    try:
        for e in (plain, eng, ref):
            e.initial_setup()
        # an untracked context refuses; tracking cannot be switched on after set-up
        for call in (lambda: plain.retrieve_ids(0), plain.save_particle_ids, lambda: plain.load_particle_ids(np.zeros(144, np.uint8))):
            with pytest.raises(EngineError) as err:
                call()
            assert err.value.code == _ffi.MPM_ERR_INVALID
        for e in (plain, eng):
            assert e.api.track_particle_ids(e.ctx, 1) == _ffi.MPM_ERR_INVALID
        blob0 = eng.save_particle_ids().copy()
        eng.run_fixed(100, DT)
        ref.run_fixed(100, DT)
        ck, blob = eng.save_checkpoint().copy(), eng.save_particle_ids().copy()
        assert pim.unpack(blob)[0][1].size != pim.unpack(blob0)[0][1].size, "the two blobs' headers agree: nothing to refuse"
        eng.run_fixed(7, DT)                                                # (anything: the state is replaced)
        eng.load_checkpoint(ck)
        for call in (lambda: eng.retrieve_ids(0), eng.save_particle_ids):
            with pytest.raises(EngineError) as err:
                call()
            assert err.value.code == _ffi.MPM_ERR_INVALID
        with pytest.raises(EngineError) as err:                             # a blob from another step count: its header does not match
            eng.load_particle_ids(blob0)
        assert err.value.code == _ffi.MPM_ERR_INVALID
        with pytest.raises(EngineError):
            eng.load_particle_ids(blob[:-4])
        bad = blob.copy()
        bad[0] ^= 1
        with pytest.raises(EngineError):
            eng.load_particle_ids(bad)
        with pytest.raises(EngineError):
            eng.retrieve_ids(0)                                             # still refused: none of those loads succeeded
        eng.load_particle_ids(blob)
        eng.run_fixed(100, DT)
        ref.run_fixed(100, DT)
        xa, ia = eng.retrieve_ids(0)
        xb, ib = ref.retrieve_ids(0)
        xyz0 = sc["models"][0]["xyz"]
        # the same ids per particle as an uninterrupted run: each run's ids name the lattice sites (the two runs' position bits differ in the
        # last places on a dense body - float atomics in P2G -, so the particles are matched by site, which is exact)
        check_sites_stride = lambda x, i, tag: check_sites(xyz0, x, i, tag)
        check_sites_stride(xa, ia, "restarted")
        check_sites_stride(xb, ib, "uninterrupted")
        oa, ob = np.argsort(ia), np.argsort(ib)
        assert np.abs(xa[oa].astype(np.float64) - xb[ob].astype(np.float64)).max() < 1e-3 * DX
        # and order_by_id hands any readout back in id order
        xs, st, lj = eng.retrieve_state(0)
        ids, x_sorted, st_sorted = eng.order_by_id(0, xs, st)
        assert np.array_equal(ids, np.arange(xyz0.shape[0])) and np.array_equal(bits_of(x_sorted), bits_of(xa[oa]))
        assert np.array_equal(sorted_rows(np.concatenate([xs, st], axis=1)), sorted_rows(np.concatenate([x_sorted, st_sorted], axis=1)))
    finally:
        for e in (plain, eng, ref):
            e.close()


def test_order_by_id_hands_out_identical_positions_in_id_order():
    idx = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.125, 0.25, 0.5]], np.float32)
    ids = np.array([3, 1, 0, 2], np.int32)
    xyz = idx[[1, 0, 3, 2]]
    val = np.array([10.0, 20.0, 30.0, 40.0])
    got_ids, got_xyz, got_val = join_by_position(idx, ids, xyz, val)
    assert got_ids.tolist() == [0, 1, 2, 3]
    assert got_val.tolist() == [20.0, 10.0, 30.0, 40.0]                   # the two rows at (0.5, 0.5, 0.5) as they stand: 20 to id 0, 40 to id 3
    assert np.array_equal(got_xyz, idx[[2, 1, 3, 0]])
    with pytest.raises(ValueError):
        join_by_position(idx, ids, xyz + np.float32(0.125), val)


# ---- 9. gmpm ---------------------------------------------------------------------------------------------------------------------------------
def test_gmpm_output_ids(tmp_path):
    """simulation.output_ids on the two-box scene of tests/test_gmpm_stress_gpu.py (one particle block each: deterministic), two frames: "id" is
    0 .. n-1 ascending in every frame, the positions are Engine.order_by_id's of the same run, beside "v" too; without the key the frames are
    the position-only ones, byte for byte."""
    import struct
    import __graft_entry__ as g
    from bgeo_reader import read_bgeo
    import test_gmpm_stress_gpu as G
    g.build_host()
    plain = G.run_gmpm(tmp_path / "plain")
    with_ids = G.run_gmpm(tmp_path / "ids", output_ids=True)
    both = G.run_gmpm(tmp_path / "both", output_ids=True, output_velocity=True)
    start = [read_bgeo(G.frame(plain, m, 0))[0] for m in range(len(G.MODELS))]
    # the same main loop on a tracked Engine
    eng = Engine(domain_bits=G.BITS, max_ppc=128, track_ids=True)
    try:
        for mod, xyz in zip(G.MODELS, start):
            mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
            eng.init_model(mat, xyz, mod["velocity"], **({k: G.FC[k] for k in G.FC} if mat == _ffi.FIXED_COROTATED else {}))
        spf = np.float32(1.0) / np.float32(G.FPS)
        max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in G.MODELS)
        dt = eng.compute_dt(max_v0, 0.0, float(spf), G.DT_DEFAULT)
        eng.initial_setup()
        for f in range(0, G.FRAMES + 1):
            if f:
                t = np.float32(0.0)
                while t < spf:
                    next_dt, _ = eng.substep(dt, float(t), float(spf), G.DT_DEFAULT)
                    t = np.float32(t + np.float32(dt))
                    dt = next_dt
            for m in range(len(G.MODELS)):
                n = start[m].shape[0]
                xv, v = eng.retrieve_velocity(m)
                ids, x_sorted, v_sorted = eng.order_by_id(m, xv, v)
                assert np.array_equal(ids, np.arange(n))
                for d in (with_ids, both):
                    x, attrs, order = read_bgeo(G.frame(d, m, f))
                    assert order == ([("v", 3, 5)] if d is both else []) + [("id", 1, 1)]
                    assert np.array_equal(attrs["id"][:, 0], np.arange(n)), (f, m, "the id attribute is not 0 .. n-1 ascending")
                    assert np.array_equal(bits_of(x), bits_of(x_sorted)), (f, m, "the frame's positions are not order_by_id's")
                    if d is both and f:
                        assert np.array_equal(bits_of(attrs["v"]), bits_of(v_sorted))
                # without the key: the position-only frame, every byte of it
                xp, ap, _ = read_bgeo(G.frame(plain, m, f))
                assert ap == {} and np.array_equal(sorted_rows(xp), sorted_rows(x_sorted))
                want = struct.pack(">IcII7I", 0x4267656F, b"V", 5, n, 0, 0, 0, 0, 0, 0, 0) + np.concatenate([xp, np.ones((n, 1), np.float32)], axis=1).astype(">f4").tobytes() + b"\x00\xff"
                assert open(G.frame(plain, m, f), "rb").read() == want
    finally:
        eng.close()

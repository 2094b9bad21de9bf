"""The halo kernels of claymore_amd/csrc/mpm_halo.inc (halo_export / halo_mark / halo_split / halo_collect / halo_reduce) one by one
against tests/halo_model.py, the plain set-level model that tests/test_halo_model_cpu.py checks against the CPU oracle.  Everything is
compared by block key; every comparison is exact (integers, float32 bit patterns) except where a derived bound is stated.
Scenes: bits 6, about 10^4 particles (halo_model.halo_scene).

Kernel mutations tried against this file on an MI355X (not committed) and the tests that failed, each with ordinary assertion failures:
  `1 << peer` -> `1 << (peer & 15)` in halo_mark_kernel     8 tests, through check_dump's marks (0x8000 where 0x80000000 is expected):
                                                              test_main_tagging..., test_list_lengths..., test_split_by_identity... (both
                                                              scenes each), test_tagging_and_collect_of_a_rebuilt_partition,
                                                              test_fused_path_truncated_peer...
  `b < nbc` -> `b < cfg.cap` in halo_mark_kernel            8 tests, through the send counts (exterior-only keys get sent): test_main_tagging...,
                                                              test_list_lengths... (both scenes), ...rebuilt_partition,
                                                              test_collect_capacity..., test_two_real_contexts..., test_fused_path_truncated_peer...
  `halo = true` only for i == 0 in halo_split_kernel        3 tests, through the halo count / identity: test_split_by_identity... (both scenes),
                                                              test_fused_path_truncated_peer...
  `i >= n` -> `i > n - 2` in halo_reduce_kernel             9 tests: test_reduce_one_addend... at nrecv 1, 3, 4, 5, 64 (whenever the last key
                                                              is an own block), test_two_real_contexts...
  `q != rank` dropped from halo_collect_kernel's offset     none: equivalent.  send_counts[rank] is always 0 (halo_mark_kernel returns for the own
                                                              rank after the export cleared the counters); only the group loop uses the
                                                              packed layout, which test_cpp_group_16_ranks_equals_oracle runs end to end
(the 40-substep phantom runs, the status words and the 16-rank group were left out of the mutation runs)"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import halo_model as hm
from claymore_amd import _ffi, mgsp
from claymore_amd.engine import EngineError, build_engine
from claymore_amd.mgsp import ROW, MgspRank
from oracle_ffi import oracle_api
from parity_util import match, run_engine

pytestmark = pytest.mark.gpu

POS_TOL = 1e-5      # the relative position bound of every parity test of this suite (tests/test_parity_gpu.py)
DT = 1e-4
CANARY = -7


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class HipRank:
    """One HIP context driven through the phase-level halo calls with torch device tensors (as claymore_amd/mgsp.py does)."""

    def __init__(self, scene, nsteps=0):
        self.eng = build_engine(scene)
        self.api, self.ctx = self.eng.api, self.eng.ctx
        self.eng.initial_setup()
        if nsteps:
            self.eng.run_fixed(nsteps, DT)

    def ok(self, rc):
        assert rc == 0, (rc, self.api.last_error(self.ctx).decode())

    def model(self):
        c = self.eng.counts()
        keys = torch.zeros((c.neighbor_blocks, 3), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cnt = C.c_int(0)
        self.ok(self.api.halo_keys(self.ctx, _ptr(keys), c.neighbor_blocks, C.byref(cnt)))
        self.ok(self.api.sync(self.ctx))
        assert cnt.value == c.neighbor_blocks
        return hm.HaloModel(keys.cpu().numpy(), c.particle_blocks, hm.G_BLOCKS)

    def tag(self, lists):
        self.ok(self.api.halo_tag_begin(self.ctx))
        keep = []
        for p, lst in lists.items():
            lst = np.asarray(lst, dtype=np.int32).reshape(-1, 3)
            t = _dev(lst if len(lst) else np.zeros((1, 3), np.int32))
            keep.append(t)
            self.ok(self.api.halo_tag_peer(self.ctx, p, _ptr(t), len(lst)))
        nh, sc = C.c_int(-1), (C.c_int * 32)()
        self.ok(self.api.halo_tag_end(self.ctx, C.byref(nh), sc))
        return nh.value, list(sc)

    def dump(self, model):
        ov = np.full(model.nbc, CANARY, np.int32)
        hl = np.full(model.pbc + 1, CANARY, np.int32)
        fl = np.full(model.pbc + 1, CANARY, np.int32)
        n = C.c_int(-1)
        self.ok(self.api.halo_dump(self.ctx, C.c_void_p(ov.ctypes.data), C.c_void_p(hl.ctypes.data), C.byref(n), C.c_void_p(fl.ctypes.data)))
        assert 0 <= n.value <= model.pbc and (hl[n.value:] == CANARY).all() and fl[model.pbc] == CANARY
        return ov, hl[:n.value], fl[:model.pbc]

    def collect(self, peer, capacity, gid=0):
        """-> rc, nsend, keys, blocks; the buffers have one canary row in front and at least one behind."""
        keys = torch.full((capacity + 2, 3), CANARY, dtype=torch.int32, device="cuda")
        blocks = torch.full((capacity + 2, 256), float(CANARY), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ns = C.c_int(-1)
        rc = self.api.halo_collect(self.ctx, peer, gid, _ptr(keys[1:]), _ptr(blocks[1:]), capacity, C.byref(ns))
        self.ok(self.api.sync(self.ctx))
        return rc, ns.value, keys.cpu().numpy(), blocks.cpu().numpy()

    def reduce(self, keys, blocks, gid=0):
        k, b = _dev(np.asarray(keys, dtype=np.int32)), _dev(np.asarray(blocks, dtype=np.float32))
        self.ok(self.api.halo_reduce(self.ctx, gid, _ptr(k), _ptr(b), len(keys)))
        self.ok(self.api.sync(self.ctx))

    def grid(self):
        return hm.grid_dict(*self.eng.dump_grid())

    def close(self):
        self.eng.close()


def check_dump(rank, model, t):
    """The marks word by word (unsigned: bit 31 included), the halo list as a duplicate-free set, the interior flags by identity."""
    ov, hl, fl = rank.dump(model)
    for i, k in enumerate(model.keys):
        assert int(np.uint32(ov[i])) == t.overlap.get(k, 0), (k, hex(int(np.uint32(ov[i]))), hex(t.overlap.get(k, 0)))
    assert ((hl >= 0) & (hl < model.pbc)).all() and len(set(hl.tolist())) == len(hl)
    halo = {model.keys[b] for b in hl}
    assert halo == t.halo_blocks
    assert set(fl.tolist()) <= {0, 1}
    interior = {model.keys[b] for b in range(model.pbc) if fl[b] == 1}
    assert interior == t.interior_blocks
    assert halo | interior == set(model.particle) and not (halo & interior)


def check_collect(rank, model, t, grid=None, peers=range(32)):
    """For every peer the collected keys are the model's send set, once each, and the blocks are the dump's blocks bit for bit."""
    grid = rank.grid() if grid is None else grid
    for p in peers:
        n = t.send_counts[p]
        rc, ns, keys, blocks = rank.collect(p, n)
        assert rc == 0 and ns == n, (p, rc, ns, n)
        got = hm.as_keys(keys[1:1 + n])
        assert len(set(got)) == n and set(got) == t.send[p], p
        for k, b in zip(got, blocks[1:1 + n]):
            assert (bits_of(b) == bits_of(grid[k])).all(), (p, k)
        assert (keys[0] == CANARY).all() and (keys[1 + n:] == CANARY).all() and (blocks[0] == CANARY).all() and (blocks[1 + n:] == CANARY).all(), p


def check_tagging(rank, model, lists, grid=None):
    t = model.tag(lists)
    nh, sc = rank.tag(lists)
    assert sc == t.send_counts, (sc, t.send_counts)
    assert nh == len(t.halo_blocks)
    check_dump(rank, model, t)
    check_collect(rank, model, t, grid)
    return t


@pytest.fixture(scope="module", params=["spheres", "wall"])
def rank(request):
    r = HipRank(hm.halo_scene(request.param))
    r.name = request.param
    yield r
    r.close()


@pytest.fixture(scope="module")
def spheres():
    r = HipRank(hm.halo_scene("spheres"))
    yield r
    r.close()


# ---- tagging, phase level -------------------------------------------------------------------------------------------
def test_main_tagging_eight_peers_up_to_31(rank):
    m = rank.model()
    hm.check_scene_conditions(m)
    if rank.name == "wall":
        assert any(0 in k for k in m.particle)
    lists = hm.main_lists(m)
    hm.check_main_lists(m, lists)
    t = check_tagging(rank, m, lists)
    hm.check_main_result(m, t)


def test_list_lengths_whole_list_and_strangers_only(rank):
    m = rank.model()
    pools = m.pools()
    rng = np.random.default_rng(7)
    lists = {p: hm.list_of_length(rng, pools, n) for p, n in zip((2, 3, 9, 10, 17, 18, 29, 31), hm.LENGTHS)}
    assert [len(lists[p]) for p in (2, 3, 9, 10, 17, 18, 29, 31)] == list(hm.LENGTHS)
    lists[6] = hm.mixed_list(rng, pools, {"exterior": 20, "foreign": 20, "outside": 20})
    t = check_tagging(rank, m, lists)
    assert t.send_counts[2] == 0 and t.send_counts[6] == 0 and t.send_counts[31] > 0
    # the whole own list: everything is sent, everything is halo
    t = check_tagging(rank, m, {5: np.array(m.keys, dtype=np.int32)[rng.permutation(m.nbc)]})
    assert t.send_counts[5] == m.nbc and len(t.halo_blocks) == m.pbc
    # a new round forgets the previous one completely; strangers only: nothing is sent, no halo block
    t = check_tagging(rank, m, {6: lists[6]})
    assert t.send_counts == [0] * 32 and not t.halo_blocks and not t.overlap


def test_split_by_identity_no_peer_one_corner_key_everything(rank):
    m = rank.model()
    t = check_tagging(rank, m, {})
    assert not t.halo_blocks and len(t.interior_blocks) == m.pbc
    part = set(m.particle)
    k = next(k for k in m.neighbor_only if sum((k[0] - i, k[1] - j, k[2] - l) in part for i, j, l in hm.CUBE) >= 2)
    t = check_tagging(rank, m, {31: np.array([k], dtype=np.int32)})
    assert t.halo_blocks == {(k[0] - i, k[1] - j, k[2] - l) for i, j, l in hm.CUBE} & part and t.overlap == {k: 1 << 31}
    everything = np.array(m.keys, dtype=np.int32)
    t = check_tagging(rank, m, {p: everything for p in range(32)})
    assert len(t.halo_blocks) == m.pbc and set(t.overlap.values()) == {0xFFFFFFFF} and t.send_counts == [m.nbc] * 32


def test_tagging_and_collect_of_a_rebuilt_partition():
    """After 40 substeps of mpm_run_fixed: the partition the rebuild chain made, not the set-up one; gid 0 holds the run's grid."""
    r = HipRank(hm.halo_scene("spheres"), nsteps=40)
    m = r.model()
    hm.check_scene_conditions(m)
    lists = hm.main_lists(m, seed=3)
    hm.check_main_lists(m, lists)
    grid = r.grid()
    assert sum(bool(np.any(b)) for b in grid.values()) >= 20
    t = check_tagging(r, m, lists, grid)
    hm.check_main_result(m, t)
    r.close()


# ---- collect --------------------------------------------------------------------------------------------------------
def test_collect_capacity_and_empty_peer(spheres):
    r, m = spheres, spheres.model()
    t = m.tag(hm.main_lists(m))
    r.tag(hm.main_lists(m))
    n = t.send_counts[31]
    assert n > 1 and t.send_counts[2] == 0
    rc, ns, keys, blocks = r.collect(31, n - 1)
    assert rc == _ffi.MPM_ERR_CAPACITY and ns == n and (keys == CANARY).all() and (blocks == CANARY).all()
    rc, ns, keys, blocks = r.collect(2, 4)
    assert rc == 0 and ns == 0 and (keys == CANARY).all() and (blocks == CANARY).all()
    check_collect(r, m, t, peers=[31])          # the context still works after the error return


# ---- reduce ---------------------------------------------------------------------------------------------------------
def _addends(rng, n):
    b = (rng.standard_normal((n, 256)) * 10.0 ** rng.integers(-6, 4, (n, 256))).astype(np.float32)
    b[:, ::5] = 0.0
    b[:, 1::7] = -0.0
    assert np.all((b == 0) | (np.abs(b) >= np.finfo(np.float32).tiny))     # no denormals
    return b


@pytest.mark.parametrize("nrecv", [1, 3, 4, 5, 64, 257])
def test_reduce_one_addend_per_node_is_the_float32_sum(rank, nrecv):
    m = rank.model()
    pools = m.pools()
    rng = np.random.default_rng(100 + nrecv)
    n_own = min(nrecv - min(nrecv // 3, 12), m.nbc)
    own = np.array(m.keys, dtype=np.int32)[rng.permutation(m.nbc)[:n_own]]
    rest = nrecv - n_own
    junk_cats = ("exterior", "outside", "foreign")      # dealt round-robin, starting with a different category for every nrecv
    counts = {c: 0 for c in junk_cats}
    for j in range(rest):
        counts[junk_cats[(nrecv + j) % 3]] += 1
    spill = max(0, counts["exterior"] - len(pools["exterior"]))
    counts["exterior"] -= spill
    counts["foreign"] += spill
    junk = hm.mixed_list(rng, pools, counts)
    keys = np.concatenate([own, junk])[rng.permutation(nrecv)]
    assert len(keys) == nrecv and (nrecv < 3 or len(junk) > 0)
    blocks = _addends(rng, nrecv)
    before = rank.grid()
    # halo_reduce_kernel skips zero addends, which differs from the float32 sum only where +0 meets a node holding -0:
    # no entry point writes a -0 into a grid, so the combination cannot be formed here; that no node holds -0 is asserted, not assumed
    assert not any((bits_of(b) == 0x80000000).any() for b in before.values())
    want = m.reduce(before, keys, blocks)
    assert len(want) == n_own and all(v[2] == 1 for v in want.values())
    rank.reduce(keys, blocks)
    after = rank.grid()
    assert set(after) == set(before)
    for k in before:
        exp = want[k][1] if k in want else before[k]        # one addend: old + addend in float32; a block not named is unchanged
        assert (bits_of(after[k]) == bits_of(exp)).all(), k


def test_reduce_several_addends_per_node_within_the_derived_bound(spheres):
    """The same key k times in one call (k = 2, 3, 7): the hardware atomics add in an unspecified order, so each node is compared with
    the float64 sum within k * 2^-24 * (|old| + sum |addend|), the standard bound for k float32 additions in any order."""
    r, m = spheres, spheres.model()
    rng = np.random.default_rng(11)
    perm = rng.permutation(m.nbc)
    keys = []
    for j, k in enumerate((2, 3, 7)):
        for b in perm[6 * j:6 * j + 6]:
            keys += [m.keys[b]] * k
    keys += hm.as_keys(hm.mixed_list(rng, m.pools(), {"exterior": 3, "foreign": 3, "outside": 3}))
    keys = np.array([keys[i] for i in rng.permutation(len(keys))], dtype=np.int32)
    blocks = _addends(rng, len(keys))
    before = r.grid()
    want = m.reduce(before, keys, blocks)
    assert sorted(v[2] for v in want.values()) == [2] * 6 + [3] * 6 + [7] * 6
    assert sum(int(np.count_nonzero(v[0] != before[k])) for k, v in want.items()) >= 100
    r.reduce(keys, blocks)
    after = r.grid()
    worst = 0.0
    for k in before:
        if k not in want:
            assert (bits_of(after[k]) == bits_of(before[k])).all(), k
            continue
        s64, _, cnt, a64 = want[k]
        err = np.abs(after[k].astype(np.float64) - s64)
        bound = cnt * 2.0 ** -24 * a64
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (k, cnt, float(err.max()))
    print(f"multi-addend reduce: worst error / bound = {worst:.3f}")


# ---- two real contexts ----------------------------------------------------------------------------------------------
def test_two_real_contexts_send_sets_are_symmetric_and_grids_sum():
    sc = hm.halo_scene("spheres")
    ranks = [HipRank(mgsp.partition_scene(sc, r, 2)) for r in range(2)]
    models = [r.model() for r in ranks]
    tags = []
    for me, other in ((0, 1), (1, 0)):
        lists = {other: np.array(models[other].keys, dtype=np.int32)}
        tags.append(check_tagging(ranks[me], models[me], lists))
    shared = tags[0].send[1]
    assert shared == tags[1].send[0] == models[0].own & models[1].own and len(shared) >= 20      # what I send to p is what p sends to me
    before = [r.grid() for r in ranks]
    sent = []
    for me, other in ((0, 1), (1, 0)):
        rc, ns, keys, blocks = ranks[me].collect(other, len(shared), gid=0)
        assert rc == 0 and ns == len(shared)
        sent.append((keys[1:1 + ns], blocks[1:1 + ns]))
    for me, other in ((0, 1), (1, 0)):
        ranks[me].reduce(*sent[other])
    after = [r.grid() for r in ranks]
    assert any(np.any(before[0][k]) and np.any(before[1][k]) for k in shared)
    for me in (0, 1):
        for k in before[me]:
            exp = before[0][k] + before[1][k] if k in shared else before[me][k]      # one addend per node: the float32 sum, exactly
            assert (bits_of(after[me][k]) == bits_of(exp)).all(), (me, k)
    for r in ranks:
        r.close()


# ---- the fused path behind MgspRank, with 31 phantom peers -----------------------------------------------------------
class PhantomComm:
    """The three collectives MgspRank calls, for ONE real rank in a world of absent peers: all_gather fills the peers' rows with
    synthetic key lists (script(keys, pad_rows) -> {peer: full list}; the header carries the full length, the rows the first
    pad_rows - 1 keys) and puts garbage into the own rank's rows behind row 0's count; all_to_all hands back the keys this rank
    sent with blocks of zeros.  It records every gathered array and what was sent."""

    def __init__(self, rank, world, script, status=None, seed=0):
        self.rank, self.world, self.script, self.status = rank, world, script, status or {}
        self.rng = np.random.default_rng(seed)
        self.gathers, self.sent = [], None

    def all_reduce_max(self, t):
        pass

    def all_gather(self, out, inp):
        mine = inp.cpu().numpy().copy()
        pad = mine.shape[0]
        n = min(int(mine[0, 0]), pad - 1)
        rows = hm.padded_rows(self.world, pad, self.script(mine[1:1 + n], pad), self.status)
        rows[self.rank] = self.rng.integers(-3, hm.G_BLOCKS + 3, (pad, 3))
        rows[self.rank, 0, 0] = mine[0, 0]
        self.gathers.append((mine, rows))
        out.copy_(torch.from_numpy(rows.reshape(-1, 3)))

    def all_to_all(self, recv, send, splits):
        recv.copy_(send)
        self.sent, off = {}, 0
        for p, s in enumerate(splits):
            c = s // ROW
            if c:
                self.sent[p] = send[off:off + 3 * c].view(torch.int32).cpu().numpy().reshape(-1, 3)
                recv[off + 3 * c:off + ROW * c] = 0.0
            off += s


def _phantom_rank(monkeypatch, rank, script, status=None, world=32):
    monkeypatch.setattr(mgsp, "partition_scene", lambda scene, r, w: scene)        # the one real rank owns the whole scene
    comm = PhantomComm(rank, world, script, status, seed=rank)
    sim = MgspRank(hm.halo_scene("spheres"), rank, world, device=0, comm=comm)
    sim.hr = HipRank.__new__(HipRank)
    sim.hr.eng, sim.hr.api, sim.hr.ctx = sim.eng, sim.api, sim.ctx
    return sim, comm


def _random_script(rng, world, rank):
    def script(keys, pad):
        return {p: hm.list_from_keys(rng, keys, hm.G_BLOCKS, int(rng.integers(0, 40)), int(rng.integers(0, 30))) for p in range(world) if p != rank}
    return script


def _check_fused_state(sim, comm, rows=None, send_counts=None, n_halo=None):
    """send counts, halo count, marks and lists of the last tagging against the model applied to the exported own row and the fabricated rows."""
    mine, last = comm.gathers[-1]
    rows = last if rows is None else rows
    c = sim.eng.counts()
    assert int(mine[0, 0]) == c.neighbor_blocks
    m = sim.hr.model()
    n = min(m.nbc, rows.shape[1] - 1)
    assert hm.as_keys(mine[1:1 + n]) == m.keys[:n] and mine[0].tolist() == [m.nbc, 0, 0] and (mine[1 + n:] == 0).all()      # the exported row
    t = m.tag_padded(rows, sim.rank)
    assert t.send_counts[sim.rank] == 0
    assert (sim.send_counts if send_counts is None else send_counts) == t.send_counts
    assert (sim.n_halo_blocks if n_halo is None else n_halo) == len(t.halo_blocks)
    check_dump(sim.hr, m, t)
    return m, t


@pytest.fixture(scope="module")
def plain_runs():
    """40 substeps of the spheres scene on the oracle and on the plain HIP engine (one context, no halo path)."""
    sc = hm.halo_scene("spheres")
    return sc, run_engine(sc, 40, DT, api=oracle_api()), run_engine(sc, 40, DT)


@pytest.mark.parametrize("own", [0, 13, 31])
def test_fused_path_world_32_with_phantom_peers(own, monkeypatch, plain_runs):
    rng = np.random.default_rng(50 + own)
    sim, comm = _phantom_rank(monkeypatch, own, _random_script(rng, 32, own))
    sim.initial_setup()
    _, t = _check_fused_state(sim, comm)
    seen_halo = 0
    for step in range(40):
        prev = t
        sim.substep(DT, DT)
        # what this substep's exchange sent is what the tagging before it listed, peer by peer
        for p in range(32):
            got = hm.as_keys(comm.sent.get(p, np.zeros((0, 3))))
            assert len(set(got)) == len(got) and set(got) == prev.send[p], (step, p)
        m, t = _check_fused_state(sim, comm)
        seen_halo = max(seen_halo, len(t.halo_blocks))
    assert seen_halo > 0 and sum(sim.send_counts) > 0
    state = sim.local_state()
    sim.close()
    # phantom peers contribute nothing: the run computes what the plain engine computes
    sc, ora, hip = plain_runs
    for mi in range(len(sc["models"])):
        x = state[mi][0].astype(np.float64)
        xo, xh = ora["state"][mi][0].astype(np.float64), hip["state"][mi][0].astype(np.float64)
        assert x.shape == xo.shape == xh.shape
        idx, _ = match(xo, x)
        rel = (np.abs(x[idx] - xo).max(axis=1) / np.abs(xo).max(axis=1)).max()
        idh, _ = match(xh, x)
        print(f"rank {own} model {mi}: position difference to the oracle {rel:.3e} (relative), to the plain HIP engine {np.abs(x[idh] - xh).max():.3e} (absolute)")
        assert rel < POS_TOL, rel


def _manual_substep(sim, comm, pad, script, status=None):
    """One fused substep through the ABI itself with a padding of the caller's choice -> (rows, send counts, halo count, max_peer_rows)."""
    # mirrors MgspRank.substep (claymore_amd/mgsp.py: mgsp_begin, _exchange beside g2p2g_interior, mgsp_rebuild_export, all_gather, mgsp_tag,
    # mgsp_end) without its re-tag branch, so that the truncated tagging can be looked at; a change there has to be repeated here
    api, ctx = sim.api, sim.ctx
    sim._check(api.mgsp_begin(ctx, DT, DT))
    sim._exchange(1, overlap_with=lambda: sim._check(api.g2p2g_interior(ctx, DT, DT)))
    with torch.cuda.stream(sim._compute_stream):
        mine = torch.full((pad, 3), CANARY, dtype=torch.int32, device="cuda")
        allk = torch.zeros((sim.world * pad, 3), dtype=torch.int32, device="cuda")
        sim._check(api.mgsp_rebuild_export(ctx, _ptr(mine), pad))
        comm.script, comm.status = script, status or {}
        comm.all_gather(allk, mine)
    sim._check(api.mgsp_tag(ctx, _ptr(allk), pad, sim.world, sim.rank))
    sc, nh, mx, mv = (C.c_int * 32)(), C.c_int(-1), C.c_int(-1), C.c_float(0)
    rc = api.mgsp_end(ctx, sc, C.byref(nh), C.byref(mx), C.byref(mv))
    return rc, comm.gathers[-1][1], list(sc), nh.value, mx.value


def test_fused_path_truncated_peer_tight_padding_and_pad_2(monkeypatch):
    own = 13
    rng = np.random.default_rng(3)
    sim, comm = _phantom_rank(monkeypatch, own, _random_script(rng, 32, own))
    sim.initial_setup()
    nbc = sim.eng.counts().neighbor_blocks

    # (1) pad_rows exactly nbc + 1: nothing to spare (the first substep moves no particle across a block face: the block set stays)
    rc, rows, sc, nh, mx = _manual_substep(sim, comm, nbc + 1, _random_script(rng, 32, own))
    assert rc == 0 and int(comm.gathers[-1][0][0, 0]) == nbc == rows.shape[1] - 1
    m, t = _check_fused_state(sim, comm, rows, sc, nh)
    assert mx == t.max_peer_rows == nbc + 1
    sim.send_counts, sim.n_halo_blocks = [sc[p] if p != own else 0 for p in range(32)], nh

    # (2) a peer whose header count exceeds pad_rows - 1: its strangers come first, so most of its own keys are cut off
    pad = nbc + 40

    def long_script(keys, pad_rows, base=_random_script(rng, 32, own)):
        lists = base(keys, pad_rows)
        model = hm.HaloModel(keys, 0, hm.G_BLOCKS)
        strangers = [k for k in model.foreign()][:pad + 10 - len(keys) // 2]
        lists[5] = np.array(strangers + hm.as_keys(keys), dtype=np.int32)
        return lists
    rc, rows, sc, nh, mx = _manual_substep(sim, comm, pad, long_script)
    assert rc == 0 and rows[5, 0, 0] > pad - 1
    m, t = _check_fused_state(sim, comm, rows, sc, nh)
    assert mx == t.max_peer_rows == rows[5, 0, 0] + 1 and 0 < t.send_counts[5] < m.nbc
    sim.send_counts, sim.n_halo_blocks = [sc[p] if p != own else 0 for p in range(32)], nh
    # MgspRank's own substep with the same peer: it tags, sees the truncation, and re-tags with a larger padding -> the full result
    sim.pad, comm.script = pad, long_script
    before = len(comm.gathers)
    sim.substep(DT, DT)
    assert len(comm.gathers) == before + 2 and comm.gathers[-1][1].shape[1] > comm.gathers[-1][1][5, 0, 0] >= comm.gathers[-2][1].shape[1]
    m, t = _check_fused_state(sim, comm)
    assert t.send_counts[5] == m.nbc and len(t.halo_blocks) == m.pbc

    # (3) pad_rows = 2: one key per rank
    rc, rows, sc, nh, mx = _manual_substep(sim, comm, 2, lambda keys, pad_rows: {p: np.array(m.keys, dtype=np.int32)[p:p + 3] for p in range(32) if p != own})
    assert rc == 0 and rows.shape[1] == 2
    m2 = sim.hr.model()
    t = m2.tag_padded(rows, own)
    mine = comm.gathers[-1][0]
    assert mine[0].tolist() == [m2.nbc, 0, 0] and hm.as_keys(mine[1:]) == m2.keys[:1]
    assert sc == t.send_counts and nh == len(t.halo_blocks) and mx == m2.nbc + 1 and max(sc) == 1
    check_dump(sim.hr, m2, t)
    sim.close()


@pytest.mark.parametrize("word", [hm.PEER_ERR_BLOCKS, hm.PEER_ERR_LIST, hm.PEER_ERR_BINS, hm.PEER_ERR_NONFINITE, hm.PEER_ERR_BOOKS, 32])
def test_a_peers_status_word_is_this_ranks_error(word, monkeypatch):
    """Row 0 of a peer carries an error bit: mpm_mgsp_end returns the status mgsp_peer_status maps it to and names the rank.  An ordinary
    error return on a healthy device; the context is destroyed afterwards."""
    rng = np.random.default_rng(word)
    sim, comm = _phantom_rank(monkeypatch, 0, _random_script(rng, 32, 0))
    sim.initial_setup()
    comm.status = {9: word}
    with pytest.raises(EngineError) as e:
        sim.substep(DT, DT)
    rows = comm.gathers[-1][1]
    t = hm.HaloModel(np.zeros((0, 3)), 0, hm.G_BLOCKS).tag_padded(rows, 0)
    assert t.status == (9, word, hm.peer_status_code(word))
    assert e.value.code == t.status[2] and "rank 9 reported" in str(e.value), str(e.value)
    sim.close()


# ---- a world above 8 through the group driver ------------------------------------------------------------------------
def test_cpp_group_16_ranks_equals_oracle():
    """mpm_group_create_local with 16 ranks as threads on one device, 30 substeps of mpm_group_run_fixed, against the oracle as
    test_cpp_group_equals_oracle does.  The equal-count slabs of partition_scene give every rank a share of both spheres (a sphere of
    radius 5 cells holds about 4000 particles), so no rank is without particles of a model."""
    from test_mgsp_gpu import _compare_with_oracle, _run_group_threads
    sc = hm.halo_scene("spheres")
    for r in range(16):
        assert all(len(mm["xyz"]) > 0 for mm in mgsp.partition_scene(sc, r, 16)["models"])
    t0 = time.time()
    res = _run_group_threads(sc, 16, 30, DT, fixed=True)
    print(f"16-rank group run: {time.time() - t0:.1f} s")
    assert max(r[1] for r in res) > 0 and max(r[2] for r in res) > 0
    _compare_with_oracle(sc, res, 30, DT)

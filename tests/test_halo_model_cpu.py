"""tests/halo_model.py against the CPU oracle, which has the same phase-level halo entry points and is an independent implementation
(oracle/mpm_oracle.c, "MGSP halo path"): what makes the model trustworthy before tests/test_halo_kernels_gpu.py lets it judge the HIP
kernels.  All 32 peers are tagged; every comparison is exact (integers, float32 bit patterns).  The oracle has no read-out of its marks
and lists, so they are compared through what it exposes: send counts, the halo block count, the collected keys and blocks, the grid."""
import ctypes as C

import numpy as np
import pytest

import halo_model as hm
from claymore_amd import _ffi
from claymore_amd.engine import build_engine
from oracle_ffi import oracle_api


def _vp(a):
    return C.c_void_p(a.ctypes.data)


class OracleRank:
    """One oracle context driven through the phase-level halo calls with host arrays."""

    def __init__(self, scene, nsteps=0):
        self.api = oracle_api()
        self.eng = build_engine(scene, api=self.api)
        self.ctx = self.eng.ctx
        self.eng.initial_setup()
        if nsteps:
            self.eng.run_fixed(nsteps, 1e-4)

    def model(self):
        c = self.eng.counts()
        keys = np.zeros((c.neighbor_blocks, 3), dtype=np.int32)
        cnt = C.c_int(0)
        assert self.api.halo_keys(self.ctx, _vp(keys), len(keys), C.byref(cnt)) == 0 and cnt.value == len(keys)
        return hm.HaloModel(keys, c.particle_blocks, hm.G_BLOCKS)

    def exterior_keys(self):
        c = self.eng.counts()
        counts3 = (C.c_int * 3)()
        keys = np.zeros((c.exterior_blocks, 3), dtype=np.int32)
        n = self.eng.models[0]["n"]
        sizes, buckets, binoff = np.zeros(c.particle_blocks + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(c.particle_blocks + 2, np.int32)
        fn = self.api.raw.mpmo_fn_book_dump
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        assert fn(self.ctx, 0, 1, counts3, _vp(keys), _vp(sizes), _vp(buckets), _vp(binoff)) == 0
        assert list(counts3) == [c.particle_blocks, c.neighbor_blocks, c.exterior_blocks]
        return hm.as_keys(keys[c.neighbor_blocks:])

    def tag(self, lists):
        assert self.api.halo_tag_begin(self.ctx) == 0
        for p, lst in lists.items():
            lst = np.ascontiguousarray(lst, dtype=np.int32)
            assert self.api.halo_tag_peer(self.ctx, p, _vp(lst), len(lst)) == 0
        nh, sc = C.c_int(-1), (C.c_int * 32)()
        assert self.api.halo_tag_end(self.ctx, C.byref(nh), sc) == 0
        return nh.value, list(sc)

    def collect(self, peer, gid=0, capacity=None, n=0):
        cap = n if capacity is None else capacity
        keys, blocks = np.full((cap + 1, 3), -7, np.int32), np.full((cap + 1, 256), np.float32(-7.0))
        ns = C.c_int(-1)
        rc = self.api.halo_collect(self.ctx, peer, gid, _vp(keys), _vp(blocks), cap, C.byref(ns))
        return rc, ns.value, keys, blocks

    def grid(self):
        return hm.grid_dict(*self.eng.dump_grid())

    def close(self):
        self.eng.close()


def check_tagging_against_oracle(rank, model, lists):
    """send counts of all 32 peers, the halo block count, and for every peer the collected keys (as a set, no duplicate) and blocks (bits)."""
    t = model.tag(lists)
    nh, sc = rank.tag(lists)
    assert sc == t.send_counts
    assert nh == len(t.halo_blocks)
    grid = rank.grid()
    for p in range(32):
        rc, ns, keys, blocks = rank.collect(p, n=t.send_counts[p])
        assert rc == 0 and ns == t.send_counts[p]
        got = hm.as_keys(keys[:ns])
        assert len(set(got)) == ns and set(got) == t.send[p], p
        want = model.collect(grid, t.send[p])
        for k, b in zip(got, blocks[:ns]):
            assert b.view(np.uint32).tolist() == want[k].view(np.uint32).tolist()
        assert (keys[ns:] == -7).all() and (blocks[ns:] == -7.0).all()
    return t


@pytest.fixture(scope="module", params=["spheres", "wall"])
def rank(request):
    r = OracleRank(hm.halo_scene(request.param))
    r.name = request.param
    yield r
    r.close()


def test_scenes_hold_enough_blocks_of_every_category(rank):
    m = rank.model()
    pools = hm.check_scene_conditions(m)
    # the model's exterior-only keys are blocks the engine really holds as exterior blocks, its strangers are blocks it does not hold
    ext = set(rank.exterior_keys())
    assert set(pools["exterior"]) <= ext
    assert not (set(pools["foreign"]) & (ext | m.own))
    assert all(not m.in_domain(k) for k in pools["outside"]) and {c for k in pools["outside"] for c in k} >= {-1, m.G, m.G + 5, 1 << 30}
    if rank.name == "wall":
        assert any(0 in k for k in m.particle)
    lists = hm.main_lists(m)
    hm.check_main_lists(m, lists)
    hm.check_main_result(m, m.tag(lists))


def test_main_lists_on_eight_peers_up_to_31(rank):
    m = rank.model()
    check_tagging_against_oracle(rank, m, hm.main_lists(m))


def test_all_32_peers_and_the_edge_lengths(rank):
    m = rank.model()
    pools = m.pools()
    rng = np.random.default_rng(7)
    lists = {p: hm.list_of_length(rng, pools, int(rng.integers(0, 120))) for p in range(32)}
    for p, n in zip((2, 3, 9, 10, 17, 18, 29, 31), hm.LENGTHS):
        lists[p] = hm.list_of_length(rng, pools, n)
        assert len(lists[p]) == n
    lists[5] = np.array(m.keys, dtype=np.int32)[rng.permutation(m.nbc)]                                   # the whole own list
    lists[6] = hm.mixed_list(rng, pools, {"exterior": 20, "foreign": 20, "outside": 20})                 # nothing of this rank's
    t = check_tagging_against_oracle(rank, m, lists)
    assert t.send_counts[5] == m.nbc and t.send_counts[6] == 0 and t.send_counts[2] == 0 and len(t.halo_blocks) == m.pbc
    # a new round forgets the previous one
    t = check_tagging_against_oracle(rank, m, {6: lists[6]})
    assert t.send_counts == [0] * 32 and not t.halo_blocks
    t = check_tagging_against_oracle(rank, m, {})
    assert not t.halo_blocks and len(t.interior_blocks) == m.pbc


def test_one_corner_key_turns_exactly_its_cube_halo(rank):
    m = rank.model()
    k = next(k for k in m.neighbor_only if sum((k[0] - i, k[1] - j, k[2] - l) in set(m.particle) for i, j, l in hm.CUBE) >= 2)
    t = check_tagging_against_oracle(rank, m, {31: np.array([k], dtype=np.int32)})
    assert t.halo_blocks == {(k[0] - i, k[1] - j, k[2] - l) for i, j, l in hm.CUBE} & set(m.particle) and t.overlap == {k: 1 << 31}


def test_tagging_of_a_rebuilt_partition():
    r = OracleRank(hm.halo_scene("spheres"), nsteps=40)
    m = r.model()
    hm.check_scene_conditions(m)
    check_tagging_against_oracle(r, m, hm.main_lists(m, seed=3))
    r.close()


@pytest.mark.parametrize("nrecv", [1, 3, 4, 5, 64, 257])
def test_reduce_against_the_oracle_grid(rank, nrecv):
    """Keys absent, exterior-only and out of the domain are ignored, a key may come several times (the oracle adds in arrival order, and
    so does the model's float32 column), every block of the dump is compared."""
    m = rank.model()
    pools = m.pools()
    rng = np.random.default_rng(nrecv)
    own = np.array(m.keys, dtype=np.int32)
    pick = own[rng.integers(0, m.nbc, nrecv)]                                                              # with repeats
    junk = hm.mixed_list(rng, pools, {"exterior": 3, "foreign": 3, "outside": 4})
    keys = np.concatenate([pick, junk])[rng.permutation(nrecv + len(junk))]
    blocks = rng.standard_normal((len(keys), 256)).astype(np.float32)
    blocks[:, ::5] = 0.0
    blocks[:, 1::7] = -0.0
    before = rank.grid()
    want = m.reduce(before, keys, blocks)
    assert rank.api.halo_reduce(rank.ctx, 0, _vp(keys), _vp(blocks), len(keys)) == 0
    after = rank.grid()
    assert set(after) == set(before)
    for k in before:
        exp = want[k][1] if k in want else before[k]
        assert after[k].view(np.uint32).tolist() == exp.view(np.uint32).tolist(), k


@pytest.mark.parametrize("own", [0, 13, 31])
def test_fused_path_with_padded_lists(own):
    """mpmo_mgsp_rebuild_export / _tag / _end on a world of 32: the exported row, the header rule with a truncated peer, the own row
    ignored, max_peer_rows."""
    r = OracleRank(hm.halo_scene("spheres"))
    api, ctx = r.api, r.ctx
    r.tag({})
    rng = np.random.default_rng(own)
    for step in range(3):
        assert api.mgsp_begin(ctx, 1e-4, 1e-4) == 0 and api.g2p2g_interior(ctx, 1e-4, 1e-4) == 0
        nbc_guess = r.eng.counts().neighbor_blocks
        pad = (nbc_guess + 40, nbc_guess + 40, 30)[step]                                                    # step 2: every long list is truncated
        mine = np.full((pad, 3), -3, dtype=np.int32)
        assert api.mgsp_rebuild_export(ctx, _vp(mine), pad) == 0
        m = r.model()
        n = min(m.nbc, pad - 1)
        assert mine[0].tolist() == [m.nbc, 0, 0] and hm.as_keys(mine[1:1 + n]) == m.keys[:n] and (mine[1 + n:] == 0).all()
        pools = m.pools()
        lists = {p: hm.list_of_length(rng, pools, int(rng.integers(0, 90))) for p in range(32) if p != own}
        rows = hm.padded_rows(32, pad, lists)
        rows[own] = mine
        rows[own, 1:] = rng.integers(-5, 20, (pad - 1, 3))                                                # garbage in the own rows changes nothing
        rows = np.ascontiguousarray(rows)
        assert api.mgsp_tag(ctx, _vp(rows), pad, 32, own) == 0
        sc, nh, mx, mv = (C.c_int * 32)(), C.c_int(-1), C.c_int(-1), C.c_float(0)
        assert api.mgsp_end(ctx, sc, C.byref(nh), C.byref(mx), C.byref(mv)) == 0
        t = m.tag_padded(rows, own)
        assert list(sc) == t.send_counts and nh.value == len(t.halo_blocks) and mx.value == t.max_peer_rows and sc[own] == 0
        if step == 2:
            assert mx.value > pad and any(len(lists[p]) > pad - 1 and t.send_counts[p] < len(m.tag({p: lists[p]}).send[p]) for p in lists)
    r.close()

"""tests/rebuild_books.check_books - the verifier of everything the partition rebuild writes - held against a plain numpy rebuild
(tests/rebuild_model.py) whose free orders are drawn from a seed, against a table of single-field corruptions it must report, against the
reference's own book (tests/golden/g20_*) and against the still-step model of tests/test_still_rebuild_model_cpu.py; and the scene generators of
tests/test_rebuild_books_gpu.py on the model alone.  No GPU."""
import numpy as np
import pytest

import ckpt_format as cf
import g2p2g_model as gm
import rebuild_books as rb
import rebuild_model as rmod
import rebuild_scenes as rs
import test_still_rebuild_model_cpu as still

BITS, MAX_PPC = 6, 16
G = 1 << (BITS - 2)
SIZES = rs.SIZES
PID_BITS = 10


# ---- (a) the model's output passes, whatever the numbering ---------------------------------------------------------------------------------
def _block(key, n, rng):
    return (4.0 * np.asarray(key, np.float64) + 1.5 + rng.uniform(0.02, 3.98, (n, 3))).astype(np.float32)


def case(seed, bits=BITS, max_ppc=MAX_PPC):
    """Two models.  Model 0 (pair layout, 4 floats per particle): one block per size of SIZES whose particles move within it, keys drawn from 1, 5,
    40 or all 216 values.  Model 1 (sliced layout, 10 floats): the same blocks with the sizes in reverse order, and blocks of its own.  Both: 3^3
    blocks in the domain's (0, 0, 0) corner and 3^3 in the opposite one - faces, edges, a corner - whose particles move by up to 2.5 cells, and
    lone particles that leave their block for one that was a neighbour or exterior block only."""
    rng = np.random.default_rng(seed)
    g = 1 << (bits - 2)
    sites = [(2 + 2 * (i % 4), 5 + 2 * (i // 8), 2 + 2 * ((i // 4) % 2) + 5) for i in range(len(SIZES))]
    assert len(set(sites)) == len(SIZES)
    corner = [(x, y, z) for x in range(3) for y in range(3) for z in range(3)]
    corner += [(g - 1 - x, g - 1 - y, g - 1 - z) for x, y, z in corner]
    lone = [(12, 3, 3), (12, 3, 12), (3, 12, 3)]
    old, new, key = [[], []], [[], []], [[], []]
    for m in range(2):
        for i, k in enumerate(sites):
            n = SIZES[i] if m == 0 else SIZES[::-1][i]
            if m == 1 and i % 5 == 4:
                continue                                                    # (blocks that hold model 0 only)
            old[m].append(_block(k, n, rng))
            new[m].append(_block(k, n, rng))
            key[m].append(rng.choice(216, (1, 5, 40, 216)[(i + m) % 4], replace=False)[rng.integers(0, (1, 5, 40, 216)[(i + m) % 4], n)])
        for k in corner[m::2] + ([(9, 12, 12)] if m else []):               # (model 1's own block)
            p = _block(k, 40, rng)
            q = np.clip(p.astype(np.float64) + rng.uniform(-2.5, 2.5, p.shape), 1.6, 4 * g + 1.4).astype(np.float32)
            old[m].append(p), new[m].append(q), key[m].append(rng.integers(0, 216, 40))
        for j, k in enumerate(lone):
            p = _block(k, 1, rng)
            q = p.copy()
            q[0, (j + m) % 3] += np.float32(4.0 if m == 0 else -4.0)
            old[m].append(p), new[m].append(q), key[m].append(rng.integers(0, 216, 1))
    parts = [(4, rmod.PAIR_LAYOUT, np.concatenate(old[0])), (10, 0, np.concatenate(old[1]))]
    prev = rmod.make_prev(bits, max_ppc, parts, rng)
    moves = [(np.concatenate(new[m]), np.concatenate(key[m])) for m in range(2)]
    return prev, moves


@pytest.fixture(scope="module")
def built():
    prev, moves = case(1)
    ckpt, rows = rmod.rebuild(prev, moves, seed=1)
    return ckpt, rows


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_the_models_books_verify_under_any_numbering(seed):
    prev, moves = case(seed)
    ckpt, rows = rmod.rebuild(prev, moves, seed=seed)
    h = cf.parse(ckpt)
    keys = cf.cur_keys(ckpt)[:h["pbc"]]
    size = [cf.section(ckpt, h, ("size", m), np.int32)[:h["pbc"]] for m in range(2)]
    # the case holds what it promises: every size in the pair layout, blocks with one model only, faces / edges / a corner, an emptied block
    assert set(SIZES) <= set(size[0].tolist()) and len(set(SIZES) & set(size[1].tolist())) >= 12
    assert ((size[0] > 0) & (size[1] == 0)).any() and ((size[0] == 0) & (size[1] > 0)).any()
    at_face = ((keys == 0) | (keys == G - 1)).sum(axis=1)
    assert (at_face == 1).any() and (at_face == 2).any() and (at_face == 3).any()
    assert h["pbc"] != prev["pbc"] or not np.array_equal(keys, prev["keys"][:prev["pbc"]])
    tags = [cf.list_records(ckpt, m)["tag"] for m in range(2)]
    assert all((t != 13).sum() > 100 for t in tags)
    assert rb.check_books(ckpt, rows, BITS, MAX_PPC, counts=[int(s.sum()) for s in size]) == []


# ---- (b) single-field corruptions ----------------------------------------------------------------------------------------------------------
def _sec(buf, name, dtype=np.int32):
    return cf.section(buf, cf.parse(buf), name, dtype)


def _first_record(buf, m, cond):
    r = cf.list_records(buf, m)
    return int(np.flatnonzero(cond(r))[0])


def c_key_to_other_tier(buf, rows):
    h, k = cf.parse(buf), _sec(buf, "cur_keys").reshape(-1, 3)
    k[[h["nbc"] - 1, h["nbc"]]] = k[[h["nbc"], h["nbc"] - 1]]


def c_particle_key_to_neighbour_tier(buf, rows):
    h, k = cf.parse(buf), _sec(buf, "cur_keys").reshape(-1, 3)
    k[[h["pbc"] - 1, h["pbc"]]] = k[[h["pbc"], h["pbc"] - 1]]


def c_key_twice(buf, rows):
    h, k = cf.parse(buf), _sec(buf, "cur_keys").reshape(-1, 3)
    k[h["ebc"] - 1] = k[h["nbc"]]


def c_size_off_by_one(buf, rows):
    _sec(buf, ("size", 0))[3] += 1


def c_bucketed(buf, rows):
    """the last block's size one short: every record still lies where it did, the sizes no longer add up to the header's bucketed"""
    size = _sec(buf, ("size", 1))
    b = int(np.flatnonzero(size[:cf.parse(buf)["pbc"]] > 1)[-1])
    size[b] -= 1


def c_row_of(buf, rows):
    r = _sec(buf, ("row_of", 1))
    r[2] = r[3]


def c_bin_of_empty_block(buf, rows):
    h = cf.parse(buf)
    b = int(np.flatnonzero(_sec(buf, ("size", 1))[:h["pbc"]] == 0)[0])
    _sec(buf, ("binoff_dst", 1))[b] = 3


def c_bins_overlap(buf, rows):
    h = cf.parse(buf)
    off, size = _sec(buf, ("binoff_dst", 0)), _sec(buf, ("size", 0))
    b = int(np.flatnonzero((off[:h["pbc"]] > 0) & (size[:h["pbc"]] > 0))[0])
    off[b] -= 1


def c_tag_mirrored(buf, rows):
    i = _first_record(buf, 0, lambda r: r["tag"] != 13)
    lst = _sec(buf, ("lists", 0)).view(np.uint32)
    tag = (int(lst[i]) >> (PID_BITS + 8)) & 31
    lst[i] = (int(lst[i]) & ~(31 << (PID_BITS + 8))) | ((26 - tag) << (PID_BITS + 8))


def c_tag_27(buf, rows):
    lst = _sec(buf, ("lists", 1)).view(np.uint32)
    lst[5] = (int(lst[5]) & ~(31 << (PID_BITS + 8))) | (27 << (PID_BITS + 8))


def c_bit_31(buf, rows):
    _sec(buf, ("lists", 0)).view(np.uint32)[7] |= np.uint32(1 << 31)


def c_slot_twice(buf, rows):
    r = cf.list_records(buf, 1)
    b = int(np.flatnonzero(np.bincount(r["blk"]) > 3)[0])
    i, j = np.flatnonzero(r["blk"] == b)[:2]
    lst = _sec(buf, ("lists", 1))
    lst[j] = lst[i]


def c_slot_outside(buf, rows):
    i = _first_record(buf, 0, lambda r: cf.source_extents(buf, 0)[np.maximum(r["src"], 0)] == 1)
    _sec(buf, ("lists", 0)).view(np.uint32)[i] |= np.uint32(1023)


def c_particle_elsewhere(buf, rows):
    r = cf.list_records(buf, 1)
    B = cf.bins(buf, 1)
    B[r["bin"][0], r["lane"][0] * 8] += np.float32(4.0)


def c_arena_in_sliced(buf, rows):
    _sec(buf, ("lists", 1)).view(np.uint32)[11] |= np.uint32(1 << 30)


def _pair_block(buf, want):
    """(first record, size, pair counts) of the first block of model 0 (pair layout) for which want(size, pf of chunk 0) holds"""
    h = cf.parse(buf)
    size = _sec(buf, ("size", 0))[:h["pbc"]]
    pinfo = _sec(buf, ("pairinfo", 0)).reshape(-1, 16)
    at = np.concatenate([[0], np.cumsum(size)])
    b = next(b for b in range(h["pbc"]) if want(int(size[b]), int(pinfo[b, 0])))
    return int(at[b]), int(size[b]), pinfo[b]


def c_swap_across_pair_slots(buf, rows):
    """the A members of the first and the last pair slot of a one-slice chunk (different keys: the keys ascend) change places"""
    lst = _sec(buf, ("lists", 0))
    keys_of = lambda at, n: (lst[at:at + n].view(np.uint32) >> PID_BITS) & 255
    at, n, pinfo = next(t for t in (_pair_block(buf, lambda s, pf, want=want: s == want and pf >= 2) for want in (65, 127, 128)) if keys_of(t[0], t[1])[0] != keys_of(t[0], t[1])[t[2][0] - 1])
    lst[[at, at + pinfo[0] - 1]] = lst[[at + pinfo[0] - 1, at]]


def c_pairinfo_plus(buf, rows):
    _pair_block(buf, lambda s, pf: s == 129)[2][0] += 1


def c_pairinfo_minus(buf, rows):
    _pair_block(buf, lambda s, pf: s == 513 and pf >= 1)[2][0] -= 1


def c_pairinfo_second_chunk(buf, rows):
    _pair_block(buf, lambda s, pf: s == 1023)[2][1] += 1


def c_arena_flipped_on_a_pair(buf, rows):
    at, n, pinfo = _pair_block(buf, lambda s, pf: s == 127 and pf >= 1)
    _sec(buf, ("lists", 0)).view(np.uint32)[at] ^= np.uint32(1 << 30)


def c_arena_flipped_on_a_single(buf, rows):
    """a single whose key has a pair slot in the same slice (one-slice chunk): its arena must be the other one"""
    h = cf.parse(buf)
    size = _sec(buf, ("size", 0))[:h["pbc"]]
    pinfo = _sec(buf, ("pairinfo", 0)).reshape(-1, 16)
    at = np.concatenate([[0], np.cumsum(size)])
    lst = _sec(buf, ("lists", 0)).view(np.uint32)
    for b in np.flatnonzero((size > 2) & (size <= 128)):
        n, pf = int(size[b]), int(pinfo[b, 0])
        key = (lst[at[b]:at[b] + n] >> PID_BITS) & 255
        L = n - pf                                                  # slots: pf pairs, then the singles (A only; X = 0 in one slice of <= 64 slots)
        for p in range(pf, L):
            if (key[:pf] == key[p]).sum() == 1:
                lst[at[b] + p] ^= np.uint32(1 << 30)
                return
    raise AssertionError("no such single")


def c_sliced_order(buf, rows):
    r = cf.list_records(buf, 1)
    b = int(np.flatnonzero(np.bincount(r["blk"]) == 63)[0])        # one slice: the list is in key order
    idx = np.flatnonzero(r["blk"] == b)
    assert r["key"][idx[0]] != r["key"][idx[-1]]
    lst = _sec(buf, ("lists", 1))
    lst[[idx[0], idx[-1]]] = lst[[idx[-1], idx[0]]]


def _lane(buf, rows, m, lanes, cond):
    for b in range(rows[m].shape[0]):
        for l in lanes:
            if cond(b, l, int(rows[m][b, l])):
                return b, l
    raise AssertionError("no such lane")


def _constrained(buf):
    h = cf.parse(buf)
    cur, prev = cf.cur_keys(buf).astype(np.int64), cf.key_map(_sec(buf, "prev_keys").reshape(-1, 3))

    def f(b, l, v):
        s = prev.get(tuple((cur[b] + cf.DIRS[l]).tolist()), -1)
        return 0 <= s < h["prev_pbc"]
    return f


def c_row_source_lane(buf, rows):
    b, l = _lane(buf, rows, 0, range(27), _constrained(buf))
    rows[0][b, l] += 1


def c_row_destination_lane(buf, rows):
    b, l = _lane(buf, rows, 1, range(27, 54), lambda b, l, v: v >= 0)
    rows[1][b, l] += 1


def c_row_grid_lane(buf, rows):
    b, l = _lane(buf, rows, 0, range(54, 62), lambda b, l, v: v >= 0)
    rows[0][b, l] -= 1


def c_row_minus_one_made_zero(buf, rows):
    b, l = _lane(buf, rows, 0, range(27, 62), lambda b, l, v: v == -1)
    rows[0][b, l] = 0


def c_row_source_minus_one_made_zero(buf, rows):
    b, l = _lane(buf, rows, 1, range(27), lambda b, l, v: v == -1)
    rows[1][b, l] = 0


def c_row_unused_lane(buf, rows):
    rows[1][0, 63] = 0


def c_row_mirrored(buf, rows):
    """lanes 27 .. 53 looked up at key + dir where key - dir belongs: the row read backwards"""
    b = next(b for b in range(rows[0].shape[0]) if not np.array_equal(rows[0][b, 27:54], rows[0][b, 27:54][::-1]))
    rows[0][b, 27:54] = rows[0][b, 27:54][::-1].copy()


CORRUPTIONS = [  # (what is changed, which findings it must raise - any of them)
    (c_key_to_other_tier, ("neighbour tier", "exterior tier")),
    (c_particle_key_to_neighbour_tier, ("particle tier",)),
    (c_key_twice, ("a key appears twice in the current numbering",)),
    (c_size_off_by_one, ("size", "sizes do not add up to bucketed")),
    (c_bucketed, ("sizes do not add up to bucketed",)),
    (c_row_of, ("row_of",)),
    (c_bin_of_empty_block, ("binoff_dst of an empty block",)),
    (c_bins_overlap, ("bin ranges do not tile [0, bincount)",)),
    (c_tag_mirrored, ("record names no particle block of the previous numbering", "record slot outside its source block's bins",
                      "a slot is named twice", "a record's particle does not lie in the record's block")),
    (c_tag_27, ("record tag above 26 or bits above the arena bit",)),
    (c_bit_31, ("record tag above 26 or bits above the arena bit",)),
    (c_slot_twice, ("a slot is named twice",)),
    (c_slot_outside, ("record slot outside its source block's bins",)),
    (c_particle_elsewhere, ("a record's particle does not lie in the record's block",)),
    (c_arena_in_sliced, ("arena bit in the sliced layout",)),
    (c_swap_across_pair_slots, ("pair slot of two keys",)),
    (c_pairinfo_plus, ("pair slot of two keys", "pairs and singles do not add up to the key counts", "two singles of one key", "pairinfo out of range")),
    (c_pairinfo_minus, ("two singles of one key", "pairs and singles do not add up to the key counts", "mismatched slots")),
    (c_pairinfo_second_chunk, ("pair slot of two keys", "pairs and singles do not add up to the key counts", "two singles of one key", "pairinfo out of range")),
    (c_arena_flipped_on_a_pair, ("arena of a pair slot is not its lane parity",)),
    (c_arena_flipped_on_a_single, ("arena rule of a single",)),
    (c_sliced_order, ("sliced layout: keys not in key-major order",)),
    (c_row_source_lane, ("row: source lane",)),
    (c_row_destination_lane, ("row: destination lane",)),
    (c_row_grid_lane, ("row: grid block lane",)),
    (c_row_minus_one_made_zero, ("row: destination lane", "row: grid block lane")),
    (c_row_source_minus_one_made_zero, ("row: source lane",)),
    (c_row_unused_lane, ("row: unused lane",)),
    (c_row_mirrored, ("row: destination lane",)),
]


@pytest.mark.parametrize("corrupt,expected", CORRUPTIONS, ids=[c.__name__ for c, _ in CORRUPTIONS])
def test_every_single_field_corruption_is_reported(built, corrupt, expected):
    ckpt, rows = built[0].copy(), [r.copy() for r in built[1]]
    corrupt(ckpt, rows)
    found = rb.check_books(ckpt, rows, BITS, MAX_PPC)
    assert found, "the corruption went unnoticed"
    assert any(f[0] in expected for f in found), (expected, [f[0] for f in found][:8])


def test_what_nobody_reads_is_not_reported(built):
    """pairinfo entries past a block's last chunk, and a source lane whose block was no particle block of the previous numbering (the kernel loads
    whatever binoff_src holds there)."""
    ckpt, rows = built[0].copy(), [r.copy() for r in built[1]]
    h = cf.parse(ckpt)
    size = _sec(ckpt, ("size", 0))[:h["pbc"]]
    pinfo = _sec(ckpt, ("pairinfo", 0)).reshape(-1, 16)
    for b in range(h["pbc"]):
        pinfo[b, len(rmod.pair_chunks(int(size[b]))):] = 12345
    con = _constrained(ckpt)
    b, l = _lane(ckpt, rows, 0, range(27), lambda b, l, v: v != -1 and not con(b, l, v))
    rows[0][b, l] = 777
    assert rb.check_books(ckpt, rows, BITS, MAX_PPC) == []


# ---- (c) the reference's own book ------------------------------------------------------------------------------------------------------------
def test_tiers_and_particle_sets_accept_the_references_own_book():
    """tests/golden/g20_*: the reference's set-up on 174 particles at 256^3 (its statements, run serially): the tier and particle-set parts of the
    verifier accept it - and notice one key moved, one size changed, one bucket entry moved."""
    from test_oracle_golden import book_tables
    T = book_tables()
    pos_keys = gm.block_keys(T["xyz"].astype(np.float32) * np.float32(256.0))
    keys, sizes, buckets = T["keys0"], T["sizes0"][:T["pbc0"]], T["buckets0"]
    have = set(map(tuple, pos_keys.tolist()))
    listed_in = np.repeat(np.arange(T["pbc0"]), sizes)
    assert buckets.size >= listed_in.size and np.unique(buckets[:listed_in.size]).size == T["n"]
    assert rb.tier_findings(keys, T["pbc0"], T["nbc0"], T["ebc0"], have, 64) == []
    assert rb.census_findings(keys, T["pbc0"], sizes, pos_keys[buckets[:listed_in.size]], listed_in) == []
    k2 = keys.copy()
    k2[[T["pbc0"], T["nbc0"]]] = k2[[T["nbc0"], T["pbc0"]]]
    assert [f[0] for f in rb.tier_findings(k2, T["pbc0"], T["nbc0"], T["ebc0"], have, 64)] == ["neighbour tier", "exterior tier"]
    s2 = sizes.copy()
    s2[0] += 1
    assert rb.census_findings(keys, T["pbc0"], s2, pos_keys[buckets[:listed_in.size]], listed_in)
    b2 = buckets[:listed_in.size].copy()
    b2[[0, -1]] = b2[[-1, 0]]
    assert rb.census_findings(keys, T["pbc0"], sizes, pos_keys[b2], listed_in)


# ---- (d) the still-step model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,nblocks", [(1, 3), (2, 20), (3, 90)])
def test_the_still_step_model_agrees_when_nobody_moves(seed, nblocks):
    """bits 5 (8 blocks per axis, the still model's grid): a random partition, nobody changes block; this model under the identity numbering and
    tests/test_still_rebuild_model_cpu.still_step write the same keys, sizes, row_of, bin offsets and rows."""
    assert still.G == 8
    rng = np.random.default_rng(seed)
    cells = rng.permutation(8 ** 3)[:nblocks]
    pkeys = np.stack([cells // 64, (cells // 8) % 8, cells % 8], axis=1)
    n = rng.integers(1, 200, nblocks)
    pos = np.concatenate([_block(k, c, rng) for k, c in zip(pkeys, n)])
    prev = rmod.make_prev(5, 16, [(4, rmod.PAIR_LAYOUT, pos)], rng)
    new = np.concatenate([_block(k, c, rng) for k, c in zip(pkeys, n)])
    ckpt, rows = rmod.rebuild(prev, [(new, rng.integers(0, 216, pos.shape[0]))], seed=seed, order="identity")
    assert rb.check_books(ckpt, rows, 5, 16) == []
    h = cf.parse(ckpt)
    pbc, ebc = prev["pbc"], prev["ebc"]
    binoff = prev["models"][0]["binoff"]
    # the rows G2P2G has just run with: those of the previous numbering against SOME numbering before it
    perm = rng.permutation(ebc)
    table = -np.ones(8 ** 3, dtype=np.int64)
    for i, k in enumerate(prev["keys"]):
        table[still.key_index(k)] = i
    before = np.where(table >= 0, perm[np.maximum(table, 0)], -1)
    rows0 = np.array([still.build_row(prev["keys"][b], table, before, rng.integers(0, 1000, ebc)) for b in range(pbc)])
    size = np.bincount(prev["models"][0]["where"][:, 0], minlength=pbc)
    new_keys, new_table, s_size, s_row_of, s_binoff, s_rows, _ = still.still_step(prev["keys"], ebc, pbc, size, binoff, rows0)
    assert (h["pbc"], h["ebc"]) == (pbc, ebc) and np.array_equal(cf.cur_keys(ckpt), new_keys)
    assert np.array_equal(cf.section(ckpt, h, ("size", 0), np.int32)[:pbc], s_size)
    assert np.array_equal(cf.section(ckpt, h, ("row_of", 0), np.int32)[:pbc], s_row_of)
    assert np.array_equal(cf.section(ckpt, h, ("binoff_dst", 0), np.int32)[:pbc], s_binoff)
    assert np.array_equal(rows[0], s_rows)


# ---- the scenes of the GPU test, on the model alone -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {name: make() for name, make in rs.GENERATORS.items()}


@pytest.mark.parametrize("name", list(rs.GENERATORS))
def test_few_particles_of_a_scene_hang_on_a_rounding_tie(scenes, name):
    """At most 1 % of a scene's particles may be left out of the sort-key comparison (rebuild_scenes.TIE_CAP), nobody is lost (every particle
    lands in its block or a neighbour of it), and every particle stays inside the domain."""
    sc = scenes[name]
    for (mat, pos), m in zip(sc["parts"], rs.model(sc)):
        out = ~rs.decided(m, sc["tier"], mat)
        print(name, gm.NAMES[mat], "particles", pos.shape[0], "left out", int(out.sum()))
        assert out.sum() <= rs.TIE_CAP * pos.shape[0]
        assert m["dir_ok"].all() and m["finite"].all()
        nk = gm.block_keys(m["pos"])
        assert ((nk >= 0) & (nk < G)).all() and (m["new_base"] >= 0).all() and (m["new_base"] + 2 < 4 * G).all()
        assert ((gm.stencil_base(pos) >= 0) & (gm.stencil_base(pos) + 2 < 4 * G)).all()


def test_the_scenes_hold_what_they_promise(scenes):
    m = rs.model(scenes["tiers_flow"])[0]
    k = gm.block_keys(scenes["tiers_flow"]["parts"][0][1])
    at_face = ((k == 0) | (k == G - 1)).sum(axis=1)
    assert np.unique(k, axis=0).shape[0] == k.shape[0] == 26 and (at_face == 1).sum() == 6 and (at_face == 2).sum() == 4 and (at_face == 3).sum() == 4
    for name in ("sizes_jfluid", "sizes_sand"):
        sc = scenes[name]
        m = rs.model(sc)[0]
        _, cnt = np.unique(gm.block_keys(m["pos"]), axis=0, return_counts=True)
        assert (m["dirtag"] == 13).all() and sorted(cnt.tolist()) == sorted(rs.SIZES)
    m = rs.model(scenes["one_cell"])[0]
    kb = np.concatenate([gm.block_keys(m["pos"]), m["sort_key"][:, None]], axis=1)
    assert np.unique(kb, axis=0).shape[0] == 3 and (m["dirtag"] == 13).all()          # one key in the first block, two in the second
    for name, counts in (("all_keys", [4] * 216), ("odd_keys", [(1, 3, 5)[k % 3] for k in range(216)])):
        m = rs.model(scenes[name])[0]
        assert (m["dirtag"] == 13).all() and np.array_equal(np.bincount(m["sort_key"], minlength=216), counts)
    # migration: the burst block is left empty and its 26 neighbours filled, the swap blocks trade places
    sc = scenes["migration"]
    m = rs.model(sc)[0]
    old, new = gm.block_keys(sc["parts"][0][1]), gm.block_keys(m["pos"])
    burst = (old == np.array(rs.BURST)).all(axis=1)
    assert burst.sum() == 104 and not (new == np.array(rs.BURST)).all(axis=1).any()
    assert np.unique(new[burst] - old[burst], axis=0).shape[0] == 26 and np.unique(m["dirtag"][burst]).size == 26
    for a, b in (rs.SWAP, rs.SWAP[::-1]):
        sel = (old == np.array(a)).all(axis=1)
        assert sel.sum() == 300 and (new[sel] == np.array(b)).all()
    sc = scenes["two_models"]
    ka, kb = (set(map(tuple, gm.block_keys(p).tolist())) for _, p in sc["parts"])
    assert len(ka & kb) == 8 and len(ka - kb) == 3 and len(kb - ka) == 3
    sc = scenes["drop"]
    m = rs.model(sc)[0]
    new = gm.block_keys(m["pos"])
    assert (new == np.array(rs.DROP[1])).all() and new.shape[0] == 1200


def test_the_sort_keys_inputs_are_the_references_on_the_golden_rows():
    """The reference has no sort key (it is this engine's own), so the model's prediction has no outside yardstick; its integer inputs have: on
    the 960 golden rows the new stencil base and the coordinate in the source block's node cube (narena) are the reference's own, and the key is
    a valid one (0 .. 215)."""
    P, arenas, rin, wf, wi = gm.golden_rows()
    for material in gm.MATERIALS:
        rows = np.flatnonzero((rin[:, 0] == material) & (rin[:, 1] < 3))
        m = gm.golden_model(material, P, arenas, rin[rows])
        assert ((m["sort_key"] >= 0) & (m["sort_key"] < 216)).all()
        assert np.array_equal(m["new_base"], wi[rows, 6:9].astype(np.int64) + 1)
        kept = wi[rows, 13] == 0
        assert kept.sum() >= 100 and np.array_equal(m["narena"][kept], wi[rows, 10:13][kept].astype(np.int64)) and np.array_equal(m["discarded"], ~kept)

"""A numpy model of the still step of the partition rebuild (claymore_amd/csrc/mpm_kernels.hpp: compact_blocks_kernel and
prepare_blocks_kernel with `still`) on a random small partition: keys, table, sizes, bin offsets and the 64-int look-up rows, built the way the
kernels build them.  The still step must arrive where a full rebuild of the same block set under the identity numbering arrives."""
import numpy as np
import pytest

G = 8            # blocks per axis
ROW = 64         # kInfoRow: [0, 27) source bin offsets, [27, 54) destination block numbers, [54, 62) grid blocks, 62 / 63 unused (-1)


def direction(j):
    """dir_components: j -> (dx, dy, dz), z fastest"""
    return np.array([j // 9 - 1, (j // 3) % 3 - 1, j % 3 - 1])


def key_index(k):
    return (int(k[0]) * G + int(k[1])) * G + int(k[2])


def query(table, k):
    return int(table[key_index(k)]) if all(0 <= int(v) < G for v in k) else -1


def build_partition(rng, nparticle):
    """particle blocks in random order, then the neighbour phase (offsets 0..1) and the exterior phase (-1..1) in registration order"""
    cells = rng.permutation(G ** 3)[:nparticle]
    keys = [np.array([c // (G * G), (c // G) % G, c % G]) for c in cells]
    table = -np.ones(G ** 3, dtype=np.int64)
    for i, k in enumerate(keys):
        table[key_index(k)] = i
    pbc = len(keys)
    for lo in (0, -1):
        for b in range(pbc):
            for o in np.ndindex(1 - lo + 1, 1 - lo + 1, 1 - lo + 1):
                k = keys[b] + np.array(o) + lo
                if all(0 <= v < G for v in k) and table[key_index(k)] < 0:
                    table[key_index(k)] = len(keys)
                    keys.append(k)
        if lo == 0:
            nbc = len(keys)
    return np.array(keys), table, pbc, nbc, len(keys)


def build_row(key, cur_table, prev_table, binoff_src):
    """prepare_blocks_kernel's look-ups for one block"""
    row = -np.ones(ROW, dtype=np.int64)
    for lane in range(27):
        src = query(prev_table, key + direction(lane))
        row[lane] = binoff_src[src] if src >= 0 else -1
        row[27 + lane] = query(cur_table, key - direction(lane))
    for lb in range(8):
        row[54 + lb] = query(cur_table, key + np.array([(lb >> 2) & 1, (lb >> 1) & 1, lb & 1]))
    return row


def still_step(keys, ebc, pbc, out_count, binoff_cur, rows):
    """What the still path writes: the new keys / table / sizes / rows of the identity numbering."""
    new_keys = keys[:ebc].copy()
    new_table = -np.ones(G ** 3, dtype=np.int64)            # (substep_clear_kernel has un-inserted the table that is written)
    for b in range(ebc):
        new_table[key_index(new_keys[b])] = b
    size, row_of, binoff_next = out_count[:pbc].copy(), np.arange(pbc), binoff_cur[:pbc].copy()
    new_rows = rows.copy()
    srcno = np.empty((pbc, 27), dtype=np.int64)
    for b in range(pbc):
        for lane in range(27):
            srcno[b, lane] = rows[b, 53 - lane]
            new_rows[b, lane] = binoff_cur[srcno[b, lane]] if srcno[b, lane] >= 0 else -1
    return new_keys, new_table, size, row_of, binoff_next, new_rows, srcno


def binoff_next_full(binoff_next, binoff_cur):
    """the buffer the first still step wrote (particle blocks) with whatever lies behind them"""
    return np.concatenate([binoff_next, binoff_cur[len(binoff_next):]])


@pytest.mark.parametrize("seed,nparticle", [(1, 1), (2, 7), (3, 60), (4, 200), (5, G ** 3)])
def test_still_step_is_the_rebuild_under_the_identity_numbering(seed, nparticle):
    rng = np.random.default_rng(seed)
    keys, table, pbc, nbc, ebc = build_partition(rng, nparticle)
    assert pbc <= nbc <= ebc and (nparticle < 60 or (keys[:pbc] == 0).any() or (keys[:pbc] == G - 1).any())      # (blocks at the domain's faces: -1 entries)
    size = rng.integers(1, 300, pbc)
    nbins = (size + 63) // 64
    order = rng.permutation(pbc)                          # bins are handed out in the order of the atomics
    first = np.empty(pbc, dtype=np.int64)
    first[order] = np.concatenate([[0], np.cumsum(nbins[order])[:-1]])
    binoff_cur = np.concatenate([first, rng.integers(0, 1000, ebc - pbc)])        # (behind the particle blocks: whatever was there)
    # the rows of the partition G2P2G has just run in: built against a PREVIOUS numbering that is some permutation of this one
    perm = rng.permutation(ebc)
    prev_table = np.where(table >= 0, perm[np.maximum(table, 0)], -1)
    binoff_prev = rng.integers(0, 1000, ebc)
    rows = np.array([build_row(keys[b], table, prev_table, binoff_prev) for b in range(pbc)])
    new_keys, new_table, new_size, row_of, binoff_next, new_rows, srcno = still_step(keys, ebc, pbc, size, binoff_cur, rows)
    # srcno(l) == info[53 - l] for all 27 directions, the -1 entries included: what the slow path looks up in the table of the partition G2P2G ran in
    for b in range(pbc):
        for lane in range(27):
            assert srcno[b, lane] == query(table, keys[b] + direction(lane))
    assert (srcno == -1).any() or nparticle < 60
    # table[key_index(keys[i])] == i for every i < ebc, and nothing else is in the table
    assert all(new_table[key_index(new_keys[i])] == i for i in range(ebc)) and (new_table >= 0).sum() == ebc
    # row_of is the identity, sizes stand, the bins do not overlap and fill the total the previous rebuild counted
    assert np.array_equal(row_of, np.arange(pbc)) and np.array_equal(new_size, size)
    o = np.argsort(binoff_next)
    assert np.all(binoff_next[o][1:] >= (binoff_next[o] + nbins[o])[:-1]) and binoff_next[o][-1] + nbins[o][-1] == nbins.sum()
    # the rows are those of a full rebuild whose numbering happens to be the identity
    want = np.array([build_row(new_keys[b], new_table, table, binoff_cur) for b in range(pbc)])
    assert np.array_equal(new_rows, want)
    # a second still step in a row finds both bin-offset buffers equal and leaves every row as it is: what lets the kernel pass over settled blocks
    again = still_step(new_keys, ebc, pbc, size, binoff_next_full(binoff_next, binoff_cur), new_rows)
    assert np.array_equal(again[5], new_rows) and np.array_equal(again[4], binoff_next) and np.array_equal(again[1], new_table)

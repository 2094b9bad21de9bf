"""tests/particle_ids_model.py on a synthetic checkpoint (built from the layout arithmetic alone, as test_g2p2g_model_cpu.py builds one for
the state patcher): the blob reader and writer round-trip, the substep's result is a permutation of the live ids, the list positions of both
list layouts are the ones the kernels use."""
import numpy as np
import pytest

import ckpt_format as cf
import particle_ids_model as pim
from test_g2p2g_model_cpu import synthetic_checkpoint

SIZES = np.array([1, 63, 64, 65, 130, 513, 1024, 3])


def test_blob_round_trip():
    rng = np.random.default_rng(1)
    models = [(100, rng.integers(0, 100, 3 * 64).astype(np.int32)), (0, np.zeros(0, np.int32)), (7, rng.integers(-5, 7, 64).astype(np.int32))]
    blob = pim.pack(models)
    assert blob.dtype == np.uint8 and blob.size == 144 + 4 * 64 * 4
    assert bytes(blob[:8]) == b"MPMPIDS1"
    back = pim.unpack(blob)
    assert len(back) == 3
    for (n, ids), (n2, ids2) in zip(models, back):
        assert n == n2 and np.array_equal(ids, ids2)
    assert np.array_equal(pim.pack(back), blob)
    with pytest.raises(AssertionError):
        pim.unpack(blob[:-4])
    bad = blob.copy()
    bad[0] ^= 1
    with pytest.raises(AssertionError):
        pim.unpack(bad)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 130, 200, 511, 512])
def test_sliced_list_positions_are_the_layout_of_the_kernels(n):
    """A chunk of n records: S = ceil(n / 64) slices, slice s holds n / S + (s < n % S) records in its first slots, records in slice-major order."""
    S = (n + 63) // 64
    want = []
    for s in range(S):
        want += [64 * s + j for j in range(n // S + (1 if s < n % S else 0))]
    assert pim.chunk_slot(n, np.arange(n)).tolist() == want
    assert pim.list_positions(n, False).tolist() == want
    assert pim.list_positions(n, True).tolist() == list(range(n))


def test_list_positions_beyond_one_chunk():
    p = pim.list_positions(513, False)
    assert p[:512].tolist() == list(range(512)) and p[512] == 512
    p = pim.list_positions(700, False)                       # the second chunk: 188 records in 3 slices of 63, 63, 62
    assert p[512:].tolist() == [512 + 64 * s + j for s, c in enumerate((63, 63, 62)) for j in range(c)]


@pytest.mark.parametrize("nch", [4, 10])
def test_substep_on_a_synthetic_checkpoint(nch):
    rng = np.random.default_rng(nch)
    buf = synthetic_checkpoint(nch, SIZES, rng)
    h = cf.parse(buf)
    M = h["models"][0]
    n = int(SIZES.sum())
    bin_, slot = cf.particle_slots(buf, 0)
    # ids 0 .. n-1 dealt to the live slots in a random order, noise elsewhere
    ids = rng.integers(-(2 ** 31), 2 ** 31 - 1, M["bincount_src"] * 64).astype(np.int32)
    given = rng.permutation(n).astype(np.int32)
    ids[bin_ * 64 + slot] = given
    blob = pim.pack([(M["n"], ids)])
    assert np.array_equal(pim.live_ids(buf, blob, 0), given)
    dst, moved = pim.substep(buf, blob, 0)
    assert np.array_equal(moved, given) and np.array_equal(np.sort(moved), np.arange(n))
    assert np.unique(dst).size == n
    exp, live = pim.expected_blob_slots(buf, blob, 0)
    assert live.sum() == n and np.array_equal(np.sort(exp[live]), np.arange(n)) and (exp[~live] == -1).all()
    # record i of block b (packed order) goes to the block's destination bins at its list position
    size = cf.section(buf, h, ("size", 0), np.int32)[:h["pbc"]]
    binoff_dst = cf.section(buf, h, ("binoff_dst", 0), np.int32)
    at = 0
    for b, s in enumerate(size.tolist()):
        pos = dst[at:at + s] - 64 * int(binoff_dst[b])
        assert (pos >= 0).all() and (pos < 64 * ((s + 63) // 64)).all(), b
        assert np.array_equal(exp[dst[at:at + s]], given[at:at + s])
        at += s
    # a blob of another checkpoint is refused
    with pytest.raises(AssertionError):
        pim.live_ids(buf, pim.pack([(M["n"] + 1, ids)]), 0)
    with pytest.raises(AssertionError):
        pim.live_ids(buf, pim.pack([(M["n"], ids[:-64])]), 0)

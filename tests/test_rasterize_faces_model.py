"""The index arithmetic of rasterize_blocks_kernel (claymore_amd/csrc/mpm_kernels.hpp) restated in Python and swept over the six faces of the
domain: node N = lround_pos(x / dx), stencil base N - 1, block key (N - 2) / 4 truncating (particle_block_key), cube offset l = base - 4 * key,
LDS index (lx << 6) | (ly << 3) | lz of the block's 8^3 node cube, written only where every l + i is in [0, 8).  The kernel runs on the GPU only
(tests/test_domain_faces_gpu.py compares its grid with the oracle's); this is the statement of what it may write, checked without one.

Also on the CPU: the oracle's set-up grid of the face scenes against a float64 restatement of the reference's rasterize."""
import itertools

import numpy as np
import pytest

import face_scenes as F
from claymore_amd.engine import build_engine
from oracle_ffi import oracle_api


def rasterize_rule(p, n):
    """rasterize_blocks_kernel for particles at cell-unit positions p (M, 3) of a domain of n nodes per axis.  Returns, per stencil node
    (M * 27 rows): whether the kernel writes it to LDS, the LDS index it computes, the global node the cube slot stands for (4 * key + l + i), the
    particle's block key, and the global node of the stencil (base + i) - the node the reference's rasterize adds to."""
    N, base, key, l = F.kernel_axis(np.asarray(p, dtype=np.float32))
    rows = []
    for i, j, k in itertools.product(range(3), repeat=3):
        o = np.array([i, j, k])
        c = l + o                                              # cube coordinates (M, 3)
        ok = np.all((c >= 0) & (c < 8), axis=1)                # (unsigned)(lx + i) < 8u && ... : the guard of the fix
        idx = (c[:, 0] << 6) | (c[:, 1] << 3) | c[:, 2]
        rows.append((ok, idx, 4 * key + c, key, base + o))
    return tuple(np.concatenate([r[f] for r in rows]) for f in range(5))


def face_sweep(n):
    """Cell-unit positions along one axis: every 1/64 cell of the outer four cells at both ends of [0, n), the exact ties k + 0.5 there, and
    the largest float32 below n."""
    lo = np.concatenate([np.arange(0, 4, 1 / 64), np.arange(0, 4) + 0.5, [0.49, 0.51, np.nextafter(np.float32(0.5), np.float32(0))]])
    hi = n - lo[lo > 0]
    return np.unique(np.concatenate([lo, hi, [np.nextafter(np.float32(n), np.float32(0))]]).astype(np.float32))


def six_face_points(n):
    """The sweep on each axis with the other two axes at the middle, at the lower corner and at the upper corner: all six faces, the
    twelve edges and the eight corners."""
    s = face_sweep(n)
    others = np.array([n / 2, 0.25, 0.0, 1.5, n - 0.01, n - 1.5], dtype=np.float32)
    pts = []
    for axis in range(3):
        for a, b in itertools.product(others, repeat=2):
            q = np.empty((s.size, 3), dtype=np.float32)
            q[:, axis] = s
            rest = [d for d in range(3) if d != axis]
            q[:, rest[0]], q[:, rest[1]] = a, b
            pts.append(q)
    return np.concatenate(pts)


@pytest.mark.parametrize("bits", [4, 5, 6, 10])
def test_lds_writes_stay_in_the_cube_and_drop_exactly_the_nodes_below_the_domain(bits):
    n = 1 << bits
    p = six_face_points(n)
    N, _, key, _ = F.kernel_axis(p)
    assert np.all((key >= 0) & (key < n // 4))               # every particle of [0, 1) has a block: set-up accepts it (no ST_LOST)
    written, idx, slot_node, keys, node = rasterize_rule(p, n)
    assert np.all((idx[written] >= 0) & (idx[written] < 512))
    assert np.array_equal(~written, np.any(node < 0, axis=1))  # dropped <=> the node has a negative global index
    assert np.array_equal(slot_node[written], node[written])    # the slot stands for the node the stencil means (the write-back's block + cell)
    # the write-back's block offset (slot >> 2) - the block queried is key + 0 or key + 1
    off = (slot_node[written] >> 2) - keys[written]
    assert np.all((off >= 0) & (off <= 1))
    assert np.array_equal(np.any(N == 0, axis=1), np.any(p < 0.5, axis=1)) and (~written).any()   # (the sweep does reach node -1)


@pytest.mark.parametrize("bits", [4, 5, 6, 10])
def test_written_nodes_are_the_oracles_nodes(bits):
    """After the write-back (table_query: blocks outside [0, G)^3 have no entry) the kernel adds to the nodes the oracle adds to:
    base from the reference's round-half-away-from-zero, nodes whose block gx >> 2 is inside the table (oracle/mpm_oracle.c, rasterize)."""
    n = 1 << bits
    p = six_face_points(n)
    written, _, slot_node, _, node = rasterize_rule(p, n)
    kept = written & np.all(slot_node >> 2 < n // 4, axis=1)
    base_ref = F.lround_half_away(p) - 1
    ref_nodes = np.concatenate([base_ref + np.array(o) for o in itertools.product(range(3), repeat=3)])
    ref_kept = np.all((ref_nodes >> 2 >= 0) & (ref_nodes >> 2 < n // 4), axis=1)
    assert np.array_equal(node, ref_nodes)                      # lround_pos == lround for p >= 0, ties included
    assert np.array_equal(kept, ref_kept)


def test_lround_pos_at_ties():
    k = np.arange(0, 1024, dtype=np.float32)
    for p in (k + np.float32(0.5), k, k + np.float32(0.49), k + np.float32(0.51)):
        assert np.array_equal(F.lround_pos(p), F.lround_half_away(p))
    assert np.array_equal(F.lround_pos(k + np.float32(0.5)), k.astype(np.int64) + 1)   # away from zero at even and odd k


def test_the_unguarded_index_falls_below_the_array_only_at_the_lower_faces():
    """What the kernel did before the range check: (lx + i) << 6 | ... with lx + i = -1 is a negative LDS index (any negative component makes
    the OR negative).  That happens exactly for particles with x / dx < 0.5 on some axis (node 0, cell -2); the upper faces stay inside."""
    n = 64
    p = six_face_points(n)
    _, _, _, l = F.kernel_axis(p)
    for i, j, k in itertools.product(range(3), repeat=3):
        c = l + np.array([i, j, k])
        raw = (c[:, 0] << 6) | (c[:, 1] << 3) | c[:, 2]
        below = np.any(c < 0, axis=1)
        assert np.array_equal(raw < 0, below)
        assert np.all(raw[~below] < 512)
    assert np.array_equal(np.any(l < 0, axis=1), np.any(p < 0.5, axis=1))


def test_face_slab_scene_reaches_node_minus_one():
    """The set-up scene of the GPU test puts mass on node -1 (what the unguarded kernel wrote below its LDS array) and on nodes beyond the
    upper faces (dropped by the write-back's table_query)."""
    sc = F.setup_slab_scene(5)
    ref, outside = F.reference_setup_grid(sc)
    total = sum(v[0] for v in ref.values())
    assert outside["lo"] > 0.01 * total and outside["hi"] > 0.01 * total, (outside, total)


@pytest.mark.parametrize("bits", [5, 6])
def test_oracle_setup_grid_at_the_faces_matches_float64(bits):
    """The oracle's rasterize on the face scene against the float64 restatement, node by node: the nodes beyond every face receive nothing,
    every other stencil node its mass * w (relative to the heaviest node: float32 weights and sums)."""
    sc = F.setup_slab_scene(bits)
    ref, _ = F.reference_setup_grid(sc)
    ref = {nd: v for nd, v in ref.items() if v[0] > 0}          # (a node at weight exactly 0: a tie's third node)
    eng = build_engine(sc, api=oracle_api())
    eng.initial_setup()
    keys, blocks = eng.dump_grid()
    eng.close()
    got = F.grid_to_nodes(keys, blocks)
    assert set(got) == set(ref)
    scale = max(v[0] for v in ref.values())
    worst = max(float(np.abs(got[nd] - ref[nd]).max()) for nd in ref) / scale
    assert worst < 1e-6, worst

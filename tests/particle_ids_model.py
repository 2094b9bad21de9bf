"""Host model of persistent particle identities (claymore_amd/csrc/mpm_particle_ids.hpp): the blob format of mpm_particle_ids_save and the
permutation one substep applies to the ids, from ONE checkpoint alone.

The blob: a 144-byte header {uint64 magic "MPMPIDS1", int32 model count, int32 0, 8 x {int64 n, int64 bincount_src}}, then per model one
int32 per slot of the source bins - 64 per bin, bincount_src bins -, in the slot order of the checkpoint's bins section, so the (bin, slot)
addresses of ckpt_format.particle_slots index it directly: ids[bin * 64 + slot].

The substep: G2P2G stores the particle of list position p of current block b at slot p of the block's destination bins, whose first bin is
binoff_dst[b]; after the rebuild's roll those are the source bins of the next checkpoint.  So with (bin, slot) per record of checkpoint k
    expected[binoff_dst[b] * 64 + p] = ids_k[bin * 64 + slot]
is what the blob of checkpoint k + 1 holds in every slot named on the left (its other slots are unspecified).  The checkpoint packs a block's
records without holes; in the pair layout the i-th packed record sits at list position p = i, in the sliced layout (chunks of 512 records cut
into ceil(n / 64) slices of 64 slots, mpm_kernels.hpp) at chunk * 512 + chunk_slot(n, i)."""
import numpy as np

import ckpt_format as cf

MAGIC = int.from_bytes(b"MPMPIDS1", "little")
HEADER_BYTES = 16 + 16 * cf.MAX_MODELS
K_LIST_CHUNK = 512


def pack(models):
    """models: [(n, ids int32 (bincount_src * 64,))] -> the blob as a uint8 array"""
    assert len(models) <= cf.MAX_MODELS
    head = np.zeros(HEADER_BYTES, np.uint8)
    head[:8].view(np.uint64)[0] = MAGIC
    head[8:16].view(np.int32)[:] = [len(models), 0]
    body = []
    for m, (n, ids) in enumerate(models):
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        assert ids.size % cf.K_BIN == 0
        head[16 + 16 * m:32 + 16 * m].view(np.int64)[:] = [n, ids.size // cf.K_BIN]
        body.append(ids.view(np.uint8))
    return np.concatenate([head] + body)


def unpack(blob):
    """the blob -> [(n, ids int32 (bincount_src * 64,))]; asserts the magic and the length"""
    blob = np.ascontiguousarray(blob, np.uint8)
    assert blob.size >= HEADER_BYTES, "truncated header"
    assert int(blob[:8].view(np.uint64)[0]) == MAGIC, "bad magic"
    nm, zero = blob[8:16].view(np.int32).tolist()
    assert 0 <= nm <= cf.MAX_MODELS and zero == 0
    out, at = [], HEADER_BYTES
    for m in range(nm):
        n, bc = blob[16 + 16 * m:32 + 16 * m].view(np.int64).tolist()
        nbytes = 4 * cf.K_BIN * bc
        out.append((int(n), blob[at:at + nbytes].view(np.int32).copy()))
        at += nbytes
    assert at == blob.size, (at, blob.size)
    return out


def chunk_slot(n, i):
    """slot of the i-th record (slice-major) of a chunk with n records in the sliced layout (chunk_slot, mpm_kernels.hpp); i: int array"""
    S = (n + 63) // 64
    q, r = divmod(n, S)
    big = r * (q + 1)
    i = np.asarray(i, np.int64)
    lo_sl = i // (q + 1)
    j = i - big
    hi_sl = j // max(q, 1)
    return np.where(i < big, lo_sl * 64 + (i - lo_sl * (q + 1)), (r + hi_sl) * 64 + (j - hi_sl * q))


def list_positions(size, dense):
    """list position p of every packed record of a block with `size` records"""
    i = np.arange(size, dtype=np.int64)
    if dense:
        return i
    p = np.empty(size, np.int64)
    for c0 in range(0, size, K_LIST_CHUNK):
        n = min(K_LIST_CHUNK, size - c0)
        p[c0:c0 + n] = c0 + chunk_slot(n, np.arange(n))
    return p


def destination_slots(ckpt, m):
    """Per packed list record of model m, in the order of ckpt_format.particle_slots: its slot in the destination bins, binoff_dst[b] * 64 + p."""
    h = cf.parse(ckpt)
    M = h["models"][m]
    size = cf.section(ckpt, h, ("size", m), np.int32)[:h["pbc"]].astype(np.int64)
    binoff_dst = cf.section(ckpt, h, ("binoff_dst", m), np.int32).astype(np.int64)
    out = [binoff_dst[b] * cf.K_BIN + list_positions(int(s), M["layout"] != 0) for b, s in enumerate(size)]
    dst = np.concatenate(out) if out else np.zeros(0, np.int64)
    assert dst.size == M["bucketed"]
    assert np.unique(dst).size == dst.size, "two records go to one slot"
    assert dst.size == 0 or dst.max() < M["bincount"] * cf.K_BIN
    return dst


def live_ids(ckpt, blob, m):
    """The ids of model m's bucketed particles in the order of ckpt_format.particle_slots."""
    n, ids = unpack(blob)[m]
    M = cf.parse(ckpt)["models"][m]
    assert n == M["n"] and ids.size == M["bincount_src"] * cf.K_BIN, "the blob does not belong to this checkpoint"
    bin_, slot = cf.particle_slots(ckpt, m)
    return ids[bin_ * cf.K_BIN + slot]


def substep(ckpt, blob, m):
    """One substep from checkpoint k and its blob: (dst, ids) - the next blob of model m holds ids[j] at flat slot dst[j]."""
    return destination_slots(ckpt, m), live_ids(ckpt, blob, m)


def expected_blob_slots(ckpt, blob, m):
    """(expected int32 (bincount * 64,), live bool mask): the next blob's array of model m where it is specified."""
    dst, ids = substep(ckpt, blob, m)
    n = cf.parse(ckpt)["models"][m]["bincount"] * cf.K_BIN
    exp, live = np.full(n, -1, np.int32), np.zeros(n, bool)
    exp[dst], live[dst] = ids, True
    return exp, live

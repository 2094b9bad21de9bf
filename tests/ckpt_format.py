"""Reader / patcher of checkpoint format 7 (claymore_amd/csrc/mpm_checkpoint.inc): a plain numpy restatement of CkptHeader and
ckpt_layout.  The header is 448 bytes; every section starts at a multiple of 16 bytes (its length is rounded up to one).  Section order:
cur_keys (3 ints per exterior block), prev_keys (3 ints per block of the previous numbering), grid (256 floats per NEIGHBOUR block:
{mass, momentum x, y, z} x 64 cells), then per model size / row_of / binoff_src / binoff_dst / bins / lists / pairinfo.

mpm_checkpoint_load validates every index of a checkpoint and copies the grid section verbatim: with_grid() therefore puts any bit pattern
into any cell of any block of a context (tests/test_grid_update_kernels_gpu.py).  The bins section is copied verbatim too, and the loader
reads none of it: with_particle_state() puts any material state into the slots of chosen particles and leaves their positions - and with
them every list, size and pair count - as they were (tests/test_g2p2g_blocks_gpu.py).

A bin (fill_bins_kernel, claymore_amd/csrc/mpm_kernels.hpp) holds 64 records of `rec` floats - 4 for the J-fluid {x/dx, y/dx, z/dx, J}, 8 for
the solids {x/dx, y/dx, z/dx, b00, b11, b22, b10, b20} - and behind them one row entry of nch - rec floats per slot: b21 (fixed-corotated),
{b21, log Jp} (sand, NACC).  The sign bit of b00 marks a reflected F.

list_records / record_positions / source_extents / key_map read the advection lists field by field without judging them: the verifier of
tests/rebuild_books.py reports what particle_slots would assert."""
import numpy as np

HEADER_BYTES = 448
MAGIC = 0x3754504B434D504D            # "MPMCKPT7"
K_BIN = 64                            # particles per bin (kBin)
K_PAIR_CHUNKS = 16                    # pair counts per particle block in the pair layout (kPairChunks)
K_KEY_BITS = 8                        # sort-key bits of an advection record, between the slot and the direction tag (kKeyBits)
MAX_MODELS = 8
MODEL_BYTES = 48                      # CkptModel: 4 x int32 {material, nch, list_in, layout}, 4 x int64 {n, bincount, bincount_src, bucketed}
_MODELS_AT = 64
SECTIONS = ("size", "row_of", "binoff_src", "binoff_dst", "bins", "lists", "pairinfo")


def pad16(nbytes):
    return (int(nbytes) + 15) & ~15


def header(buf):
    """The counts of a checkpoint's header as a dict (models: one dict per model in use)."""
    raw = np.ascontiguousarray(buf, dtype=np.uint8)[:HEADER_BYTES].tobytes()
    assert len(raw) == HEADER_BYTES, "truncated header"
    i32 = np.frombuffer(raw, np.int32)
    u64 = np.frombuffer(raw, np.uint64)
    h = {"magic": int(u64[0]), "domain_bits": int(i32[2]), "max_ppc": int(i32[3]), "nmodels": int(i32[4]), "rollid": int(i32[5]),
         "pbc": int(i32[6]), "nbc": int(i32[7]), "ebc": int(i32[8]), "prev_count": int(i32[9]), "total_bytes": int(u64[5]),
         "param_hash": int(u64[6]), "prev_pbc": int(i32[14]), "grid_velocity": int(i32[15]), "models": []}
    assert 0 <= h["nmodels"] <= MAX_MODELS
    for m in range(h["nmodels"]):
        at = _MODELS_AT + MODEL_BYTES * m
        a = np.frombuffer(raw[at:at + 16], np.int32)
        b = np.frombuffer(raw[at + 16:at + 48], np.int64)
        h["models"].append({"material": int(a[0]), "nch": int(a[1]), "list_in": int(a[2]), "layout": int(a[3]),
                            "n": int(b[0]), "bincount": int(b[1]), "bincount_src": int(b[2]), "bucketed": int(b[3])})
    return h


def layout(h):
    """ckpt_layout: {section: (offset, bytes in use)} and the end of the last section.  Per-model sections are keyed (name, model)."""
    o, out = HEADER_BYTES, {}

    def take(name, nbytes):
        nonlocal o
        out[name] = (o, int(nbytes))
        o += pad16(nbytes)
    take("cur_keys", 4 * 3 * h["ebc"])
    take("prev_keys", 4 * 3 * h["prev_count"])
    take("grid", 4 * 256 * h["nbc"])
    for m, M in enumerate(h["models"]):
        take(("size", m), 4 * (h["ebc"] + 1))
        take(("row_of", m), 4 * (h["ebc"] + 1))
        take(("binoff_src", m), 4 * (h["prev_count"] + 1))
        take(("binoff_dst", m), 4 * (h["ebc"] + 1))
        take(("bins", m), 4 * M["bincount_src"] * M["nch"] * K_BIN)
        take(("lists", m), 4 * M["bucketed"])
        take(("pairinfo", m), 4 * h["pbc"] * K_PAIR_CHUNKS if M["layout"] else 0)
    return out, o


def parse(buf):
    """Counts and section offsets of a checkpoint: the header dict plus "sections" and "end".  Asserts what the loader asserts about the
    size, and that the grid was saved as momenta (grid_velocity 0): a patched grid is a P2G result, not an updated grid."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    h = header(buf)
    assert h["magic"] == MAGIC, hex(h["magic"])
    sections, end = layout(h)
    assert h["total_bytes"] == end == buf.size, (h["total_bytes"], end, buf.size)
    assert h["grid_velocity"] == 0, "the checkpoint's grid holds velocities"
    h["sections"], h["end"] = sections, end
    return h


def section(buf, h, name, dtype):
    at, n = h["sections"][name]
    return np.ascontiguousarray(buf, dtype=np.uint8)[at:at + n].view(dtype)


def cur_keys(buf):
    h = parse(buf)
    return section(buf, h, "cur_keys", np.int32).reshape(-1, 3)


def grid(buf):
    """View (nbc, 4, 64) float32 of the grid section (a view of `buf` where buf is a contiguous uint8 array)."""
    h = parse(buf)
    return section(buf, h, "grid", np.float32).reshape(h["nbc"], 4, 64)


def with_grid(buf, new):
    """A new buffer: `buf` with its grid section replaced by `new` ((nbc, 4, 64) float32 or uint32 bit patterns), everything else byte for byte."""
    h = parse(buf)
    new = np.ascontiguousarray(new)
    assert new.shape == (h["nbc"], 4, 64) and new.dtype in (np.float32, np.uint32), (new.shape, new.dtype)
    out = np.ascontiguousarray(buf, dtype=np.uint8).copy()
    at, n = h["sections"]["grid"]
    out[at:at + n] = new.view(np.uint8).reshape(-1)
    return out


def bins(buf, m):
    """View (bincount_src, nch * 64) float32 of model m's bins section (a view of `buf` where buf is a contiguous uint8 array)."""
    h = parse(buf)
    M = h["models"][m]
    return section(buf, h, ("bins", m), np.float32).reshape(M["bincount_src"], M["nch"] * K_BIN)


def rec_floats(nch):
    return 4 if nch == 4 else 8


def particle_slots(buf, m):
    """Where every bucketed particle of model m lives: (bin, slot) int arrays in the order of the packed advection lists, found the way
    G2P2G finds them - record = (direction tag t, slot s in the source block), the source block is the block of the PREVIOUS numbering at
    the current block's key + dir_components(t), its first bin binoff_src[that block].  Right after set-up this is each block's bins up to
    size[b]; after a rebuild it follows the particles that changed block.  Asserts that no slot is named twice."""
    h = parse(buf)
    M = h["models"][m]
    ppb = K_BIN * h["max_ppc"]
    tag_shift = (ppb.bit_length() - 1) + K_KEY_BITS
    keys = section(buf, h, "cur_keys", np.int32).reshape(-1, 3)
    prev = {tuple(k): i for i, k in enumerate(section(buf, h, "prev_keys", np.int32).reshape(-1, 3).tolist())}
    size = section(buf, h, ("size", m), np.int32)[:h["pbc"]]
    binoff = section(buf, h, ("binoff_src", m), np.int32)
    recs = section(buf, h, ("lists", m), np.int32).view(np.uint32)
    assert int(size.sum()) == M["bucketed"] == recs.size
    blk = np.repeat(np.arange(h["pbc"]), size)
    tag = ((recs >> np.uint32(tag_shift)) & np.uint32(31)).astype(np.int64)
    sp = (recs & np.uint32(ppb - 1)).astype(np.int64)
    assert (tag <= 26).all()
    src_key = keys[blk].astype(np.int64) + np.stack([tag // 9 - 1, (tag // 3) % 3 - 1, tag % 3 - 1], axis=1)
    src = np.array([prev.get(tuple(k), -1) for k in src_key.tolist()], dtype=np.int64).reshape(-1)
    assert (src >= 0).all() and (src < h["prev_pbc"]).all(), "a record names a block the previous numbering does not hold"
    bin_ = binoff[src].astype(np.int64) + (sp >> 6)
    slot = sp & 63
    assert (bin_ < M["bincount_src"]).all()
    assert np.unique(bin_ * K_BIN + slot).size == recs.size, "two records name one slot"
    return bin_, slot


def particle_state(buf, m):
    """Every bucketed particle of model m as the bins hold it, in the order of particle_slots: {"xyz_cells" (n, 3), "b" (n, 6) in the order
    {00, 11, 22, 10, 20, 21} with |b00|, "reflected" (n,), "logjp" (n,), "J" (n,)} - float32; entries a material does not carry are None."""
    M = parse(buf)["models"][m]
    nch, rec = M["nch"], rec_floats(M["nch"])
    B = bins(buf, m)
    bin_, slot = particle_slots(buf, m)
    R = B[bin_[:, None], slot[:, None] * rec + np.arange(rec)[None, :]]
    out = {"xyz_cells": R[:, :3].copy(), "b": None, "reflected": None, "logjp": None, "J": None}
    if nch == 4:
        out["J"] = R[:, 3].copy()
        return out
    row = nch - rec
    b21 = B[bin_, K_BIN * rec + slot * row]
    out["reflected"] = np.signbit(R[:, 3])
    out["b"] = np.stack([np.abs(R[:, 3]), R[:, 4], R[:, 5], R[:, 6], R[:, 7], b21], axis=1)
    if row == 2:
        out["logjp"] = B[bin_, K_BIN * rec + slot * row + 1].copy()
    return out


def with_particle_state(buf, m, xyz_cells, b=None, logjp=None, J=None, reflected=None):
    """A new buffer: `buf` with the material state of the given particles of model m replaced, their positions and everything else byte for
    byte.  xyz_cells (n, 3) float32: positions in cell units, x * 2^bits (exact), which name the particles - every one must be found exactly
    once.  b (n, 6) float32 in the order {00, 11, 22, 10, 20, 21} (solids), reflected (n,) bool: the sign bit of b00, logjp (n,) float32 (sand,
    NACC), J (n,) float32 (J-fluid); an argument left None leaves those floats alone."""
    M = parse(buf)["models"][m]
    nch, rec = M["nch"], rec_floats(M["nch"])
    row = nch - rec
    out = np.ascontiguousarray(buf, dtype=np.uint8).copy()
    B = bins(out, m)
    bin_, slot = particle_slots(out, m)
    have = B[bin_[:, None], slot[:, None] * rec + np.arange(3)[None, :]]
    where = {}
    for i, k in enumerate(np.ascontiguousarray(have).view(np.uint32).tolist()):
        where.setdefault(tuple(k), []).append(i)
    want = np.ascontiguousarray(xyz_cells, dtype=np.float32).reshape(-1, 3)
    idx = np.empty(want.shape[0], np.int64)
    for i, k in enumerate(want.view(np.uint32).tolist()):
        hit = where.get(tuple(k), [])
        assert len(hit) == 1, (i, want[i].tolist(), "found %d times" % len(hit))
        idx[i] = hit[0]
    assert np.unique(idx).size == idx.size, "a particle was requested twice"
    bi, sl = bin_[idx], slot[idx]
    n = idx.size
    if nch == 4:
        assert b is None and logjp is None and reflected is None, "the J-fluid carries J alone"
        if J is not None:
            B[bi, sl * rec + 3] = np.asarray(J, np.float32).reshape(n)
        return out
    assert J is None, "a solid carries b (and log Jp), not J"
    if b is not None:
        b = np.asarray(b, np.float32).reshape(n, 6)
        assert (b[:, 0] > 0).all(), "b00 carries the reflected mark in its sign: give it positive"
        neg = np.zeros(n, bool) if reflected is None else np.asarray(reflected, bool).reshape(n)
        B[bi, sl * rec + 3] = np.where(neg, -b[:, 0], b[:, 0])
        for c in range(1, 5):
            B[bi, sl * rec + 3 + c] = b[:, c]
        B[bi, K_BIN * rec + sl * row] = b[:, 5]
    else:
        assert reflected is None, "the reflected mark is the sign of b00: give b with it"
    if logjp is not None:
        assert row == 2, "this material carries no log Jp"
        B[bi, K_BIN * rec + sl * row + 1] = np.asarray(logjp, np.float32).reshape(n)
    return out


DIRS = np.array([(t // 9 - 1, (t // 3) % 3 - 1, t % 3 - 1) for t in range(27)], dtype=np.int64)      # dir_components: z fastest
K_ARENA_BIT = 30                      # the scatter arena of a record in the pair layout (kArenaBit)


def key_map(keys):
    """{block key: its number} of a key list (n, 3); a key held twice keeps its first number."""
    out = {}
    for i, k in enumerate(np.asarray(keys).reshape(-1, 3).tolist()):
        out.setdefault(tuple(k), i)
    return out


def source_extents(buf, m):
    """Bins each particle block of the PREVIOUS numbering holds for model m, read off binoff_src the way mpm_checkpoint_load reads them: the
    distance to the next larger offset (bins are handed out without gaps; empty blocks share an offset), at most max_ppc.  (prev_pbc,) int64."""
    h = parse(buf)
    n = h["prev_pbc"]
    bsrc = section(buf, h, ("binoff_src", m), np.int32)[:n].astype(np.int64)
    ends = np.unique(np.concatenate([bsrc, [h["models"][m]["bincount_src"]]]))
    at = np.searchsorted(ends, bsrc, side="right")
    nxt = np.where(at < ends.size, ends[np.minimum(at, ends.size - 1)], bsrc)      # (an offset at or behind the end of the bins: no extent)
    return np.minimum(nxt - bsrc, h["max_ppc"])


def list_records(buf, m):
    """Every record of model m's packed advection lists, field by field and WITHOUT judging any of it (particle_slots asserts; this does not):
    {"raw" uint32, "blk": the block of the current numbering whose list holds it (by size[]), "tag", "key": the sort key field, "slot": the
    slot in the source block, "arena": bit 30, "top": bit 31, "src": the block of the previous numbering at key(blk) + dir(tag) or -1 (also
    for a tag above 26), "ok": tag <= 26 and src is a particle block of the previous numbering and the slot lies within its bins, "bin",
    "lane": where the particle lives (meaningful where ok)}.  Records that size[] leaves no room for in the section are left out."""
    h = parse(buf)
    ppb = K_BIN * h["max_ppc"]
    pid_bits = ppb.bit_length() - 1
    size = np.clip(section(buf, h, ("size", m), np.int32)[:h["pbc"]].astype(np.int64), 0, None)
    raw = section(buf, h, ("lists", m), np.int32).view(np.uint32)
    blk = np.repeat(np.arange(h["pbc"]), size)[:raw.size]
    raw = raw[:blk.size]
    r = raw.astype(np.int64)
    tag = (r >> (pid_bits + K_KEY_BITS)) & 31
    slot = r & (ppb - 1)
    keys = section(buf, h, "cur_keys", np.int32).reshape(-1, 3).astype(np.int64)
    prev = key_map(section(buf, h, "prev_keys", np.int32).reshape(-1, 3))
    src_key = keys[blk] + DIRS[np.minimum(tag, 26)]
    src = np.array([prev.get(tuple(k), -1) for k in src_key.tolist()], dtype=np.int64).reshape(-1)
    src[tag > 26] = -1
    ext = source_extents(buf, m)
    inside = (src >= 0) & (src < h["prev_pbc"])
    ok = inside.copy()
    ok[inside] = (slot[inside] >> 6) < ext[src[inside]]
    binoff = section(buf, h, ("binoff_src", m), np.int32).astype(np.int64)
    bin_ = np.where(ok, binoff[np.where(ok, src, 0)] + (slot >> 6), 0)
    ok &= bin_ < h["models"][m]["bincount_src"]
    return {"raw": raw, "blk": blk, "tag": tag, "key": (r >> pid_bits) & ((1 << K_KEY_BITS) - 1), "slot": slot, "arena": (r >> K_ARENA_BIT) & 1,
            "top": r >> 31, "src": src, "ok": ok, "bin": bin_, "lane": slot & 63}


def record_positions(buf, m, recs=None):
    """Positions in cells (n, 3) float32 of the particles list_records names (NaN where a record is not ok)."""
    recs = list_records(buf, m) if recs is None else recs
    rec = rec_floats(parse(buf)["models"][m]["nch"])
    B = bins(buf, m)
    out = np.full((recs["raw"].size, 3), np.nan, np.float32)
    ok = recs["ok"]
    out[ok] = B[recs["bin"][ok][:, None], recs["lane"][ok][:, None] * rec + np.arange(3)[None, :]]
    return out

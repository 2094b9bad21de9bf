"""Reader / patcher of checkpoint format 7 (claymore_amd/csrc/mpm_checkpoint.inc): a plain numpy restatement of CkptHeader and
ckpt_layout.  The header is 448 bytes; every section starts at a multiple of 16 bytes (its length is rounded up to one).  Section order:
cur_keys (3 ints per exterior block), prev_keys (3 ints per block of the previous numbering), grid (256 floats per NEIGHBOUR block:
{mass, momentum x, y, z} x 64 cells), then per model size / row_of / binoff_src / binoff_dst / bins / lists / pairinfo.

mpm_checkpoint_load validates every index of a checkpoint and copies the grid section verbatim: with_grid() therefore puts any bit pattern
into any cell of any block of a context (tests/test_grid_update_kernels_gpu.py)."""
import numpy as np

HEADER_BYTES = 448
MAGIC = 0x3754504B434D504D            # "MPMCKPT7"
K_BIN = 64                            # particles per bin (kBin)
K_PAIR_CHUNKS = 16                    # pair counts per particle block in the pair layout (kPairChunks)
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

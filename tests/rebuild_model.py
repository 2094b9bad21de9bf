"""A plain numpy partition rebuild: what compact_blocks_kernel, the two register_blocks_kernel phases and prepare_blocks_kernel<SORT>
(claymore_amd/csrc/mpm_kernels.hpp) write, from a previous books state and, per particle, its old slot, its new position and its predicted sort
key - written out as a checkpoint in the layout of tests/ckpt_format.py, plus the look-up rows.  The orders the kernels leave to their atomics
(new block numbers, registration order, bin order, arrival order of the records) are drawn from a seed, so that a verifier
(tests/rebuild_books.py) is never fitted to one numbering.

A books state `prev` (make_prev) is a dict: bits, max_ppc, keys (ebc, 3), pbc, nbc, models = [dict(nch, layout, binoff (ebc + 1,), bincount,
bins (bincount, nch * 64) float32, where (n, 2) = {block, slot} of every particle)].

Test infrastructure only."""
import numpy as np

import ckpt_format as cf
from rebuild_books import CUBE, OCT, ROW, block_keys
from test_pair_layout_model import pair_chunk, pair_chunks, pair_slice, div_small

PAIR_LAYOUT = 2                       # kPairLayoutId


def tiers(pkeys, G, rng=None, order_of=None):
    """The full key list of a numbering whose particle blocks are `pkeys` (in that order): neighbours at {0, 1}^3, then exteriors at {-1, 0, 1}^3,
    each phase in a random order (rng) or in the order of the numbers `order_of` ({key: number}) gives."""
    keys = [tuple(int(v) for v in k) for k in pkeys]
    have = set(keys)
    counts = [len(keys)]
    for offs in (OCT, CUBE):
        new = set()
        for k in keys[:counts[0]]:
            for o in offs:
                c = (k[0] + int(o[0]), k[1] + int(o[1]), k[2] + int(o[2]))
                if all(0 <= v < G for v in c) and c not in have:
                    new.add(c)
        new = sorted(new)
        if order_of is not None:
            new.sort(key=lambda c: order_of[c])
        elif rng is not None:
            new = [new[i] for i in rng.permutation(len(new))]
        keys += new
        have.update(new)
        counts.append(len(keys))
    return np.array(keys, dtype=np.int64).reshape(-1, 3), counts[0], counts[1], counts[2]


def hand_out_bins(size, rng=None):
    """compact_blocks_kernel's bins: ceil(size / 64) per block with particles, handed out without gaps in the order of the atomics; 0 for an
    empty block.  Returns (binoff (n,), bincount)."""
    size = np.asarray(size, np.int64)
    nbins = (size + cf.K_BIN - 1) // cf.K_BIN
    full = np.flatnonzero(size > 0)
    order = full if rng is None else full[rng.permutation(full.size)]
    off = np.zeros(size.size, np.int64)
    off[order] = np.concatenate([[0], np.cumsum(nbins[order])[:-1]]) if order.size else []
    return off, int(nbins.sum())


def make_prev(bits, max_ppc, parts, rng):
    """A books state right after a G2P2G: parts = [(nch, layout, pos_cells (n, 3) float32)] per model are the particles as they lay BEFORE the
    step; every particle sits in some slot of its block's bins (slots handed out in a random order within the block)."""
    G = 1 << (bits - 2)
    allk = np.unique(np.concatenate([block_keys(p) for _, _, p in parts]), axis=0)
    pk = allk[rng.permutation(allk.shape[0])]
    keys, pbc, nbc, ebc = tiers(pk, G, rng)
    num = cf.key_map(keys)
    models = []
    for nch, layout, pos in parts:
        pos = np.ascontiguousarray(pos, np.float32)
        blk = np.array([num[tuple(k)] for k in block_keys(pos).tolist()], dtype=np.int64).reshape(-1)
        size = np.bincount(blk, minlength=pbc)
        assert size.max(initial=0) <= cf.K_BIN * max_ppc
        off, bincount = hand_out_bins(size, rng)
        slot = np.empty(pos.shape[0], np.int64)
        for b in np.flatnonzero(size):
            sel = np.flatnonzero(blk == b)
            slot[sel] = rng.permutation(sel.size)
        binoff = np.concatenate([off, rng.integers(0, 1000, ebc + 1 - pbc)])          # (behind the particle blocks: whatever was there)
        models.append(dict(nch=nch, layout=layout, binoff=binoff, bincount=bincount, where=np.stack([blk, slot], axis=1),
                           bins=np.zeros((bincount, nch * cf.K_BIN), np.float32)))
    return dict(bits=bits, max_ppc=max_ppc, keys=keys, pbc=pbc, nbc=nbc, ebc=ebc, models=models)


def sort_sliced(recs, key):
    """sort_chunk: per 512-record chunk the p-th record in key-major order goes to slice p mod S, position p / S; packed slice after slice."""
    out = np.empty_like(recs)
    for first in range(0, recs.size, 512):
        n = min(512, recs.size - first)
        order = np.argsort(key[first:first + n], kind="stable")
        S = (n + 63) // 64
        q, r = divmod(n, S)
        start = np.array([s * q + min(s, r) for s in range(S)])
        p = np.arange(n)
        out[first + start[p % S] + p // S] = recs[first + order]
    return out


def sort_pairs(recs, key):
    """sort_chunk_pairs: per chunk (pair_chunks) the records of a key two by two into pair slots in key-major order, the odd one into the single
    slots, the last 2 X singles two by two into the mismatched slots; slot p -> slice p mod S, lane p / S; a slice's A records, then its B records;
    the arena bit: lane parity, for a single the arena its key's pair slot of the same slice does not use.  Returns (records, pair counts)."""
    out = np.empty_like(recs)
    pinfo = np.full(cf.K_PAIR_CHUNKS, -7, np.int32)                                  # (entries past the last chunk: never read)
    for c, (first, n) in enumerate(pair_chunks(recs.size)):
        k = key[first:first + n]
        order = np.argsort(k, kind="stable")
        ks, cnt = np.unique(k, return_counts=True)
        pf, n1 = int((cnt // 2).sum()), int((cnt % 2).sum())
        pc = pair_chunk(n, pf)
        S, n1s = pc["S"], pc["L"] - pc["px"]
        pp = sp = at = 0
        for nk in cnt.tolist():
            for r in range(nk):
                rec = int(recs[first + order[at]]) & ~(1 << cf.K_ARENA_BIT)
                at += 1
                paired = r < (nk & ~1)
                if paired:
                    slot, member = pp + (r >> 1), r & 1
                else:
                    slot, member = (pc["px"] + sp, 0) if sp < n1s else (pf + ((sp - n1s) >> 1), (sp - n1s) & 1)
                ln = div_small(slot, S)
                d = slot - ln * S
                pos, ca, cb = pair_slice(pc, d)
                arena = ln & 1
                if not paired:
                    i0 = (d - pp % S) % S
                    if i0 < (nk >> 1):
                        arena = 1 ^ (div_small(pp + i0, S) & 1)
                out[first + pos + (ca if member else 0) + ln] = rec | (arena << cf.K_ARENA_BIT)
            pp += nk >> 1
            sp += nk & 1
        pinfo[c] = pf
    return out, pinfo


def rebuild(prev, moves, seed, order="random"):
    """prev: make_prev's state; moves: per model (new_pos (n, 3) float32, sort_key (n,) in [0, 216)), aligned with prev's particles.  Returns
    (checkpoint buffer, rows per model).  order "identity": every free order follows the previous numbering (what a still step must arrive at
    when nobody moved)."""
    rng = np.random.default_rng(seed) if order == "random" else None
    bits, max_ppc = prev["bits"], prev["max_ppc"]
    G = 1 << (bits - 2)
    ppb = cf.K_BIN * max_ppc
    pid_bits = ppb.bit_length() - 1
    pnum = cf.key_map(prev["keys"])
    nm = len(prev["models"])
    # G2P2G's share: the moved particle is written into the slot it was worked off from, and counted at the block it now lies in
    dest = []
    out_count = np.zeros((nm, prev["ebc"]), np.int64)
    for m, (M, (npos, skey)) in enumerate(zip(prev["models"], moves)):
        npos = np.ascontiguousarray(npos, np.float32)
        rec = cf.rec_floats(M["nch"])
        blk, slot = M["where"][:, 0], M["where"][:, 1]
        M["bins"][(M["binoff"][blk] + (slot >> 6))[:, None], ((slot & 63) * rec)[:, None] + np.arange(3)[None, :]] = npos
        nk = block_keys(npos)
        assert (np.abs(nk - prev["keys"][blk]) <= 1).all(), "a particle moves further than to a neighbouring block"
        d = np.array([pnum[tuple(k)] for k in nk.tolist()], dtype=np.int64).reshape(-1)
        dest.append(d)
        out_count[m] = np.bincount(d, minlength=prev["ebc"])
    assert out_count.max(initial=0) <= ppb, "the model does not drop"
    # compaction: blocks that received particles, numbered in the order of the atomics
    alive = np.flatnonzero(out_count.sum(axis=0) > 0)
    if rng is not None:
        alive = alive[rng.permutation(alive.size)]
    keys, pbc, nbc, ebc = tiers(prev["keys"][alive], G, rng, order_of=None if rng is not None else pnum)
    num = cf.key_map(keys)
    H = dict(magic=cf.MAGIC, domain_bits=bits, max_ppc=max_ppc, nmodels=nm, rollid=int(seed) & 1, pbc=pbc, nbc=nbc, ebc=ebc, prev_count=prev["ebc"],
             prev_pbc=prev["pbc"], grid_velocity=0, models=[])
    body, rows_per_model = [], []
    for m, (M, (npos, skey)) in enumerate(zip(prev["models"], moves)):
        size = out_count[m][alive]
        binoff, bincount = hand_out_bins(size, rng) if rng is not None else (None, 0)
        if rng is None:                                                        # bins in the order of the previous offsets
            nb = (size + cf.K_BIN - 1) // cf.K_BIN
            o = np.flatnonzero(size > 0)
            o = o[np.argsort(M["binoff"][alive][o], kind="stable")]
            binoff = np.zeros(size.size, np.int64)
            binoff[o] = np.concatenate([[0], np.cumsum(nb[o])[:-1]]) if o.size else []
            bincount = int(nb.sum())
        # the records: {tag of the source block seen from the new block, sort key, slot in the source block}
        blk, slot = M["where"][:, 0], M["where"][:, 1]
        dkey = prev["keys"][blk] - prev["keys"][dest[m]]
        tag = (dkey[:, 0] + 1) * 9 + (dkey[:, 1] + 1) * 3 + dkey[:, 2] + 1
        rec = (tag << (pid_bits + cf.K_KEY_BITS)) | (np.asarray(skey, np.int64) << pid_bits) | slot
        lists, pinfo = [], np.zeros((pbc, cf.K_PAIR_CHUNKS), np.int32)
        for b in range(pbc):
            sel = np.flatnonzero(dest[m] == alive[b])
            if rng is not None:
                sel = sel[rng.permutation(sel.size)]                           # arrival order
            key = np.asarray(skey, np.int64)[sel]
            if M["layout"]:
                srt, pinfo[b] = sort_pairs(rec[sel], key)
            else:
                srt = sort_sliced(rec[sel], key)
            lists.append(srt)
        lists = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        # the look-up rows
        rows = -np.ones((pbc, ROW), np.int64)
        for b in range(pbc):
            for l in range(27):
                s = pnum.get(tuple((keys[b] + cf.DIRS[l]).tolist()), -1)
                rows[b, l] = M["binoff"][s] if s >= 0 else -1
                rows[b, 27 + l] = num.get(tuple((keys[b] - cf.DIRS[l]).tolist()), -1)
            for l in range(8):
                rows[b, 54 + l] = num.get(tuple((keys[b] + OCT[l]).tolist()), -1)
        rows_per_model.append(rows.astype(np.int32))
        pad = lambda a, n: np.concatenate([np.asarray(a, np.int64), np.zeros(n - len(a), np.int64)]).astype(np.int32)
        H["models"].append(dict(material=0, nch=M["nch"], list_in=0, layout=M["layout"], n=int(npos.shape[0]), bincount=bincount,
                                bincount_src=M["bincount"], bucketed=int(size.sum())))
        body.append([pad(size, ebc + 1), pad(alive, ebc + 1), M["binoff"].astype(np.int32), pad(binoff, ebc + 1), M["bins"].reshape(-1),
                     lists.astype(np.uint32).view(np.int32), pinfo.reshape(-1) if M["layout"] else np.zeros(0, np.int32)])
    return write_ckpt(H, keys, prev["keys"], body), rows_per_model


def write_ckpt(H, cur_keys, prev_keys, body):
    """The byte image ckpt_format.parse reads: header, cur_keys, prev_keys, a zero grid, then per model the seven sections of `body`."""
    lay, end = cf.layout(H)
    buf = np.zeros(end, np.uint8)
    i32, u64 = buf[:cf.HEADER_BYTES].view(np.int32), buf[:cf.HEADER_BYTES].view(np.uint64)
    u64[0] = H["magic"]
    i32[2:10] = [H["domain_bits"], H["max_ppc"], H["nmodels"], H["rollid"], H["pbc"], H["nbc"], H["ebc"], H["prev_count"]]
    u64[5] = end
    i32[14], i32[15] = H["prev_pbc"], H["grid_velocity"]
    for m, M in enumerate(H["models"]):
        at = 64 + cf.MODEL_BYTES * m
        buf[at:at + 16].view(np.int32)[:] = [M["material"], M["nch"], M["list_in"], M["layout"]]
        buf[at + 16:at + 48].view(np.int64)[:] = [M["n"], M["bincount"], M["bincount_src"], M["bucketed"]]

    def put(name, a):
        a = np.ascontiguousarray(a)
        at, n = lay[name]
        assert a.nbytes == n, (name, a.nbytes, n)
        buf[at:at + n] = a.view(np.uint8).reshape(-1)
    put("cur_keys", np.asarray(cur_keys, np.int32))
    put("prev_keys", np.asarray(prev_keys, np.int32))
    for m, secs in enumerate(body):
        for name, a in zip(cf.SECTIONS, secs):
            put((name, m), a)
    return buf

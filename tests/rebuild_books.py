"""check_books: everything the partition rebuild writes (claymore_amd/csrc/mpm_kernels.hpp: compact_blocks_kernel, register_blocks_kernel,
prepare_blocks_kernel), verified field by field from a checkpoint (tests/ckpt_format.py) and the dumped look-up rows (mpm_dump_block_rows).
Needs no GPU; every check is integer-exact.  A finding is a tuple (what, where ..., got, want); an empty list means consistent.

Test infrastructure only."""
from collections import Counter

import numpy as np

import ckpt_format as cf
from test_pair_layout_model import pair_chunks

ROW = 64                               # kInfoRow
OCT = np.array([((i >> 2) & 1, (i >> 1) & 1, i & 1) for i in range(8)], dtype=np.int64)
CUBE = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], dtype=np.int64)


def block_keys(pos_cells):
    """g2p2g_model.block_keys: (lround(x / dx) - 2) / 4 per axis (positions are positive)"""
    return (np.floor(np.asarray(pos_cells, np.float64) + 0.5).astype(np.int64) - 2) // 4


def _around(keys, offs, G):
    """the in-domain keys at `offs` around `keys`, as a set of tuples"""
    if len(keys) == 0:
        return set()
    k = (np.asarray(sorted(keys), dtype=np.int64)[:, None, :] + offs[None, :, :]).reshape(-1, 3)
    k = k[((k >= 0) & (k < G)).all(axis=1)]
    return set(map(tuple, k.tolist()))


def pair_layout_findings(size, recs, pinfo, pid_bits, seen=None, where=()):
    """The pair layout of one block's list (mpm_kernels.hpp), chunk by chunk - the checks of
    test_parity_gpu.py::test_the_sort_writes_the_pair_layout_it_promises: with n records and Pf full pairs (pinfo) the S = ceil(n / 128) slices hold
    L = min(Pf + n1, 64 S) slots, dense; every pair slot's two members carry the SAME sort key and the keys of the pair slots ascend; the mismatched
    slots are exactly X = max(0, Pf + n1 - 64 S) and hold two different keys; no key has two singles; both members of a pair slot carry the same
    arena bit - its lane parity -, and a single never uses the arena its own key's pair slot of the same slice uses.  pinfo entries past the
    last chunk are not read.  seen: a dict of counters to add to."""
    out = []
    recs = np.asarray(recs).astype(np.int64) & 0xffffffff
    chunks = pair_chunks(size)
    if seen is not None:
        seen["multi_chunk"] += len(chunks) > 1
        seen["merged"] += bool(chunks) and chunks[-1][1] > 512
    for c, (first, n) in enumerate(chunks):
        at = where + (("chunk", c),)
        if first != 512 * c:
            out.append(("chunk start",) + at + (first, 512 * c))
            continue
        r = recs[first:first + n]
        key, arena = (r >> pid_bits) & 255, (r >> 30) & 1
        pf = int(pinfo[c])
        n1 = n - 2 * pf
        if not (0 <= pf and n1 >= 0):
            out.append(("pairinfo out of range",) + at + (pf, n))
            continue
        S = (n + 127) // 128
        X = max(0, pf + n1 - 64 * S)
        px, L = pf + X, pf + n1 - X
        if not (L <= 64 * S and L + px == n):
            out.append(("pairinfo: slots do not fit the slices",) + at + (pf, n))
            continue
        pos = 0
        slot_key = {}
        for d in range(S):
            ca, cb = L // S + (d < L % S), px // S + (d < px % S)
            ka, kb = key[pos:pos + ca], key[pos + ca:pos + ca + cb]
            aa, ab = arena[pos:pos + ca], arena[pos + ca:pos + ca + cb]
            for ln in range(ca):
                slot_key[ln * S + d] = (int(ka[ln]), int(kb[ln]) if ln < cb else None, int(aa[ln]), ln, int(ab[ln]) if ln < cb else None)
            pos += ca + cb
            if seen is not None:
                seen["full_slices"] += ca == 64
        if not (pos == n and sorted(slot_key) == list(range(L))):
            out.append(("dense slices",) + at + (pos, n))
            continue
        pair_keys = [slot_key[p][0] for p in range(pf)]
        if not all(slot_key[p][0] == slot_key[p][1] for p in range(pf)):                       # a pair slot: two records of one key
            out.append(("pair slot of two keys",) + at + (pf,))
        if pair_keys != sorted(pair_keys):                                                     # key-major order
            out.append(("pair slots not in key order",) + at + (pf,))
        if not all(slot_key[p][2] == slot_key[p][4] == (slot_key[p][3] & 1) for p in range(pf)):   # its arena, on both members: the lane parity
            out.append(("arena of a pair slot is not its lane parity",) + at + (pf,))
        if not all(slot_key[p][1] is not None and slot_key[p][0] != slot_key[p][1] for p in range(pf, px)):   # a mismatched slot: two singles of different keys
            out.append(("mismatched slots",) + at + (X,))
        if not all(slot_key[p][1] is None for p in range(px, L)):                              # a single slot: A only
            out.append(("single slot with a second member",) + at + (L - px,))
        singles = [slot_key[p][0] for p in range(pf, L)] + [slot_key[p][1] for p in range(pf, px)]
        if not (len(singles) == len(set(singles)) == n1):                                      # one single per key at most
            out.append(("two singles of one key",) + at + (len(singles), len(set(singles)), n1))
        cnt = Counter(pair_keys)
        if not all(2 * cnt.get(k, 0) + (k in set(singles)) == int((key == k).sum()) for k in set(key.tolist())):
            out.append(("pairs and singles do not add up to the key counts",) + at + (pf,))
        # the arena of a single (and of a mismatched slot, which carries its A's rule): not the one its key's pair slot of the same slice uses
        by_slice = {}
        for p in range(pf):
            by_slice.setdefault((p % S, slot_key[p][0]), []).append(slot_key[p][2])
        for p in range(pf, L):
            used = by_slice.get((p % S, slot_key[p][0]), [])
            if len(used) == 1 and slot_key[p][2] == used[0]:
                out.append(("arena rule of a single",) + at + (p,))
        if seen is not None:
            seen["chunks"] += 1
            seen["pairs"] += pf
            seen["mismatched"] += X
            seen["singles"] += n1
    return out


def sliced_layout_findings(size, recs, pid_bits, where=()):
    """The sliced layout (prepare_blocks_kernel's sort_chunk) as a checkpoint packs it - per 512-record chunk of n records the S = ceil(n / 64)
    slices one behind the other, slice s with n / S + (s < n % S) records: in key-major order the p-th record sits in slice p mod S at position
    p / S, so the keys read in that order must ascend (the order within a key is free)."""
    out = []
    recs = np.asarray(recs).astype(np.int64) & 0xffffffff
    for c, first in enumerate(range(0, size, 512)):
        n = min(512, size - first)
        key = (recs[first:first + n] >> pid_bits) & 255
        S = (n + 63) // 64
        q, r = divmod(n, S)
        start = np.array([s * q + min(s, r) for s in range(S)])
        p = np.arange(n)
        seq = key[start[p % S] + p // S]
        if (np.diff(seq) < 0).any():
            out.append(("sliced layout: keys not in key-major order", ) + where + (("chunk", c), int(np.argmax(np.diff(seq) < 0))))
    return out


def tier_findings(cur, pbc, nbc, ebc, have, G):
    """cur (>= ebc, 3) block keys, have: the set of block keys the particle positions give.  The first pbc keys are `have` as a set, the next
    nbc - pbc exactly the in-domain keys at {0, 1}^3 of particle blocks not yet present, the rest up to ebc exactly those at {-1, 0, 1}^3;
    no key twice; the order within a tier is free."""
    F = []
    cur = np.asarray(cur).astype(np.int64)
    want2 = _around(have, OCT, G) - have
    want3 = _around(have, CUBE, G) - have - want2
    for name, a, b, want in (("particle tier", 0, pbc, set(have)), ("neighbour tier", pbc, nbc, want2), ("exterior tier", nbc, ebc, want3)):
        got = list(map(tuple, cur[a:b].tolist()))
        if set(got) != want or len(set(got)) != len(got):
            F.append((name, sorted(set(got) - want)[:4], sorted(want - set(got))[:4], len(got) - len(set(got))))
    return F


def census_findings(cur, pbc, size, pos_keys, listed_in, where=()):
    """size[b] is the number of particles whose position lies in block b (pos_keys (n, 3): the block key of every particle's position), and
    every particle lies in the block whose list names it (listed_in (n,): that block's number)."""
    F = []
    cur = np.asarray(cur).astype(np.int64)
    num = cf.key_map(cur[:pbc])
    size = np.asarray(size).astype(np.int64)[:pbc]
    lives = np.array([num.get(tuple(k), -1) for k in np.asarray(pos_keys).tolist()], dtype=np.int64).reshape(-1)
    by_pos = np.bincount(lives[lives >= 0], minlength=pbc)[:pbc] if pbc else np.zeros(0, np.int64)
    bad = np.flatnonzero(by_pos != size)
    if bad.size:
        F.append(("size",) + where + (bad[:4].tolist(), size[bad[:4]].tolist(), by_pos[bad[:4]].tolist()))
    here = np.flatnonzero(lives != np.asarray(listed_in))
    if here.size:
        F.append(("a record's particle does not lie in the record's block",) + where + (here[:4].tolist(),))
    return F


def check_books(ckpt, rows_per_model, bits, max_ppc, counts=None, loaded=False):
    """ckpt: a checkpoint saved after a rebuild; rows_per_model: per model the (particle blocks, 64) int rows of mpm_dump_block_rows; counts
    (optional): the per-model particle counts of mpm_get_counts.  The caller asserts mpm_check_table == 0 (the dense tables are not in a
    checkpoint; here "the table" of a numbering is its key list).

    loaded: the checkpoint was saved right after mpm_checkpoint_load, before any rebuild.  The loader lays the lists out anew - unpack_lists_kernel
    puts block b's list into row b and writes row_of[b] = b for every model that holds a particle -, so row_of is held to the identity there
    instead of to the block's number in the previous numbering (what the compaction of a rebuild writes).  Everything else is held as it is.

    Lanes 0 .. 26 of a row are held to -1 where the previous numbering has no block at key + dir(l) (a key outside the domain included) and
    to binoff_src of that block where it was a PARTICLE block of the previous numbering.  Where it was a neighbour or exterior block the lane
    is not constrained: prepare_blocks_kernel loads binoff_src[that number], whatever lies there, and no record can name such a block."""
    F = []
    ckpt = np.ascontiguousarray(ckpt, dtype=np.uint8)
    h = cf.parse(ckpt)
    if (h["domain_bits"], h["max_ppc"]) != (bits, max_ppc):
        F.append(("configuration", (h["domain_bits"], h["max_ppc"]), (bits, max_ppc)))
    G = 1 << (bits - 2)
    ppb = cf.K_BIN * max_ppc
    pid_bits = ppb.bit_length() - 1
    pbc, nbc, ebc, prev_pbc = h["pbc"], h["nbc"], h["ebc"], h["prev_pbc"]
    cur = cf.section(ckpt, h, "cur_keys", np.int32).reshape(-1, 3).astype(np.int64)
    prev = cf.section(ckpt, h, "prev_keys", np.int32).reshape(-1, 3).astype(np.int64)
    cur_t, prev_t = cf.key_map(cur), cf.key_map(prev)
    if len(cur_t) != ebc:
        F.append(("a key appears twice in the current numbering", ebc - len(cur_t)))
    if len(prev_t) != h["prev_count"]:
        F.append(("a key appears twice in the previous numbering", h["prev_count"] - len(prev_t)))
    if not (((cur >= 0) & (cur < G)).all() and ((prev >= 0) & (prev < G)).all()):
        F.append(("a block key outside the domain",))
    nmodels = h["nmodels"]
    if len(rows_per_model) != nmodels:
        F.append(("rows for every model", len(rows_per_model), nmodels))

    # ---- records and the particles they name
    R, P = [], []
    for m in range(nmodels):
        r = cf.list_records(ckpt, m)
        R.append(r)
        P.append(cf.record_positions(ckpt, m, r))
    # ---- tiers
    have = set()
    for m in range(nmodels):
        ok = R[m]["ok"]
        have.update(map(tuple, block_keys(P[m][ok]).tolist()))
    F += tier_findings(cur, pbc, nbc, ebc, have, G)

    for m in range(nmodels):
        M, r, pos = h["models"][m], R[m], P[m]
        size = cf.section(ckpt, h, ("size", m), np.int32)[:pbc].astype(np.int64)
        row_of = cf.section(ckpt, h, ("row_of", m), np.int32)[:pbc].astype(np.int64)
        bdst = cf.section(ckpt, h, ("binoff_dst", m), np.int32)[:pbc].astype(np.int64)
        bsrc = cf.section(ckpt, h, ("binoff_src", m), np.int32).astype(np.int64)
        ok, blk = r["ok"], r["blk"]
        # ---- per block: size, row_of, bins
        if int(size.sum()) != M["bucketed"] or r["raw"].size != M["bucketed"]:
            F.append(("sizes do not add up to bucketed", m, int(size.sum()), M["bucketed"]))
        if counts is not None and int(size.sum()) != int(counts[m]):
            F.append(("sizes do not add up to the particle count", m, int(size.sum()), int(counts[m])))
        pk = block_keys(pos[ok])
        F += census_findings(cur, pbc, size, pk, blk[ok], where=(m,))
        want_row = np.array([prev_t.get(tuple(k), -1) for k in cur[:pbc].tolist()], dtype=np.int64).reshape(-1)
        if loaded:
            want_row = np.arange(pbc) if M["bucketed"] else np.full(pbc, -1)
        bad = np.flatnonzero((want_row >= 0) & (row_of != want_row))
        if bad.size:
            F.append(("row_of", m, bad[:4].tolist(), row_of[bad[:4]].tolist(), want_row[bad[:4]].tolist()))
        bad = np.flatnonzero((size == 0) & (bdst != 0))
        if bad.size:
            F.append(("binoff_dst of an empty block", m, bad[:4].tolist(), bdst[bad[:4]].tolist()))
        full = np.flatnonzero(size > 0)
        o = full[np.argsort(bdst[full], kind="stable")]
        lo, hi = bdst[o], bdst[o] + (size[o] + cf.K_BIN - 1) // cf.K_BIN
        edges_ok = o.size == 0 and M["bincount"] == 0 or (o.size > 0 and lo[0] == 0 and (lo[1:] == hi[:-1]).all() and hi[-1] == M["bincount"])
        if not edges_ok:
            F.append(("bin ranges do not tile [0, bincount)", m, M["bincount"], lo[:6].tolist(), hi[:6].tolist()))
        # ---- records
        tag_bad = np.flatnonzero((r["tag"] > 26) | (r["top"] != 0))
        if tag_bad.size:
            F.append(("record tag above 26 or bits above the arena bit", m, tag_bad[:4].tolist()))
        src_bad = np.flatnonzero((r["tag"] <= 26) & ((r["src"] < 0) | (r["src"] >= prev_pbc)))
        if src_bad.size:
            F.append(("record names no particle block of the previous numbering", m, src_bad[:4].tolist()))
        ext_bad = np.flatnonzero((r["tag"] <= 26) & (r["src"] >= 0) & (r["src"] < prev_pbc) & ~ok)
        if ext_bad.size:
            F.append(("record slot outside its source block's bins", m, ext_bad[:4].tolist()))
        named = r["src"][ok] * ppb + r["slot"][ok]
        if np.unique(named).size != named.size:
            F.append(("a slot is named twice", m, named.size - np.unique(named).size))
        if not M["layout"] and r["arena"].any():
            F.append(("arena bit in the sliced layout", m, np.flatnonzero(r["arena"])[:4].tolist()))
        # ---- layout
        starts = np.concatenate([[0], np.cumsum(size)])
        raw = r["raw"]
        pinfo = cf.section(ckpt, h, ("pairinfo", m), np.int32).reshape(-1, cf.K_PAIR_CHUNKS) if M["layout"] else None
        for b in range(pbc):
            lst = raw[starts[b]:starts[b + 1]]
            if lst.size != size[b]:
                continue
            if M["layout"]:
                F += pair_layout_findings(int(size[b]), lst, pinfo[b], pid_bits, where=(m, ("block", b)))
            else:
                F += sliced_layout_findings(int(size[b]), lst, pid_bits, where=(m, ("block", b)))
        # ---- rows
        if m >= len(rows_per_model):
            continue
        rows = np.asarray(rows_per_model[m]).astype(np.int64)
        if rows.shape != (pbc, ROW):
            F.append(("rows shape", m, rows.shape, (pbc, ROW)))
            continue
        for b in range(pbc):
            k = cur[b]
            for l in range(27):
                s = prev_t.get(tuple((k + cf.DIRS[l]).tolist()), -1)
                if s < 0:
                    want = -1
                elif s < prev_pbc:
                    want = int(bsrc[s])
                else:
                    continue
                if rows[b, l] != want:
                    F.append(("row: source lane", m, b, l, int(rows[b, l]), want))
            for l in range(27, 54):
                want = cur_t.get(tuple((k - cf.DIRS[l - 27]).tolist()), -1)
                if rows[b, l] != want:
                    F.append(("row: destination lane", m, b, l, int(rows[b, l]), want))
            for l in range(54, 62):
                want = cur_t.get(tuple((k + OCT[l - 54]).tolist()), -1)
                if rows[b, l] != want:
                    F.append(("row: grid block lane", m, b, l, int(rows[b, l]), want))
            for l in (62, 63):
                if rows[b, l] != -1:
                    F.append(("row: unused lane", m, b, l, int(rows[b, l]), -1))
    return F


def record_keys(ckpt, m):
    """Per particle block of the current numbering (by block key): the sort-key sequence of model m's list, as a dict {key tuple: int array}."""
    h = cf.parse(ckpt)
    r = cf.list_records(ckpt, m)
    cur = cf.section(ckpt, h, "cur_keys", np.int32).reshape(-1, 3)
    return {tuple(cur[b].tolist()): r["key"][r["blk"] == b] for b in range(h["pbc"])}

"""A plain model of the MGSP halo tagging, collect and reduce (claymore_amd/csrc/mpm_halo.inc, oracle/mpm_oracle.c "MGSP halo path"):
numpy and Python integers only, no engine.  Everything is keyed by BLOCK KEY (a tuple of three ints), never by block number: the HIP
engine and the oracle number their blocks differently, so results are compared as sets / dicts of keys.

The rule that is modelled (and pinned by tests/test_halo_model_cpu.py and tests/test_halo_kernels_gpu.py):
  * a block is shared with peer p iff it is a NEIGHBOUR block (index < nbc in the key list) of this rank and its key is in p's key list;
    blocks that this rank holds only as exterior blocks, and keys it does not hold or that lie outside the domain, are never marked;
  * a particle block k is a halo block iff any of k + {0,1}^3 is one of this rank's blocks with a non-zero mark;
  * a padded key list has pad_rows rows per rank, row 0 = {count, status word, 0}; min(count, pad_rows - 1) keys of it are looked at, the
    own rank's rows are not looked at; max_peer_rows = max over ALL ranks of count + 1.

A real rank's key list holds every key once, and so does every list the generators below make: the kernels' send lists are appended to
once per listed key, so a duplicate in a peer list would show up twice in the send list.  The model works on sets and therefore would not
see it; the tests only feed duplicate-free lists and assert that the kernels' send lists are duplicate-free too."""
import itertools

import numpy as np

CATEGORIES = ("particle", "neighbor", "exterior", "foreign", "outside")
CUBE = tuple(itertools.product((0, 1), repeat=3))
# the status bits of row 0 (kPeerErr* in mpm_halo.inc), in the order mgsp_peer_status tests them, with the mpm_status each maps to
PEER_ERR_BLOCKS, PEER_ERR_LIST, PEER_ERR_BINS, PEER_ERR_NONFINITE, PEER_ERR_BOOKS = 1, 2, 4, 8, 16
MPM_ERR_DEVICE, MPM_ERR_CAPACITY, MPM_ERR_NONFINITE, MPM_ERR_INTERNAL = 2, 3, 4, 6


def peer_status_code(word):
    """The mpm_status mgsp_peer_status returns for a non-zero peer status word."""
    if word & PEER_ERR_NONFINITE:
        return MPM_ERR_NONFINITE
    if word & (PEER_ERR_BLOCKS | PEER_ERR_LIST | PEER_ERR_BINS):
        return MPM_ERR_CAPACITY
    if word & PEER_ERR_BOOKS:
        return MPM_ERR_INTERNAL
    return MPM_ERR_DEVICE


def as_keys(a):
    return [tuple(int(x) for x in k) for k in np.asarray(a, dtype=np.int64).reshape(-1, 3)]


class Tagging:
    """Result of one tagging round."""

    def __init__(self, overlap, send, halo_blocks, interior_blocks):
        self.overlap = overlap                      # key -> 32-bit pattern (Python int, 0 .. 2^32 - 1); absent = 0
        self.send = send                            # 32 sets of keys
        self.send_counts = [len(s) for s in send]
        self.halo_blocks = halo_blocks              # set of particle-block keys
        self.interior_blocks = interior_blocks
        self.max_peer_rows = None                   # padded path only
        self.status = None                          # padded path only: (peer, word, mpm_status) of the first non-zero peer word, or None


class HaloModel:
    def __init__(self, keys, pbc, G):
        """keys: this rank's key list (nbc rows; the first pbc are its particle blocks), G: blocks per axis (2^(bits - 2))."""
        self.keys = as_keys(keys)
        self.nbc, self.pbc, self.G = len(self.keys), int(pbc), int(G)
        assert 0 <= self.pbc <= self.nbc and len(set(self.keys)) == self.nbc
        self.own = set(self.keys)
        self.particle = self.keys[:self.pbc]
        self.neighbor_only = self.keys[self.pbc:]

    # ---- tagging ------------------------------------------------------------------------------------------------
    def tag(self, peer_lists):
        """peer_lists: {peer: (n, 3) keys}.  A key counts once per peer however often it is listed (see the module docstring)."""
        overlap, send = {}, [set() for _ in range(32)]
        for p, lst in peer_lists.items():
            assert 0 <= p < 32
            for k in set(as_keys(lst)):
                if k in self.own:
                    overlap[k] = overlap.get(k, 0) | (1 << p)
                    send[p].add(k)
        halo = {k for k in self.particle if any(overlap.get((k[0] + i, k[1] + j, k[2] + l), 0) for i, j, l in CUBE)}
        return Tagging(overlap, send, halo, set(self.particle) - halo)

    def tag_padded(self, rows, rank):
        """rows: (world, pad_rows, 3) ints, the all-gathered padded lists."""
        rows = np.asarray(rows, dtype=np.int64)
        world, pad_rows, _ = rows.shape
        lists = {}
        for p in range(world):
            if p != rank:
                n = max(0, min(int(rows[p, 0, 0]), pad_rows - 1))
                lists[p] = rows[p, 1:1 + n]
        t = self.tag(lists)
        t.max_peer_rows = max(int(rows[p, 0, 0]) for p in range(world)) + 1
        for p in range(world):
            w = int(rows[p, 0, 1])
            if p != rank and w != 0:
                t.status = (p, w, peer_status_code(w))
                break
        return t

    # ---- collect / reduce ---------------------------------------------------------------------------------------
    @staticmethod
    def collect(grid, send_p):
        """grid: {key: 256 floats}; the blocks of the keys sent to one peer."""
        return {k: grid[k] for k in send_p}

    def reduce(self, grid, keys, blocks):
        """Add blocks[i] into the block keys[i] for every key that is a neighbour block of this rank; all others are ignored.  A key may
        come several times.  Returns {key: (sum64, seq32, count, abs64)} for the blocks that received something: the float64 sum old + all
        addends, the float32 sum taken in arrival order, the number of addends, and |old| + sum |addend| in float64 (each 256 long)."""
        out = {}
        blocks = np.asarray(blocks, dtype=np.float32).reshape(-1, 256)
        for k, blk in zip(as_keys(keys), blocks):
            if k not in self.own:
                continue
            if k not in out:
                old = np.asarray(grid[k], dtype=np.float32).reshape(256)
                out[k] = [old.astype(np.float64), old.copy(), 0, np.abs(old.astype(np.float64))]
            e = out[k]
            e[0] = e[0] + blk.astype(np.float64)
            e[1] = (e[1] + blk).astype(np.float32)
            e[2] += 1
            e[3] = e[3] + np.abs(blk.astype(np.float64))
        return {k: tuple(v) for k, v in out.items()}

    # ---- key categories -----------------------------------------------------------------------------------------
    def in_domain(self, k):
        return all(0 <= c < self.G for c in k)

    def exterior_only(self):
        """Keys this rank holds as exterior blocks only: a particle key minus one along one axis, inside the domain and not in the list."""
        out = []
        seen = set()
        for k in self.particle:
            for ax in range(3):
                e = tuple(c - (1 if a == ax else 0) for a, c in enumerate(k))
                if self.in_domain(e) and e not in self.own and e not in seen:
                    seen.add(e)
                    out.append(e)
        return out

    def registered(self):
        """Every key this rank may have in its table: particle keys + {-1, 0, 1}^3 (exterior), which contains the neighbour blocks."""
        reg = set(self.own)
        for k in self.particle:
            for d in itertools.product((-1, 0, 1), repeat=3):
                reg.add((k[0] + d[0], k[1] + d[1], k[2] + d[2]))
        return reg

    def foreign(self):
        """In-domain keys this rank does not have at all, in row-major order."""
        reg = self.registered()
        return [k for k in itertools.product(range(self.G), repeat=3) if k not in reg]

    def outside(self):
        """Out-of-domain keys: every in-domain key of the list with one component replaced by -1, G, G + 5 or 2^30."""
        out = []
        for n, k in enumerate(self.keys):
            bad = (-1, self.G, self.G + 5, 1 << 30)[n % 4]
            ax = (n // 4) % 3
            out.append(tuple(bad if a == ax else c for a, c in enumerate(k)))
        return list(dict.fromkeys(out))

    def pools(self):
        return {"particle": list(self.particle), "neighbor": list(self.neighbor_only), "exterior": self.exterior_only(),
                "foreign": self.foreign(), "outside": self.outside()}


# ---- generators of synthetic peer lists (seeded; no duplicates inside a list) ----------------------------------------
def mixed_list(rng, pools, counts):
    """A shuffled list with counts[c] keys of every category c (a dict, or one int for all five), drawn without replacement."""
    if isinstance(counts, int):
        counts = {c: counts for c in CATEGORIES}
    out = []
    for c in CATEGORIES:
        n, pool = counts.get(c, 0), pools[c]
        assert n <= len(pool), (c, n, len(pool))
        out += [pool[i] for i in rng.permutation(len(pool))[:n]]
    assert len(set(out)) == len(out)
    return np.array([out[i] for i in rng.permutation(len(out))], dtype=np.int32).reshape(-1, 3)


def list_of_length(rng, pools, n):
    """A shuffled mix of all five categories with exactly n keys: the categories are served round-robin until n keys are drawn."""
    order = {c: list(rng.permutation(len(pools[c]))) for c in CATEGORIES}
    out = []
    while len(out) < n:
        progressed = False
        for c in CATEGORIES:
            if len(out) < n and order[c]:
                out.append(pools[c][order[c].pop()])
                progressed = True
        assert progressed, "the pools hold fewer than n keys"
    assert len(set(out)) == len(out)
    return np.array([out[i] for i in rng.permutation(len(out))], dtype=np.int32).reshape(-1, 3)


def list_from_keys(rng, keys, G, n_own, n_other):
    """For callers that know a key list but not which of its blocks hold particles (the phantom ranks of the fused test): n_own keys of
    the list, and n_other keys that are not in it - shifted copies (key - 1 along an axis), in-domain strangers and out-of-domain keys."""
    keys = as_keys(keys)
    own = set(keys)
    out = [keys[i] for i in rng.permutation(len(keys))[:n_own]]
    seen = set(out)
    tries = 0
    while len(out) < n_own + n_other and len(out) < len(keys) + 50:
        tries += 1
        kind = tries % 3
        if kind == 0 and keys:
            k = keys[int(rng.integers(len(keys)))]
            ax = int(rng.integers(3))
            c = tuple(v - (1 if a == ax else 0) for a, v in enumerate(k))
        elif kind == 1:
            c = tuple(int(v) for v in rng.integers(0, G, 3))
        else:
            c = [int(v) for v in rng.integers(0, G, 3)]
            c[int(rng.integers(3))] = (-1, G, G + 5, 1 << 30)[int(rng.integers(4))]
            c = tuple(c)
        if c not in own and c not in seen:
            seen.add(c)
            out.append(c)
    return np.array([out[i] for i in rng.permutation(len(out))], dtype=np.int32).reshape(-1, 3)


def padded_rows(world, pad_rows, lists, status=None):
    """The all-gathered array (world, pad_rows, 3): row 0 = {true count, status word, 0}, then the first pad_rows - 1 keys."""
    rows = np.zeros((world, pad_rows, 3), dtype=np.int32)
    for p, lst in lists.items():
        lst = np.asarray(lst, dtype=np.int32).reshape(-1, 3)
        n = min(len(lst), pad_rows - 1)
        rows[p, 0, 0] = len(lst)
        rows[p, 1:1 + n] = lst[:n]
    for p, w in (status or {}).items():
        rows[p, 0, 1] = w
    return rows


def grid_dict(keys, blocks):
    return {k: np.asarray(b, dtype=np.float32).reshape(256) for k, b in zip(as_keys(keys), np.asarray(blocks).reshape(-1, 256))}


def check_scene_conditions(model):
    """The conditions that keep the tests from passing with nothing to check: enough blocks of every kind."""
    pools = model.pools()
    assert model.pbc >= 20 and len(pools["neighbor"]) >= 20 and len(pools["exterior"]) >= 20, (model.pbc, len(pools["neighbor"]), len(pools["exterior"]))
    assert len(pools["foreign"]) >= 20 and len(pools["outside"]) >= 20
    return pools


def check_main_lists(model, lists):
    """Every list of the main tagging test holds at least 5 keys of each category and no duplicate."""
    part, ext, reg = set(model.particle), set(model.exterior_only()), model.registered()
    for p, lst in lists.items():
        ks = as_keys(lst)
        assert len(set(ks)) == len(ks)
        n = {c: 0 for c in CATEGORIES}
        for k in ks:
            if k in model.own:
                n["particle" if k in part else "neighbor"] += 1
            elif not model.in_domain(k):
                n["outside"] += 1
            elif k in ext:
                n["exterior"] += 1
            elif k not in reg:
                n["foreign"] += 1
        assert min(n.values()) >= 5, (p, n)


def check_main_result(model, t):
    """The main tagging test's result exercises something: a halo set that is neither empty nor everything, a block shared with 3 or
    more peers, a block carrying bit 31."""
    assert 0 < len(t.halo_blocks) < model.pbc, (len(t.halo_blocks), model.pbc)
    assert any(bin(v).count("1") >= 3 for v in t.overlap.values())
    assert any(v >> 31 for v in t.overlap.values())


MAIN_PEERS = (0, 1, 7, 8, 15, 16, 30, 31)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)


def main_lists(model, seed=1):
    """The lists of the main tagging test: peers 0, 1, 7, 8, 15, 16, 30, 31, each a different mix of 5 .. 12 keys per category.  The own
    keys are drawn from the lower half of the scene along x only (block x below the median of the particle blocks), so that part of the
    particle blocks stays interior."""
    rng = np.random.default_rng(seed)
    pools = model.pools()
    cut = sorted(k[0] for k in model.particle)[model.pbc // 2]
    for c in ("particle", "neighbor"):
        pools[c] = [k for k in pools[c] if k[0] < cut]
    return {p: mixed_list(rng, pools, {c: min(int(rng.integers(5, 13)), len(pools[c])) for c in CATEGORIES}) for p in MAIN_PEERS}


# ---- the scenes of the halo tests (bits 6, about 10^4 particles) ----------------------------------------------------
BITS = 6
G_BLOCKS = 1 << (BITS - 2)


def halo_scene(name):
    """"spheres": two touching elastic spheres flying at each other; "wall": one sphere dropped at the x = 0 face of the domain, inside the
    wall zone, so that block keys with a 0 component appear."""
    from claymore_amd import scenes
    if name == "spheres":
        return scenes.two_spheres(bits=BITS, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
    assert name == "wall"
    sc = scenes.sphere_drop(bits=BITS, radius_cells=6.0, center=(0.14, 0.5, 0.5))
    sc["models"][0]["params"].update({"youngs_modulus": 2e4, "poisson_ratio": 0.4, "rho": 1e3})
    return sc

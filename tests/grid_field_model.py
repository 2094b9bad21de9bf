"""NumPy model of the Eulerian readouts (claymore_amd/csrc/mpm_grid_field.hpp): point samples, dense volumes and
box totals of the grid of the last P2G, built from (keys, blocks) as mpm_dump_grid or ckpt_format.grid give them - the nbc neighbour blocks
and nothing else, so an exterior block (numbers nbc .. ebc - 1 of the table) holds nothing here by construction, like a block that is absent.

  sample   p_d = x_d * N in float32 (node_index's multiply), base = lround_pos(p) - 1 (ties away from zero), then everything in float64: the
           weights of bspline_weight_cells(p - base), W = w0 w1 w2, ref = sum W value and S = sum W |value| over the 27 nodes
  volume   bit-exact: stride 1 moves the words; stride 2, 4 add in float32, acc = +0 then x slowest, z fastest
  totals   float64 sums of the float32 node values over a clipped node box, with the sums of |terms| a tolerance is stated in
"""
import numpy as np


def lround_pos(p):
    """lround for p >= 0 the way the device forms it (mpm_device_math.hpp): round to nearest even, plus one where p - that is exactly +0.5.
    p: float32 array; returns int64."""
    p = np.asarray(p, dtype=np.float32)
    r = np.rint(p)                                   # ties to even, like v_rndne_f32
    return r.astype(np.int64) + ((p - r) == np.float32(0.5))


def weights(fd):
    """bspline_weight_cells in float64: fd (...,) -> (..., 3)."""
    fd = np.asarray(fd, dtype=np.float64)
    return np.stack([0.5 * (1.5 - fd) ** 2, 0.75 - (fd - 1.0) ** 2, 0.5 * (fd - 0.5) ** 2], axis=-1)


class GridField:
    PAD = 2     # nodes of zeros around the domain: a stencil reaches node -1 below and N + 1 above

    def __init__(self, keys, blocks, bits):
        self.bits, self.N = int(bits), 1 << int(bits)
        keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
        blocks = np.ascontiguousarray(blocks)
        assert blocks.dtype in (np.float32, np.uint32) and blocks.shape == (keys.shape[0], 4, 64), (blocks.dtype, blocks.shape)
        assert ((keys >= 0) & (keys < self.N // 4)).all() and np.unique(keys, axis=0).shape[0] == keys.shape[0]
        self.keys = keys
        self.dense = np.zeros((4, self.N, self.N, self.N), dtype=np.uint32)      # bit patterns: node (i, j, k) of channel c at [c, i, j, k]
        cube = blocks.view(np.uint32).reshape(-1, 4, 4, 4, 4)                     # cell ((x & 3) << 4) | ((y & 3) << 2) | (z & 3)
        for (kx, ky, kz), b in zip(keys.tolist(), cube):
            self.dense[:, 4 * kx:4 * kx + 4, 4 * ky:4 * ky + 4, 4 * kz:4 * kz + 4] = b
        self._padded = None

    def values(self):
        return self.dense.view(np.float32)

    # ---- sample ---------------------------------------------------------------------------------------------------------------------
    def stencil(self, xyz):
        """(valid (n,), base (n, 3) int64, fd (n, 3) float64) of n world-space points; base and fd are 0 where the point is not valid."""
        x = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        with np.errstate(over="ignore", invalid="ignore"):
            p = x * np.float32(self.N)                                           # one float32 multiply
            valid = (np.isfinite(p) & (p >= 0) & (p < np.float32(self.N))).all(axis=1)
        p = np.where(valid[:, None], p, np.float32(0))
        base = lround_pos(p) - 1
        fd = p.astype(np.float64) - base                                         # (exact in float32 too: |p - base| < 2)
        return valid, base, fd

    def sample(self, xyz):
        """ref (n, 4) float64 = sum W {m, px, py, pz}, S (n, 4) float64 = sum W |.| over the same stencil; zeros for points that are not valid."""
        if self._padded is None:
            P = self.PAD
            self._padded = np.zeros((4,) + (self.N + 2 * P,) * 3, dtype=np.float64)
            self._padded[:, P:-P, P:-P, P:-P] = self.values()
        valid, base, fd = self.stencil(xyz)
        w = weights(fd)                                                          # (n, axis, 3)
        n = base.shape[0]
        ref, S = np.zeros((n, 4)), np.zeros((n, 4))
        ib = base + self.PAD
        for i in range(3):
            for j in range(3):
                for k in range(3):
                    W = w[:, 0, i] * w[:, 1, j] * w[:, 2, k]
                    v = self._padded[:, ib[:, 0] + i, ib[:, 1] + j, ib[:, 2] + k].T   # (n, 4)
                    ref += W[:, None] * v
                    S += W[:, None] * np.abs(v)
        ref[~valid] = 0.0
        S[~valid] = 0.0
        return ref, S

    # ---- volume ---------------------------------------------------------------------------------------------------------------------
    def node_box(self, origin, dims):
        """uint32 (4, dims) of the nodes origin + [0, dims): zero outside the domain."""
        o, d = [int(v) for v in origin], [int(v) for v in dims]
        out = np.zeros((4,) + tuple(d), dtype=np.uint32)
        lo = [max(o[a], 0) for a in range(3)]
        hi = [min(o[a] + d[a], self.N) for a in range(3)]
        if all(hi[a] > lo[a] for a in range(3)):
            out[:, lo[0] - o[0]:hi[0] - o[0], lo[1] - o[1]:hi[1] - o[1], lo[2] - o[2]:hi[2] - o[2]] = self.dense[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        return out

    def volume(self, origin, dims, stride):
        """float32 (4, dims): output cell (X, Y, Z) over the stride^3 nodes origin + stride (X, Y, Z) + [0, stride)^3.  Bit-exact."""
        s = int(stride)
        assert s in (1, 2, 4) and min(dims) >= 1
        box = self.node_box(origin, [s * int(v) for v in dims])
        if s == 1:
            return box.view(np.float32)
        f = box.view(np.float32)
        acc = np.zeros((4,) + tuple(int(v) for v in dims), dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            for i in range(s):
                for j in range(s):
                    for k in range(s):
                        acc = acc + f[:, i::s, j::s, k::s]                       # float32 adds, one at a time, in the stated order
        return acc

    # ---- totals ---------------------------------------------------------------------------------------------------------------------
    def box_totals(self, lo, hi):
        """(out (5,), mag (5,)) float64 over the nodes of [lo, hi) clipped to the domain: out = {sum m, sum p (3), sum_{m > 0} |p|^2 / (2 m)},
        mag = the sums of the terms' absolute values."""
        lo = [max(int(v), 0) for v in lo]
        hi = [min(int(v), self.N) for v in hi]
        out, mag = np.zeros(5), np.zeros(5)
        if any(hi[a] <= lo[a] for a in range(3)):
            return out, mag
        v = self.values()[:, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].astype(np.float64)
        for c in range(4):
            out[c], mag[c] = v[c].sum(), np.abs(v[c]).sum()
        m = v[0]
        pos = m > 0
        e = (v[1][pos] ** 2 + v[2][pos] ** 2 + v[3][pos] ** 2) / (2.0 * m[pos])
        out[4] = mag[4] = e.sum()
        return out, mag


def hashed_blocks(nblocks, seed, lo_exp=-20, hi_exp=20):
    """(nblocks, 4, 64) float32 from a counter hash: magnitudes 2^u, u uniform in [lo_exp, hi_exp); masses positive, momenta of mixed sign."""
    idx = np.arange(nblocks * 256, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & (2 ** 64 - 1))
    h = idx
    for _ in range(2):                                                           # splitmix64's finaliser, twice
        h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = h ^ (h >> np.uint64(31))
    u = (h >> np.uint64(11)).astype(np.float64) / float(1 << 53)                 # [0, 1)
    sign = np.where((h & np.uint64(1)).astype(bool), -1.0, 1.0)
    val = np.exp2(lo_exp + (hi_exp - lo_exp) * u).reshape(nblocks, 4, 64)
    sign = sign.reshape(nblocks, 4, 64)
    sign[:, 0] = 1.0
    return (val * sign).astype(np.float32)

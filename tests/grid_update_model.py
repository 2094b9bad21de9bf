"""The grid update of one cell, restated with numpy float32 / float64 arrays, the scene and the seeded grid generator of
tests/test_grid_update_kernels_gpu.py.  Judged against the reference's golden cells in tests/test_grid_update_model_cpu.py, not against
the kernels.

The statements (grid_update_kernel, grid_cell(CollisionArgs), carry_grid_kernel in claymore_amd/csrc/mpm_kernels.hpp; orc_grid_cell in
oracle/mpm_oracle.c) for a cell with mass m > 0 - IEEE '>': +0, -0, negative and NaN masses skip the cell, which then keeps all four
channels bit for bit; FLT_MIN, denormals and +inf do not:

    inv = fl32(1 / m)                       the correctly rounded quotient (the build keeps the IEEE division sequence)
    v0  = wall_x ? +0 : fl32(p0 * inv)      one rounding of an exact product: float32(float64(p0) * float64(inv)), bit-exact
    v2  = wall_z ? +0 : fl32(p2 * inv)
    gdt = fl32(gravity * dt)
    v1  = fl32((wall_y ? +0 : fl32(p1 * inv)) + gdt)       `strict`: every operation rounded
       or fl32(p1 * inv + gdt)                             `fused`: one rounding (a contracted multiply-add), off the y walls only
    a block's axis is a wall where key < boundary or key >= G - boundary.

The returned maximum.  The plain kernels may contract v0 v0 + v1 v1 + v2 v2 in several ways, so the model computes Q = v0^2 + v1^2 + v2^2
in float64 FROM THE VELOCITIES THE KERNEL WROTE and bounds the kernel's float32 q: q is made of at most three product roundings and two
sum roundings of non-negative terms; every intermediate is at most Q (up to its own rounding), so each rounding is at most 1/2 ulp32(Q):
|q - Q| <= 2.5 ulp32(Q).  fmaxf, the shuffles and atomicMax on the bit patterns of non-negative floats are exact and monotone, so the
maximum obeys the same bound: |ret - max Q| <= 2.5 ulp32(max Q) (PLAIN_MAX_ULPS).  A NaN q counts as +inf.
The collision path is compiled with contraction off: its q is the float32 statement order of grid_cell(CollisionArgs),
((v0 v0 + v1 v1) + v2 v2) + v0 v0 + v1 v1 + v2 v2 (the reference's doubled |v|^2), bit for bit (collision_q32).

NaNs.  IEEE 754 leaves sign and payload of a NaN that an operation produces (or propagates from two NaN operands) to the implementation;
x86 and gfx950 differ there.  canon() maps every NaN to one pattern; it is applied to COMPUTED velocities only - masses and skipped cells
are compared on their raw bits, payloads included."""
import itertools

import numpy as np

PLAIN_MAX_ULPS = 2.5
F32 = np.float32
QNAN = np.uint32(0x7FC00000)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def canon(a):
    """uint32 bit patterns with every NaN mapped to one quiet NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), QNAN, a.view(np.uint32))


def ulp32(x):
    """Spacing of float32 at the magnitude of the float64 x (2^-149 in the denormal range)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return np.maximum(2.0 ** (e - 23), 2.0 ** -149)


def wall_flags(keys, G, boundary):
    """(nbc, 3) bool: the block's x / y / z axis lies in the slip-wall zone."""
    keys = np.asarray(keys, dtype=np.int64)
    return (keys < boundary) | (keys >= G - boundary)


def wall_class(keys, G, boundary):
    """(nbc, 3) in {0 low wall, 1 interior, 2 high wall}."""
    keys = np.asarray(keys, dtype=np.int64)
    return np.where(keys < boundary, 0, np.where(keys >= G - boundary, 2, 1))


def mul32(a, b):
    """fl32(a * b): the float64 product of two float32 is exact (48 bits), the cast is the one rounding."""
    with np.errstate(all="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def fma32(a, b, c):
    """fl32(a * b + c) with one rounding.  The float64 sum of the exact product and c is rounded to odd (TwoSum gives its error) before the
    cast: 53 >= 24 + 2 bits, so the cast then rounds as if from the exact value."""
    with np.errstate(all="ignore"):
        p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0)
        sb = s.view(np.int64).copy()
        odd = (sb & 1) == 1
        grow = (err > 0) == (s > 0)                        # the exact value lies beyond s in magnitude
        sb = np.where(fix & ~odd, np.where(grow, sb + 1, sb - 1), sb)
        return sb.view(np.float64).astype(np.float32)


def cell_update(m, p0, p1, p2, wx, wy, wz, gdt):
    """One cell each (arrays of equal shape; wx / wy / wz bool, gdt a float32 scalar) -> live, (v0, v1 strict, v1 fused, v2)."""
    m, p0, p1, p2 = (np.asarray(a, dtype=np.float32) for a in (m, p0, p1, p2))
    zero = np.zeros_like(m)
    with np.errstate(all="ignore"):
        live = m > 0
        inv = (F32(1.0) / np.where(live, m, F32(1.0))).astype(np.float32)
        v0 = np.where(wx, zero, mul32(p0, inv))
        v2 = np.where(wz, zero, mul32(p2, inv))
        g = np.full_like(m, gdt)
        v1s = (np.where(wy, zero, mul32(p1, inv)) + g).astype(np.float32)
        v1f = np.where(wy, v1s, fma32(p1, inv, g))
    return live, (v0, v1s, v1f, v2)


def gdt32(gravity, dt):
    return F32(F32(gravity) * F32(dt))


def plain(keys, G, boundary, gravity, dt, grid):
    """-> live (nbc, 64), strict (nbc, 4, 64), fused (nbc, 4, 64): the grid after the update with either v1 candidate; skipped cells and the
    mass channel are the input's bits."""
    grid = np.ascontiguousarray(grid, dtype=np.float32)
    w = wall_flags(keys, G, boundary)
    wx, wy, wz = (np.broadcast_to(w[:, d, None], grid[:, 0].shape) for d in range(3))
    live, (v0, v1s, v1f, v2) = cell_update(grid[:, 0], grid[:, 1], grid[:, 2], grid[:, 3], wx, wy, wz, gdt32(gravity, dt))
    out = []
    for v1 in (v1s, v1f):
        o = grid.view(np.uint32).copy()
        for ch, v in ((1, v0), (2, v1), (3, v2)):
            o[:, ch] = np.where(live, v.view(np.uint32), o[:, ch])
        out.append(o.view(np.float32))
    return live, out[0], out[1]


def max_q64(out, live, doubled=False):
    """max over live cells of Q = v0^2 + v1^2 + v2^2 (2 Q: the collision kernels') in float64 from the velocities in `out`; NaN -> +inf; 0 when
    no cell is live."""
    with np.errstate(all="ignore"):
        v = np.ascontiguousarray(out, dtype=np.float32).astype(np.float64)
        q = v[:, 1] ** 2 + v[:, 2] ** 2 + v[:, 3] ** 2
    q = np.where(np.isnan(q), np.inf, q)[live]
    return float(q.max() * (2.0 if doubled else 1.0)) if q.size else 0.0


def plain_q32(v0, v1, v2):
    """The reference's statement order in float32, every operation rounded: vel_sqr = 0; += v0 v0; += v1 v1; += v2 v2; NaN -> +inf."""
    with np.errstate(all="ignore"):
        q = ((v0 * v0).astype(np.float32) + (v1 * v1).astype(np.float32)).astype(np.float32)
        q = (q + (v2 * v2).astype(np.float32)).astype(np.float32)
    return np.where(np.isnan(q), F32(np.inf), q).astype(np.float32)


def collision_q32(v0, v1, v2):
    """grid_cell(CollisionArgs)'s q: vel.dot(vel), then the three += of the plain overload; NaN -> +inf."""
    with np.errstate(all="ignore"):
        a, b, c = (v0 * v0).astype(np.float32), (v1 * v1).astype(np.float32), (v2 * v2).astype(np.float32)
        q = ((a + b).astype(np.float32) + c).astype(np.float32)
        for t in (a, b, c):
            q = (q + t).astype(np.float32)
    return np.where(np.isnan(q), F32(np.inf), q).astype(np.float32)


def node_coords(keys):
    """(nbc, 3, 64) node coordinates: node = 4 key + {cell >> 4, (cell >> 2) & 3, cell & 3}."""
    cell = np.arange(64)
    local = np.stack([cell >> 4, (cell >> 2) & 3, cell & 3])
    return 4 * np.asarray(keys, dtype=np.int64)[:, :, None] + local[None]


def collision(keys, G, boundary, gravity, dt, grid, sticky_sdf=None):
    """The collision kernels' update for an object at rest at the origin (identity pose: a node's position in the level set is node * dx,
    exactly, and the trilinear interpolation returns the node's own sample).  sticky_sdf None: an object that touches no node (the `strict`
    plain velocities).  sticky_sdf (N, N, N): a STICKY object; a node inside query_sdf's box [4 boundary, 4 (G - boundary))^3 whose sample
    is <= 0 gets velocity +0, every other node the strict plain result.  -> live, grid after the update, the returned (doubled) maximum."""
    live, out, _ = plain(keys, G, boundary, gravity, dt, grid)
    out = out.copy()
    if sticky_sdf is not None:
        nd = node_coords(keys)
        inside = np.all((nd >= 4 * boundary) & (nd < 4 * (G - boundary)), axis=1)
        hit = live & inside & (np.asarray(sticky_sdf)[nd[:, 0].clip(0, 4 * G - 1), nd[:, 1].clip(0, 4 * G - 1), nd[:, 2].clip(0, 4 * G - 1)] <= 0)
        for ch in (1, 2, 3):
            out[:, ch] = np.where(hit, F32(0.0), out[:, ch])
    q = collision_q32(out[:, 1], out[:, 2], out[:, 3])[live]
    return live, out, (F32(q.max()) if q.size else F32(0.0))


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
BITS = 6
G_BLOCKS = 1 << (BITS - 2)
# cell-unit coordinates (tests/face_scenes.py: FACE_OFFSETS[-1] = 3.5 from either face, the face patches' mid[0]): stencil base block 0 / 7 / 14
AXIS_CELLS = (3.5, (1 << BITS) / 2 - 1.75, (1 << BITS) - 3.5)
AXIS_BLOCKS = (0, 7, 14)
EXTRA_CELLS = (26.25, 26.25, 30.25)       # one more particle, block (6, 6, 7): 222 neighbour blocks, no multiple of 4 or 16


def scene_cells():
    """(28, 3) particle positions in cell units: one per product of {block 0, 7, 14} per axis and the extra one.  The 3 x 3 x 3 stencils of
    two particles share no node."""
    pts = [list(p) for p in itertools.product(AXIS_CELLS, repeat=3)] + [list(EXTRA_CELLS)]
    return np.array(pts, dtype=np.float32)


def scene_particle_blocks():
    return sorted(set(itertools.product(AXIS_BLOCKS, repeat=3)) | {(6, 6, 7)})


def scene_keys():
    """The neighbour blocks of the scene as a sorted (nbc, 3) array: the 2 x 2 x 2 blocks from every particle block upwards."""
    keys = {(b[0] + i, b[1] + j, b[2] + k) for b in scene_particle_blocks() for i, j, k in itertools.product((0, 1), repeat=3)}
    return np.array(sorted(keys), dtype=np.int32)


# ---- the generator ------------------------------------------------------------------------------------------------------------------
MASS_CLASSES = ("ordinary", "flt_min", "denormal", "+0", "-0", "negative", "nan", "+inf")
LIVE_MASS = (0, 1, 2, 7)
MOM_CLASSES = ("ordinary", "+0", "-0", "denormal", "overflow", "+inf", "-inf", "nan")
FINITE_MASS = (0, 1, 2, 3, 4, 5, 0, 0)        # the finite tier's eight mass slots as classes of MASS_CLASSES
FINITE_MOM = (0, 1, 2, 3, 0, 0, 0, 0)         # ... and the momentum slots of its live cells
TIERS = ("full", "finite", "small")
SIGN = np.uint32(0x80000000)


def _f(exp, man, sign=0):
    return (np.asarray(sign, np.uint32) << np.uint32(31)) | (np.asarray(exp, np.uint32) << np.uint32(23)) | np.asarray(man, np.uint32)


def generate(nblocks, seed, tier):
    """-> bit patterns (nblocks, 4, 64) uint32, mass classes (nblocks, 64), momentum classes (nblocks, 3, 64) as indices into MASS_CLASSES /
    MOM_CLASSES.  Every cell of every block is filled.  Stratified per block: a random permutation of the 64 cells gives each of the eight
    mass slots eight cells, and within a mass slot each component's eight momentum slots once (rotated at random per block, mass slot and
    component) - so every block, hence every wall class, holds every mass class and, in live cells of every live mass class, every momentum
    class of every component.

    full:   all classes.  `overflow`: |p| ~ 2^127 over a mass <= 2^-7.
    finite: no live cell produces a NaN, an infinity or an overflow: masses ordinary / FLT_MIN / denormal in [2^-127, 2^-126) (whose
            reciprocal is finite) and the skipped classes +0 / -0 / negative; live momenta ordinary (|v| < 16) / +-0 / denormal.  SKIPPED cells
            keep the full tier's momentum classes - NaN and inf included - which must not reach the maximum.
    small:  finite with |v| < 2^-12 in every live cell."""
    assert tier in TIERS
    rng = np.random.default_rng(seed)
    shape = (nblocks, 64)
    rank = np.argsort(rng.random(shape), axis=1).astype(np.int64)          # a permutation per block: cell -> rank
    mslot, pslot = rank % 8, rank // 8
    off = rng.integers(0, 8, size=(nblocks, 3, 8))
    mom_slot = (pslot[:, None, :] + np.take_along_axis(off, np.broadcast_to(mslot[:, None, :], (nblocks, 3, 64)), axis=2)) % 8
    mcls = mslot if tier == "full" else np.asarray(FINITE_MASS)[mslot]
    live = np.isin(mcls, LIVE_MASS)
    pcls = mom_slot if tier == "full" else np.where(live[:, None, :], np.asarray(FINITE_MOM)[mom_slot], mom_slot)

    def u(lo, hi, shp=shape):
        return rng.integers(lo, hi, size=shp, dtype=np.int64).astype(np.uint32)
    mexp = u(100, 121)                                                       # ordinary masses: 2^-27 .. 2^-6
    mass = np.select([mcls == 0, mcls == 1, mcls == 2, mcls == 3, mcls == 4, mcls == 5, mcls == 6, mcls == 7],
                     [_f(mexp, u(0, 1 << 23)), np.uint32(0x00800000), (u(1, 1 << 23) if tier == "full" else u(1 << 22, 1 << 23)), np.uint32(0),
                      SIGN, _f(mexp, u(0, 1 << 23), 1), _f(255, u(1, 1 << 23), u(0, 2)), np.uint32(0x7F800000)]).astype(np.uint32)
    tiny = (mcls == 1) | (mcls == 2)
    out = np.empty((nblocks, 4, 64), np.uint32)
    out[:, 0] = mass
    for d in range(3):
        c = pcls[:, d]
        sign = u(0, 2)
        if tier == "small":
            ordinary = np.where(tiny, _f(0, u(0, 0x200), sign), _f((mexp.astype(np.int64) + rng.integers(-20, -12, size=shape)).astype(np.uint32), u(0, 1 << 23), sign))
            denormal = np.where(tiny, _f(0, u(1, 0x200), sign), _f(0, u(1, 1 << 23), sign))
        else:
            # live cells of the finite tier: |p| < 2^(e_m + 4) over an ordinary mass, exponent field 0..2 over a tiny one (|v| < 2^-124 2^127)
            ordinary = np.where(tiny & live, _f(u(0, 3), u(0, 1 << 23), sign), _f((mexp.astype(np.int64) + rng.integers(-4, 4, size=shape)).astype(np.uint32), u(0, 1 << 23), sign))
            denormal = _f(0, u(1, 1 << 23), sign)
        out[:, 1 + d] = np.select([c == 0, c == 1, c == 2, c == 3, c == 4, c == 5, c == 6, c == 7],
                                  [ordinary, np.uint32(0), SIGN, denormal, _f(254, u(0, 1 << 23), sign), np.uint32(0x7F800000), np.uint32(0xFF800000),
                                   _f(255, u(1, 1 << 23), sign)]).astype(np.uint32)
    return out, mcls, pcls


def coverage_gaps(keys, G, boundary, mcls, pcls, tier):
    """What the generator's output lacks, as a list of strings (empty: the condition holds): every mass class of the tier in each of the 27
    wall classes, and every momentum class of the tier, per component, in a LIVE cell of each of the 27 wall classes."""
    wc = wall_class(keys, G, boundary)
    want_m = set(range(8)) if tier == "full" else set(FINITE_MASS)
    want_p = set(range(8)) if tier == "full" else set(FINITE_MOM)
    live = np.isin(mcls, LIVE_MASS)
    gaps = []
    for cls in itertools.product(range(3), repeat=3):
        blk = np.all(wc == np.array(cls), axis=1)
        if not blk.any():
            gaps.append(f"wall class {cls}: no block")
            continue
        miss = want_m - set(np.unique(mcls[blk]).tolist())
        if miss:
            gaps.append(f"wall class {cls}: mass classes {sorted(miss)} missing")
        for d in range(3):
            miss = want_p - set(np.unique(pcls[blk][:, d][live[blk]]).tolist())
            if miss:
                gaps.append(f"wall class {cls}: momentum classes {sorted(miss)} of component {d} missing in live cells")
    return gaps

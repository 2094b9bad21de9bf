"""The Eulerian readouts on the GPU - mpm_sample_grid, mpm_grid_volume, mpm_grid_box_totals (claymore_amd/csrc/mpm_grid_field.hpp) - against
tests/grid_field_model.py, on INJECTED grids (the port of tests/test_grid_update_kernels_gpu.py: a checkpoint whose grid section is replaced
through ckpt_format.with_grid is loaded verbatim) and on the grid a run leaves behind.  Every output element of every call is compared.

The scene (bits 7, N = 128, wall zone 2 blocks): two boxes of 8^3 nodes x 8 particles, 4096 each.  A sits against the LOWER x face (nodes
1 .. 8: block 0 is registered, so points with x < dx / 2 - stencil base -1 - sample real values), B against the UPPER z wall zone (nodes
117 .. 124: block 31, the last, is registered).  Around both lie exterior-only blocks (numbers nbc .. ebc - 1: in the table, without grid
rows), and the rest of the domain is empty."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import ckpt_format as cf
import grid_field_model as gfm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError, build_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = 7
N = 1 << BITS
DT = 1e-4
EPS = 2.0 ** -24
A_LO, B_LO = (1, 50, 40), (114, 60, 117)


def scene():
    prm = {"volume": scenes._vol(BITS), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    box = lambda lo: scenes.lattice_box(BITS, lo, tuple(v + 8 for v in lo))     # noqa: E731
    return {"name": "grid_field", "bits": BITS, "dt": DT, "config": {"max_ppc": 128},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": box(A_LO), "v0": (0.4, -0.2, 0.3), "params": dict(prm)},
                       {"material": _ffi.FIXED_COROTATED, "xyz": box(B_LO), "v0": (-0.3, 0.2, -0.4), "params": dict(prm)}]}


def special_pattern(base):
    """The hashed grid with NaN (quiet, signalling, negative, with payloads), -0, +-inf and denormal words in a few cells of every channel."""
    pat = base.view(np.uint32).copy()
    words = np.array([0x7FC00000, 0x7FC01234, 0x7F800001, 0xFFC00000, 0xFFABCDEF, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)
    nb = pat.shape[0]
    for i, w in enumerate(words):
        pat[(7 * i + 1) % nb, i % 4, (13 * i + 5) % 64] = w
        pat[nb - 1 - (5 * i) % nb, (i + 1) % 4, (29 * i) % 64] = w
    return pat


class World:
    """One context of the scene after three substeps, its checkpoint, and the model of whichever injected grid it currently holds."""

    def __init__(self):
        self.eng = build_engine(scene())
        self.eng.initial_setup()
        self.eng.run_fixed(3, DT)
        self.ckpt = self.eng.save_checkpoint().copy()
        h = cf.parse(self.ckpt)
        self.nbc, self.ebc = h["nbc"], h["ebc"]
        allkeys = cf.cur_keys(self.ckpt)
        self.keys, self.exterior = allkeys[:self.nbc].copy(), allkeys[self.nbc:self.ebc].copy()
        hashed = gfm.hashed_blocks(self.nbc, 17)
        self.patterns = {"hashed": hashed.view(np.uint32), "special": special_pattern(hashed)}
        self.models = {}
        self.current = None

    def use(self, name):
        if self.current != name:
            self.eng.load_checkpoint(cf.with_grid(self.ckpt, self.patterns[name]))
            self.current = name
        if name not in self.models:
            self.models[name] = gfm.GridField(self.keys, self.patterns[name], BITS)
        return self.models[name]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()


def raw_sample(eng, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    out = np.full((pts.shape[0], 4), np.float32(-7.0))
    rc = eng.api.sample_grid(eng.ctx, pts.ctypes.data_as(C.c_void_p), pts.shape[0], out.ctypes.data_as(C.c_void_p))
    assert rc == _ffi.MPM_OK, eng.api.last_error(eng.ctx)
    return out


def check_sample(world, pts, label, expect_nonzero=True):
    m = world.use("hashed")
    pts = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    got = raw_sample(world.eng, pts).astype(np.float64)
    ref, S = m.sample(pts)
    err, bound = np.abs(got - ref), 64 * EPS * S
    worst = float((err / np.where(S > 0, EPS * S, 1.0))[S > 0].max()) if (S > 0).any() else 0.0
    print(f"{label}: {pts.shape[0]} points, {int((S[:, 0] > 0).sum())} with mass, worst error {worst:.2f} eps S (bound 64)")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (label, int((err > bound).sum()), pts[np.argwhere(err > bound)[0, 0]].tolist())
    if expect_nonzero:
        assert (S[:, 0] > 0).any(), label
    return got, ref, S


# ---- the scene ------------------------------------------------------------------------------------------------------------------------------
def test_scene_has_registered_exterior_and_empty_blocks(world):
    m = world.use("hashed")
    assert 0 < world.nbc < world.ebc and world.exterior.shape[0] == world.ebc - world.nbc
    assert (world.keys[:, 0] == 0).any() and (world.keys[:, 2] == N // 4 - 1).any()          # registered blocks at the lower x and the upper z face
    assert world.ebc < (N // 4) ** 3 // 8                                                       # most of the domain is empty
    keys, blocks = world.eng.dump_grid()
    assert np.array_equal(keys, world.keys) and np.array_equal(blocks.view(np.uint32), world.patterns["hashed"])
    mag = np.abs(m.values())
    assert mag[mag > 0].min() >= 2.0 ** -20 and mag.max() < 2.0 ** 20 and (m.values()[1:] < 0).any() and (m.values()[1:] > 0).any() and (m.values()[0] >= 0).all()


# ---- sample ---------------------------------------------------------------------------------------------------------------------------------
def test_sample_every_node_of_a_block(world):
    """At a node the stencil is {1/8, 3/4, 1/8} per axis around it."""
    m = world.use("hashed")
    for k in (world.keys[0], world.keys[world.nbc // 2], world.keys[(world.keys[:, 0] == 0).argmax()], world.keys[(world.keys[:, 2] == N // 4 - 1).argmax()]):
        nodes = 4 * k[None, :] + np.stack(np.meshgrid(range(4), range(4), range(4), indexing="ij"), axis=-1).reshape(-1, 3)
        got, ref, _ = check_sample(world, nodes / N, f"nodes of block {k.tolist()}")
        w = np.array([0.125, 0.75, 0.125])
        v = m.values().astype(np.float64)
        i, j, l = nodes[5]
        if min(i, j, l) >= 1 and max(i, j, l) < N - 1:
            direct = np.einsum("a,b,c,nabc->n", w, w, w, v[:, i - 1:i + 2, j - 1:j + 2, l - 1:l + 2])
            assert np.allclose(ref[5], direct, rtol=1e-12, atol=0)


def test_sample_half_cell_ties(world):
    """p = k + 0.5 exactly, k even and odd, on each axis alone and on all three: the base is k (ties away from zero), fd = 0.5, weights
    {1/2, 1/2, 0} - a tie resolved the other way would weigh node k + 2 instead of k."""
    world.use("hashed")
    pts = []
    for lo in (A_LO, B_LO):
        c = np.array(lo, dtype=np.float64) + 3.25
        for k in range(-2, 12):
            for axis in range(3):
                p = c.copy()
                p[axis] = lo[axis] + k + 0.5
                pts.append(p)
            pts.append(np.array(lo, dtype=np.float64) + k + 0.5)
    pts = np.array(pts)
    pts = pts[((pts >= 0) & (pts < N)).all(axis=1)]
    assert ((pts % 2) == 0.5).any() and ((pts % 2) == 1.5).any()                               # even and odd k
    check_sample(world, pts / N, "half-cell ties")


def test_sample_random_points_over_the_registered_region(world):
    world.use("hashed")
    rng = np.random.default_rng(11)
    n = 100003
    p = 4.0 * world.keys[rng.integers(0, world.nbc, n)] + rng.uniform(0.0, 4.0, (n, 3))
    check_sample(world, (p / N).astype(np.float32), "random points")


def test_sample_across_registered_exterior_and_absent_blocks(world):
    """Points in and on the faces of the exterior-only blocks and one block further out: their stencils mix registered nodes, exterior-only
    blocks (zero, although the table knows them) and blocks the table does not hold.  A kernel that trusted the table alone would read grid
    rows beyond nbc."""
    m = world.use("hashed")
    rng = np.random.default_rng(12)
    ex = world.exterior
    inside = 4.0 * ex[rng.integers(0, len(ex), 20000)] + rng.uniform(0.0, 4.0, (20000, 3))
    faces = 4.0 * ex[rng.integers(0, len(ex), 6000)] + rng.choice([0.0, 0.49, 0.5, 0.51, 3.49, 3.5, 3.51, 4.0], (6000, 3))
    beyond = 4.0 * (ex[rng.integers(0, len(ex), 6000)] + rng.integers(-1, 2, (6000, 3))) + rng.uniform(0.0, 4.0, (6000, 3))
    pts = np.concatenate([inside, faces, beyond])
    pts = pts[((pts >= 0) & (pts < N)).all(axis=1)]
    got, ref, S = check_sample(world, (pts / N).astype(np.float32), "exterior and absent blocks")
    # the three kinds are all met: stencils with mass, and stencils wholly inside exterior-only blocks, which read exact zeros
    _, base, _ = m.stencil((pts / N).astype(np.float32))
    exset = {tuple(k) for k in ex.tolist()}
    wholly = np.array([all(((b[0] + i) >> 2, (b[1] + j) >> 2, (b[2] + l) >> 2) in exset for i in (0, 2) for j in (0, 2) for l in (0, 2)) for b in base.tolist()])
    assert wholly.sum() > 100 and not got[wholly].any() and (S[:, 0] > 0).sum() > 1000 and (S[:, 0] == 0).sum() > 1000


def test_sample_at_the_faces(world):
    """[0, dx / 2): base -1, node -1 does not exist.  The last cell below an upper face: base up to N - 1, nodes N and N + 1 do not exist."""
    world.use("hashed")
    rng = np.random.default_rng(13)
    n = 4000
    a = np.array(A_LO) + rng.uniform(-1.0, 9.0, (n, 3))
    a[:, 0] = rng.uniform(0.0, 0.5, n)                                                          # over box A, x below dx / 2
    a[:5, 0] = [0.0, np.nextafter(np.float32(0.5), np.float32(0)), 0.25, 1e-30, 0.499]
    b = np.array(B_LO) + rng.uniform(-1.0, 9.0, (n, 3))
    b[:, 2] = rng.uniform(N - 1.0, N, n)                                                        # over box B, z in the last cell
    b[:3, 2] = [N - 1.0, N - 0.5, float(np.nextafter(np.float32(N), np.float32(0)))]
    got, _, S = check_sample(world, (np.concatenate([a, b]) / N).astype(np.float32), "faces")
    assert (S[:n, 0] > 0).sum() > n // 2 and (S[n:, 0] > 0).sum() > n // 2
    # the other four faces hold no block: zeros, through the same code path
    o = rng.uniform(0.0, N, (3000, 3))
    o[:1000, 1], o[1000:2000, 2], o[2000:, 0] = rng.uniform(0, 0.5, 1000), rng.uniform(0, 0.5, 1000), rng.uniform(N - 1.0, N, 1000)
    check_sample(world, (o / N).astype(np.float32), "empty faces", expect_nonzero=False)


def test_sample_outside_the_domain_and_not_finite(world):
    world.use("hashed")
    inside = (np.array(A_LO) + 3.3) / N
    bad = []
    for axis in range(3):
        for v in (np.nan, np.inf, -np.inf, -1e-7, -0.5, 1.0, 1.5, 3e38, -3e38, float(np.nextafter(np.float32(0), np.float32(-1)))):
            p = inside.copy()
            p[axis] = v
            bad.append(p)
    bad = np.array(bad + [[np.nan] * 3, [np.inf] * 3, [-1.0, 2.0, 0.5]], dtype=np.float32)
    pts = np.concatenate([bad, np.float32([inside])])
    got = raw_sample(world.eng, pts)
    assert not got[:-1].view(np.uint32).any(), "a point outside the domain did not give four +0"
    assert got[-1, 0] > 0                                                                        # (the one good point of the same launch is served)


@pytest.mark.parametrize("n", [0, 1, 64, 65])
def test_sample_counts(world, n):
    world.use("hashed")
    rng = np.random.default_rng(n)
    pts = ((np.array(B_LO) + rng.uniform(0.0, 8.0, (n, 3))) / N).astype(np.float32)
    if n == 0:
        assert world.eng.api.sample_grid(world.eng.ctx, None, 0, None) == _ffi.MPM_OK             # legal, launches nothing
        out = world.eng.sample_grid(np.zeros((0, 3), np.float32))
        assert out["mass"].shape == (0,) and out["momentum"].shape == (0, 3) and out["velocity"].shape == (0, 3)
        return
    guard = np.full((n + 1, 4), np.float32(-7.0))
    assert world.eng.api.sample_grid(world.eng.ctx, pts.ctypes.data_as(C.c_void_p), n, guard.ctypes.data_as(C.c_void_p)) == _ffi.MPM_OK
    assert (guard[n] == -7.0).all()                                                              # nothing written behind the n-th point
    check_sample(world, pts, f"n = {n}")
    out = world.eng.sample_grid(pts)
    assert np.array_equal(out["mass"], guard[:n, 0]) and np.array_equal(out["momentum"], guard[:n, 1:])
    assert np.array_equal(out["density"], guard[:n, 0].astype(np.float64) * float(N) ** 3)
    assert np.allclose(out["velocity"], guard[:n, 1:].astype(np.float64) / guard[:n, :1].astype(np.float64), rtol=1e-15)


# ---- volume ---------------------------------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = g != w
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), [hex(v) for v in g[bad][:4]], [hex(v) for v in w[bad][:4]])


def test_volume_stride_1_copies_the_words(world):
    """NaN payloads, -0, infinities and denormals arrive as they are: the whole domain, and boxes with a negative origin that overhang upper
    faces, aligned to nothing."""
    m = world.use("special")
    whole = world.eng.grid_volume()
    same_bits(whole, m.volume((0, 0, 0), (N, N, N), 1))
    special = {0x7FC01234, 0xFFABCDEF, 0x80000000, 0x7F800001, 0x00000001}
    assert special <= set(np.unique(whole.view(np.uint32)).tolist())
    for origin, dims in (((-5, 45, 35), (30, 37, 20)), ((101, 50, 99), (41, 30, 45)), ((-3, -2, 110), (133, 131, 19)), ((-9, -9, -9), (4, 4, 4)), ((N, 0, 0), (3, 2, 1))):
        same_bits(world.eng.grid_volume(origin, dims, 1), m.volume(origin, dims, 1))


@pytest.mark.parametrize("stride", [2, 4])
def test_volume_strides_bit_for_bit(world, stride):
    """acc = +0, then += the covered nodes, x slowest and z fastest, in float32: whole domain (aligned to stride and blocks), origin (3, 5, 6)
    (aligned to neither), a dims entry of 1, boxes that leave the domain."""
    m = world.use("hashed")
    s = stride
    same_bits(world.eng.grid_volume(stride=s), m.volume((0, 0, 0), (N // s,) * 3, s))
    cases = [((3, 5, 6), ((N - 3) // s + 1, (N - 5) // s, (N - 6) // s + 2)), ((3, 53, 6), (N // s - 1, 1, N // s)), ((0, 50, 41), (1, 9, 5)), ((113, 61, 118), (4, 3, 1)),
             ((-7, 47, 37), (11, 7, 9)), ((2, 52, 42 - N), (1, 1, 2 * N // s))]
    for origin, dims in cases:
        got, want = world.eng.grid_volume(origin, dims, s), m.volume(origin, dims, s)
        same_bits(got, want)
        assert want[0].sum() > 0, (origin, dims)                                               # (every case meets registered blocks)


def test_volume_single_cell(world):
    m = world.use("hashed")
    node = 4 * world.keys[world.nbc // 3] + (1, 2, 3)
    for s in (1, 2, 4):
        got = world.eng.grid_volume(node, (1, 1, 1), s)
        same_bits(got, m.volume(node, (1, 1, 1), s))
        assert got[0, 0, 0, 0] > 0
    same_bits(world.eng.grid_volume((70, 5, 5), (1, 1, 1), 1), np.zeros((4, 1, 1, 1), np.float32))


# ---- totals ---------------------------------------------------------------------------------------------------------------------------------
BOXES = {"whole domain": ((0, 0, 0), (N, N, N)), "beyond the domain": ((-50, -1, -7), (400, 129, 1000)), "cutting blocks": ((2, 51, 42), (7, 57, 47)),
         "cutting box B": ((110, 63, 119), (121, 90, 127)), "one node": ((118, 64, 120), (119, 65, 121)), "empty space": ((60, 8, 8), (90, 30, 30)),
         "empty box": ((5, 52, 42), (5, 60, 50)), "inverted box": ((9, 9, 9), (3, 3, 3))}


@pytest.mark.parametrize("name", sorted(BOXES))
def test_box_totals(world, name):
    m = world.use("hashed")
    lo, hi = BOXES[name]
    t = world.eng.grid_box_totals(lo, hi)
    got = np.concatenate([[t["mass"]], t["momentum"], [t["kinetic"]]])
    ref, mag = m.box_totals(lo, hi)
    print(name, "got", got.tolist(), "ref", ref.tolist(), "err / mag", (np.abs(got - ref) / np.where(mag > 0, mag, 1)).tolist())
    assert (np.abs(got - ref) <= 2.0 ** -40 * mag).all()
    if name in ("empty space", "empty box", "inverted box"):
        assert not got.any()
    else:
        assert got[0] > 0 and got[4] > 0
    if name in ("whole domain", "beyond the domain"):
        gt = world.eng.grid_totals()
        assert (np.abs(gt - got[:4]) <= 2.0 ** -40 * mag[:4]).all() and (np.abs(gt - ref[:4]) <= 2.0 ** -40 * mag[:4]).all()


# ---- a real grid ----------------------------------------------------------------------------------------------------------------------------
def test_consistency_on_the_grid_of_a_run():
    sc = scene()
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(20, DT)
    keys, blocks = eng.dump_grid()
    m = gfm.GridField(keys, blocks, BITS)
    vol = eng.grid_volume()
    same_bits(vol, m.volume((0, 0, 0), (N, N, N), 1))
    count = sum(mod["xyz"].shape[0] for mod in sc["models"])
    assert count == sum(int(c) for c in eng.counts().particles[:2]) and eng.diagnostics().lost_particles == 0
    want = count * eng.model_mass(0)
    for s in (1, 2, 4):
        total = float(eng.grid_volume(stride=s)[0].astype(np.float64).sum())
        print(f"stride {s}: mass {total!r}, particles x mass {want!r}, relative {abs(total - want) / want:.3e} (bound {220 * EPS:.3e})")
        assert abs(total - want) <= 220 * EPS * want
    t = eng.grid_box_totals((0, 0, 0), (N, N, N))
    assert abs(t["mass"] - want) <= 220 * EPS * want and t["kinetic"] > 0
    # probes through Engine.sample_grid: the model's value of the dumped grid, density = mass / dx^3, velocity = momentum / mass
    pts = ((np.array([A_LO, B_LO]) + 4.0) / N).astype(np.float32)
    probe = eng.sample_grid(pts)
    ref, S = m.sample(pts)
    assert (np.abs(np.concatenate([probe["mass"][:, None], probe["momentum"]], axis=1) - ref) <= 64 * EPS * S).all() and (ref[:, 0] > 0).all()
    assert np.array_equal(probe["density"], probe["mass"].astype(np.float64) * float(N) ** 3)
    assert np.allclose(probe["velocity"], ref[:, 1:] / ref[:, :1], rtol=1e-5, atol=0)
    print("probes: density", probe["density"].tolist(), "velocity", probe["velocity"].tolist())
    eng.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    sc = scene()
    eng = build_engine(sc)
    api, ctx = eng.api, eng.ctx
    pts = np.float32([[0.05, 0.42, 0.34]])
    out4, out5 = np.zeros((1, 4), np.float32), (C.c_double * 5)()
    i3 = lambda *v: (C.c_int * 3)(*v)                                                           # noqa: E731
    vol = np.zeros((4, 2, 2, 2), np.float32)

    def calls(origin=(0, 50, 40), dims=(2, 2, 2), stride=1):
        return (api.sample_grid(ctx, pts.ctypes.data_as(C.c_void_p), 1, out4.ctypes.data_as(C.c_void_p)),
                api.grid_volume(ctx, i3(*origin), i3(*dims), stride, vol.ctypes.data_as(C.c_void_p)),
                api.grid_box_totals(ctx, i3(0, 0, 0), i3(N, N, N), out5))

    assert calls() == (_ffi.MPM_ERR_NOT_READY,) * 3                                               # before set-up
    eng.initial_setup()
    assert calls() == (_ffi.MPM_OK,) * 3 and out4[0, 0] > 0 and out5[0] > 0
    # a bare grid update: the grid holds velocities until the next rebuild
    eng.grid_update(DT)
    assert calls() == (_ffi.MPM_ERR_INVALID,) * 3 and "holds velocities" in api.last_error(ctx).decode()
    with pytest.raises(EngineError) as e:
        eng.grid_volume()
    assert e.value.code == _ffi.MPM_ERR_INVALID
    eng.g2p2g(DT, DT)
    assert calls() == (_ffi.MPM_ERR_INVALID,) * 3
    eng.rebuild_partition()
    assert calls() == (_ffi.MPM_OK,) * 3
    # bad stride or dims
    for stride in (0, 3, 8, -1):
        assert calls(stride=stride)[1] == _ffi.MPM_ERR_INVALID and "stride" in api.last_error(ctx).decode()
        with pytest.raises(EngineError):
            eng.grid_volume(stride=stride)
    for dims in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
        assert calls(dims=dims)[1] == _ffi.MPM_ERR_INVALID and "dims" in api.last_error(ctx).decode()
    assert api.grid_volume(ctx, None, i3(1, 1, 1), 1, vol.ctypes.data_as(C.c_void_p)) == _ffi.MPM_ERR_INVALID
    assert api.grid_volume(ctx, i3(0, 0, 0), i3(1, 1, 1), 1, None) == _ffi.MPM_ERR_INVALID
    assert api.sample_grid(ctx, None, 1, out4.ctypes.data_as(C.c_void_p)) == _ffi.MPM_ERR_INVALID
    assert api.grid_box_totals(ctx, i3(0, 0, 0), i3(1, 1, 1), None) == _ffi.MPM_ERR_INVALID
    assert calls() == (_ffi.MPM_OK,) * 3                                                          # after each refusal a valid call succeeds
    # a group of one
    ctxs, groups = (C.c_void_p * 1)(ctx.value), (C.c_void_p * 1)()
    assert api.group_create_local(ctxs, 1, groups) == _ffi.MPM_OK
    try:
        assert calls() == (_ffi.MPM_ERR_INVALID,) * 3 and "group" in api.last_error(ctx).decode()
    finally:
        api.group_destroy(groups[0])
    assert calls() == (_ffi.MPM_OK,) * 3                                                          # (no group call ran: the grid is its own again)
    eng.close()


# ---- no side effects ------------------------------------------------------------------------------------------------------------------------
def written(buf):
    """Every byte mpm_checkpoint_save writes: the header and the sections in use.  (Between two sections the buffer is padded to 16 bytes;
    the save leaves those bytes as the caller's buffer had them, and Engine.save_checkpoint hands it an uninitialised one.)"""
    h = cf.parse(buf)
    return np.concatenate([buf[:cf.HEADER_BYTES]] + [buf[at:at + n] for at, n in h["sections"].values()])


def test_the_readouts_change_nothing():
    """A checkpoint taken before the calls and one taken after them are the same bytes (every byte the save writes), and five more substeps from either give the same
    particle state bit for bit.  (Two boxes of 64 particles, each inside ONE particle block and so inside one wave: P2G's float atomics then
    arrive in a fixed order and two runs of the engine agree to the bit, which a dense body's do not - tests/test_gmpm_stress_gpu.py.)"""
    prm = {"volume": scenes._vol(BITS), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    sc = {"name": "grid_field_small", "bits": BITS, "dt": DT, "config": {"max_ppc": 128},
          "models": [{"material": _ffi.FIXED_COROTATED, "xyz": scenes.lattice_box(BITS, (8, 19, 19), (10, 21, 21)), "v0": (-0.5, 0.0, 0.0), "params": dict(prm)},
                     {"material": _ffi.SAND, "xyz": scenes.lattice_box(BITS, (8, 31, 31), (10, 33, 33)), "v0": (-0.5, 0.0, 0.0), "params": {}}]}
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(4, DT)
    before = eng.save_checkpoint().copy()
    rng = np.random.default_rng(3)
    eng.sample_grid(rng.uniform(0.0, 1.0, (5000, 3)))
    for s in (1, 2, 4):
        eng.grid_volume(stride=s)
    eng.grid_volume((3, 5, 6), (20, 1, 31), 4)
    eng.grid_box_totals((0, 0, 0), (N, N, N))
    after = eng.save_checkpoint().copy()
    assert np.array_equal(written(before), written(after))
    eng.run_fixed(5, DT)                                                                         # from the context the calls were made on
    a = [eng.retrieve_state(mi) for mi in range(2)]
    eng.load_checkpoint(before)
    eng.run_fixed(5, DT)
    b = [eng.retrieve_state(mi) for mi in range(2)]
    eng.load_checkpoint(after)
    eng.run_fixed(5, DT)
    c = [eng.retrieve_state(mi) for mi in range(2)]

    def rows(x, st, lj):
        r = np.concatenate([x, st, lj[:, None]], axis=1).view(np.uint32)
        return r[np.lexsort(r.T[::-1])]
    for p, q, r in zip(a, b, c):
        assert np.array_equal(rows(*p), rows(*q)) and np.array_equal(rows(*q), rows(*r))
    eng.close()


# ---- the gmpm driver ------------------------------------------------------------------------------------------------------------------------
FPS, FRAMES, DT_DEFAULT = 500, 2, 1e-4
FC = {"rho": 1e3, "volume": float(np.float32((1 / N) ** 3 / 8)), "youngs_modulus": 5e3, "poisson_ratio": 0.4}
# (the boxes of tests/test_gmpm_stress_gpu.py at bits 7: 64 particles each, inside ONE particle block, so that two runs give the same bits)
MODELS = [dict(FC, file="box", constitutive="fixed_corotated", offset=[7.5 / N, 18.5 / N, 18.5 / N], span=[2 / N] * 3, velocity=[-0.5, 0, 0]),
          {"file": "box", "constitutive": "sand", "offset": [7.5 / N, 30.5 / N, 30.5 / N], "span": [2 / N] * 3, "velocity": [-0.5, 0, 0]}]


def run_gmpm(d, **keys):
    d.mkdir()
    sim = dict({"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d)}, **keys)
    fn = d / "scene.json"
    fn.write_text(json.dumps({"simulation": sim, "models": MODELS}))
    subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(fn)], text=True, timeout=300)
    return d


def test_gmpm_output_grid(tmp_path):
    import __graft_entry__ as g
    g.build_host()
    plain = run_gmpm(tmp_path / "plain")
    grid = run_gmpm(tmp_path / "grid", output_grid={"stride": 4})
    names = sorted(p.name for p in plain.iterdir())
    assert not [n for n in names if n.endswith(".npy")] and len([n for n in names if n.endswith(".bgeo")]) == 2 * (FRAMES + 1)
    assert sorted(p.name for p in grid.iterdir()) == sorted(names + [f"grid_frame[{f}].npy" for f in range(1, FRAMES + 1)])
    for n in names:
        if n.endswith(".bgeo"):
            assert (plain / n).read_bytes() == (grid / n).read_bytes(), n                        # the frames are what they are without the key
    eng = Engine(domain_bits=BITS)
    sand = eng.default_material(_ffi.SAND)
    eng.close()
    want = 64 * float(np.float32(FC["volume"]) * np.float32(FC["rho"])) + 64 * float(np.float32(sand.volume) * np.float32(sand.rho))
    for f in range(1, FRAMES + 1):
        raw = (grid / f"grid_frame[{f}].npy").read_bytes()
        assert raw[:8] == b"\x93NUMPY\x01\x00"
        v = np.load(grid / f"grid_frame[{f}].npy")
        assert v.dtype == np.dtype("<f4") and v.shape == (4, N // 4, N // 4, N // 4) and v.flags.c_contiguous
        total = float(v[0].astype(np.float64).sum())
        print(f"frame {f}: mass {total!r} of {want!r}, relative {abs(total - want) / want:.3e}")
        assert abs(total - want) <= 220 * EPS * want
        assert v[1].sum() < 0 and not v[:, 16:].any()                                           # both boxes fly toward -x, in the lower x half
    with pytest.raises(subprocess.CalledProcessError):
        run_gmpm(tmp_path / "bad", output_grid={"stride": 3})

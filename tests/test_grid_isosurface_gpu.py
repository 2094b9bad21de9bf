"""mpm_grid_isosurface on the GPU (claymore_amd/csrc/mpm_grid_isosurface.hpp) against tests/grid_isosurface_model.py, on INJECTED grids - the
world of tests/test_grid_field_gpu.py: two 8^3-node boxes, one against the lower x face and one in the upper z wall zone, three substeps, a
checkpoint whose grid section is replaced through ckpt_format.with_grid - and on grids a run leaves behind.

The triangles are compared as a MULTISET, bit for bit (the canonical form of the model: every triangle rotated to its smallest vertex, the
triangles sorted): a cell emitted twice, or by nobody, across a block face, edge or corner, beside an exterior or an absent block, or at
the cells -1 and N - 1 changes it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ckpt_format as cf
import grid_field_model as gfm
import grid_isosurface_model as im
from claymore_amd import _ffi
from claymore_amd.engine import Engine, EngineError, build_engine
from test_grid_field_gpu import A_LO, BITS, DT, FRAMES, MODELS, FC, N, run_gmpm, scene, special_pattern, written
from test_particle_stress_cpu import read_bgeo_attrs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
G = N // 4
BALL_CENTRE, BALL_RADIUS, BALL_ISO = np.array(A_LO) + (3.8, 3.8, 3.2), 3.5, 2.0


def ball_pattern(keys):
    """f = max(0, R + iso - r) around a non-lattice point of box A, in the valued blocks only: the contour f = iso is the sphere of radius R,
    whose inside nodes all lie in the box's own nodes.  Momenta = f times a smooth velocity."""
    local = np.stack(np.meshgrid(range(4), range(4), range(4), indexing="ij"), axis=-1).reshape(-1, 3)      # cell (x << 4) | (y << 2) | z
    nodes = 4 * keys[:, None, :] + local[None]
    f = np.maximum(0.0, BALL_RADIUS + BALL_ISO - np.linalg.norm(nodes - BALL_CENTRE, axis=-1))
    vel = np.stack([0.3 + 0.01 * nodes[..., 0], -0.2 + 0.0 * nodes[..., 1], 0.1 - 0.02 * nodes[..., 2]], axis=1)
    return np.concatenate([f[:, None, :], f[:, None, :] * vel], axis=1).astype(np.float32)


SPECIAL_WORDS = np.array([0x7FC00000, 0x7FC01234, 0x7F800001, 0xFFC00000, 0xFFABCDEF, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32)


def special_mass_pattern(base):
    """test_grid_field_gpu's special pattern with every one of its words - NaNs, -0, +-inf, denormals - in the MASS channel as well, at cells
    inside blocks and on their faces and corners."""
    pat = special_pattern(base)
    nb = pat.shape[0]
    for i, w in enumerate(SPECIAL_WORDS):
        pat[(11 * i + 3) % nb, 0, (17 * i + 21) % 64] = w
        pat[(5 * i + 2) % nb, 0, (0, 63, 3, 60, 15, 48, 12, 51, 5, 42)[i]] = w
    return pat


class World:
    """One context of the scene after three substeps, its checkpoint, and the models of the injected grids."""

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
        self.patterns = {"hashed": hashed.view(np.uint32), "special": special_mass_pattern(hashed), "ball": ball_pattern(self.keys).view(np.uint32),
                         "run": cf.grid(self.ckpt).copy().view(np.uint32)}
        self.fields, self.surfaces, self.current = {}, {}, None

    def use(self, name):
        if self.current != name:
            self.eng.load_checkpoint(cf.with_grid(self.ckpt, self.patterns[name]))
            self.current = name
        if name not in self.fields:
            self.fields[name] = gfm.GridField(self.keys, self.patterns[name], BITS)
        return self.fields[name]

    def surface(self, name, iso):
        """The model's surface of the whole grid (with velocities), computed once."""
        if (name, iso) not in self.surfaces:
            self.surfaces[name, iso] = im.isosurface(self.use(name).dense, iso, velocity=True)
        self.use(name)
        return self.surfaces[name, iso]


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.eng.close()


GUARD = np.float32(-7.0)


def raw(eng, iso, box=None, cap=None, vel=False, count_only=False):
    """One call of mpm_grid_isosurface: (status, *n on exit, tris (cap, 3, 3), vel or None).  The buffers carry four guard triangles behind
    the capacity, checked here."""
    i3 = lambda v: (C.c_int * 3)(*[int(x) for x in v])                            # noqa: E731
    lo, hi = (i3(box[0]), i3(box[1])) if box is not None else (None, None)
    n = C.c_size_t(0 if cap is None else cap)
    if count_only:
        return eng.api.grid_isosurface(eng.ctx, iso, lo, hi, None, None, C.byref(n)), n.value, None, None
    tris = np.full((cap + 4, 3, 3), GUARD)
    vels = np.full((cap + 4, 3, 3), GUARD) if vel else None
    rc = eng.api.grid_isosurface(eng.ctx, iso, lo, hi, tris.ctypes.data_as(C.c_void_p), vels.ctypes.data_as(C.c_void_p) if vel else None, C.byref(n))
    assert (tris[cap:] == GUARD).all() and (vels is None or (vels[cap:] == GUARD).all()), "written behind the capacity"
    return rc, n.value, tris[:cap], (vels[:cap] if vel else None)


def fetch(eng, iso, box=None, vel=False):
    """Count, then fetch with the exact capacity."""
    rc, count, _, _ = raw(eng, iso, box, count_only=True)
    assert rc == _ffi.MPM_OK, eng.api.last_error(eng.ctx)
    rc, n, tris, vels = raw(eng, iso, box, cap=count, vel=vel)
    assert rc == _ffi.MPM_OK and n == count, (rc, n, count, eng.api.last_error(eng.ctx))
    return tris, vels


def same_multiset(got, want, label):
    a, b = im.canonical(got), im.canonical(want)
    assert a.shape == b.shape, (label, a.shape, b.shape)
    bad = (a != b).any(axis=1)
    assert not bad.any(), (label, int(bad.sum()), a[bad][:2].view(np.float32).tolist(), b[bad][:2].view(np.float32).tolist())


# ---- the scene ------------------------------------------------------------------------------------------------------------------------------
def test_scene_has_valued_exterior_and_absent_blocks(world):
    m = world.use("hashed")
    assert 0 < world.nbc < world.ebc and world.exterior.shape[0] == world.ebc - world.nbc
    assert (world.keys[:, 0] == 0).any() and (world.keys[:, 2] == G - 1).any()               # valued blocks at key 0 and key G - 1
    assert world.ebc < G ** 3 // 8                                                           # most of the domain is absent
    valued = {tuple(k) for k in world.keys.tolist()}
    known = valued | {tuple(k) for k in world.exterior.tolist()}
    around = lambda k: [(k[0] + a, k[1] + b, k[2] + c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]   # noqa: E731
    kinds = [{"valued" if q in valued else "exterior" if q in known else "absent" for q in around(k)} for k in world.keys.tolist()]
    assert set().union(*kinds) == {"valued", "exterior", "absent"}                           # valued blocks border all three kinds
    assert any("exterior" in s for s in kinds) and any("absent" in s for s in kinds)
    assert (m.values()[0] > 1).any() and (m.values()[0] < 1).any()


# ---- 1, 2: the hashed grid ------------------------------------------------------------------------------------------------------------------
def test_hashed_grid_is_the_models_multiset(world):
    want = world.surface("hashed", 1.0)
    tris, _ = fetch(world.eng, 1.0)
    print(f"hashed grid: {len(tris)} triangles (model {want.count}), {int((~im.nondegenerate(tris)).sum())} degenerate; cells from {want.cell.min(axis=0).tolist()} to {want.cell.max(axis=0).tolist()}")
    assert len(tris) == want.count and want.count > 10000
    assert (want.cell[:, 0] == -1).any() and (want.cell[:, 2] == N - 1).any()                 # the cells outside the lowest and in the last node layer
    same_multiset(tris, want.tris, "hashed")
    assert im.open_edges(tris) == 0
    soup = world.eng.isosurface(iso_mass=1.0, weld=False)
    same_multiset(soup, want.tris, "Engine.isosurface(weld=False)")


def test_hashed_grid_velocities(world):
    want = world.surface("hashed", 1.0)
    tris, vels = fetch(world.eng, 1.0, vel=True)
    same_multiset(tris, want.tris, "hashed with velocities")                                  # the positions do not depend on the flag
    og, rg = im.canonical_order(tris)
    om, rm = im.canonical_order(want.tris)
    got = im.apply_order(vels, og, rg).astype(np.float64)
    ref, S = im.apply_order(want.ref, om, rm), im.apply_order(want.S, om, rm)
    canon = im.canonical(tris)
    twin = np.zeros(len(canon), dtype=bool)                                                   # equal triangles (degenerate ones meeting at a node) have no defined pairing
    twin[1:] |= (canon[1:] == canon[:-1]).all(axis=1)
    twin[:-1] |= twin[1:].copy()
    assert twin.sum() <= len(canon) // 100
    got, ref, S = got[~twin], ref[~twin], S[~twin]
    err = np.abs(got - ref)
    worst = float((err[S > 0] / (EPS * S[S > 0])).max())
    print(f"velocities: {got.shape[0]} triangles compared, {int(twin.sum())} twins left out, worst error {worst:.2f} eps S (bound 8)")
    assert np.isfinite(got).all() and (S > 0).all()
    assert (err <= 8 * EPS * S).all(), (int((err > 8 * EPS * S).sum()), worst)


# ---- 3: a smooth field ----------------------------------------------------------------------------------------------------------------------
def test_ball(world):
    want = world.surface("ball", BALL_ISO)
    m = world.use("ball")
    inside = np.argwhere(m.values()[0] > BALL_ISO)
    assert len(inside) > 100 and (inside >= np.array(A_LO)).all() and (inside < np.array(A_LO) + 8).all()   # the ball fits the box's own nodes
    tris, vels = fetch(world.eng, BALL_ISO, vel=True)
    same_multiset(tris, want.tris, "ball")
    vol, sphere = im.signed_volume(tris.astype(np.float64) * N), 4.0 / 3.0 * np.pi * BALL_RADIUS ** 3
    print(f"ball: {len(tris)} triangles, volume {vol:.2f} cells^3, sphere {sphere:.2f}")
    assert len(tris) > 500 and im.open_edges(tris) == 0 and 0.8 * sphere < vol < 1.05 * sphere
    r = np.linalg.norm(tris.astype(np.float64) * N - BALL_CENTRE, axis=-1)
    assert np.abs(r - BALL_RADIUS).max() < 0.3
    # the velocity is the smooth field's, up to the linear interpolation along an edge
    p = tris.astype(np.float64) * N
    field = np.stack([0.3 + 0.01 * p[..., 0], -0.2 + 0.0 * p[..., 1], 0.1 - 0.02 * p[..., 2]], axis=-1)
    assert np.abs(vels - field).max() < 0.021                                                 # (a convex combination of the two nodes' velocities)
    V, F, W = world.eng.isosurface(iso_mass=BALL_ISO, velocity=True)
    assert im.open_edges(V[F]) == 0 and len(F) == int(im.nondegenerate(tris).sum()) and W.shape == V.shape


# ---- 4: clipping ----------------------------------------------------------------------------------------------------------------------------
BOXES = {"from -1": ((-1, -1, -1), (6, 60, 50)), "ends mid-block": ((0, 50, 40), (6, 55, 46)), "one cell thick in x": ((3, 0, 0), (4, N, N)), "the cell layer -1": ((-1, 0, 0), (0, N, N)),
         "the last cell layer in z": ((0, 0, N - 1), (N, N, N)), "one cell": ((4, 54, 44), (5, 55, 45)), "empty space": ((60, 8, 8), (90, 30, 30)), "beyond the domain": ((N, 0, 0), (N + 5, 5, 5)),
         "below the domain": ((-9, -9, -9), (-1, N, N)), "far around the domain": ((-1000, -1000, -1000), (1000, 1000, 1000)), "inverted": ((9, 60, 50), (3, 50, 40))}


@pytest.mark.parametrize("name", sorted(BOXES))
def test_cell_boxes(world, name):
    whole = world.surface("hashed", 1.0)
    lo, hi = BOXES[name]
    sel = ((whole.cell >= np.array(lo)) & (whole.cell < np.array(hi))).all(axis=1)
    tris, _ = fetch(world.eng, 1.0, box=(lo, hi))
    print(f"{name}: {len(tris)} triangles, model {int(sel.sum())}")
    assert len(tris) == int(sel.sum())
    same_multiset(tris, whole.tris[sel], name)
    if name in ("empty space", "beyond the domain", "below the domain", "inverted"):
        assert len(tris) == 0
    elif name == "far around the domain":
        assert len(tris) == whole.count
    else:
        assert 0 < len(tris) < whole.count
    if name == "ends mid-block":
        same_multiset(world.eng.isosurface(iso_mass=1.0, box=(lo, hi), weld=False), whole.tris[sel], name)


# ---- 5: the capacity protocol ---------------------------------------------------------------------------------------------------------------
def test_capacity_protocol(world):
    want = world.surface("hashed", 1.0)
    eng = world.eng
    members = {row.tobytes() for row in want.canonical()}
    rc, count, _, _ = raw(eng, 1.0, count_only=True)
    assert rc == _ffi.MPM_OK and count == want.count
    n = C.c_size_t(12345)                                                                     # count only: the capacity on entry does not matter
    assert eng.api.grid_isosurface(eng.ctx, 1.0, None, None, None, None, C.byref(n)) == _ffi.MPM_OK and n.value == count
    rc, n, tris, _ = raw(eng, 1.0, cap=count)
    assert rc == _ffi.MPM_OK and n == count
    same_multiset(tris, want.tris, "exact capacity")
    rc, n, tris, _ = raw(eng, 1.0, cap=count + 100)
    assert rc == _ffi.MPM_OK and n == count and (tris[count:] == GUARD).all()
    same_multiset(tris[:count], want.tris, "room to spare")
    for cap, vel in ((count - 1, False), (1, False), (count // 2, True)):
        rc, n, tris, vels = raw(eng, 1.0, cap=cap, vel=vel)
        assert rc == _ffi.MPM_ERR_CAPACITY and n == count, (cap, rc, n)
        assert "triangles" in eng.api.last_error(eng.ctx).decode()
        assert all(row.tobytes() in members for row in im.canonical(tris)), cap               # `capacity` triangles of the surface, whichever
        assert vels is None or np.isfinite(vels).all()
        rc, n, _, _ = raw(eng, 1.0, count_only=True)                                          # the context stays usable
        assert rc == _ffi.MPM_OK and n == count
    rc, n, tris, _ = raw(eng, 1.0, cap=0)                                                     # capacity 0 with a buffer: nothing fits
    assert rc == _ffi.MPM_ERR_CAPACITY and n == count
    rc, n, tris, _ = raw(eng, 1.0, box=BOXES["empty space"], cap=0)                           # ... unless the surface is empty
    assert rc == _ffi.MPM_OK and n == 0
    one = np.zeros((1, 3, 3), np.float32)
    for huge in (1 << 40, 1 << 62):                                                           # a staging buffer the device cannot hold, or size_t
        n = C.c_size_t(huge)
        assert eng.api.grid_isosurface(eng.ctx, 1.0, None, None, one.ctypes.data_as(C.c_void_p), None, C.byref(n)) == _ffi.MPM_ERR_CAPACITY
    rc, n, tris, _ = raw(eng, 1.0, cap=count)
    assert rc == _ffi.MPM_OK and n == count
    with pytest.raises(EngineError):
        eng.isosurface()
    with pytest.raises(EngineError):
        eng.isosurface(density=1.0, iso_mass=1.0)


# ---- 6: words that are no numbers -----------------------------------------------------------------------------------------------------------
def test_special_pattern_counts(world):
    m = world.use("special")
    bits = set(np.unique(m.dense[0]).tolist())
    assert set(SPECIAL_WORDS.tolist()) <= bits                                                # NaNs, +-inf, -0, denormals in the mass channel
    for iso in (1.0, 2.0 ** -30, 2.0 ** 21):
        want = im.isosurface(m.dense, iso)
        rc, count, _, _ = raw(world.eng, iso, count_only=True)
        assert rc == _ffi.MPM_OK and count == want.count, (iso, count, want.count)
        rc, n, tris, vels = raw(world.eng, iso, cap=count, vel=True)                          # nothing faults; the positions are not asserted
        assert rc == _ffi.MPM_OK and n == count
        print(f"special pattern, iso {iso!r}: {count} triangles, {int((~np.isfinite(tris)).any(axis=(1, 2)).sum())} with a non-finite position")
    assert im.isosurface(m.dense, 2.0 ** 21).count > 0                                        # (only +inf is inside)


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    eng = build_engine(scene())
    api, ctx = eng.api, eng.ctx
    i3 = lambda *v: (C.c_int * 3)(*v)                                                          # noqa: E731
    n = C.c_size_t(0)

    def count(iso=2.0 ** -12, lo=None, hi=None):
        n.value = 0
        return api.grid_isosurface(ctx, iso, lo, hi, None, None, C.byref(n))

    assert count() == _ffi.MPM_ERR_NOT_READY                                                   # before set-up
    eng.initial_setup()
    assert count() == _ffi.MPM_OK and n.value > 0
    good = n.value
    for iso in (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        assert count(iso) == _ffi.MPM_ERR_INVALID and "iso_mass" in api.last_error(ctx).decode(), iso
        with pytest.raises(EngineError):
            eng.isosurface(iso_mass=iso)
    assert count(lo=i3(0, 0, 0)) == _ffi.MPM_ERR_INVALID and count(hi=i3(N, N, N)) == _ffi.MPM_ERR_INVALID
    assert api.grid_isosurface(ctx, 1.0, None, None, None, None, None) == _ffi.MPM_ERR_INVALID            # NULL n
    buf = np.zeros((4, 3, 3), np.float32)
    n.value = 4
    assert api.grid_isosurface(ctx, 1.0, None, None, None, buf.ctypes.data_as(C.c_void_p), C.byref(n)) == _ffi.MPM_ERR_INVALID   # velocities alone
    assert count() == _ffi.MPM_OK and n.value == good                                          # after each refusal a valid call succeeds
    eng.grid_update(DT)                                                                        # the grid holds velocities until the next rebuild
    assert count() == _ffi.MPM_ERR_INVALID and "holds velocities" in api.last_error(ctx).decode()
    with pytest.raises(EngineError) as e:
        eng.isosurface(density=500.0)
    assert e.value.code == _ffi.MPM_ERR_INVALID
    eng.g2p2g(DT, DT)
    assert count() == _ffi.MPM_ERR_INVALID
    eng.rebuild_partition()
    assert count() == _ffi.MPM_OK and n.value > 0
    ctxs, groups = (C.c_void_p * 1)(ctx.value), (C.c_void_p * 1)()                              # a group of one
    assert api.group_create_local(ctxs, 1, groups) == _ffi.MPM_OK
    try:
        assert count() == _ffi.MPM_ERR_INVALID and "group" in api.last_error(ctx).decode()
    finally:
        api.group_destroy(groups[0])
    assert count() == _ffi.MPM_OK
    eng.close()


# ---- 8: no side effects ---------------------------------------------------------------------------------------------------------------------
def test_the_readout_changes_nothing(world):
    world.use("hashed")
    before = world.eng.save_checkpoint().copy()
    fetch(world.eng, 1.0, vel=True)
    fetch(world.eng, 1.0, box=BOXES["ends mid-block"])
    raw(world.eng, 1.0, cap=7)
    world.eng.isosurface(iso_mass=3.0)
    after = world.eng.save_checkpoint().copy()
    assert np.array_equal(written(before), written(after))


# ---- 9: a real grid -------------------------------------------------------------------------------------------------------------------------
def test_engine_isosurface_on_the_grid_of_the_run(world):
    """The world's own grid after its three substeps, at half the rest density: a closed welded mesh around the two boxes."""
    m = world.use("run")
    rho = 1e3
    V, F, W = world.eng.isosurface(density=0.5 * rho, velocity=True)
    want = im.isosurface(m.dense, np.float32(0.5 * rho / float(N) ** 3))
    Vm, Fm, _ = im.weld(want.tris)
    print(f"run: {len(V)} vertices, {len(F)} faces (model {len(Vm)}, {len(Fm)}); soup {want.count}")
    assert V.dtype == np.float32 and F.dtype == np.int32 and W.shape == V.shape and np.isfinite(W).all()
    assert len(F) > 1000 and F.min() == 0 and F.max() == len(V) - 1
    assert np.array_equal(V.view(np.uint32), Vm.view(np.uint32)) and len(F) == len(Fm)
    assert im.open_edges(V[F]) == 0 and im.signed_volume(V[F].astype(np.float64) * N) > 2 * 6.0 ** 3
    pts = np.concatenate([world.eng.retrieve_state(mi)[0] for mi in range(2)]).astype(np.float64) * N
    nearest = np.full(len(V), np.inf)
    for chunk in np.array_split(pts, 16):
        nearest = np.minimum(nearest, np.linalg.norm(V[:, None, :].astype(np.float64) * N - chunk[None], axis=-1).min(axis=1))
    print(f"run: the farthest vertex is {nearest.max():.2f} cells from a particle")
    assert nearest.max() < 2.0
    soup = world.eng.isosurface(density=0.5 * rho, weld=False)
    assert soup.shape == (want.count, 3, 3)
    same_multiset(soup, want.tris, "run")


# ---- 10: the gmpm driver --------------------------------------------------------------------------------------------------------------------
def parse_obj(path):
    v, f = [], []
    for line in open(path).read().splitlines():
        tag, *rest = line.split()
        assert tag in ("v", "f") and len(rest) == 3, line
        (v if tag == "v" else f).append([float(x) for x in rest] if tag == "v" else [int(x) for x in rest])
    return np.array(v, dtype=np.float64).reshape(-1, 3), np.array(f, dtype=np.int64).reshape(-1, 3)


def test_gmpm_output_surface(tmp_path):
    import __graft_entry__ as g
    g.build_host()
    density = 500.0
    d = run_gmpm(tmp_path / "surface", output_surface={"density": density})
    names = sorted(p.name for p in d.iterdir())
    assert [n for n in names if n.endswith(".obj")] == [f"surface_frame[{f}].obj" for f in range(FRAMES + 1)]
    assert len([n for n in names if n.endswith(".bgeo")]) == 2 * (FRAMES + 1) and not [n for n in names if n.endswith(".npy")]
    meshes = [parse_obj(d / f"surface_frame[{f}].obj") for f in range(FRAMES + 1)]
    for f, (v, faces) in enumerate(meshes):
        print(f"frame {f}: {len(v)} vertices, {len(faces)} faces")
        assert len(faces) > 20 and faces.min() == 1 and faces.max() == len(v)
        assert im.open_edges(v[faces - 1].astype(np.float32)) == 0
    # frame 0 is the grid of the set-up's P2G: an Engine with the driver's particles gives the same mesh
    eng = Engine(domain_bits=BITS, max_ppc=128)
    for mi, mod in enumerate(MODELS):
        xyz, _ = read_bgeo_attrs(d / f"model_id[{mi}]_frame[0].bgeo")
        mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
        eng.init_model(mat, xyz, mod["velocity"], **({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {}))
    eng.initial_setup()
    V, F = eng.isosurface(density=density)
    eng.close()
    v0, f0 = meshes[0]
    assert len(f0) == len(F) and np.array_equal(v0.astype(np.float32).view(np.uint32), V.view(np.uint32))
    same_multiset(v0.astype(np.float32)[f0 - 1], V[F], "frame 0")                             # (the order of the faces is the soup's: unspecified)
    with pytest.raises(subprocess.CalledProcessError):
        run_gmpm(tmp_path / "bad", output_surface={"density": 0})

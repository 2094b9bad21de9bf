"""Per-particle stress output (mpm_retrieve_stress / mpm_stress_totals, claymore_amd/csrc/mpm_readout.hpp) on the GPU.

The comparator is float64: the closed forms of tests/exact_models.py (fixed_corotated, sand, nacc) and the Tait pressure written here,
evaluated on the state mpm_retrieve_state returned from the same context at the same moment - F formed as the symmetric square root of b
(numpy.linalg.eigh), P F^T divided by `volume` and by J -, rows joined on the position bits.

Tolerance.  tests/test_parity_gpu.py holds the device stress functions to 1e-5 of volume * E against these closed forms on well-conditioned
input; dividing by volume * J turns that into |sigma_dev - sigma_exact| <= 1e-5 E / J_min per entry (J_min from the comparator).  The same
bound holds the pressure (a mean of three entries), three times it the von Mises stress (q <= sqrt(3/2) |dev sigma|), and J is held to 1e-5
relative.  The J-fluid has no Young's modulus: its bulk modulus takes E's place (the Tait pressure is bulk (J^-gamma - 1), evaluated through
the 1-ulp hardware log2 / exp2: a relative error of about (1 + gamma |ln J|) 2^-22 of bulk J^-gamma, far inside 1e-5 bulk)."""
import ctypes as C

import numpy as np
import pytest

import exact_models as X
from claymore_amd import _ffi, scenes
from claymore_amd.engine import build_engine

pytestmark = pytest.mark.gpu
BITS, DT, STEPS = 7, 1e-4, 60
N = 1 << BITS
NAMES = {_ffi.J_FLUID: "fluid", _ffi.FIXED_COROTATED: "fc", _ffi.SAND: "sand", _ffi.NACC: "nacc"}


# ---- scenes -----------------------------------------------------------------------------------------------------------------------------------
def jittered_box(lo, hi, seed, jitter=0.1, keep=None):
    """The lattice particles of nodes lo <= (i, j, k) < hi (cells), each moved by up to `jitter` cells per axis."""
    xyz = scenes.lattice_box(BITS, lo, hi).astype(np.float64)
    if keep is not None:
        xyz = xyz[keep(xyz * N)]
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(xyz + rng.uniform(-jitter, jitter, xyz.shape) / N, dtype=np.float32)


def params_of(material):
    return {"volume": scenes._vol(BITS), "rho": 1e3} if material in (_ffi.J_FLUID, _ffi.FIXED_COROTATED, _ffi.NACC) else {}


def wall_scene(material):
    """A 6 x 7 x 5-cell body whose lowest layer starts at the edge of the x = 0 wall zone (8 cells), thrown at it with 0.5 m/s, no gravity:
    after 60 substeps the layers next to the wall are compressed by some 10 %.
    NACC starts from log Jp = -0.03 (yield pressure p0 = bm sinh(xi 0.03) = 200 Pa, tensile tip p_min = -100 Pa) instead of the default
    -0.01 (67 / -33 Pa).  With the default, the rows that yield in shear all sit within 1 Pa of the tensile tip, where the yield surface's
    q(p) has a vertical tangent: p_trial = -bm / 2 (J^2 - 1), bm = 8.3 kPa, carries 1e-3 Pa of float32 rounding per operation, and the
    float64 comparator itself then moves by 0.01 Pa (a fifth of the bound) when its float32 input moves by half an ulp - not the
    well-conditioned input the bound is stated for.  The same scene through the CPU oracle (whose retrieve_state gives F), with the
    comparator's own perturbation test: from -0.03, 1540 rows inside the surface and 140 projected to the tensile tip (plastic, hardening),
    none changes its case (0 % left out; from -0.01 at 0.5 m/s: 13 %), max |b - I| 0.084, and half an ulp of input noise moves the
    comparator by 2e-4 Pa (0.003 of the bound).  compare() asserts that last condition on the state it is given."""
    params = params_of(material)
    if material == _ffi.NACC:
        params["log_jp0"] = -0.03
    return {"name": "wall_" + NAMES[material], "bits": BITS, "dt": DT, "config": {"max_ppc": 128, "gravity": 0.0},
            "models": [{"material": material, "xyz": jittered_box((8, 40, 40), (14, 47, 45), seed=11 + material), "v0": (-0.5, 0.0, 0.0),
                        "params": params}]}


def mixed_scene():
    """Model 0 (fixed-corotated, at rest, no gravity): a one-particle-thick slab at x in [41.7, 41.8] cells and, 3 cells beyond it, a target
    body from x = 45.2.  Both lie in the particle blocks x in [41.5, 45.5) cells, but share no grid node (the slab's stencils end at node 43,
    the target's start at node 44 and leave 0.7 cells for its sideways bulge), so the slab stays exactly undeformed while model 1 (sand, thrown down at 1 m/s, above the target only)
    compresses the target's upper layers."""
    slab = jittered_box((42, 38, 38), (43, 48, 48), seed=5, jitter=0.05, keep=lambda c: c[:, 0] < 42.0)
    target = jittered_box((45, 40, 40), (53, 46, 46), seed=6, jitter=0.05, keep=lambda c: c[:, 0] > 45.0)
    hammer = jittered_box((45, 46, 40), (53, 51, 46), seed=7, jitter=0.05, keep=lambda c: c[:, 0] > 45.0)
    return {"name": "mixed", "bits": BITS, "dt": DT, "config": {"max_ppc": 128, "gravity": 0.0},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": np.concatenate([slab, target]), "v0": (0.0, 0.0, 0.0), "params": params_of(_ffi.FIXED_COROTATED)},
                       {"material": _ffi.SAND, "xyz": hammer, "v0": (0.0, -1.0, 0.0), "params": {}}]}


SCENES = {"wall_" + NAMES[m]: (lambda m=m: wall_scene(m)) for m in NAMES}
SCENES["mixed"] = mixed_scene


# ---- the float64 comparator ---------------------------------------------------------------------------------------------------------------------
def lame(p):
    e, nu = np.float32(p.youngs_modulus), np.float32(p.poisson_ratio)
    return float(e / (2 * (1 + nu))), float(e * nu / ((1 + nu) * (1 - 2 * nu)))


def six(M):
    """{xx, yy, zz, xy, xz, yz} of symmetric (n, 3, 3) matrices"""
    return np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]], axis=1)


def nacc_args(p):
    mu, lam = lame(p)
    return (mu, lam, 1.0, p.beta, p.xi, p.msqr, p.hardening_on)


def root_of_b(st9):
    """F = the symmetric square root of b as column-major 9-vectors (float64), and det F; asserts that no row carries the reflection mark."""
    b = np.asarray(st9, dtype=np.float64).reshape(-1, 3, 3)
    assert np.all(np.asarray(st9)[:, 0] > 0), "a reflected F is marked in this state"
    lam, U = np.linalg.eigh(b)
    assert lam.min() > 0
    F = np.einsum("nij,nj,nkj->nik", U, np.sqrt(lam), U)
    return X.to_flat(F), np.sqrt(lam.prod(axis=1))


def comparator(material, p, st9, lj):
    """(sigma6, J, modulus, keep, moved) in float64 for the rows of a retrieve_state; keep: rows whose NACC case is stable (all rows
    otherwise); moved (NACC, else 0): how far the comparator's own sigma moves when its float32 input b moves by half an ulp."""
    n = st9.shape[0]
    keep = np.ones(n, dtype=bool)
    moved = np.zeros(n)
    if material == _ffi.J_FLUID:
        J = st9[:, 0].astype(np.float64)
        pr = float(np.float32(p.bulk)) * (J ** -float(np.float32(p.gamma)) - 1.0)
        sig = np.zeros((n, 6))
        sig[:, :3] = -pr[:, None]
        return sig, J, float(p.bulk), keep, moved
    F9, J = root_of_b(st9)
    mu, lam = lame(p)
    if material == _ffi.FIXED_COROTATED:
        PF = X.fixed_corotated(F9, mu, lam, 1.0)
    elif material == _ffi.SAND:
        Fn, PF, _ = X.sand(F9, lj, mu, lam, 1.0, p.cohesion, p.beta, p.yield_surface, p.volume_correction)
        J = np.linalg.det(X.to_mats(Fn))
    else:
        Fn, PF, _, case = X.nacc(F9, lj, *nacc_args(p))
        J = np.linalg.det(X.to_mats(Fn))
        rng = np.random.default_rng(1)
        for _ in range(4):       # the perturbation test_parity_gpu.py uses for the model's discontinuous case selection
            keep &= X.nacc(F9 * (1 + 3e-6 * rng.standard_normal(F9.shape)), lj, *nacc_args(p))[3] == case
        sig = six(X.to_mats(PF)) / J[:, None]
        for _ in range(4):       # the conditioning of the input: b (1 +- 2^-24) entry by entry, symmetric
            e = np.triu(rng.choice([-1.0, 1.0], size=(n, 3, 3)))
            e = (e + np.triu(e, 1).transpose(0, 2, 1)).reshape(n, 9)
            F2, PF2, _, _ = X.nacc(root_of_b(st9.astype(np.float64) * (1 + 2.0 ** -24 * e))[0], lj, *nacc_args(p))
            moved = np.maximum(moved, np.abs(six(X.to_mats(PF2)) / np.linalg.det(X.to_mats(F2))[:, None] - sig).max(axis=1))
    return six(X.to_mats(PF)) / J[:, None], J, float(p.youngs_modulus), keep, moved


def invariants(sig):
    pr = -sig[:, :3].sum(axis=1) / 3.0
    dev = sig.copy()
    dev[:, :3] += pr[:, None]
    q = np.sqrt(1.5 * ((dev[:, :3] ** 2).sum(axis=1) + 2.0 * (dev[:, 3:] ** 2).sum(axis=1)))
    return pr, q


def join(xa, xb):
    """Row i of a = row idx[i] of b, joined on the position bits (asserts the two hold the same distinct positions)."""
    ka, kb = [np.ascontiguousarray(x, dtype=np.float32).view([("x", "u4"), ("y", "u4"), ("z", "u4")]).ravel() for x in (xa, xb)]
    oa, ob = np.argsort(ka, order=("x", "y", "z")), np.argsort(kb, order=("x", "y", "z"))
    assert ka.shape == kb.shape and np.array_equal(ka[oa], kb[ob]), "the two readouts do not hold the same positions"
    assert np.all(ka[oa][1:] != ka[oa][:-1]), "positions are not distinct"
    idx = np.empty(ka.size, dtype=np.int64)
    idx[oa] = ob
    return idx


def compare(tag, material, p, state, stress, rows=None):
    """The stress rows `rows` (default: all) against the comparator on `state`; prints every figure before it asserts.  Returns the comparator's
    (sigma6, J, q, keep) in the order of the stress readout."""
    xs, st9, lj = state
    x, s6, sc = stress
    idx = join(x, xs) if rows is None else rows
    sig, J, modulus, keep, moved = comparator(material, p, st9[idx], lj[idx])
    assert np.array_equal(x, xs[idx])                        # the position bits of mpm_retrieve_state
    pr, q = invariants(sig)
    left_out = float(np.mean(~keep))
    bound = 1e-5 * modulus / np.abs(J[keep]).min()
    ds = np.abs(s6[keep] - sig[keep]).max()
    dp = np.abs(sc[keep, 1] - pr[keep]).max()
    dq = np.abs(sc[keep, 2] - q[keep]).max()
    dj = np.abs(sc[keep, 0] / J[keep] - 1.0).max()
    print(f"{tag}: rows {x.shape[0]} left out {left_out:.4f} half an ulp of b moves the comparator by {moved[keep].max():.3g} | bound {bound:.4g} max |sigma| {np.abs(sig).max():.4g} | d sigma {ds:.3g} d p {dp:.3g} d q {dq:.3g} (3x) d J {dj:.3g}")
    assert np.all(np.isfinite(s6)) and np.all(np.isfinite(sc))
    assert left_out <= 0.05, left_out                        # (NACC only) a condition on the scene, not a measurement
    # (NACC only) the input is well conditioned, as the bound presumes: the device reaches p_trial through a dozen float32 roundings; a state
    # on which half an ulp of the input alone moves the exact answer by a quarter of the bound cannot be held to it by any float32 evaluation
    assert moved[keep].max() <= 0.25 * bound, (moved[keep].max(), bound)
    assert ds <= bound and dp <= bound and dq <= 3 * bound and dj <= 1e-5, (ds, dp, dq, dj, bound)
    return sig, J, q, keep


class Run:
    """A scene after STEPS substeps: the engine (kept open) and, per model, retrieve_state and retrieve_stress taken at that moment."""

    def __init__(self, sc):
        self.sc = sc
        self.eng = build_engine(sc)
        self.eng.initial_setup()
        self.eng.run_fixed(STEPS, sc["dt"])
        nm = len(sc["models"])
        self.state = [self.eng.retrieve_state(m) for m in range(nm)]
        self.stress = [self.eng.retrieve_stress(m) for m in range(nm)]
        self.params = [self.eng.models[m]["params"] for m in range(nm)]
        self.material = [mod["material"] for mod in sc["models"]]


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Run(SCENES[name]())
        return cache[name]
    yield get
    for r in cache.values():
        r.eng.close()


def block_sizes(xyz):
    """Particles per particle block by the kernels' rule: block key (N - 2) >> 2 of the nearest node N = lround(x / dx) per axis."""
    node = np.floor(xyz.astype(np.float32) * np.float32(N) + np.float32(0.5)).astype(np.int64)
    key = (node - 2) >> 2
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return inv.ravel(), cnt


# ---- all four materials, deformed, after 60 substeps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", sorted(NAMES))
def test_stress_of_a_deformed_body_against_the_float64_closed_form(runs, material):
    """A body thrown at the wall zone: every row of the readout against the comparator on the state read at the same moment."""
    run = runs("wall_" + NAMES[material])
    p, (xs, st9, lj), (x, s6, sc) = run.params[0], run.state[0], run.stress[0]
    cnt = run.eng.counts()
    assert x.shape[0] == xs.shape[0] == cnt.particles[0] == run.sc["models"][0]["xyz"].shape[0]
    # the state is not trivial (a zero-stress scene would pass vacuously), and the walk takes its awkward paths
    if material == _ffi.J_FLUID:
        assert np.abs(st9[:, 0] - 1.0).max() > 1e-3
    else:
        assert np.abs(st9.astype(np.float64) - np.eye(3).reshape(9)).max() > 1e-2
        assert sc[:, 2].max() > 1e-3 * p.youngs_modulus
    _, sizes = block_sizes(xs)
    assert sizes.size == cnt.particle_blocks and sizes.sum() == cnt.particles[0]
    assert np.any(sizes % 64 != 0) and np.any(sizes > 256), sizes       # a ragged last wave; a second trip of the 256-lane walk
    compare(NAMES[material], material, p, run.state[0], run.stress[0])


# ---- undeformed and deformed particles in one particle block ---------------------------------------------------------------------------------------
def test_undeformed_and_deformed_particles_share_blocks_and_two_models_of_different_materials(runs):
    """The early exit of the stress functions is a wave vote: a resting slab (b = I) shares particle blocks with a compressed body.  The
    undeformed particles read sigma = 0 (within 1e-7 E), the deformed ones match the comparator; the sand model of the same context is read
    with its own index."""
    run = runs("mixed")
    cnt = run.eng.counts()
    assert [s[0].shape[0] for s in run.stress] == [cnt.particles[0], cnt.particles[1]] == [m["xyz"].shape[0] for m in run.sc["models"]]
    p = run.params[0]
    x, s6, sc = run.stress[0]
    idx = join(x, run.state[0][0])
    st9 = run.state[0][1][idx]
    rest = np.abs(st9.astype(np.float64) - np.eye(3).reshape(9)).max(axis=1) <= 1e-7
    block, sizes = block_sizes(x)
    shared = np.intersect1d(block[rest], block[~rest & (sc[:, 2] > 1e-3 * p.youngs_modulus)])
    in_shared = np.isin(block, shared)
    print(f"mixed: {rest.sum()} particles at rest, {(~rest).sum()} deformed, {shared.size} blocks hold both ({(rest & in_shared).sum()} / {(~rest & in_shared).sum()})")
    assert rest.sum() >= 300 and shared.size >= 2 and (rest & in_shared).sum() >= 64 and (~rest & in_shared).sum() >= 32
    assert np.abs(s6[rest]).max() <= 1e-7 * p.youngs_modulus and np.abs(sc[rest, 1:]).max() <= 1e-7 * p.youngs_modulus
    assert np.abs(sc[rest, 0] - 1.0).max() <= 1e-6
    for m in range(2):
        compare(f"mixed model {m}", run.material[m], run.params[m], run.state[m], run.stress[m])
    assert np.abs(run.state[1][1].astype(np.float64) - np.eye(3).reshape(9)).max() > 1e-2


# ---- the readout leaves the particles alone --------------------------------------------------------------------------------------------------------
def sparse_scene():
    """NACC, one particle every fourth cell (2 x 4 x 4 = 32 particles at quarter-cell positions), thrown at the x = 0 wall zone without
    gravity; the first layer starts at the zone's edge (x = 8.25 cells: nodes 7 to 9), and the wall compresses it (CPU oracle: max |b - I|
    0.098, log Jp from -0.01 to -0.17 after 60 substeps: projected and hardened substep after substep; an isolated sand particle only
    dilates there, its b stays the identity).  The 3 x 3 x 3 stencils of
    two particles share no node, now or after the 0.5 cells the particles travel, so every grid node receives one contribution per substep
    and the float atomics of P2G have nothing to reorder: the engine is deterministic on such a scene (sparse_scene of
    tests/test_collision_clock_gpu.py; on a body two runs of one scene differ in the last bits), which a bit-for-bit comparison of two
    contexts needs."""
    cells = np.stack(np.meshgrid([8.25, 12.25], 40.25 + 4.0 * np.arange(4), 40.25 + 4.0 * np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3)
    return {"name": "sparse", "bits": BITS, "dt": DT, "config": {"max_ppc": 128, "gravity": 0.0},
            "models": [{"material": _ffi.NACC, "xyz": np.ascontiguousarray(cells / N, dtype=np.float32), "v0": (-0.5, 0.0, 0.0),
                        "params": params_of(_ffi.NACC)}]}


def test_state_is_untouched_and_the_run_goes_on_bit_identical():
    """NACC: a model whose stress function projects b and log Jp - which the readout must not store.  Context a is read out (stress and
    totals), b and c never are; b and c have to agree first (else the scene is not deterministic and there is nothing to compare)."""
    sc = sparse_scene()
    a, b, c = build_engine(sc), build_engine(sc), build_engine(sc)
    for e in (a, b, c):
        e.initial_setup()
        e.run_fixed(STEPS, DT)
    before, saved = a.retrieve_state(0), a.save_checkpoint().copy()
    assert np.abs(before[1].astype(np.float64) - np.eye(3).reshape(9)).max() > 1e-3      # the wall has deformed the first layer
    a.retrieve_stress(0)
    a.stress_totals()
    after = a.retrieve_state(0)
    assert np.array_equal(saved, a.save_checkpoint())                     # bins, lists, grid: every byte a checkpoint holds
    idx = join(before[0], after[0])
    assert all(np.array_equal(u.view(np.uint32), v[idx].view(np.uint32)) for u, v in zip(before, after))
    for e in (a, b, c):
        e.run_fixed(10, DT)
    xa, xb, xc = a.retrieve_positions(0), b.retrieve_positions(0), c.retrieve_positions(0)
    join(xb, xc)                                                          # the control: two contexts that never read stress agree bit for bit
    join(xa, xb)                                                          # and so does the one that did
    for e in (a, b, c):
        e.close()


# ---- the C interface: capacity, NULL columns, errors -------------------------------------------------------------------------------------------------
def test_capacity_null_columns_and_error_codes(runs):
    run = runs("wall_fc")
    api, ctx = run.eng.api, run.eng.ctx
    xs = run.state[0][0]
    count = xs.shape[0]
    k = count - 7
    x, s6, sc = np.full((k, 3), np.nan, np.float32), np.full((k, 6), np.nan, np.float32), np.full((k, 3), np.nan, np.float32)
    pX, pS, pC = (a.ctypes.data_as(C.c_void_p) for a in (x, s6, sc))
    n = C.c_size_t(k)
    assert api.retrieve_stress(ctx, 0, pX, pS, pC, C.byref(n)) == _ffi.MPM_ERR_CAPACITY
    assert n.value == k
    row_of = {r.tobytes(): i for i, r in enumerate(xs)}
    rows = np.array([row_of[r.tobytes()] for r in x])
    assert np.unique(rows).size == k and np.array_equal(xs[rows], x)       # k distinct particles of the state readout
    compare("capacity", run.material[0], run.params[0], run.state[0], (x, s6, sc), rows=rows)
    full = run.stress[0]
    idx = join(full[0], xs)
    for cols in ((None, pC), (pS, None), (None, None)):
        x2, s2, c2 = np.empty((count, 3), np.float32), np.full((count, 6), np.nan, np.float32), np.full((count, 3), np.nan, np.float32)
        n = C.c_size_t(count)
        args = [a.ctypes.data_as(C.c_void_p) if c is not None else None for a, c in zip((s2, c2), cols)]
        assert api.retrieve_stress(ctx, 0, x2.ctypes.data_as(C.c_void_p), *args, C.byref(n)) == _ffi.MPM_OK and n.value == count
        j = join(x2, xs)
        back = np.empty(count, dtype=np.int64)
        back[idx] = np.arange(count)                                       # state row -> row of the full stress readout
        if cols[0] is not None:
            assert np.array_equal(s2.view(np.uint32), full[1][back[j]].view(np.uint32))
        else:
            assert np.all(np.isnan(s2))
        if cols[1] is not None:
            assert np.array_equal(c2.view(np.uint32), full[2][back[j]].view(np.uint32))
        else:
            assert np.all(np.isnan(c2))
    n = C.c_size_t(count)
    out = (C.c_double * 8)()
    for bad in (-1, 1):
        assert api.retrieve_stress(ctx, bad, pX, pS, pC, C.byref(n)) == _ffi.MPM_ERR_INVALID
    assert api.retrieve_stress(ctx, 0, None, pS, pC, C.byref(n)) == _ffi.MPM_ERR_INVALID
    assert api.retrieve_stress(ctx, 0, pX, pS, pC, None) == _ffi.MPM_ERR_INVALID
    assert api.stress_totals(ctx, -2, out) == _ffi.MPM_ERR_INVALID and api.stress_totals(ctx, 1, out) == _ffi.MPM_ERR_INVALID
    assert api.stress_totals(ctx, 0, None) == _ffi.MPM_ERR_INVALID
    fresh = build_engine(wall_scene(_ffi.FIXED_COROTATED))
    assert api.retrieve_stress(fresh.ctx, 0, pX, pS, pC, C.byref(n)) == _ffi.MPM_ERR_NOT_READY
    assert api.stress_totals(fresh.ctx, 0, out) == _ffi.MPM_ERR_NOT_READY
    fresh.close()


# ---- totals ---------------------------------------------------------------------------------------------------------------------------------------------
def host_totals(p, stress):
    """{sum V0 tau (6), sum V0 |tau| (6), max q} of a per-particle readout, summed in float64 (tau = sigma J)."""
    _, s6, sc = stress
    tau = s6.astype(np.float64) * sc[:, :1].astype(np.float64) * float(np.float32(p.volume))
    return tau.sum(axis=0), np.abs(tau).sum(axis=0), sc[:, 2].max()


@pytest.mark.parametrize("scene", ["wall_fluid", "wall_nacc", "mixed"])
def test_totals_equal_the_per_particle_readout(runs, scene):
    run = runs(scene)
    nm = len(run.material)
    per_model = []
    for m in range(nm):
        t = run.eng.stress_totals(m)
        want, scale, qmax = host_totals(run.params[m], run.stress[m])
        err = np.abs(t["stress_integral"] - want).max()
        print(f"{scene} model {m}: integral {t['stress_integral']}, |difference| {err:.3g} of {scale.max():.3g}")
        assert t["count"] == run.stress[m][0].shape[0]
        assert err <= 1e-6 * scale.max(), (err, scale.max())
        assert np.float32(t["max_von_mises"]).view(np.uint32) == np.float32(qmax).view(np.uint32) and t["max_von_mises"] == float(qmax)
        per_model.append(t)
    both = run.eng.stress_totals()
    assert both["count"] == sum(t["count"] for t in per_model)
    assert both["max_von_mises"] == max(t["max_von_mises"] for t in per_model)
    total = sum(t["stress_integral"] for t in per_model)
    scale = sum(host_totals(run.params[m], run.stress[m])[1] for m in range(nm)).max()
    assert np.abs(both["stress_integral"] - total).max() <= 1e-6 * scale


# ---- a grouped context -------------------------------------------------------------------------------------------------------------------------------------
def test_per_rank_readout_of_a_grouped_context():
    """Two ranks of an in-process group on one device, after one mpm_group_run_fixed: each rank's retrieve_stress against that rank's own
    retrieve_state (the single-context call, which a grouped context does not refuse)."""
    from test_group_velocity_gpu import collision, run_group
    sc = collision()

    def script(sim):
        sim.initial_setup()
        sim.run_fixed(30, 1e-4)
        nm = len(sim.eng.models)
        return ([sim.eng.retrieve_state(m) for m in range(nm)], [sim.retrieve_stress(m) for m in range(nm)],
                [sim.stress_totals(m) for m in range(nm)], [sim.eng.models[m]["params"] for m in range(nm)])

    deformed = 0
    for r, (state, stress, totals, params) in enumerate(run_group(sc, 2, script)):
        for m in range(len(state)):
            if state[m][0].shape[0] == 0:
                continue
            compare(f"rank {r} model {m}", _ffi.FIXED_COROTATED, params[m], state[m], stress[m])
            assert totals[m]["count"] == stress[m][0].shape[0] and totals[m]["max_von_mises"] == float(stress[m][2][:, 2].max())
            deformed += int(np.sum(stress[m][2][:, 2] > 1e-3 * params[m].youngs_modulus))
    assert deformed > 100

"""One particle's G2P2G substep in float64 (plain numpy), the scenes and the node-velocity field of tests/test_g2p2g_blocks_gpu.py.

step() restates Projects/GMPM/mgmpm_kernels.cuh:772-905 with the material bodies :470-663 in terms of b = F F^T, the state the engine
carries (claymore_amd/csrc/mpm_g2p2g.hpp): it forms F = sqrt(b) - symmetric, the smallest stretch negated for a reflected particle -,
pushes it forward with G = I + dt grad v and hands G F to the closed forms of tests/exact_models.py.  Every model on the path is
isotropic, so the rotation that sqrt(b) drops reaches no output.  tests/test_g2p2g_model_cpu.py judges it against the oracle's
mpmo_fn_particle_step, which tests/test_oracle_golden.py ties to the reference's own statements; the deviations found there are the
yardstick Y below.

Geometry (all distances in cells, x / dx, exact in float32 for dx a power of two): node = lround(x / dx), stencil base = node - 1, particle
block key = (node - 2) / 4: block k owns x / dx in [4k + 1.5, 4k + 5.5) per axis, and its 8^3 node cube starts at node 4k (it spans
the grid blocks k and k + 1).  A stencil base has cube coordinate ((base - 1) & 3) + 1 in 1..4; after the move it may be 0..5, anything
else is discarded (:877-885).

Test infrastructure only."""
import ctypes as C
import os

import numpy as np

import exact_models as em
from claymore_amd import _ffi

J_FLUID, FC, SAND, NACC = _ffi.J_FLUID, _ffi.FIXED_COROTATED, _ffi.SAND, _ffi.NACC
MATERIALS = (J_FLUID, FC, SAND, NACC)
NAMES = {J_FLUID: "jfluid", FC: "fc", SAND: "sand", NACC: "nacc"}
BITS = 6
MAX_PPC = 16                                   # 1024 particles per block: two 512-record chunks and the merged tail
DT = float(np.float32(1e-4))
NEW_DT = float(np.float32(7.5e-5))             # different from DT on purpose: :850 takes new_dt, the rest dt
TIERS = {"rest": (0.5, 0.5), "flow": (20.0, 5.0), "fast": (60.0, 15.0), "torn": (200.0, 40.0)}      # drift / noise, m/s
DRIFT_DIR = np.array([0.8, -0.36, 0.48])       # a unit vector with no two components alike
SITES = [(x, y, z) for x in (3, 6, 9, 12) for y in (3, 6, 9, 12) for z in (3, 6, 9, 12)]     # keys three apart: disjoint node cubes, clear of the walls
BLOCK_SIZES = (1, 2, 3, 64, 65, 127, 128, 129, 511, 512, 513, 768, 769, 1024)
OFFS = np.array([(i, j, k) for i in range(3) for j in range(3) for k in range(3)])           # stencil offsets, row-major (s = 9 i + 3 j + k)

# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
# The project's bounds for the undeformed one-particle rows (tests/test_parity_gpu.py): position relative, b relative to max(1, |b|), log Jp
# absolute, J relative to max(1, |J|), the 27 x 4 stencil relative to its largest mass / momentum entry.
EXISTING = {"pos": 1e-6, "b": 1.2e-5, "logjp": 6e-6, "J": 2e-6, "stencil": 1e-5}
# Y: what the float32 oracle (the reference's arithmetic) deviates from this model by, per quantity, tier and material, on the generated
# scenes (all of them) and on the golden rows of arenas 0 .. 2 ("golden").  Measured by tests/test_g2p2g_model_cpu.py, which asserts that
# these constants are what it measures (to the three digits written) and that profiles/g2p2g_blocks_yardstick.txt holds the same.
Y = {
    ("b", "fast", "fc"): 3.75e-07, ("pos", "fast", "fc"): 5.91e-08, ("stencil", "fast", "fc"): 7.35e-06,
    ("b", "flow", "fc"): 3.68e-07, ("pos", "flow", "fc"): 5.87e-08, ("stencil", "flow", "fc"): 7.34e-06,
    ("b", "golden", "fc"): 2.82e-07, ("pos", "golden", "fc"): 3.91e-08, ("stencil", "golden", "fc"): 1.15e-05,
    ("b", "golden_violent", "fc"): 1.19e-06, ("pos", "golden_violent", "fc"): 3.91e-08, ("stencil", "golden_violent", "fc"): 1.02e-05,
    ("b", "rest", "fc"): 3.93e-07, ("pos", "rest", "fc"): 5.9e-08, ("stencil", "rest", "fc"): 6.81e-06,
    ("b", "torn", "fc"): 7.35e-07, ("pos", "torn", "fc"): 6.71e-08, ("stencil", "torn", "fc"): 8.08e-06,
    ("J", "fast", "jfluid"): 1.42e-07, ("pos", "fast", "jfluid"): 5.91e-08, ("stencil", "fast", "jfluid"): 7.27e-06,
    ("J", "flow", "jfluid"): 7.8e-08, ("pos", "flow", "jfluid"): 5.87e-08, ("stencil", "flow", "jfluid"): 7.35e-06,
    ("J", "golden", "jfluid"): 5.49e-08, ("pos", "golden", "jfluid"): 3.9e-08, ("stencil", "golden", "jfluid"): 1.33e-05,
    ("J", "golden_violent", "jfluid"): 4.17e-07, ("pos", "golden_violent", "jfluid"): 3.85e-08, ("stencil", "golden_violent", "jfluid"): 1.47e-05,
    ("J", "rest", "jfluid"): 5.94e-08, ("pos", "rest", "jfluid"): 5.9e-08, ("stencil", "rest", "jfluid"): 8.56e-06,
    ("J", "torn", "jfluid"): 3.77e-07, ("pos", "torn", "jfluid"): 6.71e-08, ("stencil", "torn", "jfluid"): 8.05e-06,
    ("b", "fast", "nacc"): 2.42e-05, ("logjp", "fast", "nacc"): 2.45e-06, ("pos", "fast", "nacc"): 5.91e-08,
    ("stencil", "fast", "nacc"): 7.27e-06, ("b", "flow", "nacc"): 3.22e-05, ("logjp", "flow", "nacc"): 2.52e-06,
    ("pos", "flow", "nacc"): 5.87e-08, ("stencil", "flow", "nacc"): 7.34e-06, ("b", "golden", "nacc"): 7.15e-06,
    ("logjp", "golden", "nacc"): 1.85e-06, ("pos", "golden", "nacc"): 3.9e-08, ("stencil", "golden", "nacc"): 1.28e-05,
    ("b", "golden_violent", "nacc"): 1.3e-06, ("logjp", "golden_violent", "nacc"): 8.23e-06, ("pos", "golden_violent", "nacc"): 3.92e-08,
    ("stencil", "golden_violent", "nacc"): 1.25e-05, ("b", "rest", "nacc"): 3.55e-05, ("logjp", "rest", "nacc"): 2.43e-06,
    ("pos", "rest", "nacc"): 5.9e-08, ("stencil", "rest", "nacc"): 6.81e-06, ("b", "torn", "nacc"): 2.09e-05,
    ("logjp", "torn", "nacc"): 2.6e-06, ("pos", "torn", "nacc"): 6.71e-08, ("stencil", "torn", "nacc"): 8.13e-06,
    ("b", "fast", "sand"): 7.72e-06, ("logjp", "fast", "sand"): 2.26e-06, ("pos", "fast", "sand"): 5.91e-08,
    ("stencil", "fast", "sand"): 7.28e-06, ("b", "flow", "sand"): 7.74e-06, ("logjp", "flow", "sand"): 2.41e-06,
    ("pos", "flow", "sand"): 5.87e-08, ("stencil", "flow", "sand"): 7.34e-06, ("b", "golden", "sand"): 4.16e-06,
    ("logjp", "golden", "sand"): 1.23e-06, ("pos", "golden", "sand"): 3.87e-08, ("stencil", "golden", "sand"): 1.16e-05,
    ("b", "golden_violent", "sand"): 3.67e-06, ("logjp", "golden_violent", "sand"): 1.36e-06, ("pos", "golden_violent", "sand"): 3.89e-08,
    ("stencil", "golden_violent", "sand"): 1.19e-05, ("b", "rest", "sand"): 7.14e-06, ("logjp", "rest", "sand"): 2.34e-06,
    ("pos", "rest", "sand"): 5.9e-08, ("stencil", "rest", "sand"): 6.81e-06, ("b", "torn", "sand"): 6.89e-06,
    ("logjp", "torn", "sand"): 2.3e-06, ("pos", "torn", "sand"): 6.71e-08, ("stencil", "torn", "sand"): 8.09e-06,
}


def bound(quantity, tier, material):
    """max(the project's bound, 3 x the reference side's own deviation from the truth)"""
    return max(EXISTING[quantity], 3.0 * Y[(quantity, tier, NAMES[material])])


# ---- materials ---------------------------------------------------------------------------------------------------------------------------
def material_overrides(material, bits=BITS):
    """The parameters of the scenes (those of the golden rows, tests/golden/g16_params.f32, with the particle volume of `bits`)."""
    dx = 0.5 ** bits
    vol = float(np.float32(dx * dx * dx / 8.0))
    if material == J_FLUID:
        return dict(rho=1e3, volume=vol, bulk=4e4, gamma=7.15, viscosity=0.01)
    p = dict(rho=1e3, volume=vol, youngs_modulus=5e3, poisson_ratio=0.4)
    if material == SAND:
        p.update(cohesion=0.0, beta=1.0, yield_surface=0.3265986442565918, volume_correction=1)
    if material == NACC:
        p.update(beta=0.5, xi=0.8, msqr=3.423772096633911, hardening_on=1)
    return p


def constants(material, overrides):
    """What step() needs of a material: the float32 parameters as float64; mass = volume * rho as the float32 product both engines form."""
    f = {k: float(np.float32(v)) for k, v in overrides.items()}
    c = dict(material=material, volume=f["volume"], mass=float(np.float32(overrides["volume"]) * np.float32(overrides["rho"])))
    if material == J_FLUID:
        c.update(bulk=f["bulk"], gamma=f["gamma"], viscosity=f["viscosity"])
        return c
    E, nu = f["youngs_modulus"], f["poisson_ratio"]
    c.update(mu=E / (2 * (1 + nu)), lam=E * nu / ((1 + nu) * (1 - 2 * nu)))
    if material == SAND:
        c.update(cohesion=f["cohesion"], beta=f["beta"], yield_surface=f["yield_surface"], volume_correction=int(overrides["volume_correction"]))
    if material == NACC:
        c.update(beta=f["beta"], xi=f["xi"], msqr=f["msqr"], hardening_on=int(overrides["hardening_on"]))
    return c


# ---- the node-velocity field -------------------------------------------------------------------------------------------------------------
def _mix(x):
    m = np.uint64(0xFFFFFFFF)
    x = x & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def field(nodes, tier, seed=0):
    """v(i, j, k) in m/s, float32 (..., 3): a uniform drift plus per-node noise from an integer hash of the node index - a pure function of
    the node, so every grid block that holds a node holds the same value, whatever the order anything is built in."""
    drift, noise = TIERS[tier]
    n = np.asarray(nodes).astype(np.int64).astype(np.uint64)
    h0 = (n[..., 0] * np.uint64(73856093)) ^ (n[..., 1] * np.uint64(19349663)) ^ (n[..., 2] * np.uint64(83492791))
    out = np.empty(n.shape[:-1] + (3,), np.float32)
    for c in range(3):
        h = _mix(_mix(h0 + np.uint64((seed * 0x9E3779B1 + c * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF)))
        u = h.astype(np.float64) / 2.0 ** 31 - 1.0                 # [-1, 1)
        out[..., c] = (drift * DRIFT_DIR[c] + noise * u).astype(np.float32)
    return out


def grid_of(keys, tier, seed=0):
    """Channels 1 .. 3 of the grid blocks `keys` (n, 3): (n, 3, 64) float32, cell = 16 x + 4 y + z."""
    keys = np.asarray(keys).astype(np.int64)
    cell = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)])
    v = field(4 * keys[:, None, :] + cell[None, :, :], tier, seed)     # (n, 64, 3)
    return np.ascontiguousarray(v.transpose(0, 2, 1))


def cube_of(key, tier, seed=0):
    """The velocity arena of particle block `key` as the reference holds it: (3, 8, 8, 8) float32, node 4 key + (i, j, k)."""
    ijk = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1)
    return np.ascontiguousarray(field(4 * np.asarray(key)[None, None, None, :] + ijk, tier, seed).transpose(3, 0, 1, 2))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def lround_cells(p):
    return np.floor(np.asarray(p, np.float64) + 0.5).astype(np.int64)          # (positions are positive: half away from zero = half up)


def block_keys(pos_cells):
    return (lround_cells(pos_cells) - 2) // 4


def stencil_base(pos_cells):
    return lround_cells(pos_cells) - 1


def _weights(fd):
    """utility_funcs.hpp:10-19 in cells: (n, 3 axes, 3 offsets)"""
    return np.stack([0.5 * (1.5 - fd) ** 2, 0.75 - (fd - 1.0) ** 2, 0.5 * (fd - 0.5) ** 2], axis=-1)


def b6_to_mats(b6):
    b = np.asarray(b6, np.float64)
    return np.stack([np.stack([b[:, 0], b[:, 3], b[:, 4]], -1), np.stack([b[:, 3], b[:, 1], b[:, 5]], -1), np.stack([b[:, 4], b[:, 5], b[:, 2]], -1)], 1)


def mats_to_b6(B):
    return np.stack([B[:, 0, 0], B[:, 1, 1], B[:, 2, 2], B[:, 1, 0], B[:, 2, 0], B[:, 2, 1]], axis=1)


def sqrt_b(b6, reflected):
    """F = sqrt(b), symmetric; a reflected particle gets its smallest stretch negated (svd.cuh:590-770 puts the sign there)."""
    lam, U = np.linalg.eigh(b6_to_mats(b6))                   # ascending
    s = np.sqrt(lam)
    s[:, 0] = np.where(np.asarray(reflected, bool), -s[:, 0], s[:, 0])
    return np.einsum("nij,nj,nkj->nik", U, s, U)


def _label(material, c, F9, logjp):
    if material == SAND:
        return em.sand_branch(F9, logjp, c["mu"], c["lam"], c["cohesion"], c["yield_surface"])
    if material == NACC:
        return em.nacc(F9, logjp, c["mu"], c["lam"], c["volume"], c["beta"], c["xi"], c["msqr"], c["hardening_on"])[3]
    return np.zeros(F9.shape[0], np.int64)


def step(c, pos_cells, vn, b6=None, reflected=None, logjp=None, J=None, dt=DT, new_dt=NEW_DT, bits=BITS):
    """One substep of n particles.  c: constants(); pos_cells (n, 3); vn (n, 27, 3): the velocities of the nodes base + OFFS[s] in m/s; b6 (n, 6)
    {00, 11, 22, 10, 20, 21} with `reflected` (n,), logjp (n,) - or J (n,) for the fluid.  Everything is taken as given (float32 inputs become
    float64) and computed in float64.  Returns a dict: base, pos (cells), new_base, dirtag, narena, discarded, b6 / reflected / logjp (or J) after
    the step, nodes (n, 27, 3) and stencil (n, 27, 4) = {m, mvx, mvy, mvz} the particle adds to them (zero where discarded), label (sand branch /
    NACC case), unstable (the label changes when the trial F is scaled by 1 +- 1e-5), finite."""
    material = c["material"]
    p = np.asarray(pos_cells, np.float64).reshape(-1, 3)
    n = p.shape[0]
    vn = np.asarray(vn, np.float64).reshape(n, 27, 3)
    dx = 0.5 ** bits
    d_inv = 4.0 / (dx * dx)
    mass = c["mass"]
    base = stencil_base(p)
    fd = p - base
    w = _weights(fd)
    W = (w[:, 0, :, None, None] * w[:, 1, None, :, None] * w[:, 2, None, None, :]).reshape(n, 27)
    xixp = (OFFS[None, :, :] - fd[:, None, :]) * dx                                  # (n, 27, 3) world units
    vel = np.einsum("ns,nsr->nr", W, vn)
    A = np.einsum("ns,nsr,nsc->nrc", W, vn, xixp)                                    # A[r, c] = sum W v_r (x_i - x_p)_c
    pos = p + vel * (dt / dx)
    out = dict(base=base, pos=pos, vel=vel, A=A)
    with np.errstate(all="ignore"):
        if material == J_FLUID:
            Jn, st9 = em.jfluid(J, em.to_flat(A), dt, d_inv, c["volume"], c["bulk"], c["gamma"], c["viscosity"])
            PF = em.to_mats(st9)
            out.update(J=Jn, label=np.zeros(n, np.int64), unstable=np.zeros(n, bool))
        else:
            G = np.eye(3)[None] + dt * d_inv * A
            Ft = G @ sqrt_b(b6, reflected)
            F9 = em.to_flat(Ft)
            lj = np.zeros(n) if logjp is None else np.asarray(logjp, np.float64)
            if material == FC:
                Fn9, PF9, ljn = F9, em.fixed_corotated(F9, c["mu"], c["lam"], c["volume"]), lj
            elif material == SAND:
                Fn9, PF9, ljn = em.sand(F9, lj, c["mu"], c["lam"], c["volume"], c["cohesion"], c["beta"], c["yield_surface"], c["volume_correction"])
            else:
                Fn9, PF9, ljn, _ = em.nacc(F9, lj, c["mu"], c["lam"], c["volume"], c["beta"], c["xi"], c["msqr"], c["hardening_on"])
            Fn, PF = em.to_mats(Fn9), em.to_mats(PF9)
            lab = _label(material, c, F9, lj)
            out.update(b6=mats_to_b6(Fn @ Fn.transpose(0, 2, 1)), reflected=np.linalg.det(Fn) < 0, logjp=ljn, label=lab,
                       unstable=(_label(material, c, F9 * (1 + 1e-5), lj) != lab) | (_label(material, c, F9 * (1 - 1e-5), lj) != lab))
        Cm = (A * mass - PF * new_dt) * d_inv                                        # :850
        nbase = stencil_base(np.where(np.isfinite(pos), pos, 0.0))
        nfd = pos - nbase
        arena = ((base - 1) & 3) + 1
        narena = arena + (nbase - base)
        disc = ((narena < 0) | (narena > 5)).any(axis=1)                             # :877-885
        dirv = (base - 1) // 4 - (nbase - 1) // 4
        w2 = _weights(nfd)
        W2 = (w2[:, 0, :, None, None] * w2[:, 1, None, :, None] * w2[:, 2, None, None, :]).reshape(n, 27)
        xp = (OFFS[None, :, :] - nfd[:, None, :]) * dx
        st = np.empty((n, 27, 4))
        st[:, :, 0] = mass * W2
        st[:, :, 1:] = (mass * W2)[:, :, None] * vel[:, None, :] + np.einsum("nrc,nsc->nsr", Cm, xp) * W2[:, :, None]
        st[disc] = 0.0
        # the sort key of the NEXT step (mpm_g2p2g.hpp): the stencil base predicted after one more advection with the current velocity, in the
        # node cube of the block the particle is in after THIS step, clamped to 0 .. 5 per axis and packed y * 36 + x * 6 + z
        sort_arg = nfd + vel * (new_dt / dx)
        pk = np.clip(((narena - 1) & 3) + np.rint(np.where(np.isfinite(sort_arg), sort_arg, 0.0)).astype(np.int64), 0, 5)
        out.update(sort_key=pk[:, 1] * 36 + pk[:, 0] * 6 + pk[:, 2], sort_arg=sort_arg)
    out.update(new_base=nbase, narena=narena, discarded=disc, dirtag=(dirv[:, 0] + 1) * 9 + (dirv[:, 1] + 1) * 3 + dirv[:, 2] + 1,
               dir_ok=(np.abs(dirv) <= 1).all(axis=1), nodes=nbase[:, None, :] + OFFS[None, :, :], stencil=st)
    fin = np.isfinite(pos).all(axis=1) & np.isfinite(st).all(axis=(1, 2))
    for k in ("b6", "logjp", "J"):
        if k in out:
            fin &= np.isfinite(out[k].reshape(n, -1)).all(axis=1)
    out["finite"] = fin
    return out


def gather_field(pos_cells, tier, seed=0):
    """vn of step() from the field."""
    return field(stencil_base(pos_cells)[:, None, :] + OFFS[None, :, :], tier, seed)


def pack_nodes(nodes):
    n = np.asarray(nodes).astype(np.int64)
    return (n[..., 0] << 40) | (n[..., 1] << 20) | n[..., 2]


def gather_grid(pos_cells, keys, blocks):
    """vn of step() from a dumped grid (keys (n, 3), blocks (n, 4, 64), channels 1 .. 3 = the node velocities): every stencil node of every
    particle must lie in a dumped block."""
    index = {tuple(k): i for i, k in enumerate(np.asarray(keys).astype(np.int64).tolist())}
    nodes = stencil_base(pos_cells)[:, None, :] + OFFS[None, :, :]
    blk = np.array([index[tuple(k)] for k in (nodes // 4).reshape(-1, 3).tolist()], np.int64).reshape(nodes.shape[:2])
    cell = (nodes[..., 0] & 3) * 16 + (nodes[..., 1] & 3) * 4 + (nodes[..., 2] & 3)
    return np.stack([np.asarray(blocks)[blk, c, cell] for c in (1, 2, 3)], axis=-1)


def unpack_nodes(k):
    k = np.asarray(k, np.int64)
    return np.stack([k >> 40, (k >> 20) & 0xFFFFF, k & 0xFFFFF], axis=-1)


def assemble(outs, stencil_bounds):
    """The grid a set of step() results leaves: the contributions of all kept particles summed per node in float64.  outs: a list of step()
    dicts (one per model sharing the grid), stencil_bounds: per dict the relative per-particle stencil bound - a number, or (n, 2) {mass, momentum} per particle.  Returns {"key" (k,) packed nodes,
    sorted, "sum" (k, 4), "n" (k,) contributions, "abs" (k, 4) sum |c|, "E" (k, 4) sum of the per-particle bounds E_p = bound x the particle's
    largest mass / momentum entry}."""
    keys, vals, errs = [], [], []
    for o, sb in zip(outs, stencil_bounds):
        keep = ~o["discarded"] & o["finite"]
        st = o["stencil"][keep]
        keys.append(pack_nodes(o["nodes"][keep]).reshape(-1))
        vals.append(st.reshape(-1, 4))
        sb = np.broadcast_to(np.asarray(sb, np.float64).reshape(-1, 2) if np.ndim(sb) == 2 else np.full((1, 2), float(sb)), (o["finite"].size, 2))[keep]
        e = np.empty((st.shape[0], 4))
        e[:, 0] = sb[:, 0] * np.abs(st[:, :, 0]).max(axis=1, initial=0.0)
        e[:, 1:] = (sb[:, 1] * np.abs(st[:, :, 1:]).max(axis=(1, 2), initial=0.0))[:, None]
        errs.append(np.repeat(e, 27, axis=0))
    keys, vals, errs = np.concatenate(keys), np.concatenate(vals), np.concatenate(errs)
    uk, inv = np.unique(keys, return_inverse=True)
    out = {"key": uk, "sum": np.zeros((uk.size, 4)), "abs": np.zeros((uk.size, 4)), "E": np.zeros((uk.size, 4)), "n": np.bincount(inv, minlength=uk.size)}
    np.add.at(out["sum"], inv, vals)
    np.add.at(out["abs"], inv, np.abs(vals))
    np.add.at(out["E"], inv, errs)
    return out


def add_contribution(exp, keys, vals):
    """assemble()'s result with one more exact addend per node: vals (k, 4) at the packed nodes keys (k,), each at most once.  It counts as a
    contribution with E = 0: sum += r, abs += |r|, n += 1; a node nobody else contributes to becomes an expected node."""
    keys, vals = np.asarray(keys, np.int64), np.asarray(vals, np.float64).reshape(-1, 4)
    assert np.unique(keys).size == keys.size
    uk = np.union1d(exp["key"], keys)
    out = {"key": uk, "sum": np.zeros((uk.size, 4)), "abs": np.zeros((uk.size, 4)), "E": np.zeros((uk.size, 4)), "n": np.zeros(uk.size, np.int64)}
    ie, ik = np.searchsorted(uk, exp["key"]), np.searchsorted(uk, keys)
    for f in ("sum", "abs", "E", "n"):
        out[f][ie] = exp[f]
    out["sum"][ik] += vals
    out["abs"][ik] += np.abs(vals)
    out["n"][ik] += 1
    return out


def restrict(exp, keep):
    """assemble()'s result on the nodes selected by the bool mask `keep` over exp["key"]."""
    return {f: v[keep] for f, v in exp.items()}


def in_blocks(node_keys, block_keys3):
    """Mask over packed node keys: the node lies in one of the grid blocks `block_keys3` (n, 3)."""
    return np.isin(pack_nodes(unpack_nodes(node_keys) // 4), pack_nodes(np.asarray(block_keys3).reshape(-1, 3)))


def grid_nodes(keys, blocks):
    """The non-zero nodes of a dumped grid (keys (n, 3), blocks (n, 4, 64)): packed node keys, sorted, and their (k, 4) float64 values."""
    keys, blocks = np.asarray(keys).astype(np.int64), np.asarray(blocks, np.float64)
    b, cell = np.nonzero(np.abs(blocks).sum(axis=1) != 0) if blocks.size else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    nodes = 4 * keys[b] + np.stack([cell >> 4, (cell >> 2) & 3, cell & 3], axis=1)
    k = pack_nodes(nodes)
    order = np.argsort(k)
    assert np.unique(k).size == k.size, "a node appears in two grid blocks"
    return k[order], blocks[b, :, cell][order]


def compare_grid(exp, got_key, got_val):
    """|got - sum_p c_p| <= sum_p E_p + (n_g + 1) 2^-23 sum_p |c_p| per node and channel over the UNION of expected and returned nodes (a missing
    node is 0; a returned node nobody contributes to has a bound of 0: nothing may appear anywhere else).  Returns (worst ratio |diff| / bound,
    number of nodes beyond the bound, a description of the worst)."""
    uk = np.union1d(exp["key"], got_key)
    S, Ab, E, G = np.zeros((uk.size, 4)), np.zeros((uk.size, 4)), np.zeros((uk.size, 4)), np.zeros((uk.size, 4))
    N = np.zeros(uk.size)
    ie, ig = np.searchsorted(uk, exp["key"]), np.searchsorted(uk, got_key)
    S[ie], Ab[ie], E[ie], N[ie] = exp["sum"], exp["abs"], exp["E"], exp["n"]
    G[ig] = got_val
    bnd = E + (N[:, None] + 1) * 2.0 ** -23 * Ab
    diff = np.abs(G - S)
    bad = ~(diff <= bnd)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, diff / bnd, np.where(diff > 0, np.inf, 0.0))
    w = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.size else (0, 0)
    what = (unpack_nodes(uk[w[0]]).tolist(), int(w[1]), float(G[w]), float(S[w]), float(bnd[w]), int(N[w[0]])) if ratio.size else None
    return (float(ratio.max()) if ratio.size else 0.0), int(bad.any(axis=1).sum()), what


# ---- per-particle deviations (the metrics of the existing one-particle test) -------------------------------------------------------------
def err_pos(got, want):
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def err_b(got6, want6):
    return np.abs(got6 - want6).max(axis=1) / np.maximum(1.0, np.abs(want6).max(axis=1))


def err_J(got, want):
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def err_stencil(got, want):
    """(n, 27, 4) against (n, 27, 4): the worst of mass / largest mass and momentum / largest momentum entry, per particle"""
    sm = np.maximum(np.abs(want[:, :, 0]).max(axis=1), 1e-300)
    sp = np.maximum(np.abs(want[:, :, 1:]).max(axis=(1, 2)), 1e-300)
    return np.maximum(np.abs(got[:, :, 0] - want[:, :, 0]).max(axis=1) / sm, np.abs(got[:, :, 1:] - want[:, :, 1:]).max(axis=(1, 2)) / sp)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _lattice(lo, width, m, n, rng, jitter=0.48):
    """n points of a jittered m^3 lattice in the cube [lo, lo + width)^3 (a random subset), float32"""
    ijk = np.array([(i, j, k) for i in range(m) for j in range(m) for k in range(m)])
    pick = rng.permutation(m ** 3)[:n]
    assert n <= m ** 3
    h = width / m
    p = np.asarray(lo, np.float64)[None, :] + (ijk[pick] + 0.5 + rng.uniform(-jitter, jitter, (n, 3))) * h
    return p.astype(np.float32)


def block_particles(key, n, rng, planted=0):
    """n particles in particle block `key`: a jittered 11^3 lattice over [4k + 1.5, 4k + 5.5)^3, the first `planted` of them moved onto tie values
    (x / dx = N + 0.5) and onto the bounds of the block's first and last cell."""
    lo = 4.0 * np.asarray(key, np.float64) + 1.5
    p = _lattice(lo, 4.0, 11, n, rng)
    T = 4.0                                                               # stands for "the last float32 below the block's upper bound"
    ties = np.array([[0.0, 1.0, 2.0], [3.0, 0.0, 1.0], [T, 2.0, 3.0], [2.0, T, 0.0], [1.0, 3.0, T], [0.0, 0.0, 0.0], [3.0, 3.0, 3.0], [T, T, T]])
    for i in range(min(planted, n)):
        t = ties[i % len(ties)]
        axes = (0, 1, 2) if i >= 5 else (i % 3,)                          # one axis on a tie, the others where the lattice put them; then the block's corners
        for ax in axes:
            v = np.float32(lo[ax] + t[ax])
            p[i, ax] = np.nextafter(v, np.float32(0)) if t[ax] == T else v
    assert (block_keys(p) == np.asarray(key)[None, :]).all()
    return p


def scene_isolated(seed=1):
    """48 sites, one particle each; the particles of the last 8 sites sit on tie values."""
    rng = np.random.default_rng(seed)
    return np.concatenate([block_particles(k, 1, rng, planted=0) for k in SITES[:40]] + [block_particles(k, 8, rng, planted=8)[i:i + 1] for i, k in enumerate(SITES[40:48])])


def scene_block_sizes(seed=2):
    """One block per size of BLOCK_SIZES on the first 14 sites; the block of 129 carries 8 planted particles."""
    rng = np.random.default_rng(seed)
    return np.concatenate([block_particles(k, n, rng, planted=8 if n == 129 else 0) for k, n in zip(SITES, BLOCK_SIZES)])


def scene_one_cell(seed=3):
    """513 particles in a single cell of one block; 257 + 256 in two cells of another: all-equal sort keys."""
    rng = np.random.default_rng(seed)
    a = _lattice(4.0 * np.array(SITES[21]) + 1.5 + np.array([1.0, 2.0, 1.0]), 1.0, 9, 513, rng, jitter=0.25)
    b = _lattice(4.0 * np.array(SITES[42]) + 1.5 + np.array([3.0, 0.0, 2.0]), 1.0, 7, 257, rng, jitter=0.25)
    c = _lattice(4.0 * np.array(SITES[42]) + 1.5 + np.array([0.0, 3.0, 2.0]), 1.0, 7, 256, rng, jitter=0.25)
    return np.concatenate([a, b, c])


CLUSTER = [(6 + x, 6 + y, 6 + z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]


def scene_cluster(seed=4, lo=185, hi=215):
    """A 2 x 2 x 2 cluster of adjacent particle blocks with about 200 particles each: they share grid blocks, particles cross between them."""
    rng = np.random.default_rng(seed)
    return np.concatenate([block_particles(k, int(rng.integers(lo, hi + 1)), rng) for k in CLUSTER])


def scene_torn(seed=5):
    """The isolated scene and one block of 129 particles."""
    rng = np.random.default_rng(seed)
    return np.concatenate([scene_isolated(seed), block_particles(SITES[50], 129, rng, planted=8)])


SLAB = [(5 + x, 6 + y, 6 + z) for x in range(4) for y in (0, 1) for z in (0, 1)]


def scene_slab(seed=6, lo=185, hi=215):
    """A 4 x 2 x 2 slab of adjacent particle blocks, drawn like the cluster: long enough along x to be cut in two with a halo and an interior layer
    of blocks on either side (tests/test_g2p2g_split_gpu.py)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([block_particles(k, int(rng.integers(lo, hi + 1)), rng) for k in SLAB])


SCENE_SEED = {"isolated": 11, "block_sizes": 12, "one_cell": 13, "cluster": 14, "torn": 15, "slab": 16, "cluster_b": 44}
SCENES = {"isolated": scene_isolated, "block_sizes": scene_block_sizes, "one_cell": scene_one_cell, "cluster": scene_cluster, "torn": scene_torn}
# Scenes that scene_state() serves but that stay out of the yardstick: test_g2p2g_model_cpu.measure_generated iterates SCENES and check_constants
# pins Y to what it measures there.  A scene here is licensed by a CPU test of its own, which holds the reference side to bound() on it.
EXTRA_SCENES = {"slab": scene_slab, "cluster_b": lambda: scene_cluster(seed=44, lo=90, hi=110)}     # cluster_b: a second, thinner model in the cluster's blocks
BANDS = ((0.97, 1.03), (0.9, 1.1), (0.75, 1.3))
BAND_SHARE = (0.5, 0.25, 0.25)                 # half of the draws from the innermost band: NACC's case 0 (inside the yield surface) lives there
# A float32 SVD that has converged reproduces F to a few ulp: the median residual max |U S V^T - F| of the reference's 4-sweep SVD (svd.cuh:167)
# on the trial F of these scenes is 4.4e-7.  On a few per cent of random F it has NOT converged - residuals up to 2e-3, and the b the reference
# stores is off by just that much, whatever the branch.  Such rows say nothing about float32 arithmetic; a scene holds none of them (scene_state).
SVD_RESIDUAL = 2e-6                            # 16 ulp of an entry of size 1


def _rotations(n, rng):
    Q, R = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    Q = Q * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]
    Q[np.linalg.det(Q) < 0, :, 2] *= -1
    return Q


def make_state(material, n, seed):
    """The particle state of a scene: F = R1 diag(s) R2 with s uniform in one of three bands, rounded to float32 (what the oracle is fed);
    b6 = fl32(F32 F32^T) computed in float64 (what the engine and the model are fed); log Jp in [-0.01, 0.01] (sand) / [-0.03, 0.01] (NACC); J in
    [0.8, 1.1] (J-fluid); 5 % of the fixed-corotated and sand particles reflected (one stretch negated, the mark set)."""
    rng = np.random.default_rng(1000 * seed + material)
    st = dict(F32=None, b6=None, reflected=None, logjp=None, J=None)
    if material == J_FLUID:
        st["J"] = rng.uniform(0.8, 1.1, n).astype(np.float32)
        return st
    band = np.array(BANDS)[rng.choice(3, n, p=BAND_SHARE)]
    s = rng.uniform(band[:, :1], band[:, 1:], (n, 3))
    refl = (rng.random(n) < 0.05) if material in (FC, SAND) else np.zeros(n, bool)
    # A reflected F carries its sign on the smallest stretch (svd.cuh:590-770), so what it means depends on WHICH stretch is the smallest: with the two
    # smallest close together that choice - in the reference's 4-sweep SVD of F as much as in an eigen-decomposition of b - is ill-conditioned (the
    # oracle's own stress then deviates from the closed form by 1e-3).  Reflected particles get their smallest stretch reduced by 7 %: a clear gap.
    s[refl, np.argmin(s[refl], axis=1)] *= 0.93
    s[refl, rng.integers(0, 3)] *= -1
    F = np.einsum("nij,nj,njk->nik", _rotations(n, rng), s, _rotations(n, rng))
    F32 = F.astype(np.float32)
    F64 = F32.astype(np.float64)
    st.update(F32=F32, b6=mats_to_b6(F64 @ F64.transpose(0, 2, 1)).astype(np.float32), reflected=refl)
    if material == SAND:
        st["logjp"] = rng.uniform(-0.01, 0.01, n).astype(np.float32)
    if material == NACC:
        st["logjp"] = rng.uniform(-0.03, 0.01, n).astype(np.float32)
    return st


def model_scene(material, pos_cells, st, tier, seed=0, dt=DT, new_dt=NEW_DT, overrides=None):
    """step() on a scene with the field of `tier`.  overrides: the model's parameters (None: material_overrides)."""
    c = constants(material, material_overrides(material) if overrides is None else overrides)
    return step(c, pos_cells, gather_field(pos_cells, tier, seed), b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"], dt=dt, new_dt=new_dt)


# ---- the oracle on the same rows ---------------------------------------------------------------------------------------------------------
def oracle_params(material, overrides, bits=BITS):
    from oracle_ffi import oracle_api
    p = _ffi.MaterialParams()
    assert oracle_api().default_material(material, bits, C.byref(p)) == 0
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def oracle_rows(material, params, bits, arena, rows13, dt, new_dt):
    """mpmo_fn_particle_step on rows {pos (world), F 9 column-major (J in F[0]), log Jp} sharing one velocity arena (3, 8, 8, 8): (out_f (n, 154),
    out_i (n, 14)), see oracle/mpm_oracle.c."""
    from oracle_ffi import oracle_api
    fn = oracle_api().raw.mpmo_fn_particle_step
    fn.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    rows = np.ascontiguousarray(rows13, np.float32)
    arena = np.ascontiguousarray(arena, np.float32)
    n = rows.shape[0]
    of, oi = np.zeros((n, 154), np.float32), np.zeros((n, 14), np.int32)
    assert fn(material, C.byref(params), bits, arena.ctypes.data, rows.ctypes.data, n, dt, new_dt, of.ctypes.data, oi.ctypes.data) == 0
    return of, oi


def oracle_scene(material, pos_cells, st, tier, seed=0, dt=DT, new_dt=NEW_DT, bits=BITS, overrides=None):
    """The oracle's particle body on a scene, block by block (the particles of a block share its velocity arena)."""
    pos_cells = np.asarray(pos_cells, np.float32)
    n = pos_cells.shape[0]
    params = oracle_params(material, material_overrides(material, bits) if overrides is None else overrides, bits)
    rows = np.zeros((n, 13), np.float32)
    rows[:, :3] = pos_cells * np.float32(0.5 ** bits)
    if material == J_FLUID:
        rows[:, 3] = st["J"]
    else:
        rows[:, 3:12] = em.to_flat(st["F32"])
        if st["logjp"] is not None:
            rows[:, 12] = st["logjp"]
    keys = block_keys(pos_cells)
    of, oi = np.zeros((n, 154), np.float32), np.zeros((n, 14), np.int32)
    for k in np.unique(keys, axis=0):
        sel = np.flatnonzero((keys == k[None, :]).all(axis=1))
        of[sel], oi[sel] = oracle_rows(material, params, bits, cube_of(k, tier, seed), rows[sel], dt, new_dt)
    return of, oi


def oracle_view(material, of, oi, bits=BITS):
    """The oracle's rows in the model's terms: pos (cells), b6 of the F it stored, logjp / J, stencil (n, 27, 4), base, new_base, discarded."""
    of64 = of.astype(np.float64)
    F = em.to_mats(of64[:, 15:24])
    base = oi[:, 0:3].astype(np.int64)
    out = dict(pos=of64[:, 12:15] * 2.0 ** bits, base=base, discarded=oi[:, 13] != 0, dirtag=oi[:, 9].astype(np.int64),
               new_base=oi[:, 6:9].astype(np.int64) + 1, stencil=of64[:, 46:154].reshape(-1, 27, 4))
    if material == J_FLUID:
        out["J"] = of64[:, 15]
    else:
        with np.errstate(all="ignore"):
            out["b6"] = mats_to_b6(F @ F.transpose(0, 2, 1))
        out["logjp"] = of64[:, 24]
    return out


def reference_svd_residual(F):
    """max |U S V^T - F| of the reference's own SVD (the oracle's orc_svd3, bit for bit math::svd by golden vector G3) on (n, 3, 3) matrices
    rounded to float32, relative to max(1, max |F|)"""
    from oracle_ffi import oracle_api
    F32 = np.asarray(F, np.float64).astype(np.float32)
    flat = np.ascontiguousarray(em.to_flat(F32))
    out = np.zeros((flat.shape[0], 21), np.float32)
    assert oracle_api().raw.mpmo_test_svd(flat.ctypes.data, flat.shape[0], out.ctypes.data, 0) == 0
    o = out.astype(np.float64)
    R = np.einsum("nij,nj,nkj->nik", em.to_mats(o[:, :9]), o[:, 9:12], em.to_mats(o[:, 12:21]))
    F64 = F32.astype(np.float64)
    return np.abs(R - F64).max(axis=(1, 2)) / np.maximum(1.0, np.abs(F64).max(axis=(1, 2)))


def ill_posed(material, pos_cells, st, tiers=tuple(TIERS), seed=0, bits=BITS, overrides=None):
    """The rows of a scene that cannot be held to a float bound on some tier: the sand branch / NACC case - at the parameters `overrides` - changes
    when the trial F is scaled by 1 +- 1e-5 (step's "unstable"), or the reference's SVD has not converged on the trial F (SVD_RESIDUAL)."""
    bad = np.zeros(np.asarray(pos_cells).shape[0], bool)
    if material == J_FLUID:
        return bad
    dx = 0.5 ** bits
    for tier in tiers:
        m = model_scene(material, pos_cells, st, tier, seed, overrides=overrides)
        G = np.eye(3)[None] + DT * (4.0 / (dx * dx)) * m["A"]
        bad |= m["unstable"] | ~m["finite"] if tier != "torn" else m["unstable"]
        bad |= reference_svd_residual(G @ st["F32"].astype(np.float64)) > SVD_RESIDUAL
    return bad


_SCENE_STATES = {}


def scene_state(name, material, overrides=None):
    """The positions (cells, float32) and the state of scene `name` for a material: one fixed draw per scene, material and parameter set
    (overrides; None: material_overrides).  Rows that are ill_posed on any tier get the state of a further draw, until none is left: no scene
    holds a row on the brink of a branch of ITS parameters, or one whose trial F the reference cannot decompose."""
    key = (name, material) if overrides is None else (name, material, tuple(sorted(overrides.items())))
    if key not in _SCENE_STATES:
        pos = (SCENES[name] if name in SCENES else EXTRA_SCENES[name])()
        st = make_state(material, pos.shape[0], SCENE_SEED[name])
        for draw in range(1, 12):
            bad = ill_posed(material, pos, st, overrides=overrides)
            if not bad.any():
                break
            new = make_state(material, pos.shape[0], SCENE_SEED[name] + 100 * draw)
            for k in ("F32", "b6", "reflected", "logjp"):
                if st[k] is not None:
                    st[k][bad] = new[k][bad]
        assert not ill_posed(material, pos, st, overrides=overrides).any()
        _SCENE_STATES[key] = (pos, st)
    pos, st = _SCENE_STATES[key]
    return pos.copy(), {k: (v.copy() if v is not None else None) for k, v in st.items()}


def min_separation(pos_cells):
    """The smallest distance between two of the positions (cells): nearest-neighbour matching needs it well above the position bound."""
    from scipy.spatial import cKDTree
    d, _ = cKDTree(pos_cells).query(pos_cells, k=2)
    return float(d[:, 1].min())


# ---- the golden rows (tests/golden/g16_*: the reference's own statements, one particle per row, tests/test_oracle_golden.py) -----------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_NAMES = "bits vol mass mu lam cohesion beta_sand yield_surface volume_correction bm xi msqr hardening_on dt new_dt beta_nacc E nu rho bulk gamma viscosity".split()


def golden_rows():
    """(P, arenas (5, 3, 8, 8, 8), rows_in (960, 15) {material, arena, pos 3, F 9, log Jp}, out_f (960, 154), out_i (960, 14))"""
    ld = lambda name, t: np.fromfile(os.path.join(GOLDEN, name), t)
    P = dict(zip(GOLDEN_NAMES, [float(v) for v in ld("g16_params.f32", np.float32)]))
    return (P, ld("g16_arenas.f32", np.float32).reshape(-1, 3, 8, 8, 8), ld("g16_particle_in.f32", np.float32).reshape(-1, 15),
            ld("g16_particle_out.f32", np.float32).reshape(-1, 154), ld("g16_particle_out.i32", np.int32).reshape(-1, 14))


def golden_overrides(P, material):
    if material == J_FLUID:
        return dict(rho=P["rho"], volume=P["vol"], bulk=P["bulk"], gamma=P["gamma"], viscosity=P["viscosity"])
    p = dict(rho=P["rho"], volume=P["vol"], youngs_modulus=P["E"], poisson_ratio=P["nu"])
    if material == SAND:
        p.update(cohesion=P["cohesion"], beta=P["beta_sand"], yield_surface=P["yield_surface"], volume_correction=int(P["volume_correction"]))
    if material == NACC:
        p.update(beta=P["beta_nacc"], xi=P["xi"], msqr=P["msqr"], hardening_on=int(P["hardening_on"]))
    return p


def golden_state(material, rin):
    """The state of golden rows as the engine is fed it: b6 = fl32(F F^T) in float64 of the row's float32 F, the mark of det F < 0, log Jp; J."""
    if material == J_FLUID:
        return dict(F32=None, b6=None, reflected=None, logjp=None, J=rin[:, 5].copy())
    F = em.to_mats(rin[:, 5:14])
    return dict(F32=F.astype(np.float32), b6=mats_to_b6(F @ F.transpose(0, 2, 1)).astype(np.float32), reflected=np.linalg.det(F) < 0,
                logjp=rin[:, 14].copy() if material != FC else None, J=None)


def golden_model(material, P, arenas, rin):
    """step() on golden rows of one material (any arenas): the stencil velocities come out of each row's arena."""
    bits = int(P["bits"])
    pos = rin[:, 2:5].astype(np.float64) * 2.0 ** bits                # (exact)
    base = stencil_base(pos)
    ac = ((base - 1) & 3) + 1
    idx = ac[:, None, :] + OFFS[None, :, :]                           # (n, 27, 3) in the 8^3 arena
    a = rin[:, 1].astype(np.int64)
    vn = arenas[a[:, None], :, idx[..., 0], idx[..., 1], idx[..., 2]]  # (n, 27, 3)
    st = golden_state(material, rin)
    c = constants(material, golden_overrides(P, material))
    return step(c, pos, vn, b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"], dt=P["dt"], new_dt=P["new_dt"], bits=bits)

"""The parameter axis of the constitutive-model tests: the variants of mpm_material_params that tests/test_material_params_gpu.py runs the HIP
stress code at (function level: mpm_test_stress; block level: the real G2P2G kernels through tests/g2p2g_bench.py), the comparison of the
function-level rows with the float64 closed forms of tests/exact_models.py, and the bounds of the block-level comparison.
tests/test_material_params_cpu.py judges all of it without a GPU, with the oracle standing in for the device.

Yardsticks are the ORACLE's deviations from the closed forms / the block model, never the device's: measured by
`python tests/test_material_params_cpu.py`, held in E1_YARDSTICK / BLOCK_YARDSTICK below and in profiles/material_params_yardstick.txt.

Test infrastructure only."""
import ctypes as C
import os

import numpy as np

import exact_models as em
import g2p2g_model as gm
from claymore_amd import _ffi

J_FLUID, FC, SAND, NACC = gm.J_FLUID, gm.FC, gm.SAND, gm.NACC
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _f(x):
    return float(np.float32(x))


# (id, material, overrides on top of the defaults); float values are the float32 roundings.
VARIANTS = [
    ("S1", SAND, dict(cohesion=_f(0.01))),                                              # the golden rows idx % 5 == 4
    ("S2", SAND, dict(volume_correction=0)),                                            # the golden rows idx % 7 == 6
    ("S3", SAND, dict(cohesion=_f(0.05), beta=_f(0.5), yield_surface=_f(0.21012822))),  # friction angle 20 degrees
    ("N1", NACC, dict(hardening_on=0)),                                                 # the golden rows idx % 7 == 6
    ("N2", NACC, dict(beta=_f(0.1), xi=_f(3.0))),
    ("N3", NACC, dict(msqr=_f(8.0))),
    ("F1", J_FLUID, dict(gamma=_f(1.0), viscosity=_f(0.0))),
    ("F2", J_FLUID, dict(bulk=_f(1e3), gamma=_f(3.0), viscosity=_f(1.0))),
    ("E1", FC, dict(poisson_ratio=_f(0.49))),                                           # lambda >> mu: function level only
    ("E1", SAND, dict(poisson_ratio=_f(0.49))),
    ("E1", NACC, dict(poisson_ratio=_f(0.49))),
]
FUNCTION_VARIANTS = [v for v in VARIANTS if v[1] != J_FLUID]                             # (there is no mpm_test_jfluid: the fluid is covered at block level)
BLOCK_VARIANTS = [v for v in VARIANTS if v[0] != "E1"]
BY_ID = {vid: (material, delta) for vid, material, delta in BLOCK_VARIANTS}
# what the block-level GPU tests run, per variant: (scene, tier)
BLOCK_CASES = (("block_sizes", "flow"), ("cluster", "flow"), ("cluster", "fast"))
MIXED = ("S3", "cluster_b", "flow")                                                     # the second model of the mixed scene (the first: the cluster at the defaults)


def vname(vid, material):
    return "%s-%s" % (vid, gm.NAMES[material])


def block_overrides(vid):
    """(material, the full parameter set of a block-level scene at variant `vid`: g2p2g_model.material_overrides with the variant's on top)"""
    material, delta = BY_ID[vid]
    return material, dict(gm.material_overrides(material), **delta)


# ---- yardsticks (measured on the CPU, asserted by tests/test_material_params_cpu.py to the three digits written) --------------------------
# E1: the oracle's worst deviation from the closed form over the kept rows, {(material name, "stress" | "b"): value}; stress relative to vol * E.
E1_YARDSTICK = {
    ("fc", "stress"): 0.00405, ("nacc", "b"): 0.000347, ("nacc", "stress"): 0.000107, ("sand", "b"): 0.000167, ("sand", "stress"): 0.000125,
}
# Block level: the oracle's deviation from the block model where it EXCEEDS g2p2g_model.bound() - {(variant, scene, tier, quantity): value}.  Everywhere
# else the oracle alone stays inside gm.bound (the licence test) and that bound is used unchanged.
BLOCK_YARDSTICK = {
    ("N2", "block_sizes", "flow", "b"): 0.000105,            # 1.09 x gm.bound: the oracle's own 4-sweep SVD, not the model
}


def block_bound(vid, scene, tier, quantity, material):
    """gm.bound, or max(gm.bound, 3 x the oracle's own deviation) where the oracle alone leaves gm.bound at this variant"""
    return max(gm.bound(quantity, tier, material), 3.0 * BLOCK_YARDSTICK.get((vid, scene, tier, quantity), 0.0))


def yardstick_lines(e1=None, block=None):
    e1 = E1_YARDSTICK if e1 is None else e1
    block = BLOCK_YARDSTICK if block is None else block
    return (["function E1 %-5s %-7s %.3g" % (mat, q, v) for (mat, q), v in sorted(e1.items())]
            + ["block %-3s %-12s %-5s %-8s %.3g" % (k + (v,)) for k, v in sorted(block.items())])


# ---- function level ------------------------------------------------------------------------------------------------------------------------
def f32(name):
    return np.fromfile(os.path.join(GOLDEN, name), dtype=np.float32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def params(api, material, delta=None):
    """The parameters of the function-level tests (tests/test_parity_gpu.py: the defaults at 8 bits with the golden generator's volume) with `delta` on top"""
    p = _ffi.MaterialParams()
    assert api.default_material(material, 8, C.byref(p)) == 0
    p.volume = float(f32("g456_params.f32")[0])
    for k, v in (delta or {}).items():
        setattr(p, k, v)
    return p


def lame(p):
    e, nu = np.float32(p.youngs_modulus), np.float32(p.poisson_ratio)
    return np.float64(e / (2 * (1 + nu))), np.float64(e * nu / ((1 + nu) * (1 - 2 * nu)))     # (numpy scalars: mu = 0 divides to nan, not to an exception)


def bform(F9):
    """b = F F^T (n, 9) in float64 of column-major deformation gradients: what the device's stress functions return for a (projected) F"""
    F = np.asarray(F9, dtype=np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)
    return np.einsum("nij,nkj->nik", F, F).reshape(-1, 9)


def inputs(material):
    """The G3 deformation gradients (2048 rows) and the material's golden log Jp inputs (None for fixed-corotated)"""
    F = f32("g3_F_in.f32").reshape(-1, 9)
    lj = None if material == FC else f32("g5_sand_logjp_in.f32" if material == SAND else "g6_nacc_logjp_in.f32")
    return F, lj


def stress_rows(api, material, p, F, lj):
    """One test_stress call of `api` (the HIP library or the oracle): (n, 19) {b or F 9, P F^T 9, log Jp}"""
    F = np.ascontiguousarray(F, np.float32)
    out = np.empty((F.shape[0], 19), dtype=np.float32)
    lj = None if lj is None else np.ascontiguousarray(lj, np.float32)
    assert api.test_stress(material, C.byref(p), ptr(F), None if lj is None else ptr(lj), F.shape[0], ptr(out), 0) == 0
    return out


def exact(material, p, F, lj):
    """The float64 closed form at the parameters p: (F_new 9 or None, P F^T 9, log Jp or None, label = sand branch / NACC case / zeros)"""
    mu, lam = lame(p)
    if material == FC:
        return None, em.fixed_corotated(F, mu, lam, p.volume), None, np.zeros(F.shape[0], np.int64)
    if material == SAND:
        Fn, PF, L = em.sand(F, lj, mu, lam, p.volume, p.cohesion, p.beta, p.yield_surface, p.volume_correction)
        return Fn, PF, L, em.sand_branch(F, lj, mu, lam, p.cohesion, p.yield_surface)
    return em.nacc(F, lj, mu, lam, p.volume, p.beta, p.xi, p.msqr, p.hardening_on)


def labels(material, p, F, lj):
    mu, lam = lame(p)
    if material == SAND:
        return em.sand_branch(F, lj, mu, lam, p.cohesion, p.yield_surface)
    if material == NACC:
        return em.nacc(F, lj, mu, lam, p.volume, p.beta, p.xi, p.msqr, p.hardening_on)[3]
    return np.zeros(F.shape[0], np.int64)


def stable_rows(material, p, F, lj):
    """The sand branch / NACC case stands under four draws of a 3e-6 perturbation of F (the draws of tests/test_parity_gpu.py)"""
    lab = labels(material, p, F, lj)
    rng = np.random.default_rng(1)
    stable = np.ones(F.shape[0], dtype=bool)
    if material != FC:
        for _ in range(4):
            stable &= labels(material, p, F.astype(np.float64) * (1 + 3e-6 * rng.standard_normal(F.shape)), lj) == lab
    return stable


GOLDEN_ROWS = {"S1": ("g5_sand_out.f32", lambda i: (i % 5 == 4) & (i % 7 != 6)), "S2": ("g5_sand_out.f32", lambda i: (i % 7 == 6) & (i % 5 != 4)),
               "N1": ("g6_nacc_out.f32", lambda i: i % 7 == 6)}
CAPS = {SAND: {"stress": 1e-5, "b": 1e-5}, NACC: {"stress": 5e-6, "b": 1e-5}, FC: {"stress": 1e-5}}
B_SLACK = {SAND: 4e-6, NACC: 6e-6}
LOGJP_BOUND = {SAND: 2e-6, NACC: 3e-6}
N_LABELS = {FC: 1, SAND: 3, NACC: 4}


def compare_function_level(vid, material, p, F, lj, got_b, got_PF, got_lj, ref, tag="", absolute=True):
    """One variant's rows against the closed form, the oracle's rows `ref` (n, 19) {F, P F^T, log Jp} as the yardstick: the rules of
    test_device_sand_vs_reference_golden_and_closed_form / test_device_nacc_vs_closed_form_and_reference_golden.  got_b (n, 9): F F^T of the
    returned state.  absolute=False leaves out the absolute rules (the caps, the log Jp bound), which are the converging device solver's: the oracle's
    own 4-sweep SVD does not meet them.  Prints every figure, returns (fails, figures); figures["e_ref"], ["f_ref"]: the oracle's worst deviation
    on the kept rows."""
    n = F.shape[0]
    idx = np.arange(n)
    name = vname(vid, material)
    exF, exPF, exL, lab = exact(material, p, F, lj)
    r64 = ref.astype(np.float64)
    wide = idx % 8 <= 5
    ok = wide & np.isfinite(ref).all(axis=1) & stable_rows(material, p, F, lj) & np.isfinite(exPF).all(axis=1)
    fails = []
    counts = np.bincount(lab[ok], minlength=N_LABELS[material])[:N_LABELS[material]]
    print(f"{tag}{name}: rows of classes <= 5: {int(wide.sum())}, left out {int((wide & ~ok).sum())}, kept per branch / case {counts.tolist()}")
    if not (wide & ~ok).sum() <= 0.01 * wide.sum():
        fails.append(("rows left out", int((wide & ~ok).sum())))
    if material != FC and not counts.min() >= 20:
        fails.append(("a branch / case holds fewer than 20 rows", counts.tolist()))
    if not np.isfinite(np.concatenate([got_b, got_PF, got_lj[:, None]], axis=1)[ok]).all():
        fails.append(("non-finite output on a kept row",))
    scale = p.volume * p.youngs_modulus
    figs = {}
    with np.errstate(invalid="ignore"):
        e_dev = np.abs(got_PF - exPF).max(axis=1) / scale
        e_ref = np.abs(r64[:, 9:18] - exPF).max(axis=1) / scale
    figs["e_ref"] = float(e_ref[ok].max())
    e1 = vid == "E1"
    cap = max(CAPS[material]["stress"], 3.0 * figs["e_ref"]) if e1 else CAPS[material]["stress"]
    over = ok & ~(e_dev <= 2.0 * e_ref + 3e-6)
    print(f"{tag}{name} stress / (vol E): worst {np.nanmax(e_dev[ok]):.3g} cap {cap:.3g}; yardstick (oracle) worst {figs['e_ref']:.3g}; rows beyond 2 e_ref + 3e-6: {int(over.sum())}")
    if absolute and not np.nanmax(e_dev[ok]) <= cap:
        fails.append(("stress cap", float(np.nanmax(e_dev[ok])), cap))
    if over.any():
        fails.append(("stress beyond 2 e_ref + 3e-6", int(over.sum()), idx[over][:5].tolist(), e_dev[over][:5].tolist(), e_ref[over][:5].tolist()))
    if material != FC:
        exB = bform(exF)
        with np.errstate(invalid="ignore"):
            f_dev = np.abs(got_b - exB).max(axis=1)
            f_ref = np.abs(bform(r64[:, 0:9]) - exB).max(axis=1)
        figs["f_ref"] = float(f_ref[ok].max())
        capb = max(CAPS[material]["b"], 3.0 * figs["f_ref"]) if e1 else CAPS[material]["b"]
        over = ok & ~(f_dev <= 2.0 * f_ref + B_SLACK[material])
        print(f"{tag}{name} b: worst {np.nanmax(f_dev[ok]):.3g} cap {capb:.3g}; yardstick (oracle) worst {figs['f_ref']:.3g}; rows beyond 2 f_ref + {B_SLACK[material]:.0e}: {int(over.sum())}")
        if absolute and not np.nanmax(f_dev[ok]) <= capb:
            fails.append(("b cap", float(np.nanmax(f_dev[ok])), capb))
        if over.any():
            fails.append(("b beyond 2 f_ref + slack", int(over.sum()), idx[over][:5].tolist(), f_dev[over][:5].tolist(), f_ref[over][:5].tolist()))
        dl = np.abs(got_lj.astype(np.float64) - exL)
        print(f"{tag}{name} log Jp: worst |dev - exact| {dl[ok].max():.3g} bound {LOGJP_BOUND[material]:.3g} (oracle {np.abs(r64[ok, 18] - exL[ok]).max():.3g})")
        if absolute and not dl[ok].max() <= LOGJP_BOUND[material]:
            fails.append(("log Jp", float(dl[ok].max()), LOGJP_BOUND[material]))
        if vid in ("S2", "N1"):                                  # the update is off: the closed form's log Jp is the input (or 0), exactly
            same = got_lj.astype(np.float64)[ok] == exL[ok]
            print(f"{tag}{name} log Jp bit-equal to the closed form's on {int(same.sum())} of {int(ok.sum())} kept rows")
            if not same.all():
                fails.append(("log Jp not bit-equal", int((~same).sum())))
    if vid in GOLDEN_ROWS:                                       # the golden rows the default-parameter tests skip, compared as those tests compare theirs
        fname, pick = GOLDEN_ROWS[vid]
        w = f32(fname).reshape(n, 19).astype(np.float64)
        g = ok & pick(idx) & np.isfinite(w).all(axis=1)
        with np.errstate(invalid="ignore"):
            e_gold = np.abs(w[:, 9:18] - exPF).max(axis=1) / scale
            f_gold = np.abs(bform(w[:, 0:9]) - exB).max(axis=1)
        bad_e = g & ~(e_dev <= 2.0 * e_gold + 3e-6)
        bad_f = g & ~(f_dev <= 2.0 * f_gold + B_SLACK[material])
        dg = np.abs(got_lj.astype(np.float64) - w[:, 18])[g].max()
        print(f"{tag}{name} golden rows: {int(g.sum())}; golden's own worst stress {e_gold[g].max():.3g}, b {f_gold[g].max():.3g}; rows beyond: stress {int(bad_e.sum())}, b {int(bad_f.sum())}; log Jp |dev - golden| {dg:.3g}")
        if not g.sum() >= 100:
            fails.append(("golden rows", int(g.sum())))
        if bad_e.any() or bad_f.any():
            fails.append(("golden yardstick", int(bad_e.sum()), int(bad_f.sum())))
        if absolute and material == SAND and not dg < 1e-5:
            fails.append(("log Jp against the golden output", float(dg)))
    return fails, figs

"""The constitutive models OFF their default parameters (tests/material_variants.py): the HIP stress code of claymore_amd/csrc/mpm_device_math.hpp
at every parameter mpm_material_params lets a caller set, against the float64 closed forms of tests/exact_models.py with the oracle at the same
parameters as the yardstick.

Function level: mpm_test_stress on the G3 inputs at every variant - the golden rows tests/test_parity_gpu.py leaves out (cohesion 0.01, volume
correction off, hardening off) among them - and the wave-level votes of the stress functions at their edges.  Block level: one substep of the real
G2P2G kernels (the stress code with the LDS scatter chain hooked into it) at S1-S3, N1-N3, F1, F2 on injected state, checked as
tests/test_g2p2g_blocks_gpu.py checks the default parameters - grid nodes and total mass included, which is what sees a hook site that a scalar
branch skipped or doubled.  The bounds are g2p2g_model.bound() wherever the oracle alone stays inside it at the variant
(tests/test_material_params_cpu.py asserts it), else max(that, 3 x the oracle's own deviation), material_variants.BLOCK_YARDSTICK.

Kernel mutations: NOT RUN on an MI355X.  From reading the code, a stress function that ignores a parameter fails the function-level test of that
variant and every block-level test of it (tests/test_material_params_cpu.py shows both comparisons rejecting the oracle run at the default
parameters); a hook site skipped or doubled under a non-default scalar branch is expected to fail the grid comparison and the total-mass check
of that variant's block-level tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

import g2p2g_model as gm
import material_variants as mv
from claymore_amd import _ffi
from g2p2g_bench import Bench
from test_g2p2g_blocks_gpu import check

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FC, SAND, NACC = _ffi.FIXED_COROTATED, _ffi.SAND, _ffi.NACC


def oracle():
    from oracle_ffi import oracle_api
    return oracle_api()


# ---- function level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vid,material,delta", mv.FUNCTION_VARIANTS, ids=[mv.vname(v, m) for v, m, _ in mv.FUNCTION_VARIANTS])
def test_device_stress_at_the_variant_against_the_closed_form(vid, material, delta):
    """One mpm_test_stress call on the 2048 G3 rows at the variant's parameters: stress, projected b and log Jp against the closed form at those
    parameters, never further from it than twice the oracle at the same parameters on the same rows (+ the slack of the default-parameter tests),
    and inside those tests' absolute caps (E1: max(the cap, 3 x the oracle's worst)).  S1, S2, N1 also against the golden rows of the reference
    itself that carry these parameters.

    E1 (poisson_ratio 0.49, lambda / E = 16.4) is what found the one weakness this file has found so far: with J = sigma_0 sigma_1 sigma_2 from three
    rooted eigenvalues and the volumetric term passed through U diag(.) U^T, 7 fixed-corotated rows and 1 sand row of 1536 left the per-row rule
    (row 460: 1.48e-5 of vol E against the oracle's 2.81e-6; sand row 229: 5.49e-6 against 4.01e-7) - the rotations' rounding in the eigenvalues and
    U's departure from orthogonality, amplified by lambda / E.  stress_fixed_corotated and stress_sand now take det b from b itself (sym_det3) and put
    the isotropic term on the diagonal directly."""
    hip = _ffi.load_hip()
    F, lj = mv.inputs(material)
    p = mv.params(hip, material, delta)
    got = mv.stress_rows(hip, material, p, F, lj)
    ref = mv.stress_rows(oracle(), material, mv.params(oracle(), material, delta), F, lj)
    with np.errstate(all="ignore"):
        fails, figs = mv.compare_function_level(vid, material, p, F, lj, got[:, 0:9].astype(np.float64), got[:, 9:18].astype(np.float64), got[:, 18], ref)
    assert not fails, fails


# ---- the wave votes at their edges ---------------------------------------------------------------------------------------------------------
N_WAVE = 256


def undeformed_rows():
    F = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (N_WAVE, 1))
    F[:, 1] = 2e-10                       # the off-diagonal dust of test_device_undeformed_wave_early_exit
    F[:, 5] = -3e-10
    return F


def against_closed_form(material, p, F, lj, got, rows, tag):
    """The rules of the function-level test on the rows `rows` (an index array), the oracle as the yardstick; returns the failures"""
    ref = mv.stress_rows(oracle(), material, p, F, lj)
    exF, exPF, exL, _ = mv.exact(material, p, F, lj)
    scale = p.volume * p.youngs_modulus
    e_dev = (np.abs(got[:, 9:18] - exPF).max(axis=1) / scale)[rows]
    e_ref = (np.abs(ref[:, 9:18] - exPF).max(axis=1) / scale)[rows]
    fails = []
    print(f"{tag} stress / (vol E): worst {e_dev.max():.3g}, oracle {e_ref.max():.3g}")
    if not (e_dev <= 2.0 * e_ref + 3e-6).all():
        fails.append(("stress", float(e_dev.max()), float(e_ref.max())))
    if material != FC:
        exB = mv.bform(exF)
        f_dev = np.abs(got[:, 0:9] - exB).max(axis=1)[rows]
        f_ref = np.abs(mv.bform(ref[:, 0:9]) - exB).max(axis=1)[rows]
        dl = np.abs(got[:, 18].astype(np.float64) - exL)[rows]
        print(f"{tag} b: worst {f_dev.max():.3g}, oracle {f_ref.max():.3g}; log Jp: worst {dl.max():.3g} bound {mv.LOGJP_BOUND[material]:.3g}")
        if not (f_dev <= 2.0 * f_ref + mv.B_SLACK[material]).all():
            fails.append(("b", float(f_dev.max()), float(f_ref.max())))
        if not dl.max() <= mv.LOGJP_BOUND[material]:
            fails.append(("log Jp", float(dl.max())))
    return fails


def test_cohesive_sand_does_not_leave_an_undeformed_wave_early():
    """Sand at S3, every lane undeformed, log Jp = +0.2: the trace is >= 0, so the cone tip applies - with cohesion the tip is b = exp(2 c) I, a
    stress of (2 mu + 3 lambda) c vol and log Jp moved by beta * sum epsilon: the undeformed wave must NOT leave early."""
    hip = _ffi.load_hip()
    p = mv.params(hip, SAND, mv.BY_ID["S3"][1])
    F, lj = undeformed_rows(), np.full(N_WAVE, 0.2, np.float32)
    got = mv.stress_rows(hip, SAND, p, F, lj)
    c = float(p.cohesion)
    exF, exPF, exL, branch = mv.exact(SAND, p, F, lj)
    assert (branch == 2).all() and np.allclose(mv.bform(exF), np.tile((np.exp(2 * c) * np.eye(3)).reshape(1, 9), (N_WAVE, 1)), atol=1e-12)
    print("b00", got[0, 0], "exp(2c)", np.exp(2 * c), "log Jp", got[0, 18], "closed form", exL[0], "P F^T / (vol E)", got[0, 9] / (p.volume * p.youngs_modulus))
    assert np.abs(got[:, [0, 4, 8]] - np.exp(2 * c)).max() < 1e-5 and np.abs(got[:, [1, 2, 3, 5, 6, 7]]).max() < 1e-5
    fails = against_closed_form(SAND, p, F, lj, got, np.arange(N_WAVE), "S3 tip")
    assert not fails, fails


@pytest.mark.parametrize("lj70", [-0.02, 0.02])
def test_sand_vote_with_one_lane_off_the_tip(lj70):
    """Sand at the defaults, every lane undeformed with log Jp = 0 but lane 70.  log Jp(70) = -0.02: that lane lies inside the cone - log Jp comes
    back 0, stress 0, b unchanged - and its wave takes the full path, which leaves the other lanes where the closed form says.  log Jp(70) = +0.02:
    every lane sits at the tip with zero strain: nothing changes anywhere, log Jp comes back bit for bit."""
    hip = _ffi.load_hip()
    p = mv.params(hip, SAND)
    F, lj = undeformed_rows(), np.zeros(N_WAVE, np.float32)
    lj[70] = lj70
    got = mv.stress_rows(hip, SAND, p, F, lj)
    exF, exPF, exL, branch = mv.exact(SAND, p, F, lj)
    scale = p.volume * p.youngs_modulus
    b_in = mv.bform(F)
    assert branch[70] == (0 if lj70 < 0 else 2)       # (the other lanes: the dust puts their trace at -1e-20, on either side of the tip condition - with the same result)
    assert np.abs(exPF).max() / scale < 1e-8 and np.abs(mv.bform(exF) - b_in).max() < 1e-8            # the truth: zero stress, b stays
    print("lane 70: log Jp", got[70, 18], "closed form", exL[70], "max |P F^T| / (vol E)", np.abs(got[:, 9:18]).max() / scale, "max |b - b_in|", np.abs(got[:, 0:9] - b_in).max())
    assert np.abs(got[:, 9:18]).max() / scale < 1e-7 and np.abs(got[:, 0:9] - b_in).max() < 4e-7      # (the bounds of test_device_undeformed_wave_early_exit)
    if lj70 < 0:
        assert got[70, 18] == 0.0 and exL[70] == 0.0
        assert np.abs(np.delete(got[:, 18], 70) - np.delete(exL, 70)).max() < 1e-7
    else:
        assert np.array_equal(got[:, 18].view(np.uint32), lj.view(np.uint32)) and np.abs(exL - lj.astype(np.float64)).max() < 1e-12      # (the dust's strain is 1e-20)
        assert np.all(got[:, 9:18] == 0.0) and np.abs(got[:, 0:9] - b_in).max() < 1e-12


def test_nacc_without_beta_takes_the_full_path_when_undeformed():
    """NACC with beta = 0 (p_min = 0 = p_trial: the early exit's premise "p_trial lies strictly inside" does not hold, the vote is off): the full
    path must give what the closed form gives - case 0, zero stress, log Jp untouched."""
    hip = _ffi.load_hip()
    p = mv.params(hip, NACC, dict(beta=0.0))
    F, lj = undeformed_rows(), np.full(N_WAVE, float(p.log_jp0), np.float32)
    got = mv.stress_rows(hip, NACC, p, F, lj)
    exF, exPF, exL, case = mv.exact(NACC, p, F, lj)
    scale = p.volume * p.youngs_modulus
    assert (case == 0).all() and np.abs(exPF).max() / scale < 1e-8 and np.array_equal(exL, lj.astype(np.float64))
    print("max |P F^T| / (vol E)", np.abs(got[:, 9:18]).max() / scale, "max |b - b_in|", np.abs(got[:, 0:9] - mv.bform(F)).max(), "log Jp", got[0, 18], "in", lj[0])
    assert np.abs(got[:, 9:18]).max() / scale < 1e-7 and np.abs(got[:, 0:9] - mv.bform(F)).max() < 4e-7
    assert np.array_equal(got[:, 18].view(np.uint32), lj.view(np.uint32))


@pytest.mark.parametrize("material", [FC, SAND, NACC])
def test_one_reflected_lane_in_an_undeformed_wave(material):
    """F = diag(1, 1, -1) in lane 70 of an otherwise undeformed wave: the early exit is voted down by that lane alone.  The other 255 lanes stay
    at zero stress (the bounds of test_device_undeformed_wave_early_exit).  The reflected lane: sand - the closed form (|S| enters: the tip with
    zero strain, b = I, the reflection gone from the state); NACC - the oracle's finite / non-finite pattern (powf(Je < 0, -2/3) is NaN in the
    reference); fixed-corotated - the closed form.  b = I does not say WHICH stretch is the negative one (diag(1, 1, -1) = R_x(pi) diag(1, -1, 1) =
    R_y(pi) diag(-1, 1, 1): three SVDs with "the sign on the smallest value", three stresses that differ by a permutation of the axes), so the
    fixed-corotated lane is held to the closed form's principal stresses {2 lambda, 2 lambda, 4 mu + 2 lambda} vol on the coordinate axes, in the
    closed form's order or permuted."""
    hip = _ffi.load_hip()
    p = mv.params(hip, material)
    F = undeformed_rows()
    F[70] = np.array([1, 0, 0, 0, 1, 0, 0, 0, -1], np.float32)
    lj = np.full(N_WAVE, float(p.log_jp0), np.float32)
    got = mv.stress_rows(hip, material, p, F, lj)
    ref = mv.stress_rows(oracle(), material, p, F, lj)
    keep = np.arange(N_WAVE) != 70
    scale = p.volume * p.youngs_modulus
    b_in = mv.bform(F)
    print("other lanes: max |P F^T| / (vol E)", np.abs(got[keep, 9:18]).max() / scale, "max |b - b_in|", np.abs(got[keep, 0:9] - b_in[keep]).max())
    assert np.abs(got[keep, 9:18]).max() / scale < 1e-7 and np.abs(got[keep, 0:9] - b_in[keep]).max() < 4e-7 and np.abs(got[keep, 18] - lj[keep]).max() < 1e-7
    with np.errstate(all="ignore"):
        exF, exPF, exL, _ = mv.exact(material, p, F, lj if material != FC else None)
    print("lane 70: device P F^T / (vol E)", (got[70, 9:18] / scale).tolist(), "closed form", (exPF[70] / scale).tolist(), "oracle", (ref[70, 9:18] / scale).tolist())
    if material == NACC:
        assert np.array_equal(np.isfinite(got[70, 9:18]), np.isfinite(ref[70, 9:18])) and np.isfinite(got[70, 18]) == np.isfinite(ref[70, 18])
        assert np.array_equal(np.isfinite(got[70, 0:9]), np.isfinite(mv.bform(ref[70:71, 0:9])[0]))
    elif material == SAND:
        fails = against_closed_form(SAND, p, F, lj, got, np.array([70]), "reflected sand lane")
        assert not fails, fails
    else:
        d_dev, d_ex = got[70, 9:18].reshape(3, 3).astype(np.float64), exPF[70].reshape(3, 3)
        off = ~np.eye(3, dtype=bool)
        assert np.abs(d_dev[off]).max() / scale <= 3e-6 and np.abs(d_ex[off]).max() / scale < 1e-9
        e = np.abs(np.sort(np.diag(d_dev)) - np.sort(np.diag(d_ex))).max() / scale
        e_ref = np.abs(np.sort(np.diag(ref[70, 9:18].reshape(3, 3).astype(np.float64))) - np.sort(np.diag(d_ex))).max() / scale
        print("principal stresses: device off by", e, "oracle by", e_ref)
        assert e <= 2.0 * e_ref + 3e-6


def test_sand_without_stiffness_takes_the_dead_path():
    """Sand with youngs_modulus = 0 (mu = 0) on the G3 inputs.  Tip rows: finite, the closed form (b = I, zero stress, the tip's log Jp).  Every other
    row is the reference's logf(0) path: P F^T is non-finite exactly where the oracle's is, b and log Jp come back as they went in (b: the float
    product F F^T, within 1e-6 relative).  The oracle is the reference for the pattern."""
    hip = _ffi.load_hip()
    p = mv.params(hip, SAND, dict(youngs_modulus=0.0))
    F, lj = mv.inputs(SAND)
    got = mv.stress_rows(hip, SAND, p, F, lj)
    ref = mv.stress_rows(oracle(), SAND, p, F, lj)
    idx = np.arange(F.shape[0])
    with np.errstate(all="ignore"):
        exF, exPF, exL, branch = mv.exact(SAND, p, F, lj)
        ok = (idx % 8 <= 5) & mv.stable_rows(SAND, p, F, lj)
    tip, dead = ok & (branch == 2), ok & (branch != 2)
    print("rows", int(ok.sum()), "tip", int(tip.sum()), "dead", int(dead.sum()))
    assert tip.sum() >= 100 and dead.sum() >= 100
    # tip rows
    assert np.isfinite(got[tip]).all() and np.isfinite(ref[tip]).all()
    f_dev = np.abs(got[tip, 0:9] - mv.bform(exF[tip])).max(axis=1)
    f_ref = np.abs(mv.bform(ref[tip, 0:9]) - mv.bform(exF[tip])).max(axis=1)
    dl = np.abs(got[tip, 18].astype(np.float64) - exL[tip])
    print("tip: max |P F^T|", np.abs(got[tip, 9:18]).max(), "b worst", f_dev.max(), "oracle", f_ref.max(), "log Jp worst", dl.max())
    assert np.all(got[tip, 9:18] == 0.0) and np.all(exPF[tip] == 0.0)                    # no stiffness, no stress: there is no scale to be relative to
    assert f_dev.max() < 1e-5 and (f_dev <= 2.0 * f_ref + mv.B_SLACK[SAND]).all() and dl.max() <= mv.LOGJP_BOUND[SAND]
    # the dead rows
    nf_dev, nf_ref = ~np.isfinite(got[:, 9:18]).all(axis=1), ~np.isfinite(ref[:, 9:18]).all(axis=1)
    print("dead: non-finite P F^T rows: device", int(nf_dev[dead].sum()), "oracle", int(nf_ref[dead].sum()), "of", int(dead.sum()))
    assert np.array_equal(nf_dev[dead], nf_ref[dead]) and nf_ref[dead].all()
    b_in = mv.bform(F)
    rel = np.abs(got[dead, 0:9] - b_in[dead]).max(axis=1) / np.maximum(1.0, np.abs(b_in[dead]).max(axis=1))
    print("dead: b against F F^T, worst relative", rel.max())
    assert rel.max() <= 1e-6
    assert np.array_equal(got[dead, 18].view(np.uint32), lj[dead].view(np.uint32))


# ---- block level ---------------------------------------------------------------------------------------------------------------------------
def check_variant(bench, res, models, tier, where, tag):
    """check() of tests/test_g2p2g_blocks_gpu.py with the bounds of the variants: where[i] = (variant id or None, scene) of model i"""
    def bound_of(i, q, t, material):
        vid, scene = where[i]
        return gm.bound(q, t, material) if vid is None else mv.block_bound(vid, scene, t, q, material)
    check(bench, res, models, tier, tag, bound_of=bound_of)


def run_block(parts, tiers, tag):
    """parts: [(variant id or None, scene)].  One bench, per tier one injection, one step, one check."""
    specs = []
    for vid, scene in parts:
        material, over = mv.block_overrides(vid) if vid is not None else (SAND, gm.material_overrides(SAND))
        pos, st = gm.scene_state(scene, material, overrides=over if vid is not None else None)
        specs.append((material, over, pos, st))
    bench = Bench([(m, pos) for m, _, pos, _ in specs], overrides=[o for _, o, _, _ in specs])
    try:
        for tier in tiers:
            bench.inject([st for _, _, _, st in specs], lambda keys: gm.grid_of(keys, tier))
            res = bench.step()
            models = [gm.step(c, pos, gm.gather_field(pos, tier), b6=st["b6"], reflected=st["reflected"], logjp=st["logjp"], J=st["J"]) for c, (_, _, pos, st) in zip(bench.consts, specs)]
            check_variant(bench, res, models, tier, parts, tag)
    finally:
        bench.close()


@pytest.mark.parametrize("vid", [v[0] for v in mv.BLOCK_VARIANTS])
def test_block_sizes_at_the_variant(vid):
    """One block per size 1 .. 1024 (4616 particles) on the flow tier: rows beyond a block's first bin, partial iterations, the merged tail."""
    run_block([(vid, "block_sizes")], ["flow"], f"{vid} block sizes")


@pytest.mark.parametrize("vid", [v[0] for v in mv.BLOCK_VARIANTS])
def test_neighbour_blocks_at_the_variant(vid):
    """The 2 x 2 x 2 cluster (1579 particles) on flow and fast: shared grid blocks and the shell path."""
    run_block([(vid, "cluster")], ["flow", "fast"], f"{vid} cluster")


def test_two_sand_models_with_different_parameters_in_the_same_blocks():
    """Sand at the defaults and sand at S3 in the same blocks of the cluster (laid out as test_mixed_materials_in_the_same_blocks lays out its two
    models): constants cached per material instead of per model would give one of them the other's."""
    vid, scene, tier = mv.MIXED
    run_block([(None, "cluster"), (vid, scene)], [tier], "mixed sand")


# ---- both kernels ----------------------------------------------------------------------------------------------------------------------------
def test_both_kernels_pass_this_file():
    """Everything above runs in process with the default mask (the pair kernel).  This test runs the file again in a fresh child process with
    MPM_G2P2G_PAIRS=0 - the one-particle-per-lane kernel - under a time limit, deselecting itself there.  A child that ends on a signal or at its
    limit fails the test, and nothing else is started."""
    env = dict(os.environ, MPM_G2P2G_PAIRS="0")
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "not test_both_kernels_pass_this_file"], env=env, capture_output=True, text=True, cwd=os.path.dirname(HERE))
    tail = r.stdout[-3000:]
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), ("the child ended on a signal or at its time limit", r.returncode, tail, r.stderr[-1500:])
    assert r.returncode == 0 and " passed" in tail and "failed" not in tail, (r.returncode, tail, r.stderr[-1500:])

"""Force fields, CPU side: the ABI surface, the x86 build of claymore_amd/csrc/mpm_force_field.hpp (tools/hostcheck/check_forces.cpp) against
the float32 model of tests/force_field_model.py bit for bit, that model against the float64 closed forms with bounds counted from the
statements' roundings, the weights at a region's edge, the corner cases (d == 0, DRAG with s = 0 and with a huge s), slot order, every refusal
of the validator, and the install / remove rule of a scene's "forces" (host/force_rule.hpp through host_selftest against scenes.ForceEntry).
(The ISA of the kernels: tests/test_force_field_isa.py; the kernels themselves: tests/test_force_field_gpu.py.)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collision_shape_model as sm
import force_field_model as fm
import grid_update_model as gm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

DX = fm.DX
U = 2.0 ** -24                      # unit roundoff of float32: one rounding changes a value by at most U of its magnitude
SLACK = 1.01                        # the second-order terms (products of roundings) of every bound below


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def ffi_field(f):
    """A model field as the ABI struct, with what the caller hands over (the axis and a half-space normal not normalised)."""
    s = _ffi.ForceField()
    if f is None:
        return s
    s.kind, s.falloff = f["kind"], f["falloff"]
    for d in range(3):
        s.vec[d], s.centre[d] = float(f["vec_given"][d]), float(f["centre"][d])
    s.strength, s.swirl, s.pull, s.lift, s.soft, s.feather = (float(f[k]) for k in ("strength", "swirl", "pull", "lift", "soft", "feather"))
    r = f["region"]
    if r is not None:
        s.region.kind, s.region.inside_out, s.region.radius = r["kind"], int(r["inside_out"]), float(r["radius"])
        for d in range(3):
            s.region.a[d], s.region.b[d] = float(r["a"][d]), float(r["b_given"][d])
    return s


def ffi_fields(fields):
    arr = (_ffi.ForceField * max(1, len(fields)))()
    for i, f in enumerate(fields):
        arr[i] = ffi_field(f)
    return arr


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_force_field_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert "int mpm_set_force_field(mpm_ctx* ctx, int slot, const mpm_force_field* f);" in hdr
    assert "int mpm_get_force_field(mpm_ctx* ctx, int slot, mpm_force_field* out);" in hdr
    assert re.search(r"int mpm_test_force_field\(const mpm_force_field\* fields, int n_fields, float dt, float dx, const float\* xyz, const float\* mp4, size_t n, float\* out4, int device\);", hdr)
    assert "MPM_FORCE_UNIFORM = 1, MPM_FORCE_POINT, MPM_FORCE_VORTEX, MPM_FORCE_DRAG" in hdr and "MPM_MAX_FORCE_FIELDS = 4" in hdr
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    for name in ("set_force_field", "get_force_field", "test_force_field"):
        assert re.search(rf"\bT mpm_{name}$", out, re.M), f"mpm_{name} is not exported"
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES
    api = _ffi.load_hip()
    assert api.set_force_field.argtypes[1] is C.c_int and len(api.set_force_field.argtypes) == 3 and len(api.test_force_field.argtypes) == 9
    assert C.sizeof(_ffi.ForceField) == 4 * (2 + 3 + 3 + 6 + 14 + 6) and _ffi.ForceField.region.offset == 4 * 14
    assert (_ffi.FORCE_UNIFORM, _ffi.FORCE_POINT, _ffi.FORCE_VORTEX, _ffi.FORCE_DRAG, _ffi.MAX_FORCE_FIELDS) == (1, 2, 3, 4, 4)
    assert callable(Engine.set_force_field) and callable(Engine.force_fields)
    assert " abi7 " in api.build_info().decode()


# ---- 2. the x86 build against the float32 model -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_forces(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostforces.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tools", "hostcheck"),
                           "-I" + entry.CSRC, "-o", out, os.path.join(ROOT, "tools", "hostcheck", "check_forces.cpp")])
    lib = C.CDLL(out)
    lib.host_force_cell.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def host_cell(lib, fields, dt, X, mp4):
    X, mp4 = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(mp4, dtype=np.float32)
    out = np.empty_like(mp4)
    assert lib.host_force_cell(C.byref(ffi_fields(fields)), len(fields), float(dt), ptr(X), ptr(mp4), len(X), ptr(out)) == 0
    return out


def assert_cells_equal(got, want, acted, mp4):
    """Mass and rows no slot acted on: the input's bits; computed momenta: equal with every NaN one NaN (grid_update_model's note)."""
    assert np.array_equal(gm.bits(got[:, 0]), gm.bits(mp4[:, 0])), "the mass changed"
    assert np.array_equal(gm.bits(got[~acted]), gm.bits(mp4[~acted])), "a row with w == 0 changed"
    bad = gm.canon(got) != gm.canon(want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist())


CASES = fm.case_list()
FOUR = [fm.make("uniform", "box", feather=fm.FEATHER), fm.make("drag", "sphere"), fm.make("vortex", "capsule", inside_out=True), fm.make("point1", "halfspace")]


@pytest.mark.parametrize("dt", [1e-4, 0.0])
@pytest.mark.parametrize("name,f", CASES, ids=[c[0] for c in CASES])
def test_host_build_equals_the_float32_model_bit_for_bit(host_forces, name, f, dt):
    """force_cell of the x86 build against the model on force_field_model.adversarial_points: seeded points and nodes, the special points of the
    region (faces, edges, corners, centres, NaN coordinates) and points half-way through and at the end of the feather, the field's centre
    (d == 0); {m, p} of every class of grid_update_model.generate's full tier: denormal and huge momenta, +-0, inf, NaN, masses ordinary,
    FLT_MIN, denormal, inf and the skipped classes (force_cell itself does not look at the sign of the mass)."""
    X, mp4 = fm.adversarial_points([f], 3)
    want, acted = fm.force_cell([f], X, dt, mp4)
    got = host_cell(host_forces, [f], dt, X, mp4)
    assert_cells_equal(got, want, acted, mp4)
    if f["region"] is not None:
        assert 0.02 < acted.mean() < 0.98, acted.mean()
    else:
        assert acted.all()


def test_host_build_four_slots_and_empty_slots(host_forces):
    fields_sets = [FOUR, [FOUR[1], None, FOUR[0]], [None, None, None, FOUR[2]], [], [None]]
    for fields in fields_sets:
        X, mp4 = fm.adversarial_points(fields, 5)
        want, acted = fm.force_cell(fields, X, 1e-4, mp4)
        got = host_cell(host_forces, fields, 1e-4, X, mp4)
        assert_cells_equal(got, want, acted, mp4)
        if not any(fields):
            assert np.array_equal(gm.bits(got), gm.bits(mp4))


# ---- 3. the model against the float64 closed forms -----------------------------------------------------------------------------------------
def ordinary_points(seed, n=20000):
    rng = np.random.default_rng(seed)
    X = (rng.random((n, 3)) * 0.9 + 0.05).astype(np.float32)
    m = (2.0 ** rng.uniform(-20, -8, n)).astype(np.float32)
    p = (m[:, None] * rng.standard_normal((n, 3)) * 2).astype(np.float32)
    return X, m, p


@pytest.mark.parametrize("name", list(fm.KIND_CASES))
def test_model_against_the_float64_closed_forms(name):
    """One slot without a region (w = 1) at 20000 ordinary points, dt = float32(1e-4), against the closed form in float64 on the same float32
    inputs.  The bounds are counted, not measured; U = 2^-24 per rounding, t = m a w dt the impulse, |.| per component:
      UNIFORM  g, a g, m (a g), the sum: 3 U |t| + U |p'|                                         <= U (4 |t| + |p|)
      POINT    r_i 1; r_i r_i 3; two sums 5; soft^2 and its sum 6 = d2; d 6/2 + 1 = 4; falloff 0: r / d 1 + 4 + 1, strength 7; falloff 1:
               r / d2 1 + 6 + 1, strength 9; falloff 2: d2 d 11, r / (d2 d) 13, strength 14 = A;  then as UNIFORM: U ((A + 4) |t| + |p|)
      VORTEX   cancellation in rp and the cross product: absolute bounds in rho = |r|_1 (n a unit vector, |n_i| <= 1).  h: 4 U rho; rp_i: 8 U rho,
               |rp_i| <= 2 rho; c_i: 24 U rho, |c_i| <= 4 rho; a_i: E_a = U (36 |swirl| rho + 14 |pull| rho + 2 |lift|), |a_i| <= A = 4 |swirl| rho +
               2 |pull| rho + |lift|; then |m g| (E_a + 3 U A) + U (|p| + |m g| A)
      DRAG     s 2; T = s (m vec) 4; numerator 4 U |T| + U (|p| + |T|); 1 + s 3; the quotient 1:  U ((5 |T| + |p|) / (1 + s) + 4 |p'|)"""
    f = fm.make(name)
    X, m, p = ordinary_points(17)
    dt = np.float32(1e-4)
    got, _ = fm.apply_one(f, X, dt, m, p)
    want = fm.closed_apply(f, X, dt, m, p, w=np.ones(len(X)))
    err = np.abs(got.astype(np.float64) - want)
    m64, p64 = m.astype(np.float64)[:, None], np.abs(p.astype(np.float64))
    if f["kind"] == fm.DRAG:
        s = float(f["strength"]) * float(dt)
        T = np.abs(s * m64 * f["vec"].astype(np.float64)[None])
        bound = U * ((5 * T + p64) / (1 + s) + 4 * np.abs(want))
    elif f["kind"] == fm.VORTEX:
        rho = np.abs(X.astype(np.float64) - f["centre"].astype(np.float64)).sum(axis=1)[:, None]
        sw, pu, li = (abs(float(f[k])) for k in ("swirl", "pull", "lift"))
        A = 4 * sw * rho + 2 * pu * rho + li
        Ea = 36 * sw * rho + 14 * pu * rho + 2 * li
        bound = U * (m64 * float(dt) * (Ea + 4 * A) + p64)
    else:
        t = np.abs(m64 * fm.closed_acceleration(f, X) * float(dt))
        A = {fm.UNIFORM: 0, fm.POINT: (7, 9, 14)[f["falloff"]]}[f["kind"]]
        bound = U * ((A + 4) * t + p64)
    ratio = (err / (SLACK * bound + 1e-300)).max()
    print(f"{name}: max |model - closed form| / bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert (np.abs(got.astype(np.float64) - p) > 0).mean() > 0.5          # the field does something at this dt


# ---- 4. weights ---------------------------------------------------------------------------------------------------------------------------
def test_weights_at_inside_and_outside_an_edge_and_across_the_feather(host_forces):
    """The half-space y <= 32 dx (axis normal: sdis = y - 32 dx exactly).  feather 0: w = 1 on the plane and inside, 0 outside.  feather 3 dx:
    w = 0 on the plane and outside, (depth / feather) inside - 1/3, 1/2, 2/3 at depths 1, 1.5, 2 dx -, 1 from depth 3 dx on.  Inside out:
    the complement, with the plane still counted in.  The x86 build gives the same momenta as the model at every one of these points."""
    ys = np.array([33, 32.5, 32, 31, 30.5, 30, 29, 28, 10], np.float64) * DX
    X = np.stack([np.full_like(ys, 0.3), ys, np.full_like(ys, 0.7)], axis=1).astype(np.float32)
    hard, soft = fm.make("uniform", "halfspace"), fm.make("uniform", "halfspace", feather=fm.FEATHER)
    assert fm.weight(hard, X).tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1]
    w = fm.weight(soft, X)
    assert w[:3].tolist() == [0, 0, 0] and w[5:].tolist() == [np.float32(2) / np.float32(3), 1, 1, 1] and w[4] == 0.5 and w[3] == np.float32(1) / np.float32(3)
    assert np.allclose(w, fm.closed_weight(soft, X), atol=2 * U)
    assert fm.weight(fm.make("uniform", "halfspace", inside_out=True), X).tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]
    nan = np.array([[np.nan, 0.2, 0.2]], np.float32)
    for reg in fm.REGIONS:
        for fe in (0.0, fm.FEATHER):
            assert fm.weight(fm.make("uniform", reg, feather=fe), nan)[0] == 0, "a NaN sdis must give w = 0"
    mp4 = np.tile(np.array([[0.25, 1.0, -2.0, 0.5]], np.float32), (len(X), 1))
    for f in (hard, soft):
        want, acted = fm.force_cell([f], X, 1e-3, mp4)
        assert_cells_equal(host_cell(host_forces, [f], 1e-3, X, mp4), want, acted, mp4)
        assert np.array_equal(acted, fm.weight(f, X) != 0)
        # the impulse is proportional to the weight: p' - p = m a (w dt)
        # (p' is rounded at its own magnitude, |p'| <= 2.1 here: U |p'| and three roundings of the impulse)
        dp = want[:, 1:].astype(np.float64) - mp4[:, 1:]
        t = 0.25 * f["vec"].astype(np.float64)[None] * float(np.float32(1e-3)) * fm.weight(f, X)[:, None]
        assert (np.abs(dp - t) <= SLACK * U * (2.1 + 3 * np.abs(t))).all()


# ---- 5. corner cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["point0", "point1", "point2"])
def test_point_field_at_its_centre(host_forces, name):
    """d == 0 (the node on the centre, soft = 0) gives a = 0: the momentum keeps its value (p + m (0 g) = p for a finite m) and nothing is
    divided by zero; with soft > 0 the centre has r = 0 and a = 0 through 0 / soft."""
    f = fm.make(name, soft=0.0)
    X = np.stack([f["centre"], f["centre"] + np.float32(DX)]).astype(np.float32)
    mp4 = np.array([[0.5, 1.0, -2.0, 3.0]] * 2, np.float32)
    want, acted = fm.force_cell([f], X, 1e-2, mp4)
    assert acted.all() and np.array_equal(gm.bits(want[0]), gm.bits(mp4[0])) and not np.array_equal(gm.bits(want[1]), gm.bits(mp4[1]))
    assert np.isfinite(want).all()
    assert np.array_equal(gm.bits(host_cell(host_forces, [f], 1e-2, X, mp4)), gm.bits(want))
    g = fm.make(name, soft=2 * DX)
    assert np.array_equal(gm.bits(fm.force_cell([g], X[:1], 1e-2, mp4[:1])[0]), gm.bits(mp4[:1]))


def test_drag_with_no_step_and_with_a_huge_rate(host_forces):
    """s = 0 (dt = 0, or strength = 0): p' = (p + 0) / 1 = p.  A huge s: p' -> m vec, monotonically, never past it (implicit Euler is
    unconditionally stable): |p' - m vec| = |p - m vec| / (1 + s) up to rounding."""
    X, m, p = ordinary_points(23, 4096)
    mp4 = np.concatenate([m[:, None], p], axis=1)
    for f, dt in ((fm.make("drag"), 0.0), (fm.make("drag", strength=0.0), 1e-4)):
        want, acted = fm.force_cell([f], X, dt, mp4)
        assert acted.all() and np.array_equal(gm.bits(want), gm.bits(mp4))
        assert np.array_equal(gm.bits(host_cell(host_forces, [f], dt, X, mp4)), gm.bits(want))
    target = m.astype(np.float64)[:, None] * fm.KIND_CASES["drag"]["vec"]
    last = np.abs(p - target)
    for k in (1e2, 1e6, 1e12, 1e30):
        f = fm.make("drag", strength=k)
        want, _ = fm.force_cell([f], X, 1e-4, mp4)
        assert np.array_equal(gm.bits(host_cell(host_forces, [f], 1e-4, X, mp4)), gm.bits(want))
        gap = np.abs(want[:, 1:].astype(np.float64) - target)
        s = float(np.float32(np.float32(k) * np.float32(1e-4)))
        assert np.isfinite(want).all()
        assert (gap <= np.abs(p - target) / (1 + s) + 8 * U * (np.abs(target) + np.abs(p) / (1 + s))).all()
        assert (gap <= last + 8 * U * np.abs(target)).all()
        last = gap
    assert (last <= 8 * U * np.abs(target)).all()                         # s = 1e26: p' = m vec to rounding


def test_slot_order_matters_for_drag_and_not_for_two_uniform_fields():
    """DRAG then UNIFORM differs from UNIFORM then DRAG by the damping of the uniform impulse, (m a dt) s / (1 + s), which the model shows.  Two UNIFORM fields commute up to the association of the two additions: (p + t1) + t2 against (p + t2) + t1, at most U (|p + t1| + |p + t2| + 2 |p'|)."""
    X, m, p = ordinary_points(29, 4096)
    mp4 = np.concatenate([m[:, None], p], axis=1)
    dt = np.float32(1e-3)
    d, u1, u2 = fm.make("drag"), fm.make("uniform"), fm.make("uniform", vec=(-3.0, 1.5, 0.125))
    a, _ = fm.force_cell([d, u1], X, dt, mp4)
    b, _ = fm.force_cell([u1, d], X, dt, mp4)
    assert (gm.bits(a[:, 1:]) != gm.bits(b[:, 1:])).mean() > 0.9
    s = float(d["strength"]) * float(dt)
    want = m.astype(np.float64)[:, None] * u1["vec"].astype(np.float64) * float(dt) * s / (1 + s)
    # (either order rounds a handful of times at the magnitude of its momenta: DRAG's bound of test_model_against_the_float64_closed_forms plus UNIFORM's)
    assert (np.abs(a[:, 1:].astype(np.float64) - b[:, 1:] - want) <= 10 * U * (np.abs(a[:, 1:]) + np.abs(b[:, 1:]) + np.abs(p))).all()
    assert (np.abs(want) > 100 * U * np.abs(p)).mean() > 0.5              # ... and the difference is far above that
    a, _ = fm.force_cell([u1, u2], X, dt, mp4)
    b, _ = fm.force_cell([u2, u1], X, dt, mp4)
    one, _ = fm.force_cell([u1], X, dt, mp4)
    two, _ = fm.force_cell([u2], X, dt, mp4)
    bound = U * (np.abs(one[:, 1:]) + np.abs(two[:, 1:]) + 2 * np.abs(a[:, 1:])).astype(np.float64) * SLACK
    assert (np.abs(a[:, 1:].astype(np.float64) - b[:, 1:]) <= bound).all()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def validator_rc(api, fields):
    """mpm_test_force_field validates its fields as mpm_set_force_field does before it touches a device: MPM_ERR_INVALID for a refused field;
    for an accepted one it goes on to the device (MPM_OK with a GPU, MPM_ERR_DEVICE without)."""
    X, mp4 = np.zeros((1, 3), np.float32), np.ones((1, 4), np.float32)
    out = np.empty_like(mp4)
    return api.test_force_field(fields, len(fields), 1e-4, DX, ptr(X), ptr(mp4), 1, ptr(out), 0)


def bad_fields():
    nan, inf = float("nan"), float("inf")

    def with_(base, **kw):
        f = ffi_field(fm.make(base, "box", feather=fm.FEATHER))
        for k, v in kw.items():
            obj, path = f, k.split("__")
            for part in path[:-1]:
                obj = getattr(obj, part)
            cur = getattr(obj, path[-1])
            if hasattr(cur, "__len__"):
                for i, x in enumerate(v):
                    cur[i] = x
            else:
                setattr(obj, path[-1], v)
        return f
    yield "kind 5", with_("uniform", kind=5)
    yield "kind -1", with_("uniform", kind=-1)
    yield "falloff 3", with_("point0", falloff=3)
    yield "falloff -1", with_("point0", falloff=-1)
    for name in ("vec", "centre"):
        yield f"NaN {name}", with_("uniform", **{name: (0.0, nan, 0.0)})
        yield f"inf {name}", with_("vortex", **{name: (inf, 1.0, 0.0)})
    for name in ("strength", "swirl", "pull", "lift", "soft", "feather"):
        yield f"NaN {name}", with_("point1", **{name: nan})
        yield f"inf {name}", with_("point1", **{name: inf})
    yield "zero axis", with_("vortex", vec=(0.0, 0.0, 0.0))
    yield "drag strength < 0", with_("drag", strength=-1.0)
    yield "soft < 0", with_("point1", soft=-1e-3)
    yield "feather < 0", with_("uniform", feather=-1e-3)
    yield "region kind 7", with_("uniform", region__kind=7)
    yield "region box half extent 0", with_("uniform", region__b=(0.1, 0.0, 0.1))
    yield "region NaN a", with_("uniform", region__a=(nan, 0.0, 0.1))
    yield "region inf a", with_("uniform", region__a=(inf, 0.0, 0.1))
    yield "region sphere radius 0", with_("uniform", region__kind=2, region__radius=0.0)
    yield "region capsule a == b", with_("uniform", region__kind=4, region__radius=0.1, region__a=(0.5, 0.5, 0.5), region__b=(0.5, 0.5, 0.5))
    yield "region half-space zero normal", with_("uniform", region__kind=1, region__b=(0.0, 0.0, 0.0))
    yield "reserved", with_("uniform", reserved=(0, 0, 1, 0, 0, 0))


def test_every_refusal():
    api = _ffi.load_hip()
    for name, f in CASES:
        rc = validator_rc(api, ffi_fields([f]))
        assert rc in (_ffi.MPM_OK, _ffi.MPM_ERR_DEVICE), (name, rc)               # every field the tests use is accepted
    seen = 0
    for what, f in bad_fields():
        arr = (_ffi.ForceField * 1)(f)
        assert validator_rc(api, arr) == _ffi.MPM_ERR_INVALID, what
        seen += 1
    assert seen >= 30
    good = ffi_fields(FOUR)
    assert validator_rc(api, good) in (_ffi.MPM_OK, _ffi.MPM_ERR_DEVICE)
    five = (_ffi.ForceField * 5)(*([good[0]] * 5))
    X = np.zeros((1, 3), np.float32)
    assert api.test_force_field(five, 5, 1e-4, DX, ptr(X), ptr(X), 1, ptr(X), 0) == _ffi.MPM_ERR_INVALID
    assert api.test_force_field(good, -1, 1e-4, DX, ptr(X), ptr(X), 1, ptr(X), 0) == _ffi.MPM_ERR_INVALID
    # without a context nothing is installed: mpm_set_force_field / mpm_get_force_field answer MPM_ERR_INVALID and touch nothing
    assert api.set_force_field(None, 0, C.byref(good[0])) == _ffi.MPM_ERR_INVALID and api.set_force_field(None, 4, None) == _ffi.MPM_ERR_INVALID
    assert api.get_force_field(None, 0, C.byref(_ffi.ForceField())) == _ffi.MPM_ERR_INVALID


# ---- 7. the install / remove rule of a scene's "forces" -------------------------------------------------------------------------------------
RULE_CASES = [
    ({"start": 0.0, "end": 0.003}, [0.0, 0.001, 0.002, 0.003, 0.004]),                        # installed at t == start, removed at t == end
    ({"start": 0.002, "end": 0.004}, [0.0, 0.0019999, 0.002, 0.003, 0.0039999, 0.004, 0.01]),
    ({"start": 0.002, "end": 0.002}, [0.0, 0.002, 0.003]),                                    # start == end: never installed
    ({"start": 0.001}, [0.0, 0.001, 1.0, 1e9]),                                               # no end: stays
    ({}, [0.0, 1.0]),
    ({"start": 0.002, "end": 0.0021}, [0.0, 0.001, 0.0015, 0.0022, 0.003]),                   # a window no boundary falls into: never installed
    ({"start": 0.5, "end": 0.1}, [0.0, 0.3, 0.6]),
]


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("force") / "host_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "claymore_amd", "host", "host_selftest.cpp")])
    return exe


@pytest.mark.parametrize("times,ts", RULE_CASES)
def test_force_rule_in_cpp_equals_the_python_mirror(selftest, times, ts):
    """host/force_rule.hpp (through host_selftest --force) against scenes.ForceEntry.due on a list of boundary times: +1 install, -1 remove,
    0 nothing, boundary by boundary."""
    exe = selftest
    fe = scenes.ForceEntry.from_dict({"kind": "uniform", "vec": (0, -1, 0), **times})
    want = [fe.due(t) for t in ts]
    out = subprocess.check_output([exe, "--force", json.dumps(times)] + [repr(float(t)) for t in ts], text=True)
    got = [int(x) for x in out.split()]
    assert got == want, (times, ts, got, want)
    if times == RULE_CASES[0][0]:
        assert want == [1, 0, 0, -1, 0]
    if times.get("start") == times.get("end") and "start" in times:
        assert want == [0] * len(ts)


def test_new_scenes_carry_forces():
    for sc in (scenes.sand_in_wind(), scenes.stirred_tank()):
        assert sc["forces"] and all("kind" in f for f in sc["forces"]) and len(sc["forces"]) <= _ffi.MAX_FORCE_FIELDS
        for f in sc["forces"]:
            scenes.ForceEntry.from_dict(f)
    assert scenes.sand_in_wind()["forces"][0]["kind"] == "drag" and scenes.sand_in_wind()["forces"][0]["feather"] > 0
    st = scenes.stirred_tank()["forces"][0]
    assert st["kind"] == "vortex" and st["region"]["kind"] == "capsule" and np.isfinite(st["end"])

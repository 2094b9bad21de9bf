"""Analytic collision shapes, CPU side: the ABI surface, the x86 build of claymore_amd/csrc/mpm_collision_shapes.hpp (tools/hostcheck/check_shapes.cpp)
against the float32 model of tests/collision_shape_model.py bit for bit, that model's class against the float64 closed forms, the shape
response against the oracle's level-set response on a field sampled from the model.  (The ISA of the grid kernels: tests/test_grid_update_isa.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collision_shape_model as sm
import grid_update_model as gm
from claymore_amd import _ffi
from claymore_amd.engine import Engine
from oracle_ffi import oracle_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

N = 1 << gm.BITS
DX = sm.DX


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def ffi_pair(c):
    """A model collider as the two ABI structs."""
    obj, sh = _ffi.CollisionObject(), _ffi.CollisionShape()
    obj.type, obj.friction, obj.scale, obj.dsdt, obj.time = c["type"], float(c["friction"]), float(c["scale"]), float(c["dsdt"]), float(c["time"])
    for d in range(3):
        obj.trans[d], obj.trans_vel[d], obj.omega[d] = float(c["trans"][d]), float(c["trans_vel"][d]), float(c["omega"][d])
        sh.a[d], sh.b[d] = float(c["a"][d]), float(c["b_given"][d])
    for e in range(9):
        obj.rot_mat[e] = float(c["rot"][e])
    sh.kind, sh.inside_out, sh.radius = c["kind"], int(c["inside_out"]), float(c["radius"])
    return obj, sh


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_shape_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert re.search(r"int mpm_set_collision_shape\(mpm_ctx\* ctx, int slot, const mpm_collision_object\* obj, const mpm_collision_shape\* shape\);", hdr)
    assert re.search(r"int mpm_test_collision_shape\(const mpm_collision_object\* obj, const mpm_collision_shape\* shape, float time, float dx,", hdr)
    assert "MPM_SHAPE_HALFSPACE = 1, MPM_SHAPE_SPHERE = 2, MPM_SHAPE_BOX = 3, MPM_SHAPE_CAPSULE = 4" in hdr and "MPM_MAX_COLLISION_SHAPES = 4" in hdr
    assert "does NOT apply" in hdr                                                  # (query_sdf's box: said in the header)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    for sym in ("mpm_set_collision_shape", "mpm_test_collision_shape"):
        assert re.search(rf"\bT {sym}$", out, re.M), f"{sym} is not exported"
    for name in ("set_collision_shape", "test_collision_shape"):
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES
    api = _ffi.load_hip()
    assert api.set_collision_shape.argtypes[1] is C.c_int and len(api.set_collision_shape.argtypes) == 4 and len(api.test_collision_shape.argtypes) == 8
    assert C.sizeof(_ffi.CollisionShape) == 4 * (2 + 3 + 3 + 1 + 5)
    assert callable(Engine.set_collision_shape)
    assert " abi7 " in api.build_info().decode()


# ---- the x86 build ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_shapes(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostshapes.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tools", "hostcheck"),
                           "-I" + entry.CSRC, "-o", out, os.path.join(ROOT, "tools", "hostcheck", "check_shapes.cpp")])
    lib = C.CDLL(out)
    lib.host_shape_query.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.host_shape_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def host_query(lib, c, t, X):
    obj, sh = ffi_pair(c)
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(X), 7), np.float32)
    assert lib.host_shape_query(C.byref(obj), C.byref(sh), float(t), ptr(X), len(X), ptr(out)) == 0
    return out[:, 0], out[:, 1:4], out[:, 4:7]


def host_resolve(lib, c, t, nodes, vel):
    obj, sh = ffi_pair(c)
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    got = np.ascontiguousarray(vel, dtype=np.float32).copy()
    assert lib.host_shape_resolve(C.byref(obj), C.byref(sh), float(t), DX, ptr(nodes), len(nodes), ptr(got)) == 0
    return got


def domain_points_of(c, t, x):
    """Domain points X whose material points are (about) x: X = R (x - trans) / (scale inv) + shift, in float64."""
    p = sm.pose(c, t)
    R = p["rot"].astype(np.float64).reshape(3, 3)
    x0 = (np.asarray(x, np.float64) - c["trans"].astype(np.float64)) / float(c["scale"])
    return ((x0 @ R) / float(p["inv"]) + p["shift"].astype(np.float64)).astype(np.float32)


CASES = [(name, moved, io) for name in sm.KIND_CASES + ("halfspace_tilted",) for moved in (False, True) for io in (False, True)]


# ---- 2. the x86 build against the float32 model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,moved,inside_out", CASES)
def test_host_build_equals_the_float32_model_bit_for_bit(host_shapes, name, moved, inside_out):
    """Material point, sdis and n of the x86 build against the model on 4096 seeded domain points and the special points of
    collision_shape_model.special_points (a sphere's centre and a capsule's axis: n = 0; points on a surface: sdis == 0; box face ties and the
    box centre; the capsule's t clamped at both ends; NaN input), identity pose and the moved pose at T = 0.37, plain and inside_out; then the
    response (all three boundary types, friction 0 and 0.3) on the scene's nodes."""
    c = sm.make(name, moved, inside_out=inside_out)
    t = sm.T_MOVED if moved else 0.0
    sp = sm.special_points(c)
    X = np.concatenate([sm.seeded_points(7), sp if not moved else domain_points_of(c, t, sp)])
    sd, n, x = host_query(host_shapes, c, t, X)
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    sdm, nm = sm.query(c, xm)
    assert np.array_equal(gm.canon(x), gm.canon(xm))
    assert np.array_equal(gm.canon(sd), gm.canon(sdm)), np.argwhere(gm.canon(sd) != gm.canon(sdm))[:4].tolist()
    assert np.array_equal(gm.canon(n), gm.canon(nm)), np.argwhere(gm.canon(n) != gm.canon(nm))[:4].tolist()
    touched = sdm <= 0
    assert 0.02 < touched.mean() < 0.98 and not touched[np.isnan(sdm)].any() and np.isnan(sdm[-3:]).all()
    if not moved:                                                         # the special points are hit exactly only where x == X
        k = len(sp)
        s_sp, n_sp = sdm[-k:], nm[-k:]
        assert (s_sp == 0).any(), "no special point lies on the surface"
        if c["kind"] in (sm.SPHERE, sm.CAPSULE):
            assert ((n_sp == 0).all(axis=1) & (s_sp == (float(c["radius"]) if inside_out else -float(c["radius"])))).any(), "no point with n = 0"
        if c["kind"] == sm.BOX:
            assert (np.abs(n_sp[0]) == [0, 1, 0]).all() or (np.abs(n_sp[0]) == [0, 0, 1]).all() or (np.abs(n_sp[0]) == [1, 0, 0]).all()
    keys = gm.scene_keys()
    nodes = gm.node_coords(keys).transpose(0, 2, 1).reshape(-1, 3)
    vel = (np.random.default_rng(3).standard_normal((len(nodes), 3)) * 2).astype(np.float32)
    Xn = (nodes.astype(np.float32) * np.float32(DX)).astype(np.float32)
    for typ in (0, 1, 2):
        for fr in (0.0, 0.3):
            cc = {**c, "type": typ, "friction": np.float32(fr)}
            want, hit = sm.resolve(cc, t, Xn, vel)
            got = host_resolve(host_shapes, cc, t, nodes, vel)
            assert 0.05 < hit.mean() < 0.95
            assert np.array_equal(gm.canon(got), gm.canon(want)), (typ, fr, np.argwhere(gm.canon(got) != gm.canon(want))[:4].tolist())
            assert np.array_equal(got[~hit].view(np.uint32), vel[~hit].view(np.uint32))


def test_separate_returns_early_where_the_normal_is_zero(host_shapes):
    """A sphere's centre and a capsule's axis point on a node: n = 0, and SEPARATE leaves velocity 0 without adding the object's velocity back,
    as the level set's response does for a zero gradient; SLIP with n = 0 keeps the relative velocity."""
    for c in (sm.collider("sphere", a=(0.5, 0.5, 0.5), radius=0.1, type=2, trans_vel=(1.0, 0, 0)),
              sm.collider("capsule", a=(0.25, 0.5, 0.5), b=(0.75, 0.5, 0.5), radius=0.1, type=2, trans_vel=(1.0, 0, 0))):
        nodes = np.array([[32, 32, 32], [33, 32, 32]], np.int32)
        vel = np.array([[0.5, 0.25, -1.0]] * 2, np.float32)
        got = host_resolve(host_shapes, c, 0.0, nodes, vel)
        want, hit = sm.resolve(c, 0.0, (nodes * np.float32(DX)).astype(np.float32), vel)
        assert hit.all() and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (got[0] == 0).all()
        if c["kind"] == sm.SPHERE:
            assert (got[1] != 0).any()


# ---- 3. the model's class against the float64 closed forms -----------------------------------------------------------------------------------
# measured on the x86 build (identical to the float32 model, test 2) over 20000 seeded points per shape: (sdis in ulp32 of the extent, n in ulp32(1))
CLOSED_FORM_MEASURED = {"halfspace": (0.250, 0.0), "halfspace_tilted": (2.249, 0.359), "sphere": (1.997, 1.042), "box": (0.901, 14.730), "capsule": (2.303, 13.255)}
CLOSED_FORM_MARGIN = 2.0          # the asserted bound: twice the measured value


@pytest.mark.parametrize("name", sm.KIND_CASES + ("halfspace_tilted",))
def test_host_build_against_the_float64_closed_forms(host_shapes, name):
    """sdis and n of the x86 build at 20000 seeded material points (identity pose: x = X) against the closed forms of include/claymore_amd.h
    evaluated in float64 on the same float32 inputs.  Unit of sdis: ulp32 of the extent E = max(|a|, |b|, r, |x|) over shape and point, the
    magnitude the subtractions x - a work at; unit of n: ulp32(1) = 2^-23.  n is compared where the core is at least E / 64 away (|d| -> 0
    divides a rounding error of the extent's size by |d|), and for the box outside a band of 2 ulp32(E) around the planes where the branch
    (inside / outside, the largest q) changes.
    Measured (sdis, n): half-space with an axis normal 0.250 / 0 (n = b exactly), tilted half-space 2.249 / 0.359, sphere 1.997 / 1.042, box
    0.901 / 14.730 (outside near an edge, |max(q, 0)| is small against the extent), capsule 2.303 / 13.255.  Asserted: twice these."""
    c = sm.make(name)
    rng = np.random.default_rng(11)
    X = (rng.random((20000, 3)) * 1.5 - 0.25).astype(np.float32)
    sd, n, x = host_query(host_shapes, c, 0.0, X)
    assert np.array_equal(x.view(np.uint32), X.view(np.uint32))
    sd64, n64 = sm.closed_form(c, X)
    E = np.maximum(sm.extent(c), np.abs(X.astype(np.float64)).max(axis=1))
    u = gm.ulp32(E)
    es = np.abs(sd.astype(np.float64) - sd64) / u
    ok = np.ones(len(X), bool)
    if c["kind"] in (sm.SPHERE, sm.CAPSULE):
        ok = (sd64 + float(c["radius"])) >= E / 64
    if c["kind"] == sm.BOX:
        q = np.abs(X.astype(np.float64) - c["a"].astype(np.float64)) - c["b"].astype(np.float64)
        qs = np.sort(q, axis=1)
        ok = (np.abs(q).min(axis=1) > 2 * u) & (qs[:, 2] - qs[:, 1] > 2 * u)
        es = es[ok]
    en = np.abs(n.astype(np.float64) - n64).max(axis=1)[ok] / 2.0 ** -23
    print(f"{name}: sdis max {es.max():.3f} ulp32(extent), n max {en.max():.3f} ulp32(1) over {int(ok.sum())} points")
    assert ok.mean() > 0.9
    ms, mn = CLOSED_FORM_MEASURED[name]
    assert es.max() <= CLOSED_FORM_MARGIN * ms and en.max() <= CLOSED_FORM_MARGIN * mn, (es.max(), en.max())


# ---- 4. equivalence with the level-set path (the oracle) --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_ctx():
    api = oracle_api()
    cfg = _ffi.Config()
    assert api.default_config(gm.BITS, C.byref(cfg)) == 0
    ctx = C.c_void_p()
    assert api.create(C.byref(cfg), 0, C.byref(ctx)) == 0
    yield api, ctx, cfg
    api.destroy(ctx)


def oracle_resolve(api, ctx, c, field, nodes, vel):
    obj, _ = ffi_pair(c)
    f = [np.ascontiguousarray(field[0])] + [np.ascontiguousarray(field[1][d]) for d in range(3)]
    assert api.set_collision_object(ctx, C.byref(obj), ptr(f[0]), ptr(f[1]), ptr(f[2]), ptr(f[3])) == 0
    want = np.ascontiguousarray(vel, dtype=np.float32).copy()
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    assert api.raw.mpmo_fn_collision_resolve(ctx, ptr(nodes), len(nodes), 0.0, ptr(want)) == 0
    return want


ROUND_MEASURED = 1.751e-7          # sphere and capsule alike, SLIP and SEPARATE (STICKY: 0), relative to max(1, |v|max)
ROUND_BOUND = 2.0 * ROUND_MEASURED


@pytest.mark.parametrize("friction", [0.0, 0.3])
@pytest.mark.parametrize("typ", [0, 1, 2], ids=["sticky", "slip", "separate"])
@pytest.mark.parametrize("name", ["halfspace", "box", "sphere", "capsule"])
def test_shape_response_equals_the_oracles_level_set_response(host_shapes, oracle_ctx, name, typ, friction):
    """mpmo_fn_collision_resolve on a field sampled at the nodes from the float32 model, identity pose at bits 6 (a node's material position is
    node dx exactly and the interpolation returns the node's own sample), against the x86 build of the shape on the same nodes, restricted to
    query_sdf's box.  Half-space with an axis normal and box (gradient norm exactly 1): bit for bit.  Sphere and capsule: the same touched
    nodes and velocities within ROUND_BOUND - the level set normalises an already rounded unit normal again.  Measured: 1.751e-7 of
    max(1, |v|max) for sphere and capsule under SLIP and SEPARATE, 0 under STICKY; asserted: twice that."""
    api, ctx, cfg = oracle_ctx
    c = sm.make(name, type=typ, friction=friction, trans_vel=(0.25, -0.5, 0.125), omega=(0.5, 1.0, -0.25))   # (a moving surface, clock at 0)
    field = sm.sample_field(c, N, DX)
    lo, hi = 4 * cfg.boundary_blocks, N - 4 * cfg.boundary_blocks
    rng = np.random.default_rng(5)
    nodes = rng.integers(lo, hi, size=(6000, 3)).astype(np.int32)
    vel = (rng.standard_normal((len(nodes), 3)) * 2).astype(np.float32)
    want = oracle_resolve(api, ctx, c, field, nodes, vel)
    got = host_resolve(host_shapes, c, 0.0, nodes, vel)
    hit_o, hit_s = (want != vel).any(axis=1), (got != vel).any(axis=1)
    assert 0.1 < hit_s.mean() < 0.9
    if name in ("halfspace", "box"):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:4].tolist()
    else:
        assert np.array_equal(hit_o, hit_s)
        err = np.abs(got.astype(np.float64) - want).max() / max(1.0, np.abs(want).max())
        print(f"{name} type {typ} friction {friction}: max |shape - level set| = {err:.3e} (relative to max(1, |v|max))")
        assert err <= ROUND_BOUND, err

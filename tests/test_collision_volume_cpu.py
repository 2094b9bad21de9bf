"""The volume collider, CPU side: the ABI surface, the float32 model of tests/collision_volume_model.py against float64 trilinear interpolation,
the footprint rule, the x86 builds of claymore_amd/csrc/mpm_collision_volume.hpp (tools/hostcheck/check_volume.cpp and
claymore_amd/host/host_selftest.cpp --volume-query) against that model bit for bit, the auto-sizing rule of a mesh install, and the refusals the
library makes before it touches a device.  (The ISA of the kernels: tests/test_collision_volume_isa.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collision_mesh_model as cm
import collision_shape_model as sm
import collision_volume_model as vm
import grid_update_model as gm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

DX = sm.DX
HOSTCHECK = os.path.join(ROOT, "tools", "hostcheck")
HOST = os.path.join(ROOT, "claymore_amd", "host")
TABLES = ("ico", "2x2x2")
EPS = 2.0 ** -23


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def ffi_triple(c):
    """A model volume as the two ABI structs and the table."""
    obj, vol = _ffi.CollisionObject(), _ffi.CollisionVolume()
    obj.type, obj.friction, obj.scale, obj.dsdt, obj.time = c["type"], float(c["friction"]), float(c["scale"]), float(c["dsdt"]), float(c["time"])
    for d in range(3):
        obj.trans[d], obj.trans_vel[d], obj.omega[d] = float(c["trans"][d]), float(c["trans_vel"][d]), float(c["omega"][d])
        vol.dims[d], vol.origin[d] = c["table"].shape[d], float(c["origin"][d])
    for e in range(9):
        obj.rot_mat[e] = float(c["rot"][e])
    vol.spacing, vol.inside_out = float(c["spacing"]), int(c["inside_out"])
    return obj, vol, np.ascontiguousarray(c["table"], dtype=np.float32)


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_volume_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert "enum { MPM_VOLUME_MAX_SAMPLES = 1024 };" in hdr
    for decl in ("int mpm_set_collision_volume(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4);",
                 "int mpm_set_collision_volume_mesh(mpm_ctx* ctx, int slot, const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* verts, size_t nv, "
                 "const int32_t* tris, size_t nt);",
                 "int mpm_get_collision_volume(mpm_ctx* ctx, int slot, mpm_collision_volume* vol_out, const int lo[3], const int dims[3], float* out4);",
                 "int mpm_test_collision_volume(const mpm_collision_object* obj, const mpm_collision_volume* vol, const float* field4, float time, const float* xyz, size_t n, "
                 "float* out4, int device);"):
        assert decl in hdr, decl
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    for name in ("set_collision_volume", "set_collision_volume_mesh", "get_collision_volume", "test_collision_volume"):
        assert re.search(rf"\bT mpm_{name}$", out, re.M), f"mpm_{name} is not exported"
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES
    assert C.sizeof(_ffi.CollisionVolume) == 64 and _ffi.VOLUME_MAX_SAMPLES == 1024
    for m in ("set_collision_volume", "set_collision_volume_mesh", "collision_volume"):
        assert callable(getattr(Engine, m))
    assert " abi7 " in _ffi.load_hip().build_info().decode()


# ---- 2. the model against float64 ---------------------------------------------------------------------------------------------------------------
def affine_volume(dims=(7, 5, 9), origin=(0.1, -0.2, 0.3), spacing=0.0625):
    """sdis = a . p + b at the samples, g = a: trilinear interpolation reproduces an affine field exactly."""
    a, b = np.array([0.75, -0.5, 0.25]), -0.125
    p = vm.sample_points(origin, spacing, dims).astype(np.float64)
    T = np.concatenate([(p @ a + b)[:, None], np.broadcast_to(a, (len(p), 3))], axis=1).reshape(tuple(dims) + (4,))
    return vm.volume(T, origin=origin, spacing=spacing), a, b


def interp_bound(c, x):
    """Error bound of the four interpolated channels against exact trilinear interpolation of the float32 table, counted from the statements
    to first order in u = eps / 2, with M_c = max |t.c|, V_c = the largest difference of t.c between neighbouring samples, U = max(dims) - 1:
      xl: one subtraction, relative u of |xl| <= |x| + |origin|: a shift of xl / spacing by u (|x| + |o|) / spacing =: d_x cells per axis;
      dis = xl - cid spacing: the product rounds (u cid spacing), the difference rounds (u spacing): in cells u (U + 1); dis / spacing: u;
        1 - w: u - per axis a weight error of at most d_w = d_x + u (U + 3);  a weight shift of d moves a channel by at most V_c d, three axes;
      the two weight products 2 u, w * v u, the eight additions of partial sums <= M_c: 8 u                  -> 11 u M_c, taken as 6 eps M_c
      => d_c = 6 eps M_c + 3 V_c d_w."""
    T = c["table"].astype(np.float64)
    U = max(T.shape[:3]) - 1
    M = np.abs(T).max(axis=(0, 1, 2))
    V = np.max([np.abs(np.diff(T, axis=a)).max(axis=(0, 1, 2)) for a in range(3)], axis=0)
    u = EPS / 2
    d_x = u * (np.abs(x).max() + np.abs(c["origin"]).max()) / float(c["spacing"])
    return 6 * EPS * M + 3 * V * (d_x + u * (U + 3))


def test_model_equals_an_affine_field_and_a_spheres_interpolation_in_float64():
    """The model's trilinear query on an affine field - which trilinear interpolation reproduces exactly - against a . x + b in float64, and on
    a sphere's field against exact trilinear interpolation of the same float32 table, both within interp_bound; the normal of the affine
    field is a / |a| within 4 eps."""
    rng = np.random.default_rng(3)
    c, a, b = affine_volume()
    dims = np.array(c["table"].shape[:3])
    x = (c["origin"].astype(np.float64) + rng.random((5000, 3)) * (dims - 1) * float(c["spacing"])).astype(np.float32)
    sd, n = vm.query(c, x)
    ok = ~np.isnan(sd)
    assert ok.sum() > 4900
    bound = interp_bound(c, x)
    err = np.abs(sd[ok].astype(np.float64) - (x[ok].astype(np.float64) @ a + b))
    print("affine: sdis error", err.max() / EPS, "eps, bound", bound[0] / EPS)
    assert err.max() <= bound[0]
    assert np.abs(n[ok].astype(np.float64) - a / np.linalg.norm(a)).max() <= 4 * EPS + 3 * bound[1:].max()
    s = vm.sphere_volume(dims=(21, 21, 21), origin=(0.0, 0.0, -0.5), spacing=0.05)
    x = (s["origin"].astype(np.float64) + rng.random((5000, 3)) * 20 * 0.05).astype(np.float32)
    sd, n = vm.query(s, x)
    val, inside = vm.closed_form(s, x)
    ok = ~np.isnan(sd) & inside
    assert ok.sum() > 4900
    bound = interp_bound(s, x)
    err = np.abs(sd[ok].astype(np.float64) - val[ok, 0])
    print("sphere: sdis error", err.max() / EPS, "eps, bound", bound[0] / EPS)
    assert err.max() <= bound[0]
    g = val[ok, 1:]
    n64 = g / np.linalg.norm(g, axis=1)[:, None]
    glen = np.linalg.norm(g, axis=1).min()
    assert np.abs(n[ok].astype(np.float64) - n64).max() <= (4 * EPS + 3 * bound[1:].max()) / glen
    # and the interpolated distance is the sphere's within the interpolation error of a curved field: h^2 / (8 r_min) per axis
    r = np.linalg.norm(x[ok].astype(np.float64) - sm.make("sphere")["a"].astype(np.float64), axis=1)
    true = r - float(sm.make("sphere")["radius"])
    far = r > 0.1
    assert np.abs(sd[ok].astype(np.float64) - true)[far].max() <= 3 * 0.05 ** 2 / (8 * 0.1) + bound[0]


# ---- 3. the footprint, the clamp, inside_out -----------------------------------------------------------------------------------------------------
def test_footprint_rule_and_the_clamp_at_the_upper_face():
    """u = 0 and u = dims - 1 are inside, one float outside each is outside, a NaN is outside: sdis NaN, n = 0 whatever inside_out says.  On the
    upper face cid is clamped to dims - 2 and the weights are (0, 1): the query returns the face's own sample."""
    c, a, b = affine_volume(origin=(0.25, 0.5, 0.0), spacing=0.25)                        # (every sample position, and one float beyond it, is exact)
    o, sp, dims = c["origin"], c["spacing"], c["table"].shape[:3]
    ax = [(o[d] + (np.arange(dims[d]).astype(np.float32) * sp).astype(np.float32)).astype(np.float32) for d in range(3)]
    mid = [ax[d][2] for d in range(3)]
    inf = np.float32(np.inf)
    for io in (False, True):
        cc = {**c, "inside_out": io}
        for d in range(3):
            for v, inside in ((ax[d][0], True), (np.nextafter(ax[d][0], -inf), False), (ax[d][-1], True), (np.nextafter(ax[d][-1], inf), False), (np.float32(np.nan), False)):
                p = np.array(mid, np.float32)
                p[d] = v
                want = inside
                sd, n = vm.query(cc, p[None])
                assert vm.footprint(cc, p[None])[0] == want
                assert (not np.isnan(sd[0])) == want and (want or (n[0] == 0).all()), (d, float(v), io)
    # the upper face exactly: choose a table whose upper face is exactly representable
    T = np.random.default_rng(1).standard_normal((3, 4, 5, 4)).astype(np.float32)
    f = vm.volume(T, origin=(0.0, 0.0, 0.0), spacing=0.25)
    x = np.array([[0.5, 0.75, 1.0], [0.25, 0.75, 0.5], [0.5, 0.25, 1.0]], np.float32)                 # x on the +x face, y on the +y face, z on the +z face ...
    idx = (x / np.float32(0.25)).astype(int)
    sd, n = vm.query(f, x)
    assert np.array_equal(sd, T[idx[:, 0], idx[:, 1], idx[:, 2], 0])
    g = T[idx[:, 0], idx[:, 1], idx[:, 2], 1:]
    nn = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).astype(np.float32) + g[:, 2] * g[:, 2]).astype(np.float32))
    assert np.array_equal(n, (g / nn[:, None]).astype(np.float32))
    sd_io, n_io = vm.query({**f, "inside_out": True}, x)
    assert np.array_equal(sd_io, -sd) and np.array_equal(n_io, -n)


# ---- 4. the x86 builds against the model ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_vol(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostvolume.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + HOSTCHECK, "-I" + entry.CSRC, "-o", out,
                           os.path.join(HOSTCHECK, "check_volume.cpp")])
    lib = C.CDLL(out)
    lib.host_volume_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.host_volume_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.host_volume_sample_points.argtypes = [C.c_float, C.c_float, C.c_int, C.c_void_p]
    lib.host_volume_autosize.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("volume") / "host_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-o", exe, os.path.join(HOST, "host_selftest.cpp")])
    return exe


def selftest_query(exe, c, x, tmp_path):
    t, p = tmp_path / "table.f32", tmp_path / "points.f32"
    c["table"].astype("<f4").tofile(str(t))
    np.ascontiguousarray(x, dtype="<f4").tofile(str(p))
    args = [exe, "--volume-query", str(t)] + [str(n) for n in c["table"].shape[:3]] + ["%.9g" % float(v) for v in c["origin"]] + ["%.9g" % float(c["spacing"]), str(int(c["inside_out"])), str(p)]
    out = subprocess.check_output(args, text=True, timeout=120)
    w = np.array([[int(h, 16) for h in line.split()] for line in out.strip().splitlines()], dtype=np.uint32).view(np.float32)
    return w[:, 0], w[:, 1:]


@pytest.mark.parametrize("inside_out", [False, True], ids=["outward", "inside_out"])
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("name", TABLES)
def test_host_builds_equal_the_float32_model_bit_for_bit(host_vol, selftest, tmp_path, name, moved, inside_out):
    """Material point, sdis and n of tools/hostcheck/check_volume.cpp, and sdis and n of host_selftest --volume-query on the model's material
    points, against the model on 4096 seeded domain points and the special points (on samples, on cell edges, u = 0 and u = dims - 1 and
    one float outside each, NaN), identity pose and the moved pose at T = 0.37, both signs; then the response (all three boundary types) on
    the scene's nodes.  On the model: between 2 % and 98 % of the points are touched and the outside points answer NaN."""
    c = vm.make(name, moved, inside_out=inside_out)
    t = sm.T_MOVED if moved else 0.0
    X = vm.query_points(c, t, moved)
    obj, vol, T = ffi_triple(c)
    out = np.empty((len(X), 7), np.float32)
    assert host_vol.host_volume_query(C.byref(obj), C.byref(vol), ptr(T), float(t), ptr(X), len(X), ptr(out)) == 0
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    sdm, nm = vm.query(c, xm)
    assert np.array_equal(gm.canon(out[:, 4:7]), gm.canon(xm))
    assert np.array_equal(gm.canon(out[:, 0]), gm.canon(sdm)), np.argwhere(gm.canon(out[:, 0]) != gm.canon(sdm))[:4].tolist()
    assert np.array_equal(gm.canon(out[:, 1:4]), gm.canon(nm)), np.argwhere(gm.canon(out[:, 1:4]) != gm.canon(nm))[:4].tolist()
    sd2, n2 = selftest_query(selftest, c, xm, tmp_path)
    assert np.array_equal(gm.canon(sd2), gm.canon(sdm)) and np.array_equal(gm.canon(n2), gm.canon(nm))
    touched = sdm <= 0
    outside = ~vm.footprint(c, xm)
    assert 0.02 < touched.mean() < 0.98, touched.mean()
    assert outside.sum() > 100 and np.isnan(sdm[outside]).all() and (nm[outside] == 0).all() and np.isnan(sdm[-3:]).all() and not np.isnan(sdm[~outside]).any()
    if not moved:
        k = len(vm.special_points(c))
        assert np.isnan(sdm[-k:]).sum() >= 6 + 6 + 2 + 3
    nodes = gm.node_coords(gm.scene_keys()).transpose(0, 2, 1).reshape(-1, 3)
    vel = (np.random.default_rng(3).standard_normal((len(nodes), 3)) * 2).astype(np.float32)
    Xn = (nodes.astype(np.float32) * np.float32(DX)).astype(np.float32)
    nodes32 = np.ascontiguousarray(nodes, dtype=np.int32)
    for typ in (0, 1, 2):
        cc = {**c, "type": typ}
        want, hit = vm.resolve(cc, t, Xn, vel)
        obj, vol, T = ffi_triple(cc)
        got = vel.copy()
        assert host_vol.host_volume_resolve(C.byref(obj), C.byref(vol), ptr(T), float(t), DX, ptr(nodes32), len(nodes32), ptr(got)) == 0
        assert hit.any() and not hit.all()
        assert np.array_equal(gm.canon(got), gm.canon(want)), (typ, np.argwhere(gm.canon(got) != gm.canon(want))[:4].tolist())
        assert np.array_equal(got[~hit].view(np.uint32), vel[~hit].view(np.uint32))


# ---- 5. the samples' positions and the auto-sized box ----------------------------------------------------------------------------------------------
def test_sample_points_and_the_auto_sizing_rule(host_vol):
    """origin + (float) i * spacing of the x86 build equals the model's; the auto-sized box of a box mesh and of an icosphere equals the rule
    origin = min - pad spacing, dims = ceil((max - min) / spacing) + 2 pad + 1 in float64, contains the mesh with its margin, and leaves
    the limits where the rule says so."""
    for o, sp, n in ((0.26, 0.037, 18), (-0.4, 0.041, 45), (0.0, DX, 64)):
        out = np.empty(n, np.float32)
        host_vol.host_volume_sample_points(o, sp, n, ptr(out))
        want = vm.sample_points((o, o, o), sp, (n, 2, 2)).reshape(n, 2, 2, 3)[:, 0, 0, 0]
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    meshes = {"box": scenes.box_mesh((0.21, 0.3, 0.4), (0.55, 0.41, 0.83)), "icosphere": scenes.icosphere((0.47, 0.52, 0.55), 0.21, 2)}
    for name, (v, f) in meshes.items():
        v = np.ascontiguousarray(v, dtype=np.float32)
        for sp, pad in ((0.037, 2), (DX, 1), (0.011, 5)):
            origin, dims, ok = vm.autosize(v, sp, pad)
            o, d = np.empty(3, np.float32), np.empty(3, np.int32)
            assert host_vol.host_volume_autosize(ptr(v), len(v), sp, pad, ptr(o), ptr(d)) == (0 if ok else 1) and ok
            assert np.array_equal(o.view(np.uint32), origin.view(np.uint32)) and d.tolist() == dims, (name, sp, pad)
            hi = origin.astype(np.float64) + (np.array(dims) - 1) * float(np.float32(sp))
            m = (pad - 1e-3) * sp
            assert (origin <= v.min(axis=0) - m).all() and (hi >= v.max(axis=0) + m).all()
        origin, dims, ok = vm.autosize(v, 1e-4, 2)
        assert not ok and host_vol.host_volume_autosize(ptr(v), len(v), 1e-4, 2, ptr(o), ptr(d)) == 1


# ---- 6. refusals that need no device --------------------------------------------------------------------------------------------------------------
def test_function_level_entry_refuses_bad_arguments_before_touching_a_device():
    """mpm_test_collision_volume validates on the host first: MPM_ERR_INVALID for NULL arguments, a dim outside 2..1024, a product above 2^27,
    zero dims, a bad spacing, a NaN origin, pad < 0, a boundary type outside 0..2 and a sample that is not finite - with device -1, which no
    call that got past the checks could use."""
    api = _ffi.load_hip()
    c = vm.make("2x2x2")
    X, out = np.zeros((1, 3), np.float32), np.zeros((1, 4), np.float32)

    def call(obj, vol, T, n=1):
        return api.test_collision_volume(C.byref(obj) if obj else None, C.byref(vol) if vol else None, ptr(T) if T is not None else None, 0.0, ptr(X), n, ptr(out), -1)

    obj, vol, T = ffi_triple(c)
    assert call(None, vol, T) == call(obj, None, T) == call(obj, vol, None) == call(obj, vol, T, 0) == _ffi.MPM_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    for field, value in (("dims", (1, 2, 2)), ("dims", (2, 1025, 2)), ("dims", (1024, 1024, 256)), ("dims", (0, 0, 0)), ("spacing", 0.0), ("spacing", -1.0), ("spacing", inf),
                         ("spacing", nan), ("origin", (0.0, nan, 0.0)), ("pad", -1)):
        obj, vol, T = ffi_triple(c)
        if field in ("dims", "origin"):
            for d in range(3):
                getattr(vol, field)[d] = value[d]
        else:
            setattr(vol, field, value)
        assert call(obj, vol, T) == _ffi.MPM_ERR_INVALID, (field, value)
    for typ in (-1, 3):
        obj, vol, T = ffi_triple({**c, "type": typ})
        assert call(obj, vol, T) == _ffi.MPM_ERR_INVALID
    for bad in (nan, inf):
        obj, vol, T = ffi_triple(c)
        T = T.copy()
        T[1, 0, 1, 2] = bad
        assert call(obj, vol, T) == _ffi.MPM_ERR_INVALID

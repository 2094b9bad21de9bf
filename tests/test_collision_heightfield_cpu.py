"""The heightfield collider, CPU side: the ABI surface, the x86 build of claymore_amd/csrc/mpm_collision_heightfield.hpp
(tools/hostcheck/check_heightfield.cpp) against the float32 model of tests/heightfield_model.py bit for bit, that model against the float64
closed form within a counted bound, a flat table against the half-space shape, and the index arithmetic under a sanitizer in a stand-alone
program.  (The ISA of the grid kernels: tests/test_grid_update_isa.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import collision_shape_model as sm
import grid_update_model as gm
import heightfield_model as hm
from claymore_amd import _ffi
from claymore_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

DX = sm.DX
HOSTCHECK = os.path.join(ROOT, "tools", "hostcheck")
TABLES = ("2x2", "5x3", "65x65", "33x17")


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def ffi_triple(c):
    """A model heightfield as the two ABI structs and the heights."""
    obj, hf = _ffi.CollisionObject(), _ffi.Heightfield()
    obj.type, obj.friction, obj.scale, obj.dsdt, obj.time = c["type"], float(c["friction"]), float(c["scale"]), float(c["dsdt"]), float(c["time"])
    for d in range(3):
        obj.trans[d], obj.trans_vel[d], obj.omega[d] = float(c["trans"][d]), float(c["trans_vel"][d]), float(c["omega"][d])
    for e in range(9):
        obj.rot_mat[e] = float(c["rot"][e])
    hf.nx, hf.nz = c["heights"].shape
    hf.origin[0], hf.origin[1], hf.spacing, hf.inside_out = float(c["origin"][0]), float(c["origin"][1]), float(c["spacing"]), int(c["inside_out"])
    return obj, hf, np.ascontiguousarray(c["heights"], dtype=np.float32)


def domain_points_of(c, t, x):
    """Domain points X whose material points are (about) x: X = R (x - trans) / (scale inv) + shift, in float64."""
    p = sm.pose(c, t)
    R = p["rot"].astype(np.float64).reshape(3, 3)
    x0 = (np.asarray(x, np.float64) - c["trans"].astype(np.float64)) / float(c["scale"])
    return ((x0 @ R) / float(p["inv"]) + p["shift"].astype(np.float64)).astype(np.float32)


def seeded_points(c, t, seed=7, n=4096):
    """n seeded domain points: half of them anywhere in [-0.25, 1.25)^3 (every 16th snapped to a node), half of them with material points over
    the table's footprint widened by a tenth, heights in [0, 1)."""
    rng = np.random.default_rng(seed)
    free = sm.seeded_points(seed, n // 2)
    (nx, nz), o, sp = c["heights"].shape, c["origin"].astype(np.float64), float(c["spacing"])
    ext = np.array([(nx - 1) * sp, (nz - 1) * sp])
    r = rng.random((n - n // 2, 3))
    x = np.stack([o[0] + ext[0] * (1.2 * r[:, 0] - 0.1), r[:, 1], o[1] + ext[1] * (1.2 * r[:, 2] - 0.1)], axis=1)
    return np.concatenate([free, domain_points_of(c, t, x)]).astype(np.float32)


def query_points(c, t, moved):
    sp = hm.special_points(c)
    return np.concatenate([seeded_points(c, t), sp if not moved else domain_points_of(c, t, sp)])


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------------
def test_heightfield_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert re.search(r"int mpm_set_collision_heightfield\(mpm_ctx\* ctx, int slot, const mpm_collision_object\* obj, const mpm_heightfield\* hf, const float\* heights\);", hdr)
    assert re.search(r"int mpm_test_collision_heightfield\(const mpm_collision_object\* obj, const mpm_heightfield\* hf, const float\* heights, float time, const float\* xyz, size_t n,", hdr)
    assert "MPM_HEIGHTFIELD_MAX_SAMPLES = 4096" in hdr and "tangent plane" in hdr
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    for sym in ("mpm_set_collision_heightfield", "mpm_test_collision_heightfield"):
        assert re.search(rf"\bT {sym}$", out, re.M), f"{sym} is not exported"
    for name in ("set_collision_heightfield", "test_collision_heightfield"):
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES
    api = _ffi.load_hip()
    assert api.set_collision_heightfield.argtypes[1] is C.c_int and len(api.set_collision_heightfield.argtypes) == 5 and len(api.test_collision_heightfield.argtypes) == 8
    assert C.sizeof(_ffi.Heightfield) == 4 * (2 + 2 + 1 + 1 + 6)
    assert callable(Engine.set_collision_heightfield)
    assert " abi7 " in api.build_info().decode()


# ---- the x86 build ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_hf(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostheightfield.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + HOSTCHECK, "-I" + entry.CSRC, "-o", out,
                           os.path.join(HOSTCHECK, "check_heightfield.cpp")])
    lib = C.CDLL(out)
    lib.host_heightfield_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
    lib.host_heightfield_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.host_heightfield_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def host_shapes(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostshapes.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + HOSTCHECK, "-I" + entry.CSRC, "-o", out,
                           os.path.join(HOSTCHECK, "check_shapes.cpp")])
    lib = C.CDLL(out)
    lib.host_shape_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def host_query(lib, c, t, X):
    obj, hf, H = ffi_triple(c)
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty((len(X), 7), np.float32)
    assert lib.host_heightfield_query(C.byref(obj), C.byref(hf), ptr(H), float(t), ptr(X), len(X), ptr(out)) == 0
    return out[:, 0], out[:, 1:4], out[:, 4:7]


def host_resolve(lib, c, t, nodes, vel):
    obj, hf, H = ffi_triple(c)
    nodes = np.ascontiguousarray(nodes, dtype=np.int32)
    got = np.ascontiguousarray(vel, dtype=np.float32).copy()
    assert lib.host_heightfield_resolve(C.byref(obj), C.byref(hf), ptr(H), float(t), DX, ptr(nodes), len(nodes), ptr(got)) == 0
    return got


def scene_nodes():
    nodes = gm.node_coords(gm.scene_keys()).transpose(0, 2, 1).reshape(-1, 3)
    vel = (np.random.default_rng(3).standard_normal((len(nodes), 3)) * 2).astype(np.float32)
    return nodes, vel, (nodes.astype(np.float32) * np.float32(DX)).astype(np.float32)


# ---- 2. the x86 build against the float32 model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inside_out", [False, True], ids=["floor", "ceiling"])
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("name", TABLES)
def test_host_build_equals_the_float32_model_bit_for_bit(host_hf, name, moved, inside_out):
    """The table, then material point, sdis and n of the x86 build against the model on 4096 seeded domain points and the special points of
    heightfield_model.special_points (on samples, on cell edges, u = 0 and u = nx - 1 exactly and one nextafter outside each, exactly on the
    surface, NaN input), identity pose and the moved pose at T = 0.37, floor and ceiling; then the response (all three boundary types) on the
    scene's nodes.  On the model: between 2 % and 98 % of the points are touched, and the outside points answer NaN."""
    c = hm.make(name, moved, inside_out=inside_out)
    t = sm.T_MOVED if moved else 0.0
    H = c["heights"]
    tab = np.empty(H.shape + (4,), np.float32)
    assert host_hf.host_heightfield_build(ptr(H), H.shape[0], H.shape[1], float(c["spacing"]), ptr(tab)) == 0
    assert np.array_equal(tab.view(np.uint32), c["table"].view(np.uint32))
    X = query_points(c, t, moved)
    sd, n, x = host_query(host_hf, c, t, X)
    _, xm = sm.material_point(c, sm.pose(c, t), X)
    sdm, nm = hm.query(c, xm)
    assert np.array_equal(gm.canon(x), gm.canon(xm))
    assert np.array_equal(gm.canon(sd), gm.canon(sdm)), np.argwhere(gm.canon(sd) != gm.canon(sdm))[:4].tolist()
    assert np.array_equal(gm.canon(n), gm.canon(nm)), np.argwhere(gm.canon(n) != gm.canon(nm))[:4].tolist()
    touched = sdm <= 0
    assert 0.02 < touched.mean() < 0.98, touched.mean()
    (nx, nz), o, sp = H.shape, c["origin"], c["spacing"]
    with np.errstate(all="ignore"):
        u, w = ((xm[:, 0] - o[0]) / sp).astype(np.float32), ((xm[:, 2] - o[1]) / sp).astype(np.float32)
    outside = ~((u >= 0) & (u <= nx - 1) & (w >= 0) & (w <= nz - 1))
    assert outside.sum() > 100 and np.isnan(sdm[outside]).all() and (nm[outside] == 0).all() and np.isnan(sdm[-3:]).all()
    assert not np.isnan(sdm[~outside][:-3]).any()
    if not moved:                                                         # the special points are hit exactly only where x == X
        k = len(hm.special_points(c))
        assert (sdm[-k:] == 0).sum() >= 4, "no special point lies on the surface"
        assert (np.isnan(sdm[-k:])).sum() >= 16 + 4 + 3
    nodes, vel, Xn = scene_nodes()
    for typ in (0, 1, 2):
        cc = {**c, "type": typ}
        want, hit = hm.resolve(cc, t, Xn, vel)
        got = host_resolve(host_hf, cc, t, nodes, vel)
        assert hit.any() and not hit.all()
        assert np.array_equal(gm.canon(got), gm.canon(want)), (typ, np.argwhere(gm.canon(got) != gm.canon(want))[:4].tolist())
        assert np.array_equal(got[~hit].view(np.uint32), vel[~hit].view(np.uint32))


# ---- 3. the model against the float64 closed form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
def test_model_against_the_float64_closed_form(name):
    """h, sdis and n of the float32 model at seeded material points (identity pose: x = X) against exact bilinear interpolation of the same
    float32 table in float64.  The bound is counted from the statements, first order in u = eps / 2 (eps = 2^-23), per channel c of the table
    with M_c = max |t.c|, V_c = the largest difference of t.c between two neighbouring samples, U = max(nx, nz) - 1 >= u, w:
      u, w: a subtraction and a division, relative 2 u each -> |d fu| <= eps U (fu = u - (float) i is exact); a shift of fu or fw by d moves an
        interpolated channel by at most V_c d: 2 V_c eps U for the pair;
      cu, cw: one rounding each of a value <= 1, breaking the partition of unity by u: 2 u M_c; the four weight products: u M_c; the four
        products with t: u M_c; the three additions of partial sums <= M_c: 3 u M_c          -> 7 u M_c = 3.5 eps M_c, taken as 4 eps M_c
        (second-order terms)
      => d_c = eps (4 M_c + 2 U V_c);  d_g = max(d_gx, d_gz)
      len: gx gx, + 1, gz gz, +, each relative u under the root (halved), the root u: 3 u = 1.5 eps relative, plus (|gx| d_gx + |gz| d_gz) / len
        <= 2 d_g                                                                             -> rho = 1.5 eps + 2 d_g   (len >= 1)
      n_i = g_i / len: d_g + rho + u                                                         -> 3 d_g + 2 eps
      sdis = (x1 - h) / len: d_h + (|x1| + M_h) (u + u + rho)                                -> d_h + (|x1| + M_h) (2.5 eps + 2 d_g)
    so sdis is bounded by a multiple of eps times max|h| + |x1| (the multiple: 4 + 2 U V_h / M_h + 2.5 + 2 d_g / eps, from the table alone)
    and n by the multiple 3 d_g / eps + 2 of eps.  Points whose u or w lies within 2 eps U of the footprint's rim may be inside in one
    precision and outside in the other; they are compared where both are inside."""
    c = hm.make(name)
    X = seeded_points(c, 0.0, seed=11, n=20000)
    sd, n, h = hm.query(c, X, want_h=True)
    h64, sd64, n64, in64 = hm.closed_form(c, X)
    both = ~np.isnan(sd) & in64
    assert both.sum() > 5000 and (np.isnan(sd) != ~in64).sum() <= 4
    eps = 2.0 ** -23
    T = c["table"].astype(np.float64)
    U = max(T.shape[:2]) - 1
    M = np.abs(T).max(axis=(0, 1))
    V = np.maximum(np.abs(np.diff(T, axis=0)).max(axis=(0, 1)), np.abs(np.diff(T, axis=1)).max(axis=(0, 1)))
    d = eps * (4 * M + 2 * U * V)
    d_h, d_g = d[0], max(d[1], d[2])
    x1 = np.abs(X[both, 1].astype(np.float64))
    eh = np.abs(h[both].astype(np.float64) - h64[both])
    es = np.abs(sd[both].astype(np.float64) - sd64[both])
    en = np.abs(n[both].astype(np.float64) - n64[both]).max(axis=1)
    b_s = d_h + (x1 + M[0]) * (2.5 * eps + 2 * d_g)
    b_n = 3 * d_g + 2 * eps
    print(f"{name}: h {eh.max() / eps:.2f} eps (bound {d_h / eps:.1f}), sdis max ratio to its bound {np.max(es / b_s):.4f}, n {en.max() / eps:.2f} eps (bound {b_n / eps:.1f})")
    assert eh.max() <= d_h and (es <= b_s).all() and en.max() <= b_n


# ---- 4. a flat table is the half-space -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["identity", "moved"])
@pytest.mark.parametrize("typ", [0, 1, 2], ids=["sticky", "slip", "separate"])
def test_flat_table_is_the_halfspace(host_hf, host_shapes, typ, moved):
    """A table of constant height c = 32 dx (9 x 9 samples one unit apart about the domain: every material point of the scene's nodes lies in
    its footprint, at both poses) and the shape halfspace(a = (., c, .), b = +y) give bit-identical velocities through resolve on the scene's
    nodes, in the model and in the host build."""
    from test_collision_shapes_cpu import ffi_pair
    cst = np.float32(32 * DX)
    mv = sm.MOVED if moved else {}
    t = sm.T_MOVED if moved else 0.0
    hf = hm.heightfield(np.full((9, 9), cst, np.float32), origin=(-4.0, -4.0), spacing=1.0, type=typ, friction=0.3, **mv)
    hs = sm.collider("halfspace", a=(0.25, cst, 0.75), b=(0.0, 1.0, 0.0), type=typ, friction=0.3, **mv)
    nodes, vel, Xn = scene_nodes()
    want_hf, hit_hf = hm.resolve(hf, t, Xn, vel)
    want_hs, hit_hs = sm.resolve(hs, t, Xn, vel)
    assert np.array_equal(hit_hf, hit_hs) and 0.05 < hit_hf.mean() < 0.95
    assert np.array_equal(want_hf.view(np.uint32), want_hs.view(np.uint32)), np.argwhere(want_hf.view(np.uint32) != want_hs.view(np.uint32))[:4].tolist()
    got_hf = host_resolve(host_hf, hf, t, nodes, vel)
    obj, sh = ffi_pair(hs)
    got_hs = vel.copy()
    assert host_shapes.host_shape_resolve(C.byref(obj), C.byref(sh), float(t), DX, ptr(np.ascontiguousarray(nodes, dtype=np.int32)), len(nodes), ptr(got_hs)) == 0
    assert np.array_equal(got_hf.view(np.uint32), got_hs.view(np.uint32)) and np.array_equal(got_hf.view(np.uint32), want_hf.view(np.uint32))


# ---- 5. the index arithmetic under a sanitizer ------------------------------------------------------------------------------------------------
def test_selftest_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tools/hostcheck/heightfield_selftest.cpp - a program of its own that includes only the header - built with
    -fsanitize=address,undefined and run as a child process: 2 x 2, 2 x 9 and 9 x 2 tables in heap blocks of exactly nx nz entries, queried at the
    footprint's corners, edges and one float outside.  Nothing sanitised is loaded into this process."""
    exe = str(tmp_path / "heightfield_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + HOSTCHECK,
                           "-I" + entry.CSRC, "-o", exe, os.path.join(HOSTCHECK, "heightfield_selftest.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "heightfield_selftest ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])

"""Rigid bodies, CPU side: the ABI surface, the x86 build of claymore_amd/csrc/mpm_rigid_body.hpp (tools/hostcheck/check_body.cpp) against
tests/rigid_body_model.py ON BITS, the step against closed forms (free fall, a free asymmetric body, a symmetric top, locks), the mass properties
of the host-only calls against the textbook formulas, a quadrature and the polyhedral integrals of known solids, and every refusal that needs no
device.  The kernels are judged against the same model in tests/test_rigid_body_gpu.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import collision_shape_model as sm
import rigid_body_model as bm
from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
NAMES = ("set_collider_body", "get_collider_body", "set_collider_body_state", "shape_mass_properties", "mesh_mass_properties")


def test_abi_surface():
    for name in NAMES:
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES
    api = _ffi.load_hip()
    assert C.sizeof(_ffi.RigidBody) == 4 * (1 + 6 + 3 + 1 + 1 + 3 + 3 + 8) and C.sizeof(_ffi.RigidBodyState) == 8 * 26
    assert " abi7 " in api.build_info().decode()
    for m in ("set_collider_body", "collider_body", "set_collider_body_state", "shape_mass_properties", "mesh_mass_properties"):
        assert callable(getattr(Engine, m))
    header = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    for name in NAMES:
        assert f"int mpm_{name}(" in header


# ---- the x86 build --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostbody.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tools", "hostcheck"),
                           "-I" + entry.CSRC, "-o", out, os.path.join(ROOT, "tools", "hostcheck", "check_body.cpp")])
    lib = C.CDLL(out)
    lib.host_body_constants.restype = lib.host_body_object.restype = lib.host_body_restart.restype = C.c_char_p
    lib.host_body_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_float, C.c_float, C.c_int]
    lib.host_body_start.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.host_body_pose.argtypes = [C.c_void_p, C.c_void_p]
    lib.host_body_restart.argtypes = [C.c_void_p] * 6
    return lib


def ffi_body(mass=2.0, inertia=(0.3, 0.2, 0.25, 0.01, -0.02, 0.015), com=(0.5, 0.5, 0.5), gravity=True, lock=0, force=(0, 0, 0), torque=(0, 0, 0)):
    b = _ffi.RigidBody()
    b.mass = mass
    for i in range(6):
        b.inertia[i] = inertia[i]
    for d in range(3):
        b.com[d], b.force[d], b.torque[d] = com[d], force[d], torque[d]
    b.gravity, b.lock = int(bool(gravity)), bm.constants(1, (1, 1, 1, 0, 0, 0), (0, 0, 0), lock=lock)["lock"]
    return b


def model_const(b):
    return bm.constants(b.mass, b.inertia[:], b.com[:], b.gravity, b.lock, b.force[:], b.torque[:])


def ffi_state(s):
    st = _ffi.RigidBodyState()
    C.memmove(C.byref(st), bm.state_words(s).tobytes(), C.sizeof(st))
    return st


def words(st):
    return np.frombuffer(bytes(st), dtype=np.uint64).copy()


def random_state(rng, c):
    s = bm.new_state()
    q = rng.normal(size=4)
    s["q"] = (q / np.linalg.norm(q)).tolist()
    s["x"], s["v"], s["l"] = rng.random(3).tolist(), rng.normal(size=3).tolist(), (0.3 * rng.normal(size=3)).tolist()
    bm.omega_of(s, c)
    return s


def test_x86_step_equals_the_model_on_bits(host):
    rng = np.random.default_rng(11)
    for i in range(1000):
        lock = int(rng.integers(0, 64)) if i % 3 == 0 else 0
        on = lambda k: (rng.normal(size=3) * 0.5).tolist() if (i >> k) & 1 else (0.0, 0.0, 0.0)  # noqa: E731
        a = rng.normal(size=(3, 3))
        I = a @ a.T * 0.05 + np.eye(3) * 0.1
        b = ffi_body(mass=float(rng.uniform(0.5, 20)), inertia=(I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]), com=rng.random(3).tolist(), gravity=bool(i & 1),
                     lock=lock, force=on(1), torque=on(2))
        c = model_const(b)
        assert c is not None
        s = random_state(rng, c)
        J, L = (rng.normal(size=3) * 10.0 ** rng.uniform(-6, 0)), (rng.normal(size=3) * 10.0 ** rng.uniform(-7, -1))
        if i % 5 == 0:
            J, L = np.zeros(3), np.zeros(3)
        n, m, dt, g = float(rng.integers(0, 5000)), float(rng.uniform(0, 3)), float(np.float32(10.0 ** rng.uniform(-5, -2))), float(np.float32(-9.8))
        st = ffi_state(s)
        Jc, Lc = (C.c_double * 3)(*J), (C.c_double * 3)(*L)
        steps = 1 + i % 3
        assert host.host_body_step(C.byref(st), C.byref(b), Jc, Lc, n, m, dt, g, steps) == 0
        for _ in range(steps):
            assert bm.body_step(s, c, J, L, n, m, dt, g)
        assert np.array_equal(words(st), bm.state_words(s)), (i, np.flatnonzero(words(st) != bm.state_words(s)))
        pose = np.zeros(18, np.float32)
        host.host_body_pose(C.byref(st), pose.ctypes.data)
        p = bm.pose_of(s)
        assert np.array_equal(pose.view(np.uint32), np.concatenate([p["rot"], p["shift"], p["vel"], p["omega"]]).view(np.uint32))
    # a non-finite impulse is reported, and the state says so
    st = ffi_state(s)
    assert host.host_body_step(C.byref(st), C.byref(b), (C.c_double * 3)(float("nan"), 0, 0), Lc, 1.0, 1.0, dt, g, 1) == 1
    assert not bm.body_step(s, c, [float("nan"), 0, 0], L, 1.0, 1.0, dt, g)


def test_x86_start_equals_the_model_on_bits(host):
    rng = np.random.default_rng(12)
    for i, moved in enumerate([False, True, True, False]):
        col = sm.make("box", moved=False, **(dict(trans=(0.4, 0.5, 0.45), trans_vel=(0.1, -0.2, 0.3), omega=(1.0, -0.5, 1.5), rot_mat=sm.TILT) if moved else {}))
        b = ffi_body(com=(0.28, 0.5, 0.5) if i < 2 else rng.random(3).tolist(), lock=("rx" if i == 3 else 0))
        c = model_const(b)
        t = 0.37 if i == 2 else 0.0
        obj = _ffi.CollisionObject()
        obj.scale = 1.0
        for d in range(3):
            obj.trans[d], obj.trans_vel[d], obj.omega[d] = col["trans"][d], col["trans_vel"][d], col["omega"][d]
        for k in range(9):
            obj.rot_mat[k] = col["rot"][k]
        st, pose = _ffi.RigidBodyState(), np.zeros(18, np.float32)
        assert host.host_body_start(C.byref(obj), t, C.byref(b), C.byref(st), pose.ctypes.data) == 0
        s = bm.start(col, c, t)
        assert np.array_equal(words(st), bm.state_words(s)), i
        if not moved:
            assert s["q"] == [1.0, 0.0, 0.0, 0.0] and s["omega"] == [0.0] * 3
        # every node's material point is what it was: R^T (X - x0) + com against rot (X - shift) + trans, to float32 rounding
        X = rng.random((64, 3))
        p = sm.pose(col, t)
        before = (X - p["shift"].astype(np.float64)) @ p["rot"].astype(np.float64).reshape(3, 3).T + col["trans"].astype(np.float64)
        R = np.array(bm.rotation(s["q"])).reshape(3, 3)
        after = (X - np.array(s["x"])) @ R + np.array(c["com"])
        assert np.abs(before - after).max() < 4 * 2.0 ** -24


# ---- closed forms on the x86 build -----------------------------------------------------------------------------------------------------------
def run(host, b, s, steps, dt, g=-9.8, J=(0, 0, 0), L=(0, 0, 0)):
    st = ffi_state(s)
    assert host.host_body_step(C.byref(st), C.byref(b), (C.c_double * 3)(*J), (C.c_double * 3)(*L), 0.0, 0.0, dt, g, steps) == 0
    out = _ffi.RigidBodyState.from_buffer_copy(bytes(st))
    return out


def test_free_fall_closed_form(host):
    n, dt, g = 1000, float(np.float32(1e-4)), float(np.float32(-9.8))
    b = ffi_body()
    s = bm.new_state()
    s["x"] = [0.5, 0.75, 0.5]
    st = run(host, b, s, n, dt, g)
    v, x = n * g * dt, 0.75 + g * dt * dt * n * (n + 1) / 2
    assert abs(st.velocity[1] - v) <= 4 * n * U * abs(v)
    assert abs(st.position[1] - x) <= 4 * n * U * abs(x)
    assert st.position[0] == 0.5 and st.position[2] == 0.5 and st.velocity[0] == 0.0 and st.updates == n and list(st.orientation) == [1.0, 0.0, 0.0, 0.0]


def test_free_asymmetric_body_keeps_l_on_bits_and_q_unit(host):
    b = ffi_body(inertia=(0.3, 0.1, 0.2, 0.02, -0.03, 0.01), gravity=False)
    c = model_const(b)
    s = random_state(np.random.default_rng(3), c)
    l0 = list(s["l"])
    st = run(host, b, s, 10000, float(np.float32(1e-3)))
    assert list(st.angular_momentum) == l0
    q = np.array(st.orientation[:])
    assert abs(math.sqrt(math.fsum((q * q).tolist())) - 1.0) <= 2.0 ** -52
    assert np.abs(np.array(st.omega[:]) - np.array(s["omega"])).max() > 1e-3                 # (it did tumble)


def test_symmetric_top_keeps_omega(host):
    b = ffi_body(inertia=(0.2, 0.2, 0.2, 0, 0, 0), gravity=False)
    c = model_const(b)
    s = bm.new_state()
    s["l"] = [0.02, -0.05, 0.03]
    bm.omega_of(s, c)
    w0 = np.array(s["omega"])
    st = run(host, b, s, 2000, float(np.float32(1e-3)))
    assert np.abs(np.array(st.omega[:]) - w0).max() <= 16 * U * np.abs(w0).max()
    assert np.abs(np.array(st.orientation[:]) - np.array([1.0, 0, 0, 0])).max() > 0.1        # (it did turn)


def test_locked_axes_stay_exactly_zero(host):
    b = ffi_body(lock="x z rx ry", force=(1.0, 2.0, 3.0), torque=(0.1, 0.2, 0.3))
    s = bm.new_state()
    st = run(host, b, s, 500, float(np.float32(1e-3)), J=(0.01, 0.02, -0.01), L=(0.001, -0.002, 0.003))
    assert st.velocity[0] == 0.0 and st.velocity[2] == 0.0 and st.position[0] == 0.0 and st.position[2] == 0.0 and st.velocity[1] != 0.0
    assert st.omega[0] == 0.0 and st.omega[1] == 0.0 and st.omega[2] != 0.0
    assert st.orientation[1] == 0.0 and st.orientation[2] == 0.0 and st.orientation[3] != 0.0  # a turn about z alone


# ---- mass properties ---------------------------------------------------------------------------------------------------------------------------
def ulps32(got, want):
    want32 = np.float32(want)
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(want32))) if want32 != 0 else abs(float(got))


def test_sphere_and_box_against_the_textbook():
    rho, r = 2500.0, float(np.float32(0.11))
    m, i6, com = Engine.shape_mass_properties("sphere", rho, a=(0.4, 0.5, 0.6), radius=r)
    wm, wi = bm.sphere_mass(rho, r)
    assert ulps32(m, wm) <= 4 and all(ulps32(i6[k], wi[k]) <= 4 for k in range(6)) and np.array_equal(com, np.float32([0.4, 0.5, 0.6]))
    bh = [float(v) for v in np.float32([0.1, 0.05, 0.2])]
    m, i6, com = Engine.shape_mass_properties("box", rho, a=(0.3, 0.2, 0.1), b=bh)
    wm, wi = bm.box_mass(rho, bh)
    assert ulps32(m, wm) <= 4 and all(ulps32(i6[k], wi[k]) <= 4 for k in range(6)) and np.array_equal(com, np.float32([0.3, 0.2, 0.1]))


def test_capsule_against_a_quadrature():
    rho, r = 800.0, float(np.float32(0.07))
    a, b = [float(v) for v in np.float32([0.3, 0.4, 0.35])], [float(v) for v in np.float32([0.55, 0.5, 0.7])]
    m, i6, com = Engine.shape_mass_properties("capsule", rho, a=a, b=b, radius=r)
    tol = 1e-6                                                                              # relative; a few float32 roundings of the outputs are 2e-7
    fine, coarse = bm.capsule_quadrature(rho, a, b, r, 400000), bm.capsule_quadrature(rho, a, b, r, 200000)
    scale = np.abs(fine[1]).max()
    assert abs(fine[0] - coarse[0]) < 0.1 * tol * fine[0] and np.abs(fine[1] - coarse[1]).max() < 0.1 * tol * scale
    I = np.array([[i6[0], i6[3], i6[4]], [i6[3], i6[1], i6[5]], [i6[4], i6[5], i6[2]]], dtype=np.float64)
    assert abs(m - fine[0]) <= tol * fine[0] and np.abs(I - fine[1]).max() <= tol * scale and np.abs(com - fine[2]).max() <= 2.0 ** -24


def test_mesh_properties_box_and_icosphere():
    api = _ffi.load_hip()
    # a box whose mass properties ARE float32 numbers (dyadic half extents 1/8, 1/16, 1/4, a density divisible by 3): the ABI's float32 fields
    # hold the float64 results without a rounding of their own, and the bound is the integrals'
    rho = 3000.0
    lo, hi = np.float32([0.25, 0.3125, 0.25]), np.float32([0.5, 0.4375, 0.75])
    v, f = scenes.box_mesh(lo, hi)
    out = _ffi.RigidBody()
    v = np.ascontiguousarray(v, np.float32)
    f = np.ascontiguousarray(f, np.int32)
    assert api.mesh_mass_properties(v.ctypes.data, len(v), f.ctypes.data, len(f), rho, C.byref(out)) == 0
    bh = (hi.astype(np.float64) - lo.astype(np.float64)) / 2
    wm, wi = bm.box_mass(rho, bh)
    assert float(np.float32(wm)) == wm and all(float(np.float32(w)) == w for w in wi)
    assert abs(out.mass - wm) <= 1e-12 * wm
    for k in range(3):
        assert abs(out.inertia[k] - wi[k]) <= 1e-12 * wi[k], (k, out.inertia[k], wi[k])
        assert abs(out.inertia[3 + k]) <= 1e-12 * wi[0]
        assert abs(out.com[k] - (float(lo[k]) + float(hi[k])) / 2) <= 1e-12
    assert out.gravity == 1 and out.lock == 0
    errs = []
    for sub in (1, 2, 3):
        v, f = scenes.icosphere((0.5, 0.5, 0.5), 0.2, sub)
        m, i6, com = Engine.mesh_mass_properties(v, f, rho)
        wm, wi = bm.sphere_mass(rho, 0.2)
        errs.append(max(abs(m - wm) / wm, abs(i6[0] - wi[0]) / wi[0]))
        assert np.abs(com - 0.5).max() < 1e-6 and np.abs(i6[3:]).max() < 1e-6 * wi[0]
    assert errs[0] > errs[1] > errs[2] and errs[2] < 0.02, errs


# ---- refusals that need no device ------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(host):
    nan = float("nan")
    for kw, word in ((dict(mass=0.0), b"mass"), (dict(mass=-1.0), b"mass"), (dict(mass=float("inf")), b"mass"), (dict(mass=nan), b"mass"),
                     (dict(inertia=(0.3, 0.2, 0.25, 0.4, 0.0, 0.0)), b"positive definite"), (dict(inertia=(0.0, 0.2, 0.25, 0, 0, 0)), b"positive definite"),
                     (dict(inertia=(-0.1, 0.2, 0.25, 0, 0, 0)), b"positive definite"), (dict(inertia=(nan, 0.2, 0.25, 0, 0, 0)), b"NaN"),
                     (dict(com=(nan, 0, 0)), b"NaN"), (dict(force=(0, nan, 0)), b"NaN"), (dict(torque=(0, 0, nan)), b"NaN")):
        msg = host.host_body_constants(C.byref(ffi_body(**kw)))
        assert msg is not None and word in msg, (kw, msg)
    assert host.host_body_constants(C.byref(ffi_body())) is None
    b = ffi_body()
    b.lock = 64
    assert b"lock" in host.host_body_constants(C.byref(b))

    def obj(**kw):
        o = _ffi.CollisionObject()
        o.scale = kw.get("scale", 1.0)
        o.dsdt = kw.get("dsdt", 0.0)
        for k, x in enumerate(np.asarray(kw.get("rot_mat", np.eye(3)), np.float32).ravel()):
            o.rot_mat[k] = float(x)
        o.trans[0] = kw.get("trans0", 0.5)
        return o

    assert host.host_body_object(C.byref(obj())) is None and host.host_body_object(C.byref(obj(rot_mat=sm.TILT))) is None
    assert b"scale" in host.host_body_object(C.byref(obj(scale=1.125))) and b"scale" in host.host_body_object(C.byref(obj(dsdt=0.5)))
    assert b"not a rotation" in host.host_body_object(C.byref(obj(rot_mat=np.eye(3) * 1.01)))
    assert b"not a rotation" in host.host_body_object(C.byref(obj(rot_mat=np.array([[1, 1e-3, 0], [0, 1, 0], [0, 0, 1]]))))
    assert b"reflection" in host.host_body_object(C.byref(obj(rot_mat=np.diag([1.0, -1.0, 1.0]))))
    assert b"NaN" in host.host_body_object(C.byref(obj(rot_mat=np.array([[nan, 0, 0], [0, 1, 0], [0, 0, 1]]))))
    assert host.host_body_object(C.byref(obj(trans0=nan))) is not None
    # the host-only calls
    for kind, kw in (("halfspace", dict(b=(0, 1, 0))), ("sphere", dict(radius=0.0)), ("box", dict(b=(0.1, 0.0, 0.1))), ("capsule", dict(a=(0.5,) * 3, b=(0.5,) * 3, radius=0.1))):
        with pytest.raises(EngineError) as e:
            Engine.shape_mass_properties(kind, 1000.0, **kw)
        assert e.value.code == _ffi.MPM_ERR_INVALID
    for rho in (0.0, -1.0, nan):
        with pytest.raises(EngineError):
            Engine.shape_mass_properties("sphere", rho, radius=0.1)
    v, f = scenes.box_mesh((0.2, 0.2, 0.2), (0.4, 0.4, 0.4))
    with pytest.raises(EngineError):
        Engine.mesh_mass_properties(v, np.asarray(f)[:-1], 1000.0)                          # an open mesh: mpm_set_collision_mesh's validation
    with pytest.raises(EngineError):
        Engine.mesh_mass_properties(v, np.asarray(f)[:, ::-1], 1000.0)                      # inside out: no positive volume
    api = _ffi.load_hip()
    assert api.shape_mass_properties(None, 1.0, None) == _ffi.MPM_ERR_INVALID and api.mesh_mass_properties(None, 0, None, 0, 1.0, None) == _ffi.MPM_ERR_INVALID
    # a restart refuses what is not a state
    st = ffi_state(bm.new_state())
    assert host.host_body_restart(C.byref(st), C.byref(ffi_body()), None, (C.c_double * 4)(0, 0, 0, 0), None, None) is not None
    assert host.host_body_restart(C.byref(st), C.byref(ffi_body()), (C.c_double * 3)(nan, 0, 0), None, None, None) is not None
    assert host.host_body_restart(C.byref(st), C.byref(ffi_body()), None, (C.c_double * 4)(0, 0, 2.0, 0), None, (C.c_double * 3)(0, 0, 1.0)) is None
    assert list(st.orientation) == [0.0, 0.0, 1.0, 0.0] and abs(st.omega[2] - 1.0) < 1e-15

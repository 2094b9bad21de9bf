"""Moving collision object, CPU side: the clock's ABI surface, the `sphere_through_block` scene on the oracle, the pose / per-node split of
claymore_amd/csrc/mpm_collision.hpp on x86 against the oracle's detect_and_resolve_collision.  (The ISA of the fused carry-over:
tests/test_grid_update_isa.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

from claymore_amd import _ffi, scenes
from claymore_amd.engine import Engine, build_engine
from oracle_ffi import oracle_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

# The scene both the CPU and the GPU tests run: a 12 x 8 x 12-cell elastic block at rest (E = 5e3, nu = 0.4, rho = 1e3: p-wave speed
# sqrt((lambda + 2 mu) / rho) = 3.3) and a sphere of 5 cells radius that starts 2 cells clear of it and moves at 1.0 - a third of the wave
# speed: the block is pushed, not shattered - for 400 substeps of 4e-4 (0.026 cells per substep, 10 cells in all: the sphere ends well inside
# the block, in full contact).  Chosen on the CPU oracle alone: the share of test_oracle_moving_sphere_displaces_the_block is 28-30 % there,
# and the oracle against itself with the particles handed over in another order (summation order only) differs by 0.9-1.1e-6 relative in
# position after these 400 substeps with the full motion of the GPU tests (0.4-0.6e-6 after 300, 1.2-1.6e-6 after 500; with translation
# alone 2.2e-6 after 600): a tenth of the 1e-5 the GPU comparison allows.  (At speed 3.0, just below the wave speed, the same measure was
# 0.7-0.9e-6 after 200 substeps, but two runs of the HIP engine differed from each other by 4-6e-6 there: too close to the bound for a test.)
SCENE = dict(bits=6, block_cells=(12, 8, 12), radius_cells=5.0, gap_cells=2.0, speed=1.0, dt=4e-4)
STEPS = 400


def drive_oracle(sc, steps, moving=True, api=None):
    """The oracle reads col.time at every grid update: the clock's rule - the update of a substep sees T, then T = T + dt in float32 - is
    driven from here by installing the object again with time = T_k.  Returns positions, the max-velocity series, grid totals, T."""
    col = {k: v for k, v in sc["collision"].items() if k != "animate"}
    eng = build_engine({**sc, "collision": col}, api=api or oracle_api())
    eng.initial_setup()
    T, dt = np.float32(col.get("time", 0.0)), np.float32(sc["dt"])
    mv = []
    for _ in range(steps):
        if moving:
            eng.set_collision_object(**{**col, "time": float(T)})
        mv.append(eng.grid_update(sc["dt"]))
        eng.g2p2g(sc["dt"], sc["dt"])
        eng.rebuild_partition()
        T = np.float32(T + dt)
    xyz, tot = eng.retrieve_positions(0), eng.grid_totals()
    eng.close()
    return xyz, np.array(mv), tot, float(T)


def test_clock_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "claymore_amd.h")).read()
    assert re.search(r"int mpm_set_collision_clock\(mpm_ctx\* ctx, int running, float time\);", hdr)
    assert re.search(r"int mpm_get_collision_time\(mpm_ctx\* ctx, float\* time, int\* running\);", hdr)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ffi.HIP_LIB_PATH], text=True)
    for sym in ("mpm_set_collision_clock", "mpm_get_collision_time"):
        assert re.search(rf"\bT {sym}$", out, re.M), f"{sym} is not exported"
    for name in ("set_collision_clock", "get_collision_time"):
        assert name in _ffi.HIP_ONLY and name not in _ffi.SIGNATURES             # (the oracle's time is set with the object)
    api = _ffi.load_hip()
    assert api.set_collision_clock.argtypes == [C.c_void_p, C.c_int, C.c_float] and api.set_collision_clock.restype is C.c_int
    assert len(api.get_collision_time.argtypes) == 3
    assert callable(Engine.set_collision_clock) and callable(Engine.collision_time)
    sc = scenes.sphere_through_block(**SCENE)
    assert sc["collision"]["animate"] is True and sc["collision"]["trans_vel"][0] == SCENE["speed"]


@pytest.mark.parametrize("boundary", ["sticky", "slip", "separate"])
def test_oracle_moving_sphere_displaces_the_block(boundary):
    """With the clock driven the sphere ploughs into the block: the block's centroid moves along the sphere's motion and no particle ends
    deeper than 1.25 dx (test_oracle_obstacle_stops_the_sphere's bound) inside the MOVED level set.  With the time held at 0 the object
    never reaches the block, which stays the initial lattice bit for bit.
    Particles carry no identity through a run, so "more than one cell away from the held-clock run" is counted as: farther than one cell from
    EVERY particle of the held run - a lower bound of a particle's own displacement.  Required share: >= 10 % (measured on the oracle:
    sticky 30 %, slip 28 %, separate 28 %)."""
    sc = scenes.sphere_through_block(boundary=boundary, **SCENE)
    dx = 1.0 / 64
    xm, mv, _, T = drive_oracle(sc, STEPS, moving=True)
    xh, _, _, _ = drive_oracle(sc, STEPS, moving=False)
    x0 = sc["models"][0]["xyz"]
    order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
    assert np.array_equal(order(xh), order(x0))
    assert T == pytest.approx(STEPS * sc["dt"], rel=1e-5)
    shift = (xm.astype(np.float64).mean(axis=0) - xh.astype(np.float64).mean(axis=0)) / dx
    assert shift[0] > 2.0 and abs(shift[1]) < 0.5 * shift[0] and abs(shift[2]) < 0.5 * shift[0], shift
    away = cKDTree(xh.astype(np.float64)).query(xm.astype(np.float64))[0] / dx
    print(boundary, "share farther than one cell:", (away > 1.0).mean(), "centroid shift / dx:", shift)
    assert (away > 1.0).mean() >= 0.10, (away > 1.0).mean()
    centre = np.array(sc["collision"]["trans"], dtype=np.float64) + np.array(sc["collision"]["trans_vel"], dtype=np.float64) * T
    depth = SCENE["radius_cells"] * dx - np.linalg.norm(xm.astype(np.float64) - centre, axis=1)
    assert depth.max() < 1.25 * dx, depth.max() / dx
    assert np.isfinite(mv).all() and mv.max() > 0


@pytest.fixture(scope="module")
def host_collision(tmp_path_factory):
    """tools/hostcheck/check_collision.cpp: mpm_collision.hpp built for x86 without contraction."""
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhostcollision.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tools", "hostcheck"),
                           "-I" + entry.CSRC, "-o", out, os.path.join(ROOT, "tools", "hostcheck", "check_collision.cpp")])
    return C.CDLL(out)


def test_pose_split_matches_the_oracle_on_g14(host_collision):
    """collision_pose (host, once per launch) + collision_resolve (per node) against mpmo_fn_collision_resolve on G14's twelve configurations and
    384 nodes.  t = 0: bit for bit (the pose is {start orientation, 1, trans} exactly).  t = 0.37: the same nodes hit and values within
    4e-6 * max(1, |v|max) - what test_g14_detect_and_resolve_collision allows the oracle against the reference's own code (libm's cosf /
    sinf; here both sides call the same libm and multiply in the same order, so the difference is expected to be zero as well)."""
    from test_oracle_golden import f32, hashed_sdf_field, i32, ptr
    api = oracle_api()
    cfg = _ffi.Config()
    assert api.default_config(8, C.byref(cfg)) == 0
    ctx = C.c_void_p()
    assert api.create(C.byref(cfg), 0, C.byref(ctx)) == 0
    field = hashed_sdf_field(256)
    field = [np.ascontiguousarray(f) for f in field]
    field4 = np.ascontiguousarray(np.stack(field, axis=-1))
    cfgs = f32("g14_col_cfg.f32").reshape(-1, 23)
    nodes = i32("g14_col_nodes.i32")
    vin = f32("g14_col_vel_in.f32")
    m = nodes.size // 3
    assert cfgs.shape[0] == 12
    host_collision.host_collision_resolve.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p]
    moving = 0
    try:
        for cf in cfgs:
            obj = _ffi.CollisionObject()
            api.default_collision_object(C.byref(obj))
            obj.type, obj.friction, obj.scale, obj.dsdt = int(cf[0]), float(cf[1]), float(cf[2]), float(cf[3])
            for d in range(3):
                obj.trans[d], obj.trans_vel[d], obj.omega[d] = float(cf[4 + d]), float(cf[7 + d]), float(cf[10 + d])
            for e in range(9):
                obj.rot_mat[e] = float(cf[13 + e])
            assert api.set_collision_object(ctx, C.byref(obj), ptr(field[0]), ptr(field[1]), ptr(field[2]), ptr(field[3])) == 0
            want = vin.copy()
            assert api.raw.mpmo_fn_collision_resolve(ctx, ptr(nodes), m, float(cf[22]), ptr(want)) == 0
            got = vin.copy()
            assert host_collision.host_collision_resolve(C.byref(obj), ptr(field4), 256, 1.0 / 256, cfg.boundary_blocks, 64, ptr(nodes), m, float(cf[22]), ptr(got)) == 0
            assert 0.2 < (want.reshape(m, 3) != vin.reshape(m, 3)).any(axis=1).mean() < 0.8
            if cf[22] == 0.0:
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (cf[:4],)
            else:
                moving += 1
                err = np.abs(got - want).max()
                print("t = %.2f type %d friction %.1f: max |host - oracle| = %g" % (cf[22], int(cf[0]), cf[1], err))
                assert np.array_equal(got != vin, want != vin)
                assert err <= 4e-6 * max(1.0, np.abs(want).max()), (cf[:4], err)
    finally:
        api.destroy(ctx)
    assert moving == 6

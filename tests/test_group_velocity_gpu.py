"""Velocity output of a multi-GPU group (mpm_group_retrieve_velocity, mpm_group_particle_momentum) and the totals of a single context
(mpm_particle_momentum), with every rank a context of ONE GPU: the in-process LocalGroup (one thread per rank), or the RCCL double in a
subprocess (this file run as a script, see the bottom).

The premise of the group readout is checked first: at the return of every group call, and inside mpm_group_main_loop's on_frame, each
rank's grid[0] holds the mass and momentum summed over the ranks on every block it holds - the same values on every rank that holds a
block, and, as a union, the grid of a single context on the same scene.  Then the readout run on those grids equals the single engine's."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import EngineError, build_engine  # noqa: E402
from claymore_amd.mgsp import LocalGroup, MgspGroupRank, partition_scene  # noqa: E402

DT = 1e-4


def collision(material=_ffi.FIXED_COROTATED, gravity=None):
    """Two spheres in head-on contact (the scene of test_mgsp_gpu.py's test_cpp_group_equals_single_engine): the slab cut crosses both, and
    the velocity field is not uniform near the contact."""
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4, material=material)
    if material == _ffi.SAND:
        for m in sc["models"]:
            m["params"] = {}
    if gravity is not None:
        sc["config"] = dict(sc["config"], gravity=gravity)
    return sc


def run_group(sc, world, script, timeout=600):
    """`world` ranks of an in-process group on GPU 0, script(sim) on every rank's own thread; returns the scripts' results."""
    lg = LocalGroup(world)
    ranks = [MgspGroupRank(sc, r, world, device=0, local_group=lg) for r in range(world)]
    lg.create()
    out, errors = [None] * world, []

    def work(r):
        try:
            out[r] = script(ranks[r])
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    for r in ranks:
        r.close()
    assert not errors, errors
    return out


def set_transport(monkeypatch, transport):
    if transport.startswith("peer"):
        monkeypatch.setenv("MPM_GROUP_TRANSPORT", "peer")
    else:
        monkeypatch.delenv("MPM_GROUP_TRANSPORT", raising=False)
    if transport.endswith("tightpad"):
        monkeypatch.setenv("MPM_GROUP_PAD_TIGHT", "1")
    else:
        monkeypatch.delenv("MPM_GROUP_PAD_TIGHT", raising=False)


# ---- float64 references (restated from test_particle_velocity_gpu.py) -----------------------------------------------------------------------------
from test_particle_velocity_gpu import gather64, node_velocities  # noqa: E402


def union_grid(dumps):
    """{key: block (4, 64) float64} of the ranks' dumps, and the worst relative difference between two ranks' copies of one block (per
    channel scale: mass, and one scale shared by the momentum channels)."""
    allb = np.concatenate([b for _, b in dumps]).astype(np.float64)
    scale = np.abs(allb).max(axis=(0, 2))
    scale[1:] = scale[1:].max()
    grid, worst = {}, 0.0
    for keys, blocks in dumps:
        for k, b in zip(keys, blocks):
            k = tuple(int(x) for x in k)
            b = b.astype(np.float64)
            if k in grid:
                worst = max(worst, float((np.abs(grid[k] - b) / scale[:, None]).max()))
            else:
                grid[k] = b
    return grid, worst


def compare_grids(ga, gb):
    """Node-by-node comparison of two {key: block} grids on the keys of either (a key missing on one side must be empty on the other), relative
    to the per-channel scale of gb as parity_util.grid_compare."""
    allb = np.stack(list(gb.values()))
    scale = np.abs(allb).max(axis=(0, 2))
    scale[1:] = scale[1:].max()
    worst = 0.0
    for k in set(ga) | set(gb):
        a, b = ga.get(k), gb.get(k)
        if a is None or b is None:
            assert np.all((a if a is not None else b) == 0), f"block {k} holds mass on one side only"
            continue
        worst = max(worst, float((np.abs(a - b) / scale[:, None]).max()))
    return worst


def as_grid(keys, blocks):
    return {tuple(int(x) for x in k): b.astype(np.float64) for k, b in zip(keys, blocks)}


def match_rows(xa, xb):
    from parity_util import match
    idx, _ = match(xa.astype(np.float64), xb.astype(np.float64))
    return idx


# ---- 1. the summed grid ------------------------------------------------------------------------------------------------------------------------
def test_every_rank_holds_the_summed_grid():
    """After mpm_group_initial_setup, mpm_group_substep, mpm_group_run_fixed(20) and inside on_frame: a block that two ranks hold has the same
    mass and momentum on both (float-atomic noise), and the union of the ranks' grids is a single context's grid after the same substeps
    within parity_util.grid_compare's bound (1e-5 of the channel's largest value)."""
    sc = collision()
    stages = ["setup", "substep", "run_fixed", "on_frame"]

    def script(sim):
        d = [sim.eng.dump_grid()]
        sim.substep(DT, DT)
        d.append(sim.eng.dump_grid())
        sim.run_fixed(20, DT)
        d.append(sim.eng.dump_grid())
        frames = []
        sim.main_loop(1, 2000, DT, on_frame=lambda f: frames.append(sim.eng.dump_grid()))
        d.append(frames[0])
        return d

    eng = build_engine(sc)
    eng.initial_setup()
    single = [as_grid(*eng.dump_grid())]
    eng.run_fixed(1, DT)
    single.append(as_grid(*eng.dump_grid()))
    eng.run_fixed(20, DT)
    single.append(as_grid(*eng.dump_grid()))
    eng.close()
    for world in (2, 3):
        res = run_group(sc, world, lambda sim: (sim.initial_setup(), script(sim))[1])
        for s, name in enumerate(stages):
            dumps = [r[s] for r in res]
            keys = [set(map(tuple, k.tolist())) for k, _ in dumps]
            shared = sum(len(keys[a] & keys[b]) for a in range(world) for b in range(a + 1, world))
            assert shared > 0, (world, name)                                     # the cut crosses blocks both sides hold
            grid, worst = union_grid(dumps)
            print(f"world {world} {name}: {shared} shared blocks, ranks differ by {worst:.3g}")
            assert worst < 1e-5, (world, name, worst)
            if s < len(single):
                cmp = compare_grids(grid, single[s])
                print(f"world {world} {name}: union vs single context {cmp:.3g}")
                assert cmp < 1e-5, (world, name, cmp)


# ---- 2. readout equals the single engine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["in-process", "peer", "peer-tightpad"])
@pytest.mark.parametrize("material", [_ffi.SAND, _ffi.FIXED_COROTATED])
def test_group_readout_equals_single_engine(material, transport, monkeypatch):
    """World 2 and 3: the ranks' mpm_group_retrieve_velocity, concatenated and matched by position, against one context's mpm_retrieve_velocity
    after the same 30 substeps, and against the float64 gather from the ranks' summed dumps (the union of the grids).  Measured on one MI355X
    over all parameters: v within 2.0e-6 of max |v| and C within 3.2e-6 of max |C| of the single engine (bounds 5e-6 / 6e-6, tightened from
    the 1e-5 / 1e-5 first asked for); against the float64 gather 4.3e-7 / 4.9e-7 (bound 1e-6)."""
    set_transport(monkeypatch, transport)
    sc = collision(material)
    nsteps = 30
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(nsteps, DT)
    one = [eng.retrieve_velocity(m, affine=True) for m in range(2)]
    eng.close()

    def script(sim):
        sim.initial_setup()
        sim.run_fixed(nsteps, DT)
        out = [sim.retrieve_velocity(m, affine=True) for m in range(2)]
        plain = [sim.retrieve_velocity(m) for m in range(2)]
        return out, plain, sim.eng.dump_grid()

    for world in (2, 3):
        res = run_group(sc, world, script)
        grid, _ = union_grid([r[2] for r in res])
        V = node_velocities(np.array(list(grid)), np.stack(list(grid.values())), sc["bits"])
        for m in range(2):
            x = np.concatenate([r[0][m][0] for r in res])
            v = np.concatenate([r[0][m][1] for r in res])
            c = np.concatenate([r[0][m][2] for r in res])
            for r in res:                                          # without C: the same particles, the same values (slot order is unspecified)
                a, b = np.lexsort(r[0][m][0].T[::-1]), np.lexsort(r[1][m][0].T[::-1])
                assert np.array_equal(r[1][m][0][b], r[0][m][0][a]) and np.array_equal(r[1][m][1][b], r[0][m][1][a])
            xo, vo, co = one[m]
            assert x.shape == xo.shape
            idx = match_rows(xo, x)
            vmax, cmax = np.abs(vo).max(), np.abs(co).max()
            dv = np.abs(v[idx] - vo).max()
            dc = np.abs(c[idx] - co).max()
            vr, cr = gather64(x, V, sc["bits"])
            dv64, dc64 = np.abs(v - vr).max(), np.abs(c - cr).max()
            spread = np.abs(vo - vo.mean(axis=0)).max()
            print(f"world {world} model {m}: |dv| {dv:.3g} of {vmax:.3g}, |dC| {dc:.3g} of {cmax:.3g}; vs float64 gather {dv64:.3g} / {dc64:.3g}; spread {spread:.3g}")
            assert spread > 0.05 * vmax                             # the collision makes the field non-uniform
            assert dv <= 5e-6 * vmax, (world, m, dv, vmax)
            assert dc <= 6e-6 * cmax, (world, m, dc, cmax)
            assert dv64 <= 1e-6 * np.abs(vr).max(), (world, m, dv64)
            assert dc64 <= 1e-6 * np.abs(cr).max(), (world, m, dc64)


# ---- 3. totals ---------------------------------------------------------------------------------------------------------------------------------
def _sum64(eng, sc, models):
    n, p, k = 0, np.zeros(3), 0.0
    for m in models:
        _, v = eng.retrieve_velocity(m)
        mass = eng.model_mass(m)
        v = v.astype(np.float64)
        n += v.shape[0]
        p += mass * v.sum(axis=0)
        k += 0.5 * mass * float(np.sum(v * v))
    return n, p, k


def test_single_context_momentum_equals_float64_sum_of_the_readout():
    sc = collision()
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(30, DT)
    for model in (None, 0, 1):
        got = eng.particle_momentum(model)
        n, p, k = _sum64(eng, sc, [0, 1] if model is None else [model])
        assert got["count"] == n
        scale = np.abs(p).max() if model is not None else max(abs(eng.model_mass(0)) * 2.0 * n, 1e-30)   # (all models: the two momenta cancel)
        assert np.abs(got["momentum"] - p).max() <= 1e-6 * scale, (model, got, p)
        assert abs(got["kinetic"] - k) <= 1e-6 * k, (model, got, k)
    assert eng.particle_momentum()["count"] == sum(m["xyz"].shape[0] for m in sc["models"])
    eng.close()


@pytest.mark.parametrize("world", [2, 3])
def test_group_momentum_is_identical_on_every_rank_and_equals_the_single_engine(world):
    sc = collision()
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(30, DT)
    one = {m: eng.particle_momentum(m) for m in (None, 0, 1)}
    eng.close()

    def script(sim):
        sim.initial_setup()
        sim.run_fixed(30, DT)
        return {m: sim.particle_momentum(m) for m in (None, 0, 1)}

    res = run_group(sc, world, script)
    for m in (None, 0, 1):
        vals = [np.concatenate([[r[m]["count"]], r[m]["momentum"], [r[m]["kinetic"]]]) for r in res]
        for v in vals[1:]:
            assert np.array_equal(v.view(np.uint64), vals[0].view(np.uint64)), (m, vals)
        o = one[m]
        assert res[0][m]["count"] == o["count"]
        pscale = np.abs(one[0]["momentum"]).max()                 # (one sphere's momentum: the two spheres' cancel in the total)
        assert np.abs(res[0][m]["momentum"] - o["momentum"]).max() <= 1e-5 * pscale, (m, res[0][m], o)
        assert abs(res[0][m]["kinetic"] - o["kinetic"]) <= 1e-5 * o["kinetic"], (m, res[0][m], o)
    assert res[0][None]["count"] == sum(m["xyz"].shape[0] for m in sc["models"])


def test_head_on_collision_conserves_momentum_while_kinetic_energy_drops():
    """Two equal spheres, gravity off: sum m v stays zero (float noise) through the impact while the kinetic energy goes into the bodies."""
    sc = collision(gravity=0.0)
    world = 2
    per = 40

    def script(sim):
        sim.initial_setup()
        out = [sim.particle_momentum()]
        for _ in range(5):
            sim.run_fixed(per, DT)
            out.append(sim.particle_momentum())
        return out

    res = run_group(sc, world, script)
    series = res[0]
    k0 = series[0]["kinetic"]
    mv_one = k0 / 2.0                                           # |M v| of one sphere: K0 = 2 (M v^2 / 2) with v = 2 m/s
    print([(s["momentum"].tolist(), s["kinetic"]) for s in series])
    for s in series:
        assert np.abs(s["momentum"]).max() <= 1e-5 * mv_one, s
    assert series[-1]["kinetic"] < 0.9 * k0, [s["kinetic"] for s in series]


# ---- 4. state and error codes ------------------------------------------------------------------------------------------------------------------
def test_state_and_error_codes():
    sc = collision()
    world = 2
    def sorted_rows(arrs):
        order = np.lexsort(arrs[0].T[::-1])
        return [a[order] for a in arrs]

    def codes(fn):
        try:
            fn()
            return 0
        except EngineError as e:
            return e.code

    def script(sim):
        api, g = sim.api, sim.grp
        out = {}
        n = C.c_size_t(10)
        buf = np.zeros((10, 3), dtype=np.float32)
        tot = (C.c_double * 5)()
        out["not_ready_v"] = api.group_retrieve_velocity(g, 0, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), None, C.byref(n))
        out["not_ready_p"] = api.group_particle_momentum(g, -1, tot)           # (collective: both ranks call it)
        sim.initial_setup()
        out["ok_after_setup"] = codes(lambda: sim.retrieve_velocity(0)) + codes(lambda: sim.particle_momentum())
        sim.run_fixed(3, DT)
        before = sorted_rows(sim.retrieve_velocity(1, affine=True))
        mom_before = sim.particle_momentum()
        ck = sim.save_checkpoint()
        # a phase-level call on the grouped context: INVALID until the next group call
        sim.eng.grid_update(DT)
        out["after_phase_v"] = codes(lambda: sim.retrieve_velocity(0))
        out["after_phase_p"] = codes(lambda: sim.particle_momentum())
        # a checkpoint load is phase-level as well; mpm_group_resume (a group call) makes the readout valid again, with the same output
        sim.eng.load_checkpoint(ck)
        out["after_load_v"] = codes(lambda: sim.retrieve_velocity(0))
        sim._check(api.group_resume(g))
        after = sorted_rows(sim.retrieve_velocity(1, affine=True))
        out["resume_same"] = all(np.array_equal(a, b) for a, b in zip(before, after))
        out["resume_mom"] = (mom_before, sim.particle_momentum())
        # bad arguments and short arrays (readout errors leave the group usable)
        out["bad_model_v"] = api.group_retrieve_velocity(g, 5, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), None, C.byref(n))
        out["bad_model_p"] = codes(lambda: sim.particle_momentum(5))
        out["null_v"] = api.group_retrieve_velocity(g, 0, None, None, None, C.byref(n))
        out["null_p"] = api.group_particle_momentum(g, -1, None)
        n = C.c_size_t(10)
        out["short_v"] = api.group_retrieve_velocity(g, 0, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p), None, C.byref(n))
        out["short_n"] = n.value
        sim.run_fixed(2, DT)
        out["usable"] = codes(lambda: sim.retrieve_velocity(0)) + codes(lambda: sim.particle_momentum())
        # the single-context readouts stay refused on a grouped context
        out["single_refused"] = codes(lambda: sim.eng.retrieve_velocity(0)) + 100 * codes(lambda: sim.eng.particle_momentum())
        return out

    res = run_group(sc, world, script)
    for r, o in enumerate(res):
        assert o["not_ready_v"] == _ffi.MPM_ERR_NOT_READY and o["not_ready_p"] == _ffi.MPM_ERR_NOT_READY, (r, o)
        assert o["ok_after_setup"] == 0, (r, o)
        assert o["after_phase_v"] == _ffi.MPM_ERR_INVALID and o["after_phase_p"] == _ffi.MPM_ERR_INVALID, (r, o)
        assert o["after_load_v"] == _ffi.MPM_ERR_INVALID, (r, o)
        assert o["usable"] == 0, (r, o)
        assert o["bad_model_v"] == o["bad_model_p"] == o["null_v"] == o["null_p"] == _ffi.MPM_ERR_INVALID, (r, o)
        assert o["short_v"] == _ffi.MPM_ERR_CAPACITY and o["short_n"] == 10, (r, o)
        assert o["single_refused"] == _ffi.MPM_ERR_INVALID * 101, (r, o)
        assert o["resume_same"], r
        mb, ma = o["resume_mom"]
        assert mb["count"] == ma["count"]
        assert np.abs(mb["momentum"] - ma["momentum"]).max() <= 1e-9 * max(abs(mb["kinetic"]), 1.0)
        assert abs(mb["kinetic"] - ma["kinetic"]) <= 1e-9 * mb["kinetic"]


@pytest.fixture(scope="session")
def rccl_double_library(tmp_path_factory):
    """tests/rccl_double/rccl_double.cpp built with hipcc, as test_mgsp_gpu.py's fixture of the same name does."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path_factory.mktemp("rccl_double_v") / "librccl_double.so"
    src = os.path.join(HERE, "rccl_double", "rccl_double.cpp")
    subprocess.run([hipcc, "-O1", "-std=c++17", "-fPIC", "-shared", "-o", str(out), src, "-lpthread"], check=True, capture_output=True, timeout=600)
    return str(out)


def test_state_after_a_failed_group_call(rccl_double_library):
    """A rank outgrows its block capacity inside mpm_group_run_fixed (tests/rccl_double/run_group.py's "fail" scene): every rank returns
    MPM_ERR_CAPACITY, and then both readouts return MPM_ERR_INVALID on every rank - the grid is no longer known to be summed."""
    env = dict(os.environ, MPM_RCCL_LIBRARY=rccl_double_library)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "2", "fail"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK world 2 fail" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ---- 5. the RCCL transport ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_rccl_double_totals_equal_the_in_process_transport(world, rccl_double_library):
    """The RCCL branch (ncclAllGather of the ranks' rows) through the in-process double, in a subprocess: the totals agree with the in-process
    transport's, and a readout error on one rank (a bad model) is returned by every rank."""
    sc = collision()

    def script(sim):
        sim.initial_setup()
        sim.run_fixed(30, DT)
        return sim.particle_momentum()

    local = run_group(sc, world, script)[0]
    env = dict(os.environ, MPM_RCCL_LIBRARY=rccl_double_library)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(world), "totals"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"OK world {world} totals" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("TOTALS ")][0]
    vals = np.array([float.fromhex(x) for x in line.split()[1:]])
    want = np.concatenate([[local["count"]], local["momentum"], [local["kinetic"]]])
    assert vals[0] == want[0]
    pscale = np.abs(want[1:4]).max() + 1e-3 * want[4]
    assert np.abs(vals[1:4] - want[1:4]).max() <= 1e-5 * pscale, (vals, want)
    assert abs(vals[4] - want[4]) <= 1e-5 * want[4], (vals, want)


# ---- 6. mgsp --output-velocity -----------------------------------------------------------------------------------------------------------------
def test_mgsp_output_velocity(tmp_path):
    """Scenario 2 of the mgsp driver (two elastic cubes side by side, one per rank, falling under MGSP's gravity -4.9 m/s^2) with and without
    --output-velocity: the flag adds "v" to every frame; frame 0 is byte for byte the position part of the plain one with v = v0 = 0; later
    frames hold the same particles (positions to float noise: P2G's float atomics make two runs differ in the last bits) and v is the group
    readout at that frame - the same scene run by an in-process group whose main loop reads out in on_frame; without the flag nothing changes
    (the plain frames are position-only, as test_host_driver.py checks against the oracle)."""
    from test_particle_velocity_cpu import read_bgeo_v
    from test_particle_velocity_gpu import _read_bgeo_any
    import __graft_entry__ as g
    g.build_host()
    exe = os.path.join(HERE, os.pardir, "claymore_amd", "host", "mgsp")
    frames, fps, bits = 2, 48, 7
    runs = {}
    for flag in (False, True):
        d = tmp_path / ("v" if flag else "plain")
        d.mkdir()
        cmd = [exe, "--devices", "2", "--same-device", "--bits", str(bits), "--frames", str(frames), "--fps", str(fps), "--out", str(d)]
        subprocess.run(cmd + (["--output-velocity"] if flag else []), check=True, capture_output=True, text=True, timeout=600)
        runs[flag] = d
    # the same scene through the Python layer (host/mgsp.cpp scenario 2, as test_host_driver.py restates it)
    n = 1 << bits
    dx = 1.0 / n
    length, stride, o = 54 * n // 256, 56 * n // 256, 18 * n // 256
    local = []
    for d in range(2):
        lo = (o + (stride if d & 1 else 0), o, o)
        hi = tuple(c + length for c in lo)
        local.append({"name": "mgsp_scenario2", "bits": bits, "dt": 1e-4, "config": {"max_ppc": 128, "gravity": -9.8 * 0.5, "cfl": 0.3},
                      "models": [{"material": _ffi.FIXED_COROTATED, "xyz": scenes.lattice_box(bits, lo, hi), "v0": (0.0, 0.0, 0.0),
                                  "params": {"volume": float(np.float32(dx) ** 3 / np.float32(8.0))}}]})
    lg = LocalGroup(2)
    ranks = [MgspGroupRank(local[r], r, 2, device=0, local_group=lg, prepartitioned=True) for r in range(2)]
    lg.create()
    readout, errors = [{}, {}], []

    def work(r):
        try:
            sim = ranks[r]
            sim.initial_setup()
            sim.main_loop(frames, fps, 1e-4, on_frame=lambda f: readout[r].__setitem__(f, sim.retrieve_velocity(0)))
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    for r in ranks:
        r.close()
    assert not errors, errors
    for dev in range(2):
        for f in range(frames + 1):
            name = f"model_dev[{dev}]_frame[{f}].bgeo"
            xp, vp = _read_bgeo_any(runs[False] / name)
            xv, vv = read_bgeo_v(runs[True] / name)
            assert vp is None and xp.shape == xv.shape
            if f == 0:
                assert open(runs[False] / name, "rb").read()[41:] == b"".join(
                    open(runs[True] / name, "rb").read()[62:-2][28 * i:28 * i + 16] for i in range(xv.shape[0])) + b"\x00\xff"
                assert np.array_equal(xp, xv) and np.all(vv == 0.0)
                continue
            idx = match_rows(xp, xv)
            assert np.abs(xp - xv[idx]).max() < 1e-5
            xr, vr = readout[dev][f]
            assert xr.shape == xv.shape
            j = match_rows(xv, xr)
            dv = np.abs(vv - vr[j]).max()
            vmax = np.abs(vr).max()
            print(f"dev {dev} frame {f}: |v - group readout| {dv:.3g} of max |v| {vmax:.3g}; positions {np.abs(xv - xr[j]).max():.3g}")
            assert vmax > 0.1 and dv <= 1e-5 * vmax, (dev, f, dv, vmax)        # (measured 2.1e-6: two runs differ by float-atomic noise)


# ---- subprocess driver of the RCCL double (MPM_RCCL_LIBRARY set): python test_group_velocity_gpu.py WORLD totals|fail ------------------------------
def _rccl_ranks(locals_, world, script):
    ident, have_id = {}, threading.Event()

    def bootstrap(raw):
        if raw is not None:
            ident["raw"] = raw
            have_id.set()
        else:
            assert have_id.wait(120)
        return ident["raw"]

    out, sims = [None] * world, [None] * world

    def work(rank):
        try:
            sims[rank] = MgspGroupRank(locals_[rank], rank, world, device=0, bootstrap=bootstrap, prepartitioned=True)
            out[rank] = script(sims[rank])
        except Exception as e:  # noqa: BLE001
            out[rank] = ("exception", repr(e))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), f"a rank is stuck in a collective: {out}"
    for s in sims:
        if s is not None:
            s.close()
    return out


def _code(fn):
    try:
        fn()
        return 0
    except EngineError as e:
        return e.code


def _main(world, kind):
    if kind == "totals":
        sc = collision()
        locals_ = [partition_scene(sc, r, world) for r in range(world)]

        def script(sim):
            assert sim.api.group_transport(sim.grp).decode() == "rccl"
            sim.initial_setup()
            sim.run_fixed(30, DT)
            tot = sim.particle_momentum()
            bad = _code(lambda: sim.particle_momentum(7 if sim.rank == world - 1 else None))     # one rank asks for a model it lacks
            again = sim.particle_momentum()
            return tot, bad, again

        out = _rccl_ranks(locals_, world, script)
        assert all(isinstance(o[0], dict) for o in out), out
        vals = [np.concatenate([[o[0]["count"]], o[0]["momentum"], [o[0]["kinetic"]]]) for o in out]
        assert all(np.array_equal(v, vals[0]) for v in vals), vals
        assert all(o[1] == _ffi.MPM_ERR_INVALID for o in out), [o[1] for o in out]
        assert all(o[2]["kinetic"] == out[0][2]["kinetic"] for o in out)             # the group is still usable (every rank the same bits;
        assert abs(out[0][2]["kinetic"] - out[0][0]["kinetic"]) <= 1e-12 * out[0][0]["kinetic"]   # the device's float64 atomics: last bits may vary)
        print("TOTALS " + " ".join(float(x).hex() for x in vals[0]))
        print(f"OK world {world} totals")
    elif kind == "fail":
        import copy
        sc = scenes.sphere_drop(bits=6, radius_cells=6.0, center=(0.5, 0.26, 0.5), material=_ffi.SAND)
        sc["models"][0]["params"] = {}
        sc["models"][0]["v0"] = (0.0, -4.0, 0.0)
        locals_ = [copy.deepcopy(partition_scene(sc, r, world)) for r in range(world)]
        probe = build_engine(locals_[1])
        probe.initial_setup()
        ebc0 = probe.counts().exterior_blocks
        probe.close()
        locals_[1]["config"] = dict(locals_[1].get("config", {}), max_blocks=ebc0 + 8, grow=0)

        def script(sim):
            sim.initial_setup()
            ok = _code(lambda: sim.retrieve_velocity(0)) + _code(lambda: sim.particle_momentum())
            rc = _code(lambda: sim.run_fixed(900, DT))
            return ok, rc, _code(lambda: sim.retrieve_velocity(0)), _code(lambda: sim.particle_momentum())

        out = _rccl_ranks(locals_, world, script)
        assert all(o[0] == 0 for o in out), out
        assert all(o[1] == _ffi.MPM_ERR_CAPACITY for o in out), out
        assert all(o[2] == _ffi.MPM_ERR_INVALID and o[3] == _ffi.MPM_ERR_INVALID for o in out), out
        print(f"OK world {world} fail: {out}")
    else:
        raise SystemExit(f"unknown kind {kind}")


if __name__ == "__main__":
    _main(int(sys.argv[1]), sys.argv[2])
else:
    pytestmark = pytest.mark.gpu

"""Per-particle initial conditions on the GPU (mpm_add_model_particles, mpm_set_model_velocity_field; claymore_amd/csrc/mpm_particle_init.hpp):
the state a model is given comes back bit for bit, the set-up grid is the float64 model's (tests/particle_init_model.py) node by node within a
bound counted from the kernel's statements, a linear velocity field is reproduced by the grid and by the velocity readout, a snapshot re-seeds
a second context, the refusals refuse, and a group's ranks start from their shares of the arrays.

Every numeric bound is (n + r) roundings of 2^-24 times the sum of the terms' magnitudes: n the number of terms of the sum, r the roundings of one
term, counted in particle_init_model.py beside the kernel's own count.  None was fitted to what the kernels return."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ckpt_format as cf  # noqa: E402
import face_scenes as fs  # noqa: E402
import g2p2g_bench as gb  # noqa: E402
import g2p2g_model as gm  # noqa: E402
import particle_init_model as pim  # noqa: E402
from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import EngineError, build_engine  # noqa: E402

pytestmark = pytest.mark.gpu

U = pim.U
DX = np.float32(0.5 ** gm.BITS)
POSITIONS = {"block_sizes": gm.scene_block_sizes, "one_cell": gm.scene_one_cell, "cluster": gm.scene_cluster}


def state9_of(material, st):
    """make_state's state as mpm_retrieve_state would return it (state_kind "b")"""
    if material == gm.J_FLUID:
        s = np.zeros((st["J"].shape[0], 9), np.float32)
        s[:, 0] = st["J"]
        return s
    b = st["b6"]
    s = np.stack([np.where(st["reflected"], -b[:, 0], b[:, 0]), b[:, 3], b[:, 4], b[:, 3], b[:, 1], b[:, 5], b[:, 4], b[:, 5], b[:, 2]], axis=1)
    return np.ascontiguousarray(s, np.float32)


def model_dict(material, pos_cells, **extra):
    return dict({"material": material, "xyz": np.ascontiguousarray(pos_cells, np.float32) * DX, "v0": (0.0, 0.0, 0.0),
                 "params": dict(gm.material_overrides(material))}, **extra)


def scene_of(models, bits=gm.BITS, max_ppc=gm.MAX_PPC, **extra):
    return dict({"name": "particle_init", "bits": bits, "dt": gm.DT, "config": {"max_ppc": max_ppc}, "models": models}, **extra)


def set_up(sc):
    eng = build_engine(sc)
    eng.initial_setup()
    return eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_state_is(eng, model, material, pos_cells, st):
    """retrieve_state of `model`, joined on the position bits, holds st bit for bit"""
    x, s9, lj = eng.retrieve_state(model)
    assert x.shape[0] == pos_cells.shape[0]
    og, ow = gb.by_position_bits(x * np.float32(2.0 ** gm.BITS)), gb.by_position_bits(pos_cells)
    assert same_bits((x * np.float32(2.0 ** gm.BITS))[og], np.ascontiguousarray(pos_cells, np.float32)[ow])
    if material == gm.J_FLUID:
        assert same_bits(s9[og, 0], st["J"][ow])
        return
    b6, refl = gb.st9_to_b6(s9)
    assert same_bits(b6[og], st["b6"][ow]) and np.array_equal(refl[og], st["reflected"][ow])
    if st["logjp"] is not None:
        assert same_bits(lj[og], st["logjp"][ow])


def assert_same_particle_state(a, b):
    """two ckpt_format.particle_state dicts hold the same particles, joined on the position bits"""
    oa, ob = gb.by_position_bits(a["xyz_cells"]), gb.by_position_bits(b["xyz_cells"])
    for k in ("xyz_cells", "b", "reflected", "logjp", "J"):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert same_bits(a[k][oa], b[k][ob]), k


# ---- 1. the state, bit for bit -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", gm.MATERIALS, ids=[gm.NAMES[m] for m in gm.MATERIALS])
def test_state_comes_back_bit_for_bit_and_equals_a_patched_checkpoint(material):
    for si, (name, make) in enumerate(POSITIONS.items()):
        pos = make()
        st = gm.make_state(material, pos.shape[0], 70 + si)
        eng = set_up(scene_of([model_dict(material, pos, state=state9_of(material, st), logjp=st["logjp"], state_kind="b")]))
        assert_state_is(eng, 0, material, pos, st)
        mine = cf.particle_state(eng.save_checkpoint(), 0)
        eng.close()
        plain = gb.Bench([(material, pos)])                      # the route the block tests trust: a plain context's checkpoint, patched
        if material == gm.J_FLUID:
            buf = cf.with_particle_state(plain.ckpt, 0, pos, J=st["J"])
        else:
            buf = cf.with_particle_state(plain.ckpt, 0, pos, b=st["b6"], logjp=st["logjp"], reflected=st["reflected"])
        plain.close()
        assert_same_particle_state(mine, cf.particle_state(buf, 0))


def test_two_models_of_different_materials_and_only_a_logjp():
    pa, pb = gm.scene_cluster(), gm.EXTRA_SCENES["cluster_b"]()
    sa, sb = gm.make_state(gm.SAND, pa.shape[0], 81), gm.make_state(gm.J_FLUID, pb.shape[0], 82)
    pc = gm.scene_isolated()
    lj = np.linspace(-0.02, 0.005, pc.shape[0]).astype(np.float32)
    eng = set_up(scene_of([model_dict(gm.SAND, pa, state=state9_of(gm.SAND, sa), logjp=sa["logjp"]), model_dict(gm.J_FLUID, pb, state=state9_of(gm.J_FLUID, sb)),
                           model_dict(gm.NACC, pc, logjp=lj)]))
    assert_state_is(eng, 0, gm.SAND, pa, sa)
    assert_state_is(eng, 1, gm.J_FLUID, pb, sb)
    ident = dict(b6=np.tile(np.float32([1, 1, 1, 0, 0, 0]), (pc.shape[0], 1)), reflected=np.zeros(pc.shape[0], bool), logjp=lj)
    assert_state_is(eng, 2, gm.NACC, pc, ident)                  # no state9: stress-free, with the given log Jp
    eng.close()


def test_tracked_ids_name_the_input_rows():
    pos = gm.scene_block_sizes()
    st = gm.make_state(gm.FC, pos.shape[0], 83)
    s9 = state9_of(gm.FC, st)
    eng = set_up(scene_of([model_dict(gm.FC, pos, state=s9)], track_ids=True))
    ids, x, got = eng.order_by_id(0, *eng.retrieve_state(0)[:2])
    assert np.array_equal(ids, np.arange(pos.shape[0]))
    assert same_bits(x, pos * DX) and same_bits(got, s9)          # row k of the readout, ordered by id, is input row k
    eng.close()


# ---- 2. state_kind "f" ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", [gm.FC, gm.SAND, gm.NACC], ids=["fc", "sand", "nacc"])
def test_deformation_gradients_become_b(material):
    pos = gm.scene_block_sizes()
    st = gm.make_state(material, pos.shape[0], 90)
    eng = set_up(scene_of([model_dict(material, pos, state=st["F32"], logjp=st["logjp"], state_kind="f")]))
    x, s9, _ = eng.retrieve_state(0)
    eng.close()
    og, ow = gb.by_position_bits(x * np.float32(2.0 ** gm.BITS)), gb.by_position_bits(pos)
    F = st["F32"].astype(np.float64)[ow]
    want = F @ F.transpose(0, 2, 1)
    # b_ij = sum_k F_ik F_jk in float32: three products and two additions -> (3 + 2) u sum_k |F_ik F_jk|
    bound = (3 + 2) * U * (np.abs(F) @ np.abs(F).transpose(0, 2, 1))
    got = s9[og].astype(np.float64).reshape(-1, 3, 3)
    refl = np.signbit(got[:, 0, 0])
    got[:, 0, 0] = np.abs(got[:, 0, 0])
    err = np.abs(got - want)
    print(f"{gm.NAMES[material]}: |b - F F^T| at most {(err / bound).max():.3f} of its bound")
    assert (err <= bound).all()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    det = np.linalg.det(F)
    assert np.abs(det).min() > 0.1 and np.array_equal(refl, det < 0)
    assert refl.any() == bool(st["reflected"].any())


def test_deformation_gradients_become_J_for_the_fluid():
    pos = gm.scene_cluster()
    F32 = gm.make_state(gm.FC, 2 * pos.shape[0], 91)["F32"]
    F32 = F32[np.linalg.det(F32.astype(np.float64)) > 0][:pos.shape[0]]
    assert F32.shape[0] == pos.shape[0]
    eng = set_up(scene_of([model_dict(gm.J_FLUID, pos, state=F32, state_kind="f")]))
    x, s9, _ = eng.retrieve_state(0)
    eng.close()
    og, ow = gb.by_position_bits(x * np.float32(2.0 ** gm.BITS)), gb.by_position_bits(pos)
    F = F32.astype(np.float64)[ow]
    aF = np.abs(F)
    products = sum(aF[:, 0, i] * aF[:, 1, j] * aF[:, 2, k] for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)))
    err = np.abs(s9[og, 0].astype(np.float64) - np.linalg.det(F))
    print(f"jfluid: |J - det F| at most {(err / (8 * U * products)).max():.3f} of its bound")
    assert (err <= 8 * U * products).all()


# ---- 3. the grid after set-up ----------------------------------------------------------------------------------------------------------------
def random_motion(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32), rng.uniform(-50.0, 50.0, (n, 3, 3)).astype(np.float32)


def check_setup_grid(sc, interior, extra_momentum=0):
    """dump_grid against the model node by node, grid_totals against the model's sums; returns (model nodes, bounds, dumped values)"""
    g = pim.setup_nodes(sc)
    nb = pim.node_bounds(g, extra_momentum)
    eng = set_up(sc)
    nodes, val = pim.dumped_nodes(*eng.dump_grid(), sc["bits"])
    tot = eng.grid_totals()
    eng.close()
    assert np.array_equal(nodes, g["nodes"]), "the massed nodes differ"
    err = np.abs(val - g["val"])
    print(f"{sc['name']}: {nodes.shape[0]} nodes, up to {g['count'].max()} terms; worst error / bound per channel {(err / nb).max(axis=0)}")
    assert (err <= nb).all(), np.argwhere(err > nb)[:5]
    want = g["val"].sum(axis=0)
    assert (np.abs(tot - want) <= nb.sum(axis=0)).all(), (tot, want, nb.sum(axis=0))
    if interior:                                                   # nothing falls off the domain: the affine term carries no net momentum
        pm = np.zeros(3)
        for m in sc["models"]:
            _, mass, v, _, _ = pim.model_particles(sc, m)
            pm += mass * v.sum(axis=0)
        assert np.abs(want[1:] - pm).max() <= 1e-12 * g["mag"][:, 1:].sum()
        assert (np.abs(tot[1:] - pm) <= nb[:, 1:].sum(axis=0) + 1e-12 * g["mag"][:, 1:].sum()).all()
    return g, nb, val


@pytest.mark.parametrize("name", sorted(POSITIONS))
def test_setup_grid_with_random_velocities_and_affine(name):
    pos = POSITIONS[name]()
    v, Cm = random_motion(pos.shape[0], 5)
    sc = scene_of([model_dict(gm.FC, pos, velocity=v, affine=Cm)])
    sc["name"] = name
    check_setup_grid(sc, interior=True)


def test_setup_grid_at_the_six_faces():
    """node -1 dropped, the top cells, cells -2 / -1: face_scenes' slab with a velocity and an APIC matrix per particle"""
    sc = fs.setup_slab_scene()
    m = sc["models"][0]
    v, Cm = random_motion(m["xyz"].shape[0], 6)
    per = dict(sc, models=[dict(m, velocity=v, affine=Cm)])
    g, _, _ = check_setup_grid(per, interior=False)
    assert g["outside"]["lo"] > 0 and g["outside"]["hi"] > 0


def test_setup_grid_of_a_lone_particle_and_of_partial_arrays():
    pos = np.float32([[33.3, 20.7, 41.1]])
    v, Cm = random_motion(1, 8)
    sc = scene_of([model_dict(gm.SAND, pos, velocity=v, affine=Cm)])
    sc["name"] = "lone particle"
    g, _, _ = check_setup_grid(sc, interior=True)
    assert g["nodes"].shape[0] == 27
    # a velocity without an affine, and an affine over the model's v0, in one context with a plain model (which takes the uniform kernel)
    pa, pb, pc = gm.scene_cluster(), gm.EXTRA_SCENES["cluster_b"](), gm.scene_isolated()
    va, _ = random_motion(pa.shape[0], 9)
    _, Cb = random_motion(pb.shape[0], 10)
    sc = scene_of([model_dict(gm.FC, pa, velocity=va), model_dict(gm.J_FLUID, pb, affine=Cb, v0=(0.5, -1.0, 0.25)), model_dict(gm.NACC, pc, v0=(1.0, 2.0, -1.5))])
    sc["name"] = "partial arrays"
    check_setup_grid(sc, interior=True)


# ---- 4. a linear field is reproduced ---------------------------------------------------------------------------------------------------------
def field_scene(name):
    sc = scenes.spinning_ball(bits=6) if name == "spinning_ball" else scenes.sheared_block(bits=6)
    sc["config"] = dict(sc["config"], max_ppc=16)
    return sc


def as_arrays(sc, affine=True):
    """the scene's field as per-particle arrays: v_p = fl32(a + A x_p), C_p = A"""
    m = sc["models"][0]
    a, A = scenes.model_velocity_field(m)
    x = m["xyz"].astype(np.float64)
    mm = {k: v for k, v in m.items() if k not in ("omega", "velocity_gradient", "pivot")}
    mm["velocity"] = (a[None, :] + x @ A.T).astype(np.float32)
    if affine:
        mm["affine"] = np.broadcast_to(A.astype(np.float32), (x.shape[0], 3, 3)).copy()
    return dict(sc, models=[mm])


def readout_errors(eng_or_rank, a, A):
    x, v, Cp = eng_or_rank.retrieve_velocity(0, affine=True)
    want = a[None, :] + x.astype(np.float64) @ A.T
    return x, np.abs(v - want).max(axis=1), np.abs(Cp.astype(np.float64) - A[None]).max(axis=(1, 2))


@pytest.mark.parametrize("name", ["spinning_ball", "sheared_block"])
def test_linear_field_is_reproduced_by_grid_and_readout(name):
    sc = field_scene(name)
    a, A = scenes.model_velocity_field(sc["models"][0])
    g = pim.setup_nodes(sc)
    nb = pim.node_bounds(g, extra_momentum=pim.R_FIELD)          # (the array form rounds v_p once, the field form forms it in R_FIELD roundings)
    want = a[None, :] + (g["nodes"] / 64.0) @ A.T
    assert np.abs(g["val"][:, 1:] - want * g["val"][:, :1]).max() <= 1e-12 * g["mag"][:, 1:].max()      # the model itself carries the field
    for form, scene in (("field", sc), ("arrays", as_arrays(sc))):
        eng = set_up(scene)
        nodes, val = pim.dumped_nodes(*eng.dump_grid(), 6)
        assert np.array_equal(nodes, g["nodes"])
        # p / m = a + A x_i:  |p - want m| <= |p - p_exact| + |want| |m_exact - m|
        err = np.abs(val[:, 1:] - want * val[:, :1])
        bound = nb[:, 1:] + np.abs(want) * nb[:, :1]
        assert (np.abs(val - g["val"]) <= nb).all()
        assert (err <= bound).all(), (form, (err / bound).max())
        x, ev, ec = readout_errors(eng, a, A)
        eng.close()
        bv, bc = pim.linear_field_bounds(g, nb, x, 6, a, A)
        print(f"{name} / {form}: node error {(err / bound).max():.3f}, v_p error {(ev / bv).max():.3f}, C_p error {(ec / bc).max():.3f} of their bounds; "
              f"|C - A| <= {ec.max():.3g} of {np.abs(A).max():.3g}")
        assert (ev <= bv).all() and (ec <= bc).all(), (form, (ev / bv).max(), (ec / bc).max())
    # the same velocities WITHOUT the affine term: the surface particles do not see C = A, by far more than the bound
    eng = set_up(as_arrays(sc, affine=False))
    x, ev, ec = readout_errors(eng, a, A)
    eng.close()
    _, bc = pim.linear_field_bounds(g, nb, x, 6, a, A)
    worst = int(np.argmax(ec))
    print(f"{name} without affine: |C - A| up to {ec.max():.3g} (bound {bc[worst]:.3g})")
    assert ec[worst] > 100.0 * bc[worst] and ec[worst] > 0.05 * np.abs(A).max()
    assert (ec > bc).mean() > 0.1, "the surface layer"


def test_velocity_field_on_a_mesh_filled_model():
    """mpm_add_model_mesh's positions never reach the host: the field form serves them"""
    verts, faces = scenes.icosphere((0.5, 0.5, 0.5), 6.0 / 64.0, 2)
    omega = (0.0, 10.0, 20.0)
    sc = {"name": "mesh_spin", "bits": 6, "dt": 1e-4, "config": {"max_ppc": 16, "gravity": 0.0},
          "models": [{"material": _ffi.FIXED_COROTATED, "mesh": {"vertices": verts, "faces": faces}, "omega": omega, "pivot": (0.5, 0.5, 0.5),
                      "params": {"volume": scenes._vol(6), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}}]}
    eng = set_up(sc)
    x = eng.retrieve_positions(0)
    a, A = scenes.model_velocity_field(sc["models"][0])
    ref = dict(sc, models=[dict(sc["models"][0], xyz=x)])
    del ref["models"][0]["mesh"]
    g = pim.setup_nodes(ref)
    nb = pim.node_bounds(g, extra_momentum=pim.R_FIELD)
    xr, ev, ec = readout_errors(eng, a, A)
    eng.close()
    bv, bc = pim.linear_field_bounds(g, nb, xr, 6, a, A)
    assert x.shape[0] > 1000 and (ev <= bv).all() and (ec <= bc).all()


# ---- 5. one substep --------------------------------------------------------------------------------------------------------------------------
def test_one_substep_of_the_spinning_ball():
    sc = field_scene("spinning_ball")
    g = pim.setup_nodes(sc)
    # the bound of the set-up grid's total momentum, summed over the nodes.  The ball turns about z, so the z channel's own bound is zero; the
    # substep's P2G adds the stress term, whose roundings reach every channel: each channel is held to the largest channel's bound
    bound = pim.node_bounds(g, extra_momentum=pim.R_FIELD)[:, 1:].sum(axis=0).max()
    eng = set_up(sc)
    n = sc["models"][0]["xyz"].shape[0]
    before = eng.particle_momentum()
    eng.substep(1e-4, 0.0, 1.0, 1e-4)
    after = eng.particle_momentum()
    d = eng.diagnostics()
    print(f"linear momentum before {before['momentum']}, after {after['momentum']}, bound {bound}; kinetic {before['kinetic']:.6g} -> {after['kinetic']:.6g}")
    assert before["count"] == after["count"] == n
    assert (np.abs(before["momentum"]) <= bound).all() and (np.abs(after["momentum"]) <= bound).all()
    assert after["kinetic"] > 0.9 * before["kinetic"] > 0
    assert d.lost_particles == 0 and d.dropped_particles == 0 and d.discarded_p2g == 0 and d.overflow_flags == 0
    assert eng.api.check_table(eng.ctx) == 0
    assert eng.retrieve_positions(0).shape[0] == n
    eng.close()


def test_precompressed_fluid_has_pressure_before_any_substep():
    pos = gm.scene_cluster()
    s9 = np.zeros((pos.shape[0], 9), np.float32)
    s9[:, 0] = 0.9
    pressure = []
    for state in (s9, None):
        eng = set_up(scene_of([model_dict(gm.J_FLUID, pos, state=state)]))
        t = eng.stress_totals()
        pressure.append(-t["stress_integral"][:3].sum() / 3.0)
        assert t["count"] == pos.shape[0]
        eng.close()
    assert pressure[0] > 0 and pressure[1] == 0.0, pressure


# ---- 6. re-seed ------------------------------------------------------------------------------------------------------------------------------
def test_snapshot_reseeds_a_second_context():
    sc = scenes.two_spheres(bits=6, radius_cells=5.0, gap_cells=0.5, speed=2.0, youngs=2e4)
    src = set_up(sc)
    src.run_fixed(20, 1e-4)
    snap = src.snapshot_models()
    states = [src.retrieve_state(m) for m in range(2)]
    src.close()
    assert all(np.abs(s["affine"]).max() > 0 and np.abs(s["state"] - np.eye(3, dtype=np.float32).ravel()).max() > 0 for s in snap)
    new_sc = {"name": "reseed", "bits": 6, "dt": 1e-4, "config": {"max_ppc": 32}, "models": snap}      # another max_ppc
    g = pim.setup_nodes(new_sc)
    nb = pim.node_bounds(g).sum(axis=0)
    dst = set_up(new_sc)
    for m in range(2):
        xa, sa, la = states[m]
        xb, sb, lb = dst.retrieve_state(m)
        oa, ob = gb.by_position_bits(xa), gb.by_position_bits(xb)
        assert same_bits(xa[oa], xb[ob]) and same_bits(sa[oa], sb[ob]) and same_bits(la[oa], lb[ob])
    tot = dst.grid_totals()
    dst.close()
    mass = sum(pim.model_particles(new_sc, m)[1] * m["xyz"].shape[0] for m in snap)
    pm = sum(pim.model_particles(new_sc, m)[1] * m["velocity"].astype(np.float64).sum(axis=0) for m in snap)
    slack = 1e-12 * g["mag"].sum(axis=0)
    print(f"re-seed: mass {tot[0]:.9g} of {mass:.9g} (bound {nb[0]:.3g}), momentum {tot[1:]} of {pm} (bound {nb[1:]})")
    assert abs(tot[0] - mass) <= nb[0] + slack[0]
    assert (np.abs(tot[1:] - pm) <= nb[1:] + slack[1:]).all()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------------
def raw_add(eng, material, xyz, init, params=None):
    p = params if params is not None else eng.default_material(material)
    mid = C.c_int(-1)
    rc = eng.api.add_model_particles(eng.ctx, material, C.byref(p), xyz.ctypes.data, xyz.shape[0], (C.c_float * 3)(0, 0, 0),
                                     None if init is None else C.byref(init), C.byref(mid))
    return rc, mid.value, eng.api.last_error(eng.ctx).decode()


def test_refusals_change_nothing():
    pos = gm.scene_isolated()
    xyz = np.ascontiguousarray(pos * DX)
    n = xyz.shape[0]
    good = {"velocity": np.zeros((n, 3), np.float32), "affine9": np.zeros((n, 9), np.float32), "state9": np.tile(np.eye(3, dtype=np.float32).ravel(), (n, 1)),
            "logjp": np.zeros(n, np.float32)}
    eng = build_engine(scene_of([]))

    def init_with(**over):
        init = _ffi.ParticleInit()
        init.state_kind = _ffi.STATE_B
        keep = []
        for k, v in over.items():
            if isinstance(v, np.ndarray):
                keep.append(np.ascontiguousarray(v, np.float32))
                setattr(init, k, keep[-1].ctypes.data)
            elif k == "reserved":
                init.reserved[v] = 1
            else:
                setattr(init, k, v)
        return init, keep

    cases = {"reserved": (dict(reserved=1), "reserved"), "state_kind": (dict(state9=good["state9"], state_kind=7), "state_kind")}
    for k in good:
        for bad in (np.nan, np.inf):
            a = good[k].copy()
            a.reshape(-1)[a.size // 2] = bad
            cases[f"{k} {bad}"] = ({k: a}, k)
    for entry, label in ((4, "b11"), (8, "b22"), (0, "b00")):
        for value in (0.0, -1.0) if entry else (0.0,):
            a = good["state9"].copy()
            a[n - 1, entry] = value
            cases[f"{label} = {value}"] = (dict(state9=a), "strictly positive")
    for name, (over, word) in cases.items():
        init, keep = init_with(**over)
        rc, _, msg = raw_add(eng, gm.SAND, xyz, init)
        assert rc == _ffi.MPM_ERR_INVALID and word in msg, (name, rc, msg)
    a = good["state9"].copy()
    a[0, 0] = 0.0
    init, keep = init_with(state9=a)
    rc, _, msg = raw_add(eng, gm.J_FLUID, xyz, init)
    assert rc == _ffi.MPM_ERR_INVALID and "J" in msg, (rc, msg)
    assert len(eng.models) == 0 and eng.api.initial_setup(eng.ctx) == _ffi.MPM_ERR_INVALID      # nothing was added: there is no model to set up
    # a velocity field on a model that carries a velocity or an affine array, and on a model that does not exist
    v, Cm = random_motion(n, 3)
    eng.init_model(gm.SAND, xyz, velocity=v, affine=Cm, **gm.material_overrides(gm.SAND))
    for call in (lambda: eng.set_model_velocity_field(0, omega=(0, 0, 1.0)), lambda: eng.set_model_velocity_field(3, omega=(0, 0, 1.0)),
                 lambda: eng.set_model_velocity_field(0, grad=np.full((3, 3), np.nan))):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.code == _ffi.MPM_ERR_INVALID
    # the context then sets up and runs with the valid model, which kept its arrays
    sc = scene_of([model_dict(gm.SAND, pos, velocity=v, affine=Cm)])
    g = pim.setup_nodes(sc)
    eng.initial_setup()
    nodes, val = pim.dumped_nodes(*eng.dump_grid(), gm.BITS)
    assert np.array_equal(nodes, g["nodes"]) and (np.abs(val - g["val"]) <= pim.node_bounds(g)).all()
    eng.run_fixed(2, 1e-5)
    assert eng.retrieve_positions(0).shape[0] == n
    # after set-up both calls are refused
    init, keep = init_with(velocity=good["velocity"])
    rc, _, msg = raw_add(eng, gm.SAND, xyz, init)
    assert rc == _ffi.MPM_ERR_INVALID and "before mpm_initial_setup" in msg
    with pytest.raises(EngineError) as e:
        eng.set_model_velocity_field(0, omega=(0, 0, 1.0))
    assert e.value.code == _ffi.MPM_ERR_INVALID
    eng.close()


def test_oracle_api_refuses_the_arrays_clearly():
    class NoSymbol:                                               # an API without the two symbols, as the oracle's is
        def __getattr__(self, name):
            if name in ("add_model_particles", "set_model_velocity_field"):
                raise AttributeError(name)
            return getattr(_ffi.load_hip(), name)
    eng = build_engine(scene_of([]), api=NoSymbol())
    xyz = np.ascontiguousarray(gm.scene_isolated() * DX)
    with pytest.raises(EngineError, match="HIP library"):
        eng.init_model(gm.FC, xyz, velocity=np.zeros_like(xyz))
    assert eng.init_model(gm.FC, xyz) == 0                        # without arrays: mpm_add_model, as before
    with pytest.raises(EngineError, match="HIP library"):
        eng.set_model_velocity_field(0, omega=(0, 0, 1.0))
    eng.close()


def test_null_init_is_add_model():
    pos = gm.scene_block_sizes()
    xyz = np.ascontiguousarray(pos * DX)
    out = []
    for how in ("add_model", "null init"):
        eng = build_engine(scene_of([]))
        prm = eng.default_material(gm.NACC)
        for k, v in gm.material_overrides(gm.NACC).items():
            setattr(prm, k, v)
        if how == "add_model":
            eng.init_model(gm.NACC, xyz, v0=(0.5, -1.0, 0.25), params=prm)
        else:
            mid = C.c_int(-1)
            assert eng.api.add_model_particles(eng.ctx, gm.NACC, C.byref(prm), xyz.ctypes.data, xyz.shape[0], (C.c_float * 3)(0.5, -1.0, 0.25), None, C.byref(mid)) == 0
            eng.models.append({"material": gm.NACC, "n": xyz.shape[0], "params": prm})
        eng.initial_setup()
        x, s9, lj = eng.retrieve_state(0)
        o = gb.by_position_bits(x)
        out.append((x[o], s9[o], lj[o], cf.particle_state(eng.save_checkpoint(), 0), pim.dumped_nodes(*eng.dump_grid(), gm.BITS)))
        eng.close()
    a, b = out
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2])
    assert_same_particle_state(a[3], b[3])
    g = pim.setup_nodes(scene_of([model_dict(gm.NACC, pos, v0=(0.5, -1.0, 0.25))]))
    for nodes, val in (a[4], b[4]):                               # (float atomics: the order of the adds is free, so the two grids are held to the model)
        assert np.array_equal(nodes, g["nodes"]) and (np.abs(val - g["val"]) <= pim.node_bounds(g)).all()


# ---- 8. a group ------------------------------------------------------------------------------------------------------------------------------
def test_group_ranks_start_from_their_shares_of_the_arrays():
    from claymore_amd.mgsp import LocalGroup, MgspGroupRank, partition_scene
    world = 2
    sc = field_scene("spinning_ball")
    a, A = scenes.model_velocity_field(sc["models"][0])
    per = as_arrays(sc)
    m = per["models"][0]
    parts, index = scenes.split_slabs(m["xyz"], world, axis=0, return_index=True)
    shares = [dict(per, models=[dict(m, xyz=parts[r], velocity=m["velocity"][index[r]], affine=m["affine"][index[r]])]) for r in range(world)]
    for r in range(world):                                        # partition_scene cuts the arrays the same way
        auto = partition_scene(per, r, world, axis=0)["models"][0]
        assert all(np.array_equal(auto[k], shares[r]["models"][0][k]) for k in ("xyz", "velocity", "affine"))
    g = pim.setup_nodes(sc)
    nb = pim.node_bounds(g, extra_momentum=pim.R_FIELD, extra_terms=world)

    def script(sim):
        sim.initial_setup()
        return readout_errors(sim, a, A)

    lg = LocalGroup(world)                                        # two ranks on the one GPU, as test_group_velocity_gpu.run_group builds them
    ranks = [MgspGroupRank(shares[r], r, world, device=0, local_group=lg, prepartitioned=True) for r in range(world)]
    lg.create()
    res, errors = [None] * world, []

    def work(r):
        try:
            res[r] = script(ranks[r])
        except Exception as e:  # noqa: BLE001
            errors.append((r, repr(e)))

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    for r in ranks:
        r.close()
    assert not errors, errors
    assert sum(r[0].shape[0] for r in res) == m["xyz"].shape[0]
    for rank, (x, ev, ec) in enumerate(res):
        bv, bc = pim.linear_field_bounds(g, nb, x, 6, a, A)
        print(f"rank {rank}: {x.shape[0]} particles, v_p error {(ev / bv).max():.3f}, C_p error {(ec / bc).max():.3f} of their bounds")
        assert x.shape[0] == parts[rank].shape[0] and (ev <= bv).all() and (ec <= bc).all()


# ---- the gmpm driver ---------------------------------------------------------------------------------------------------------------------------
def test_gmpm_runs_a_scene_with_omega(tmp_path):
    """A model object with "omega" and "pivot": frame 0 carries the field itself as "v", and after a frame of five substeps without gravity the
    ball still turns as it started (it has turned by 0.01 rad: the readout is within a few per cent of the initial field at the new positions)."""
    import json
    import subprocess
    import __graft_entry__ as g
    from test_particle_velocity_gpu import _read_bgeo_any
    g.build_host()
    omega, c = np.array([0.0, 5.0, 20.0]), np.array([0.5, 0.5, 0.5])
    model = {"file": "sphere", "constitutive": "fixed_corotated", "rho": 1e3, "volume": float(np.float32((1 / 64) ** 3 / 8)), "youngs_modulus": 5e3,
             "poisson_ratio": 0.4, "offset": [0.421875] * 3, "span": [0.15625] * 3, "velocity": [0.25, 0, 0], "omega": omega.tolist(), "pivot": c.tolist()}
    sim = {"gpuid": 0, "fps": 2000, "frames": 1, "default_dt": 1e-4, "domain_bits": 6, "gravity": 0.0, "output_dir": str(tmp_path), "output_velocity": True}
    (tmp_path / "scene.json").write_text(json.dumps({"simulation": sim, "models": [model]}))
    subprocess.check_output([os.path.join(os.path.dirname(HERE), "claymore_amd", "host", "gmpm"), "-f", str(tmp_path / "scene.json")], text=True, timeout=300)
    for f in (0, 1):
        x, v = _read_bgeo_any(tmp_path / f"model_id[0]_frame[{f}].bgeo")
        want = np.array([0.25, 0, 0])[None, :] + np.cross(omega[None, :], x.astype(np.float64) - c[None, :])
        err = np.abs(v - want).max()
        print(f"gmpm frame {f}: {x.shape[0]} particles, |v - field| <= {err:.3g} of {np.abs(want).max():.3g}")
        assert x.shape[0] > 1000 and np.abs(want).max() > 1.0
        assert err <= (4 * U if f == 0 else 0.05) * np.abs(want).max()

"""The NumPy statement of the emission contract (tests/particle_emit_model.py) held against itself and against particle_init_model, and the layer
rule of scenes.Emitter against the model's second statement of it and against the C++ header gmpm uses (claymore_amd/host/emitter_rule.hpp,
through host_selftest --emitter).  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import g2p2g_model as gm  # noqa: E402
import particle_emit_model as pem  # noqa: E402
import particle_init_model as pim  # noqa: E402
from claymore_amd import scenes  # noqa: E402

BITS = 6
DX = np.float32(0.5 ** BITS)


def particles(n, seed, ids_from=None):
    rng = np.random.default_rng(seed)
    p = {"xyz": rng.uniform(0.2, 0.8, (n, 3)).astype(np.float32), "state9": rng.uniform(0.5, 1.5, (n, 9)).astype(np.float32), "logjp": rng.uniform(-0.1, 0.0, n).astype(np.float32)}
    p["ids"] = None if ids_from is None else np.arange(ids_from, ids_from + n, dtype=np.int32)
    return p


# ---- the contract ------------------------------------------------------------------------------------------------------------------------------------
def test_merged_set_ids_and_books():
    old, new = particles(50, 1, ids_from=0), particles(7, 2)
    new["ids"] = pem.new_ids(50, 7)
    m = pem.merged_particles(old, new)
    assert m["xyz"].shape == (57, 3) and np.array_equal(m["ids"], np.arange(57))
    shuffled = {k: v[np.random.default_rng(3).permutation(57)] for k, v in m.items()}
    assert pem.same_set(m, shuffled), "the order is unspecified"
    flipped = {k: v.copy() for k, v in shuffled.items()}
    flipped["state9"].view(np.uint32)[11, 4] ^= 1
    assert not pem.same_set(m, flipped), "one bit of one state entry"
    swapped = {k: v.copy() for k, v in shuffled.items()}
    swapped["ids"][[0, 1]] = swapped["ids"][[1, 0]]
    assert not pem.same_set(m, swapped), "an id that went to another particle"
    books = {"n": [100, 40], "bucketed": [97, 40], "lost": 2, "dropped": 1, "bias": 0}
    after = pem.books_after(books, 1, 9)
    assert pem.books_balance(books) and pem.books_balance(after)
    assert after["n"] == [100, 49] and after["bucketed"] == [97, 49] and (after["lost"], after["dropped"], after["bias"]) == (2, 1, 0)
    assert books["n"] == [100, 40], "the input is not touched"


def test_default_state():
    assert np.array_equal(pem.default_state9(False, 2), np.tile(np.eye(3, dtype=np.float32).ravel(), (2, 1)))
    assert np.array_equal(pem.default_state9(True, 1), np.float32([[1, 0, 0, 0, 0, 0, 0, 0, 0]]))


def node_grid(g, bits):
    """a setup_nodes result as the float32 grid a dump would hold: (flat, val float32)"""
    n = 1 << bits
    flat = (g["nodes"][:, 0] * n + g["nodes"][:, 1]) * n + g["nodes"][:, 2]
    return flat, g["val"].astype(np.float32)


def test_expected_grid_is_old_plus_the_new_particles_setup_p2g():
    """old grid = the set-up grid of the old particles; old + new rasterised alone = the set-up grid of both, within float32's rounding of the old
    values; the reached set holds every node the new particles give mass to and nothing four cells away"""
    rng = np.random.default_rng(4)
    prm = {"volume": scenes._vol(BITS), "rho": 1e3}
    old = gm.scene_cluster() * DX
    new = gm.block_particles((7, 7, 8), 60, rng) * DX
    v, Cm = rng.uniform(-2, 2, (60, 3)).astype(np.float32), rng.uniform(-50, 50, (60, 3, 3)).astype(np.float32)
    g_old = pim.setup_nodes(pem.new_particle_scene(BITS, prm, old, v0=(0.5, 0.0, -1.0)))
    flat0, val0 = node_grid(g_old, BITS)
    sc_new = pem.new_particle_scene(BITS, prm, new, velocity=v, affine=Cm)
    flat, want, bound = pem.expected_grid(flat0, val0, sc_new)
    both = {"bits": BITS, "models": [pem.new_particle_scene(BITS, prm, old, v0=(0.5, 0.0, -1.0))["models"][0], sc_new["models"][0]]}
    g_both = pim.setup_nodes(both)
    fb, vb = node_grid(g_both, BITS)
    at = np.searchsorted(fb, flat)
    assert np.array_equal(fb[at], flat)
    # only the float32 rounding of the old values (at most u of their magnitude) and float64's own additions lie between the two
    assert (np.abs(g_both["val"][at] - want) <= (pim.U + 1e-12) * g_both["mag"][at]).all()
    assert (bound > 0).all() and (bound[:, 0] < 1e-4 * want[:, 0]).all()
    reached = pem.reached_nodes(new, BITS)
    assert np.isin(flat, reached).all()
    n = 1 << BITS
    xyz = np.stack([reached // (n * n), (reached // n) % n, reached % n], axis=1)
    cells = new.astype(np.float64) * n
    assert xyz.min(axis=0).tolist() == (np.round(cells).astype(int).min(axis=0) - 1).tolist() and (xyz.max(axis=0) <= np.round(cells).astype(int).max(axis=0) + 1).all()
    # a node of the old grid that is not reached keeps its bits: expected_grid does not list it
    assert (~np.isin(flat0, flat)).any()


def test_reached_nodes_at_the_faces_stay_inside_the_domain():
    n = 1 << BITS
    pts = np.float32([[-0.4, 5.2, 5.2], [n + 0.4, 5.2, 5.2], [5.2, 0.1, n - 0.2]]) * DX
    r = pem.reached_nodes(pts, BITS)
    assert r.min() >= 0 and r.max() < n ** 3
    lone = pem.reached_nodes(np.float32([[20.3, 30.7, 40.1]]) * DX, BITS)
    assert lone.size == 27


def test_grid_by_node_reads_a_dump():
    keys = np.int32([[1, 2, 3], [15, 15, 15]])
    blocks = np.arange(2 * 4 * 64, dtype=np.float32).reshape(2, 4, 64)
    flat, val = pem.grid_by_node(keys, blocks, BITS)
    n = 1 << BITS
    cell = (2 << 4) | (1 << 2) | 3                                 # node (4 + 2, 8 + 1, 12 + 3) of block (1, 2, 3)
    at = np.searchsorted(flat, ((4 + 2) * n + 8 + 1) * n + 12 + 3)
    assert flat.size == 128 and np.array_equal(val[at], blocks[0, :, cell])


# ---- the emitter's layer rule ----------------------------------------------------------------------------------------------------------------------
NOZZLES = {
    "disc pouring down": dict(shape="disc", velocity=(0.0, -2.0, 0.0), start=0.001, end=0.02, center=(0.5, 0.8, 0.5), radius=3.3 / 64),
    "box along +x": dict(shape="box", velocity=(1.5, 0.0, 0.0), start=0.0, end=0.03, lo=(0.2, 0.3, 0.4), hi=(0.26, 0.41, 0.47)),
    "disc at the lower x face": dict(shape="disc", velocity=(0.7, 0.0, 0.0), start=0.0, end=0.05, center=(0.0, 0.5, 0.5), radius=2.0 / 64, normal=(1.0, 0.0, 0.0)),
    "box at the upper z face, reaching past the edge": dict(shape="box", velocity=(0.0, 0.0, -1.0), start=0.002, end=0.04, lo=(0.9, 0.45, 1.0), hi=(1.1, 0.55, 1.0)),
}


def step_sequences(end):
    rng = np.random.default_rng(21)
    out = {"even": np.arange(0, end * 1.3, 1e-4), "coarse": np.arange(0, end * 1.3, 3.7e-3), "one step past the end": np.array([0.0, end * 2])}
    out["random"] = np.concatenate([[0.0], np.cumsum(rng.uniform(2e-5, 6e-3, 200))])
    out["random"] = out["random"][out["random"] < end * 1.5]
    return out


@pytest.mark.parametrize("name", sorted(NOZZLES))
def test_emitter_hands_out_every_layer_once_on_the_same_lattice_whatever_the_steps(name):
    geom = dict(NOZZLES[name])
    v = np.asarray(geom["velocity"], np.float64)
    axis = int(np.argmax(np.abs(v)))
    lattice = pem.nozzle_lattice(BITS, geom["shape"], axis, **{k: geom[k] for k in ("lo", "hi", "center", "radius") if k in geom})
    tk = pem.layer_times(BITS, float(np.abs(v[axis])), geom["start"], geom["end"])
    assert lattice.shape[0] > 0 and tk.size > 3
    assert (lattice >= 0).all() and (lattice <= 1).all(), "a nozzle at a face emits inside the domain"
    assert np.array_equal(np.unique(np.round(lattice * (4 << BITS)).astype(int) % 2), [1]), "the reference's lattice: odd multiples of dx / 4"
    if name.startswith("box at the upper z"):
        assert lattice[:, 0].max() < 1.0 and lattice[:, 2].max() == 1.0 - 0.25 / 64
    for seq, times in step_sequences(geom["end"]).items():
        em = scenes.Emitter(BITS, **geom)
        assert np.array_equal(np.sort(em.layer, axis=0), np.sort(lattice, axis=0))
        want = pem.expected_emissions(BITS, geom["shape"], geom["velocity"], geom["start"], geom["end"], times, **{k: geom[k] for k in ("lo", "hi", "center", "radius") if k in geom})
        layers_seen = []
        for t, now in zip(times, want):
            got = em.due(t)
            exp = np.concatenate([p for _, p in now]) if now else np.zeros((0, 3))
            assert got.dtype == np.float32 and got.shape == exp.shape, (name, seq, t)
            assert np.array_equal(got, exp.astype(np.float32)), (name, seq, t)
            layers_seen += [k for k, _ in now]
            # moved back to its due time every point is the lattice again (to the float32 rounding of the emitted position)
            for k, p in now:
                back = p.astype(np.float32).astype(np.float64) - v[None, :] * (t - tk[k])
                assert np.abs(back - lattice).max() <= 2.0 ** -24 * 1.0 + 1e-15
        due_by_end = int((tk <= times[-1]).sum())
        assert layers_seen == list(range(due_by_end)), (name, seq, "a layer was missed or handed out twice")
        assert em.due(times[-1]).shape[0] == 0, "nothing twice"
        if times[-1] >= geom["end"]:
            assert due_by_end == tk.size and em.due(1e9).shape[0] == 0, "nothing after the end"


def test_emitter_density_is_the_lattices_along_the_flow():
    """consecutive layers, emitted at one boundary, lie dx / 2 apart along the flow: 8 particles per cell"""
    em = scenes.Emitter(BITS, "disc", (0.0, -2.0, 0.0), start=0.0, end=1.0, center=(0.5, 0.8, 0.5), radius=2.0 / 64)
    m = em.layer.shape[0]
    pts = em.due(10.5 * em.period).astype(np.float64)
    assert pts.shape[0] == 11 * m
    ys = np.sort(np.unique(pts[:, 1]))
    assert ys.size == 11 and np.abs(np.diff(ys) - 0.5 / 64).max() <= 2.0 ** -23


def test_emitter_refuses_what_it_does_not_serve():
    for bad in (dict(shape="disc", velocity=(1.0, 1.0, 0.0), center=(0.5, 0.5, 0.5), radius=0.1), dict(shape="disc", velocity=(0.0, 0.0, 0.0), center=(0.5, 0.5, 0.5), radius=0.1),
                dict(shape="disc", velocity=(1.0, 0.0, 0.0), center=(0.5, 0.5, 0.5), radius=0.1, normal=(0.0, 1.0, 0.0)), dict(shape="cone", velocity=(1.0, 0.0, 0.0)),
                dict(shape="box", velocity=(1.0, 0.0, 0.0), lo=(0.1, 0.1, 0.1))):
        with pytest.raises(ValueError):
            scenes.Emitter(BITS, **bad)


def test_scenes_with_emitters():
    for sc in (scenes.faucet(bits=BITS), scenes.sand_pour(bits=BITS)):
        assert sc["models"][0]["xyz"].shape == (0, 3) and len(sc["emitters"]) == 1
        em = scenes.Emitter.from_dict(sc["bits"], sc["emitters"][0])
        first = em.due(0.0)
        assert first.shape[0] > 8 and em.model == 0 and (first > 8.0 / 64).all() and (first < 1 - 8.0 / 64).all(), "the nozzle is clear of the wall zone"
    hf = scenes.sand_pour(bits=BITS)["colliders"][0]
    n = 1 << BITS
    assert hf["kind"] == "heightfield" and first[:, 1].min() > hf["heights"][n // 2 - 4:n // 2 + 5, n // 2 - 4:n // 2 + 5].max() + 4.0 / n, "the nozzle is above the ground under it"


# ---- the C++ header of the same rule ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emitter") / "host_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "claymore_amd", "host", "host_selftest.cpp")])
    return exe


@pytest.mark.parametrize("name", sorted(NOZZLES))
def test_the_c_header_states_the_same_rule(selftest, name):
    geom = dict(NOZZLES[name])
    times = step_sequences(geom["end"])["random"]
    entry = dict({k: (list(v) if isinstance(v, tuple) else v) for k, v in geom.items()}, model=0)
    out = subprocess.check_output([selftest, "--emitter", json.dumps(entry), str(BITS)] + [float(t).hex() for t in times], text=True).split("\n")
    em = scenes.Emitter(BITS, **geom)
    line = 0
    for t in times:
        want = em.due(t)
        assert out[line] == f"due {want.shape[0]}", (name, t, out[line])
        got = np.array([[int(w, 16) for w in out[line + 1 + i].split()] for i in range(want.shape[0])], dtype=np.uint32).reshape(-1, 3)
        line += 1 + want.shape[0]
        a, b = np.sort(got.view([("", np.uint32)] * 3).ravel()), np.sort(np.ascontiguousarray(want).view(np.uint32).view([("", np.uint32)] * 3).ravel())
        assert np.array_equal(a, b), (name, t)
    assert em.next_layer > 3


def test_the_c_header_refuses_a_malformed_entry(selftest):
    r = subprocess.run([selftest, "--emitter", json.dumps({"shape": "disc", "velocity": [1.0, 1.0, 0.0], "center": [0.5, 0.5, 0.5], "radius": 0.1}), str(BITS), "0.0"], capture_output=True, text=True)
    assert r.returncode == 1 and "principal axis" in r.stderr

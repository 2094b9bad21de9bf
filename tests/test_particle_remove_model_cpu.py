"""The NumPy statement of mpm_remove_particles' contract (tests/particle_remove_model.py) on hand-made grids, the sweep rule of scenes.Sink
against its definition and against the C++ header of the same rule (claymore_amd/host/sink_rule.hpp, through host_selftest --sink), and the
scenes that carry sinks.  No GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

import particle_emit_model as pem
import particle_init_model as pim
import particle_remove_model as prm
from claymore_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = 6
N = 1 << BITS
DX = 1.0 / N
PARAMS = {"volume": scenes._vol(BITS), "rho": 1e3}


def cells(p):
    return (np.array(p, np.float64) * DX).astype(np.float32)


def old_grid_of(xyz, v=(1.0, -2.0, 0.5)):
    """the set-up grid of the particles xyz with one velocity, as float32, over a box of nodes around them (zeros where nobody reaches)"""
    g = pim.setup_nodes({"bits": BITS, "models": [{"xyz": xyz, "v0": v, "params": PARAMS}]})
    lo, hi = g["nodes"].min(axis=0) - 2, g["nodes"].max(axis=0) + 3
    nd = np.stack(np.meshgrid(*[np.arange(lo[d], hi[d]) for d in range(3)], indexing="ij"), axis=-1).reshape(-1, 3)
    flat = (nd[:, 0] * N + nd[:, 1]) * N + nd[:, 2]
    val = np.zeros((flat.size, 4), np.float32)
    val[np.searchsorted(flat, (g["nodes"][:, 0] * N + g["nodes"][:, 1]) * N + g["nodes"][:, 2])] = g["val"].astype(np.float32)
    return flat, val


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_node_reached_only_by_removed_particles_is_exactly_zero_and_an_unreached_node_is_unchanged():
    far, near, gone = cells([20.2, 20.4, 20.6]), cells([30.3, 30.1, 30.7]), cells([31.8, 30.4, 30.6])        # near and gone share nodes, far shares none
    flat, val = old_grid_of(np.stack([far, near, gone]))
    reached, exact, want, bound = prm.expected_grid(flat, val, gone[None], prm.survivor_scene(BITS, [(PARAMS, np.stack([far, near]))]))
    r_gone, r_near, r_far = (np.isin(flat, pem.reached_nodes(p[None], BITS)) for p in (gone, near, far))
    assert np.array_equal(reached, r_gone) and (r_gone & r_near).any() and not (r_gone & r_far).any()
    only = r_gone & ~r_near & (val[:, 0] > 0)
    assert only.any() and exact[only].all() and (want[only] == 0).all() and not np.signbit(want[only]).any()
    assert exact[~reached].all() and np.array_equal(want[~reached], val[~reached].astype(np.float64)) and (bound[~reached] == 0).all()
    both = r_gone & r_near & (val[:, 0] > 0)
    m1 = pim.setup_nodes(prm.survivor_scene(BITS, [(PARAMS, near[None])]))
    assert not exact[both].any() and both.sum() == np.isin((m1["nodes"][:, 0] * N + m1["nodes"][:, 1]) * N + m1["nodes"][:, 2], flat[r_gone]).sum()
    # the rescale keeps the node velocity: p' / m' == p / m
    v_old, v_new = val[both, 1:].astype(np.float64) / val[both, :1], want[both, 1:] / want[both, :1]
    assert np.abs(v_old - v_new).max() <= 1e-12 and (want[both, 0] < val[both, 0]).all()
    assert (bound[both, 0] > 0).all() and (bound[both, 0] <= pim.gamma(27 + pim.R_MASS) * want[both, 0] + 27 * 2.0 ** -126).all()


def test_a_reached_node_without_old_mass_keeps_its_bits():
    a, b = cells([30.3, 30.1, 30.7]), cells([31.2, 30.4, 30.6])
    flat, val = old_grid_of(np.stack([a, b]))
    hit = np.flatnonzero(np.isin(flat, pem.reached_nodes(b[None], BITS)) & (val[:, 0] > 0))
    val[hit[0]] = (0.0, 3.0, -1.0, 2.0)                                     # m_old == 0 with momenta: kept
    val[hit[1]] = (-1e-3, 3.0, -1.0, 2.0)                                   # m_old < 0: kept
    val[hit[2], 0] = np.nan                                                 # !(NaN > 0): kept
    reached, exact, want, _ = prm.expected_grid(flat, val, b[None], prm.survivor_scene(BITS, [(PARAMS, a[None])]))
    assert reached[hit[:3]].all() and exact[hit[:3]].all()
    assert np.array_equal(want[hit[:3]].astype(np.float32).view(np.uint32), val[hit[:3]].view(np.uint32))


def test_check_grid_accepts_the_model_and_rejects_a_wrong_grid():
    a, b = cells([30.3, 30.1, 30.7]), cells([32.2, 30.4, 30.6])
    flat, val = old_grid_of(np.stack([a, b]))
    sc = prm.survivor_scene(BITS, [(PARAMS, a[None])])
    _, _, want, _ = prm.expected_grid(flat, val, b[None], sc)
    new = want.astype(np.float32)
    prm.check_grid(flat, val, flat, new, b[None], sc)
    # a dropped block: the nodes that hold exact zeros may be missing from the new grid, no other may
    zero = (new == 0).all(axis=1)
    prm.check_grid(flat, val, flat[~zero], new[~zero], b[None], sc)
    with pytest.raises(AssertionError):
        prm.check_grid(flat, val, flat[zero], new[zero], b[None], sc)
    for at, ch, factor in ((np.flatnonzero(~zero & ~np.isin(flat, pem.reached_nodes(b[None], BITS)))[0], 1, 1 + 2.0 ** -23), (np.flatnonzero(new[:, 0] != val[:, 0])[0], 0, 1.001)):
        bad = new.copy()
        bad[at, ch] *= np.float32(factor)
        with pytest.raises(AssertionError):
            prm.check_grid(flat, val, flat, bad, b[None], sc)


def test_the_predicate_the_split_and_the_books():
    rng = np.random.default_rng(3)
    x = rng.uniform(0.3, 0.7, (500, 3)).astype(np.float32)
    ids = rng.permutation(500).astype(np.int32)
    sph = {"kind": "sphere", "center": (0.5, 0.5, 0.5), "radius": 0.1}
    inside = prm.selected(x, [sph])
    d = np.linalg.norm(x.astype(np.float64) - 0.5, axis=1)
    assert np.array_equal(inside[np.abs(d - 0.1) > 1e-6], (d <= 0.1)[np.abs(d - 0.1) > 1e-6]) and 0 < inside.sum() < 500
    assert np.array_equal(prm.selected(x, [dict(sph, inside_out=True)]), ~inside | (prm.selected(x, [sph]) & (d == 0.1)))
    assert not prm.selected(x, [{"kind": "box", "center": (np.nan, 0.5, 0.5), "half_extents": (1.0, 1.0, 1.0)}]).any(), "a NaN sdis selects nothing"
    listed = prm.selected(x, [sph], ids, [3, 3, 499, 1000])
    assert listed.sum() == inside.sum() + (~inside[np.isin(ids, [3, 499])]).sum()
    half = {"kind": "halfspace", "point": (0.5, 0.5, 0.5), "normal": (0.0, 4.0, 0.0)}                      # normalised like a collider's
    assert np.array_equal(prm.selected(x, [half]), x[:, 1] <= np.float32(0.5))
    p = {"xyz": x, "state9": np.zeros((500, 9), np.float32), "logjp": np.zeros(500, np.float32), "ids": ids}
    keep, gone = prm.split(p, inside)
    assert keep["xyz"].shape[0] + gone["xyz"].shape[0] == 500 and pem.same_set(pem.merged_particles(keep, gone), p)
    books = {"n": [500, 20], "bucketed": [490, 20], "lost": 7, "dropped": 3, "bias": 0}
    assert pem.books_balance(books)
    after = prm.books_after(books, [int(inside.sum()), 5])
    assert pem.books_balance(after) and after["n"] == [500, 20] and after["bucketed"] == [490 - int(inside.sum()), 15] and (after["lost"], after["dropped"]) == (7, 3)


# ---- the sink's sweep rule --------------------------------------------------------------------------------------------------------------------------------
SINKS = {
    "from the start": dict(start=0.0, end=0.04, period=1e-3),
    "late, coarse": dict(start=0.0123, end=0.05, period=7.3e-3),
    "no end": dict(start=0.001, end=np.inf, period=2.5e-4),
}
REGION = {"kind": "box", "center": (0.5, 0.1, 0.5), "half_extents": (0.5, 0.1, 0.5)}


def step_sequences(end):
    rng = np.random.default_rng(21)
    end = min(end, 0.06)
    out = {"even": np.arange(0, end * 1.3, 1e-4), "coarse": np.arange(0, end * 1.3, 3.7e-3), "one step past the end": np.array([0.0, end * 2])}
    out["random"] = np.concatenate([[0.0], np.cumsum(rng.uniform(2e-5, 6e-3, 200))])
    out["random"] = out["random"][out["random"] < end * 1.5]
    return out


@pytest.mark.parametrize("name", sorted(SINKS))
def test_sink_serves_every_sweep_once_whatever_the_steps(name):
    rule = SINKS[name]
    tk = prm.sweep_times(rule["start"], min(rule["end"], 0.2), rule["period"])
    assert tk.size > 3
    for seq, times in step_sequences(rule["end"]).items():
        sk = scenes.Sink(BITS, REGION, model=0, **rule)
        want = prm.expected_sweeps(rule["start"], rule["end"], rule["period"], times) if np.isfinite(rule["end"]) else prm.expected_sweeps(rule["start"], times[-1] + 1.0, rule["period"], times)
        seen = []
        for t, now in zip(times, want):
            assert sk.due(t) == len(now), (name, seq, t)
            seen += now
        assert seen == list(range(int((tk <= times[-1]).sum()))), (name, seq, "a sweep was missed or served twice")
        assert sk.due(times[-1]) == 0, "nothing twice"
        if times[-1] >= rule["end"]:
            assert len(seen) == tk.size and sk.due(1e9) == 0, "nothing after the end"


def test_sink_refuses_what_it_does_not_serve():
    for bad in (dict(), dict(period=0.0), dict(period=-1.0), dict(period=np.inf), dict(period=np.nan)):
        with pytest.raises(ValueError):
            scenes.Sink(BITS, REGION, **bad)
    with pytest.raises(ValueError):
        scenes.Sink(BITS, {"center": (0.5, 0.5, 0.5)}, period=1e-3)
    sk = scenes.Sink.from_dict(BITS, dict(REGION, model=2, start=0.5, end=0.75, period=0.125))
    assert (sk.model, sk.start, sk.end, sk.period, sk.region) == (2, 0.5, 0.75, 0.125, REGION)
    assert scenes.Sink.from_dict(BITS, dict(REGION, period=1.0)).model == -1


def test_scenes_with_sinks():
    sc = scenes.fountain(bits=BITS)
    assert sc["models"][0]["xyz"].shape == (0, 3) and len(sc["emitters"]) == 1 and len(sc["sinks"]) == 1
    sk, em = scenes.Sink.from_dict(BITS, sc["sinks"][0]), scenes.Emitter.from_dict(BITS, sc["emitters"][0])
    assert sk.period == em.period and sk.model == 0
    nozzle = em.due(0.0)
    assert not prm.selected(nozzle, [sk.region]).any(), "the nozzle is above the drain"
    floor = nozzle.copy()
    for cell in (3.0, 9.0, 11.5):                                           # inside the wall zone, and above it where the jet arrives
        floor[:, 1] = cell * DX
        assert prm.selected(floor, [sk.region]).all(), "what reaches the floor under the nozzle is drained"
    sc = scenes.drain(bits=BITS)
    sk = scenes.Sink.from_dict(BITS, sc["sinks"][0])
    x = sc["models"][0]["xyz"]
    assert x.shape[0] > 1000 and not prm.selected(x, [sk.region]).any(), "the block starts above the slab"
    assert prm.selected(x - np.float32([0, 8 * DX, 0]), [sk.region]).any() and sk.region["kind"] == "halfspace"


# ---- the C++ header of the same rule ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sink") / "host_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "claymore_amd", "host", "host_selftest.cpp")])
    return exe


@pytest.mark.parametrize("name", sorted(SINKS))
def test_the_c_header_states_the_same_rule(selftest, name):
    rule = SINKS[name]
    times = step_sequences(rule["end"])["random"]
    entry = dict({k: v for k, v in rule.items() if np.isfinite(v)}, shape="box", center=[0.5, 0.1, 0.5], half_extents=[0.5, 0.1, 0.5], model=1)
    out = subprocess.check_output([selftest, "--sink", json.dumps(entry)] + [float(t).hex() for t in times], text=True).split("\n")
    sk = scenes.Sink(BITS, REGION, model=1, **rule)
    assert out[0] == "model 1"
    for line, t in zip(out[1:], times):
        assert line == f"due {sk.due(t)}", (name, t, line)
    assert sk.next_sweep > 3


def test_the_c_header_refuses_a_malformed_entry(selftest):
    for entry in ({"shape": "box"}, {"period": 0.0}, {"period": -2.0}):
        r = subprocess.run([selftest, "--sink", json.dumps(entry), "0.0"], capture_output=True, text=True)
        assert r.returncode == 1 and "period" in r.stderr

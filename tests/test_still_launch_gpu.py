"""Launch sizes that follow the still streak (claymore_hip.hip: still_launch_rule; MPM_STILL_LAUNCH=auto|full|thin:N, read when a context is created) on
the GPU: the rebuild's prepare launch and its two registration launches compute the same at every size, on the still path - where a thin launch is all
they need - and on the full path a thin window runs into when somebody moves.

The setting is read by mpm_create, so every run sets it in this process's environment around the creation of its context."""
import os

import numpy as np
import pytest

from claymore_amd import _ffi, scenes
from claymore_amd.engine import build_engine
from test_still_rebuild_gpu import BITS, DT, RUN_TOL, block_census, book_findings, falling_box, rel_dev, still_count, triple

pytestmark = pytest.mark.gpu


def engine_with(setting, sc):
    old = os.environ.get("MPM_STILL_LAUNCH")
    os.environ["MPM_STILL_LAUNCH"] = setting
    try:
        eng = build_engine(sc)
    finally:
        if old is None:
            del os.environ["MPM_STILL_LAUNCH"]
        else:
            os.environ["MPM_STILL_LAUNCH"] = old
    eng.initial_setup()
    return eng


def resting_block():
    """24^3 cells of undeformed fixed-corotated material without gravity or velocity (110 592 particles): nothing ever moves, every rebuild but the first is
    still.  Its lattice spans six blocks per axis: 216 particle blocks, so a prepare launch of ONE workgroup walks its skip loop four times, one of three twice."""
    lo = np.array([18, 18, 18])
    prm = {"volume": float(np.float32((1.0 / 64) ** 3 / 8)), "youngs_modulus": 5e3, "poisson_ratio": 0.4, "rho": 1e3}
    return {"name": "resting_block", "bits": BITS, "dt": DT, "config": {"gravity": 0.0, "sync_interval": 4},
            "models": [{"material": _ffi.FIXED_COROTATED, "xyz": scenes.lattice_box(BITS, lo, lo + 24), "v0": (0.0, 0.0, 0.0), "params": prm}]}


def finish(eng):
    cnt = eng.counts()
    d = eng.diagnostics()
    out = {"still": still_count(eng), "blocks": triple(cnt), "particles": int(cnt.particles[0]), "lost": int(d.lost_particles), "dropped": int(d.dropped_particles),
           "discarded": int(d.discarded_p2g), "findings": book_findings(eng), "x": eng.retrieve_positions(0)}
    eng.close()
    return out


def test_a_streak_at_every_launch_size():
    """20 substeps at rest in windows of four: from the second window on `auto` launches thin; thin:1 and thin:3 do from the first rebuild on, the first one
    (never offered the still path: a full rebuild through one and three workgroups) and the streak's first (every row written, block by block) included."""
    sc = resting_block()
    x0 = np.sort(sc["models"][0]["xyz"], axis=0)
    runs = {}
    for setting in ("thin:1", "thin:3", "full", "auto"):
        eng = engine_with(setting, sc)
        assert eng.counts().particle_blocks >= 65
        eng.run_fixed(20, DT)
        runs[setting] = finish(eng)
    ref = runs["full"]
    assert ref["still"] == 19 and ref["particles"] == 110592 and ref["blocks"][0] == len(block_census(sc["models"][0]["xyz"])) == 216
    for setting, r in runs.items():
        assert (r["still"], r["blocks"], r["particles"]) == (ref["still"], ref["blocks"], ref["particles"]), setting
        assert r["lost"] == r["dropped"] == r["discarded"] == 0, setting
        assert not r["findings"], (setting, r["findings"][:5])
        assert np.array_equal(np.sort(r["x"], axis=0), x0), setting                       # nobody has moved, under any launch


@pytest.fixture(scope="module")
def fall_full():
    eng = engine_with("full", falling_box(sync_interval=8))
    eng.run_fixed(100, DT)
    return finish(eng)


@pytest.mark.parametrize("setting", ["auto", "thin:2"])
def test_a_thin_window_that_meets_movers(fall_full, setting):
    """test_still_rebuild_gpu's falling box (32 768 particles of sand in free fall) in windows of eight: some seventy still substeps, then particles cross block
    faces in a burst of a few substeps inside one window - launched thin, since the read-back before it saw a long streak - whose rebuilds take the full path
    grid-stride: the registrations claim every particle block's neighbourhood through the few workgroups they were given, prepare sorts every block's list.  Books verified
    (tests/rebuild_books.py), nobody lost, counts and still rebuilds those of full launches, and the state equal to theirs particle by particle to the bound
    two runs of the engine are held to (RUN_TOL: the order of the P2G atomics is not fixed)."""
    eng = engine_with(setting, falling_box(sync_interval=8))
    eng.run_fixed(100, DT)
    r = finish(eng)
    print(setting, "still_rebuilds", r["still"], "blocks", r["blocks"])
    assert 80 <= fall_full["still"] < 99, fall_full["still"]                              # a streak, and full rebuilds: the scene tests what it is meant to
    assert (r["still"], r["blocks"], r["particles"]) == (fall_full["still"], fall_full["blocks"], 32768)
    assert r["lost"] == r["dropped"] == r["discarded"] == 0
    assert not r["findings"] and not fall_full["findings"], r["findings"][:5]
    assert rel_dev(r["x"], fall_full["x"]) < RUN_TOL

"""The gmpm driver's frames with simulation.output_stress (claymore_amd/host/gmpm.cpp): the point attributes "stress", "J", "pressure" and
"vonmises" of mpm_retrieve_stress beside "v" of mpm_retrieve_velocity, aligned on the host by the position bits; without the key the frames
are the ones the driver wrote before."""
import json
import os
import subprocess

import numpy as np
import pytest

from claymore_amd import _ffi
from claymore_amd.engine import Engine
from test_particle_stress_cpu import read_bgeo_attrs
from test_particle_stress_gpu import join

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS, FPS, FRAMES, DT_DEFAULT = 6, 500, 2, 1e-4
FC = {"rho": 1e3, "volume": float(np.float32((1 / 64) ** 3 / 8)), "youngs_modulus": 5e3, "poisson_ratio": 0.4}
# Two 2 x 2 x 2-cell boxes (64 particles each) thrown at the x = 0 wall zone, whose edge (cell 8) they straddle.  Each stays inside ONE
# particle block and so inside one wave: a grid node receives its contributions in a fixed order and the engine is deterministic, which a
# comparison of two processes' frames bit for bit needs (a dense body differs in the last bits from run to run: float atomics in P2G,
# tests/test_collision_clock_gpu.py).  x cells [7.5, 9.5): nearest nodes 8 and 9, block 1; y / z cells [18.5, 20.5) and [30.5, 32.5).
MODELS = [dict(FC, file="box", constitutive="fixed_corotated", offset=[7.5 / 64, 18.5 / 64, 18.5 / 64], span=[2 / 64] * 3, velocity=[-0.5, 0, 0]),
          {"file": "box", "constitutive": "sand", "offset": [7.5 / 64, 30.5 / 64, 30.5 / 64], "span": [2 / 64] * 3, "velocity": [-0.5, 0, 0]}]


# nPointAttrib 1 and the rest of the header, then the definition of "v": what the frames with output_velocity alone have always started with
V_HEADER = b"\x00\x00\x00\x01" + b"\x00" * 12 + b"\x00\x01v\x00\x03\x00\x00\x00\x05" + b"\x00" * 12


def run_gmpm(d, **keys):
    d.mkdir()
    sim = dict({"gpuid": 0, "fps": FPS, "frames": FRAMES, "default_dt": DT_DEFAULT, "domain_bits": BITS, "output_dir": str(d)}, **keys)
    fn = d / "scene.json"
    fn.write_text(json.dumps({"simulation": sim, "models": MODELS}))
    subprocess.check_output([os.path.join(ROOT, "claymore_amd", "host", "gmpm"), "-f", str(fn)], text=True, timeout=300)
    return d


def frame(d, model, f):
    return d / f"model_id[{model}]_frame[{f}].bgeo"


def engine_frames(start):
    """gmpm's main loop (float32 clock, adaptive dt from the largest initial speed) on an Engine with the particles of the driver's frame 0,
    in its order: per frame and model the two direct readouts."""
    eng = Engine(domain_bits=BITS, max_ppc=128)
    for mod, xyz in zip(MODELS, start):
        mat = _ffi.MATERIAL_NAMES[mod["constitutive"]]
        eng.init_model(mat, xyz, mod["velocity"], **({k: FC[k] for k in FC} if mat == _ffi.FIXED_COROTATED else {}))
    spf = np.float32(1.0) / np.float32(FPS)
    max_v0 = max(float(np.sqrt(np.float32(np.sum(np.float32(mod["velocity"]) ** 2)))) for mod in MODELS)
    dt = eng.compute_dt(max_v0, 0.0, float(spf), DT_DEFAULT)
    eng.initial_setup()
    out = []
    for _ in range(FRAMES):
        t = np.float32(0.0)
        while t < spf:
            next_dt, _ = eng.substep(dt, float(t), float(spf), DT_DEFAULT)
            t = np.float32(t + np.float32(dt))
            dt = next_dt
        out.append([(eng.retrieve_velocity(m), eng.retrieve_stress(m)) for m in range(len(MODELS))])
    eng.close()
    return out


def test_gmpm_output_stress_beside_output_velocity(tmp_path):
    import __graft_entry__ as g
    g.build_host()
    plain = run_gmpm(tmp_path / "plain")
    vel = run_gmpm(tmp_path / "v", output_velocity=True)
    both = run_gmpm(tmp_path / "both", output_velocity=True, output_stress=True)
    only = run_gmpm(tmp_path / "stress", output_stress=True)
    start = []
    for m, mod in enumerate(MODELS):
        raw = open(frame(plain, m, 0), "rb").read()
        x0, attrs = read_bgeo_attrs(frame(plain, m, 0))
        assert x0.shape == (64, 3)
        assert attrs == {} and len(raw) == 41 + 16 * x0.shape[0] + 2                        # without the keys: the position-only frame
        assert open(frame(vel, m, 0), "rb").read()[:62] == raw[:25] + V_HEADER                # (one attribute: "v" alone, as before)
        start.append(x0)
        xb, ab = read_bgeo_attrs(frame(both, m, 0))
        assert list(ab) == ["v", "stress", "J", "pressure", "vonmises"] and np.array_equal(xb, x0)
        assert np.array_equal(ab["v"], np.tile(np.float32(mod["velocity"]), (x0.shape[0], 1)))
        assert not ab["stress"].any() and not ab["pressure"].any() and not ab["vonmises"].any() and np.all(ab["J"] == 1.0)
        assert list(read_bgeo_attrs(frame(only, m, 0))[1]) == ["stress", "J", "pressure", "vonmises"]
    want = engine_frames(start)
    loaded = 0
    for f in range(1, FRAMES + 1):
        for m in range(len(MODELS)):
            (xv, v), (xs, s6, sc) = want[f - 1][m]
            for d in (both, only):
                x, a = read_bgeo_attrs(frame(d, m, f))
                assert [a[k].shape[1] for k in ("stress", "J", "pressure", "vonmises")] == [6, 1, 1, 1]
                idx = join(x, xs)                                                          # the frame's rows among the direct stress readout's
                got = np.concatenate([a["stress"], a["J"], a["pressure"], a["vonmises"]], axis=1)
                assert np.array_equal(got.view(np.uint32), np.concatenate([s6, sc], axis=1)[idx].view(np.uint32))
                if d is both:
                    assert np.array_equal(a["v"].view(np.uint32), v[join(x, xv)].view(np.uint32))
            loaded += int(np.sum(sc[:, 2] > 0))
            # without output_stress the frames are what they were: the same bytes as a run of the driver that knows no such key writes
            xp, ap = read_bgeo_attrs(frame(plain, m, f))
            xq, aq = read_bgeo_attrs(frame(vel, m, f))
            assert ap == {} and list(aq) == ["v"] and xp.shape == xq.shape == xs.shape
            n = xs.shape[0]
            rp, rq = open(frame(plain, m, f), "rb").read(), open(frame(vel, m, f), "rb").read()
            assert len(rp) == 41 + 16 * n + 2 and len(rq) == 62 + 28 * n + 2 and rq[:62] == rp[:25] + V_HEADER
            join(xp, xs), join(xq, xs)                                                     # (assert the same position bits)
    assert loaded > 64                                                                     # the wall has deformed the boxes: the stress is not zero

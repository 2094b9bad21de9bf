#!/usr/bin/env python
"""What a removal costs (mpm_remove_particles) - the driver behind profiles/particle_remove.txt.
  fountain  scenes.fountain at test size (64^3, max_ppc 16) after 100 served substeps: one sweep of its sink box, then a sweep that selects nothing
  c3        C3 (sand_column(9), 40 108 032 particles) after bench.py's default warm-up (10 substeps of 1e-4): a call that selects nothing, then the
            particles in a 32 x 4 x 32-cell box under the column's highest particle (36 864 of them when profiles/particle_remove.txt was taken)
Each against the yardstick of the same process: mpm_initial_setup of the surviving particle set (its positions read back) in a second context.
Wall times are host-side, around calls that synchronise; the per-kernel times come from the profiler.
Usage (one MI355X): rocprofv3 --kernel-trace --stats -f csv -d OUT -o remove -- python tools/particle_remove_cost.py fountain|c3"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from claymore_amd import scenes
from claymore_amd.engine import build_engine

case = sys.argv[1] if len(sys.argv) > 1 else "fountain"
far = {"kind": "sphere", "center": (0.05, 0.95, 0.05), "radius": 0.01}
if case == "fountain":
    sc = scenes.fountain(bits=6, radius_cells=3.0, speed=8.0, height_cells=16, end=1.0)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.serve_emitters(0.0)
    for _ in range(100):
        eng.substep(1e-4, 0.0, 1.0, 1e-4)
        eng.cur_time += 1e-4
        eng.serve_emitters()                                       # (the sink is not served: what has arrived waits for the measured sweep)
    region = eng.sinks[0].region
else:
    sc = scenes.sand_column(9)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(10, sc["dt"])
    x = eng.retrieve_positions(0)
    top = float(x[:, 1].max())
    dx = 1.0 / 512
    region = {"kind": "box", "center": (0.5, top - 2 * dx, 0.5), "half_extents": (16 * dx, 2 * dx + dx / 8, 16 * dx)}
    del x
print("build_info", eng.api.build_info().decode())
for what, reg in (("nothing selected", far), ("sweep", region), ("nothing selected, again", far)):
    held = int(eng.counts().particles[0])
    t0 = time.perf_counter()
    res = eng.remove(regions=[reg], model=0)
    t1 = time.perf_counter()
    c = eng.counts()
    print(f"{case} {what}: {res['removed'][0]} of {held} particles removed, relaid {res['relaid']}: wall {1e3 * (t1 - t0):.3f} ms; blocks {c.particle_blocks}/{c.neighbor_blocks}/{c.exterior_blocks}, "
          f"mass out {res['mass']:.6g}, transient staging {52 * int(c.particles[0]) / 1e6:.1f} MB at 52 B a surviving particle (untracked) + {c.neighbor_blocks * 2 / 1024:.1f} MiB of grids")
left = eng.retrieve_positions(0)
eng.close()
ref = build_engine(dict(sc, models=[dict(sc["models"][0], xyz=left)], emitters=[], sinks=[]))
t0 = time.perf_counter()
ref.initial_setup()
t1 = time.perf_counter()
print(f"{case} yardstick: mpm_initial_setup of the surviving {left.shape[0]} particles: wall {1e3 * (t1 - t0):.3f} ms")
ref.close()

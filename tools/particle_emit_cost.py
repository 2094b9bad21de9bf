#!/usr/bin/env python
"""What an emission costs (mpm_emit_particles) - the driver behind profiles/particle_emit.txt.
  faucet  scenes.faucet at test size (64^3, max_ppc 16) after 20 served substeps: one lattice layer of its disc
  c3      C3 (sand_column(9), 40 108 032 particles) after bench.py's default warm-up (10 substeps of 1e-4): 65 536 particles, a 32 x 8 x 32-cell
          slab of the lattice above the column
Each against the yardstick of the same process: mpm_initial_setup of the merged particle set (its positions read back) in a second context.
Wall times are host-side, around calls that synchronise; the per-kernel times come from the profiler.
Usage (one MI355X): rocprofv3 --kernel-trace --stats -f csv -d OUT -o emit -- python tools/particle_emit_cost.py faucet|c3"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from claymore_amd import scenes
from claymore_amd.engine import build_engine

case = sys.argv[1] if len(sys.argv) > 1 else "faucet"
if case == "faucet":
    sc = scenes.faucet(bits=6, radius_cells=3.0, speed=8.0, end=1.0)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.serve_emitters(0.0)
    for _ in range(20):
        eng.substep(1e-4, 0.0, 1.0, 1e-4)
        eng.cur_time += 1e-4
        eng.serve_emitters()
    new = eng.emitters[0].layer.astype(np.float32)
    v0 = tuple(eng.emitters[0].velocity)
else:
    sc = scenes.sand_column(9)
    eng = build_engine(sc)
    eng.initial_setup()
    eng.run_fixed(10, sc["dt"])
    new = scenes.lattice_box(9, (240, 340, 240), (272, 348, 272))
    v0 = (0.0, -1.0, 0.0)
print("build_info", eng.api.build_info().decode())
n_before = int(eng.counts().particles[0])
cap0 = eng.capacity()
reps = 3 if case == "faucet" else 2
for rep in range(reps):
    t0 = time.perf_counter()
    eng.emit(0, new + np.float32([0.0, 0.0, rep * 0.25 / (1 << sc["bits"])]) if rep else new, v0=v0)
    t1 = time.perf_counter()
    c = eng.counts()
    print(f"{case} emission {rep}: {new.shape[0]} particles into {n_before + rep * new.shape[0]}: wall {1e3 * (t1 - t0):.3f} ms; blocks {c.particle_blocks}/{c.neighbor_blocks}/{c.exterior_blocks}, "
          f"transient staging {56 * int(c.particles[0]) / 1e6:.1f} MB at 56 B a particle (tracked; 52 B untracked), capacity events {eng.capacity()[2] - cap0[2]}")
merged = eng.retrieve_positions(0)
eng.close()
ref = build_engine(dict(sc, models=[dict(sc["models"][0], xyz=merged)], emitters=[]))
t0 = time.perf_counter()
ref.initial_setup()
t1 = time.perf_counter()
print(f"{case} yardstick: mpm_initial_setup of the merged {merged.shape[0]} particles: wall {1e3 * (t1 - t0):.3f} ms")
ref.close()

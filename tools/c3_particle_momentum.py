#!/usr/bin/env python
"""C3 (40.1 M sand particles) after bench.py's default warm-up (10 substeps of 1e-4): twice a velocity readout and the device-side totals of
the same readout (mpm_particle_momentum) - the driver behind profiles/c3_particle_momentum.txt (readout_kernel<kReadVelocity> against
readout_kernel<kReadMomentum>, then kernels of their own), with the totals checked against a float64 sum over the readout.
Usage (one MI355X): rocprofv3 --kernel-trace --stats -f csv -d OUT -o c3 -- python tools/c3_particle_momentum.py"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from claymore_amd import scenes
from claymore_amd.engine import build_engine
sc = scenes.sand_column(9)
eng = build_engine(sc)
eng.initial_setup()
eng.run_fixed(10, sc["dt"])
print("build_info", eng.api.build_info().decode())
mass = eng.model_mass(0)
for rep in range(2):
    t0 = time.perf_counter(); x, v = eng.retrieve_velocity(0); t1 = time.perf_counter()
    tot = eng.particle_momentum(0); t2 = time.perf_counter()
    v64 = v.astype(np.float64)
    p, k = mass * v64.sum(axis=0), 0.5 * mass * float(np.sum(v64 * v64))
    print(f"rep {rep}: n {x.shape[0]} count {tot['count']}  wall velocity {t1-t0:.3f} s  totals {t2-t1:.4f} s")
    print(f"  momentum {tot['momentum'].tolist()} (float64 sum {p.tolist()}, rel {np.abs(tot['momentum'] - p).max() / np.abs(p).max():.3g})")
    print(f"  kinetic {tot['kinetic']!r} (float64 sum {k!r}, rel {abs(tot['kinetic'] - k) / k:.3g})")
eng.close()

#!/usr/bin/env python
"""C3 (40.1 M sand particles) after bench.py's default warm-up (10 substeps of 1e-4): twice a position readout, a velocity readout and a
velocity + C readout - the driver behind profiles/c3_velocity_readout.txt (readout_kernel<kReadState> against readout_kernel<kReadVelocity>;
that profile predates both, when the position readout was a kernel of its own with one slot atomic per particle).
Usage (one MI355X): rocprofv3 --kernel-trace --stats -f csv -d OUT -o c3 -- python tools/c3_velocity_readout.py"""
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
for rep in range(2):
    t0 = time.perf_counter(); x = eng.retrieve_positions(0); t1 = time.perf_counter()
    x2, v = eng.retrieve_velocity(0); t2 = time.perf_counter()
    x3, v3, c3 = eng.retrieve_velocity(0, affine=True); t3 = time.perf_counter()
    print(f"rep {rep}: n {x.shape[0]} {x2.shape[0]} {x3.shape[0]}  wall positions {t1-t0:.3f} s  velocity {t2-t1:.3f} s  velocity+C {t3-t2:.3f} s")
print("v_y range", float(v[:, 1].min()), float(v[:, 1].max()), "g t", 10 * 1e-4 * float(np.float32(eng.cfg.gravity)))
eng.close()

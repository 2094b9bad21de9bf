#!/usr/bin/env python
"""C3 (40.1 M sand particles) after bench.py's default warm-up (10 substeps of 1e-4): three times a state readout (mpm_retrieve_state), a
stress readout (mpm_retrieve_stress) and the stress totals (mpm_stress_totals) in one process - the driver behind
profiles/c3_stress_readout.txt.  Wall time of each call (kernel, device-to-host copies and the host arrays' first touch included), the best
of the repetitions, and the ratios to the state readout of the same run.  After the warm-up the column is still in free fall: every
particle is undeformed and the stress functions leave through their wave-uniform early exit, so --steps N runs N further substeps first
(the column reaches the floor after some 900).
Usage (one MI355X): python tools/c3_stress_readout.py [--steps N] [--out profiles/c3_stress_readout.txt]"""
import argparse
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from claymore_amd import scenes
from claymore_amd.engine import build_engine
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "c3_stress_readout.txt"))
args = ap.parse_args()
sc = scenes.sand_column(9)
eng = build_engine(sc)
eng.initial_setup()
eng.run_fixed(10 + args.steps, sc["dt"])
lines = [f"C3 sand column, {10 + args.steps} substeps of {sc['dt']}; {eng.api.build_info().decode()}"]
best = {"state": 1e30, "stress": 1e30, "totals": 1e30}
for rep in range(args.reps):
    t0 = time.perf_counter(); xs, st, lj = eng.retrieve_state(0); t1 = time.perf_counter()
    x, s6, scal = eng.retrieve_stress(0); t2 = time.perf_counter()
    tot = eng.stress_totals(0); t3 = time.perf_counter()
    took = {"state": t1 - t0, "stress": t2 - t1, "totals": t3 - t2}
    lines.append(f"rep {rep}: n {xs.shape[0]} {x.shape[0]} {tot['count']}  wall mpm_retrieve_state {took['state']:.4f} s  mpm_retrieve_stress {took['stress']:.4f} s  mpm_stress_totals {took['totals']:.4f} s")
    best = {k: min(best[k], took[k]) for k in best}
    del xs, st, lj
lines.append(f"best: state {best['state']:.4f} s  stress {best['stress']:.4f} s ({best['stress'] / best['state']:.2f} x state)  totals {best['totals']:.4f} s ({best['totals'] / best['state']:.3f} x state)")
lines.append(f"max von Mises {tot['max_von_mises']:.6g} (readout {float(scal[:, 2].max()):.6g}), J range {float(scal[:, 0].min()):.6g} .. {float(scal[:, 0].max()):.6g}, stress integral {tot['stress_integral']}")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
open(args.out, "w").write(text)
eng.close()

#!/usr/bin/env python
"""Times of the surface readout (mpm_grid_isosurface) on C3 = scenes.sand_column(9) at half the rest density, beside mpm_grid_volume at
stride 1 over the box of nodes that holds every registered block - the only way to a surface before - the driver behind
profiles/grid_isosurface.txt.
  --flow K   run K substeps after the 10 of the rest window first (3000: the column has collapsed into a pile)
The calls are timed with the host clock (they end in a synchronise; a fetch includes the staging allocation and the copy to the host); the
kernels' own times come from the profiler:
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/grid_isosurface_rates.py [--flow K]; python tools/rocpd_summary.py OUT/t_results.db"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from claymore_amd import scenes  # noqa: E402
from claymore_amd.engine import build_engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--flow", type=int, default=0)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

sc = scenes.sand_column(9)
N = 1 << sc["bits"]
eng = build_engine(sc)
eng.initial_setup()
eng.run_fixed(10 + args.flow, sc["dt"])
rho = eng.default_material(sc["models"][0]["material"]).rho
iso = float(np.float32(0.5 * rho * eng.dx ** 3))
print("build_info", eng.api.build_info().decode(), "| particles", sum(m["xyz"].shape[0] for m in sc["models"]), "| substeps", 10 + args.flow, "| lost", eng.diagnostics().lost_particles)
cnt = eng.counts()
print("blocks particle / neighbour / exterior:", cnt.particle_blocks, cnt.neighbor_blocks, cnt.exterior_blocks, f"| rho {rho} -> iso_mass {iso!r}")


def best(fn):
    walls = []
    for _ in range(args.reps + 1):                                              # (the first is the warm-up)
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
    return 1e3 * min(walls[1:]), out


def call(tris=None, vel=None, cap=0):
    n = C.c_size_t(cap)
    eng._check(eng.api.grid_isosurface(eng.ctx, iso, None, None, None if tris is None else tris.ctypes.data_as(C.c_void_p),
                                       None if vel is None else vel.ctypes.data_as(C.c_void_p), C.byref(n)))
    return n.value


ms, count = best(call)
print(f"count only: {count} triangles; call wall best {ms:.3f} ms")
tris, vel = np.empty((count, 3, 3), np.float32), np.empty((count, 3, 3), np.float32)
ms, _ = best(lambda: call(tris, None, count))
print(f"positions: {tris.nbytes} B to the host; call wall best {ms:.3f} ms")
ms, _ = best(lambda: call(tris, vel, count))
print(f"positions and velocities: {tris.nbytes + vel.nbytes} B to the host; call wall best {ms:.3f} ms")
ms, mesh = best(lambda: eng.isosurface(iso_mass=iso))
print(f"Engine.isosurface (count, fetch, weld on the host): {len(mesh[0])} vertices, {len(mesh[1])} faces; wall best {ms:.1f} ms")
keys, _ = eng.dump_grid()
lo, hi = 4 * keys.min(axis=0), 4 * keys.max(axis=0) + 4
dims = tuple(int(v) for v in hi - lo)
ms, vol = best(lambda: eng.grid_volume(tuple(int(v) for v in lo), dims, 1))
print(f"for scale, mpm_grid_volume stride 1 over the registered blocks' box {dims} from {tuple(int(v) for v in lo)}: {vol.nbytes} B to the host; call wall best {ms:.3f} ms; "
      f"{int((vol[0] > iso).sum())} nodes inside")
eng.close()

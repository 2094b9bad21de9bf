#!/usr/bin/env python
"""Times of the Eulerian readouts (mpm_grid_volume at strides 1, 2, 4; mpm_sample_grid; mpm_grid_box_totals) beside a device-to-device
hipMemcpy that moves the same number of bytes in the same process - the driver behind profiles/grid_field.txt.
  --case c1   scenes.two_spheres(7) (C1): the whole 128^3 domain
  --case c3   scenes.sand_column(9) (C3, 40.1 M particles) after 10 substeps: the box of nodes around the column, 136 x 316 x 136
What the volume kernel must move: every registered block that meets the box once (1 KiB) and the output once (16 B a cell).  The copy is
timed with events around hipMemcpyAsync of HALF that many bytes (a copy reads and writes each byte: the same traffic), the calls with the
host clock (they end in a synchronise and include the scratch allocation and the copy of the result to the host); the kernels' own times
come from the profiler:
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/grid_field_rates.py --case c3; python tools/rocpd_summary.py OUT/t_results.db"""
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
ap.add_argument("--case", choices=["c1", "c3"], default="c1")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

sc = scenes.two_spheres(7) if args.case == "c1" else scenes.sand_column(9)
N = 1 << sc["bits"]
eng = build_engine(sc)
eng.initial_setup()
eng.run_fixed(10, sc["dt"])
print("build_info", eng.api.build_info().decode(), "| case", args.case, "| particles", sum(m["xyz"].shape[0] for m in sc["models"]))
cnt = eng.counts()
print("blocks particle / neighbour / exterior:", cnt.particle_blocks, cnt.neighbor_blocks, cnt.exterior_blocks)
keys, _ = eng.dump_grid()

hip = C.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
hip.hipFree.argtypes = [C.c_void_p]
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def ok(rc):
    if rc != 0:
        raise RuntimeError(f"hip error {rc}")


def copy_ms(nbytes, reps):
    """Best of `reps` device-to-device hipMemcpyAsync of nbytes on the null stream, by events (ms)."""
    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(a), nbytes)), ok(hip.hipMalloc(C.byref(b), nbytes))
    ok(hip.hipMemset(a, 1, nbytes)), ok(hip.hipMemset(b, 2, nbytes))
    ok(hip.hipEventCreate(C.byref(e0))), ok(hip.hipEventCreate(C.byref(e1)))
    best = None
    for rep in range(reps + 1):                                                  # (the first is the warm-up)
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(b, a, nbytes, 3, None))                             # 3 = hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float(0)
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        best = ms.value if rep <= 1 else min(best, ms.value)
    hip.hipFree(a), hip.hipFree(b)
    return best


if args.case == "c1":
    origin, nodes = (0, 0, 0), (N, N, N)
else:
    origin, nodes = (188, 8, 188), (136, 316, 136)
lo, hi = np.array(origin), np.array(origin) + np.array(nodes)
met = int((((4 * keys + 3) >= lo) & ((4 * keys) < hi)).all(axis=1).sum())
for stride in (1, 2, 4):
    dims = tuple(n // stride for n in nodes)
    out_bytes = 16 * dims[0] * dims[1] * dims[2]
    traffic = 1024 * met + out_bytes
    walls = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        v = eng.grid_volume(origin, dims, stride)
        walls.append(time.perf_counter() - t0)
    cms = copy_ms(traffic // 2, args.reps)
    print(f"volume stride {stride}: box {dims} cells from {origin}, {met} registered blocks met, reads {1024 * met} B + writes {out_bytes} B = {traffic} B; "
          f"call wall best {1e3 * min(walls[1:]):.3f} ms (with allocation and the copy to the host); hipMemcpy D2D of {traffic // 2} B: {cms:.4f} ms = {traffic / cms / 1e6:.1f} GB/s of traffic; "
          f"mass {float(v[0].astype(np.float64).sum())!r}")
rng = np.random.default_rng(1)
for n in (1000, 1000000):
    pts = ((4.0 * keys[rng.integers(0, len(keys), n)] + rng.uniform(0, 4, (n, 3))) / N).astype(np.float32)
    walls = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        s = eng.sample_grid(pts)
        walls.append(time.perf_counter() - t0)
    print(f"sample {n} points over the registered blocks: call wall best {1e3 * min(walls[1:]):.3f} ms; {int((s['mass'] > 0).sum())} with mass")
walls = []
for _ in range(args.reps + 1):
    t0 = time.perf_counter()
    t = eng.grid_box_totals(lo, hi)
    walls.append(time.perf_counter() - t0)
print(f"box totals over the same box: call wall best {1e3 * min(walls[1:]):.3f} ms; mass {t['mass']!r} kinetic {t['kinetic']!r}; grid_totals mass {eng.grid_totals()[0]!r}")
eng.close()

#!/usr/bin/env python
"""Times of the mesh-sampled model (mpm_sample_mesh) for a subdivision-5 icosphere (20 480 triangles) of radius 0.3 at several resolutions,
beside mpm_set_collision_mesh of the same mesh in the same run - the existing kernel doing one evaluation per node where this one decides
8 candidates per node - the driver behind profiles/mesh_fill.txt.
  --bits 7 8 9   the resolutions
  --reps 3       repetitions; the calls alternate
The calls are timed with the host clock (they end in a synchronise); the classify / scan / emit split, the tiles of the clipped range and
the tiles decided from their centre come from mpm_test_mesh_fill (device events around the kernels)."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, nargs="+", default=[7, 8, 9])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--subdivisions", type=int, default=5)
args = ap.parse_args()

api = _ffi.load_hip()
verts, tris = scenes.icosphere((0.5, 0.5, 0.5), 0.3, args.subdivisions)
print(f"icosphere: {len(tris)} triangles, {len(verts)} vertices, radius 0.3", flush=True)
for bits in args.bits:
    call = (bits, verts.ctypes.data, len(verts), tris.ctypes.data, len(tris), None)
    n = C.c_size_t(0)
    assert api.sample_mesh(*call, None, C.byref(n), 0) == 0                                         # warm-up, and the count
    total = n.value
    buf = np.empty((total, 3), dtype=np.float32)
    eng = Engine(domain_bits=bits)
    eng.set_collision_mesh(verts, tris)                                                             # warm-up
    t_count, t_fetch, t_field, stats = [], [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        assert api.sample_mesh(*call, None, C.byref(n), 0) == 0
        t1 = time.perf_counter()
        n = C.c_size_t(total)
        assert api.sample_mesh(*call, buf.ctypes.data, C.byref(n), 0) == 0
        t2 = time.perf_counter()
        eng.set_collision_mesh(verts, tris)
        t3 = time.perf_counter()
        st = (C.c_double * 8)()
        assert api.test_mesh_fill(*call, st, 0) == 0
        t_count.append(t1 - t0), t_fetch.append(t2 - t1), t_field.append(t3 - t2), stats.append(list(st))
    eng.close()
    nodes = (1 << bits) ** 3
    st = min(stats, key=lambda s: s[3] + s[4] + s[5])
    dev = (st[3] + st[4] + st[5]) * 1e-3
    cand = 8 * 64 * st[1]
    ms = lambda ts: " ".join(f"{1e3 * t:.2f}" for t in ts)
    print(f"bits {bits}: {total} points; tiles {int(st[1])}, decided from the centre {int(st[2])} ({100 * st[2] / st[1]:.1f} %)")
    print(f"  mpm_sample_mesh count call  : {ms(t_count)} ms (host clock, whole call)")
    print(f"  mpm_sample_mesh fetch call  : {ms(t_fetch)} ms (host clock, whole call, with the copy of {12 * total / 2 ** 20:.0f} MiB to the host)")
    print(f"  kernels (device events)     : classify {' '.join(f'{s[3]:.3f}' for s in stats)} ms, scan {' '.join(f'{s[4]:.3f}' for s in stats)} ms, "
          f"emit {' '.join(f'{s[5]:.3f}' for s in stats)} ms")
    print(f"  mpm_set_collision_mesh      : {ms(t_field)} ms (host clock, whole call; {nodes} nodes)")
    print(f"  per candidate of the clipped range ({int(cand)}): {1e9 * dev / cand:.3f} ns (kernels); per node of the field: {1e9 * min(t_field) / nodes:.3f} ns "
          f"(whole call)", flush=True)

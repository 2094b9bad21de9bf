#!/usr/bin/env python
"""Install times of the mesh-built collision field (mpm_set_collision_mesh) for a subdivision-5 icosphere (20 480 triangles) at several
resolutions, beside mpm_set_collision_object fed the same field from host arrays - the route it replaces - the driver behind
profiles/collision_mesh.txt.
  --bits 7 8 9   the resolutions
  --tiles K      tiles sampled for the candidate statistics (the kernel's own test restated with the NumPy model's float32 walk, on the host)
The calls are timed with the host clock (they end in a synchronise).  The host part of an install - validation, adjacency, records - is the
time of an install of the same mesh wound inward: it goes through all of it and is refused by the last check, before the device is touched.
The kernel's own time comes from the profiler:
    rocprofv3 --kernel-trace --stats -d OUT -o t -- python tools/collision_mesh_rates.py --bits 8; python tools/rocpd_summary.py OUT/t_results.db"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import collision_mesh_model as mm  # noqa: E402
from claymore_amd import scenes  # noqa: E402
from claymore_amd.engine import Engine, EngineError  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bits", type=int, nargs="+", default=[7, 8, 9])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tiles", type=int, default=256)
ap.add_argument("--subdivisions", type=int, default=5)
args = ap.parse_args()

verts, tris = scenes.icosphere((0.47, 0.53, 0.51), 0.3, args.subdivisions)
mesh = mm.Mesh(verts, tris)
print(f"icosphere: {len(verts)} vertices, {len(tris)} triangles, volume {mesh.volume:.6f}")


def best(fn):
    walls = []
    for _ in range(args.reps + 1):                                              # (the first is the warm-up)
        t0 = time.perf_counter()
        out = fn()
        walls.append(time.perf_counter() - t0)
    return 1e3 * min(walls[1:]), out


def refused(eng):
    try:
        eng.set_collision_mesh(verts, tris[:, ::-1])
    except EngineError:
        return
    raise SystemExit("the inward-wound mesh was accepted")


def candidates(bits, count):
    """Per sampled tile: the triangles that pass the kernel's test q(centre) <= ((D + 2 r) (1 + 2^-6) + slack)^2."""
    n, dx = 1 << bits, np.float32(1.0 / (1 << bits))
    rng = np.random.default_rng(1)
    tiles = rng.integers(0, n // 4, (count, 3))
    centre = ((4 * tiles).astype(np.float32) + np.float32(1.5)) * dx
    slack = max(np.float32(0.25) * dx, np.float32(max(1.0, np.abs(verts).max())) * np.float32(2.0 ** -12))
    out = []
    for s in range(0, count, 32):
        q, _, _ = mm.walk(centre[s:s + 32, None, :], mesh.a[None], mesh.ab[None], mesh.ac[None])
        thr = (np.sqrt(q.min(axis=1)) + np.float32(2.0) * (np.float32(2.598076211) * dx)) * np.float32(1.015625) + slack
        out.append((q <= (thr * thr)[:, None]).sum(axis=1))
    return np.concatenate(out)


for bits in args.bits:
    eng = Engine(domain_bits=bits)
    n = 1 << bits
    print(f"--- domain_bits {bits}: {n}^3 nodes, field {16 * n ** 3 / 2 ** 20:.0f} MiB; build_info {eng.api.build_info().decode()}")
    host_ms, _ = best(lambda: refused(eng))
    total_ms, _ = best(lambda: eng.set_collision_mesh(verts, tris))
    print(f"mpm_set_collision_mesh: call wall best {total_ms:.1f} ms, of it host validation / adjacency / records {host_ms:.1f} ms, "
          f"allocation + upload + kernel {total_ms - host_ms:.1f} ms")
    read_ms, field = best(lambda: eng.collision_field())
    sdf = np.ascontiguousarray(field[..., 0])
    grad = np.ascontiguousarray(np.moveaxis(field[..., 1:], -1, 0))
    del field
    print(f"mpm_get_collision_field, whole domain: {sdf.nbytes * 4} B to the host; call wall best {read_ms:.1f} ms")
    object_ms, _ = best(lambda: eng.set_collision_object(sdf, grad))
    print(f"mpm_set_collision_object fed that field from host arrays ({sdf.nbytes * 4 / 2 ** 20:.0f} MiB over the call): call wall best {object_ms:.1f} ms")
    if args.tiles:
        c = candidates(bits, args.tiles)
        print(f"candidates per tile over {len(c)} random tiles: mean {c.mean():.1f}, max {int(c.max())}, of {len(tris)}")
    eng.close()

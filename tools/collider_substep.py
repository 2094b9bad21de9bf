#!/usr/bin/env python
"""Per-phase substep times of mpm_run_fixed with a collision object: none / static / moving / shape / shapes4, for one or several prebuilt engine
libraries in ONE process, interleaved (lib A, lib B, lib A, ...), so that a parent build and a branch build are compared on the same
box under the same conditions.

    python tools/collider_substep.py [--scene c1|c2|c3] [--steps 200] [--warmup 50] [--reps 3] [--objects none,static,moving,shape,body,shapes4,ground_hf,ground_shape,ground_field,vol_mesh,vol_mesh4,field_mesh] [--phase 20]
                                     [--loads] [--forces none,uniform,drag_box,four] [--out FILE] [lib.so ...]

Scene: C2 (one elastic sphere of ~5 M particles dropped at 256^3; the level-set field is 256^3 float4 = 256 MiB) or C3 (the sand column at
512^3; the field is 2 GiB).  The object is a sphere below the material, far enough that nothing touches it during the measurement: the
kernel evaluates it at every grid node with mass either way, which is the cost in question.  A library without the clock's entry points
(a parent build) runs `none` and `static` only.  `shape`: the same sphere given in closed form (mpm_set_collision_shape: no field, no loads);
`body`: that sphere as a rigid body (mpm_set_collider_body, every axis locked, so at rest like the prescribed one: mpm_run_fixed then applies every update through grid_update_body_kernel +
body_step_kernel, unfused; with --loads the readout ahead of it is collider_loads_kernel<BodyArgs>, the same frame without the stores); `shapes4`: that sphere, a floor half-space, a box and a capsule in the four slots, all clear of the material.  A library without
mpm_set_collision_shape skips both.  `ground_hf` / `ground_shape` / `ground_field`: one flat ground just under the material given three ways -
a heightfield (mpm_set_collision_heightfield: an (N + 1)^2 table of constant height at spacing dx, four float4 gathers per massed cell), the
half-space shape at that height, and the level set of the same plane (sdf = y - height, gradient +y) - the same physics (the level set
alone stops at query_sdf's box); a library without mpm_set_collision_heightfield skips `ground_hf`.  --phase N: after the run, N more substeps phase by phase (grid update, G2P2G, rebuild), whose median
grid-update time is the stand-alone kernel's (`phase_grid_ms`); in mpm_run_fixed the update rides on the carry-over inside `partition_ms`.
`vol_mesh` / `vol_mesh4` / `field_mesh`: a subdivision-5 icosphere (20 480 triangles) of the sphere's place and size as a volume at
spacing dx built on the device (mpm_set_collision_volume_mesh), four such bodies in the four slots, and the same body through mpm_set_collision_mesh (the level-set
object: a float4 per node of the whole domain); `install_ms` is the wall-clock time of the installs.  `--scene c1`: C2's sphere at 128^3.
`object_bytes`: device memory taken by installing the collider (hipMemGetInfo before and after).  Prints one JSON line per (rep, library, object) with the library's per-substep averages
(HIP events on the compute stream) and the wall-clock time per substep, then a summary of medians.  --loads: a library with mpm_load_gauge then switches the
load gauge on and measures again - `loads_*`: mpm_run_fixed with every grid update a kernel of its own behind collider_loads_kernel and its reduction (no fused
carry-over), and the phase-level grid update, whose time then holds the readout's two kernels as well: `loads_phase_grid_ms - phase_grid_ms` is their cost.
--forces: every (library, object) is measured once per entry of the list - `none`: no force field; `uniform`: one UNIFORM field; `drag_box`: one DRAG
field in a feathered box around the material; `four`: UNIFORM in a half-space, DRAG in a feathered box, VORTEX in a capsule and POINT in a sphere, all four
slots (mpm_set_force_field; a library without it runs `none` only).  With a field mpm_run_fixed applies every grid update in a launch of its own behind
grid_force_kernel (no fused carry-over): `grid_ms` then holds the fields' pass and the update, `partition_ms` a rebuild without the update, and
`phase_grid_ms - phase_grid_ms of none` is the fields' pass alone."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from claymore_amd import _ffi, scenes  # noqa: E402
from claymore_amd.engine import build_engine  # noqa: E402


def load(path):
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    names = {n: sig for n, sig in {**_ffi.SIGNATURES, **_ffi.HIP_ONLY}.items() if hasattr(lib, "mpm_" + n)}
    return _ffi.Api(lib, "mpm_", names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", default=[_ffi.HIP_LIB_PATH])
    ap.add_argument("--scene", default="c2", choices=["c1", "c2", "c3"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--objects", default="none,static,moving,shape,shapes4")
    ap.add_argument("--phase", type=int, default=20)
    ap.add_argument("--loads", action="store_true")
    ap.add_argument("--forces", default="none")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = scenes.sphere_drop() if a.scene == "c2" else scenes.sphere_drop(bits=7, radius_cells=26.5) if a.scene == "c1" else scenes.sand_column()
    bits = sc["bits"]
    sdf, grad = scenes.sphere_level_set(bits, (0.5, 0.12, 0.5), 0.06)
    col = {"sdf": sdf, "grad": grad, "type": 1, "friction": 0.3, "trans": (0.5, 0.12, 0.5)}
    ground, n = 0.02, 1 << bits
    bodies = [((0.5, 0.12, 0.5), 0.06), ((0.2, 0.1, 0.2), 0.05), ((0.75, 0.1, 0.3), 0.04), ((0.3, 0.1, 0.75), 0.04)]
    meshes = [scenes.icosphere(c, r, 5) for c, r in bodies] if any(o in a.objects.split(",") for o in ("vol_mesh", "vol_mesh4", "field_mesh")) else []
    apis = [(os.path.basename(os.path.dirname(os.path.abspath(p))) + "/" + os.path.basename(p), load(p)) for p in a.libs]
    rows, lines = [], []
    box = {"kind": "box", "a": (0.5, 0.4, 0.5), "b": (0.3, 0.35, 0.3)}
    force_sets = {"none": [], "uniform": [dict(kind="uniform", vec=(0.5, 0.0, 0.25))],
                  "drag_box": [dict(kind="drag", vec=(1.0, 0.0, 0.0), strength=5.0, region=box, feather=8.0 / n)],
                  "four": [dict(kind="uniform", vec=(0.5, 0.0, 0.25), region={"kind": "halfspace", "a": (0.5, 0.5, 0.5), "b": (0.0, 1.0, 0.0)}),
                           dict(kind="drag", vec=(1.0, 0.0, 0.0), strength=5.0, region=box, feather=8.0 / n),
                           dict(kind="vortex", vec=(0.0, 1.0, 0.0), centre=(0.5, 0.0, 0.5), swirl=2.0, pull=0.5, region={"kind": "capsule", "a": (0.5, 0.1, 0.5), "b": (0.5, 0.7, 0.5), "radius": 0.2}),
                           dict(kind="point", centre=(0.5, 0.4, 0.5), strength=0.5, falloff=1, soft=0.05, region={"kind": "sphere", "a": (0.5, 0.4, 0.5), "radius": 0.3})]}
    for rep in range(a.reps):
        for name, api in apis:
            for obj, force in ((o, f) for o in a.objects.split(",") for f in a.forces.split(",")):
                if force != "none" and not hasattr(api, "set_force_field"):
                    continue
                if (obj == "moving" and not hasattr(api, "set_collision_clock")) or (obj in ("shape", "shapes4") and not hasattr(api, "set_collision_shape")):
                    continue
                if obj in ("vol_mesh", "vol_mesh4") and not hasattr(api, "set_collision_volume_mesh"):
                    continue
                if (obj == "ground_hf" and not hasattr(api, "set_collision_heightfield")) or (obj == "ground_shape" and not hasattr(api, "set_collision_shape")):
                    continue
                if obj == "body" and not hasattr(api, "set_collider_body"):
                    continue
                eng = build_engine(sc, api=api)
                free0 = torch.cuda.mem_get_info()[0]
                t_install = time.perf_counter()
                if obj in ("shape", "shapes4", "body"):
                    eng.set_collision_shape(0, "sphere", a=(0.5, 0.12, 0.5), radius=0.06, type=1, friction=0.3, trans=(0.5, 0.12, 0.5))
                if obj == "body":  # the same sphere as a rigid body, every axis locked (at rest like the prescribed one): every update is grid_update_body_kernel + body_step_kernel
                    eng.set_collider_body(0, density=2500.0, gravity=False, lock="x y z rx ry rz")
                if obj == "shapes4":
                    eng.set_collision_shape(1, "halfspace", a=(0.5, 0.02, 0.5), b=(0.0, -1.0, 0.0), inside_out=True, type=1, friction=0.3)
                    eng.set_collision_shape(2, "box", a=(0.2, 0.1, 0.2), b=(0.05, 0.04, 0.05), type=0)
                    eng.set_collision_shape(3, "capsule", a=(0.75, 0.1, 0.3), b=(0.75, 0.1, 0.7), radius=0.04, type=2, friction=0.3)
                elif obj == "ground_hf":
                    eng.set_collision_heightfield(0, np.full((n + 1, n + 1), ground, np.float32), origin=(0.0, 0.0), spacing=1.0 / n, type=1, friction=0.3)
                elif obj == "ground_shape":
                    eng.set_collision_shape(0, "halfspace", a=(0.5, ground, 0.5), b=(0.0, 1.0, 0.0), type=1, friction=0.3)
                elif obj == "ground_field":
                    gsdf = np.broadcast_to((np.arange(n, dtype=np.float32) / np.float32(n) - np.float32(ground))[None, :, None], (n, n, n))
                    ggrad = np.zeros((3, n, n, n), np.float32)
                    ggrad[1] = 1.0
                    eng.set_collision_object(sdf=gsdf, grad=ggrad, type=1, friction=0.3)
                    del gsdf, ggrad
                elif obj in ("vol_mesh", "vol_mesh4"):
                    for slot, mesh in enumerate(meshes[:4 if obj == "vol_mesh4" else 1]):
                        eng.set_collision_volume_mesh(slot, *mesh, spacing=1.0 / n, pad=2, type=1, friction=0.3)
                elif obj == "field_mesh":
                    eng.set_collision_mesh(*meshes[0], type=1, friction=0.3)
                elif obj in ("static", "moving"):
                    eng.set_collision_object(**col, **({"trans_vel": (0.0, 0.05, 0.0), "omega": (1.0, 2.0, 3.0), "dsdt": 0.1} if obj == "moving" else {}))
                if obj == "moving":
                    eng.set_collision_clock(True, 0.0)
                install_ms = (time.perf_counter() - t_install) * 1e3
                object_bytes = free0 - torch.cuda.mem_get_info()[0]
                eng.initial_setup()
                for slot, f in enumerate(force_sets[force]):
                    eng.set_force_field(slot, **f)
                eng.run_fixed(a.warmup, sc["dt"])
                t0 = time.perf_counter()
                eng.run_fixed(a.steps, sc["dt"])
                wall = (time.perf_counter() - t0) * 1e3 / a.steps
                t = eng.timers()
                phase = []
                for _ in range(a.phase):
                    eng.grid_update(sc["dt"])
                    phase.append(eng.timers().grid_update_ms)
                    eng.g2p2g(sc["dt"], sc["dt"])
                    eng.rebuild_partition()
                row = {"rep": rep, "lib": name, "build": api.build_info().decode(), "scene": a.scene, "object": obj, "forces": force, "steps": a.steps, "wall_ms": round(wall, 5),
                       "grid_ms": round(t.grid_update_ms, 5), "g2p2g_ms": round(t.g2p2g_ms, 5), "partition_ms": round(t.partition_ms, 5), "total_ms": round(t.total_ms, 5),
                       "phase_grid_ms": round(statistics.median(phase), 5) if phase else None, "object_bytes": int(object_bytes), "install_ms": round(install_ms, 3)}
                if a.loads and hasattr(api, "load_gauge"):
                    eng.load_gauge(True)
                    eng.run_fixed(a.warmup, sc["dt"])
                    t0 = time.perf_counter()
                    eng.run_fixed(a.steps, sc["dt"])
                    wall = (time.perf_counter() - t0) * 1e3 / a.steps
                    t = eng.timers()
                    phase = []
                    for _ in range(a.phase):
                        eng.grid_update(sc["dt"])
                        phase.append(eng.timers().grid_update_ms)
                        eng.g2p2g(sc["dt"], sc["dt"])
                        eng.rebuild_partition()
                    gauge_rows, _, updates = eng.read_load_gauge()
                    row.update(loads_wall_ms=round(wall, 5), loads_grid_ms=round(t.grid_update_ms, 5), loads_g2p2g_ms=round(t.g2p2g_ms, 5), loads_partition_ms=round(t.partition_ms, 5),
                               loads_total_ms=round(t.total_ms, 5), loads_phase_grid_ms=round(statistics.median(phase), 5) if phase else None, loads_updates=updates,
                               loads_touched=sum(int(r["count"]) for r in gauge_rows.values()))
                eng.close()
                rows.append(row)
                lines.append(json.dumps(row))
                print(lines[-1], flush=True)
    for name, _ in apis:
        for obj, force in ((o, f) for o in a.objects.split(",") for f in a.forces.split(",")):
            sel = [r for r in rows if r["lib"] == name and r["object"] == obj and r["forces"] == force]
            if sel:
                med = {k: round(statistics.median(r[k] for r in sel), 5) for k in ("wall_ms", "grid_ms", "g2p2g_ms", "partition_ms", "total_ms") + (("phase_grid_ms",) if a.phase else ())}
                med.update(partition_lo=min(r["partition_ms"] for r in sel), partition_hi=max(r["partition_ms"] for r in sel), object_bytes=sel[0]["object_bytes"], install_ms=round(statistics.median(r["install_ms"] for r in sel), 3))
                med.update(lo=min(r["wall_ms"] for r in sel), hi=max(r["wall_ms"] for r in sel))
                if "loads_wall_ms" in sel[0]:
                    med.update({k: round(statistics.median(r[k] for r in sel), 5) for k in ("loads_wall_ms", "loads_grid_ms", "loads_g2p2g_ms", "loads_partition_ms", "loads_total_ms") + (("loads_phase_grid_ms",) if a.phase else ())})
                lines.append(json.dumps({"summary": name, "object": obj, "forces": force, "n": len(sel), **med}))
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

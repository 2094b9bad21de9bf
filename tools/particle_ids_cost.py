#!/usr/bin/env python
"""What persistent particle ids cost (mpm_track_particle_ids): per-phase substep times of mpm_run_fixed with tracking off and on,
interleaved in ONE process, in free fall (right after the warm-up) and in the flow (after --flow-start substeps).

    python tools/particle_ids_cost.py [--scene c3|c2] [--steps 100] [--warmup 10] [--flow-start 3000] [--reps 2] [--out FILE]

Scene: C3 (the sand column of the benchmark at full size) or C2 (one elastic sphere, ~5 M particles).  All times are per-substep averages
over --steps substeps from HIP events on the compute stream (mpm_get_timers).  move_ids_kernel is launched between the two events that
bracket the G2P2G launches, right behind G2P2G on the same stream, and nothing else differs between the two contexts: its own time is
`move_ms` = g2p2g_ms (on) - g2p2g_ms (off), the difference of two event intervals of the same rep.  `ids_bytes`: device memory the tracked
context takes beyond the untracked one (hipMemGetInfo).  Prints one JSON line per (rep, window, tracking) and a summary of medians with the
two ratios total_ms (on) / total_ms (off)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from claymore_amd import scenes  # noqa: E402
from claymore_amd.engine import build_engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="c3", choices=["c2", "c3"])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--flow-start", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = scenes.sphere_drop() if a.scene == "c2" else scenes.sand_column()
    dt = sc["dt"]
    rows, lines = [], []

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    for rep in range(a.reps):
        for track in (False, True):
            free0 = torch.cuda.mem_get_info()[0]
            eng = build_engine(dict(sc, track_ids=track))
            eng.initial_setup()
            used = free0 - torch.cuda.mem_get_info()[0]
            done = 0
            for window, start in (("fall", a.warmup), ("flow", a.flow_start)):
                if start > done:
                    eng.run_fixed(start - done, dt)
                    done = start
                t0 = time.perf_counter()
                eng.run_fixed(a.steps, dt)
                wall = (time.perf_counter() - t0) * 1e3 / a.steps
                done += a.steps
                t = eng.timers()
                row = {"rep": rep, "scene": a.scene, "window": window, "first_step": start, "steps": a.steps, "track_ids": track, "particles": int(eng.counts().particles[0]),
                       "wall_ms": round(wall, 5), "grid_ms": round(t.grid_update_ms, 5), "g2p2g_ms": round(t.g2p2g_ms, 5), "partition_ms": round(t.partition_ms, 5),
                       "total_ms": round(t.total_ms, 5), "device_bytes": int(used)}
                rows.append(row)
                say(row)
            if track:
                _, ids = eng.retrieve_ids(0)
                assert ids.size == row["particles"] and int(ids.min()) >= 0, "the tracked run lost its ids"
            eng.close()
    for window in ("fall", "flow"):
        med = {}
        for track in (False, True):
            sel = [r for r in rows if r["window"] == window and r["track_ids"] == track]
            med[track] = {k: statistics.median(r[k] for r in sel) for k in ("wall_ms", "grid_ms", "g2p2g_ms", "partition_ms", "total_ms", "device_bytes")}
        move = [on["g2p2g_ms"] - off["g2p2g_ms"] for off, on in zip([r for r in rows if r["window"] == window and not r["track_ids"]], [r for r in rows if r["window"] == window and r["track_ids"]])]
        say({"summary": window, "off": {k: round(v, 5) for k, v in med[False].items()}, "on": {k: round(v, 5) for k, v in med[True].items()},
             "move_ms": round(statistics.median(move), 5), "move_ms_lo_hi": [round(min(move), 5), round(max(move), 5)],
             "total_ratio": round(med[True]["total_ms"] / med[False]["total_ms"], 4), "g2p2g_ratio": round(med[True]["g2p2g_ms"] / med[False]["g2p2g_ms"], 4),
             "ids_bytes": int(med[True]["device_bytes"] - med[False]["device_bytes"])})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

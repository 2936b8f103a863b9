#!/usr/bin/env python3
"""Kernel time of the 3D env's render() (rbc3d_render.hpp) per frame at 800 x 608, next to what a host-side renderer would pay
before drawing anything: get_state() of the same handle.

    python scripts/render3d_timing.py [--lib path/to/variant.so] [--reps 30] [--out result.json]

Kernel time: HIP events recorded on the handle's stream around the launch (rbc_set_profiling / rbc_profile_read), after a
warm-up, median and minimum over --reps launches of the default view.  render() itself also uploads the table and copies the
frames to the host; its wall time is printed next to the kernel time.  The states are one real env-step after a random reset.
--lib selects a variant build made with __graft_entry__.build_hip(extra_flags=[...], out=...), e.g. "-DRBC_RENDER_TARGET=" (the
kernel with packed float32 instructions allowed, rbc3d_render.hpp).  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rbc-gym_amd"))

CASES = [((16, 32, 32), 1), ((32, 48, 48), 1), ((32, 48, 48), 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.lib:
        os.environ["RBC_HIP_LIB"] = os.path.abspath(args.lib)
    from rbc_gym import _native
    rows = []
    for shape, batch in CASES:
        for precision in ("f64", "f32"):
            sim = _native.NativeSim3D(batch=batch, shape=shape, ra=10000.0, precision=precision)
            sim.reset(np.arange(batch, dtype=np.uint64) + 1)
            sim.step(np.zeros((batch, 8, 8), np.float32))
            for _ in range(3):                                   # warm-up: code object, frame buffer
                sim.render()
            sim.set_profiling(args.reps)
            t0 = time.perf_counter()
            for _ in range(args.reps):
                frames = sim.render()
            wall = (time.perf_counter() - t0) / args.reps
            ms = sim.profile_read()
            sim.set_profiling(0)
            assert len(ms) == args.reps and (frames != 255).any()
            sim.get_state()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                sim.get_state()
            state = (time.perf_counter() - t0) / args.reps
            row = {"shape": list(shape), "batch": batch, "precision": precision, "lib": args.lib or "shipped",
                   "kernel_ms_per_frame_median": float(np.median(ms)) / batch, "kernel_ms_per_frame_min": float(ms.min()) / batch,
                   "kernel_ms_per_launch_median": float(np.median(ms)), "render_wall_ms_per_call": wall * 1e3,
                   "get_state_wall_ms_per_call": state * 1e3, "reps": args.reps}
            rows.append(row)
            print(json.dumps(row), flush=True)
            sim.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

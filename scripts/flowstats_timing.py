#!/usr/bin/env python3
"""Time rbc_get_flowstats (csrc/rbc_flowstats.hpp) with HIP events on the sim's stream: achieved bytes/s = the
state bytes, read once, over the time of the two launches, next to the on-box streaming rate rbc_copy_ceiling reports in the same run.
Every shape is timed over as many identical handles as hold 1 GiB of state, called in turn, so that no call finds its state in the
256 MB last-level cache; a warm-up, then three repeats of about half a second of device work each, interleaved over the shapes.
usage: python scripts/flowstats_timing.py [seconds per repeat]
       python scripts/flowstats_timing.py host     the route it replaces: get_fields() + the numpy expressions, wall time (needs
                                                   nothing of the statistics kernel, so it runs on older checkouts: RBC_GYM_PATH=...)"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.environ.get("RBC_GYM_PATH", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rbc-gym_amd")))
from rbc_gym import _native

SHAPES = [("2D 96x64 B=1024", 2, (64, 96), 1024), ("3D 32x48x48 B=32", 3, (32, 48, 48), 32)]


def make(dim, shape, B, prec):
    if dim == 3:
        sim = _native.NativeSim3D(batch=B, shape=shape, random_kick=0.1, precision=prec)
        nbytes = B * (3 * np.prod(shape) + (shape[0] + 1) * shape[1] * shape[2]) * (4 if prec == "f32" else 8)
    else:
        sim = _native.NativeSim(batch=B, nz=shape[0], nx=shape[1], precision=_native.PRECISIONS[prec])
        nbytes = B * (3 * shape[0] + 1) * shape[1] * 8                   # the resident kernel's state is float64 in both precisions
    sim.reset(np.arange(B, dtype=np.uint64) + 1)
    return sim, int(nbytes)


def numpy_route(sim):
    f = sim.get_fields()
    b, u, w = f[0], f[1], f[-1][:, :-1]
    hz = tuple(range(2, b.ndim))
    prof = [b.mean(hz), (u ** 2).mean(hz), (w ** 2).mean(hz), (b * w).mean(hz), (b ** 2).mean(hz)] + ([(f[2] ** 2).mean(hz)] if len(f) == 4 else [])
    ext = [np.abs(x).max(axis=tuple(range(1, x.ndim))) for x in f[1:]] + [b.min(axis=(1,) + hz), b.max(axis=(1,) + hz)]
    return prof, ext


if len(sys.argv) > 1 and sys.argv[1] == "host":
    for name, dim, shape, B in SHAPES:
        for prec in ("f64", "f32"):
            sim, _ = make(dim, shape, B, prec)
            numpy_route(sim)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                numpy_route(sim)
                ts.append(time.perf_counter() - t0)
            print(f"host route {name} {prec}: get_fields() + numpy {min(ts) * 1e3:.1f} ms (three runs: {', '.join(f'{t * 1e3:.1f}' for t in ts)})", flush=True)
            sim.close()
    sys.exit(0)

import torch
WINDOW = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5           # seconds of device work per repeat and shape
ROTATE_BYTES = 1 << 30                                               # state rotated through: four times the 256 MB last-level cache
stream = torch.cuda.Stream()
sets = []                                                            # (name, handles, state bytes of one handle)
for name, dim, shape, B in SHAPES:
    for prec in ("f64", "f32"):
        group, nbytes = [], 0
        while not group or len(group) * nbytes < ROTATE_BYTES:      # identical handles, called in turn: no call finds its state in the cache
            sim, nbytes = make(dim, shape, B, prec)
            sim._check(sim.lib.rbc_set_stream(sim.h, _native.torch_stream_handle(stream)))
            group.append(sim)
        sets.append((f"{name} {prec}", group, nbytes))


def timed(group, n):
    """n calls, round robin over the handles (both launches, nothing copied, nothing waited for) -> seconds per call by HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for i in range(n):
        sim = group[i % len(group)]
        sim._check(sim.lib.rbc_get_flowstats(sim.h, None, None))
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


calls = {name: max(200, int(WINDOW / timed(group, 10 * len(group)))) for name, group, _ in sets}      # (warm-up, and the window's length)
ceil = _native.copy_ceiling(0, 1 << 30, 10)
print(f"rbc_copy_ceiling: copy kernel {ceil['kernel_gbs']:.0f} GB/s, hipMemcpyAsync D2D {ceil['memcpy_d2d_gbs']:.0f} GB/s (bytes read + written)", flush=True)
times = {name: [] for name, _, _ in sets}
for rep in range(3):
    for name, group, _ in sets:
        times[name].append(timed(group, calls[name]))
for name, group, nbytes in sets:
    t = min(times[name])
    print(f"{name}: {t * 1e6:.1f} us per call ({calls[name]} calls over {len(group)} handles; three repeats: {', '.join(f'{x * 1e6:.1f}' for x in times[name])}), "
          f"{nbytes / 1e6:.1f} MB read once, {nbytes / t / 1e9:.0f} GB/s = {nbytes / t / 1e9 / ceil['kernel_gbs']:.2f} of the copy kernel's rate", flush=True)
    for sim in group:
        sim.close()

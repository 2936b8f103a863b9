#!/usr/bin/env python3
"""Time 3D grids that run the row / pencil projection (k3p_*): env-steps/s back to back and the fraction of the
10 F C s HBM roofline at 8 TB/s.
usage: python scripts/pencil3d_timing.py [steps] [B nz ny nx [precision [projection [dt_solver]]]]
projection: auto | pencil | chunked (the chunked y-z solve: grids beyond the one-plane bound, e.g. 8 64 128 128 f64 chunked 0.005;
RBC_PENCIL_CHUNK=<levels> and RBC_PENCIL_PREFETCH=0 are its A/B knobs).  Per-kernel times: run one grid under `rocprofv3 --kernel-trace --stats -- python scripts/pencil3d_timing.py 5 32 32 96 96`."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rbc-gym_amd"))
from rbc_gym import _native

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def run(B, shape, prec, **kw):
    sim = _native.NativeSim3D(batch=B, shape=shape, ra=1e4, random_kick=0.1, precision=prec, **kw)
    sim.reset(np.arange(B, dtype=np.uint64) + 1)
    act = np.random.default_rng(0).uniform(-1, 1, (B, 8, 8)).astype(np.float32)
    dact = torch.from_numpy(act).to("cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        sim.step_dev(dact.data_ptr())
    sim.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.step_dev(dact.data_ptr())                              # back to back: no host wait between env-steps
    sim.synchronize()
    dt = (time.perf_counter() - t0) / steps
    ok = not sim.get_flags().any()
    frac = sim.algorithmic_bytes_per_env_step() * B / dt / 8e12
    print(f"{shape[2]}x{shape[1]}x{shape[0]} {prec} B={B} projection path {sim.projection_path()}: {dt * 1e3:.2f} ms per batched env-step, {B / dt:.0f} env-steps/s, "
          f"{frac:.3f} of the roofline, {sim.algorithmic_bytes_per_env_step() / 1e6:.1f} MB algorithmic per env-step, finite={ok}, Nu={sim.get_nusselt()[0]:.4f}", flush=True)
    sim.close()


if len(sys.argv) > 5:
    kw = dict(projection=sys.argv[7]) if len(sys.argv) > 7 else {}
    if len(sys.argv) > 8:
        kw["dt_solver"] = float(sys.argv[8])
    run(int(sys.argv[2]), tuple(int(a) for a in sys.argv[3:6]), sys.argv[6] if len(sys.argv) > 6 else "f64", **kw)
else:
    run(32, (32, 96, 96), "f64")
    # (dz = 2/64: the default dt_solver = 0.01 is beyond the explicit scheme's stability range on this grid -- NaN after 13 env-steps,
    #  none with 0.005 -- so 25 substeps per env-step here; the roofline fraction is per byte and does not depend on it)
    run(8, (64, 128, 128), "f32", dt_solver=0.005)

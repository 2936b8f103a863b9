"""GPU parity, 3D grids beyond the one-plane pencil solve: the chunked y-z solve k3p_yz_chunked (projection="chunked", DESIGN.md section
3b) against the float64 3D CPU oracle.  RBC_PENCIL_CHUNK forces the chunk height: these small grids would all be one chunk."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity3d import native, o3, rel_l2  # noqa: F401  (fixtures)
from test_gpu_pencil3d import DOM, max_div, reset_and_step

gpu = pytest.mark.gpu
CHUNKED = 2      # rbc_debug_projection_path


@gpu
@pytest.mark.parametrize("shape, kc, precision", [((8, 64, 96), 4, "f64"),       # register-blocked transforms, even split
                                                  ((8, 64, 96), 3, "f64"),       # remainder chunk of 2
                                                  ((8, 64, 96), 16, "f64"),      # single chunk, no round trip through memory
                                                  ((9, 81, 75), 4, "f64"),       # generic transforms, odd sizes, remainder of 1
                                                  ((10, 60, 100), 1, "f64"),     # every level its own chunk
                                                  ((8, 96, 128), 3, "f32")])
def test_chunked_matches_oracle(native, o3, monkeypatch, shape, kc, precision):
    """the tolerances of test_pencil_matches_oracle and test_pencil_float32: the arithmetic per element is the same"""
    monkeypatch.setenv("RBC_PENCIL_CHUNK", str(kc))
    g0, o0, g1, o1, sim, o = reset_and_step(native, o3, shape, DOM, 9, projection="chunked", precision=precision)
    assert sim.projection_path() == CHUNKED
    errs = [rel_l2(x, y) for x, y in zip(g1, o1)]
    divs = (max_div(g0, shape, DOM), max_div(g1, shape, DOM))
    print(shape, kc, "rel-L2 after the step", errs, "max |div| after reset / step", divs)
    if precision == "f32":
        assert errs[0] < 1e-6 and max(errs[1:]) < 1e-4 and abs(sim.get_nusselt()[0] - o.nusselt()) < 1e-5 * abs(o.nusselt()), errs
        assert divs[1] < 2e-5 * np.abs(g1[1]).max() / (DOM[2] / shape[2])
    else:
        assert max(np.abs(x - y).max() for x, y in zip(g0, o0)) < 1e-13 and max(errs) < 1e-11 and max(divs) < 1e-13


@gpu
def test_chunked_env_groups_and_masked_reset(native, monkeypatch):
    """test_pencil_env_groups_and_masked_reset on the chunked solve: B = 9 is two env groups, every env bitwise a batch of one"""
    monkeypatch.setenv("RBC_PENCIL_CHUNK", "3")
    B, seeds, act = 9, np.arange(9, dtype=np.uint64) + 5, np.random.default_rng(2).uniform(-1, 1, (9, 8, 8)).astype(np.float32)
    kw = dict(shape=(8, 64, 96), domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1, projection="chunked")
    sim, one = native.NativeSim3D(batch=B, **kw), native.NativeSim3D(batch=1, **kw)
    sim.reset(seeds)
    assert sim.step(act)
    f = sim.get_fields()
    for e in range(B):
        one.reset(seeds[e:e + 1])
        assert one.step(act[e:e + 1])
        assert all(np.array_equal(x[e], y[0]) for x, y in zip(f, one.get_fields())), e
    sim.reset(seeds + 100, mask=[1] + [0] * (B - 1))
    for x, y in zip(f, sim.get_fields()):
        assert np.array_equal(x[1:], y[1:]) and not np.array_equal(x[0], y[0])


@gpu
def test_large_grid_runs_chunked_by_request_only(native):
    """float64 128 x 128 x 64, no chunk knob: refused under "auto" (the one-plane bound), served by projection="chunked".  Bound on
    max |div|: 4 x what the one-plane pencil solve gives on (32, 128, 128) with the same seed, domain and step, 8.22e-15 after the reset
    and 1.21e-14 after the step -- the recurrence is twice as long and round-off grows with nz"""
    shape, pencil_div_32 = (64, 128, 128), (8.215650382226158e-15, 1.2101430968414206e-14)
    kw = dict(batch=1, shape=shape, domain=DOM, ra=8000.0, dt_solver=0.005, dt_control=0.005, random_kick=0.1)
    with pytest.raises(native.RbcError, match=r"ny\*nz <= "):
        native.NativeSim3D(projection="auto", **kw)
    sim = native.NativeSim3D(projection="chunked", **kw)
    assert sim.projection_path() == CHUNKED
    sim.reset(np.array([9], dtype=np.uint64))
    d0 = max_div([x[0] for x in sim.get_fields()], shape, DOM)
    assert sim.step(np.random.default_rng(4).uniform(-1, 1, (1, 8, 8)).astype(np.float32))
    d1 = max_div([x[0] for x in sim.get_fields()], shape, DOM)
    print("max |div| after reset / step", d0, d1)
    assert np.isfinite(sim.get_nusselt()).all() and d0 < 4 * pencil_div_32[0] and d1 < 4 * pencil_div_32[1]


@pytest.mark.parametrize("value", [-1, 3])
def test_bad_projection_is_refused_before_touching_the_device(native, value):
    cfg, h = native.default_config(), C.c_void_p()
    cfg.dim, cfg.ny, cfg.projection = 3, 32, value
    assert native.load_library().rbc_create(C.byref(cfg), C.byref(h)) == native.RBC_ERR_INVALID and not h.value
    assert "projection" in native.load_library().rbc_last_error().decode()

"""GPU parity, 3D grids beyond the LDS slab: the row / pencil pressure projection (k3p_div_fftx, k3p_yz_solve,
k3p_ifftx_correct) against the float64 3D CPU oracle.  Every float64 grid here except the forced ones
has a horizontal slab the slab-FFT workgroup cannot hold, so it runs the pencil path by itself."""
import numpy as np
import pytest

from test_gpu_parity3d import DOMAIN, SHAPE, native, o3, rel_l2  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DOM = (2.0, 4 * np.pi, 5 * np.pi)


def max_div(fields, shape, dom):
    _, u, v, w = fields
    dz, dy, dx = (dom[q] / shape[q] for q in range(3))
    return float(np.abs((np.roll(u, -1, 2) - u) / dx + (np.roll(v, -1, 1) - v) / dy + (w[1:] - w[:-1]) / dz).max())


def reset_and_step(native, o3, shape, dom, seed, **kw):
    """test_fast_fft_sizes' sequence: random reset on the oracle, the same fields onto the GPU (whose reset projects them once more),
    one actuated env-step on both.  Returns the GPU and the oracle fields after the reset and after the step, and both sims."""
    o = o3.Oracle3D(ra=8000.0, shape=shape, domain=dom, kick=0.1, dt_control=0.02)
    o.reset_random(seed)
    sim = native.NativeSim3D(batch=1, shape=shape, domain=dom, ra=8000.0, dt_control=0.02, **kw)
    sim.reset_from_arrays(*[x[None] for x in o.fields()])
    g0, o0 = [x[0] for x in sim.get_fields()], o.fields()
    act = np.random.default_rng(4).uniform(-1, 1, (1, 8, 8)).astype(np.float32)
    assert sim.step(act) and o.step(act[0])
    return g0, o0, [x[0] for x in sim.get_fields()], o.fields(), sim, o


@pytest.mark.parametrize("shape", [(8, 64, 96),      # 8 x 8 and 8 x 12: register-blocked transforms both ways
                                   (8, 60, 100),     # generic two-factor transforms both ways
                                   (9, 81, 75)])     # odd nz, ny, nx: unpaired last row, no Nyquist mode
def test_pencil_matches_oracle(native, o3, shape):
    g0, o0, g1, o1, _, _ = reset_and_step(native, o3, shape, DOM, 9)
    for x, y in zip(g0, o0):
        assert np.abs(x - y).max() < 1e-13
    errs = [rel_l2(x, y) for x, y in zip(g1, o1)]
    divs = (max_div(g0, shape, DOM), max_div(g1, shape, DOM))
    print(shape, "rel-L2 after the step", errs, "max |div| after reset / step", divs)
    assert max(errs) < 1e-11
    assert max(divs) < 1e-13


@pytest.mark.parametrize("shape", [SHAPE, (15,) + SHAPE[1:]])
def test_pencil_forced_on_a_slab_grid(native, o3, monkeypatch, shape):
    """RBC_3D_PENCIL=1 on a grid the slab kernels run too (and on odd nz, which they run unpacked)"""
    monkeypatch.setenv("RBC_3D_PENCIL", "1")
    _, _, g1, o1, _, _ = reset_and_step(native, o3, shape, DOMAIN, 9)
    assert max(rel_l2(x, y) for x, y in zip(g1, o1)) < 1e-11
    assert max_div(g1, shape, DOMAIN) < 1e-13


def test_pencil_float32(native, o3):
    """128 x 96 planes in float32, at the tolerances test_float32_3d_within_stated_tolerances_of_the_float64_oracle states:
    b 1e-6 rel-L2, u, v, w 1e-4, Nusselt number 1e-5, divergence at float32 round-off"""
    shape = (8, 96, 128)
    _, _, g1, o1, sim, o = reset_and_step(native, o3, shape, DOM, 9, precision="f32")
    errs = [rel_l2(x, y) for x, y in zip(g1, o1)]
    assert errs[0] < 1e-6 and max(errs[1:]) < 1e-4, errs
    assert abs(sim.get_nusselt()[0] - o.nusselt()) < 1e-5 * abs(o.nusselt())
    assert max_div(g1, shape, DOM) < 2e-5 * np.abs(g1[1]).max() / (DOM[2] / shape[2])


def test_pencil_env_groups_and_masked_reset(native):
    """B = 9 runs as two env groups: every env bitwise what a batch of one gives for its seed, and a masked reset of env 0
    leaves the others alone"""
    shape, B = (8, 64, 96), 9
    seeds = np.arange(B, dtype=np.uint64) + 5
    act = np.random.default_rng(2).uniform(-1, 1, (B, 8, 8)).astype(np.float32)
    sim = native.NativeSim3D(batch=B, shape=shape, domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1)
    one = native.NativeSim3D(batch=1, shape=shape, domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1)
    sim.reset(seeds)
    assert sim.step(act)
    f = sim.get_fields()
    for e in range(B):
        one.reset(seeds[e:e + 1])
        assert one.step(act[e:e + 1])
        for x, y in zip(f, one.get_fields()):
            assert np.array_equal(x[e], y[0]), e
    sim.reset(seeds + 100, mask=[1] + [0] * (B - 1))
    for x, y in zip(f, sim.get_fields()):
        assert np.array_equal(x[1:], y[1:]) and not np.array_equal(x[0], y[0])


def test_pencil_bound_is_an_error(native):
    """a (y, z) plane beyond k3p_yz_solve's LDS: refused at creation with the bound in the message, and the process goes on"""
    with pytest.raises(native.RbcError, match=r"ny\*nz <= "):
        native.NativeSim3D(batch=1, shape=(64, 128, 128))
    sim = native.NativeSim3D(batch=1, shape=SHAPE, domain=DOMAIN)
    sim.reset(np.array([1], dtype=np.uint64))
    assert np.isfinite(sim.get_nusselt()).all()

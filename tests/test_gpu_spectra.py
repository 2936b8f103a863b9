"""GPU: rbc_get_spectra (csrc/rbc_spectra.hpp) against numpy in float64 on the arrays get_fields() returns from
the same handle: np.fft.rfft(f, axis) / n, the one-sided weights, w[:, :-1].

Tolerance: a DFT with twiddles good to a few ulp has coefficient error <= ~(n + 3) 2^-53 mean|f|; squaring and averaging the rows gives
|gpu - numpy| <= 2 (4 n + n_other + 16) 2^-53 sqrt(<f^2>_k <g^2>_k), n the transformed and n_other the averaged length, f = g for
the power spectra and (f, g) = (b, w) for the co- and quadrature spectrum.  Every mode of these broadband fields carries more than
10^6 times that, so a wrong mode index, weight, row or Nyquist case misses by O(1)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DOM = (2.0, 4 * np.pi, 5 * np.pi)          # tests/test_gpu_flowstats.py


@pytest.fixture(scope="module")
def native():
    from rbc_gym import _native
    return _native


def make(native, dim, shape, precision, B):
    if dim == 3:
        return native.NativeSim3D(batch=B, shape=shape, domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1, precision=precision)
    kw = {(40, 100): dict(heaters=7, heater_limit=0.6, obs_nz=5, obs_nx=25, dt_control=0.08)}.get(shape, dict(dt_control=0.09))
    return native.NativeSim(batch=B, nx=shape[1], nz=shape[0], random_kick=0.05, precision=native.PRECISIONS[precision], **kw)


def numpy_spectra(fields, axis):
    """-> ref, bound (B, 6, nz, n//2 + 1) along `axis` (-1: x, -2: y) of the (B, nz, ny, nx) fields"""
    b, u, v, w = fields
    n, other = b.shape[axis], b.shape[-3 - axis]
    c = np.full(n // 2 + 1, 2.0)
    c[0] = 1.0
    if n % 2 == 0:
        c[-1] = 1.0
    F = [np.moveaxis(np.fft.rfft(f, axis=axis) / n, axis, -1) for f in (b, u, v, w)]          # (B, nz, other, modes)
    cross = F[0] * np.conj(F[3])
    ref = np.stack([(np.abs(F[0]) ** 2).mean(2), (np.abs(F[1]) ** 2).mean(2), (np.abs(F[2]) ** 2).mean(2), (np.abs(F[3]) ** 2).mean(2),
                    cross.real.mean(2), cross.imag.mean(2)], axis=1) * c
    ms = [(f ** 2).mean((2, 3)) for f in (b, u, v, w)]
    bw = np.sqrt(ms[0] * ms[3])
    bound = 2 * (4 * n + other + 16) * 2.0 ** -53 * np.stack([ms[0], ms[1], ms[2], ms[3], bw, bw], axis=1)[..., None]
    return ref, np.broadcast_to(bound, ref.shape)


def check(sim, dim):
    px, py = sim.get_spectra()
    f = sim.get_fields()
    if dim == 2:
        assert py is None and not px[:, 2].any()              # channel 2: exact zeros
        b, u, w = (x[:, :, None, :] for x in f)
        f = (b, u, np.zeros_like(u), w)
    f = (f[0], f[1], f[2], f[3][:, :-1])
    prof = sim.get_flowstats()[0]
    for name, got, axis in (("x", px, -1), ("y", py, -2))[:dim - 1]:
        ref, bound = numpy_spectra(f, axis)
        err = np.abs(got - ref)
        pars = np.abs(got.sum(-1)[:, :5] - prof[:, [5, 1, 2, 3, 4]])
        print(f"p{name}: max |gpu - numpy| / bound per channel:", [float((err[:, ch] / np.maximum(bound[:, ch], 1e-300)).max()) for ch in range(6)],
              "Parseval:", [float((pars[:, ch] / np.maximum(bound[:, ch, :, 0], 1e-300)).max()) for ch in range(5)])
        assert got.shape == ref.shape and (err <= bound).all()
        assert (pars <= bound[:, :5, :, 0]).all()
    return px, py


CASES = [(2, (64, 96), "f64", 2),          # resident layout, 8 * 12 lines
         (2, (64, 96), "f32", 3),          # packed pairs, odd batch
         (2, (40, 100), "f64", 2),         # streaming, ny = 1, generic two-factor
         (3, (8, 16, 32), "f64", 2),       # generic y lines, register-blocked x lines, even sizes with a Nyquist mode
         (3, (8, 64, 96), "f64", 1),       # register-blocked both ways, several row and column blocks
         (3, (9, 81, 75), "f64", 1),       # odd nz, ny, nx: no Nyquist mode, odd env_stride
         (3, (9, 81, 75), "f32", 1)]


@pytest.mark.parametrize("dim,shape,precision,B", CASES, ids=[f"{d}d-{'x'.join(map(str, s))}-{p}" for d, s, p, _ in CASES])
def test_spectra_match_numpy(native, dim, shape, precision, B):
    """after a random reset and again after one actuated env-step (the streaming path's other state buffer)"""
    sim = make(native, dim, shape, precision, B)
    sim.reset(np.arange(B, dtype=np.uint64) + 3)
    p0 = check(sim, dim)[0]
    nact = (B, sim.heaters) if dim == 2 else (B, sim.heaters, sim.heaters)
    assert sim.step(np.random.default_rng(4).uniform(-1, 1, nact).astype(np.float32))
    assert not np.array_equal(p0, check(sim, dim)[0])
    sim.close()


@pytest.mark.parametrize("dim,shape,precision", [(2, (64, 96), "f64"), (3, (9, 81, 75), "f64"), (3, (9, 81, 75), "f32")])
def test_env_is_bitwise_independent_of_the_batch(native, dim, shape, precision):
    B = 5
    seeds = np.arange(B, dtype=np.uint64) + 11
    sim, one = make(native, dim, shape, precision, B), make(native, dim, shape, precision, 1)
    sim.reset(seeds)
    px, py = sim.get_spectra()
    for e in range(B):
        one.reset(seeds[e:e + 1])
        x1, y1 = one.get_spectra()
        assert np.array_equal(px[e], x1[0]) and (dim == 2 or np.array_equal(py[e], y1[0])), e
    sim.close(), one.close()


@pytest.mark.parametrize("field", [0, 1])    # b: the NaN stays one cell; u: the projection of the reset spreads it over the env's velocities
def test_nan_pairs(native, field):
    sim = make(native, 3, (8, 16, 32), "f64", 3)
    sim.reset(np.arange(3, dtype=np.uint64) + 7)
    f = [x.copy() for x in sim.get_fields()]
    sim.reset_from_arrays(*f)                             # the clean run: the same arrays through the same reset
    clean = sim.get_spectra()
    f[field][1, 3, 4, 5] = np.nan
    sim.reset_from_arrays(*f)
    want = np.zeros((3, 6, 8), bool)
    if field == 0:
        want[1, [0, 3, 4, 5], 3] = True                   # b and w of level 3 travel as one line
    else:   # u, v of every level and w of every interior face are NaN (tests/test_gpu_flowstats.py); face 0 is the wall, so level 0 keeps b, w
        want[1, 1:3] = True
        want[1, [0, 3, 4, 5], 1:] = True
    for got, ref in zip(sim.get_spectra(), clean):
        assert np.array_equal(np.isnan(got), np.broadcast_to(want[..., None], got.shape))      # at every mode, nowhere else
        assert np.array_equal(got[~np.isnan(got)], ref[~np.isnan(got)])                        # ... and nothing else changes by a bit
    sim.close()


def test_env_layer_views_and_errors(native):
    import rbc_gym  # noqa: F401
    from rbc_gym._gym import gym
    from rbc_gym.wrappers import VectorRBCNormalizeObservation
    ID3 = "rbc_gym/RayleighBenardConvection3D-v0"
    kw = dict(num_envs=3, state_shape=(8, 16, 32), heater_duration=0.0625, rayleigh_number=5000)
    raw, two = gym.make_vec(ID3, **kw), gym.make_vec(ID3, devices=[0, 0], **kw)
    fused = VectorRBCNormalizeObservation(gym.make_vec(ID3, **kw), heater_limit=0.9, u_limit=None, clip=True)
    single = gym.make(ID3, state_shape=(8, 16, 32), heater_duration=0.0625, rayleigh_number=5000)
    act = np.random.default_rng(1).uniform(-1, 1, (3, 8, 8)).astype(np.float32)
    for env in (raw, two, fused):
        env.reset(seed=9)
        env.step(act)
    single.reset(seed=10)
    single.step(act[1])
    want, s = raw.unwrapped.power_spectra(), single.unwrapped.power_spectra()
    assert want["x"].shape == (3, 6, 8, 17) and want["y"].shape == (3, 6, 8, 9) and want["channels"] == ("b", "u", "v", "w", "bw_co", "bw_quad")
    assert np.allclose(want["kx"], 2 * np.pi * np.arange(17) / raw.unwrapped.sim.cfg.lx) and len(want["ky"]) == 9
    for other in (two.unwrapped.power_spectra(), fused.unwrapped.power_spectra()):
        assert all(np.array_equal(want[k], other[k]) for k in ("x", "y", "kx", "ky"))
    assert all(np.array_equal(s[k], want[k][1]) for k in ("x", "y"))
    for env in (raw, two, fused, single):
        env.close()

    sim = make(native, 3, (8, 16, 32), "f32", 2)
    assert sim.lib.rbc_dev_spectra(sim.h, 0) is None and sim.lib.rbc_dev_spectra(sim.h, 2) is None
    assert b"which must be 0" in sim.lib.rbc_last_error()      # a pointer-returning entry has no code to return
    with pytest.raises(native.RbcError) as ei:             # before the first reset
        sim.get_spectra()
    assert ei.value.code == native.RBC_ERR_NOT_INITIALIZED
    sim.reset(np.array([1, 2], dtype=np.uint64))
    px, py = sim.get_spectra()
    views = sim.spectra_views()
    sim.synchronize()
    assert np.array_equal(views["x"].cpu().numpy(), px) and np.array_equal(views["y"].cpu().numpy(), py)
    del views
    sim.close()

    flat = make(native, 2, (64, 96), "f64", 1)
    flat.reset(np.array([5], dtype=np.uint64))
    buf = np.empty((1, 6, 64, 49))
    assert flat.lib.rbc_get_spectra(flat.h, None, buf.ctypes.data_as(C.POINTER(C.c_double))) == native.RBC_ERR_INVALID
    assert set(flat.spectra_views()) == {"x"} and flat.lib.rbc_dev_spectra(flat.h, 1) is None
    flat.close()

"""GPU: rbc_get_flowstats (csrc/rbc_flowstats.hpp) against plain numpy in float64 on the arrays get_fields()
returns from the same handle: tests/profile_pins.py::row_moments_batch for the 2D moments, the same expressions with v for 3D.

Moments: |gpu - numpy| <= n_h 2^-52 mean|terms of the level|, the float64 summation bound for ANY order of addition (each side is
within (n_h - 1) 2^-53 sum|terms| of the exact sum; the one rounding of each division fits in the n_h - 1 -> n_h slack), NaNs in
the same places.  Extrema: equal, a maximum of float64 values is exact."""
import numpy as np
import pytest

from profile_pins import row_moments_batch

pytestmark = pytest.mark.gpu

DOM = (2.0, 4 * np.pi, 5 * np.pi)          # tests/test_gpu_pencil3d.py
EXT = ("u_max", "v_max", "w_max", "b_min", "b_max")


@pytest.fixture(scope="module")
def native():
    from rbc_gym import _native
    return _native


def numpy_flowstats(fields):
    """-> prof (B, 6, nz), ext (B, 5), bound (B, 6, nz) from get_fields() arrays: (b, u, w) of a 2D handle, (b, u, v, w) of a 3D one"""
    if len(fields) == 3:
        b, u, w = fields
        v, hz = np.zeros_like(u), (2,)
        rm = row_moments_batch(b, u, w)
        prof = np.stack([rm[:, 0], rm[:, 1], np.zeros_like(rm[:, 0]), rm[:, 2], rm[:, 3], rm[:, 4]], axis=1)
    else:
        b, u, v, w = fields
        wc, hz = w[:, :-1], (2, 3)
        prof = np.stack([b.mean(hz), (u ** 2).mean(hz), (v ** 2).mean(hz), (wc ** 2).mean(hz), (b * wc).mean(hz), (b ** 2).mean(hz)], axis=1)
    wc = w[:, :-1]
    n_h = int(np.prod(b.shape[2:]))
    bound = n_h * 2.0 ** -52 * np.stack([np.abs(t).mean(hz) for t in (b, u ** 2, v ** 2, wc ** 2, b * wc, b ** 2)], axis=1)
    flat = [x.reshape(len(x), -1) for x in (u, v, w, b)]
    ext = np.stack([np.abs(flat[0]).max(1), np.abs(flat[1]).max(1), np.abs(flat[2]).max(1), flat[3].min(1), flat[3].max(1)], axis=1)
    return prof, ext, bound


def check(sim):
    prof, ext = sim.get_flowstats()
    rp, re, bound = numpy_flowstats(sim.get_fields())
    err = np.abs(prof - rp)
    print("max |gpu - numpy| / bound per moment:", [float(np.nanmax(err[:, m] / np.maximum(bound[:, m], 1e-300))) for m in range(6)])
    assert np.array_equal(np.isnan(prof), np.isnan(rp))
    assert (err[~np.isnan(rp)] <= bound[~np.isnan(rp)]).all()
    assert np.array_equal(ext, re, equal_nan=True)
    return prof, ext


def make(native, dim, shape, precision, B):
    if dim == 3:
        return native.NativeSim3D(batch=B, shape=shape, domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1, precision=precision)
    # the streaming grids as tests/test_gpu_stream2d.py configures them
    kw = {(40, 100): dict(heaters=7, heater_limit=0.6, obs_nz=5, obs_nx=25, dt_control=0.08),
          (27, 72): dict(heaters=5, heater_limit=0.5, obs_nz=9, obs_nx=36, dt_control=0.07, ra=5e3, lz=1.5, min_b=0.5, delta_b=2.0)}.get(shape, dict(dt_control=0.09))
    return native.NativeSim(batch=B, nx=shape[1], nz=shape[0], random_kick=0.05, precision=native.PRECISIONS[precision], **kw)


CASES = [(2, (64, 96), "f64", 2),          # resident 2D
         (2, (64, 96), "f32", 3),          # packed pairs with an odd batch; `fields` is float64 with nz + 1 rows of w
         (2, (40, 100), "f64", 2),         # streaming 2D: ny = 1, a v block of zeros
         (2, (27, 72), "f64", 2),          # ... odd nz
         (3, (8, 16, 32), "f64", 2),       # small levels: one wave per level
         (3, (9, 81, 75), "f64", 1),       # planes of 6075 cells: four waves per level, every second level misaligned
         (3, (9, 81, 75), "f32", 1)]


@pytest.mark.parametrize("dim,shape,precision,B", CASES, ids=[f"{d}d-{'x'.join(map(str, s))}-{p}" for d, s, p, _ in CASES])
def test_flowstats_match_numpy(native, dim, shape, precision, B):
    """after a random reset and again after one actuated env-step (the streaming path's other state buffer)"""
    sim = make(native, dim, shape, precision, B)
    sim.reset(np.arange(B, dtype=np.uint64) + 3)
    p0, e0 = check(sim)
    nact = (B, sim.heaters) if dim == 2 else (B, sim.heaters, sim.heaters)
    assert sim.step(np.random.default_rng(4).uniform(-1, 1, nact).astype(np.float32))
    p1, e1 = check(sim)
    assert not np.array_equal(p0, p1) and (e1[:, 0] > 0).all()
    if dim == 2:
        assert not p1[:, 2].any() and not e1[:, 1].any()          # exact zeros
    sim.close()


# (9, 81, 75): env_stride = 6075 * 37 values is odd, so the five envs start at every offset within 16 bytes (two in float64, four in
# float32) and a level that is aligned in a batch of one is not at the next position
@pytest.mark.parametrize("dim,shape,precision", [(3, (8, 16, 32), "f64"), (2, (64, 96), "f64"), (3, (9, 81, 75), "f64"), (3, (9, 81, 75), "f32")])
def test_env_is_bitwise_independent_of_the_batch(native, dim, shape, precision):
    B = 5
    seeds = np.arange(B, dtype=np.uint64) + 11
    sim, one = make(native, dim, shape, precision, B), make(native, dim, shape, precision, 1)
    sim.reset(seeds)
    prof, ext = sim.get_flowstats()
    for e in range(B):
        one.reset(seeds[e:e + 1])
        p1, e1 = one.get_flowstats()
        assert np.array_equal(prof[e], p1[0]) and np.array_equal(ext[e], e1[0]), e
    sim.close(), one.close()


@pytest.mark.parametrize("field", [1, 0])    # u: the projection of the reset spreads the NaN over the env's velocities; b: it stays one cell
def test_nan_goes_where_numpy_puts_it(native, field):
    sim = make(native, 3, (8, 16, 32), "f64", 3)
    sim.reset(np.arange(3, dtype=np.uint64) + 7)
    f = [x.copy() for x in sim.get_fields()]
    sim.reset_from_arrays(*f)                             # the clean run: the same arrays through the same reset (it projects them again)
    clean_p, clean_e = sim.get_flowstats()
    f[field][1, 3, 4, 5] = np.nan
    sim.reset_from_arrays(*f)
    prof, ext = check(sim)
    m = {1: 1, 0: 0}[field]
    assert np.isnan(prof[1, m, 3]) and np.isnan(ext[1, {1: 0, 0: 3}[field]])
    if field == 1:   # a NaN potential all over env 1: u^2, v^2 of every level, w^2 and b w of every interior face, the three velocity maxima; b's stay
        assert np.isnan(prof[1, 1:3]).all() and np.isnan(prof[1, 3:5, 1:]).all() and np.isnan(ext[1, :3]).all()
        assert np.isfinite(prof[1, [0, 5]]).all() and np.isfinite(ext[1, 3:]).all()
    if field == 0:   # one cell of b: its level's b, b w, b^2 and both extrema of b, nothing else
        assert np.isnan(ext[1, 4]) and np.isnan(prof[1, [0, 4, 5], 3]).all() and np.isnan(prof[1]).sum() == 3
    # whatever is not NaN in env 1 is the clean run's; envs 0 and 2 are the clean run's bit for bit
    assert np.array_equal(prof[1][~np.isnan(prof[1])], clean_p[1][~np.isnan(prof[1])])
    assert np.array_equal(ext[1][~np.isnan(ext[1])], clean_e[1][~np.isnan(ext[1])])
    assert np.array_equal(prof[[0, 2]], clean_p[[0, 2]]) and np.array_equal(ext[[0, 2]], clean_e[[0, 2]])
    sim.close()


def test_env_layer(native):
    """flow_statistics() of a batched 3D env under active observation normalisation = the unnormalised numbers = the sharded env's
    (both shards on device 0) = the single env's"""
    import rbc_gym  # noqa: F401
    from rbc_gym._gym import gym
    from rbc_gym.wrappers import VectorRBCNormalizeObservation
    ID3 = "rbc_gym/RayleighBenardConvection3D-v0"
    kw = dict(num_envs=3, state_shape=(8, 16, 32), heater_duration=0.0625, rayleigh_number=5000)
    raw, two = gym.make_vec(ID3, **kw), gym.make_vec(ID3, devices=[0, 0], **kw)
    fused = VectorRBCNormalizeObservation(gym.make_vec(ID3, **kw), heater_limit=0.9, u_limit=None, clip=True)
    assert fused.fused
    act = np.random.default_rng(1).uniform(-1, 1, (3, 8, 8)).astype(np.float32)
    for env in (raw, two, fused):
        env.reset(seed=9)
        env.step(act)
    want = raw.unwrapped.flow_statistics()
    prof, ext = raw.unwrapped.sim.get_flowstats()
    assert set(want) == {"profiles", "kinetic_energy", *EXT} and want["profiles"].shape == (3, 6, 8)
    assert np.array_equal(want["kinetic_energy"], 0.5 * (prof[:, 1] + prof[:, 2] + prof[:, 3]).mean(1)) and want["kinetic_energy"].min() > 0
    for other in (two.unwrapped.flow_statistics(), fused.unwrapped.flow_statistics()):
        assert all(np.array_equal(want[k], other[k]) for k in want)
    single = gym.make(ID3, state_shape=(8, 16, 32), heater_duration=0.0625, rayleigh_number=5000)
    single.reset(seed=10)
    single.step(act[1])
    s = single.unwrapped.flow_statistics()
    assert s["profiles"].shape == (6, 8) and all(np.array_equal(s[k], want[k][1]) for k in want)
    for env in (raw, two, fused, single):
        env.close()


def test_views_and_error_codes(native):
    sim = make(native, 3, (8, 16, 32), "f32", 2)
    assert sim.lib.rbc_dev_flowstats(sim.h, 0) is None and sim.lib.rbc_dev_flowstats(sim.h, 2) is None
    assert b"which must be 0" in sim.lib.rbc_last_error()      # the RBC_ERR_INVALID refusal; a pointer-returning entry has no code to return
    with pytest.raises(native.RbcError) as ei:             # before the first reset
        sim.get_flowstats()
    assert ei.value.code == native.RBC_ERR_NOT_INITIALIZED
    sim.reset(np.array([1, 2], dtype=np.uint64))
    prof, ext = sim.get_flowstats()
    views = sim.flowstats_views()
    sim.synchronize()
    assert np.array_equal(views["profiles"].cpu().numpy(), prof) and np.array_equal(views["extrema"].cpu().numpy(), ext)
    del views
    sim.close()

"""GPU: rbc_get_dissipation (csrc/rbc_dissipation.hpp) against the same formulas in numpy, float64, on the
arrays get_fields() returns from the same handle.

cells, faces: |gpu - numpy| <= (n_h + 16) 2^-52 mean|terms of that level|: each side is within (n_h - 1) 2^-53 sum|terms| of the exact
sum for any order of addition, and within ~8 roundings per term (the scaling by 1/h, the square or product, up to three additions
inside a term); the subtractions are identical IEEE operations on identical inputs.  tot: the same form with nz + 1 + 16, against the
fold of numpy's own profiles.  NaNs in the same places."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_flowstats import make

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from rbc_gym import _native
    return _native


def fold(cells, faces):
    """tot (B, 4): volume means, faces 0 and nz with weight 1/2"""
    wk = np.ones(faces.shape[2])
    wk[[0, -1]] = 0.5
    C_, F = cells.sum(2), (faces * wk).sum(2)
    return np.stack([C_[:, 0] + F[:, 0], C_[:, 1], C_[:, 2] + F[:, 1] + F[:, 3], C_[:, 3] + F[:, 2] + F[:, 4]], axis=1) / cells.shape[2]


def numpy_dissipation(cfg, fields, wall_b=None):
    """-> cells (B, 4, nz), faces (B, 5, nz + 1) and mean|terms| of both, from get_fields() arrays of a 2D (b, u, w) or 3D handle"""
    d3 = len(fields) == 4
    b, u, v, w = fields if d3 else (fields[0][:, :, None], fields[1][:, :, None], np.zeros_like(fields[0])[:, :, None], fields[2][:, :, None])
    B, nz, ny, nx = b.shape
    dx, dy, dz = cfg.lx / nx, (cfg.ly / ny if d3 else 1.0), cfg.lz / nz
    wall = np.full((B, ny, nx), cfg.min_b + cfg.delta_b) if wall_b is None else np.reshape(wall_b, (B, ny, nx))
    ddx = lambda f: (f - np.roll(f, 1, -1)) / dx
    ddy = lambda f: (f - np.roll(f, 1, -2)) / dy if d3 else np.zeros_like(f)
    ddz = lambda f, lo, hi: np.concatenate([lo / dz, (f[:, 1:] - f[:, :-1]) / dz, hi / dz], axis=1)
    dzb = ddz(b, 2 * (b[:, :1] - wall[:, None]), 2 * (cfg.min_b - b[:, -1:]))
    dzu, dzv = ddz(u, 2 * u[:, :1], -2 * u[:, -1:]), ddz(v, 2 * v[:, :1], -2 * v[:, -1:])
    dxu, dyv, dzw = (np.roll(u, -1, -1) - u) / dx, ((np.roll(v, -1, -2) - v) / dy if d3 else 0 * v), (w[:, 1:] - w[:, :-1]) / dz
    cterms = [ddx(b) ** 2 + ddy(b) ** 2, dxu ** 2 + dyv ** 2 + dzw ** 2, ddy(u) ** 2 + ddx(v) ** 2, ddy(u) * ddx(v)]
    fterms = [dzb ** 2, dzu ** 2 + ddx(w) ** 2, dzu * ddx(w), dzv ** 2 + ddy(w) ** 2, dzv * ddy(w)]
    mean = lambda ts: np.stack([t.mean((2, 3)) for t in ts], axis=1)
    return mean(cterms), mean(fterms), mean([np.abs(t) for t in cterms]), mean([np.abs(t) for t in fterms])


def check(sim, wall_b=None):
    got = sim.get_dissipation(wall_b)
    rc, rf, ac, af = numpy_dissipation(sim.cfg, sim.get_fields(), wall_b)
    n_h = sim.nx * getattr(sim, "ny", 1)
    for name, g, ref, a, n in (("cells", got[0], rc, ac, n_h), ("faces", got[1], rf, af, n_h), ("tot", got[2], fold(rc, rf), fold(ac, af), sim.nz + 1)):
        bound, err, ok = (n + 16) * 2.0 ** -52 * a, np.abs(g - ref), ~np.isnan(ref)
        print(f"max |gpu - numpy| / bound, {name}:", [float(np.nanmax(err[:, m] / np.maximum(bound[:, m], 1e-300))) for m in range(g.shape[1])])
        assert g.shape == ref.shape and np.array_equal(np.isnan(g), np.isnan(ref)), name
        assert (err[ok] <= bound[ok]).all(), name
    return got


CASES = [(2, (64, 96), "f64", 2),          # resident 2D: one wave per (env, chunk)
         (2, (64, 96), "f32", 3),          # packed pairs, odd batch
         (2, (27, 72), "f64", 2),          # streaming 2D, odd nz: a last chunk of three levels and the top face
         (2, (40, 100), "f64", 2),
         (3, (8, 16, 16), "f64", 2),       # 256 cells: the largest one-wave level, with its y terms
         (3, (8, 16, 32), "f64", 2),       # eight waves, one strip, one column per thread
         (3, (9, 81, 75), "f64", 1),       # odd everything, misaligned levels: three strips of 27 rows, chunks of 4, 4, 1 levels
         (3, (9, 81, 75), "f32", 1),
         (3, (9, 45, 46), "f64", 1)]       # 2070 cells, the smallest plane over the 2048-cell tile: strips of 23 and 22 rows (the seam
                                           # between rows 22 and 23 and the periodic one, each through a halo row), chunk seams at 4 and 8


@pytest.mark.parametrize("dim,shape,precision,B", CASES, ids=[f"{d}d-{'x'.join(map(str, s))}-{p}" for d, s, p, _ in CASES])
def test_dissipation_matches_numpy(native, dim, shape, precision, B):
    """after a random reset and again after one actuated env-step (the streaming path's other state buffer); uniform and random plate"""
    sim = make(native, dim, shape, precision, B)
    sim.reset(np.arange(B, dtype=np.uint64) + 3)
    wall = sim.cfg.min_b + sim.cfg.delta_b + np.random.default_rng(5).uniform(-0.5, 0.5, (B,) + tuple(shape[1:]))
    first = check(sim)
    nact = (B, sim.heaters) if dim == 2 else (B, sim.heaters, sim.heaters)
    assert sim.step(np.random.default_rng(4).uniform(-1, 1, nact).astype(np.float32))
    for got in (check(sim), check(sim, wall)):
        assert not np.array_equal(got[0], first[0]) and (got[2][:, :3] > 0).all()
        if dim == 2:
            assert not got[0][:, 2:].any() and not got[1][:, 3:].any()          # exact zeros
    sim.close()


@pytest.mark.parametrize("dim,shape", [(3, (8, 16, 32)), (2, (64, 96))])
def test_conduction_state(native, dim, shape):
    """b linear in z, no flow: |grad b|^2 = (delta_b / lz)^2 and Nu = 1 to 64 nz 2^-53 (b <= 2 carries an error of up to 2^-52 into a
    difference of delta_b / (2 nz)), everything else exactly 0"""
    from rbc_gym.envs._common import dissipation_rates_dict
    sim = make(native, dim, shape, "f64", 2)
    c, nz = sim.cfg, shape[0]
    b = np.empty((2,) + tuple(shape))
    b[:] = (c.min_b + c.delta_b * (1 - (np.arange(nz) + 0.5) / nz)).reshape((nz,) + (1,) * (len(shape) - 1))
    zero, w0 = np.zeros_like(b), np.zeros((2, nz + 1) + tuple(shape[1:]))
    sim.reset_from_arrays(*((b, zero, w0) if dim == 2 else (b, zero, zero, w0)))
    cells, faces, tot = sim.get_dissipation()
    assert not cells.any() and not faces[:, 1:].any() and not tot[:, 1:].any()
    want, tol = (c.delta_b / c.lz) ** 2, 64 * nz * 2.0 ** -53
    assert np.abs(faces[:, 0] / want - 1).max() <= tol and np.abs(tot[:, 0] / want - 1).max() <= tol
    assert np.abs(dissipation_rates_dict(sim)["nusselt_thermal"] - 1).max() <= tol
    sim.close()


# (9, 81, 75): env_stride is odd, so the five envs start at every offset within 16 bytes (tests/test_gpu_flowstats.py)
@pytest.mark.parametrize("dim,shape,precision", [(2, (64, 96), "f64"), (3, (9, 81, 75), "f64"), (3, (9, 81, 75), "f32")])
def test_env_is_bitwise_independent_of_the_batch(native, dim, shape, precision):
    B = 5
    seeds = np.arange(B, dtype=np.uint64) + 11
    sim, one = make(native, dim, shape, precision, B), make(native, dim, shape, precision, 1)
    sim.reset(seeds)
    got = sim.get_dissipation()
    for e in range(B):
        one.reset(seeds[e:e + 1])
        assert all(np.array_equal(g[e], o[0]) for g, o in zip(got, one.get_dissipation())), e
    sim.close(), one.close()


def test_one_nan(native):
    """one cell of b in env 1 of three: NaNs where numpy has them, every other bit the clean run's"""
    sim = make(native, 3, (8, 16, 32), "f64", 3)
    sim.reset(np.arange(3, dtype=np.uint64) + 7)
    f = [x.copy() for x in sim.get_fields()]
    sim.reset_from_arrays(*f)                             # the clean run: the same arrays through the same reset
    clean = sim.get_dissipation()
    f[0][1, 3, 4, 5] = np.nan
    sim.reset_from_arrays(*f)
    for g, c in zip(check(sim), clean):
        assert np.isnan(g[1]).any() and np.array_equal(g[1][~np.isnan(g[1])], c[1][~np.isnan(g[1])]) and np.array_equal(g[[0, 2]], c[[0, 2]])
    sim.close()


def test_views_error_codes_and_env_layer(native):
    sim = make(native, 3, (8, 16, 32), "f32", 2)
    assert sim.lib.rbc_dev_dissipation(sim.h, 0) is None and sim.lib.rbc_dev_dissipation(sim.h, 3) is None
    assert b"which must be 0" in sim.lib.rbc_last_error()
    with pytest.raises(native.RbcError) as ei:             # before the first reset
        sim.get_dissipation()
    assert ei.value.code == native.RBC_ERR_NOT_INITIALIZED
    sim.reset(np.array([1, 2], dtype=np.uint64))
    host, views = sim.get_dissipation(), sim.dissipation_views()
    sim.synchronize()
    assert all(np.array_equal(views[k].cpu().numpy(), h) for k, h in zip(("cells", "faces", "tot"), host))
    del views
    sim.close()
    # batched = sharded (both shards on device 0) = single, with per-env Rayleigh numbers
    import rbc_gym  # noqa: F401
    from rbc_gym._gym import gym
    ID3 = "rbc_gym/RayleighBenardConvection3D-v0"
    kw = dict(num_envs=3, state_shape=(8, 16, 32), heater_duration=0.0625, rayleigh_number=[4000.0, 5000.0, 6000.0])
    raw, two = gym.make_vec(ID3, **kw), gym.make_vec(ID3, devices=[0, 0], **kw)
    single = gym.make(ID3, state_shape=(8, 16, 32), heater_duration=0.0625, rayleigh_number=5000)
    act = np.random.default_rng(1).uniform(-1, 1, (3, 8, 8)).astype(np.float32)
    for env in (raw, two):
        env.reset(seed=9)
        env.step(act)
    single.reset(seed=10)
    single.step(act[1])
    want, other, s = raw.unwrapped.dissipation_rates(), two.unwrapped.dissipation_rates(), single.unwrapped.dissipation_rates()
    assert set(want) == {"cells", "faces", "thermal_dissipation", "kinetic_dissipation", "enstrophy", "nusselt_thermal", "nusselt_viscous"}
    tot = raw.unwrapped.sim.get_dissipation()[2]
    assert np.array_equal(want["kinetic_dissipation"], np.sqrt(0.7 / np.array(kw["rayleigh_number"])) * (tot[:, 1] + tot[:, 2]))
    assert want["cells"].shape == (3, 4, 8) and s["faces"].shape == (5, 9) and want["enstrophy"].min() > 0
    assert all(np.array_equal(want[k], other[k]) and np.array_equal(want[k][1], s[k]) for k in want)
    for env in (raw, two, single):
        env.close()

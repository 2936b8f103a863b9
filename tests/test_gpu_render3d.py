"""GPU: render() of the 3D envs -- the device's volume ray-caster (rbc3d_render.hpp) against the float64 restatement of the
picture's definition (tests/render3d_ref.py), against the closed form for a uniform field, and through the env layer."""
import ctypes as C

import numpy as np
import pytest

import render3d_ref

pytestmark = pytest.mark.gpu

DOMAIN = (2.0, 4 * np.pi, 4 * np.pi)
S = np.linspace(0.0, 1.0, 256)
# a table whose every channel, alpha included, varies: a nearest-entry lookup or a swapped channel shows
LUT = np.stack([S, 1 - S, 0.5 + 0.5 * np.cos(3 * np.pi * S), 0.15 + 0.4 * (2 * S - 1) ** 2], axis=1).astype(np.float32)


def structured_fields(shape):
    """3 envs: the linear profile plus smooth modes of other wavenumbers per axis and env, leaving clim = (1, 2) on both sides;
    env 2 carries a block of NaN"""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    b = np.stack([2 - z + 0.8 * np.sin(2 * np.pi * (1 + e % 2) * x + e) * np.cos(2 * np.pi * (2 - e % 2) * y) * np.sin(np.pi * (1 + e) * z + 0.3)
                  + 0.6 * np.cos(2 * np.pi * (x + 2 * y) + 0.7 * e) for e in range(3)])
    b[2, nz // 2:nz // 2 + 3, 2:6, 3:8] = np.nan
    return b


@pytest.fixture(scope="module")
def sims():
    """one handle of 3 envs per (grid, precision), holding structured_fields; made on first use"""
    from rbc_gym import _native
    made = {}

    def get(shape, precision):
        if (shape, precision) not in made:
            sim = _native.NativeSim3D(batch=3, shape=shape, domain=DOMAIN, precision=precision)
            zero = np.zeros((3,) + shape)
            sim.reset_from_arrays(structured_fields(shape), zero, zero, np.zeros((3, shape[0] + 1) + shape[1:]))
            made[shape, precision] = (sim, sim.get_fields()[0])         # what the handle holds: float32-rounded for "f32"
        return made[shape, precision]
    yield get
    for sim, _ in made.values():
        sim.close()


@pytest.mark.parametrize("size", [(40, 24), (97, 61)])
@pytest.mark.parametrize("view_from", [(1, 1, 1), (-2, 1, -0.5), (0, -1, 0), (0, 0, 1)])
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(8, 12, 16), (16, 32, 32)])
def test_structured_field_matches_the_float64_definition(sims, shape, precision, view_from, size):
    """Every byte within 1 level.  Derived, not measured: the picture is a continuous function of the field and the pixel (partial
    last segment), float32 accumulation over at most a few hundred samples is orders of magnitude below half a level, the permitted
    early exit at A >= 0.999 drops less than 0.26 of a level, the rest is the final rounding."""
    sim, held = sims(shape, precision)
    got = sim.render(size=size, view_from=view_from, lut=LUT, first_env=1, n_envs=2)
    assert got.shape == (2, size[1], size[0], 3) and got.dtype == np.uint8
    for k, e in enumerate((1, 2)):
        ref = render3d_ref.render(held[e], DOMAIN, size=size, view_from=view_from, lut=LUT)
        span = ref.reshape(-1, 3).max(0).astype(int) - ref.reshape(-1, 3).min(0)
        assert (span >= 100).all(), ("flat reference picture", span)
        err = np.abs(got[k].astype(int) - ref)
        assert err.max() <= 1, (int(err.max()), np.argwhere(err > 1)[:5])


@pytest.mark.parametrize("step", [0.0, 0.31])
def test_uniform_field_matches_the_closed_form(step):
    """constant T: A = 1 - (1 - a)^(l / unit) whatever the step (partial segment + opacity correction), colour A rgb + (1 - A) bg"""
    from rbc_gym import _native
    shape, size, view, unit, bg, temp = (8, 12, 16), (97, 61), (-2, 1, -0.5), 1.5, (0.2, 0.9, 0.4), 1.6
    sim = _native.NativeSim3D(batch=1, shape=shape, domain=DOMAIN)
    zero = np.zeros((1,) + shape)
    sim.reset_from_arrays(np.full((1,) + shape, temp), zero, zero, np.zeros((1, shape[0] + 1) + shape[1:]))
    got = sim.render(size=size, view_from=view, lut=LUT, step=step, unit=unit, bg=bg)[0]
    sim.close()
    box = (np.array(shape[::-1]) - 1) * np.array(DOMAIN[::-1]) / np.array(shape[::-1])
    _, _, t0, t1, hit = render3d_ref.rays(view, box, *size)
    x = 255 * (temp - 1.0)
    rgba = LUT[int(x)].astype(float) * (1 - (x - int(x))) + LUT[int(x) + 1].astype(float) * (x - int(x))
    A = np.where(hit, 1 - (1 - rgba[3]) ** (np.where(hit, t1 - t0, 0.0) / unit), 0.0)
    want = np.floor(255 * (A[..., None] * rgba[:3] + (1 - A)[..., None] * np.array(bg)) + 0.5)
    assert A.max() > 0.5 and (A > 0).mean() > 0.1                                  # the box is in the picture and not saturated
    assert np.abs(got.astype(int) - want).max() <= 1


def test_env_layer_and_argument_checks():
    import rbc_gym  # noqa: F401  (registers the ids)
    from rbc_gym import _native
    from rbc_gym._gym import gym
    ID3 = "rbc_gym/RayleighBenardConvection3D-v0"
    env = gym.make(ID3, render_mode="rgb_array")
    venv = gym.make_vec(ID3, num_envs=2, render_mode="rgb_array")
    env.reset(seed=11)
    venv.reset(seed=11)
    act = np.zeros((8, 8), np.float32)
    env.step(act)
    venv.step(np.stack([act, act]))
    frame = env.render()
    assert frame.shape == (608, 800, 3) and frame.dtype == np.uint8 and (frame != 255).any()
    frames = venv.render()
    assert frames.shape == (2, 608, 800, 3) and np.array_equal(frames[0], frame) and not np.array_equal(frames[1], frame)
    sim = env.unwrapped.sim
    sim.set_obs_normalization([1, -1, -1, -1], [2.9, 1, 1, 1])                     # the picture comes from the solver's state
    assert np.array_equal(env.render(), frame)
    plain = gym.make(ID3)
    assert plain.render() is None                                                 # no render mode: None (rbc3D.py:260-265)
    for kw in (dict(size=(0, 8)), dict(size=(8, -1)), dict(first_env=1), dict(n_envs=2), dict(n_envs=0), dict(view_from=(0, 0, 0)), dict(clim=(1.5, 1.5))):
        with pytest.raises(_native.RbcError) as e:
            sim.render(**kw)
        assert e.value.code == _native.RBC_ERR_INVALID and "rbc_render3" in str(e.value), kw
    fresh = _native.NativeSim3D(batch=1, shape=(8, 16, 16))
    with pytest.raises(_native.RbcError) as e:
        fresh.render(size=(16, 16))
    assert e.value.code == _native.RBC_ERR_NOT_INITIALIZED
    flat = _native.NativeSim(batch=1)                                                # a dim = 2 handle is refused
    out, p = np.zeros((8, 8, 3), np.uint8), _native.RbcRender3Params(width=8, height=8, n_envs=1)
    rc = flat.lib.rbc_render3(flat.h, C.byref(p), LUT.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == _native.RBC_ERR_INVALID and "dim=3" in flat.lib.rbc_last_error().decode()
    for s in (fresh, flat, plain, env, venv):
        s.close()

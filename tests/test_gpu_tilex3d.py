"""GPU parity of the x- and y-tiled LDS tendency kernel k3_tilex_all (3D grids wider than 64 cells): one reset
plus one actuated env-step per case against the float64 CPU oracle, the full-row tile kernel, and itself across env groups."""
import numpy as np
import pytest

from test_gpu_parity3d import native, o3, rel_l2  # noqa: F401  (fixtures)
from test_gpu_pencil3d import DOM, max_div, reset_and_step

pytestmark = pytest.mark.gpu
X_TILED = 4      # rbc_debug_tendency_path


@pytest.mark.parametrize("shape", [(8, 16, 96),      # one y tile: its halo rows are its own rows; first / last x tile wrap
                                   (8, 32, 128),     # two y tiles
                                   (12, 24, 160)])   # 32 x 8 tiles (ny % 16 != 0), three chunks of 4 levels: the middle one touches no wall
def test_tilex_matches_oracle(native, o3, shape):
    g0, o0, g1, o1, sim, _ = reset_and_step(native, o3, shape, DOM, 9)      # the bars of test_pencil_matches_oracle
    assert sim.tendency_path() == X_TILED
    for x, y in zip(g0, o0):
        assert np.abs(x - y).max() < 1e-13
    assert max(rel_l2(x, y) for x, y in zip(g1, o1)) < 1e-11
    assert max(max_div(g0, shape, DOM), max_div(g1, shape, DOM)) < 1e-13


def test_tilex_against_the_full_row_tiles(native, o3, monkeypatch):
    """8 x 8 full-row tiles by default, the x-tiled kernel with RBC_TILE_X=1: the same bodies, but two instantiations whose fma
    contraction the compiler chooses separately (measured: 2e-16), so the project's A/B bar, not bitwise equality"""
    shape = (8, 16, 64)
    _, _, a, _, sim, _ = reset_and_step(native, o3, shape, DOM, 9)
    assert sim.tendency_path() == 2
    monkeypatch.setenv("RBC_TILE_X", "1")
    _, _, b, _, sim, _ = reset_and_step(native, o3, shape, DOM, 9)
    assert sim.tendency_path() == X_TILED
    assert max(rel_l2(x, y) for x, y in zip(b, a)) < 1e-12


def test_tilex_float32(native, o3):
    """the bars test_pencil_float32 states: b 1e-6 rel-L2, u, v, w 1e-4, Nusselt number 1e-5"""
    _, _, g1, o1, sim, o = reset_and_step(native, o3, (8, 16, 96), DOM, 9, precision="f32")
    assert sim.tendency_path() == X_TILED
    errs = [rel_l2(x, y) for x, y in zip(g1, o1)]
    assert errs[0] < 1e-6 and max(errs[1:]) < 1e-4, errs
    assert abs(sim.get_nusselt()[0] - o.nusselt()) < 1e-5 * abs(o.nusselt())


def test_tilex_env_groups(native):
    """B = 9 runs as env groups: every env bitwise what a batch of one gives for its seed"""
    shape, B = (8, 16, 96), 9
    seeds = np.arange(B, dtype=np.uint64) + 5
    act = np.random.default_rng(2).uniform(-1, 1, (B, 8, 8)).astype(np.float32)
    sim = native.NativeSim3D(batch=B, shape=shape, domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1)
    one = native.NativeSim3D(batch=1, shape=shape, domain=DOM, ra=8000.0, dt_control=0.02, random_kick=0.1)
    assert sim.tendency_path() == X_TILED and one.tendency_path() == X_TILED
    sim.reset(seeds)
    assert sim.step(act)
    f = sim.get_fields()
    for e in range(B):
        one.reset(seeds[e:e + 1])
        assert one.step(act[e:e + 1])
        for x, y in zip(f, one.get_fields()):
            assert np.array_equal(x[e], y[0]), e

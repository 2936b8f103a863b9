"""Shared machinery of the two single-env classes.

The reference implements its 2D and 3D envs as two independent classes talking to Julia (src/rbc_gym/envs/rbc2D.py,
rbc3D.py).  Here both are thin descriptions (kwargs -> simulation config, spaces, info keys) on top of one base that
owns the episode logic: seeding quirk, checkpoint episodes, stepping a batch-of-one native simulation, truncation,
error behaviour.  Every behaviour cites the reference line it reproduces.
"""
import logging
import warnings
from enum import IntEnum
from pathlib import Path

import numpy as np

from .._gym import gym
from ..checkpoint import read_checkpoint


class RBCField(IntEnum):
    """channel order of observations / states (rbc2D.py:21-26)"""
    T = 0
    UX = 1
    UY = 2
    P = 3


def pick_checkpoint_episode(num_episodes, seed):
    """The reference draws `idx = rand(1:n)` from Julia's global RNG right after `Random.seed!(seed)`
    (rbc_sim2D_api.jl:44, rbc_sim2D.jl:176-177).  That stream cannot be reproduced outside Julia; this is the
    documented stand-in: deterministic in the seed."""
    return int(np.random.default_rng(int(seed) % (2**63)).integers(0, num_episodes))


def checkpoint_index(checkpoint_idx, num_episodes, seed):
    """0-based row of the episode to load.  `checkpoint_idx` is the reference's kwarg and keeps its meaning: it goes
    straight into Julia's `read(h5, "b")[idx, :, :, :]` (rbc_sim3D.jl:186-192), i.e. it is 1-BASED (eval_sarl.py:45 uses
    checkpoint_idx=1 for the first episode); 0 or > num_episodes is Julia's BoundsError, an IndexError here.  None =
    the seeded draw that stands in for `rand(1:n)`."""
    if checkpoint_idx is None:
        return pick_checkpoint_episode(num_episodes, seed)
    idx = int(checkpoint_idx)
    if not 1 <= idx <= int(num_episodes):
        raise IndexError(f"checkpoint_idx={checkpoint_idx} out of range: episodes are numbered 1..{int(num_episodes)} "
                         "(1-based, as in the reference's Julia reader)")
    return idx - 1


def check_checkpoint_grid(path, data, fields, state_shape):
    """the arrays of a checkpoint go to the device as raw pointers: refuse a file written on another grid"""
    cen = tuple(int(n) for n in state_shape)
    for f in fields:
        want = (cen[0] + 1,) + cen[1:] if f == "w" else cen
        got = tuple(data[f].shape[1:])
        if got != want:
            raise ValueError(f"{path}: dataset {f!r} has grid {got}, this env needs {want} (state_shape={list(cen)})")


def box_stack(shape, bounds):
    """Box over `len(bounds)` channels of `shape`, channel c bounded by bounds[c] = (low, high)."""
    shape = tuple(int(s) for s in shape)
    low = np.stack([np.full(shape, lo, dtype=np.float32) for lo, _ in bounds])
    high = np.stack([np.full(shape, hi, dtype=np.float32) for _, hi in bounds])
    return gym.spaces.Box(low, high, shape=(len(bounds),) + shape, dtype=np.float32)


def temperature_image(field, vmin, vmax):
    """(nz, nx) temperature -> (nx, nz, 3) uint8 through matplotlib's turbo map with z flipped so that the bottom plate
    is at the bottom of a top-left-origin canvas (what rbc2D.py:236-240 hands to pygame)."""
    import matplotlib
    scaled = (np.flip(np.transpose(field), axis=1) - vmin) / (vmax - vmin)
    return matplotlib.colormaps["turbo"](scaled, bytes=True)[:, :, :3]


def volume_lut():
    """Default transfer function of the 3D render(): float32 (256, 4) RGBA.  RGB is matplotlib's turbo at 256 entries (cmap="turbo",
    rbc3D.py:301); alpha is 1 / (1 + exp(-x)) for x = linspace(-1, 1, 256), which is PyVista's opacity="sigmoid_1" (rbc3D.py:303)
    as recalled -- PyVista is not installed here, so that is unchecked."""
    import matplotlib
    lut = np.empty((256, 4), np.float32)
    lut[:, :3] = matplotlib.colormaps["turbo"](np.linspace(0.0, 1.0, 256))[:, :3]
    lut[:, 3] = 1.0 / (1.0 + np.exp(-np.linspace(-1.0, 1.0, 256)))
    return lut


class _Window:
    """pygame window of the 'human' render mode (rbc2D.py:222-255); created lazily, closed with the env."""

    def __init__(self, size, fps, caption="Rayleigh Benard Convection"):
        self.size, self.fps, self.caption = size, fps, caption
        self.screen = None
        self.clock = None

    def show(self, image, native_size):
        try:
            import pygame
        except ImportError as e:
            raise RuntimeError("render_mode='human' needs pygame, which is not installed") from e
        if self.screen is None:
            pygame.init()
            pygame.display.init()
            self.screen = pygame.display.set_mode(self.size)
            pygame.display.set_caption(self.caption)
            self.clock = pygame.time.Clock()
        canvas = pygame.Surface(native_size)
        pygame.surfarray.blit_array(canvas, image)
        self.screen.blit(pygame.transform.scale(canvas, self.size), (0, 0))
        pygame.event.pump()
        self.clock.tick(self.fps)
        pygame.display.flip()

    def close(self):
        if self.screen is not None:
            import pygame
            pygame.display.quit()
            pygame.quit()
            self.screen = None


def flow_statistics_dict(prof, ext, single=False):
    """(prof, ext) of `get_flowstats()` under names: "profiles" (B, 6, nz) -- per-level means of b, u^2, v^2, w^2, b w, b^2 --,
    "u_max", "v_max", "w_max", "b_min", "b_max" (B,) and "kinetic_energy" = 1/2 mean over the levels of <u^2> + <v^2> + <w^2>;
    single: one env, without the batch axis"""
    out = {"profiles": prof, "kinetic_energy": 0.5 * (prof[:, 1] + prof[:, 2] + prof[:, 3]).mean(axis=1)}
    for j, name in enumerate(("u_max", "v_max", "w_max", "b_min", "b_max")):
        out[name] = ext[:, j].copy()
    if single:
        out = {k: (v[0] if k == "profiles" else float(v[0])) for k, v in out.items()}
    return out


SPECTRA_CHANNELS = ("b", "u", "v", "w", "bw_co", "bw_quad")


def power_spectra_dict(sim, single=False):
    """`sim.get_spectra()` under names: "x" (B, 6, nz, nx//2 + 1) and "y" (B, 6, nz, ny//2 + 1; None for 2D) -- one-sided power of
    b, u, v, w and the co- and quadrature spectrum of (b, w) per level, include/rbc_hip.h rbc_get_spectra --, the wavenumbers "kx" =
    2 pi m / Lx and "ky" = 2 pi n / Ly (None for 2D) and the channel names; single: one env, without the batch axis"""
    px, py = sim.get_spectra()
    kx, ky = sim.spectra_axes()
    if single:
        px, py = px[0], (None if py is None else py[0])
    return {"x": px, "y": py, "kx": kx, "ky": ky, "channels": SPECTRA_CHANNELS}


def dissipation_rates_dict(sim, wall_b=None, single=False):
    """`sim.get_dissipation(wall_b)` under names (include/rbc_hip.h rbc_get_dissipation; wall_b: the bottom plate's temperature,
    None = the uniform plate): "cells" (B, 4, nz) and "faces" (B, 5, nz + 1), the level means of the squared difference quotients,
    and per env, with the viscosity nu = sqrt(Pr / Ra) and the diffusivity kappa = 1 / sqrt(Pr Ra) the solver uses for that env,
      "thermal_dissipation" = kappa <|grad b|^2>,  "kinetic_dissipation" = nu <d_j u_i d_j u_i>,  "enstrophy" = <|curl u|^2>,
      "nusselt_thermal" = <|grad b|^2> lz^2 / delta_b^2,  "nusselt_viscous" = 1 + kinetic_dissipation lz / (kappa delta_b).
    The last two follow from the volume means of b times its equation (kappa <|grad b|^2> = the plates' flux times delta_b / lz) and
    of u times its equation (the buoyancy term of the w equation is b itself: eps_u = <w b> = kappa delta_b / lz (Nu - 1)); they
    equal the Nusselt number only for uniform plates in a statistically steady state -- the Nusselt number in units of the conductive
    flux kappa delta_b / lz, that is 1 + (Nu_info - 1) lz / delta_b for the 3D envs' info["nusselt"] = 1 + <w b'> / kappa (the reference's
    normalisation, rbc_sim3D_api.jl:134-159).  single: one env, without the batch axis"""
    cells, faces, tot = sim.get_dissipation(wall_b)
    nu, kappa = sim.nu_kappa()
    lz, delta_b = sim.cfg.lz, sim.cfg.delta_b
    eps_u = nu * (tot[:, 1] + tot[:, 2])
    out = {"cells": cells, "faces": faces, "thermal_dissipation": kappa * tot[:, 0], "kinetic_dissipation": eps_u,
           "enstrophy": tot[:, 2] - 2.0 * tot[:, 3], "nusselt_thermal": tot[:, 0] * lz ** 2 / delta_b ** 2,
           "nusselt_viscous": 1.0 + eps_u * lz / (kappa * delta_b)}
    if single:
        out = {k: (v[0] if k in ("cells", "faces") else float(v[0])) for k, v in out.items()}
    return out


class NativeEnvBase(gym.Env):
    """One env = a batch-of-one simulation handle.  Subclasses provide `_fields` (dataset names of a checkpoint
    episode), `_observe()`, `_info()` and `_reward()`."""

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 10}
    _fields = ("b", "u", "w")

    def _setup(self, sim, episode_length, checkpoint, render_mode, logger):
        self.sim = sim
        self.episode_length = episode_length
        self.checkpoint = checkpoint
        self.render_mode = render_mode
        self.logger = logger
        self.closed = False
        self._episodes = None
        logger.info(f"Using Rayleigh number Ra={self.ra}")
        logger.info(f"Using episode length {self.episode_length} timesteps")

    # ---- reset -----------------------------------------------------------------------------------
    def _checkpoint_episode(self, seed):
        path = Path(self.checkpoint)
        self.logger.info(f"Using checkpoint file {path.absolute()}")
        if not path.exists():
            raise FileNotFoundError(f"Checkpoint file {path} does not exist. Please provide a valid checkpoint directory.")
        key = str(path.absolute())
        if self._episodes is None or self._episodes[0] != key:
            self._episodes = (key, read_checkpoint(path))
        data = self._episodes[1]
        missing = [f for f in self._fields if f not in data]
        if missing:
            raise ValueError(f"{path}: checkpoint lacks dataset(s) {missing} needed by this env")
        idx = checkpoint_index(getattr(self, "checkpoint_idx", None), data["num_episodes"], seed)
        check_checkpoint_grid(path, data, self._fields, self.state_shape)
        return [data[f][idx:idx + 1] for f in self._fields]

    def reset(self, seed=None, options=None):
        super().reset(seed=seed)
        # quirk kept from the reference (rbc2D.py:150): reset(seed=None) re-uses the env's seed, so
        # every un-seeded reset of one env object starts the same episode
        seed = self.np_random_seed
        if self.checkpoint:
            self.sim.reset_from_arrays(*self._checkpoint_episode(seed))
        else:
            self.sim.reset(np.array([seed % (2**64)], dtype=np.uint64))
        self.last_action = np.zeros(self.action_space.shape, dtype=self.action_space.dtype)
        return self._observe(), self._info()

    # ---- step ------------------------------------------------------------------------------------
    def _checked_action(self, action):
        return np.asarray(action, dtype=np.float32).reshape((1,) + tuple(self.action_space.shape))

    def step(self, action=None):
        if action is None:                                     # rbc2D.py:164-166
            warnings.warn("No action provided, using zero action")
            action = np.zeros(self.action_space.shape, dtype=np.float32)
        if not self.sim.step(self._checked_action(action)):    # NaN scan of step_simulation (rbc_sim2D_api.jl:91-94)
            self.logger.error("Simulation step failed, probably NaN values in the simulation.")
            raise RuntimeError("Error in simulation step, probably NaN values")
        self.last_obs, self.last_reward, self.last_info = self._observe(), self._reward(), self._info()
        truncated = bool(self.last_info["t"] >= self.episode_length)
        return self.last_obs, self.last_reward, False, truncated, self.last_info      # there is no terminal state

    def flow_statistics(self):
        """Horizontal statistics of the current state, computed on the device (include/rbc_hip.h rbc_get_flowstats; what the
        reference's experiments/flowstats/flowstats_ra.py:64-67 takes from whole fields on the host): see flow_statistics_dict"""
        return flow_statistics_dict(*self.sim.get_flowstats(), single=True)

    def power_spectra(self):
        """Horizontal power and co-spectra of the current state, level by level, computed on the device: see power_spectra_dict"""
        return power_spectra_dict(self.sim, single=True)

    def dissipation_rates(self, wall_b=None):
        """Dissipation rates, enstrophy and the dissipation-based Nusselt numbers of the current state, computed on the device:
        see dissipation_rates_dict (wall_b: (ny, nx), 2D (nx,); None = the uniform plate)"""
        return dissipation_rates_dict(self.sim, None if wall_b is None else np.asarray(wall_b, np.float64)[None], single=True)

    # ---- teardown --------------------------------------------------------------------------------
    def close(self):
        window = getattr(self, "_window", None)
        if window is not None:
            window.close()
        if getattr(self, "sim", None) is not None:             # shutdown_simulation (rbc_sim3D_api.jl:164-172)
            self.sim.close()
            self.sim = None
        self.closed = True


def env_logger(name, log_dir=None, env_id=None):
    """module logger, optionally with the per-env file handler of rbc3D.py:84-99"""
    logger = logging.getLogger(name if env_id is None else f"{name}.{env_id}")
    if log_dir is not None:
        handler = logging.FileHandler(str(Path(log_dir) / f"env_{env_id}.log"))
        handler.setFormatter(logging.Formatter("%(asctime)s - %(name)s - %(levelname)s - %(message)s"))
        logger.addHandler(handler)
    return logger

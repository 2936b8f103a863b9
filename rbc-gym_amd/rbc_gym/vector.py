"""Batched on-device VectorEnv: replaces the reference's process-per-env fan-out.

The reference vectorises with `gym.make_vec(id, num_envs, vectorization_mode="async")`
(example/run_vectorized.py:11-20) or SB3's SubprocVecEnv (experiments/run_sarl.py:152-153):
one OS process and one Julia runtime per env.  Here all `num_envs` instances live in the HBM of
one MI355X and one kernel launch advances them all.  API and semantics follow gymnasium 1.1.x
`VectorEnv`: `reset(seed=s)` seeds env i with s+i, NEXT_STEP autoreset, infos as dict of stacked
arrays with `_key` masks.
"""
import logging
from pathlib import Path

import numpy as np

from ._gym import gym
from . import _native
from .checkpoint import read_checkpoint
from .sharded import ShardedSim
from .envs._common import check_checkpoint_grid, checkpoint_index, dissipation_rates_dict, flow_statistics_dict, power_spectra_dict
from .envs.rbc2D import build_spaces, sim_kwargs


class DeviceArray:
    """Zero-copy view of a device buffer of the simulation (`__cuda_array_interface__`, which
    PyTorch-ROCm understands: `torch.as_tensor(DeviceArray(...), device="cuda")`)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner


def _batch_space(space, n):
    return gym.spaces.Box(np.broadcast_to(space.low, (n,) + space.shape).copy(),
                          np.broadcast_to(space.high, (n,) + space.shape).copy(),
                          shape=(n,) + space.shape, dtype=space.dtype)


class _BatchedEnv(gym.vector.VectorEnv):
    """Seeding, NEXT_STEP autoreset and info stacking shared by the batched 2D and 3D envs.  Subclasses set
    `self.sim`, the spaces, `_fields` (checkpoint datasets) and implement `_observations()` / `_stacked_info()`."""

    metadata = {"render_modes": ["rgb_array"], "render_fps": 10, "autoreset_mode": "NextStep"}
    _fields = ("b", "u", "w")

    def _finish_init(self, num_envs, episode_length, checkpoint, render_mode):
        self.episode_length = episode_length
        self.checkpoint = checkpoint
        self.render_mode = render_mode
        self.logger = logging.getLogger(__name__)
        self.action_space = _batch_space(self.single_action_space, num_envs)
        self.observation_space = _batch_space(self.single_observation_space, num_envs)
        self._seeds = None
        self._autoreset = np.zeros(num_envs, dtype=bool)
        self._ckpt = None
        self.closed = False

    def _reset_envs(self, mask):
        seeds = self._seeds
        if self.checkpoint:
            path = Path(self.checkpoint)
            if not path.exists():
                raise FileNotFoundError(f"Checkpoint file {path} does not exist. Please provide a valid checkpoint directory.")
            if self._ckpt is None:
                self._ckpt = read_checkpoint(path)
            ck = self._ckpt
            missing = [f for f in self._fields if f not in ck]
            if missing:
                raise ValueError(f"{path}: checkpoint lacks dataset(s) {missing} needed by this env")
            check_checkpoint_grid(path, ck, self._fields, self.state_shape)
            fixed = getattr(self, "checkpoint_idx", None)                 # 1-based, like the reference's (rbc_sim3D.jl:186-192)
            idx = np.array([checkpoint_index(fixed, ck["num_episodes"], s) for s in seeds])
            self.sim.reset_from_arrays(*[ck[f][idx] for f in self._fields], mask=mask)
        else:
            self.sim.reset(np.asarray(seeds, dtype=np.uint64), mask=mask)

    def reset(self, *, seed=None, options=None):
        super().reset(seed=seed)
        n = self.num_envs
        if seed is None:
            if self._seeds is None:                      # each sub-env keeps the seed it drew first (rbc2D.py:150)
                self._seeds = np.random.SeedSequence().generate_state(n, dtype=np.uint64) % np.uint64(2**31)
        elif np.ndim(seed) == 0:
            self._seeds = (np.uint64(int(seed)) + np.arange(n, dtype=np.uint64))
        else:
            s = list(seed)
            if len(s) != n:
                raise ValueError("seed sequence must have num_envs entries")
            old = self._seeds if self._seeds is not None else np.random.SeedSequence().generate_state(n, dtype=np.uint64) % np.uint64(2**31)
            self._seeds = np.array([old[i] if s[i] is None else s[i] for i in range(n)], dtype=np.uint64)
        self._reset_envs(None)
        self._autoreset[:] = False
        info, _, _ = self._stacked_info()
        return self._observations(), info

    def step(self, actions):
        a = np.asarray(actions, dtype=np.float32).reshape((self.num_envs,) + tuple(self.single_action_space.shape))
        if not self.sim.step(a):
            bad = np.nonzero(self.sim.get_flags())[0]
            if not np.all(self._autoreset[bad]):         # an env that is re-initialised below may be ignored
                raise RuntimeError("Error in simulation step, probably NaN values")
        resetting = self._autoreset.copy()
        if resetting.any():                              # NEXT_STEP autoreset: these envs restart now, their action is ignored
            self._reset_envs(resetting.astype(np.uint8))
        info, t, nusselt = self._stacked_info()
        rewards = -nusselt
        rewards[resetting] = 0.0
        terminated = np.zeros(self.num_envs, dtype=bool)
        truncated = (t >= self.episode_length) & ~resetting
        self._autoreset = truncated.copy()
        return self._observations(), rewards, terminated, truncated, info

    def step_device(self, actions_device_ptr):
        """Advance all envs with actions already on the device (float32, batch-major); no host copy, no autoreset,
        asynchronous on the simulation's own stream: complete the writes of the actions before the call and
        `self.sim.synchronize()` (or an event) before another stream reads the device views.  With devices=[...]: a
        list of pointers, one per shard, each on that shard's GPU."""
        self.sim.step_dev(actions_device_ptr)

    def flow_statistics(self):
        """Horizontal statistics of every env's current state, computed on the device from the solver's own state (observation
        normalisation does not touch them); with devices=[...] the shards' results in env order.  See flow_statistics_dict."""
        return flow_statistics_dict(*self.sim.get_flowstats())

    def power_spectra(self):
        """Horizontal power and co-spectra of every env's current state, level by level, computed on the device from the solver's own
        state; with devices=[...] the shards' results in env order.  See power_spectra_dict."""
        return power_spectra_dict(self.sim)

    def dissipation_rates(self, wall_b=None):
        """Dissipation rates, enstrophy and the dissipation-based Nusselt numbers of every env's current state, computed on the device
        from the solver's own state; with devices=[...] the shards' results in env order.  See dissipation_rates_dict."""
        return dissipation_rates_dict(self.sim, wall_b)

    def _pooled(self, shape, mode):
        """destination for a large host output: a page-locked array nobody else references (None: let the getter allocate)"""
        if mode == "fresh" or int(np.prod(shape)) * 4 < _native.POOL_MIN_BYTES:
            return None
        pool = getattr(self, "_out_pool", None)
        if pool is None or pool.shape != tuple(shape):
            pool = self._out_pool = _native.PinnedPool(shape)
        return pool.take()

    def close(self, **kwargs):
        self._out_pool = None
        if getattr(self, "sim", None) is not None:
            self.sim.close()
            self.sim = None
        self.closed = True


class RayleighBenardConvection2DVectorEnv(_BatchedEnv):
    def __init__(self, num_envs=1, rayleigh_number=10_000, episode_length=300, observation_shape=(8, 48),
                 state_shape=(64, 96), heater_segments=12, heater_limit=0.75, heater_duration=1.5, pressure=False,
                 use_gpu=True, checkpoint=None, render_mode=None, device=0, devices=None, info_state=True, precision="f64",
                 reference_clock="documented", **_ignored):
        # info_state: True = info["state"] is a new array every step as far as the caller can tell (the reference's behaviour: large
        # ones come from _native.PinnedPool, which reuses a page-locked array only once the caller has dropped it), "fresh" = always
        # np.empty (the A/B partner), "pinned" = it rotates over three page-locked buffers unconditionally (an array is overwritten
        # three steps later), False = omitted
        self.num_envs = int(num_envs)
        self.ra = rayleigh_number
        self.observation_shape = list(observation_shape)
        self.state_shape = list(state_shape)
        self.temperature_difference = [1, 2]
        self.heater_segments = heater_segments
        self.heater_limit = heater_limit
        self.heater_duration = heater_duration
        self.include_pressure = pressure
        self.episode_steps = int(episode_length / heater_duration)
        self.info_state = info_state
        self.single_action_space, self.single_observation_space = build_spaces(self.observation_shape, heater_segments,
                                                                               heater_limit, pressure)
        ra0 = float(np.asarray(rayleigh_number, dtype=np.float64).ravel()[0])
        kw = sim_kwargs(ra0, self.observation_shape, self.state_shape, heater_segments, heater_limit, heater_duration)
        kw["precision"] = _native.PRECISIONS[precision]      # "f32": float32 arithmetic, envs paired up per workgroup
        self.precision = precision
        kw["reference_clock"] = self.reference_clock = reference_clock     # "recorded": see _native.CLOCKS
        # devices=[0, 1, ...]: the envs are split into contiguous ranges, one library handle per GPU (rbc_gym/sharded.py)
        self.devices = None if devices is None else [int(d) for d in devices]
        if self.devices is None:
            self.sim = _native.NativeSim(batch=self.num_envs, device=device, **kw)
        else:
            self.sim = ShardedSim(lambda count, dev: _native.NativeSim(batch=count, device=dev, **kw), self.num_envs, self.devices)
        if np.ndim(rayleigh_number) > 0:                 # per-env Rayleigh numbers (Ra sweeps)
            self.sim.set_rayleigh(np.asarray(rayleigh_number, dtype=np.float64))
        self._nch = 5 if pressure else 3
        self._pinned, self._pin_at = None, 0
        self._finish_init(self.num_envs, episode_length, checkpoint, render_mode)

    def _observations(self):
        return self.sim.get_obs(self._nch)

    def _stacked_info(self):
        t, step = self.sim.get_info()
        nus, nuo = self.sim.get_nusselt()
        ones = np.ones(self.num_envs, dtype=bool)
        info = {"t": t, "_t": ones, "step": step, "_step": ones.copy(),
                "nusselt_state": nus, "_nusselt_state": ones.copy(), "nusselt_obs": nuo, "_nusselt_obs": ones.copy()}
        if self.info_state:
            if self.info_state == "pinned":              # rotating page-locked buffers: an array stays valid for two more steps
                if self._pinned is None:
                    self._pinned = [_native.pinned_empty((self.num_envs, self._nch) + tuple(self.state_shape)) for _ in range(3)]
                self._pin_at = (self._pin_at + 1) % len(self._pinned)
                info["state"] = self.sim.get_state(self._nch, out=self._pinned[self._pin_at])
            else:
                info["state"] = self.sim.get_state(self._nch, out=self._pooled((self.num_envs, self._nch) + tuple(self.state_shape), self.info_state))
            info["_state"] = ones.copy()
        return info, t, nuo

    # -- device-resident rollout API (zero-copy PyTorch-ROCm tensors) --------------------------------
    def device_views(self):
        """zero-copy views of the library's output buffers; with devices=[...] a LIST with one dict per shard, each on its
        own GPU and covering that shard's contiguous env range (`self.sim.ranges`)"""
        (oz, ox), (nz, nx) = self.observation_shape, self.state_shape

        def views(p, B):
            return {"obs": DeviceArray(p["obs"], (B, 5, oz, ox), "<f4", self), "state": DeviceArray(p["state"], (B, 5, nz, nx), "<f4", self),
                    "nusselt": DeviceArray(p["nusselt"], (B, 2), "<f8", self), "flags": DeviceArray(p["flags"], (B,), "<i4", self)}
        if self.devices is None:
            return views(self.sim.dev_ptrs(), self.num_envs)
        return [dict(views(p, count), device=dev, env_range=(start, start + count))
                for p, dev, (start, count) in zip(self.sim.dev_ptrs(), self.devices, self.sim.ranges)]

    def render(self):
        """One frame per env, as gymnasium's vector envs return them (a tuple): the temperature field through the
        reference's colour map (rbc2D.py:236-240,258), from the float32 state already on the host side of the ABI."""
        if self.render_mode is None:
            gym.logger.warn("You are calling render method without specifying any render mode. "
                            "You can specify the render_mode at initialization, ")
            return None
        if self.render_mode != "rgb_array":
            raise ValueError(f"the batched env renders rgb_array frames only, not {self.render_mode!r}")
        from .envs._common import temperature_image
        temp = self.sim.get_state(1)[:, 0]                                   # (B, nz, nx)
        return tuple(temperature_image(t, 1, 2 + self.heater_limit).transpose(1, 0, 2) for t in temp)


class RayleighBenardConvection3DVectorEnv(_BatchedEnv):
    """Batched 3D env (BASELINE.json configs[4]: 32 envs per GPU): constructor kwargs of the reference's 3D env
    (rbc3D.py:43-61) plus num_envs / device; observations are the float32 states (B, 4, Nz, Ny, Nx), info {t, step, nusselt}."""
    metadata = {"render_modes": ["rgb_array"], "render_fps": 10, "autoreset_mode": "NextStep"}
    _fields = ("b", "u", "v", "w")

    def __init__(self, num_envs=1, rayleigh_number=2500, prandtl_number=0.7, domain=(2, 4 * np.pi, 4 * np.pi),
                 state_shape=(16, 32, 32), temperature_difference=(1, 2), heater_segments=8, heater_limit=0.9,
                 heater_duration=0.125, episode_length=300, dt_solver=0.01, use_gpu=True, checkpoint=None, checkpoint_idx=None,
                 render_mode=None, device=0, devices=None, precision="f64", obs_buffers=None, reference_clock="documented",
                 render_size=(800, 608), view_from=(1, 1, 1), projection="auto", **_ignored):
        # obs_buffers: None = every reset / step returns a new observation array as far as the caller can tell (the reference's
        # behaviour; large ones come from _native.PinnedPool: a page-locked array is reused only once the caller has dropped it),
        # "fresh" = always np.empty (the A/B partner), "pinned" = the observations rotate over three page-locked buffers
        # unconditionally (an array stays valid for two more steps).  The 38 MB of a configs[4] batch cross PCIe at the pinned rate
        # either way: 5.7k instead of 3.6k env-steps/s through the gym API
        from .envs.rbc3D import build_spaces3d
        self.obs_buffers = obs_buffers
        self.render_size, self.view_from = tuple(int(n) for n in render_size), tuple(float(x) for x in view_from)
        self._pinned, self._pin_at = None, 0
        self.num_envs = int(num_envs)
        self.reference_clock = reference_clock                       # "recorded": see _native.CLOCKS
        self.precision = precision                                   # "f32": the float32 instantiation of the 3D kernels (1.5x at configs[4])
        self.ra, self.pr = rayleigh_number, prandtl_number
        self.dim = 3
        self.domain, self.state_shape = list(domain), list(state_shape)
        self.temperature_difference = list(temperature_difference)
        self.heater_segments, self.heater_limit, self.heater_duration = heater_segments, heater_limit, heater_duration
        self.dt_solver = dt_solver
        self.checkpoint_idx = checkpoint_idx
        self.single_action_space, self.single_observation_space = build_spaces3d(state_shape, temperature_difference,
                                                                                 heater_segments, heater_limit)
        ra0 = float(np.asarray(rayleigh_number, dtype=np.float64).ravel()[0])
        def make(count, dev):
            return _native.NativeSim3D(batch=count, device=dev, shape=tuple(state_shape), domain=tuple(domain), ra=ra0,
                                       pr=float(prandtl_number), t_diff=tuple(temperature_difference), heaters=heater_segments,
                                       heater_limit=heater_limit, dt_control=heater_duration, dt_solver=dt_solver, precision=precision,
                                       reference_clock=reference_clock, projection=projection)
        self.projection = projection                                 # "pencil" | "chunked": see _native.PROJECTIONS; every shard runs the same
        self.devices = None if devices is None else [int(d) for d in devices]
        self.sim = make(self.num_envs, device) if self.devices is None else ShardedSim(make, self.num_envs, self.devices)
        if np.ndim(rayleigh_number) > 0:
            self.sim.set_rayleigh(np.asarray(rayleigh_number, dtype=np.float64))
        self._finish_init(self.num_envs, episode_length, checkpoint, render_mode)

    def _observations(self):
        if self.obs_buffers == "pinned":
            if self._pinned is None:
                self._pinned = [_native.pinned_empty((self.num_envs, 4) + tuple(self.state_shape)) for _ in range(3)]
            self._pin_at = (self._pin_at + 1) % len(self._pinned)
            return self.sim.get_state(out=self._pinned[self._pin_at])
        return self.sim.get_state(out=self._pooled((self.num_envs, 4) + tuple(self.state_shape), self.obs_buffers))

    def device_views(self):
        """zero-copy views of the library's output buffers (SURVEY 8(f) row 2 for the 3D env, whose observation IS the float32
        state: rbc3D.py:229-232): "obs" (B, 4, Nz, Ny, Nx) float32, "nusselt" (B,) float64, "flags" (B,) int32; with devices=[...] a
        LIST with one dict per shard, each on its own GPU and covering that shard's contiguous env range (`self.sim.ranges`).
        Same stream rules as `step_device`."""
        nz, ny, nx = self.state_shape

        def views(p, B):
            return {"obs": DeviceArray(p["state"], (B, 4, nz, ny, nx), "<f4", self), "nusselt": DeviceArray(p["nusselt"], (B,), "<f8", self),
                    "flags": DeviceArray(p["flags"], (B,), "<i4", self)}
        if self.devices is None:
            return views(self.sim.dev_ptrs(), self.num_envs)
        return [dict(views(p, count), device=dev, env_range=(start, start + count))
                for p, dev, (start, count) in zip(self.sim.dev_ptrs(), self.devices, self.sim.ranges)]

    def render(self):
        """The frames of all envs as one (num_envs, height, width, 3) uint8 array, frame i what the single env's render() returns
        for env i (envs/rbc3D.py): one launch of the device's volume ray-caster over the batch."""
        if self.render_mode is None:
            gym.logger.warn("You are calling render method without specifying any render mode. "
                            "You can specify the render_mode at initialization, ")
            return None
        if self.render_mode != "rgb_array":
            raise ValueError(f"the batched env renders rgb_array frames only, not {self.render_mode!r}")
        return self.sim.render(size=self.render_size, view_from=self.view_from, clim=self.temperature_difference)

    def _stacked_info(self):
        t, step = self.sim.get_info()
        nu = self.sim.get_nusselt()
        ones = np.ones(self.num_envs, dtype=bool)
        return {"t": t, "_t": ones, "step": step, "_step": ones.copy(), "nusselt": nu, "_nusselt": ones.copy()}, t, nu.copy()

"""CitationVecEnv -- the PH-LAB Citation env step-wise, batched on the GPU (C ABI v9 serl_venv_reset / serl_venv_step).

The reference's env is a gym object, `CitationEnv.reset()` / `.step(action)` (envs/phlabenv.py:401-482), stepped by whatever
policy its user has.  This is the same env for N envs at once: one HIP launch per `reset` / `step` (one lane = one env), the
actions a device tensor from any torch policy, no host synchronisation inside `step`.

    env = CitationVecEnv(4096, mode='PHlab_attitude_nominal', t_max=20)
    obs = env.reset()                                   # f64 [N, S] on the device
    while not bool(done.all()):                         # (the check syncs; a fixed step count does not)
        obs, reward, done, info = env.step(policy(obs.float()))
    obs = env.reset(done)                               # only the finished envs

Semantics (include/serl_amd.h, serl_venv_desc): the env does not clip the action; `reset` keeps the carried tracking error and the
model clock, as the reference does; a done env is frozen until it is reset (reward 0, done True, its last obs); by default there
is no auto-reset.  The tensors `reset` / `step` return are buffers of the env that the next call overwrites: clone what you keep.

`auto_reset=True` (serl_venv_step_auto) restarts a finished env inside the `step` launch that finishes it -- no `env.reset(done)`,
no second launch, no host synchronisation -- with the "same-step" convention of gymnasium's vector envs and SB3:

    env = CitationVecEnv(4096, t_max=20, auto_reset=True)
    obs = env.reset()                                   # starts the first episodes: auto-reset only restarts
    for _ in range(n_steps):
        obs, reward, done, info = env.step(policy(obs.float()))
        # where done: obs is obs0 of the NEW episode; reward, info['x' | 'ref' | 't' | 'cost'] are the terminal step's;
        # info['final_obs'] is the terminal observation, info['episode_return' | 'episode_length'] the finished episode's

The restart is what `reset(mask)` does (carried error kept, one clock tick, sensor-noise entry 0); the restarted episode flies the
given references again, reuses the env's sensor-noise table, and with `refs=None` takes the next of `ref_pool` references drawn per
env by the last explicit `reset` (the pool recycles after `ref_pool` episodes; an explicit `reset` draws a new one).

`env.rollout(policy, K)` (serl_venv_rollout) collects K such steps in ONE launch, the actor running inside the kernel:

    out = env.rollout(actor, 64, transitions=True)      # dict of step-major device tensors: obs [K + 1, N, S], actions, reward, done, ...
    replay.append_rows(out['transitions'].reshape(-1, 20))

By default (`path='auto'`) that kernel takes the SERL50 actor on the attitude task (7 -> 32 .. -> 3) and every other shape is stepped
one by one with a batched torch forward.  `path='fused'` also runs every other actor the C ABI packs -- hidden a multiple of 4 up to 128,
up to 16 hidden layers, any activation -- on every env configuration in one launch (serl_venv_rollout_general, transition rows of
2 S + A + 3 floats), or raises; `path='loop'` forces the step loop.

`sensor_noise='device'` (with auto_reset=True) draws the sensor noise inside the kernels from a counter-based generator (csrc/serl_rng.h,
serl_venv_*_noise): no table, no host draw, a fresh realisation for every episode of every env, reproducible from `env.noise_seed` and
`env.noise_episode`; `rollout(..., action_noise='device', noise_sd=, noise_clip=)` draws the exploration noise the same way.  `venv_noise`
writes any episode's draws out as a table.

`kernel='wave'` (serl_venv_*_wave) runs `reset` / `step` with one wavefront per env instead of one lane per env: the small-batch path, for one
to a few hundred envs, where a lane call is pure latency.  Same results bit for bit in every output, same state buffer layout; the lane rollout kernels are not run on such
an env (their table3 interval cache is the one state field the wave kernels cannot reproduce): `rollout(..., path='fused')` runs the wave rollout kernel instead
(serl_venv_rollout_wave, the actor on the wavefront), while the default path keeps to the step loop or raises.  `kernel='auto'` takes the wave path up to WAVE_MAX_ENVS envs; `env.last_step_kernel` says what the last call launched.
"""
import ctypes
import numpy as np
import torch

from . import _capi, builds, refsignals
from .actor import Actor, pad_rows, spec_of, unpack_into


# kernel='auto': the wave kernels (one wavefront per env) up to this many envs, the lane kernels beyond.  The largest measured n_envs at which the wave path
# beats the lane path by more than the lane runs' own spread, both with no env and with 3 % of the envs finishing per step, in
# profiles/venv_wave_timing.json (tools/bench_venv.py --kernel lane,wave; its `wave_max_envs`): 3x - 4x up to 1 024 envs, 2 - 7 % at 4 096, a loss of 13x at
# 65 536.  0 would mean never.
WAVE_MAX_ENVS = 4096
KERNELS = ('lane', 'wave', 'auto')


class CitationVecEnv:
    """n_envs copies of CitationEnv(configuration, mode) of one dynamics build, on one GPU.

    mode          an env name 'PHlab_<configuration>_<mode>' or a bare mode ('nominal', 'be', 'ice', 'gust', 'incremental' ...):
                  build, actuator-fault row, configuration (attitude / symmetric / full) and incremental control (builds.py)
    refs          None: every reset draws a fresh training reference per env, as CitationEnv.reset() does without user_refs
                  (refsignals.training_references, the draws make_evaluate makes), generated in the kernel (serl_ref_spec rows);
                  or a f64 table [N, T, 3] / [T, 3] (radians, rows at the env's accumulated step times: T bounds the episode), or
                  refsignals.ref_specs rows [N] / [1] (hand-made rows must satisfy refsignals.check_specs).  Given references stay until `reset(refs=...)` replaces those of the reset envs.
    sensor_noise  None: the modes with a sensor model ('noise', 'gust') draw builds.sensor_noise_table per env at every reset;
                  False: none; or f64 [N, T + 1, 7] (entry 0 belongs to the step of reset(), entry k + 1 to env step k); or 'device'
                  (needs auto_reset=True): the sensor model's addends (builds.sensor_terms) of normals drawn inside the kernels per
                  (seed, env, episode ordinal, entry) -- no table, and a restarted episode gets a realisation of its own.
    seed          the generator's 64-bit seed (None: one from np.random).  `noise_seed` and `noise_episode` (i32 [N]: episode starts
                  of every env so far; the running episode's ordinal is one less) are the generator's whole state: venv_noise replays
                  any episode from them.  A seed alone (no 'device' sensor noise) only prepares rollout(action_noise='device').
    engine        the RolloutEngine whose HIP context holds the build tables (default: the process's engine).
    auto_reset    True: `step` restarts the envs whose episode it ends, in the same launch; info gains 'final_obs' f64 [N, S],
                  'episode_return' f64 [N] and 'episode_length' i32 [N] (the last two valid where done).  The sensor-noise tables given
                  or drawn at the explicit reset are reused by the restarted episodes.
    ref_pool      auto_reset with refs=None: training references drawn per env by every explicit reset; the episode the reset starts
                  flies row 0, the j-th restart after it row j % ref_pool (the pool recycles after ref_pool episodes).
    kernel        'lane' (default): one lane per env; 'wave': one wavefront per env for reset / step (small batches); 'auto': 'wave' up to
                  WAVE_MAX_ENVS envs.  Every output is the same bit for bit; on an env that steps on the wave kernels rollout(path='fused') runs the wave rollout kernel,
                  and the default path raises a ValueError where it would have taken the lane kernel."""

    # device noise (serl_venv_noise_desc): the seed, the per-env count of episode starts, whether the sensor noise comes from the generator
    noise_seed = None
    noise_episode = None
    _dev_sensor = False

    def __init__(self, n_envs, mode='PHlab_attitude_nominal', t_max=20, refs=None, sensor_noise=None, engine=None, auto_reset=False,
                 ref_pool=4, seed=None, kernel='lane'):
        if kernel not in KERNELS:
            raise ValueError("kernel: one of 'lane', 'wave', 'auto', not %r" % (kernel,))
        if isinstance(refs, np.ndarray) and refs.dtype.names:
            refsignals.check_specs(refs)      # (widths > 0, non-decreasing times: before any device work)
        dev_sensor = isinstance(sensor_noise, str)
        if dev_sensor and sensor_noise != 'device':
            raise ValueError("sensor_noise: None, False, a table or 'device', not %r" % (sensor_noise,))
        if dev_sensor and not auto_reset:
            raise ValueError("sensor_noise='device' needs an env made with auto_reset=True")
        if seed is not None and not auto_reset:
            raise ValueError('seed: device noise needs an env made with auto_reset=True')
        if seed is not None and (isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2**64):
            raise ValueError('seed: an integer in [0, 2^64), not %r' % (seed,))
        if dev_sensor:
            sensor_noise = False      # (no table)
        if not torch.cuda.is_available():
            raise RuntimeError('serl_amd.CitationVecEnv needs a ROCm GPU (torch.cuda.is_available() is False); '
                               'the product has no CPU path')
        from .evaluator import default_engine
        self.n_envs = int(n_envs)
        if self.n_envs < 1:
            raise ValueError('n_envs must be >= 1')
        self.kernel = kernel
        self._wave = kernel == 'wave' or (kernel == 'auto' and self.n_envs <= WAVE_MAX_ENVS)
        self.mode, self.t_max = mode, float(t_max)
        self.auto_reset, self.ref_pool = bool(auto_reset), int(ref_pool)
        if self.auto_reset and self.ref_pool < 1:
            raise ValueError('ref_pool must be >= 1')
        self.env_config, self.incremental = builds.env_config(mode)
        self.state_dim, self.action_dim = builds.env_dims(self.env_config, self.incremental)
        self.build, row = builds.resolve_mode(mode)
        self.engine = engine or default_engine()
        self.lib = self.engine.lib
        self.device = self.engine.device
        N, dev = self.n_envs, self.device
        theta0 = float(np.asarray(builds.load(self.build)[0]['x0'])[7])
        # (one action: init_ref keeps the class default 0.22 deg, envs/phlabenv.py:202,304-313)
        self._trim = float(np.rad2deg(theta0)) if self.action_dim == 3 else 0.22
        self._draw_refs = refs is None
        self._ref = self._spec = self._pool = None
        if refs is None:
            self.max_steps = refsignals.n_steps_for(self.t_max)
            if self.auto_reset:      # [N][ref_pool] rows: the kernel walks them through its cursor
                self._pool = torch.zeros(N, self.ref_pool, refsignals.REF_SPEC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            else:
                self._spec = torch.zeros(N, refsignals.REF_SPEC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            self._spec_shared = False
        elif isinstance(refs, np.ndarray) and refs.dtype.names:
            if refs.dtype != refsignals.REF_SPEC_DTYPE or len(refs) not in (1, N):
                raise ValueError('refs: refsignals.ref_specs rows, one per env or one shared')
            self.max_steps = refsignals.n_steps_for(self.t_max)
            self._spec = self._spec_tensor(refs)
            self._spec_shared = len(refs) == 1
        else:
            r = torch.as_tensor(refs, dtype=torch.float64).to(dev).contiguous()
            if r.dim() not in (2, 3) or r.shape[-1] != 3 or (r.dim() == 3 and r.shape[0] != N):
                raise ValueError('refs: f64 [N, T, 3] or [T, 3]')
            self._ref, self.max_steps = r, int(r.shape[-2])
        self._draw_noise = sensor_noise is None and builds.has_sensor_noise(mode)
        self._noise = None
        if self._draw_noise:
            self._noise = torch.zeros(N, self.max_steps + 1, 7, dtype=torch.float64, device=dev)
        elif sensor_noise is not None and sensor_noise is not False:
            self._noise = torch.as_tensor(sensor_noise, dtype=torch.float64).to(dev).contiguous()
            if self._noise.shape != (N, self.max_steps + 1, 7):
                raise ValueError('sensor_noise: f64 [N, max_steps + 1, 7] = %s' % ((N, self.max_steps + 1, 7),))
        if dev_sensor or seed is not None:
            self._enable_device_noise(seed, dev_sensor, started=False)
        self._faults = None
        if row != builds.NOMINAL_ROW:
            self._faults = torch.as_tensor(np.tile(np.asarray(row, np.float64), (N, 1))).to(dev).contiguous()
        nbytes = int(self.lib.serl_venv_state_bytes(N))
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)      # zero-filled: fresh envs, not running
        S, A = self.state_dim, self.action_dim
        self._obs = torch.zeros(N, S, dtype=torch.float64, device=dev)
        self._reward = torch.zeros(N, dtype=torch.float64, device=dev)
        self._done = torch.ones(N, dtype=torch.bool, device=dev)               # (a bool tensor is one byte 0 / 1 per element)
        self._x = torch.zeros(N, 12, dtype=torch.float64, device=dev)
        self._refk = torch.zeros(N, 3, dtype=torch.float64, device=dev)
        self._t = torch.zeros(N, dtype=torch.float64, device=dev)
        self._cost = torch.zeros(N, dtype=torch.int32, device=dev)
        self.desc = _capi.VenvDesc(n_envs=N, build_slot=self.engine.slot_of(self.build), env_config=self.env_config,
                                   incremental=int(self.incremental), state_dim=S, action_dim=A, max_steps=self.max_steps,
                                   t_max=self.t_max, state=self._state.data_ptr())
        if self._faults is not None:
            self.desc.faults = self._faults.data_ptr()
        if self._ref is not None:
            self.desc.ref, self.desc.ref_stride = self._ref.data_ptr(), (0 if self._ref.dim() == 2 else self.max_steps * 3)
        elif self._pool is not None:      # (serl_venv_reset reads no reference; serl_venv_step_auto reads the pool)
            self.desc.ref_spec, self.desc.ref_spec_stride = self._pool.data_ptr(), 1
        else:
            self.desc.ref_spec, self.desc.ref_spec_stride = self._spec.data_ptr(), (0 if self._spec_shared else 1)
        if self._noise is not None:
            self.desc.sensor_noise = self._noise.data_ptr()
        if self.auto_reset:
            self._final_obs = torch.zeros(N, S, dtype=torch.float64, device=dev)
            self._ep_return = torch.zeros(N, dtype=torch.float64, device=dev)
            self._ep_length = torch.zeros(N, dtype=torch.int32, device=dev)
            self._run_return = torch.zeros(N, dtype=torch.float64, device=dev)
            self._run_length = torch.zeros(N, dtype=torch.int32, device=dev)
            self._cursor = torch.zeros(N, dtype=torch.int32, device=dev)
            self.auto_desc = _capi.VenvAutoDesc(final_obs=self._final_obs.data_ptr(), ep_return=self._ep_return.data_ptr(),
                                                ep_length=self._ep_length.data_ptr(), run_return=self._run_return.data_ptr(),
                                                run_length=self._run_length.data_ptr(), cursor=self._cursor.data_ptr())
            if self._pool is not None:
                self.auto_desc.ref_pool, self.auto_desc.pool_rows = self._pool.data_ptr(), self.ref_pool

    def _enable_device_noise(self, seed=None, sensor=False, started=True):
        """Give the env a generator state; from here on reset / step / rollout run the noise instantiations of their kernels, which count
        the episode starts.  started: the envs are already flying an episode the count has not seen (ordinal 0)."""
        if seed is None:
            seed = int(np.random.randint(0, 2**32)) << 32 | int(np.random.randint(0, 2**32))
        self.noise_seed = int(seed)
        self._dev_sensor = bool(sensor)
        self.noise_episode = torch.full((self.n_envs,), 1 if started else 0, dtype=torch.int32, device=self.device)

    def _nz_desc(self, action=False, sd=0.0, clip=0.0):
        bias, scale = builds.sensor_bias_scale()
        return _capi.VenvNoiseDesc(seed=self.noise_seed, episode_count=self.noise_episode.data_ptr(), sensor=int(self._dev_sensor),
                                   sensor_bias=(ctypes.c_double * 7)(*bias), sensor_scale=(ctypes.c_double * 7)(*scale),
                                   action=int(action), action_sd=float(sd), action_clip=float(clip))

    def _spec_tensor(self, specs):
        return torch.from_numpy(np.ascontiguousarray(specs).view(np.uint8).reshape(len(specs), -1)).to(self.device)

    # 'lane' or 'wave': the kernel family the library said it launched for THIS env's most recent reset / step (serl_venv_last_info, read right
    # behind the call: the library's record is per context, which other envs share); None before the first one
    last_step_kernel = None

    def _call(self, name, noise, *args):
        """the entry point `name` of this env's kernel family (`_wave`) and noise flavour on (ctx, *args); notes what the library launched"""
        name += ('_wave' if self._wave else '') + ('_noise' if noise else '')
        _capi.check(getattr(self.lib, name)(self.engine.ctx, *args), name)
        info = (ctypes.c_int32 * 4)()
        _capi.check(self.lib.serl_venv_last_info(self.engine.ctx, info), 'serl_venv_last_info')
        self.last_step_kernel = _capi.FAMILIES[int(info[0])]

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self, mask=None, refs=None, sensor_noise=None, err0=None, tick0=None):
        """Reset the envs of `mask` (bool [N] device tensor; None = all) -> obs f64 [N, S]: obs0 of the reset envs, the current
        observation of the others.  refs / sensor_noise: new references / sensor-noise tables for the reset envs, one row per
        reset env in env order (the env's kind: table rows [T, 3] or ref_specs rows).  err0 f64 [N, 3] / tick0 i32 [N]: carried
        error and model clock to start the reset envs from instead of their own (a fresh env carries 0 and 0).
        auto_reset: also clears the running return / length and the pool cursor of the reset envs; with refs=None at construction it
        draws their ref_pool references (env-major), or `refs` rows become their pool row 0 -- rows 1 .. ref_pool - 1 keep what they
        held (the previous draw; zero references, i.e. trim only, if no drawing reset came before), and the restarts fly them."""
        N, dev = self.n_envs, self.device
        if isinstance(refs, np.ndarray) and refs.dtype.names:
            refsignals.check_specs(refs)      # (before any device work)
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=dev)
            if m.shape != (N,) or m.dtype != torch.bool:
                raise ValueError('mask: bool [%d]' % N)
            m = m.contiguous()
        need_index = refs is not None or sensor_noise is not None or self._draw_refs or self._draw_noise
        idx = None
        if need_index:      # (the host draws / row copies need the indices: one sync per reset, none per step)
            idx = torch.arange(N, device=dev) if m is None else torch.nonzero(m).reshape(-1)
        if refs is not None:
            if isinstance(refs, np.ndarray) and refs.dtype.names:
                if self._pool is not None:
                    self._pool[idx, 0] = self._spec_tensor(refs)
                elif self._spec is None or self._spec_shared:
                    raise ValueError('refs: this env reads per-env ref_specs rows only if it was made with them (or with refs=None)')
                else:
                    self._spec[idx] = self._spec_tensor(refs)
            else:
                if self._ref is None or self._ref.dim() != 3:
                    raise ValueError('refs: this env reads per-env tables only if it was made with them')
                self._ref[idx] = torch.as_tensor(refs, dtype=torch.float64).to(dev).reshape(-1, self.max_steps, 3)
        elif self._draw_refs and len(idx):
            R = self.ref_pool if self._pool is not None else 1
            th, ph = refsignals.training_references(len(idx) * R, self.t_max, np.random, n_actions=self.action_dim)
            rows = self._spec_tensor(refsignals.ref_specs(th, ph, theta_trim_deg=self._trim))
            if self._pool is not None:
                self._pool[idx] = rows.reshape(len(idx), R, -1)
            else:
                self._spec[idx] = rows
        if sensor_noise is not None:
            if self._dev_sensor:
                raise ValueError("sensor_noise: this env draws its sensor noise on the device (sensor_noise='device')")
            if self._noise is None:
                raise ValueError('sensor_noise: this env was made without a sensor model')
            self._noise[idx] = torch.as_tensor(sensor_noise, dtype=torch.float64).to(dev).reshape(-1, self.max_steps + 1, 7)
        elif self._draw_noise and len(idx):
            self._noise[idx] = torch.from_numpy(np.stack([builds.sensor_noise_table(self.max_steps) for _ in range(len(idx))])).to(dev)
        if self.auto_reset:      # (masked device ops: no index, no synchronisation)
            for buf in (self._run_return, self._run_length, self._cursor):
                buf.zero_() if m is None else buf.masked_fill_(m, 0)
        keep = []
        d = _capi.VenvDesc.from_buffer_copy(self.desc)
        if err0 is not None:
            e0 = torch.as_tensor(err0, dtype=torch.float64).to(dev).reshape(N, 3).contiguous()
            d.err0 = e0.data_ptr(); keep.append(e0)
        if tick0 is not None:
            t0 = torch.as_tensor(tick0, dtype=torch.int32).to(dev).reshape(N).contiguous()
            d.tick0 = t0.data_ptr(); keep.append(t0)
        if self.noise_episode is not None:
            nz = self._nz_desc()
            self._call('serl_venv_reset', True, ctypes.byref(d), None if m is None else m.data_ptr(), self._obs.data_ptr(), ctypes.byref(nz),
                       self._stream())
        else:
            self._call('serl_venv_reset', False, ctypes.byref(d), None if m is None else m.data_ptr(), self._obs.data_ptr(), self._stream())
        del keep      # (freed memory is handed out again only to work ordered behind this launch on the same stream)
        return self._obs

    def step(self, actions):
        """actions [N, A] f32 or f64 on the device, in [-1, 1] by convention (not clipped here) -> (obs f64 [N, S], reward f64 [N],
        done bool [N], info {'x': f64 [N, 12], 'ref': f64 [N, 3], 't': f64 [N], 'cost': i32 [N]}).  auto_reset: one launch that also
        restarts the envs it finishes (obs is then obs0 of the new episode); info adds 'final_obs', 'episode_return', 'episode_length'."""
        a = actions
        if not isinstance(a, torch.Tensor) or a.device != self.device or a.dtype not in (torch.float32, torch.float64):
            raise ValueError('actions: a f32 / f64 tensor on %s' % self.device)
        if a.shape != (self.n_envs, self.action_dim):
            raise ValueError('actions: [%d, %d], not %s' % (self.n_envs, self.action_dim, tuple(a.shape)))
        a = a.contiguous()
        if self.auto_reset:
            if self.noise_episode is not None:
                nz = self._nz_desc()
                self._call('serl_venv_step_auto', True, ctypes.byref(self.desc), a.data_ptr(), int(a.dtype == torch.float64),
                           self._obs.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(),
                           self._x.data_ptr(), self._refk.data_ptr(), self._t.data_ptr(), self._cost.data_ptr(),
                           ctypes.byref(self.auto_desc), ctypes.byref(nz), self._stream())
            else:
                self._call('serl_venv_step_auto', False, ctypes.byref(self.desc), a.data_ptr(), int(a.dtype == torch.float64),
                           self._obs.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(), self._x.data_ptr(),
                           self._refk.data_ptr(), self._t.data_ptr(), self._cost.data_ptr(),
                           ctypes.byref(self.auto_desc), self._stream())
            return self._obs, self._reward, self._done, {'x': self._x, 'ref': self._refk, 't': self._t, 'cost': self._cost,
                                                         'final_obs': self._final_obs, 'episode_return': self._ep_return,
                                                         'episode_length': self._ep_length}
        self._call('serl_venv_step', False, ctypes.byref(self.desc), a.data_ptr(), int(a.dtype == torch.float64),
                   self._obs.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(), self._x.data_ptr(),
                   self._refk.data_ptr(), self._t.data_ptr(), self._cost.data_ptr(), self._stream())
        return self._obs, self._reward, self._done, {'x': self._x, 'ref': self._refk, 't': self._t, 'cost': self._cost}

    # ---- K policy-driven steps in one launch (serl_venv_rollout) ------------------------------------------------------------------
    # 'fused' (serl_venv_rollout), 'fused-general' (serl_venv_rollout_general), 'fused-wave' (serl_venv_rollout_wave) or 'loop' (step by step with a torch forward) of the last rollout()
    last_rollout_path = None
    ROLLOUT_PATHS = ('auto', 'fused', 'loop')

    def _kernel_takes(self, entry, spec):
        """whether the rollout entry point `entry` runs `spec` actors on this env: the library's own contract (serl_shape_query)"""
        return _capi.shape_query(entry, spec, int(self.env_config) + 3 * bool(self.incremental)).takes

    def fused_rollout_ok(self, spec):
        """True when rollout() runs `spec` actors inside the kernel: the attitude task without rate control and the lane actor's
        shape (7 observations, hidden 32, 3 actions; any number of hidden layers and activation)."""
        return self._kernel_takes('serl_venv_rollout', spec)

    def fused_general_ok(self, spec):
        """True when rollout(path='fused') can run `spec` actors inside the general kernel (serl_venv_rollout_general): every env
        configuration; an actor that fits this env, hidden a multiple of 4 in 4 .. 128, 0 .. 16 hidden layers, any activation."""
        return self._kernel_takes('serl_venv_rollout_general', spec)

    def fused_wave_ok(self, spec):
        """True when rollout(path='fused') on an env that steps on the wave kernels can run `spec` actors inside the wave rollout kernel
        (serl_venv_rollout_wave, one wavefront per env): the shapes of fused_general_ok, the lane kernel's 7 -> 32 .. -> 3 among them."""
        return self.fused_general_ok(spec)

    def _check_rollout_args(self, policy, n_steps, spec, member_of_env, action_noise, path='auto'):
        """The argument checks of rollout() that need no device work -> (K, list of actor modules or None, NetSpec)."""
        if path not in self.ROLLOUT_PATHS:
            raise ValueError("path: one of 'auto', 'fused', 'loop', not %r" % (path,))
        if not self.auto_reset:
            raise ValueError('rollout needs an env made with auto_reset=True')
        if isinstance(n_steps, bool) or int(n_steps) != n_steps or int(n_steps) < 1:
            raise ValueError('n_steps: an integer >= 1, not %r' % (n_steps,))
        K, N = int(n_steps), self.n_envs
        mods = None
        if isinstance(policy, torch.Tensor):
            if spec is None:
                raise ValueError('policy: packed weights need spec=NetSpec(...)')
            if policy.device != self.device:
                raise ValueError('policy: packed weights on %s, the env is on %s' % (policy.device, self.device))
            if policy.dtype != torch.float32 or policy.dim() != 2 or policy.shape[0] < 1 or policy.shape[1] < spec.param_count:
                raise ValueError('policy: packed f32 [members, >= %d]' % spec.param_count)
        else:
            mods = [getattr(p, 'actor', p) for p in (policy if isinstance(policy, (list, tuple)) else [policy])]
            if not mods:
                raise ValueError('policy: an empty list')
            spec = spec_of(mods[0])
            if any(spec_of(m) != spec for m in mods):
                raise ValueError('policy: the actors of a list must have one shape')
        if (spec.state_dim, spec.action_dim) != (self.state_dim, self.action_dim):
            raise ValueError('actor %d -> %d does not fit the env (%d observations, %d actions)'
                             % (spec.state_dim, spec.action_dim, self.state_dim, self.action_dim))
        if member_of_env is not None and tuple(np.shape(member_of_env)) != (N,):
            raise ValueError('member_of_env: i32 [%d], not %s' % (N, tuple(np.shape(member_of_env))))
        if action_noise is not None and tuple(np.shape(action_noise)) != (K, N, 3):
            raise ValueError('action_noise: f64 %s, not %s' % ((K, N, 3), tuple(np.shape(action_noise))))
        if path == 'fused' and not (self.fused_rollout_ok(spec) or self.fused_general_ok(spec)):
            raise ValueError("path='fused': no kernel runs a %d -> %d x %d -> %d actor (hidden: a multiple of 4 in 4 .. 128; 0 .. 16 "
                             "hidden layers)" % (spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim))
        return K, mods, spec

    def rollout(self, policy, n_steps, *, member_of_env=None, action_noise=None, transitions=False, info=True, spec=None, path='auto',
                noise_sd=None, noise_clip=None):
        """n_steps steps of every env under `policy`, restarts included, in ONE launch without host synchronisation
        (serl_venv_rollout: the actor runs inside the kernel, bit-identical to the fused rollout kernels' forward).  Needs auto_reset=True.

        policy         an Actor / GeneticAgent, a list of them, or packed f32 weights [members, >= P] on the env's device with
                       spec=NetSpec(...) (the zero-overhead form: modules are packed on the device at every call)
        member_of_env  i32 [N], each in [0, members): the env's member of the population; None: every env runs member 0
        action_noise   f64 [n_steps, N, 3] added to the actor's output, the sum clipped to [-1, 1] (base/core/agent.py:90-93); or 'device'
                       with noise_sd= and noise_clip=: clip(noise_sd z, +-noise_clip) of normals drawn inside the kernel per (noise_seed,
                       env, episode ordinal, in-episode step) -- rollout(K1) then rollout(K2) draws what rollout(K1 + K2) draws.  On an
                       env made without seed= / sensor_noise='device' the first such call draws a seed and starts counting episodes.
        -> dict of fresh device tensors, step-major: 'obs' f64 [K + 1, N, S] (row 0: where the segment started; row k + 1: what
        step() returns after step k), 'actions' f64 [K, N, A] (the executed action, actor units), 'reward' f64, 'done' bool,
        'final_obs' f64 [K, N, S], 'ep_return' f64 / 'ep_length' i32 (valid where done, 0 elsewhere); info: 'x' [K, N, 12], 'ref'
        [K, N, 3], 't', 'cost' i32; transitions: 'transitions' f32 [K, N, 2 S + A + 3] = (obs, action, final_obs, reward, fin, cost),
        what DeviceReplay.append_rows takes after reshape(-1, 20) -- fin is the bounds / t_max flag, not the end of a reference table.
        Never-reset envs stay frozen (reward 0, done, action 0; their transition rows carry fin = 1: mask them out).
        step() and rollout() share the env state and may be mixed.
        path           'auto': the lane kernel where fused_rollout_ok(spec) (attitude task, 7 -> 32 .. -> 3), else one step() per step with
                       a batched torch forward, to the same dictionary; 'fused': in a kernel or ValueError -- the lane kernel where
                       fused_rollout_ok, else the general kernel (serl_venv_rollout_general: every env configuration, hidden a multiple
                       of 4 up to 128, up to 16 hidden layers) where fused_general_ok; 'loop': always the step loop (A/B runs, tests;
                       on an env with device noise its forward is the kernels' own, serl_venv_actor_forward, for every shape a kernel takes:
                       there the paths agree bit for bit).
                       On an env that steps on the wave kernels (kernel='wave' / 'auto') 'fused' runs the wave rollout kernel
                       (serl_venv_rollout_wave: one wavefront per env, every shape of fused_wave_ok, bit for bit what the lane kernels
                       compute); 'auto' there keeps to the step loop, and raises for the lane kernel's shape.
                       `last_rollout_path` says 'fused', 'fused-general', 'fused-wave' or 'loop'."""
        dev_action = isinstance(action_noise, str)
        if dev_action:
            if action_noise != 'device':
                raise ValueError("action_noise: f64 [n_steps, N, 3] or 'device', not %r" % (action_noise,))
            if noise_sd is None or noise_clip is None or not float(noise_sd) >= 0.0 or not float(noise_clip) >= 0.0:
                raise ValueError("action_noise='device' needs noise_sd >= 0 and noise_clip >= 0")
            action_noise = None
        elif noise_sd is not None or noise_clip is not None:
            raise ValueError("noise_sd / noise_clip belong to action_noise='device'")
        K, mods, spec = self._check_rollout_args(policy, n_steps, spec, member_of_env, action_noise, path)
        N, S, A, dev = self.n_envs, self.state_dim, self.action_dim, self.device
        if dev_action and self.noise_episode is None:
            self._enable_device_noise()
        nz = None
        if self.noise_episode is not None:
            nz = self._nz_desc(dev_action, noise_sd or 0.0, noise_clip or 0.0)
        moe = None
        if member_of_env is not None:
            moe = torch.as_tensor(member_of_env).to(device=dev, dtype=torch.int32).contiguous()
        noise = None
        if action_noise is not None:
            noise = torch.as_tensor(action_noise, dtype=torch.float64).to(dev).contiguous()
        lane32 = self.fused_rollout_ok(spec)
        if path == 'loop' or (path == 'auto' and not lane32):
            self.last_rollout_path = 'loop'
            return self._rollout_loop(policy, mods, spec, K, moe, noise, transitions, info, nz if dev_action else None)
        if self._wave and path == 'fused':      # K steps on the wave kernels themselves: one wavefront per env, the wave-cooperative actor
            if not self.fused_wave_ok(spec):
                raise ValueError("path='fused': no wave kernel runs a %d -> %d x %d -> %d actor (hidden: a multiple of 4 in 4 .. 128; 0 .. 16 "
                                 "hidden layers)" % (spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim))
            lane32 = False
        elif self._wave:
            # The lane step walks the table3 S-function's interval cache (IW[0..2] of the state) from a work word it never initialises, so what a
            # lane call leaves there depends on the compiled kernel and the wave calls cannot reproduce it (they leave the words alone).  No output
            # has been seen to depend on it, but the lane rollout kernels are not handed a state they did not write.
            raise ValueError("rollout in a kernel: this env steps on the wave kernels (kernel=%r), whose state the lane rollout kernels do not take over; "
                             "make the env with kernel='lane', or take path='fused' (the wave rollout kernel) or path='loop'" % (self.kernel,))
        w = self._packed_rows(policy, mods)
        out = self._rollout_buffers(K, transitions, info)
        rd = _capi.VenvRolloutDesc(state_dim=spec.state_dim, action_dim=spec.action_dim, hidden=spec.hidden, num_layers=spec.num_layers,
                                   activation=spec.activation_id, n_members=w.shape[0], weights=w.data_ptr(),
                                   weight_stride=w.stride(0) if w.shape[0] > 1 else w.shape[1], n_steps=K,
                                   member_of_env=None if moe is None else moe.data_ptr(),
                                   action_noise=None if noise is None else noise.data_ptr(),
                                   obs=out['obs'].data_ptr(), actions=out['actions'].data_ptr(), reward=out['reward'].data_ptr(),
                                   done=out['done'].data_ptr(), final_obs=out['final_obs'].data_ptr(),
                                   ep_return=out['ep_return'].data_ptr(), ep_length=out['ep_length'].data_ptr())
        if info:
            rd.x, rd.ref, rd.t, rd.cost = (out[k].data_ptr() for k in ('x', 'ref', 't', 'cost'))
        if transitions:
            rd.transitions = out['transitions'].data_ptr()
        entry = 'serl_venv_rollout_wave' if self._wave else 'serl_venv_rollout' if lane32 else 'serl_venv_rollout_general'
        if nz is not None:
            entry += '_noise'
            _capi.check(getattr(self.lib, entry)(self.engine.ctx, ctypes.byref(self.desc), ctypes.byref(self.auto_desc), ctypes.byref(rd),
                                                 ctypes.byref(nz), self._stream()), entry)
        else:
            _capi.check(getattr(self.lib, entry)(self.engine.ctx, ctypes.byref(self.desc), ctypes.byref(self.auto_desc), ctypes.byref(rd),
                                                 self._stream()), entry)
        del w, moe, noise      # (freed memory is handed out again only to work ordered behind this launch on the same stream)
        self.last_rollout_path = 'fused-wave' if self._wave else 'fused' if lane32 else 'fused-general'
        return out

    def _packed_rows(self, policy, mods):
        """the packed f32 rows the kernels read: 16-byte aligned, a multiple of 4 floats apart"""
        if mods is None:
            w = policy
        else:      # packed on the device: no .cpu() round trip, no synchronisation
            w = torch.stack([torch.cat([p.detach().reshape(-1) for p in m.parameters()]).to(device=self.device, dtype=torch.float32) for m in mods])
        if w.shape[1] % 4 or w.stride(0) % 4 or not w.is_contiguous():
            w = pad_rows(w)
        if w.data_ptr() % 16:      # (a view into a larger tensor: the kernel reads rows with 16-byte loads)
            w = w.clone()
        return w

    def _rollout_buffers(self, K, transitions, info):
        N, S, A, dev = self.n_envs, self.state_dim, self.action_dim, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        out = {'obs': torch.empty(K + 1, N, S, **f64), 'actions': torch.empty(K, N, A, **f64), 'reward': torch.empty(K, N, **f64),
               'done': torch.empty(K, N, dtype=torch.bool, device=dev), 'final_obs': torch.empty(K, N, S, **f64),
               'ep_return': torch.zeros(K, N, **f64), 'ep_length': torch.zeros(K, N, dtype=torch.int32, device=dev)}
        if info:
            out.update(x=torch.empty(K, N, 12, **f64), ref=torch.empty(K, N, 3, **f64), t=torch.empty(K, N, **f64),
                       cost=torch.empty(K, N, dtype=torch.int32, device=dev))
        if transitions:
            out['transitions'] = torch.empty(K, N, 2 * S + A + 3, dtype=torch.float32, device=dev)
        return out

    def _rollout_loop(self, policy, mods, spec, K, moe, noise, transitions, info, nz=None):
        """rollout() for the shapes serl_venv_rollout does not take: K x step() with a batched torch forward, to the same dictionary.
        nz (action_noise='device'): the step's addends are what the kernels would draw, written out by serl_venv_noise_fill.
        On an env with device noise (noise_episode is set) the forward is the kernels' own where a kernel takes the shape
        (serl_venv_actor_forward instead of torch, whose f32 kernels differ from the ABI's arithmetic in the last bits): device noise
        promises bit-exact replay, so there the loop computes what path='fused' computes.  Every other env keeps the torch forward."""
        N, S, A, dev = self.n_envs, self.state_dim, self.action_dim, self.device
        abi_forward = self.noise_episode is not None and (self.fused_rollout_ok(spec) or self.fused_general_ok(spec))
        if abi_forward:
            w = self._packed_rows(policy, mods)
            fd = _capi.VenvRolloutDesc(state_dim=spec.state_dim, action_dim=spec.action_dim, hidden=spec.hidden, num_layers=spec.num_layers,
                                       activation=spec.activation_id, n_members=w.shape[0], weights=w.data_ptr(),
                                       weight_stride=w.stride(0) if w.shape[0] > 1 else w.shape[1],
                                       member_of_env=None if moe is None else moe.data_ptr())
        elif mods is None:      # packed rows -> modules (a host round trip per member: this is the slow path)
            import types
            args = types.SimpleNamespace(state_dim=spec.state_dim, action_dim=spec.action_dim, hidden_size=spec.hidden,
                                         num_layers=spec.num_layers, activation_actor=spec.activation, device=dev)
            mods = []
            for row in policy:
                mods.append(Actor(args))
                unpack_into(mods[-1], row)
        else:
            import copy
            mods = [m if next(m.parameters()).device == dev else copy.deepcopy(m).to(dev) for m in mods]

        def forward(o):
            if abi_forward:      # (o: a row of out['obs'], f64 and contiguous; the kernel converts to f32 as the rollout kernels do)
                a = torch.empty(N, A, dtype=torch.float32, device=dev)
                _capi.check(self.lib.serl_venv_actor_forward(self.engine.ctx, ctypes.byref(fd), N, o.data_ptr(), a.data_ptr(), self._stream()),
                            'serl_venv_actor_forward')
                return a
            with torch.no_grad():
                if moe is None:
                    return mods[0](o)
                a = torch.zeros(N, A, dtype=torch.float32, device=dev)
                for j, m in enumerate(mods):
                    a = torch.where((moe == j)[:, None], m(o), a)
                return a
        # the state buffer (csrc/rollout_device.h SerlVenvF64 / SerlVenvI32): 73 f64 fields, then 17 i32 fields, [field][N rounded up to 64]
        npad = (N + 63) // 64 * 64
        t_env = self._state[:73 * npad * 8].view(torch.float64).view(73, npad)[57, :N]      # SERL_VF_T: the env's accumulated time
        live = self._state[73 * npad * 8:].view(torch.int32).view(17, npad)[15, :N].ne(0).clone()      # SERL_VI_LIVE: never changes under auto-reset
        k_env = self._state[73 * npad * 8:].view(torch.int32).view(17, npad)[14, :N]      # SERL_VI_K: steps of the running episode
        env_index = torch.arange(N, dtype=torch.int32, device=dev)
        deg = 3.14159265358979323846 / 180.0
        out = self._rollout_buffers(K, transitions, info)
        # the current observation of every env: a reset of no env writes it
        none = torch.zeros(N, dtype=torch.bool, device=dev)
        _capi.check(self.lib.serl_venv_reset(self.engine.ctx, ctypes.byref(self.desc), none.data_ptr(), self._obs.data_ptr(),
                                             self._stream()), 'serl_venv_reset')
        out['obs'][0].copy_(self._obs)
        for k in range(K):
            o = out['obs'][k]
            a = forward(o if abi_forward else o.float())
            if noise is not None:
                a = torch.clamp(a.double() + noise[k, :, :A], -1.0, 1.0)
            elif nz is not None:      # (a view of the state buffer is contiguous along the envs; the count is read in stream order)
                addend = _noise_fill(self.engine, nz, 3, env_index, self.noise_episode - 1, k_env.contiguous(), 1)
                a = torch.clamp(a.double() + addend[:, 0, :A], -1.0, 1.0)
            out['actions'][k].copy_(torch.where(live[:, None], a.double(), torch.zeros_like(a, dtype=torch.float64)))
            timed_out = t_env >= self.t_max      # (at the pre-increment t, as the env decides it)
            obs, rew, done, inf = self.step(a)
            out['obs'][k + 1].copy_(obs); out['reward'][k].copy_(rew); out['done'][k].copy_(done)
            out['final_obs'][k].copy_(inf['final_obs'])
            ended = done & live
            out['ep_return'][k].copy_(torch.where(ended, inf['episode_return'], torch.zeros_like(rew)))
            out['ep_length'][k].copy_(torch.where(ended, inf['episode_length'], torch.zeros_like(inf['episode_length'])))
            if info:
                for key in ('x', 'ref', 't', 'cost'):
                    out[key][k].copy_(inf[key])
            if transitions:
                x = inf['x']
                fin = timed_out | (x[:, 7].abs() > 60.0 * deg) | (x[:, 6].abs() > 75.0 * deg) | (x[:, 9] < 50.0)
                fin = torch.where(live, fin, torch.ones_like(fin))
                out['transitions'][k].copy_(torch.cat([o.float(), out['actions'][k].float(), inf['final_obs'].float(), rew.float()[:, None],
                                                       fin.float()[:, None], inf['cost'].ne(0).float()[:, None]], dim=1))
        return out


_FILL_MODES = {'bits': (0, 24, torch.int32), 'normal': (1, 7, torch.float64), 'sensor': (2, 7, torch.float64), 'action': (3, 3, torch.float64)}


def _noise_fill(engine, nz, mode, env, episode, entry0, entries):
    """serl_venv_noise_fill on device i32 [rows] tensors -> a fresh tensor [rows, entries, W]"""
    code, W, dtype = [v for v in _FILL_MODES.values() if v[0] == mode][0]
    rows = int(env.shape[0])
    out = torch.empty(rows, int(entries), W, dtype=dtype, device=engine.device)
    _capi.check(engine.lib.serl_venv_noise_fill(engine.ctx, ctypes.byref(nz), code, rows, env.data_ptr(), episode.data_ptr(), entry0.data_ptr(),
                                                int(entries), out.data_ptr(),
                                                ctypes.c_void_p(torch.cuda.current_stream(engine.device).cuda_stream)), 'serl_venv_noise_fill')
    return out


def venv_noise(seed, env, episode, entries, kind='sensor', *, entry0=0, noise_sd=None, noise_clip=None, engine=None):
    """What CitationVecEnv's kernels draw for `entries` consecutive entries, entry0 onwards, of the episodes (seed; env[i], episode[i]) ->
    a device tensor [rows, entries, W], written by the kernels' own device functions (serl_venv_noise_fill).

    env, episode, entry0   integers or integer arrays / tensors [rows] (scalars are broadcast): env index, episode ordinal of that env
                           (env.noise_episode - 1 is the running one), first entry
    kind  'sensor'  f64 W = 7: the sensor model's addends (builds.sensor_terms of the normals); entries = max_steps + 1 from entry 0 is the
                    table CitationVecEnv(sensor_noise=...), reset(sensor_noise=...), evaluate_pop and the oracle take
          'normal'  f64 W = 7: the standard normals behind them
          'action'  f64 W = 3: clip(noise_sd z, +-noise_clip), the exploration noise of in-episode step entry0 + j
          'bits'    the raw Philox words as i32 bit patterns, W = 24: the sensor stream's four blocks, then the action stream's two"""
    if kind not in _FILL_MODES:
        raise ValueError("kind: one of 'sensor', 'normal', 'action', 'bits', not %r" % (kind,))
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2**64:
        raise ValueError('seed: an integer in [0, 2^64), not %r' % (seed,))
    if isinstance(entries, bool) or int(entries) != entries or int(entries) < 1:
        raise ValueError('entries: an integer >= 1, not %r' % (entries,))
    if kind == 'action' and (noise_sd is None or noise_clip is None or not float(noise_sd) >= 0.0 or not float(noise_clip) >= 0.0):
        raise ValueError("kind='action' needs noise_sd >= 0 and noise_clip >= 0")
    if not torch.cuda.is_available():
        raise RuntimeError('serl_amd.venv_noise needs a ROCm GPU (torch.cuda.is_available() is False); the product has no CPU path')
    from .evaluator import default_engine
    engine = engine or default_engine()
    cols = [torch.as_tensor(v).to(device=engine.device, dtype=torch.int32).reshape(-1) for v in (env, episode, entry0)]
    rows = max(len(c) for c in cols)
    if any(len(c) not in (1, rows) for c in cols):
        raise ValueError('env / episode / entry0: scalars or arrays of one length')
    cols = [c.expand(rows).contiguous() for c in cols]
    bias, scale = builds.sensor_bias_scale()
    nz = _capi.VenvNoiseDesc(seed=int(seed), sensor_bias=(ctypes.c_double * 7)(*bias), sensor_scale=(ctypes.c_double * 7)(*scale),
                             action_sd=float(noise_sd or 0.0), action_clip=float(noise_clip or 0.0))
    return _noise_fill(engine, nz, _FILL_MODES[kind][0], cols[0], cols[1], cols[2], int(entries))

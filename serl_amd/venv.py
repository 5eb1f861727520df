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
"""
import ctypes
import numpy as np
import torch

from . import _capi, builds, refsignals


class CitationVecEnv:
    """n_envs copies of CitationEnv(configuration, mode) of one dynamics build, on one GPU.

    mode          an env name 'PHlab_<configuration>_<mode>' or a bare mode ('nominal', 'be', 'ice', 'gust', 'incremental' ...):
                  build, actuator-fault row, configuration (attitude / symmetric / full) and incremental control (builds.py)
    refs          None: every reset draws a fresh training reference per env, as CitationEnv.reset() does without user_refs
                  (refsignals.training_references, the draws make_evaluate makes), generated in the kernel (serl_ref_spec rows);
                  or a f64 table [N, T, 3] / [T, 3] (radians, rows at the env's accumulated step times: T bounds the episode), or
                  refsignals.ref_specs rows [N] / [1].  Given references stay until `reset(refs=...)` replaces those of the reset envs.
    sensor_noise  None: the modes with a sensor model ('noise', 'gust') draw builds.sensor_noise_table per env at every reset;
                  False: none; or f64 [N, T + 1, 7] (entry 0 belongs to the step of reset(), entry k + 1 to env step k).
    engine        the RolloutEngine whose HIP context holds the build tables (default: the process's engine).
    auto_reset    True: `step` restarts the envs whose episode it ends, in the same launch; info gains 'final_obs' f64 [N, S],
                  'episode_return' f64 [N] and 'episode_length' i32 [N] (the last two valid where done).  The sensor-noise tables given
                  or drawn at the explicit reset are reused by the restarted episodes.
    ref_pool      auto_reset with refs=None: training references drawn per env by every explicit reset; the episode the reset starts
                  flies row 0, the j-th restart after it row j % ref_pool (the pool recycles after ref_pool episodes)."""

    def __init__(self, n_envs, mode='PHlab_attitude_nominal', t_max=20, refs=None, sensor_noise=None, engine=None, auto_reset=False,
                 ref_pool=4):
        if not torch.cuda.is_available():
            raise RuntimeError('serl_amd.CitationVecEnv needs a ROCm GPU (torch.cuda.is_available() is False); '
                               'the product has no CPU path')
        from .evaluator import default_engine
        self.n_envs = int(n_envs)
        if self.n_envs < 1:
            raise ValueError('n_envs must be >= 1')
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

    def _spec_tensor(self, specs):
        return torch.from_numpy(np.ascontiguousarray(specs).view(np.uint8).reshape(len(specs), -1)).to(self.device)

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
        _capi.check(self.lib.serl_venv_reset(self.engine.ctx, ctypes.byref(d), None if m is None else m.data_ptr(),
                                             self._obs.data_ptr(), self._stream()), 'serl_venv_reset')
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
            _capi.check(self.lib.serl_venv_step_auto(self.engine.ctx, ctypes.byref(self.desc), a.data_ptr(), int(a.dtype == torch.float64),
                                                     self._obs.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(), self._x.data_ptr(),
                                                     self._refk.data_ptr(), self._t.data_ptr(), self._cost.data_ptr(),
                                                     ctypes.byref(self.auto_desc), self._stream()), 'serl_venv_step_auto')
            return self._obs, self._reward, self._done, {'x': self._x, 'ref': self._refk, 't': self._t, 'cost': self._cost,
                                                         'final_obs': self._final_obs, 'episode_return': self._ep_return,
                                                         'episode_length': self._ep_length}
        _capi.check(self.lib.serl_venv_step(self.engine.ctx, ctypes.byref(self.desc), a.data_ptr(), int(a.dtype == torch.float64),
                                            self._obs.data_ptr(), self._reward.data_ptr(), self._done.data_ptr(), self._x.data_ptr(),
                                            self._refk.data_ptr(), self._t.data_ptr(), self._cost.data_ptr(), self._stream()),
                    'serl_venv_step')
        return self._obs, self._reward, self._done, {'x': self._x, 'ref': self._refk, 't': self._t, 'cost': self._cost}

#!/usr/bin/env python3
"""Throughput of the step-wise vector env (serl_amd.CitationVecEnv, C ABI v9 serl_venv_step) on the GPU box:
    python tools/bench_venv.py [--sizes 1024,8192,65536] [--steps 2001] [--warmup 50]
One JSON line: env-steps/s and microseconds per `step` call at each N, in three configurations --
    env        a fixed action tensor (the env alone)
    mlp        a torch SERL50-shaped actor (7 -> 32 tanh, 3 x [32 LayerNorm tanh], -> 3 tanh; the shipped actor 18) on the same stream,
               closed loop, no host synchronisation inside the loop
    fused      for reference: the fused lane rollout (lanes_per_wave = 64: actor + env + dynamics in one kernel) at the same N
-- timed with device events after a warm-up, every env flying the base reference (one shared table) from a fresh reset; only live env
steps count (a done env is frozen and costs little).  Also the resource usage of the new kernels (tools/kernel_regs.sh on the build's objects).

    python tools/bench_venv.py --auto-reset [--sizes 1024,65536] [--auto-steps 1000] [--reps 5] [--out profiles/venv_auto_timing.json]
runs the auto-reset leg instead: CitationVecEnv(auto_reset=True) (serl_venv_step_auto) against the loop it replaces, medians and
[min .. max] of `reps` repetitions after a warm-up, the versions of a comparison alternating within each repetition --
    staggered  episodes of 32 steps on a shared table, the envs' phases spread evenly (3 % of the envs finish per step):
               `step` with auto_reset=True against `step` followed by `reset(done)` every step (two launches, no host draw)
    drawn      the same with refs=None at t_max = 5 (502 steps, 0.2 % finish per step): the manual loop's `reset(done)` then finds the
               finished envs on the host and draws their references there (one synchronisation per step); auto flies its pool
               (N <= --drawn-max-n only: the host draws dominate beyond)
    idle       no env finishing (t_max = 20, fewer steps than an episode): the auto step against the plain step -- the cost of the larger kernel

    python tools/bench_venv.py --rollout [--sizes 1024,65536] [--auto-steps 1000] [--rollout-k 50] [--reps 5] [--out profiles/venv_rollout_timing.json]
runs the rollout leg: `env.rollout(actor, K)` (serl_venv_rollout: the SERL50 actor inside the kernel, K steps per launch, fresh output
tensors per call) against the loop it replaces, `obs, ... = env.step(actor(obs.float()))` on an auto_reset env with the same actor as a
torch module on the same stream -- the same `staggered` and `idle` settings, medians and [min .. max] of `reps` repetitions of
--auto-steps env steps after a warm-up, the versions alternating.

    python tools/bench_venv.py --rollout --hidden 72 [--layers 3] [--path fused] [--out profiles/venv_rollout_general_timing.json]
runs the same leg for an actor of another shape (7 -> hidden x layers -> 3, tanh, seeded default initialisation) on the attitude task:
`env.rollout(actor, K, path=<--path>)` (serl_venv_rollout_general for 'fused') against `env.rollout(actor, K, path='loop')`, the only
path these shapes had before.  --hidden takes a comma-separated list; the results of all shapes go into one file.

    python tools/bench_venv.py --device-noise [--sizes 1024,65536] [--auto-steps 1000] [--rollout-k 50] [--reps 5] [--out profiles/venv_device_noise_timing.json]
runs the device-noise leg: mode 'noise', episodes of 64 steps on a shared table at spread phases, CitationVecEnv(sensor_noise='device')
(serl_venv_*_noise: the sensor noise drawn inside the kernels) against the table path (a pre-drawn f64 [N, 65, 7] table, 238 MB at 65 536 envs) --
`step` under auto-reset with a fixed action, and `rollout(actor, K)` with the SERL50 actor, there also with action_noise='device' against a
pre-drawn [K, N, 3] tensor; medians and [min .. max] of `reps` repetitions after a warm-up, the versions alternating.  Then the wall time and
the bytes of noise tables of one full `reset()` at --reset-n envs with t_max = 20 on both paths (--reset-n 0 skips it).

    python tools/bench_venv.py --kernel lane,wave [--sizes 1,16,64,256,1024,4096,65536] [--auto-steps 1000] [--reps 5] [--out profiles/venv_wave_timing.json]
runs the kernel-family leg: CitationVecEnv(kernel='lane') (one lane per env) against kernel='wave' (one wavefront per env, serl_venv_*_wave) in the loops
of the auto-reset leg, a fixed action, medians and [min .. max] of `reps` repetitions after a warm-up, the versions alternating --
    step            the plain `step`, no env finishing (the auto-reset leg's `idle`, manual version)
    auto_idle       `step` with auto_reset=True, no env finishing (its `idle`, auto version)
    auto_staggered  `step` with auto_reset=True, episodes of 32 steps at spread phases: 3 % of the envs finish per step (its `staggered`, auto version)
-- and derives the env count up to which kernel='auto' should take the wave path: the largest measured N at which the wave median is below the lane
median by more than the lane repetitions' own spread (max - min) in auto_idle and in auto_staggered.  `--kernel lane` or `--kernel wave` measures one.

    python tools/bench_venv.py --rollout --kernel wave [--sizes 1,16,64,256,1024,4096] [--auto-steps 500] [--rollout-k 50] [--reps 5] [--out profiles/venv_rollout_wave_timing.json]
runs the wave rollout leg: `rollout(actor, K, path='fused')` on CitationVecEnv(kernel='wave') (serl_venv_rollout_wave: one wavefront per env, the actor on
the wavefront) against (a) `path='loop'` on the same kind of env, the only way to roll out there before, and (b) `path='fused'` on a kernel='lane' env (the
lane rollout kernels) -- for the SERL50 actor and for hidden 72 x 3, with no env finishing (`idle`) and with 3 % of the envs finishing per step (`staggered`),
medians and [min .. max] of `reps` repetitions after a warm-up, the three versions taking turns within each repetition."""
import argparse, json, os, subprocess, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import serl_amd
from serl_amd import build as hip_build, refsignals as rs


def serl50_policy(device):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'actors.npz'))['serl50'][18]
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    layers = {}
    for name, o, shape in spec.param_layout():
        layers[name] = torch.from_numpy(g[o:o + int(np.prod(shape))].reshape(shape).copy())
    a = serl_amd.Actor(argparse.Namespace(hidden_size=32, num_layers=3, activation_actor='tanh', state_dim=7, action_dim=3, device=torch.device('cpu')))
    a.load_state_dict(layers)
    return a.to(device).eval()


def live_steps(t_final, dt=0.01):
    """env steps taken: a done env's t is frozen at its last step"""
    return int(np.rint(t_final.cpu().numpy() / dt).sum())


def bench_env(eng, N, steps, warmup, ref, policy=None):
    env = serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=ref, engine=eng)
    dev = env.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    with torch.no_grad():
        obs = env.reset()
        for _ in range(warmup):
            obs, _, _, _ = env.step(policy(obs.float()) if policy is not None else fixed)
        obs = env.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            obs, rew, done, info = env.step(policy(obs.float()) if policy is not None else fixed)
        e1.record()
        e1.synchronize()
    ms = e0.elapsed_time(e1)
    n = live_steps(info['t'])
    return dict(N=N, config='mlp' if policy is not None else 'env', calls=steps, ms=round(ms, 3), us_per_call=round(1e3 * ms / steps, 2),
                live_env_steps=n, env_steps_per_s=round(n / (ms * 1e-3), 1), done_at_end=int(done.sum()))


def bench_fused(eng, N, ref, warmup):
    w = torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', 'actors.npz'))['serl50'][[18]])
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    moe = np.zeros(N, np.int32)
    if warmup:
        eng.rollout(w, spec, moe, ref, t_max=20, lanes_per_wave=64)
    out = eng.rollout(w, spec, moe, ref, t_max=20, lanes_per_wave=64)
    ms = eng.last_kernel_ms
    n = int(out['length_steps'].abs().sum())
    return dict(N=N, config='fused', calls=1, ms=round(ms, 3), us_per_call=None, live_env_steps=n, env_steps_per_s=round(n / (ms * 1e-3), 1))


def _stagger(env, L, fixed):
    """phases spread evenly over an episode of L steps: afterwards env e has taken (L - 1 - e % L) steps of its episode"""
    e = torch.arange(env.n_envs, device=env.device)
    for j in range(L):
        env.reset(e % L == j)
        if j + 1 < L:
            obs, rew, done, info = env.step(fixed)
            if not env.auto_reset:
                env.reset(done)


def _timed(env, steps, fixed, manual_reset):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nfin = torch.zeros((), dtype=torch.int64, device=env.device)
    e0.record()
    for _ in range(steps):
        obs, rew, done, info = env.step(fixed)
        if manual_reset:
            env.reset(done)
    e1.record()
    e1.synchronize()
    nfin += done.sum()
    return e0.elapsed_time(e1), int(nfin)


def _summary(N, steps, ms):
    rate = sorted(N * steps / (m * 1e-3) for m in ms)
    us = sorted(1e3 * m / steps for m in ms)
    med = lambda v: v[len(v) // 2]
    return dict(env_steps_per_s=dict(median=round(med(rate), 1), min=round(rate[0], 1), max=round(rate[-1], 1)),
                us_per_step=dict(median=round(med(us), 2), min=round(us[0], 2), max=round(us[-1], 2)), reps_ms=[round(m, 3) for m in ms])


def bench_auto(eng, N, steps, warmup, reps, drawn_steps, drawn_max_n):
    """One size: the three comparisons of the module docstring.  Every env is live in every timed step of every version."""
    dev = eng.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    L = 32
    table = np.ascontiguousarray(rs.tabulate(*rs.base_reference(20), 20)[:L])
    out = dict(N=N, steps=steps, reps=reps, warmup=warmup)

    def compare(name, make, steps, stagger_L, manual_reset):
        envs = {v: make(v == 'auto') for v in ('auto', 'manual')}
        ms = {v: [] for v in envs}
        fin = {}
        with torch.no_grad():
            for v, env in envs.items():
                if stagger_L:
                    _stagger(env, stagger_L, fixed)
                else:
                    env.reset()
                _timed(env, warmup, fixed, manual_reset and v == 'manual')
            for r in range(reps):
                for v, env in (list(envs.items()) if r % 2 == 0 else list(envs.items())[::-1]):      # alternate the order
                    if not stagger_L:
                        env.reset()      # idle: every repetition from a fresh episode, so that no env finishes
                    m, fin[v] = _timed(env, steps, fixed, manual_reset and v == 'manual')
                    ms[v].append(m)
        out[name] = dict(steps=steps, auto=_summary(N, steps, ms['auto']), manual=_summary(N, steps, ms['manual']),
                         finished_on_last_step=fin)
        a, m = out[name]['auto']['env_steps_per_s'], out[name]['manual']['env_steps_per_s']
        out[name]['speedup_of_medians'] = round(a['median'] / m['median'], 3)

    compare('staggered', lambda auto: serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=table, engine=eng, auto_reset=auto),
            steps, L, True)
    np.random.seed(0)
    if N <= drawn_max_n:      # (beyond, the manual loop's time is the host's reference draws, not the GPU's)
        compare('drawn', lambda auto: serl_amd.CitationVecEnv(N, mode='nominal', t_max=5, engine=eng, auto_reset=auto), drawn_steps,
                rs.n_steps_for(5), True)
    full = rs.tabulate(*rs.base_reference(20), 20)
    assert steps + warmup < len(full)
    compare('idle', lambda auto: serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=full, engine=eng, auto_reset=auto), steps, 0, False)
    return out


def bench_kernels(eng, N, steps, warmup, reps, kernels):
    """One size: the kernel families of `kernels` in the three loops of the module docstring.  Every env is live in every timed step."""
    dev = eng.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    L = 32
    full = rs.tabulate(*rs.base_reference(20), 20)
    table = np.ascontiguousarray(full[:L])
    assert steps + warmup < len(full)
    out = dict(N=N, steps=steps, reps=reps, warmup=warmup)
    for name, refs, auto, stagger_L in (('step', full, False, 0), ('auto_idle', full, True, 0), ('auto_staggered', table, True, L)):
        envs = {k: serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=refs, engine=eng, auto_reset=auto, kernel=k) for k in kernels}
        ms, fin, ran = {k: [] for k in envs}, {}, {}
        with torch.no_grad():
            for k, env in envs.items():
                if stagger_L:
                    _stagger(env, stagger_L, fixed)
                else:
                    env.reset()
                _timed(env, warmup, fixed, False)
                ran[k] = env.last_step_kernel
            for r in range(reps):
                for k, env in (list(envs.items()) if r % 2 == 0 else list(envs.items())[::-1]):      # alternate the order
                    if not stagger_L:
                        env.reset()      # every repetition from a fresh episode, so that no env finishes
                    m, fin[k] = _timed(env, steps, fixed, False)
                    ms[k].append(m)
        out[name] = {k: _summary(N, steps, ms[k]) for k in envs}
        out[name].update(launched=ran, finished_on_last_step=fin)
        if len(envs) == 2:
            a, b = (out[name][k]['us_per_step'] for k in ('lane', 'wave'))
            out[name]['wave_over_lane_us_per_step'] = round(b['median'] / a['median'], 4)
            out[name]['wave_wins_beyond_lane_spread'] = bool(a['median'] - b['median'] > a['max'] - a['min'])
        del envs
    return out


def wave_max_envs(results):
    """the largest measured N at which the wave path beats the lane path by more than the lane runs' own spread, both with no env and with 3 % of the envs
    finishing per step; 0 if there is none"""
    wins = [r['N'] for r in results if all(r[c].get('wave_wins_beyond_lane_spread') for c in ('auto_idle', 'auto_staggered'))]
    return max(wins) if wins else 0


def seeded_policy(device, hidden, layers):
    """a 7 -> hidden x layers -> 3 tanh actor with torch's default initialisation under a fixed seed"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        a = serl_amd.Actor(argparse.Namespace(hidden_size=hidden, num_layers=layers, activation_actor='tanh', state_dim=7, action_dim=3,
                                              device=torch.device('cpu')))
    return a.to(device).eval()


def bench_rollout(eng, N, steps, K, warmup, reps, hidden=None, layers=3, path='fused'):
    """One size: rollout(actor, K) against the step loop with the torch actor, episodes of 32 steps at spread phases and no env finishing.
    hidden: another actor shape -- rollout(path=path) against rollout(path='loop')."""
    dev = eng.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    actor = serl50_policy(dev) if hidden is None else seeded_policy(dev, hidden, layers)
    L = 32
    table = np.ascontiguousarray(rs.tabulate(*rs.base_reference(20), 20)[:L])
    full = rs.tabulate(*rs.base_reference(20), 20)
    assert steps % K == 0 and warmup % K == 0 and steps + warmup < len(full)
    out = dict(N=N, steps=steps, K=K, reps=reps, warmup=warmup)
    if hidden is not None:
        out.update(hidden=hidden, layers=layers, path=path)

    def run(env, v, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if hidden is not None:      # both versions through rollout(): the kernel (or whatever `path` picks) against the step loop
            for _ in range(n // K):
                o = env.rollout(actor, K, path=path if v == 'rollout' else 'loop')
            if n:
                out.setdefault('paths', {})[v] = env.last_rollout_path
                done = o['done'][-1]
            else:
                done = torch.zeros(N, dtype=torch.bool, device=dev)
        elif v == 'rollout':
            for _ in range(n // K):
                o = env.rollout(actor, K)
            assert env.last_rollout_path == 'fused'
            done = o['done'][-1]
        else:
            obs = env.reset(torch.zeros(N, dtype=torch.bool, device=dev)) if n else None      # (the current observation; one launch per run)
            for _ in range(n):
                obs, rew, done, info = env.step(actor(obs.float()))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), int(done.sum())

    for name, refs, stagger_L in (('staggered', table, L), ('idle', full, 0)):
        envs = {v: serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=refs, engine=eng, auto_reset=True) for v in ('rollout', 'loop')}
        ms, fin = {v: [] for v in envs}, {}
        with torch.no_grad():
            for v, env in envs.items():
                if stagger_L:
                    _stagger(env, stagger_L, fixed)
                else:
                    env.reset()
                run(env, v, warmup)
            for r in range(reps):
                for v, env in (list(envs.items()) if r % 2 == 0 else list(envs.items())[::-1]):      # alternate the order
                    if not stagger_L:
                        env.reset()      # idle: every repetition from a fresh episode, so that no env finishes
                    m, fin[v] = run(env, v, steps)
                    ms[v].append(m)
        out[name] = dict(rollout=_summary(N, steps, ms['rollout']), loop=_summary(N, steps, ms['loop']), finished_on_last_step=fin)
        a, m = out[name]['rollout']['env_steps_per_s'], out[name]['loop']['env_steps_per_s']
        out[name]['speedup_of_medians'] = round(a['median'] / m['median'], 3)
    return out


def bench_rollout_wave(eng, N, steps, K, warmup, reps, hidden=None, layers=3):
    """One size and actor: the wave rollout kernel against the step loop on a wave env and against the lane rollout kernel, idle and staggered."""
    dev = eng.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    actor = serl50_policy(dev) if hidden is None else seeded_policy(dev, hidden, layers)
    L = 32
    full = rs.tabulate(*rs.base_reference(20), 20)
    table = np.ascontiguousarray(full[:L])
    assert steps % K == 0 and warmup % K == 0 and steps + warmup < len(full)
    versions = {'wave_fused': ('wave', 'fused'), 'wave_loop': ('wave', 'loop'), 'lane_fused': ('lane', 'fused')}
    out = dict(N=N, steps=steps, K=K, reps=reps, warmup=warmup, hidden=32 if hidden is None else hidden, layers=layers)

    def run(env, v, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n // K):
            o = env.rollout(actor, K, path=versions[v][1])
        e1.record()
        e1.synchronize()
        out.setdefault('paths', {})[v] = env.last_rollout_path
        return e0.elapsed_time(e1), int(o['done'][-1].sum())

    for name, refs, stagger_L in (('idle', full, 0), ('staggered', table, L)):
        envs = {v: serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=refs, engine=eng, auto_reset=True, kernel=k) for v, (k, _) in versions.items()}
        ms, fin = {v: [] for v in envs}, {}
        order = list(envs.items())
        with torch.no_grad():
            for v, env in order:
                if stagger_L:
                    _stagger(env, stagger_L, fixed)
                else:
                    env.reset()
                run(env, v, warmup)
            for r in range(reps):
                for v, env in order[r % 3:] + order[:r % 3]:      # the versions take turns at going first
                    if not stagger_L:
                        env.reset()      # idle: every repetition from a fresh episode, so that no env finishes
                    m, fin[v] = run(env, v, steps)
                    ms[v].append(m)
        out[name] = {v: _summary(N, steps, ms[v]) for v in envs}
        out[name]['finished_on_last_step'] = fin
        w = out[name]['wave_fused']['us_per_step']
        for other in ('wave_loop', 'lane_fused'):
            o = out[name][other]['us_per_step']
            out[name]['%s_over_wave_fused' % other] = round(o['median'] / w['median'], 3)
            out[name]['%s_spread_us' % other] = round(o['max'] - o['min'], 2)
            out[name]['wave_fused_wins_beyond_%s_spread' % other] = bool(o['median'] - w['median'] > o['max'] - o['min'])
        del envs
    return out


def bench_device_noise(eng, N, steps, K, warmup, reps):
    """One size: the device generator against the table path, step(auto) and rollout(actor, K), every env live, 1 / 64 of them finishing per step."""
    dev = eng.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    actor = serl50_policy(dev)
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    w = torch.zeros(1, 3716, dtype=torch.float32, device=dev)
    w[0, :3715] = torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', 'actors.npz'))['serl50'][18]).to(dev)
    L = 64
    table = np.ascontiguousarray(rs.tabulate(*rs.base_reference(20), 20)[:L])
    assert steps % K == 0 and warmup % K == 0
    out = dict(N=N, steps=steps, K=K, reps=reps, warmup=warmup, episode_steps=L, table_bytes=N * (L + 1) * 7 * 8)

    def make(v):
        if v == 'device':
            return serl_amd.CitationVecEnv(N, mode='noise', t_max=20, refs=table, engine=eng, auto_reset=True, sensor_noise='device', seed=1)
        g = torch.Generator(device=dev).manual_seed(2)
        z = torch.randn(N, L + 1, 7, generator=g, dtype=torch.float64, device=dev)
        bias, scale = (torch.from_numpy(a).to(dev) for a in serl_amd.builds.sensor_bias_scale())
        return serl_amd.CitationVecEnv(N, mode='noise', t_max=20, refs=table, engine=eng, auto_reset=True, sensor_noise=bias + scale * z)

    def run(env, v, what, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if what == 'step_auto':
            for _ in range(n):
                env.step(fixed)
        elif what == 'rollout':
            for _ in range(n // K):
                env.rollout(w, K, spec=spec)
        else:      # rollout with exploration noise: drawn in the kernel, or a torch draw and clamp per call as the caller of the table path writes them
            for _ in range(n // K):
                if v == 'device':
                    env.rollout(w, K, spec=spec, action_noise='device', noise_sd=0.3, noise_clip=0.5)
                else:
                    env.rollout(w, K, spec=spec, action_noise=torch.clamp(0.3 * torch.randn(K, N, 3, dtype=torch.float64, device=dev), -0.5, 0.5))
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for what in ('step_auto', 'rollout', 'rollout_action_noise'):
        envs = {v: make(v) for v in ('device', 'table')}
        ms = {v: [] for v in envs}
        with torch.no_grad():
            for v, env in envs.items():
                _stagger(env, L, fixed)
                run(env, v, what, warmup)
            for r in range(reps):
                for v, env in (list(envs.items()) if r % 2 == 0 else list(envs.items())[::-1]):      # alternate the order
                    ms[v].append(run(env, v, what, steps))
        out[what] = dict(device=_summary(N, steps, ms['device']), table=_summary(N, steps, ms['table']))
        a, m = out[what]['device']['us_per_step'], out[what]['table']['us_per_step']
        out[what]['device_over_table_us_per_step'] = round(a['median'] / m['median'], 4)
        del envs
    return out


def bench_noise_reset(eng, N):
    """wall time and noise-table bytes of one full reset() of N envs at t_max = 20 (2 001 steps), mode 'noise', shared table references"""
    import time
    table = rs.tabulate(*rs.base_reference(20), 20)
    out = dict(N=N, t_max=20, max_steps=len(table))
    for v in ('device', 'table'):
        kw = dict(sensor_noise='device', seed=1) if v == 'device' else {}
        env = serl_amd.CitationVecEnv(N, mode='noise', t_max=20, refs=table, engine=eng, auto_reset=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.reset()
        torch.cuda.synchronize()
        out[v] = dict(reset_wall_s=round(time.perf_counter() - t0, 4), noise_table_bytes=0 if env._noise is None else env._noise.numel() * 8,
                      host_normals_drawn=0 if env._noise is None else env._noise.numel())
        del env
        torch.cuda.empty_cache()
    return out


def kernel_report(stem='rollout_%s.o', noise_twins=False):
    """noise_twins: the unit holds a kernel and its SERL_VENV_NOISE twin: the twin's record gets a key of its own"""
    rep = {}
    for v in ('nominal', 'ice', 'cg_timed', 'gust', 'test'):
        obj = os.path.join(ROOT, 'serl_amd', 'csrc', 'build', stem % v)
        try:
            r = subprocess.run(['bash', os.path.join(ROOT, 'tools', 'kernel_regs.sh'), obj, 'venv'], capture_output=True, text=True, timeout=120)
        except Exception as ex:
            return {'error': str(ex)[:200]}
        for line in r.stdout.splitlines():
            if '.name:' not in line:
                continue
            f = dict(p.strip().split(': ', 1) for p in line.split('\t') if ': ' in p)
            name = f['.name'].strip()
            kind = ('rollout_general' if 'venv_rollout_general' in name else 'rollout' if 'venv_rollout' in name else 'step_auto' if 'step_auto' in name
                    else 'step' if 'step' in name else 'reset')
            if noise_twins and '_noise_' in name:
                kind += '_noise'
            rep['%s_%s' % (kind, v)] = dict(vgpr=int(f['.vgpr_count']), vgpr_spill=int(f['.vgpr_spill_count']), sgpr_spill=int(f['.sgpr_spill_count']),
                                            lds_bytes=int(f['.group_segment_fixed_size']), scratch_bytes=int(f['.private_segment_fixed_size']))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1024,8192,65536')
    ap.add_argument('--steps', type=int, default=2001)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--no-fused', action='store_true')
    ap.add_argument('--auto-reset', action='store_true', help='the auto-reset leg instead of the others')
    ap.add_argument('--auto-steps', type=int, default=1000)
    ap.add_argument('--drawn-steps', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--drawn-max-n', type=int, default=8192, help='largest N of the drawn comparison')
    ap.add_argument('--rollout', action='store_true', help='the rollout leg instead of the others')
    ap.add_argument('--rollout-k', type=int, default=50, help='steps per rollout() call')
    ap.add_argument('--hidden', default=None, help='--rollout: hidden size(s) of another actor shape, e.g. 72,96 (default: the SERL50 actor, hidden 32)')
    ap.add_argument('--layers', type=int, default=3, help='--rollout --hidden: hidden layers')
    ap.add_argument('--path', default='fused', choices=['auto', 'fused', 'loop'], help="--rollout --hidden: rollout(path=...) of the version compared with 'loop'")
    ap.add_argument('--device-noise', action='store_true', help='the device-noise leg instead of the others')
    ap.add_argument('--reset-n', type=int, default=65536, help='--device-noise: envs of the full-reset measurement at t_max = 20 (0: skip)')
    ap.add_argument('--kernel', default=None, help="the kernel-family leg instead of the others: 'lane,wave' (the comparison), 'lane' or 'wave'")
    ap.add_argument('--out', default=None, help='default: profiles/venv_auto_timing.json (--auto-reset), profiles/venv_rollout_timing.json (--rollout), '
                                                'profiles/venv_rollout_general_timing.json (--rollout --hidden)')
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', ('venv_rollout_general_timing.json' if args.hidden else 'venv_rollout_timing.json') if args.rollout
                                else 'venv_auto_timing.json')
    eng = serl_amd.RolloutEngine(0)
    if args.rollout and args.kernel is not None:
        if args.kernel != 'wave':
            ap.error("--rollout --kernel: 'wave' (the wave rollout leg)")
        if args.out.endswith('venv_rollout_timing.json') or args.out.endswith('venv_rollout_general_timing.json'):
            args.out = os.path.join(ROOT, 'profiles', 'venv_rollout_wave_timing.json')
        sizes = [int(s) for s in (args.sizes if args.sizes != ap.get_default('sizes') else '1,16,64,256,1024,4096').split(',')]
        steps = args.auto_steps if args.auto_steps != ap.get_default('auto_steps') else 500
        shapes = [int(h) for h in args.hidden.split(',')] if args.hidden else [None, 72]      # the SERL50 actor and hidden 72 x 3
        res = dict(tool='bench_venv --rollout --kernel wave', device=torch.cuda.get_device_name(0), source_hash=hip_build.source_hash(),
                   results=[bench_rollout_wave(eng, N, steps, args.rollout_k, args.warmup, args.reps, H, args.layers) for H in shapes for N in sizes])
        kernels_rep = kernel_report('rollout_venvwr_%s.o', noise_twins=True)      # (needs the build's objects: empty where only the library was shipped)
        if kernels_rep:
            res['kernels'] = kernels_rep
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return
    if args.kernel is not None:
        kernels = args.kernel.split(',')
        if not kernels or any(k not in ('lane', 'wave') for k in kernels) or len(set(kernels)) != len(kernels):
            ap.error("--kernel: 'lane', 'wave' or 'lane,wave'")
        if args.out.endswith('venv_auto_timing.json'):
            args.out = os.path.join(ROOT, 'profiles', 'venv_wave_timing.json')
        sizes = [int(s) for s in (args.sizes if args.sizes != ap.get_default('sizes') else '1,16,64,256,1024,4096,65536').split(',')]
        res = dict(tool='bench_venv --kernel %s' % args.kernel, device=torch.cuda.get_device_name(0), source_hash=hip_build.source_hash(),
                   results=[bench_kernels(eng, N, args.auto_steps, args.warmup, args.reps, kernels) for N in sizes])
        if len(kernels) == 2:
            res['wave_max_envs'] = wave_max_envs(res['results'])
        kernels_rep = kernel_report('rollout_venvw_%s.o')      # (needs the build's objects: empty where only the library was shipped)
        if kernels_rep:
            res['kernels'] = kernels_rep
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return
    if args.device_noise:
        if args.out.endswith('venv_auto_timing.json'):
            args.out = os.path.join(ROOT, 'profiles', 'venv_device_noise_timing.json')
        sizes = [int(s) for s in (args.sizes if args.sizes != ap.get_default('sizes') else '1024,65536').split(',')]
        res = dict(tool='bench_venv --device-noise', device=torch.cuda.get_device_name(0), source_hash=hip_build.source_hash(),
                   results=[bench_device_noise(eng, N, args.auto_steps, args.rollout_k, args.warmup, args.reps) for N in sizes])
        kernels = kernel_report('rollout_lanenz_%s.o')      # (needs the build's objects: empty where only the library was shipped)
        if kernels:
            res['kernels'] = kernels

        def write():
            with open(args.out, 'w') as f:
                json.dump(res, f, indent=1)
                f.write('\n')
        write()      # (the timings first: the table path's full reset below draws 0.9 G normals on the host)
        if args.reset_n > 0:
            res['full_reset'] = bench_noise_reset(eng, args.reset_n)
            write()
        print(json.dumps(res))
        return
    if args.rollout:
        sizes = [int(s) for s in (args.sizes if args.sizes != ap.get_default('sizes') else '1024,65536').split(',')]
        res = dict(tool='bench_venv --rollout', device=torch.cuda.get_device_name(0), source_hash=hip_build.source_hash(),
                   results=[bench_rollout(eng, N, args.auto_steps, args.rollout_k, args.warmup, args.reps, H, args.layers, args.path)
                            for H in ([int(h) for h in args.hidden.split(',')] if args.hidden else [None]) for N in sizes])
        if args.hidden:
            res['tool'] += ' --hidden %s --layers %d --path %s' % (args.hidden, args.layers, args.path)
        kernels = kernel_report()      # (needs the build's objects: empty where only the library was shipped)
        if kernels:
            res['kernels'] = kernels
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return
    if args.auto_reset:
        sizes = [int(s) for s in (args.sizes if args.sizes != ap.get_default('sizes') else '1024,65536').split(',')]
        res = dict(tool='bench_venv --auto-reset', device=torch.cuda.get_device_name(0), source_hash=hip_build.source_hash(),
                   results=[bench_auto(eng, N, args.auto_steps, args.warmup, args.reps, args.drawn_steps, args.drawn_max_n) for N in sizes])
        kernels = kernel_report()      # (needs the build's objects: empty where only the library was shipped)
        if kernels:
            res['kernels'] = kernels
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        print(json.dumps(res))
        return
    ref = rs.tabulate(*rs.base_reference(20), 20)
    policy = serl50_policy(eng.device)
    res = []
    for N in (int(s) for s in args.sizes.split(',')):
        res.append(bench_env(eng, N, args.steps, args.warmup, ref))
        res.append(bench_env(eng, N, args.steps, args.warmup, ref, policy))
        if not args.no_fused:
            res.append(bench_fused(eng, N, ref, args.warmup))
    print(json.dumps(dict(tool='bench_venv', device=torch.cuda.get_device_name(0), steps=args.steps, results=res, kernels=kernel_report())))


if __name__ == '__main__':
    main()

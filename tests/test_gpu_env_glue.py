"""The env-step glue of every kernel on the scenarios of tests/env_glue.py, at ZERO tolerance against the literal Python env (the glue is a
few IEEE f64 / f32 operations with contraction off; the dynamics is bit-identical to the same-libm oracle the Python env steps).

Fused rollouts: every hint of FAMILIES_OF_HINT and the lane kernels (64 per wavefront) on the attitude task, teamx / wavex on the other
configurations (serl_capi.hip: `general_env` accepts the TEAM and WAVE hints only), the family asserted by kernel() / ran().  One launch
carries the scenarios of one build and configuration as separate episodes (h2000_v90 attitude: the three long flights in a launch of
their own), each with its own zero-weight actor (the output bias is the scenario's), action-noise row and sensor-noise row.
CitationVecEnv: step, step with auto_reset, rollout(path='fused') on the 7-32-3 actor and on a 7-16-3 one-layer actor (the general kernel;
the other configurations: only the general kernel), one env per scenario.

A launch has one table length, so a scenario whose table is shorter is flown on its table padded with zeros -- by the kernel and by the
Python env alike (env_glue.fly of the padded scenario, cached): it ends where the padded flight ends."""
import numpy as np
import pytest
import torch
import env_glue as G
from test_gpu_rollout import kernel, ran, FAMILIES_OF_HINT, _spec

pytestmark = pytest.mark.gpu
MODE_OF_BUILD = {'h2000_v90': 'nominal', 'cg_timed': 'cg-timed', 'gust': 'gust', 'test': 'test', 'ice': 'ice'}
CFG_NAME = {G.ATTITUDE: 'attitude', G.SYMMETRIC: 'symmetric', G.FULL: 'full'}
LONG = 450      # flights longer than this many steps fly in a launch of their own


def _np(t):
    return t.cpu().numpy()


def _groups(pred=lambda s: True, extra=lambda s: ()):
    """scenarios by (build, config, incremental, long) + extra(s) -> {key: [scenario]}"""
    out = {}
    for s in G.scenarios():
        if pred(s):
            out.setdefault((s['build'], s['config'], s['incremental'], len(s['ref']) > LONG) + tuple(extra(s)), []).append(s)
    return out


def _id(key):
    return '-'.join([key[0], CFG_NAME[key[1]]] + (['incr'] if key[2] else []) + (['long'] if key[3] else []) + [str(k) for k in key[4:]])


_PADDED = {}


def _expected(sc, T):
    """(the scenario on its table padded with zero rows to T, its flight by the Python env): flown once, shared, never changed.  A dict that is not
    one of G.scenarios() (a changed copy under a name of its own) is flown by G.fly as it is."""
    if (sc['name'], T) not in _PADDED:
        n = len(sc['ref'])
        stock = any(s is sc for s in G.scenarios())      # (the cache is keyed by name: a changed copy under a stock name would get, or leave, the wrong flight)
        assert stock or sc['name'] not in [s['name'] for s in G.scenarios()], 'a changed copy of %s needs a name of its own' % sc['name']
        if n == T:
            _PADDED[sc['name'], T] = sc, (G.flown(sc['name']) if stock else G.fly(sc))
        else:
            def pad(a, rows):
                return None if a is None else np.concatenate([a, np.zeros((rows - len(a),) + a.shape[1:], a.dtype)])
            p = dict(sc, ref=pad(sc['ref'], T), sensor_noise=pad(sc['sensor_noise'], T + 1))
            for k in ('noise', 'act32', 'act64'):
                if k in sc:
                    p[k] = pad(sc[k], T)
            if sc['name'] == 'bias_actor':
                p['act32'] = np.tile(sc['actor_out'], (T, 1))
            _PADDED[sc['name'], T] = p, G.fly(p)
    return _PADDED[sc['name'], T]


def _weights(scs, S, A, H, L):
    """one zero-weight actor per scenario: it outputs det_tanhf(bias) whatever it observes"""
    from oracle import rollout as R
    w = np.zeros((len(scs), (R.param_count(S, H, L, A) + 3) // 4 * 4), np.float32)
    P = R.param_count(S, H, L, A)
    for e, s in enumerate(scs):
        if 'bias' in s:
            w[e, P - A:P] = s['bias'][:A]
    return w


def _sensor(scs, T):
    """(table [rows, T + 1, 7], row of each scenario or -1)"""
    rows, idx = [], []
    for s in scs:
        idx.append(len(rows) if s['sensor_noise'] is not None else -1)
        if s['sensor_noise'] is not None:
            rows.append(s['sensor_noise'])
    return (np.stack(rows) if rows else None), np.array(idx, np.int32)


# ---- fused rollouts --------------------------------------------------------------------------------------------------------------------
FUSED = _groups(lambda s: s['fused'], extra=lambda s: (s['t_max'],))      # (t_max is the launch's)
ATT_KERNELS = sorted(FAMILIES_OF_HINT) + [64]
FUSED_CASES = [(key, kern) for key in FUSED for kern in (ATT_KERNELS if (key[1], key[2]) == (G.ATTITUDE, False) else ['team', 'wave'])]


@pytest.mark.parametrize('key,kern', FUSED_CASES, ids=['%s-%s' % (_id(k), kn) for k, kn in FUSED_CASES])
def test_fused_rollout_families_on_the_scenarios(engine, key, kern):
    build, cfg, incr, _, t_max = key

    def check_ran(eng):      # (what the kernel() block asserts on its way out, here right behind the launch)
        if isinstance(kern, int):
            ran(eng, 'lane', episodes_per_team=kern)
        else:
            ran(eng, *sorted(FAMILIES_OF_HINT[kern]))
        if (cfg, incr) != (G.ATTITUDE, False):
            ran(eng, 'teamx' if kern == 'team' else 'wavex')

    with kernel(kern, engine):
        fused_case(engine, FUSED[key], build, cfg, incr, t_max, dict(lanes_per_wave=kern if isinstance(kern, int) else 0), check_ran, what=str(kern))


def fused_case(eng, scs0, build, cfg, incr, t_max, launch_kw, check_ran, H=32, L=3, what=''):
    """ONE launch of `eng` that flies the scenarios `scs0` as its episodes 0, 1, ... in the order given.  A scenario may come more than once: every
    episode has its own zero-weight S-HxL-A actor row, action-noise row and sensor-noise row, and flies on its table padded to the longest.
    launch_kw: further keywords of RolloutEngine.rollout (kernel, lanes_per_wave); check_ran(eng) asserts WHAT was launched, right behind the launch.
    Every episode is compared at ZERO tolerance with env_glue.fly of its padded scenario: length, states, executed command, rewards, transitions,
    fitness, length_t, cost_steps.  -> the launch's outputs as arrays"""
    T = max(len(s['ref']) for s in scs0)
    pairs = [_expected(s, T) for s in scs0]
    scs = [p for p, _ in pairs]
    E = len(scs)
    S, A = scs[0]['S'], scs[0]['A']
    net = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation='tanh')
    noise_rows = [s['noise'] for s in scs if s['kind'] == 'noise']
    noise_idx, j = [], 0
    for s in scs:
        noise_idx.append(j if s['kind'] == 'noise' else -1)
        j += s['kind'] == 'noise'
    sn, sn_idx = _sensor(scs, T)
    kw = dict(build=build, faults=np.array([G.fault_row(s['fault']) for s in scs]), t_max=t_max, traces=True, transitions=True, sync=False,
              env_config=cfg, incremental=incr,
              err0=np.array([s['err0'] or [0.0, 0.0, 0.0] for s in scs]), tick0=np.array([s['tick0'] or 0 for s in scs]))
    if noise_rows:
        kw.update(action_noise=np.stack(noise_rows), noise_row=np.array(noise_idx, np.int32))
    if sn is not None:
        kw.update(sensor_noise=sn, sensor_row=sn_idx)
    kw.update(launch_kw)
    out = eng.rollout(torch.from_numpy(_weights(scs, S, A, H, L)), _spec(net), np.arange(E), np.stack([s['ref'] for s in scs]), **kw)
    check_ran(eng)
    out = {k: _np(v) for k, v in out.items() if torch.is_tensor(v)}
    got = [{k: v[e] for k, v in out.items()} for e in range(E)]
    for e, (s, o) in enumerate(pairs):
        g, n, ep = got[e], o['n'], '%s episode %d %s' % (what, e, s['name'])
        assert g['length_steps'] == o['length_steps'], '%s: length %d, the Python env %d' % (ep, g['length_steps'], o['length_steps'])
        np.testing.assert_array_equal(g['states'][:n], o['states'], err_msg=ep + ': states')
        np.testing.assert_array_equal(g['actions'][:n, :A], o['actions'][:, :A], err_msg=ep + ': executed command')
        np.testing.assert_array_equal(g['rewards'][:n], o['rewards'], err_msg=ep + ': rewards')
        np.testing.assert_array_equal(g['transitions'][:n], o['transitions'], err_msg=ep + ': transitions')
        assert g['fitness'] == o['fitness'], '%s: fitness %r, the Python env %r' % (ep, g['fitness'], o['fitness'])
        assert g['length_t'] == o['length_t'] and g['cost_steps'] == o['cost_steps'], ep
    return out


# ---- CitationVecEnv --------------------------------------------------------------------------------------------------------------------
def _make_env(engine, key, scs, T, auto, kernel='lane'):
    import serl_amd
    build, cfg, incr = key[:3]
    mode = 'PHlab_%s_%s' % (CFG_NAME[cfg], 'incremental' if incr else MODE_OF_BUILD[build])
    assert not incr or build == 'h2000_v90'
    N = len(scs)
    sn = np.stack([s['sensor_noise'] if s['sensor_noise'] is not None else np.zeros((T + 1, 7)) for s in scs])
    with_noise = any(s['sensor_noise'] is not None for s in scs) or build == 'gust'
    env = serl_amd.CitationVecEnv(N, mode=mode, t_max=scs[0]['t_max'], engine=engine, refs=np.stack([s['ref'] for s in scs]),
                                  sensor_noise=sn if with_noise else False, auto_reset=auto, kernel=kernel)
    assert (env.build, env.env_config, env.incremental, env.max_steps) == (build, cfg, incr, T)
    assert env._faults is None      # per-env fault rows: the descriptor's table, set as the constructor sets it for a fault mode
    env._faults = torch.from_numpy(np.array([G.fault_row(s['fault']) for s in scs])).to(env.device).contiguous()
    env.desc.faults = env._faults.data_ptr()
    obs0 = _np(env.reset(err0=np.array([s['err0'] or [0.0, 0.0, 0.0] for s in scs]), tick0=np.array([s['tick0'] or 0 for s in scs])))
    assert env.last_step_kernel == kernel
    return env, obs0


def _restart_obs(s, o):
    """obs0 of the episode an auto-reset starts: the error stays, the clock has ticked once per reset and once per step"""
    env = G.GlueEnv(s['build'], s['config'], s['incremental'], s['fault'], s['ref'], s['sensor_noise'], s['t_max'], err0=o['err'],
                    tick0=(s['tick0'] or 0) + 1 + o['n'])
    return np.array(env.reset())


def _act_exec(s, T, A):
    """the action of every step as the step kernels are fed it: f32 as it is; f64 = the clipped sum of actor output and noise, or the script"""
    if s['kind'] == 'f32':
        return s['act32'][:T, :A]
    if s['kind'] == 'f64':
        return s['act64'][:T, :A]
    return np.clip(s['actor_out'][None, :A].astype(np.float64) + s['noise'][:T, :A], -1.0, 1.0)


STEP = _groups(extra=lambda s: (s['t_max'], 'f32' if s['kind'] == 'f32' else 'f64'))


@pytest.mark.parametrize('auto', [False, True], ids=['step', 'auto'])
@pytest.mark.parametrize('key', list(STEP), ids=[_id(k) for k in STEP])
def test_env_step_kernels_on_the_scenarios(engine, key, auto):
    step_case(engine, key, auto)


def step_case(engine, key, auto, kernel='lane'):
    """the scenarios of STEP[key] through step() of an env of the `kernel` family, one env per scenario -> the env behind its last step"""
    scs0 = STEP[key]
    T = max(len(s['ref']) for s in scs0)
    pairs = [_expected(s, T) for s in scs0]
    scs = [p for p, _ in pairs]
    N, S, A = len(scs), scs0[0]['S'], scs0[0]['A']
    env, obs0 = _make_env(engine, key, scs, T, auto, kernel)
    dev = env.device
    acts = torch.from_numpy(np.ascontiguousarray(np.stack([_act_exec(s, T, A) for s in scs], axis=1))).to(dev)      # [T, N, A]
    assert acts.dtype == (torch.float32 if key[-1] == 'f32' else torch.float64)
    K = T + 2
    f64 = dict(dtype=torch.float64, device=dev)
    rec = {'obs': torch.zeros(K, N, S, **f64), 'reward': torch.zeros(K, N, **f64), 'done': torch.zeros(K, N, dtype=torch.bool, device=dev),
           'x': torch.zeros(K, N, 12, **f64), 'ref': torch.zeros(K, N, 3, **f64), 't': torch.zeros(K, N, **f64),
           'cost': torch.zeros(K, N, dtype=torch.int32, device=dev)}
    if auto:
        rec.update(final_obs=torch.zeros(K, N, S, **f64), episode_return=torch.zeros(K, N, **f64),
                   episode_length=torch.zeros(K, N, dtype=torch.int32, device=dev))
    zero = torch.zeros(N, A, dtype=acts.dtype, device=dev)
    for k in range(K):
        obs, rew, done, info = env.step(acts[k] if k < T else zero)
        rec['obs'][k].copy_(obs); rec['reward'][k].copy_(rew); rec['done'][k].copy_(done)
        for name in rec:
            if name in info:
                rec[name][k].copy_(info[name])
    assert env.last_step_kernel == kernel
    rec = {k: _np(v) for k, v in rec.items()}
    for e, (s, o) in enumerate(pairs):
        n, what = o['n'], '%s env %d %s' % ('auto' if auto else 'step', e, s['name'])
        np.testing.assert_array_equal(obs0[e], o['obs0'], err_msg=what + ': obs0')
        np.testing.assert_array_equal(rec['x'][:n, e], o['states'], err_msg=what + ': x')
        np.testing.assert_array_equal(rec['reward'][:n, e], o['rewards'], err_msg=what + ': reward')
        np.testing.assert_array_equal(rec['cost'][:n, e], o['cost'], err_msg=what + ': cost')
        np.testing.assert_array_equal(rec['ref'][:n, e], o['refs'], err_msg=what + ': ref')
        np.testing.assert_array_equal(rec['t'][:n, e], o['t'], err_msg=what + ': t')
        d = rec['done'][:, e]
        assert not d[:n - 1].any() and d[n - 1], '%s: done first rises at step %d, not %d' % (what, int(np.argmax(d)), n - 1)
        terminal = rec['final_obs'] if auto else rec['obs']
        np.testing.assert_array_equal(terminal[:n, e], o['obs'], err_msg=what + ': observation')
        if auto:
            np.testing.assert_array_equal(rec['obs'][:n - 1, e], o['obs'][:n - 1], err_msg=what + ': observation')
            assert rec['episode_return'][n - 1, e] == o['fitness'] and rec['episode_length'][n - 1, e] == n, what
            np.testing.assert_array_equal(rec['obs'][n - 1, e], _restart_obs(s, o), err_msg=what + ': obs0 of the restarted episode')
        else:      # frozen behind done
            assert d[n - 1:].all() and (rec['reward'][n:, e] == 0.0).all(), what
            np.testing.assert_array_equal(rec['obs'][n:, e], np.tile(o['obs'][-1], (K - n, 1)), err_msg=what + ': frozen')
    return env


ROLL = _groups(lambda s: s['fused'], extra=lambda s: (s['t_max'], 'noise' if s['kind'] == 'noise' else 'plain'))
ROLL_CASES = [(key, shape) for key in ROLL for shape in (['lane32', 'general'] if (key[1], key[2]) == (G.ATTITUDE, False) else ['general'])]


@pytest.mark.parametrize('key,shape', ROLL_CASES, ids=['%s-%s' % (_id(k), s) for k, s in ROLL_CASES])
def test_env_rollout_kernels_on_the_scenarios(engine, key, shape):
    roll_case(engine, key, shape)


def roll_case(engine, key, shape, kernel='lane'):
    """the scenarios of ROLL[key] through rollout(path='fused') of an env of the `kernel` family: the 7-32x3-3 actor ('lane32') or the
    one-layer hidden-16 actor ('general'); on a wave env both go through the one wave rollout kernel -> the env behind the launch"""
    import serl_amd
    scs0 = ROLL[key]
    T = max(len(s['ref']) for s in scs0)
    pairs = [_expected(s, T) for s in scs0]
    scs = [p for p, _ in pairs]
    N, S, A = len(scs), scs0[0]['S'], scs0[0]['A']
    env, obs0 = _make_env(engine, key, scs, T, True, kernel)
    H, L = (32, 3) if shape == 'lane32' else (16, 1)
    spec = serl_amd.NetSpec(S, A, H, L, 'tanh')
    K = T + 1
    noise = None
    if key[-1] == 'noise':
        noise = np.zeros((K, N, 3))
        noise[:T] = np.stack([s['noise'] for s in scs], axis=1)
    w = torch.from_numpy(_weights(scs, S, A, H, L)).to(env.device)
    out = env.rollout(w, K, spec=spec, member_of_env=np.arange(N, dtype=np.int32), action_noise=noise, transitions=True, path='fused')
    assert env.last_rollout_path == ('fused-wave' if kernel == 'wave' else 'fused' if shape == 'lane32' else 'fused-general')
    out = {k: _np(v) for k, v in out.items()}
    for e, (s, o) in enumerate(pairs):
        n, what = o['n'], '%s env %d %s' % (shape, e, s['name'])
        np.testing.assert_array_equal(out['obs'][0, e], o['obs0'], err_msg=what + ': obs0')
        np.testing.assert_array_equal(out['x'][:n, e], o['states'], err_msg=what + ': x')
        np.testing.assert_array_equal(out['reward'][:n, e], o['rewards'], err_msg=what + ': reward')
        np.testing.assert_array_equal(out['cost'][:n, e], o['cost'], err_msg=what + ': cost')
        np.testing.assert_array_equal(out['ref'][:n, e], o['refs'], err_msg=what + ': ref')
        np.testing.assert_array_equal(out['t'][:n, e], o['t'], err_msg=what + ': t')
        np.testing.assert_array_equal(out['final_obs'][:n, e], o['obs'], err_msg=what + ': observation')
        np.testing.assert_array_equal(out['obs'][1:n, e], o['obs'][:n - 1], err_msg=what + ': observation')
        np.testing.assert_array_equal(out['transitions'][:n, e], o['transitions'], err_msg=what + ': transitions')
        np.testing.assert_array_equal(out['actions'][:n, e].astype(np.float32), o['transitions'][:, S:S + A], err_msg=what + ': action')
        d = out['done'][:, e]
        assert not d[:n - 1].any() and d[n - 1], '%s: done first rises at step %d, not %d' % (what, int(np.argmax(d)), n - 1)
        assert out['ep_return'][n - 1, e] == o['fitness'] and out['ep_length'][n - 1, e] == n, what
        np.testing.assert_array_equal(out['obs'][n, e], _restart_obs(s, o), err_msg=what + ': obs0 of the restarted episode')
    return env

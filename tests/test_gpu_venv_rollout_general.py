"""K policy-driven env steps in one launch for every env configuration and actor shape (C ABI serl_venv_rollout_general,
CitationVecEnv.rollout(path='fused')) on the GPU, at ZERO tolerance.

The yardsticks are the ones of tests/test_gpu_venv_rollout.py: a twin auto-reset env that is fed the recorded actions through `step`,
the fused team / wave rollout kernels (engine.rollout) on the same env configuration, and the CPU oracle for the in-kernel forward pass.
Episodes are six steps (t_max = 0.05 s, table references), so restarts fall inside every segment; K <= 15."""
import ctypes
import numpy as np
import pytest
import torch

from actor_shapes import make_weights, _shape, spec_of, ATTITUDE, SYMMETRIC, FULL

pytestmark = pytest.mark.gpu
T_SHORT = 0.05
KEYS = ('reward', 'done', 'final_obs', 'x', 'ref', 't', 'cost')
DEG = 3.14159265358979323846 / 180.0

# the covering subset of the actor shapes: hidden sizes with one, several and a partial last group of sixteen columns / LayerNorm rows,
# no hidden layer and sixteen, every activation, and one shape per env configuration other than the plain attitude task
ATT_SHAPES = ([_shape(H, 3) for H in (4, 20, 72, 96, 128)] + [_shape(12, 0), _shape(128, 0), _shape(8, 16), _shape(100, 3)]
              + [_shape(72, 3, 'elu'), _shape(72, 3, 'relu')])
CFG_SHAPES = [_shape(32, 2, 'elu', ATTITUDE, True), _shape(12, 2, 'tanh', SYMMETRIC), _shape(8, 1, 'tanh', SYMMETRIC, True),
              _shape(72, 3, 'relu', FULL), _shape(48, 3, 'tanh', FULL, True)]
SHAPES = ATT_SHAPES + CFG_SHAPES
S72 = _shape(72, 3)


def _sid(s):
    return '%s%s_H%d_L%d_%s' % (('att', 'sym', 'full')[s['env_config']], '_inc' if s['incremental'] else '', s['hidden'], s['num_layers'],
                                s['activation'])


def _mode_of(s, mode='nominal'):
    if s['env_config'] == ATTITUDE and not s['incremental']:
        return mode
    assert mode == 'nominal'
    return 'PHlab_%s_%s' % (('attitude', 'symmetric', 'full')[s['env_config']], 'incremental' if s['incremental'] else 'nominal')


def _venv(n, mode, engine, **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(n, mode=mode, t_max=T_SHORT, engine=engine, auto_reset=True, **kw)


def _tables(N, seed):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rs.n_steps_for(T_SHORT)])
    assert np.isfinite(r).all() and r.shape[1] == 6
    return r


def _env_kw(mode, N):
    from serl_amd import builds, refsignals as rs
    kw = {'refs': _tables(N, 41)}
    if builds.has_sensor_noise(mode):
        T = rs.n_steps_for(T_SHORT)
        kw['sensor_noise'] = np.stack([builds.sensor_noise_table(T, np.random.RandomState(300 + e)) for e in range(N)])
    return kw


def _noise(K, N, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(K, N, 3, generator=g, dtype=torch.float64) * 0.4      # wide enough for the clip at +-1 to bite


def _np(t):
    return t.cpu().numpy()


def _follow(twin, out, f64):
    """Feed the recorded actions of a rollout to `twin` through step() and compare every output of every step."""
    K = out['reward'].shape[0]
    rec = []
    for k in range(K):
        a = out['actions'][k]
        obs, rew, done, info = twin.step(a if f64 else a.float())
        r = {'obs': obs.clone(), 'reward': rew.clone(), 'done': done.clone(), 'final_obs': info['final_obs'].clone(),
             'ep_return': info['episode_return'].clone(), 'ep_length': info['episode_length'].clone()}
        for key in ('x', 'ref', 't', 'cost'):
            r[key] = info[key].clone()
        rec.append(r)
    tw = {k: np.stack([_np(r[k]) for r in rec]) for k in rec[0]}
    o = {k: _np(v) for k, v in out.items()}
    np.testing.assert_array_equal(o['obs'][1:], tw['obs'], err_msg='obs')
    for k in KEYS:
        np.testing.assert_array_equal(o[k], tw[k], err_msg=k)
    done = tw['done']
    np.testing.assert_array_equal(o['ep_return'][done], tw['ep_return'][done])
    np.testing.assert_array_equal(o['ep_length'][done], tw['ep_length'][done])
    assert (o['ep_return'][~done] == 0).all() and (o['ep_length'][~done] == 0).all()
    return o


def _same_state(a, b):
    for name in ('_state', '_run_return', '_run_length', '_cursor', '_ep_return', '_ep_length'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def _stagger(envs):
    """reset all, two steps, reset every third env: phases spread over the envs, identically for all `envs`"""
    N, A, dev = envs[0].n_envs, envs[0].action_dim, envs[0].device
    g = torch.Generator(device='cpu').manual_seed(7)
    acts = ((torch.rand(2, N, A, generator=g) * 2 - 1) * 0.6).to(dev)
    third = torch.arange(N, device=dev) % 3 == 0
    obs = []
    for env in envs:
        env.reset()
        env.step(acts[0]); env.step(acts[1])
        obs.append(env.reset(third).clone())
    for o in obs[1:]:
        assert torch.equal(o, obs[0])
    return obs[0]


def _weights(s, n, seed, dev):
    return torch.from_numpy(np.ascontiguousarray(make_weights(s, n, seed))).to(dev)


# ---- 1. against step() on a twin env --------------------------------------------------------------------------------------------------
def _twin_case(engine, s, mode, noisy, N=70, segments=(1, 5, 15), moe_of=3):
    kw = _env_kw(mode, N)
    env, twin = _venv(N, mode, engine, **kw), _venv(N, mode, engine, **kw)
    S, A, dev = s['state_dim'], s['action_dim'], env.device
    assert (env.state_dim, env.action_dim) == (S, A)
    obs0 = _stagger([env, twin])
    M = moe_of or 1
    w = _weights(s, M, 21, dev)
    moe = (torch.arange(N, dtype=torch.int32, device=dev) % M) if moe_of else None
    ends = 0
    for i, K in enumerate(segments):
        noise = _noise(K, N, 50 + i).to(dev) if noisy else None
        out = env.rollout(w, K, spec=spec_of(s), member_of_env=moe, action_noise=noise, transitions=True, path='fused')
        assert env.last_rollout_path == 'fused-general'
        assert out['obs'].shape == (K + 1, N, S) and out['actions'].shape == (K, N, A) and out['done'].dtype == torch.bool
        assert out['transitions'].shape == (K, N, 2 * S + A + 3)
        assert torch.equal(out['obs'][0], obs0)
        o = _follow(twin, out, f64=noisy)
        _same_state(env, twin)
        obs0 = out['obs'][K]
        ends += o['done'].sum(0)
        assert np.isfinite(o['obs']).all() and np.isfinite(o['reward']).all()
        if noisy:
            assert (np.abs(o['actions']) <= 1.0).all() and (K < 15 or (np.abs(o['actions']) == 1.0).any())
    assert (ends >= (2 if sum(segments) >= 15 else 1)).all(), 'an env never restarted'


@pytest.mark.parametrize('noisy', [False, True], ids=['f32', 'noise'])
@pytest.mark.parametrize('mode', ['nominal', 'cg-timed', 'gust'])
def test_rollout_equals_step_on_its_actions(engine, mode, noisy):
    _twin_case(engine, S72, mode, noisy)


@pytest.mark.parametrize('noisy', [False, True], ids=['f32', 'noise'])
@pytest.mark.parametrize('s', CFG_SHAPES, ids=_sid)
def test_rollout_equals_step_in_every_env_configuration(engine, s, noisy):
    _twin_case(engine, s, _mode_of(s), noisy)


# ---- 2. the in-kernel actor and episode against the fused rollout kernels and the oracle ------------------------------------------------
def _fresh_episode(engine, s, w, noisy):
    M, K = len(w), 6
    refs = _tables(M, 61)
    env = _venv(M, _mode_of(s), engine, refs=refs)
    env.reset()
    noise = _noise(K, M, 77) if noisy else None
    out = env.rollout(torch.from_numpy(w).to(env.device), K, spec=spec_of(s), member_of_env=np.arange(M, dtype=np.int32), action_noise=noise,
                      transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-general'
    return refs, noise, {k: _np(v) for k, v in out.items()}


def _commands(s, o, noisy):
    """what the rollout kernels trace as `actions`: the commanded deflections u [K, M, 3] -- the scaled action, integrated over the
    steps of the episode under incremental control (u += rate x 0.01, the kernels' own two roundings)"""
    bound = (25.0 if s['incremental'] else 10.0) * DEG
    a = o['actions']
    if noisy:
        scl = -bound + 0.5 * (a + 1.0) * (bound - -bound)
    else:
        sc = (np.float32(0.5) * (a.astype(np.float32) + np.float32(1.0))).astype(np.float32)
        scl = -bound + sc.astype(np.float64) * (bound - -bound)
    full = np.zeros(a.shape[:2] + (3,))
    full[..., :a.shape[2]] = scl
    if not s['incremental']:
        return full
    u, acc = np.zeros_like(full), np.zeros(full.shape[1:])
    for k in range(len(full)):
        acc = acc + full[k] * 0.01
        u[k] = acc
    return u


@pytest.mark.parametrize('s', SHAPES, ids=_sid)
def test_actor_and_episode_equal_the_fused_kernel_and_the_oracle(engine, s):
    from oracle import rollout as R
    M = 3
    w = np.ascontiguousarray(make_weights(s, M, 33))
    refs, _, o = _fresh_episode(engine, s, w, False)
    kw = dict(t_max=T_SHORT, traces=True, transitions=True, env_config=s['env_config'], incremental=s['incremental'])
    f = engine.rollout(w, spec_of(s), np.arange(M), refs, **kw)
    assert (_np(f['length_steps']) == 6).all() and o['done'][5].all() and not o['done'][:5].any()
    cmds = _commands(s, o, False)
    np.testing.assert_array_equal(o['transitions'].transpose(1, 0, 2), _np(f['transitions']))
    np.testing.assert_array_equal(cmds.transpose(1, 0, 2), _np(f['actions']))
    np.testing.assert_array_equal(o['x'].transpose(1, 0, 2), _np(f['states']))
    np.testing.assert_array_equal(o['reward'].T, _np(f['rewards']))
    np.testing.assert_array_equal(o['ep_return'][5], _np(f['fitness']))
    assert (o['ep_length'][5] == 6).all()
    net = {k: s[k] for k in ('state_dim', 'action_dim', 'hidden', 'num_layers', 'activation')}
    r = R.rollout(w, net, np.arange(M), refs, short_libm=True, threads=1, **kw)
    assert (np.asarray(r['length_steps']) == 6).all()
    np.testing.assert_array_equal(o['transitions'].transpose(1, 0, 2), r['transitions'][:, :6])
    np.testing.assert_array_equal(cmds.transpose(1, 0, 2), r['actions'][:, :6])
    np.testing.assert_array_equal(o['x'].transpose(1, 0, 2), r['states'][:, :6])
    np.testing.assert_array_equal(o['reward'].T, r['rewards'][:, :6])
    a = o['actions']
    assert (np.abs(a) < 1.0).any() and not np.array_equal(a[:, 0], a[:, 1])      # not all saturated, and the members act differently


@pytest.mark.parametrize('s', [S72] + CFG_SHAPES, ids=_sid)
def test_noisy_episode_equals_the_fused_kernel(engine, s):
    M = 3
    w = np.ascontiguousarray(make_weights(s, M, 34))
    refs, noise, o = _fresh_episode(engine, s, w, True)
    f = engine.rollout(w, spec_of(s), np.arange(M), refs, t_max=T_SHORT, traces=True, transitions=True, env_config=s['env_config'],
                       incremental=s['incremental'], action_noise=np.ascontiguousarray(_np(noise).transpose(1, 0, 2)))
    assert (_np(f['length_steps']) == 6).all()
    np.testing.assert_array_equal(o['transitions'].transpose(1, 0, 2), _np(f['transitions']))
    np.testing.assert_array_equal(_commands(s, o, True).transpose(1, 0, 2), _np(f['actions']))
    np.testing.assert_array_equal(o['x'].transpose(1, 0, 2), _np(f['states']))
    np.testing.assert_array_equal(o['reward'].T, _np(f['rewards']))


# ---- 3. more than one lane per wavefront ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N, shared', [(600, False), (600, True), (601, False)], ids=['600-members', '600-shared', '601-members'])
def test_several_lanes_per_wavefront(engine, N, shared):
    """The launch puts ceil(N / 256) envs in a wavefront: three at N = 600 (200 wavefronts) and at 601 (the last wavefront holds one env).
    With member = env % 3 the lanes of a wavefront run three different members; the shared policy runs without member_of_env."""
    _twin_case(engine, S72, 'nominal', False, N=N, segments=(8,), moe_of=0 if shared else 3)


# ---- 4. never-reset envs stay frozen, in a configuration whose rows are not 7 / 3 / 20 wide ----------------------------------------------
def test_never_reset_envs_are_frozen(engine):
    s = _shape(12, 2, 'tanh', SYMMETRIC)
    N, K, S, A = 70, 8, 2, 1
    mode = _mode_of(s)
    kw = _env_kw(mode, N)
    env, twin = _venv(N, mode, engine, **kw), _venv(N, mode, engine, **kw)
    dev = env.device
    mask = torch.arange(N, device=dev) % 2 == 0
    env.reset(mask); twin.reset(mask)
    cold = ~_np(mask)
    npad = (N + 63) // 64 * 64
    fields = lambda e: (_np(e._state[:73 * npad * 8].view(torch.float64).view(73, npad)), _np(e._state[73 * npad * 8:].view(torch.int32).view(17, npad)))
    f0, i0 = fields(env)
    out = env.rollout(_weights(s, 1, 6, dev), K, spec=spec_of(s), transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-general'
    o = _follow(twin, out, f64=False)
    _same_state(env, twin)
    assert o['done'][:, cold].all() and (o['reward'][:, cold] == 0).all() and (o['actions'][:, cold] == 0).all()
    for k in range(K):
        np.testing.assert_array_equal(o['obs'][k + 1][cold], o['obs'][0][cold])
        np.testing.assert_array_equal(o['final_obs'][k][cold], o['obs'][0][cold])
    tr = o['transitions'][:, cold]
    assert tr.shape[-1] == 2 * S + A + 3 == 8
    np.testing.assert_array_equal(tr[..., :S], np.broadcast_to(o['obs'][0][cold].astype(np.float32), tr[..., :S].shape))
    np.testing.assert_array_equal(tr[..., S + A:2 * S + A], tr[..., :S])
    assert (tr[..., S:S + A] == 0).all() and (tr[..., 2 * S + A] == 0).all() and (tr[..., 2 * S + A + 1] == 1).all()
    f1, i1 = fields(env)
    np.testing.assert_array_equal(f1[:, :N][:, cold], f0[:, :N][:, cold])
    np.testing.assert_array_equal(i1[:, :N][:, cold], i0[:, :N][:, cold])
    for name in ('_run_return', '_run_length', '_cursor'):
        assert (_np(getattr(env, name))[cold] == 0).all()
    assert not o['done'][:5, ~cold].any() and o['done'][5, ~cold].all()


# ---- 5. segments chain, and rollout / step share the state -------------------------------------------------------------------------------
def test_segments_chain(engine):
    N, s = 70, S72
    kw = _env_kw('nominal', N)
    a, b, c, d = (_venv(N, 'nominal', engine, **kw) for _ in range(4))
    _stagger([a, b, c, d])
    dev = a.device
    w, spec, moe = _weights(s, 3, 3, dev), spec_of(s), np.arange(N) % 3
    ro = lambda env, K: env.rollout(w, K, spec=spec, member_of_env=moe, transitions=True, path='fused')
    whole, first = ro(a, 15), ro(b, 5)
    for k in range(5):                                               # the other route to the same point: step() on the recorded actions
        c.step(whole['actions'][k].float())
    _same_state(b, c)
    second = ro(b, 10)
    assert a.last_rollout_path == b.last_rollout_path == 'fused-general'
    _same_state(a, b)
    for key in whole:
        joined = torch.cat([first[key], second[key][1:] if key == 'obs' else second[key]])
        assert torch.equal(joined, whole[key]), key
    assert torch.equal(first['obs'][5], second['obs'][0])
    assert _np(whole['done']).sum(0).min() >= 2
    # rollout(5), 3 x step, rollout(7) == rollout(15); the steps equal those of the env that only stepped
    ro(d, 5)
    for k in range(5, 8):
        od, rd, dd, idd = d.step(whole['actions'][k].float())
        oc, rc, dc, ic = c.step(whole['actions'][k].float())
        assert torch.equal(od, oc) and torch.equal(rd, rc) and torch.equal(dd, dc)
        for key in ic:
            assert torch.equal(idd[key], ic[key]), key
        assert torch.equal(od, whole['obs'][k + 1])
    _same_state(d, c)
    tail = ro(d, 7)
    for key in ('obs', 'actions', 'reward', 'done', 'transitions'):
        assert torch.equal(tail[key], whole[key][8:]), key
    _same_state(d, a)


# ---- 6. transition rows feed a ring of the env's widths ------------------------------------------------------------------------------
def test_transition_rows_fill_a_replay_ring(engine):
    from serl_amd.replay import DeviceReplay
    s = _shape(72, 3, 'relu', FULL)
    N, K, S, A = 70, 15, 13, 3
    mode = _mode_of(s)
    env = _venv(N, mode, engine, **_env_kw(mode, N))
    _stagger([env])
    out = env.rollout(_weights(s, 1, 8, env.device), K, spec=spec_of(s), transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-general'
    o = {k: _np(v) for k, v in out.items()}
    W = 2 * S + A + 3
    assert o['transitions'].shape == (K, N, W) and o['done'].any() and not o['done'].all()
    # tables as long as t_max: every episode ends by t >= t_max, done == fin
    want = np.concatenate([o['obs'][:-1].astype(np.float32), o['actions'].astype(np.float32), o['final_obs'].astype(np.float32),
                           o['reward'].astype(np.float32)[..., None], o['done'].astype(np.float32)[..., None],
                           (o['cost'] != 0).astype(np.float32)[..., None]], axis=-1)
    np.testing.assert_array_equal(o['transitions'], want)
    d = o['done']
    assert not np.array_equal(o['transitions'][d][:, S + A:2 * S + A], o['obs'][1:][d].astype(np.float32))
    ring, ring2 = DeviceReplay(2048, env.device, engine, S, A), DeviceReplay(2048, env.device, engine, S, A)
    ring.append_rows(out['transitions'].reshape(-1, W))
    ring2.append_rows(torch.from_numpy(want.reshape(-1, W)))
    assert len(ring) == K * N == len(ring2) and ring.position == ring2.position
    assert torch.equal(ring.rows, ring2.rows)


# ---- 7. the lane-32 kernel keeps its shape; 'loop' is always the loop --------------------------------------------------------------------
def test_path_on_a_hidden_32_attitude_env(engine):
    N, K, s = 70, 15, _shape(32, 3)
    kw = _env_kw('nominal', N)
    a, b, c = (_venv(N, 'nominal', engine, **kw) for _ in range(3))
    _stagger([a, b, c])
    w, spec, moe = _weights(s, 3, 5, a.device), spec_of(s), np.arange(N) % 3
    auto = a.rollout(w, K, spec=spec, member_of_env=moe, transitions=True)
    assert a.last_rollout_path == 'fused'
    fused = b.rollout(w, K, spec=spec, member_of_env=moe, transitions=True, path='fused')
    assert b.last_rollout_path == 'fused'
    assert fused.keys() == auto.keys()
    for key in auto:
        assert torch.equal(fused[key], auto[key]), key
    _same_state(a, b)
    loop = c.rollout(w, K, spec=spec, member_of_env=moe, transitions=True, path='loop')
    assert c.last_rollout_path == 'loop' and loop.keys() == auto.keys()
    assert torch.equal(loop['done'], auto['done']) and loop['obs'].shape == auto['obs'].shape


# ---- 8. bad arguments: a clean error, no launch ------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(engine):
    import serl_amd
    from serl_amd import _capi
    N, s = 4, S72
    env = _venv(N, 'nominal', engine, **_env_kw('nominal', N))
    env.reset()
    dev = env.device
    L, ctx = engine.lib, engine.ctx
    wd = torch.zeros(1, 24000, dtype=torch.float32, device=dev)      # room for every shape below
    out = env._rollout_buffers(3, False, False)
    state0 = env._state.clone()
    run0 = [getattr(env, n).clone() for n in ('_run_return', '_run_length', '_cursor')]

    def rdesc(**over):
        d = dict(state_dim=7, action_dim=3, hidden=72, num_layers=3, activation=0, n_members=1, weights=wd.data_ptr(), weight_stride=wd.shape[1],
                 n_steps=3, obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr())
        d.update(over)
        return _capi.VenvRolloutDesc(**d)

    def call(d, au, rd):
        return L.serl_venv_rollout_general(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), None)
    P = L.serl_param_count(7, 72, 3, 3)
    assert P % 4 == 3 and wd.data_ptr() % 16 == 0
    bad = _capi.E_INVALID, _capi.E_UNSUPPORTED
    for over in (dict(hidden=30), dict(hidden=132), dict(hidden=0), dict(num_layers=17), dict(state_dim=13), dict(state_dim=10), dict(action_dim=1),
                 dict(weight_stride=P - 3), dict(weight_stride=P + 3), dict(weights=wd.data_ptr() + 4), dict(n_steps=0), dict(n_members=0),
                 dict(activation=3), dict(obs=None), dict(weights=None)):
        assert call(env.desc, env.auto_desc, rdesc(**over)) in bad, over
        assert b'serl_venv_rollout_general' in L.serl_last_error()
    assert (P + 3) % 4 == 2
    assert call(env.desc, env.auto_desc, rdesc(hidden=30)) == _capi.E_UNSUPPORTED
    assert call(env.desc, env.auto_desc, rdesc(num_layers=17)) == _capi.E_UNSUPPORTED
    for field in ('cursor', 'run_return', 'run_length'):
        au = _capi.VenvAutoDesc.from_buffer_copy(env.auto_desc)
        setattr(au, field, None)
        assert call(env.desc, au, rdesc()) == _capi.E_INVALID, field
    d = _capi.VenvDesc.from_buffer_copy(env.desc)
    d.build_slot = 63
    assert call(d, env.auto_desc, rdesc()) == _capi.E_INVALID            # behind the descriptor checks: serl_venv_check
    # Python: a shape no kernel takes, an unknown path
    class A30:
        state_dim, action_dim, hidden_size, num_layers, activation_actor = 7, 3, 30, 1, 'tanh'
    with pytest.raises(ValueError, match="path='fused'"):
        env.rollout(serl_amd.Actor(A30()), 3, path='fused')
    with pytest.raises(ValueError, match='path'):
        env.rollout(serl_amd.Actor(A30()), 3, path='bogus')
    torch.cuda.synchronize()
    assert torch.equal(env._state, state0)                           # nothing was launched
    for n, r in zip(('_run_return', '_run_length', '_cursor'), run0):
        assert torch.equal(getattr(env, n), r), n
    # a following good call still matches a twin
    twin = _venv(N, 'nominal', engine, **_env_kw('nominal', N))
    twin.reset()
    _follow(twin, env.rollout(_weights(s, 1, 9, dev), 7, spec=spec_of(s), path='fused'), f64=False)
    assert env.last_rollout_path == 'fused-general'
    _same_state(env, twin)

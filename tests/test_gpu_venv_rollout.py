"""K policy-driven env steps in one launch (C ABI serl_venv_rollout, CitationVecEnv.rollout) on the GPU, at ZERO tolerance.

Three yardsticks, all existing and pinned elsewhere: a twin auto-reset env that is fed the recorded actions through `step`
(tests/test_gpu_venv_auto.py pins it to step + reset(done), tests/test_gpu_venv.py to the oracle), the fused lane / team rollout kernels
(engine.rollout) and the CPU oracle for the in-kernel actor forward.  Episodes are six steps (t_max = 0.05 s) so that restarts fall
inside a segment of 15 steps; the drawn pool needs t_max = 5 (refsignals.training_references has no shorter sequence) and therefore one
long segment across its restart."""
import ctypes
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T_SHORT = 0.05
KEYS = ('reward', 'done', 'final_obs', 'x', 'ref', 't', 'cost')
NET32 = dict(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation='tanh')
BOUND = 10.0 * (3.14159265358979323846 / 180.0)


def _venv(n, mode, t_max, engine, **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(n, mode=mode, t_max=t_max, engine=engine, auto_reset=True, **kw)


def _tables(N, t_max, seed, rows=None):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rows or rs.n_steps_for(t_max)])
    assert np.isfinite(r).all()
    return r


def _actors(n, hidden=32, layers=2, activation='elu', seed=0, device='cpu'):
    """n torch actors of one shape with weights large enough for actions that differ visibly between members"""
    import serl_amd

    class A:
        state_dim, action_dim, hidden_size, num_layers, activation_actor = 7, 3, hidden, layers, activation
    torch.manual_seed(1000 + seed)
    out = []
    for _ in range(n):
        a = serl_amd.Actor(A())
        with torch.no_grad():
            for p in a.parameters():
                if p.dim() == 2:
                    p.mul_(2.0)
        out.append(a.to(device))
    return out


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


def _stagger(envs, seed=None):
    """reset all, two steps, reset every third env: phases spread over the envs, identically for all `envs`"""
    N, dev = envs[0].n_envs, envs[0].device
    g = torch.Generator(device='cpu').manual_seed(7)
    acts = ((torch.rand(2, N, 3, generator=g) * 2 - 1) * 0.6).to(dev)
    third = torch.arange(N, device=dev) % 3 == 0
    obs = []
    for env in envs:
        if seed is not None:
            np.random.seed(seed)
        env.reset()
        env.step(acts[0]); env.step(acts[1])
        obs.append(env.reset(third).clone())
    for o in obs[1:]:
        assert torch.equal(o, obs[0])
    return obs[0]


# ---- 1. self-consistency against step(), every mode and reference kind, with and without action noise -----------------------------
def _env_kw(mode, refkind, N, t_max):
    from serl_amd import builds, refsignals as rs
    kw = {}
    if refkind == 'table':
        kw['refs'] = _tables(N, t_max, 41)
    elif refkind == 'spec':
        kw['refs'] = rs.ref_specs(*rs.training_references(1, 20, np.random.RandomState(8)), 0.2106)
    else:
        kw['refs'], kw['ref_pool'] = None, 2
    if builds.has_sensor_noise(mode):
        T = rs.n_steps_for(t_max)
        kw['sensor_noise'] = np.stack([builds.sensor_noise_table(T, np.random.RandomState(300 + e)) for e in range(N)])
    return kw


@pytest.mark.parametrize('noisy', [False, True], ids=['f32', 'noise'])
@pytest.mark.parametrize('refkind', ['table', 'spec', 'pool'])
@pytest.mark.parametrize('mode', ['nominal', 'cg-timed', 'gust'])
def test_rollout_equals_step_on_its_actions(engine, mode, refkind, noisy):
    N = 70
    t_max = 5 if refkind == 'pool' else T_SHORT
    kw = _env_kw(mode, refkind, N, t_max)
    env, twin = _venv(N, mode, t_max, engine, **kw), _venv(N, mode, t_max, engine, **kw)
    obs0 = _stagger([env, twin], seed=99 if refkind == 'pool' else None)
    dev = env.device
    actors = _actors(3)
    moe = torch.arange(N, dtype=torch.int32, device=dev) % 3
    ends = 0
    # K = 1, 5, 15: none, one or two episode ends inside a segment of six-step episodes; the pool's episodes are 500 steps
    for i, K in enumerate((1, 5, 15) + ((520,) if refkind == 'pool' else ())):
        noise = _noise(K, N, 50 + i).to(dev) if noisy else None
        out = env.rollout(actors, K, member_of_env=moe, action_noise=noise)
        assert env.last_rollout_path == 'fused'
        assert out['obs'].shape == (K + 1, N, 7) and out['actions'].shape == (K, N, 3) and out['done'].dtype == torch.bool
        assert torch.equal(out['obs'][0], obs0)
        o = _follow(twin, out, f64=noisy)
        _same_state(env, twin)
        obs0 = out['obs'][K]
        ends += o['done'].sum(0)
        assert np.isfinite(o['obs']).all() and np.isfinite(o['reward']).all()
        if noisy:
            assert (np.abs(o['actions']) <= 1.0).all() and (K < 15 or (np.abs(o['actions']) == 1.0).any())
    assert (ends >= (1 if refkind == 'pool' else 3)).all(), 'an env never restarted'
    if refkind == 'pool':
        assert (_np(env._cursor) == ends % 2).all()                     # a pool of two rows: the cursor of an env is its restarts modulo 2


# ---- 2. the in-kernel actor and episode against the fused rollout kernels and the oracle --------------------------------------------
def _fresh_episode(engine, w, noisy):
    import serl_amd
    M, K = len(w), 6
    refs = _tables(M, T_SHORT, 61)
    assert refs.shape[1] == K
    env = _venv(M, 'nominal', T_SHORT, engine, refs=refs)
    env.reset()
    dev = env.device
    noise = _noise(K, M, 77) if noisy else None
    spec = serl_amd.NetSpec(**NET32)
    wt = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    out = env.rollout(wt, K, spec=spec, member_of_env=np.arange(M, dtype=np.int32), action_noise=noise, transitions=True)
    assert env.last_rollout_path == 'fused'
    return refs, noise, spec, {k: _np(v) for k, v in out.items()}


def _scaled(o, noisy):
    a = o['actions']
    if noisy:
        return -BOUND + 0.5 * (a + 1.0) * (BOUND - -BOUND)
    s = (np.float32(0.5) * (a.astype(np.float32) + np.float32(1.0))).astype(np.float32)
    return -BOUND + s.astype(np.float64) * (BOUND - -BOUND)


@pytest.mark.parametrize('noisy', [False, True], ids=['plain', 'noise'])
def test_actor_and_episode_equal_the_fused_kernel(engine, golden, noisy):
    w = golden('actors')['serl50'][:5]
    refs, noise, spec, o = _fresh_episode(engine, w, noisy)
    M = len(w)
    kw = {} if noise is None else {'action_noise': np.ascontiguousarray(_np(noise).transpose(1, 0, 2))}
    f = engine.rollout(w, spec, np.arange(M), refs, t_max=T_SHORT, traces=True, transitions=True, **kw)
    assert (_np(f['length_steps']) == 6).all() and o['done'][5].all() and not o['done'][:5].any()
    np.testing.assert_array_equal(o['transitions'].transpose(1, 0, 2), _np(f['transitions']))
    np.testing.assert_array_equal(_scaled(o, noisy).transpose(1, 0, 2), _np(f['actions']))
    np.testing.assert_array_equal(o['x'].transpose(1, 0, 2), _np(f['states']))
    np.testing.assert_array_equal(o['reward'].T, _np(f['rewards']))
    np.testing.assert_array_equal(o['ep_return'][5], _np(f['fitness']))
    assert (o['ep_length'][5] == 6).all()


def test_actor_and_episode_equal_the_oracle(engine, golden):
    from oracle import rollout as R
    w = golden('actors')['serl50'][3:4]
    refs, _, _, o = _fresh_episode(engine, w, False)
    r = R.rollout(w, NET32, np.arange(1), refs, t_max=T_SHORT, traces=True, transitions=True, short_libm=True, threads=1)
    assert int(r['length_steps'][0]) == 6
    np.testing.assert_array_equal(o['transitions'][:, 0], r['transitions'][0])
    np.testing.assert_array_equal(_scaled(o, False)[:, 0], r['actions'][0])
    np.testing.assert_array_equal(o['x'][:, 0], r['states'][0])


# ---- 3. segments chain, and rollout / step share the state --------------------------------------------------------------------------
def test_segments_chain(engine):
    N = 70
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    a, b, c, d = (_venv(N, 'nominal', T_SHORT, engine, **kw) for _ in range(4))
    _stagger([a, b, c, d])
    actors = _actors(3, layers=1, activation='relu', seed=3)
    moe = np.arange(N) % 3
    whole = a.rollout(actors, 15, member_of_env=moe, transitions=True)
    first = b.rollout(actors, 5, member_of_env=moe, transitions=True)
    for k in range(5):                                               # the other route to the same point: step() on the recorded actions
        c.step(whole['actions'][k].float())
    _same_state(b, c)
    second = b.rollout(actors, 10, member_of_env=moe, transitions=True)
    _same_state(a, b)
    for key in whole:
        joined = torch.cat([first[key], second[key][1:] if key == 'obs' else second[key]])
        assert torch.equal(joined, whole[key]), key
    assert torch.equal(first['obs'][5], second['obs'][0])
    assert _np(whole['done']).sum(0).min() >= 2
    # rollout(5) then 3 x step == 8 x step
    d.rollout(actors, 5, member_of_env=moe)
    for k in range(5, 8):
        od, rd, dd, idd = d.step(whole['actions'][k].float())
        oc, rc, dc, ic = c.step(whole['actions'][k].float())
        assert torch.equal(od, oc) and torch.equal(rd, rc) and torch.equal(dd, dc)
        for key in ic:
            assert torch.equal(idd[key], ic[key]), key
        assert torch.equal(od, whole['obs'][k + 1])
    _same_state(d, c)


# ---- 4. one shared policy; one env ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 70])
def test_shared_policy(engine, N):
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    envs = [_venv(N, 'nominal', T_SHORT, engine, **kw) for _ in range(4)]
    _stagger(envs)
    actor = _actors(1, layers=3, activation='tanh', seed=4)[0]
    outs = [envs[0].rollout(actor, 15), envs[1].rollout(actor, 15, member_of_env=np.zeros(N, np.int32)), envs[2].rollout([actor], 15)]
    assert all(e.last_rollout_path == 'fused' for e in envs[:3])
    for o in outs[1:]:
        assert o.keys() == outs[0].keys()
        for key in o:
            assert torch.equal(o[key], outs[0][key]), key
    _follow(envs[3], outs[0], f64=False)
    assert _np(outs[0]['done']).sum(0).min() >= 2
    assert 'x' in outs[0] and 'transitions' not in outs[0]


def test_info_false_and_packed_rows_with_padding(engine):
    import serl_amd
    N = 6
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    a, b = _venv(N, 'nominal', T_SHORT, engine, **kw), _venv(N, 'nominal', T_SHORT, engine, **kw)
    _stagger([a, b])
    actors = _actors(2, layers=0, seed=5)                            # no hidden layer: P = 355, rows padded to 356
    full = a.rollout(actors, 7, member_of_env=np.arange(N) % 2)
    w = serl_amd.pack_population(actors).to(b.device)
    assert w.shape == (2, 356)
    lean = b.rollout(w, 7, spec=actors[0].spec, member_of_env=np.arange(N) % 2, info=False)
    assert set(full) - set(lean) == {'x', 'ref', 't', 'cost'}
    for key in lean:
        assert torch.equal(lean[key], full[key]), key
    _same_state(a, b)


# ---- 5. never-reset envs stay frozen --------------------------------------------------------------------------------------------------
def test_never_reset_envs_are_frozen(engine):
    N = 70
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    env, twin = _venv(N, 'nominal', T_SHORT, engine, **kw), _venv(N, 'nominal', T_SHORT, engine, **kw)
    dev = env.device
    mask = torch.arange(N, device=dev) % 2 == 0
    env.reset(mask); twin.reset(mask)
    cold = ~_np(mask)
    npad = (N + 63) // 64 * 64
    fields = lambda e: (_np(e._state[:73 * npad * 8].view(torch.float64).view(73, npad)), _np(e._state[73 * npad * 8:].view(torch.int32).view(17, npad)))
    f0, i0 = fields(env)
    out = env.rollout(_actors(1, seed=6)[0], 8, transitions=True)
    o = _follow(twin, out, f64=False)
    _same_state(env, twin)
    assert o['done'][:, cold].all() and (o['reward'][:, cold] == 0).all() and (o['actions'][:, cold] == 0).all()
    for k in range(8):
        np.testing.assert_array_equal(o['obs'][k + 1][cold], o['obs'][0][cold])
        np.testing.assert_array_equal(o['final_obs'][k][cold], o['obs'][0][cold])
    tr = o['transitions'][:, cold]
    np.testing.assert_array_equal(tr[..., :7], np.broadcast_to(o['obs'][0][cold].astype(np.float32), tr[..., :7].shape))
    np.testing.assert_array_equal(tr[..., 10:17], tr[..., :7])
    assert (tr[..., 7:10] == 0).all() and (tr[..., 17] == 0).all() and (tr[..., 18] == 1).all()
    f1, i1 = fields(env)
    np.testing.assert_array_equal(f1[:, :N][:, cold], f0[:, :N][:, cold])
    np.testing.assert_array_equal(i1[:, :N][:, cold], i0[:, :N][:, cold])
    for name in ('_run_return', '_run_length', '_cursor'):
        assert (_np(getattr(env, name))[cold] == 0).all()
    assert not o['done'][:5, ~cold].any() and o['done'][5, ~cold].all()


# ---- 6. transition rows: what DeviceReplay.append_rows takes ------------------------------------------------------------------------
def _assembled(o, fin):
    return np.concatenate([o['obs'][:-1].astype(np.float32), o['actions'].astype(np.float32), o['final_obs'].astype(np.float32),
                           o['reward'].astype(np.float32)[..., None], fin.astype(np.float32)[..., None],
                           (o['cost'] != 0).astype(np.float32)[..., None]], axis=-1)


@pytest.mark.parametrize('noisy', [False, True], ids=['plain', 'noise'])
def test_transition_rows_fill_a_replay_ring(engine, noisy):
    from serl_amd.replay import DeviceReplay
    N, K = 70, 15
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    env = _venv(N, 'nominal', T_SHORT, engine, **kw)
    _stagger([env])
    out = env.rollout(_actors(1, seed=8)[0], K, transitions=True, action_noise=_noise(K, N, 9) if noisy else None)
    o = {k: _np(v) for k, v in out.items()}
    assert o['transitions'].shape == (K, N, 20) and o['done'].any() and not o['done'].all()
    want = _assembled(o, o['done'])                                  # tables as long as t_max: every episode ends by t >= t_max, done == fin
    np.testing.assert_array_equal(o['transitions'], want)
    # the next observation of a terminal row is the terminal one, not the restarted one
    d = o['done']
    assert not np.array_equal(o['transitions'][d][:, 10:17], o['obs'][1:][d].astype(np.float32))
    ring, ring2 = DeviceReplay(2048, env.device, engine), DeviceReplay(2048, env.device, engine)
    ring.append_rows(out['transitions'].reshape(-1, 20))
    ring2.append_rows(torch.from_numpy(want.reshape(-1, 20)))
    assert len(ring) == K * N == len(ring2) and ring.position == ring2.position
    assert torch.equal(ring.rows, ring2.rows)


def test_table_exhaustion_is_done_but_not_terminal(engine):
    N, K, rows = 5, 9, 4
    env = _venv(N, 'nominal', T_SHORT, engine, refs=_tables(N, T_SHORT, 62, rows=rows))
    twin = _venv(N, 'nominal', T_SHORT, engine, refs=_tables(N, T_SHORT, 62, rows=rows))
    assert env.max_steps == rows
    env.reset(); twin.reset()
    out = env.rollout(_actors(1, seed=10)[0], K, transitions=True)
    o = _follow(twin, out, f64=False)
    assert o['done'][3].all() and o['done'][7].all() and o['done'].sum() == 2 * N      # the tables end after four steps ...
    assert (o['t'][o['done']] < T_SHORT).all()
    assert (o['transitions'][..., 18] == 0).all()                                    # ... which is no terminal state: fin stays 0
    np.testing.assert_array_equal(o['transitions'], _assembled(o, np.zeros_like(o['done'])))
    assert (o['ep_length'][o['done']] == rows).all()


# ---- 7. shapes the kernel does not take: the step loop, the same dictionary -----------------------------------------------------------
@pytest.mark.parametrize('noisy', [False, True], ids=['plain', 'noise'])
def test_loop_fallback_for_other_actor_shapes(engine, noisy):
    N, K = 5, 8
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    env, twin = _venv(N, 'nominal', T_SHORT, engine, **kw), _venv(N, 'nominal', T_SHORT, engine, **kw)
    dev = env.device
    mask = torch.arange(N, device=dev) != 2                         # env 2 is never reset
    env.reset(mask)
    obs = twin.reset(mask).clone()
    actors = _actors(2, hidden=72, layers=1, activation='tanh', seed=11, device=dev)
    moe = torch.tensor([0, 1, 0, 1, 1], dtype=torch.int32, device=dev)
    noise = _noise(K, N, 12).to(dev) if noisy else None
    out = env.rollout(actors, K, member_of_env=moe, action_noise=noise, transitions=True)
    assert env.last_rollout_path == 'loop'
    want = {k: [] for k in ('obs', 'actions', 'reward', 'done', 'final_obs', 'ep_return', 'ep_length', 'x', 'ref', 't', 'cost', 'transitions')}
    want['obs'].append(obs)
    live = _np(mask)
    for k in range(K):
        with torch.no_grad():
            a = torch.where((moe == 0)[:, None], actors[0](obs.float()), actors[1](obs.float()))
        if noisy:
            a = torch.clamp(a.double() + noise[k], -1.0, 1.0)
        nobs, rew, done, info = twin.step(a)
        a = torch.where(mask[:, None], a.double(), torch.zeros_like(a, dtype=torch.float64))
        ended = done & mask
        fin = torch.where(mask, done, torch.ones_like(done))          # tables as long as t_max: done == fin for a running env
        row = torch.cat([obs.float(), a.float(), info['final_obs'].float(), rew.float()[:, None], fin.float()[:, None],
                         info['cost'].ne(0).float()[:, None]], dim=1)
        for key, v in (('obs', nobs), ('actions', a), ('reward', rew), ('done', done), ('final_obs', info['final_obs']),
                       ('ep_return', torch.where(ended, info['episode_return'], torch.zeros_like(rew))),
                       ('ep_length', torch.where(ended, info['episode_length'], torch.zeros_like(info['episode_length']))),
                       ('x', info['x']), ('ref', info['ref']), ('t', info['t']), ('cost', info['cost']), ('transitions', row)):
            want[key].append(v.clone())
        obs = nobs.clone()
    assert set(out) == set(want)
    for key in want:
        w = torch.stack(want[key])
        assert out[key].dtype == w.dtype and out[key].shape == w.shape, key
        assert torch.equal(out[key], w), key
    _same_state(env, twin)
    d = _np(out['done'])
    assert d[:, live].any() and not d[:, live].all() and d[:, ~live].all()


# ---- 8. bad arguments: a clean error, no launch ------------------------------------------------------------------------------------------
def test_bad_arguments(engine):
    import serl_amd
    from serl_amd import _capi
    N = 4
    kw = _env_kw('nominal', 'table', N, T_SHORT)
    env = _venv(N, 'nominal', T_SHORT, engine, **kw)
    env.reset()
    dev = env.device
    actor = _actors(1, seed=13)[0]
    state0 = env._state.clone()
    manual = serl_amd.CitationVecEnv(N, mode='nominal', t_max=T_SHORT, engine=engine, refs=kw['refs'])
    with pytest.raises(ValueError, match='auto_reset'):
        manual.rollout(actor, 3)
    with pytest.raises(ValueError, match='n_steps'):
        env.rollout(actor, 0)
    w = serl_amd.pack_population([actor])
    with pytest.raises(ValueError, match='packed weights on cpu'):
        env.rollout(w, 3, spec=actor.spec)
    with pytest.raises(ValueError, match='member_of_env'):
        env.rollout(actor, 3, member_of_env=np.zeros(N + 1, np.int32))
    with pytest.raises(ValueError, match='action_noise'):
        env.rollout(actor, 3, action_noise=torch.zeros(3, N, 2, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match='action_noise'):
        env.rollout(actor, 3, action_noise=torch.zeros(4, N, 3, dtype=torch.float64, device=dev))
    # the C entry: another env configuration, another actor shape, NULL run state -- SERL_E_INVALID, nothing launched
    L, ctx = engine.lib, engine.ctx
    wd = w.to(dev)
    out = env._rollout_buffers(3, False, False)
    spec = actor.spec

    def rdesc(**over):
        d = dict(state_dim=7, action_dim=3, hidden=32, num_layers=spec.num_layers, activation=spec.activation_id, n_members=1,
                 weights=wd.data_ptr(), weight_stride=wd.shape[1], n_steps=3, obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr())
        d.update(over)
        return _capi.VenvRolloutDesc(**d)

    def call(d, au, rd):
        return L.serl_venv_rollout(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), None)
    for name in ('PHlab_full_nominal', 'PHlab_full_incremental', 'PHlab_symmetric_nominal', 'PHlab_attitude_incremental'):
        other = _venv(2, name, T_SHORT, engine, refs=_tables(2, T_SHORT, 63))
        other.reset()
        s0 = other._state.clone()
        assert call(other.desc, other.auto_desc, rdesc()) == _capi.E_INVALID, name
        assert b'attitude' in L.serl_last_error()
        torch.cuda.synchronize()
        assert torch.equal(other._state, s0)
    for over in (dict(hidden=72), dict(n_steps=0), dict(n_members=0), dict(obs=None), dict(weights=None), dict(weight_stride=8)):
        assert call(env.desc, env.auto_desc, rdesc(**over)) == _capi.E_INVALID, over
    au = _capi.VenvAutoDesc.from_buffer_copy(env.auto_desc)
    au.cursor = None
    assert call(env.desc, au, rdesc()) == _capi.E_INVALID
    d = _capi.VenvDesc.from_buffer_copy(env.desc)
    d.build_slot = 63
    assert call(d, env.auto_desc, rdesc()) == _capi.E_INVALID            # behind the descriptor checks: serl_venv_check
    torch.cuda.synchronize()
    assert torch.equal(env._state, state0)                           # nothing was launched
    # a following good call still matches a twin
    twin = _venv(N, 'nominal', T_SHORT, engine, **kw)
    twin.reset()
    _follow(twin, env.rollout(actor, 7), f64=False)
    _same_state(env, twin)

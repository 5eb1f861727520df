"""CitationVecEnv.rollout(path='fused') on an env that steps on the wave kernels (C ABI serl_venv_rollout_wave / _wave_noise, csrc/venv_wave_rollout.inc):
K policy-driven steps in one launch with ONE WAVEFRONT PER ENV, at ZERO tolerance against the yardsticks the lane rollout kernels are held to --
a twin wave env that is fed the recorded actions through step(), the lane kernels (path='fused' on a lane env), engine.rollout and the CPU oracle.

Shapes are the smallest at which each mechanism can go wrong: 1 env (a lone wavefront), 5 (no multiple of the wavefronts per workgroup), 66 (across the
64-env padding of the state buffer); six-step episodes (t_max = 0.05 s) and segments of 1, 5 and 15 steps, so that none, one and two restarts fall inside a
launch, staggered over the envs; the drawn pool needs t_max = 5 and one segment of 520 steps across its restart."""
import ctypes
import numpy as np
import pytest
import torch

from actor_shapes import make_weights, _shape, spec_of, ATTITUDE, SYMMETRIC, FULL
import test_gpu_venv_rollout as R
import test_gpu_venv_rollout_general as G
import test_gpu_venv_wave as W

pytestmark = pytest.mark.gpu
T_SHORT = 0.05
SEGMENTS = (1, 5, 15)
SIZES = (1, 5, 66)
SD, CLIP = 0.3, 0.5
_np = G._np


def _venv(n, mode, t_max, engine, kernel='wave', **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(n, mode=mode, t_max=t_max, engine=engine, auto_reset=True, kernel=kernel, **kw)


def _bits(out):
    """every tensor of a rollout as bit patterns (NaN-proof, -0.0 is not 0.0)"""
    view = {torch.float64: torch.int64, torch.float32: torch.int32}
    return {k: _np(v.view(view[v.dtype]) if v.dtype in view else v) for k, v in out.items()}


def _same_out(a, b, what=''):
    a, b = _bits(a), _bits(b)
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (what, k))


def _stagger(envs, seed=None):
    """R._stagger for any action width: reset all, two steps, reset every third env"""
    N, A, dev = envs[0].n_envs, envs[0].action_dim, envs[0].device
    g = torch.Generator(device='cpu').manual_seed(7)
    acts = ((torch.rand(2, N, 3, generator=g) * 2 - 1) * 0.6)[:, :, :A].contiguous().to(dev)
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


# ---- 1. equals step() on its own actions ---------------------------------------------------------------------------------------------
def _twin_case(engine, mode, refkind, noisy, N, s=None):
    s = s or _shape(72, 3)
    t_max = 5 if refkind == 'pool' else T_SHORT
    kw = R._env_kw(mode, refkind, N, t_max)
    env, twin = _venv(N, mode, t_max, engine, **kw), _venv(N, mode, t_max, engine, **kw)
    obs0 = _stagger([env, twin], seed=99 if refkind == 'pool' else None)
    dev = env.device
    w = G._weights(s, 3, 21, dev)
    moe = torch.arange(N, dtype=torch.int32, device=dev) % 3
    ends = 0
    for i, K in enumerate(SEGMENTS + ((520,) if refkind == 'pool' else ())):
        noise = R._noise(K, N, 50 + i).to(dev) if noisy else None
        out = env.rollout(w, K, spec=spec_of(s), member_of_env=moe, action_noise=noise, transitions=True, path='fused')
        assert env.last_rollout_path == 'fused-wave'
        assert out['obs'].shape == (K + 1, N, 7) and out['actions'].shape == (K, N, 3) and out['done'].dtype == torch.bool
        assert torch.equal(out['obs'][0], obs0)
        o = R._follow(twin, out, f64=noisy)
        assert twin.last_step_kernel == 'wave'
        R._same_state(env, twin)      # every byte of the state buffer and of the run buffers
        obs0 = out['obs'][K]
        ends += o['done'].sum(0)
        assert np.isfinite(o['obs']).all() and np.isfinite(o['reward']).all()
        if noisy:
            assert (np.abs(o['actions']) <= 1.0).all() and (K < 15 or N < 5 or (np.abs(o['actions']) == 1.0).any())
    assert (ends >= (1 if refkind == 'pool' else 3)).all(), 'an env never restarted'
    if refkind == 'pool':
        assert (_np(env._cursor) == ends % 2).all()
    if N >= 3:
        a = _np(out['actions'])
        assert not np.array_equal(a[:, 0], a[:, 1])      # the members act differently


@pytest.mark.parametrize('noisy', [False, True], ids=['f32', 'noise'])
@pytest.mark.parametrize('mode', ['nominal', 'ice', 'cg-timed', 'gust', 'test'])
def test_rollout_equals_step_on_its_actions(engine, mode, noisy):
    _twin_case(engine, mode, 'table', noisy, 66)


@pytest.mark.parametrize('N', [1, 5])
def test_rollout_equals_step_at_small_sizes(engine, N):
    _twin_case(engine, 'nominal', 'table', True, N)


@pytest.mark.parametrize('noisy', [False, True], ids=['f32', 'noise'])
@pytest.mark.parametrize('refkind', ['spec', 'pool'])
def test_rollout_equals_step_with_generated_references(engine, refkind, noisy):
    _twin_case(engine, 'gust' if refkind == 'spec' else 'nominal', refkind, noisy, 5, _shape(32, 3))


# ---- 2. equals the lane kernels ------------------------------------------------------------------------------------------------------
LANE_SHAPES = [_shape(32, 2), _shape(64, 1), _shape(72, 3), _shape(128, 1), _shape(4, 0), _shape(32, 16), _shape(96, 2, 'elu'), _shape(20, 1, 'relu'),
               _shape(12, 2, 'tanh', SYMMETRIC), _shape(72, 3, 'relu', FULL), _shape(32, 2, 'elu', ATTITUDE, True), _shape(8, 1, 'tanh', SYMMETRIC, True)]


@pytest.mark.parametrize('s', LANE_SHAPES, ids=G._sid)
def test_rollout_equals_the_lane_kernels(engine, s):
    N = 66 if s['hidden'] in (32, 72) else 5
    mode = G._mode_of(s)
    kw = G._env_kw(mode, N)
    lane, wave = _venv(N, mode, T_SHORT, engine, kernel='lane', **kw), _venv(N, mode, T_SHORT, engine, **kw)
    _stagger([lane, wave])
    dev = lane.device
    w = G._weights(s, 3, 23, dev)
    moe = torch.arange(N, dtype=torch.int32, device=dev) % 3
    lane32 = lane.fused_rollout_ok(spec_of(s))
    assert lane32 == (s['hidden'] == 32 and s['env_config'] == ATTITUDE and not s['incremental'])
    assert wave.fused_wave_ok(spec_of(s))
    ends = 0
    for i, K in enumerate(SEGMENTS):
        noise = R._noise(K, N, 60 + i).to(dev) if i == 1 else None      # (the middle segment through the f64 clip form)
        a = lane.rollout(w, K, spec=spec_of(s), member_of_env=moe, action_noise=noise, transitions=True, path='fused')
        b = wave.rollout(w, K, spec=spec_of(s), member_of_env=moe, action_noise=noise, transitions=True, path='fused')
        assert lane.last_rollout_path == ('fused' if lane32 else 'fused-general') and wave.last_rollout_path == 'fused-wave'
        _same_out(a, b, '%s segment %d' % (G._sid(s), i))
        W._same_state(lane, wave)
        for name in ('_run_return', '_run_length', '_cursor', '_ep_return', '_ep_length'):
            assert torch.equal(getattr(lane, name), getattr(wave, name)), name
        ends += _np(b['done']).sum(0)
    assert (ends >= 3).all()
    acts = _np(b['actions'])
    assert (np.abs(acts) < 1.0).any() and (N < 3 or not np.array_equal(acts[:, 0], acts[:, 1]))


# ---- 3. the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [_shape(32, 3), _shape(72, 3), _shape(12, 2, 'tanh', SYMMETRIC)], ids=G._sid)
def test_actor_and_episode_equal_the_fused_kernel_and_the_oracle(engine, s):
    from oracle import rollout as O
    M, K = 3, 6
    w = np.ascontiguousarray(make_weights(s, M, 33))
    refs = G._tables(M, 61)
    env = _venv(M, G._mode_of(s), T_SHORT, engine, refs=refs)
    env.reset()
    out = env.rollout(torch.from_numpy(w).to(env.device), K, spec=spec_of(s), member_of_env=np.arange(M, dtype=np.int32), transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-wave'
    o = {k: _np(v) for k, v in out.items()}
    kw = dict(t_max=T_SHORT, traces=True, transitions=True, env_config=s['env_config'], incremental=s['incremental'])
    f = engine.rollout(w, spec_of(s), np.arange(M), refs, **kw)
    assert (_np(f['length_steps']) == 6).all() and o['done'][5].all() and not o['done'][:5].any()
    cmds = G._commands(s, o, False)
    np.testing.assert_array_equal(o['transitions'].transpose(1, 0, 2), _np(f['transitions']))
    np.testing.assert_array_equal(cmds.transpose(1, 0, 2), _np(f['actions']))
    np.testing.assert_array_equal(o['x'].transpose(1, 0, 2), _np(f['states']))
    np.testing.assert_array_equal(o['reward'].T, _np(f['rewards']))
    np.testing.assert_array_equal(o['ep_return'][5], _np(f['fitness']))
    assert (o['ep_length'][5] == 6).all()
    net = {k: s[k] for k in ('state_dim', 'action_dim', 'hidden', 'num_layers', 'activation')}
    r = O.rollout(w, net, np.arange(M), refs, short_libm=True, threads=1, **kw)
    assert (np.asarray(r['length_steps']) == 6).all()
    np.testing.assert_array_equal(o['transitions'].transpose(1, 0, 2), r['transitions'][:, :6])
    np.testing.assert_array_equal(cmds.transpose(1, 0, 2), r['actions'][:, :6])
    np.testing.assert_array_equal(o['x'].transpose(1, 0, 2), r['states'][:, :6])
    np.testing.assert_array_equal(o['reward'].T, r['rewards'][:, :6])
    a = o['actions']
    assert (np.abs(a) < 1.0).any() and not np.array_equal(a[:, 0], a[:, 1])


# ---- 4. device noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['PHlab_attitude_noise', 'gust'])
def test_device_noise_equals_lane_and_loop(engine, mode):
    """identically seeded envs: wave path='fused' against lane path='fused' and wave path='loop', key for key; rollout(K1) then rollout(K2) = rollout(K1 + K2)"""
    N, K1, K2, seed = 5, 5, 10, 0x1234ABCD5678EF01
    s = _shape(32, 3) if mode == 'gust' else _shape(72, 3)
    refs = G._tables(N, 41)
    mk = lambda kernel: _venv(N, mode, T_SHORT, engine, kernel=kernel, refs=refs, sensor_noise='device', seed=seed)
    lane, wave, loop, whole = mk('lane'), mk('wave'), mk('wave'), mk('wave')
    dev = lane.device
    w = G._weights(s, 3, 25, dev)
    moe = torch.arange(N, dtype=torch.int32, device=dev) % 3
    third = torch.arange(N, device=dev) % 3 == 0
    ro = lambda env, K, path: env.rollout(w, K, spec=spec_of(s), member_of_env=moe, action_noise='device', noise_sd=SD, noise_clip=CLIP,
                                          transitions=True, path=path)
    obs = []
    for env in (lane, wave, loop, whole):
        env.reset()
        ro(env, 2, 'loop' if env is loop else 'fused')
        obs.append(env.reset(third).clone())      # stagger the phases; an abandoned episode takes an ordinal of its own
    assert all(torch.equal(o, obs[0]) for o in obs)
    parts = []
    for K in (K1, K2):
        a, b, c = ro(lane, K, 'fused'), ro(wave, K, 'fused'), ro(loop, K, 'loop')
        assert lane.last_rollout_path in ('fused', 'fused-general') and wave.last_rollout_path == 'fused-wave' and loop.last_rollout_path == 'loop'
        _same_out(a, b, 'lane / wave, %d steps' % K)
        _same_out(c, b, 'loop / wave, %d steps' % K)
        for other in (lane, loop):
            np.testing.assert_array_equal(_np(other.noise_episode), _np(wave.noise_episode))
        W._same_state(lane, wave)
        R._same_state(loop, wave)
        parts.append(b)
    one = ro(whole, K1 + K2, 'fused')
    for key in one:
        joined = torch.cat([parts[0][key], parts[1][key][1:] if key == 'obs' else parts[1][key]])
        assert torch.equal(joined, one[key]), key
    R._same_state(whole, wave)
    np.testing.assert_array_equal(_np(whole.noise_episode), _np(wave.noise_episode))
    assert int(_np(wave.noise_episode).min()) >= 3 and _np(one['done']).sum(0).min() >= 2
    a = _np(one['actions'])
    assert (np.abs(a) <= 1.0).all() and (np.abs(a) < 1.0).any()


def test_device_noise_episodes_replay_on_the_oracle(engine):
    """every episode the wave rollout kernel flew under device noise is reproduced on the CPU oracle from serl_amd.venv_noise's tables of (seed, env,
    episode ordinal): the check tests/test_gpu_venv_noise_replay.py makes of the lane kernels, on an env made with kernel='wave'"""
    import test_gpu_venv_noise_replay as lane_test
    env = lane_test._replay_case(engine, 'gust', 5, 8, 1, 'fused', 'fused-wave', kernel='wave')
    assert env._wave and env.last_rollout_path == 'fused-wave'


# ---- 5. frozen envs, mixing with step(), chaining ------------------------------------------------------------------------------------------
def test_never_reset_envs_are_frozen(engine):
    s = _shape(12, 2, 'tanh', SYMMETRIC)
    N, K, S, A = 66, 70, 2, 1      # (70 steps: a frozen env's rows are spread over the 64 lanes, so some lanes write two)
    mode = G._mode_of(s)
    kw = G._env_kw(mode, N)
    env, lane = _venv(N, mode, T_SHORT, engine, **kw), _venv(N, mode, T_SHORT, engine, kernel='lane', **kw)
    dev = env.device
    mask = torch.arange(N, device=dev) % 2 == 0
    env.reset(mask); lane.reset(mask)
    cold = ~_np(mask)
    before = W._state(env)
    out = env.rollout(G._weights(s, 1, 6, dev), K, spec=spec_of(s), transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-wave'
    _same_out(lane.rollout(G._weights(s, 1, 6, dev), K, spec=spec_of(s), transitions=True, path='fused'), out)
    o = {k: _np(v) for k, v in out.items()}
    assert o['done'][:, cold].all() and (o['reward'][:, cold] == 0).all() and (o['actions'][:, cold] == 0).all()
    for k in range(K):
        np.testing.assert_array_equal(o['obs'][k + 1][cold], o['obs'][0][cold])
        np.testing.assert_array_equal(o['final_obs'][k][cold], o['obs'][0][cold])
    tr = o['transitions'][:, cold]
    assert tr.shape[-1] == 2 * S + A + 3 == 8
    np.testing.assert_array_equal(tr[..., :S], np.broadcast_to(o['obs'][0][cold].astype(np.float32), tr[..., :S].shape))
    np.testing.assert_array_equal(tr[..., S + A:2 * S + A], tr[..., :S])
    assert (tr[..., S:S + A] == 0).all() and (tr[..., 2 * S + A] == 0).all() and (tr[..., 2 * S + A + 1] == 1).all()
    after = W._state(env)
    for b, a in zip(before, after):
        np.testing.assert_array_equal(a[:, cold], b[:, cold])
    for name in ('_run_return', '_run_length', '_cursor'):
        assert (_np(getattr(env, name))[cold] == 0).all()
    assert not o['done'][:5, ~cold].any() and o['done'][5, ~cold].all()


def test_step_and_rollout_alternate_and_segments_chain(engine):
    N, s = 66, _shape(72, 3)
    kw = G._env_kw('nominal', N)
    a, b, c, d = (_venv(N, 'nominal', T_SHORT, engine, **kw) for _ in range(4))
    _stagger([a, b, c, d])
    dev = a.device
    w, spec, moe = G._weights(s, 3, 3, dev), spec_of(s), np.arange(N) % 3
    ro = lambda env, K: env.rollout(w, K, spec=spec, member_of_env=moe, transitions=True, path='fused')
    whole, first = ro(a, 15), ro(b, 5)
    for k in range(5):                                               # the twin that only steps
        c.step(whole['actions'][k].float())
    R._same_state(b, c)
    second = ro(b, 10)
    assert a.last_rollout_path == b.last_rollout_path == 'fused-wave'
    R._same_state(a, b)
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
        assert d.last_step_kernel == 'wave'
        assert torch.equal(od, oc) and torch.equal(rd, rc) and torch.equal(dd, dc)
        for key in ic:
            assert torch.equal(idd[key], ic[key]), key
        assert torch.equal(od, whole['obs'][k + 1])
    R._same_state(d, c)
    tail = ro(d, 7)
    for key in ('obs', 'actions', 'reward', 'done', 'transitions'):
        assert torch.equal(tail[key], whole[key][8:]), key
    R._same_state(d, a)


def test_info_false_modules_and_no_member_table(engine):
    """info=False and transitions=False leave their rows out; torch modules are packed on the device; member_of_env=None runs member 0"""
    N, K = 5, 7
    kw = G._env_kw('nominal', N)
    env, twin = _venv(N, 'nominal', T_SHORT, engine, **kw), _venv(N, 'nominal', T_SHORT, engine, **kw)
    _stagger([env, twin])
    actors = R._actors(1, hidden=64, layers=1)
    out = env.rollout(actors, K, info=False, path='fused')
    assert env.last_rollout_path == 'fused-wave'
    assert sorted(out) == ['actions', 'done', 'ep_length', 'ep_return', 'final_obs', 'obs', 'reward']
    full = twin.rollout(actors[0], K, transitions=True, path='fused')
    for key in out:
        assert torch.equal(out[key], full[key]), key
    R._same_state(env, twin)


# ---- 6. reporting and refusals ---------------------------------------------------------------------------------------------------------
def test_reporting_and_refusals(engine):
    import serl_amd
    from serl_amd import _capi
    N, s = 5, _shape(72, 3)
    env = _venv(N, 'nominal', T_SHORT, engine, **G._env_kw('nominal', N))
    env.reset()
    dev = env.device
    L, ctx = engine.lib, engine.ctx
    env.rollout(G._weights(s, 1, 9, dev), 3, spec=spec_of(s), path='fused')
    assert env.last_rollout_path == 'fused-wave'
    info = (ctypes.c_int32 * 4)()
    assert L.serl_venv_last_info(ctx, info) == 0
    assert info[0] == 10 and 1 <= info[2] <= 4 and info[1] * info[2] >= N and info[1] == (N + info[2] - 1) // info[2]      # SERL_FAMILY_WAVE
    torch.cuda.synchronize()
    state0 = env._state.clone()
    run0 = [getattr(env, n).clone() for n in ('_run_return', '_run_length', '_cursor')]

    class A30:
        state_dim, action_dim, hidden_size, num_layers, activation_actor = 7, 3, 30, 1, 'tanh'
    with pytest.raises(ValueError, match="path='fused'"):
        env.rollout(serl_amd.Actor(A30()), 3, path='fused')
    with pytest.raises(ValueError, match='wave kernels'):      # the default path still refuses the lane kernel on a wave env
        env.rollout(G._weights(_shape(32, 3), 1, 9, dev), 3, spec=spec_of(_shape(32, 3)))
    with pytest.raises(ValueError, match='path'):
        env.rollout(G._weights(s, 1, 9, dev), 3, spec=spec_of(s), path='bogus')
    assert env.ROLLOUT_PATHS == ('auto', 'fused', 'loop')
    wd = torch.zeros(1, 24000, dtype=torch.float32, device=dev)
    out = env._rollout_buffers(3, False, False)

    def rdesc(**over):
        d = dict(state_dim=7, action_dim=3, hidden=72, num_layers=3, activation=0, n_members=1, weights=wd.data_ptr(), weight_stride=wd.shape[1],
                 n_steps=3, obs=out['obs'].data_ptr(), reward=out['reward'].data_ptr())
        d.update(over)
        return _capi.VenvRolloutDesc(**d)
    seeded = _venv(N, 'nominal', T_SHORT, engine, seed=5, **G._env_kw('nominal', N))
    seeded.reset()
    nzd = seeded._nz_desc()

    def call(rd, au=None, d=None):
        return L.serl_venv_rollout_wave(ctx, ctypes.byref(d or env.desc), ctypes.byref(au or env.auto_desc), ctypes.byref(rd), None)

    def call_nz(rd, nzp):
        return L.serl_venv_rollout_wave_noise(ctx, ctypes.byref(seeded.desc), ctypes.byref(seeded.auto_desc), ctypes.byref(rd), nzp, None)
    P = L.serl_param_count(7, 72, 3, 3)
    want = {'obs': _capi.E_INVALID, 'n_steps': _capi.E_INVALID, 'hidden': _capi.E_UNSUPPORTED, 'weights': _capi.E_INVALID}
    for key, over in (('obs', dict(obs=None)), ('n_steps', dict(n_steps=0)), ('hidden', dict(hidden=132)), ('weights', dict(weights=wd.data_ptr() + 4))):
        assert call(rdesc(**over)) == want[key], over
        assert b'serl_venv_rollout_wave' in L.serl_last_error()
        assert call_nz(rdesc(**over), ctypes.byref(nzd)) == want[key], over
    for over in (dict(hidden=30), dict(hidden=0), dict(num_layers=17), dict(state_dim=13), dict(action_dim=1), dict(weight_stride=P - 3),
                 dict(weight_stride=P + 3), dict(n_members=0), dict(activation=3), dict(weights=None)):
        assert call(rdesc(**over)) in (_capi.E_INVALID, _capi.E_UNSUPPORTED), over
    for field in ('cursor', 'run_return', 'run_length'):
        au = _capi.VenvAutoDesc.from_buffer_copy(env.auto_desc)
        setattr(au, field, None)
        assert call(rdesc(), au=au) == _capi.E_INVALID, field
    d = _capi.VenvDesc.from_buffer_copy(env.desc)
    d.build_slot = 63
    assert call(rdesc(), d=d) == _capi.E_INVALID
    assert call_nz(rdesc(), None) == _capi.E_INVALID and b'nz is NULL' in L.serl_last_error()
    torch.cuda.synchronize()
    assert torch.equal(env._state, state0)                           # nothing was launched
    for n, r in zip(('_run_return', '_run_length', '_cursor'), run0):
        assert torch.equal(getattr(env, n), r), n


# ---- 7. replay -----------------------------------------------------------------------------------------------------------------------------
def test_transition_rows_fill_a_replay_ring(engine):
    from serl_amd.replay import DeviceReplay
    s = _shape(32, 3)
    N, K, S, A = 66, 15, 7, 3
    env = _venv(N, 'nominal', T_SHORT, engine, **G._env_kw('nominal', N))
    _stagger([env])
    out = env.rollout(G._weights(s, 1, 8, env.device), K, spec=spec_of(s), transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-wave'
    o = {k: _np(v) for k, v in out.items()}
    assert o['transitions'].shape == (K, N, 20) and o['done'].any() and not o['done'].all()
    want = np.concatenate([o['obs'][:-1].astype(np.float32), o['actions'].astype(np.float32), o['final_obs'].astype(np.float32),
                           o['reward'].astype(np.float32)[..., None], o['done'].astype(np.float32)[..., None],
                           (o['cost'] != 0).astype(np.float32)[..., None]], axis=-1)
    np.testing.assert_array_equal(o['transitions'], want)
    ring, ring2 = DeviceReplay(2048, env.device, engine, S, A), DeviceReplay(2048, env.device, engine, S, A)
    ring.append_rows(out['transitions'].reshape(-1, 20))
    ring2.append_rows(torch.from_numpy(want.reshape(-1, 20)))
    assert len(ring) == K * N == len(ring2) and ring.position == ring2.position
    assert torch.equal(ring.rows, ring2.rows)

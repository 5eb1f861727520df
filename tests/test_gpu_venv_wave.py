"""CitationVecEnv(kernel='wave'): reset / step with one wavefront per env (serl_venv_*_wave, csrc/venv_wave.inc) against the lane kernels and the CPU
oracle, bit for bit in every output tensor, and the state buffer the two families share: any call of either may follow any call of the other.

Shapes are the smallest at which each mechanism can go wrong: 1 env (a lone wavefront), 5 (no multiple of the wavefronts per workgroup), 65 (across
the 64-env padding of the state buffer); 12 steps alternate both Derivative-block banks several times; 3-row reference tables end episodes by
k == max_steps, t_max = 0.03 s by t >= t_max with the termination penalty."""
import ctypes
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NET32 = dict(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation='tanh')
STEPS = 12
# the five code variants through one mode each, and the env configurations on the nominal build
VARIANT_MODES = ['PHlab_attitude_nominal', 'ice', 'cg-timed', 'gust', 'test']
CONFIG_MODES = ['PHlab_symmetric_nominal', 'PHlab_full_nominal', 'PHlab_attitude_incremental', 'PHlab_symmetric_incremental']
T3_ROWS = slice(0, 3)         # SERL_VI_IW + 0 .. 2
HINT_ROWS = slice(6, 14)      # SERL_VI_HINT .. + 8 of the 17 i32 fields (csrc/rollout_device.h)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _venv(engine, n, mode, t_max, **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(n, mode=mode, t_max=t_max, engine=engine, **kw)


def _tables(N, rows, seed):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rows])
    assert np.isfinite(r).all() and r.shape == (N, rows, 3)
    return r


def _actions(N, A, seed, steps=STEPS):
    return torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (steps, N, A)).astype(np.float32))


def _sensor(env_kw, mode, N, rows):
    """the modes with a sensor model get a fixed table, so that both runs add the same noise"""
    from serl_amd import builds
    if builds.has_sensor_noise(mode):
        env_kw['sensor_noise'] = np.stack([builds.sensor_noise_table(rows, np.random.RandomState(300 + e)) for e in range(N)])


def _state(env):
    """(f64 fields [73, N], i32 fields [17, N]) of the env's state buffer, as bit patterns"""
    N = env.n_envs
    npad = (N + 63) // 64 * 64
    raw = env._state
    f = raw[:73 * npad * 8].view(torch.int64).view(73, npad)[:, :N]
    i = raw[73 * npad * 8:].view(torch.int32).view(17, npad)[:, :N]
    return _np(f), _np(i)


def _same_state(a, b):
    """every field of the two state buffers but the hint words and IW[0..2], the table3 interval cache: the lane step walks it from a work word it never
    initialises (citation_step_dev.h never loads lc.DW[26..28]), so the lane kernels' own words depend on the compiled kernel and cannot be reproduced.
    The wave kernels leave them alone (test_wave_steps_leave_the_table3_cache_alone) and CitationVecEnv.rollout() does not run the lane rollout kernels
    on a wave env (test_rollout_refuses_on_a_wave_env)."""
    fa, ia = _state(a)
    fb, ib = _state(b)
    np.testing.assert_array_equal(fa, fb, err_msg='f64 fields of the state')
    keep = np.ones(17, bool)
    keep[HINT_ROWS] = False
    keep[T3_ROWS] = False
    np.testing.assert_array_equal(ia[keep], ib[keep], err_msg='i32 fields of the state (IW[4], tick, error word, k, live, cost)')


def _outputs(ret):
    """everything a step returned, as bit patterns"""
    obs, rew, done, info = ret
    out = {'obs': obs, 'reward': rew, 'done': done}
    out.update(info)
    return {k: _np(v if v.dtype != torch.float64 else v.view(torch.int64)) for k, v in out.items()}


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (what, k))


# ---- 1. the keyword exists and the library says what it launched ------------------------------------------------------------------------
def test_wave_env_constructs_and_reports_its_kernel(engine):
    env = _venv(engine, 4, 'PHlab_attitude_nominal', 0.2, refs=_tables(4, 20, 3), kernel='wave')
    env.reset()
    assert env.last_step_kernel == 'wave'
    env.step(torch.zeros(4, 3, dtype=torch.float32, device=env.device))
    assert env.last_step_kernel == 'wave'
    info = (ctypes.c_int32 * 4)()
    assert engine.lib.serl_venv_last_info(engine.ctx, info) == 0
    assert info[0] == 10 and info[1] * info[2] >= 4 and 1 <= info[2] <= 4      # SERL_FAMILY_WAVE; one wavefront per env
    lane = _venv(engine, 4, 'PHlab_attitude_nominal', 0.2, refs=_tables(4, 20, 3))
    lane.reset()
    assert lane.last_step_kernel == 'lane' and lane.kernel == 'lane'
    auto = _venv(engine, 4, 'PHlab_attitude_nominal', 0.2, refs=_tables(4, 20, 3), kernel='auto')
    auto.reset()
    from serl_amd import venv
    assert auto.last_step_kernel == ('wave' if 4 <= venv.WAVE_MAX_ENVS else 'lane')


# ---- 2. wave against lane ----------------------------------------------------------------------------------------------------------------
def _lane_and_wave(engine, mode, N, rows=20, t_max=0.2, steps=STEPS, **kw):
    refs = _tables(N, rows, 5 + N)
    _sensor(kw, mode, N, rows)
    lane = _venv(engine, N, mode, t_max, refs=refs, **kw)
    wave = _venv(engine, N, mode, t_max, refs=refs, kernel='wave', **kw)
    return lane, wave, _actions(N, lane.action_dim, 17 + N, steps).to(lane.device)


@pytest.mark.parametrize('N', [1, 5, 65])
@pytest.mark.parametrize('mode', VARIANT_MODES + CONFIG_MODES)
def test_wave_equals_lane(engine, mode, N):
    if mode in CONFIG_MODES and N == 65:
        N = 66      # (the configurations run once across the padding too, at another remainder)
    lane, wave, acts = _lane_and_wave(engine, mode, N)
    np.testing.assert_array_equal(_np(lane.reset().view(torch.int64)), _np(wave.reset().view(torch.int64)))
    assert wave.last_step_kernel == 'wave'
    for k in range(STEPS):
        a = _outputs(lane.step(acts[k]))
        assert lane.last_step_kernel == 'lane'
        b = _outputs(wave.step(acts[k]))
        assert wave.last_step_kernel == 'wave'
        _same(a, b, '%s, %d envs, step %d' % (mode, N, k))
    _same_state(lane, wave)


def test_wave_equals_lane_f64_actions_faults_and_a_running_clock(engine):
    """f64 actions, a fault row (mode 'be'), err0 / tick0 at the reset"""
    N = 5
    lane, wave, acts = _lane_and_wave(engine, 'be', N)
    err0 = np.random.RandomState(2).normal(0, 0.01, (N, 3))
    tick0 = np.array([0, 1, 7, 1999, 2000], np.int32)
    np.testing.assert_array_equal(_np(lane.reset(err0=err0, tick0=tick0)), _np(wave.reset(err0=err0, tick0=tick0)))
    for k in range(4):
        _same(_outputs(lane.step(acts[k].double())), _outputs(wave.step(acts[k].double())), 'step %d' % k)
    _same_state(lane, wave)


# ---- 3. against the CPU oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,build,noisy', [('nominal', 'h2000_v90', False), ('ice', 'ice', False), ('cg-timed', 'cg_timed', False),
                                              ('gust', 'gust', True), ('test', 'test', False)])
def test_wave_replays_oracle_episodes(engine, golden, mode, build, noisy):
    from serl_amd import builds, refsignals as rs
    from test_gpu_venv import _oracle, _replay
    E, t_max = 5, 1
    w = golden('actors')['serl50']
    moe = np.arange(E) % len(w)
    refs = _tables(E, rs.n_steps_for(t_max), 31 + len(mode))
    kw, env_kw = {}, {}
    if noisy:
        sn = np.stack([builds.sensor_noise_table(refs.shape[1], np.random.RandomState(100 + e)) for e in range(E)])
        kw['sensor_noise'] = env_kw['sensor_noise'] = sn
    o = _oracle(w, NET32, moe, refs, build=build, t_max=t_max, traces=True, transitions=True, **kw)
    env = _venv(engine, E, mode, t_max, refs=refs, kernel='wave', **env_kw)
    assert env.build == build
    _replay(env, o, 7, 3)
    assert env.last_step_kernel == 'wave'


# ---- 4. ends of episodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,t_max', [(3, 0.2), (6, 0.03)])
def test_finished_envs_freeze_as_on_lanes(engine, rows, t_max):
    N = 5
    lane, wave, acts = _lane_and_wave(engine, 'PHlab_attitude_nominal', N, rows=rows, t_max=t_max, steps=6)
    first = torch.tensor([True, True, False, True, False], device=lane.device)      # envs 2 and 4 are never reset: frozen from the start
    np.testing.assert_array_equal(_np(lane.reset(first)), _np(wave.reset(first)))
    seen = []
    for k in range(6):
        a, b = _outputs(lane.step(acts[k])), _outputs(wave.step(acts[k]))
        _same(a, b, 'step %d' % k)
        seen.append(b)
        if k == 1:      # a partial mask: the others keep what the lane kernel writes for them
            second = torch.tensor([False, True, False, False, False], device=lane.device)
            np.testing.assert_array_equal(_np(lane.reset(second)), _np(wave.reset(second)))
    _same_state(lane, wave)
    done = np.stack([s['done'] for s in seen])
    assert done[:, [2, 4]].all()                          # never reset
    assert not done[0, [0, 1, 3]].any() and done[-1].all()      # the others ran, then froze
    end = int(np.argmax(done[:, 0]))      # env 0's episode ends here (k == max_steps after 3 steps; t >= 0.03 s at the fourth)
    assert end == (2 if rows == 3 else 3)
    reward = np.stack([s['reward'] for s in seen]).view(np.float64)
    assert (reward[end + 1:, 0] == 0.0).all() and reward[end, 0] != 0.0
    for key in ('obs', 'x', 'ref', 't', 'cost'):      # frozen: the last outputs
        for k in range(end + 1, 6):
            np.testing.assert_array_equal(seen[k][key][0], seen[end][key][0])


@pytest.mark.parametrize('rows,t_max,pool', [(3, 0.2, False), (6, 0.03, False), (None, 5, True)])
def test_auto_reset_equals_lane(engine, rows, t_max, pool):
    """8 steps of 5 envs whose episodes end at different steps (staggered by reset(mask) and tick0); with refs=None the restarts walk the reference pool"""
    N, steps = 5, 8
    envs = []
    for kernel in ('lane', 'wave'):
        np.random.seed(77)      # (the pool's references are drawn from np.random at the reset)
        kw = dict(auto_reset=True, kernel=kernel)
        if pool:
            kw['ref_pool'] = 2
        else:
            kw['refs'] = _tables(N, rows, 9)
        envs.append(_venv(engine, N, 'PHlab_attitude_nominal', t_max, **kw))
        if pool:      # (drawn references need seconds of t_max: the episodes are cut to three steps through the descriptor instead)
            envs[-1].desc.max_steps = 3
    lane, wave = envs
    acts = _actions(N, 3, 23, steps).to(lane.device)
    tick0 = np.array([0, 3, 1998, 5, 0], np.int32)
    first = torch.tensor([True, True, True, True, False], device=lane.device)      # env 4 is never reset
    for env in envs:
        np.random.seed(78)
        env.reset(first, tick0=tick0)
    np.testing.assert_array_equal(_np(lane._obs), _np(wave._obs))
    done_rows, cursor_rows = [], []
    for k in range(steps):
        a, b = _outputs(lane.step(acts[k])), _outputs(wave.step(acts[k]))
        assert sorted(b) == ['cost', 'done', 'episode_length', 'episode_return', 'final_obs', 'obs', 'ref', 'reward', 't', 'x']
        _same(a, b, 'step %d' % k)
        np.testing.assert_array_equal(_np(lane._cursor), _np(wave._cursor), err_msg='cursor after step %d' % k)
        np.testing.assert_array_equal(_np(lane._run_length), _np(wave._run_length))
        np.testing.assert_array_equal(_np(lane._run_return), _np(wave._run_return))
        done_rows.append(b['done'])
        cursor_rows.append(_np(wave._cursor))
        if k in (0, 1):      # stagger: env k starts over, so that the episodes end at different steps
            m = torch.arange(N, device=lane.device) == k
            for env in envs:
                np.random.seed(79 + k)
                env.reset(m)
            np.testing.assert_array_equal(_np(lane._obs), _np(wave._obs))
    _same_state(lane, wave)
    done = np.stack(done_rows)
    assert done[:, 4].all() and (done[:, :4].sum(0) >= 1).all()
    assert len({int(np.argmax(done[:, e])) for e in range(3)}) == 3      # envs 0, 1, 2 end at different steps
    assert wave.last_step_kernel == 'wave'
    cursors = np.stack(cursor_rows)      # every running env's cursor moved (with a pool of two rows it is back at 0 after two episodes)
    assert (cursors[:, :4].max(0) >= 1).all() and (cursors[:, 4] == 0).all()


# ---- 5. interchange on one state buffer --------------------------------------------------------------------------------------------------
def test_families_alternate_on_one_state_buffer(engine, golden):
    """lane reset, wave step, lane step, wave auto-step, lane rollout(actor, 3), wave step ... : every output of every call is the all-lane run's.
    The env is made with kernel='lane' and its private family switch is flipped per call: this is the C ABI's interchange, which the issue asks to be
    shown; the public wave env refuses the lane rollout kernels (test_rollout_refuses_on_a_wave_env), since IW[0..2] are not an all-lane run's."""
    import serl_amd
    N = 5
    refs = _tables(N, 40, 13)
    w = torch.from_numpy(np.ascontiguousarray(golden('actors')['serl50'][:2])).to(engine.device)
    spec = serl_amd.NetSpec(**NET32)
    mixed = _venv(engine, N, 'PHlab_attitude_nominal', 0.4, refs=refs, auto_reset=True)
    lanes = _venv(engine, N, 'PHlab_attitude_nominal', 0.4, refs=refs, auto_reset=True)
    acts = _actions(N, 3, 29, 16).to(engine.device)

    def call(env, what, k, wave):
        env._wave = wave
        if what == 'reset':
            return {'obs': _np(env.reset())}
        if what == 'rollout':
            return {key: _np(v) for key, v in env.rollout(w, 3, spec=spec, member_of_env=np.arange(N, dtype=np.int32) % 2, transitions=True).items()}
        env.auto_reset = what == 'auto'      # (a plain step on the same buffers: serl_venv_step / serl_venv_step_wave)
        try:
            return _outputs(env.step(acts[k]))
        finally:
            env.auto_reset = True

    script = [('reset', False), ('step', True), ('step', False), ('auto', True), ('rollout', False), ('step', True),
              ('auto', False), ('auto', True), ('step', False), ('step', True), ('rollout', False), ('auto', True), ('step', True), ('auto', True)]
    stepped = 0
    for k, (what, wave) in enumerate(script):
        a, b = call(lanes, what, k, False), call(mixed, what, k, wave)
        if what != 'rollout':      # (what the env's own reset / step launched)
            assert mixed.last_step_kernel == ('wave' if wave else 'lane')
        _same(a, b, 'call %d (%s on %s)' % (k, what, 'wave' if wave else 'lane'))
        stepped += 3 if what == 'rollout' else (what != 'reset')
    assert stepped >= 12
    _same_state(lanes, mixed)


def test_wave_steps_leave_the_table3_cache_alone(engine):
    """IW[0..2]: a wave reset stores initialize()'s image (zeros in every shipped build), a wave step -- auto-reset restarts apart, which store the image
    again -- leaves what it finds, hint words included"""
    N = 5
    env = _venv(engine, N, 'ice', 0.2, refs=_tables(N, 20, 3), kernel='wave')
    acts = _actions(N, 3, 41, 3).to(env.device)
    env.reset()
    i32 = _state(env)[1]
    assert (i32[T3_ROWS] == 0).all() and (i32[3] == 0).all() and (i32[5] == 0).all()      # the cache image, IW[3], the error word
    npad = 64
    words = env._state[73 * npad * 8:].view(torch.int32).view(17, npad)
    marks = torch.arange(11 * N, dtype=torch.int32, device=env.device).reshape(11, N) % 3      # in the walks' range: a lane kernel would take them too
    words[T3_ROWS, :N] = marks[:3]
    words[HINT_ROWS, :N] = marks[3:] + 7
    for k in range(3):
        env.step(acts[k])
    i32 = _state(env)[1]
    np.testing.assert_array_equal(i32[T3_ROWS], _np(marks[:3]))
    np.testing.assert_array_equal(i32[HINT_ROWS], _np(marks[3:] + 7))


def test_rollout_refuses_on_a_wave_env(engine, golden):
    """the contract: reset / step of the two families interchange on one buffer in every output (test_families_alternate_on_one_state_buffer drives that
    through the private switch), but the public env does not run the lane ROLLOUT kernels behind wave steps, because three state words are not a lane run's"""
    import serl_amd
    w = torch.from_numpy(np.ascontiguousarray(golden('actors')['serl50'][:1])).to(engine.device)
    env = _venv(engine, 3, 'PHlab_attitude_nominal', 0.2, refs=_tables(3, 20, 3), auto_reset=True, kernel='wave')
    env.reset()
    with pytest.raises(ValueError, match='wave kernels'):
        env.rollout(w, 2, spec=serl_amd.NetSpec(**NET32))
    assert env.rollout(w, 2, spec=serl_amd.NetSpec(**NET32), path='loop')['obs'].shape == (3, 3, 7) and env.last_step_kernel == 'wave'
    env = _venv(engine, 3, 'PHlab_attitude_nominal', 0.2, refs=_tables(3, 20, 3), auto_reset=True)
    env.reset()
    assert env.rollout(w, 2, spec=serl_amd.NetSpec(**NET32))['obs'].shape == (3, 3, 7)


# ---- 6. device noise -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['PHlab_attitude_noise', 'gust'])
def test_device_noise_equals_lane(engine, mode):
    N, steps, seed = 5, 8, 0x1234ABCD5678EF01
    refs = _tables(N, 3, 15)
    envs = [_venv(engine, N, mode, 0.2, refs=refs, auto_reset=True, sensor_noise='device', seed=seed, kernel=k) for k in ('lane', 'wave')]
    lane, wave = envs
    acts = _actions(N, 3, 37, steps).to(lane.device)
    np.testing.assert_array_equal(_np(lane.reset()), _np(wave.reset()))
    for k in range(steps):
        _same(_outputs(lane.step(acts[k])), _outputs(wave.step(acts[k])), 'step %d' % k)
        np.testing.assert_array_equal(_np(lane.noise_episode), _np(wave.noise_episode))
        if k == 3:
            m = torch.tensor([False, True, False, False, True], device=lane.device)
            np.testing.assert_array_equal(_np(lane.reset(m)), _np(wave.reset(m)))
    assert wave.last_step_kernel == 'wave' and int(_np(wave.noise_episode).min()) >= 3
    _same_state(lane, wave)


def test_device_noise_replays_on_the_oracle(engine):
    """the step loop of a device-noise env on the wave kernels: every episode it flew is replayed on the CPU oracle from (seed, env, episode ordinal)
    through serl_amd.venv_noise -- the check tests/test_gpu_venv_noise_replay.py makes of the lane kernels (which asserts the family of the env and
    of its noise-free twin)"""
    import test_gpu_venv_noise_replay as lane_test
    env = lane_test._replay_case(engine, 'gust', 5, 8, 1, 'loop', 'loop', kernel='wave')
    assert env._wave and env.last_step_kernel == 'wave'


# ---- 7. refusals that need a context -------------------------------------------------------------------------------------------------
def test_wave_entry_points_refuse_what_their_namesakes_refuse(engine):
    from serl_amd import _capi
    L = engine.lib
    env = _venv(engine, 4, 'PHlab_attitude_nominal', 0.2, refs=_tables(4, 20, 3), auto_reset=True, kernel='wave', seed=5)
    env.reset()
    before = _state(env)
    a = torch.zeros(4, 3, dtype=torch.float32, device=env.device)
    out = (env._obs.data_ptr(), env._reward.data_ptr(), env._done.data_ptr(), env._x.data_ptr(), env._refk.data_ptr(), env._t.data_ptr(),
           env._cost.data_ptr())
    d, au, nz = env.desc, env.auto_desc, env._nz_desc()
    for f64 in (2, -1):
        assert L.serl_venv_step_wave(engine.ctx, ctypes.byref(d), a.data_ptr(), f64, *out, None) == _capi.E_INVALID
        assert b'actions_f64' in L.serl_last_error()
        assert L.serl_venv_step_auto_wave(engine.ctx, ctypes.byref(d), a.data_ptr(), f64, *out, ctypes.byref(au), None) == _capi.E_INVALID
        assert L.serl_venv_step_auto_wave_noise(engine.ctx, ctypes.byref(d), a.data_ptr(), f64, *out, ctypes.byref(au), ctypes.byref(nz), None) == _capi.E_INVALID
    assert L.serl_venv_step_wave(engine.ctx, ctypes.byref(d), None, 0, *out, None) == _capi.E_INVALID
    assert L.serl_venv_reset_wave(engine.ctx, ctypes.byref(d), None, None, None) == _capi.E_INVALID
    assert L.serl_venv_reset_wave_noise(engine.ctx, ctypes.byref(d), None, env._obs.data_ptr(), None, None) == _capi.E_INVALID
    assert L.serl_venv_step_auto_wave_noise(engine.ctx, ctypes.byref(d), a.data_ptr(), 0, *out, ctypes.byref(au), None, None) == _capi.E_INVALID
    assert b'nz is NULL' in L.serl_last_error()
    pool = torch.zeros(4, 2, 256, dtype=torch.uint8, device=env.device)
    au2 = _capi.VenvAutoDesc.from_buffer_copy(au)
    au2.ref_pool, au2.pool_rows = pool.data_ptr(), 2      # (this env reads tables: desc->ref is set)
    assert L.serl_venv_step_auto_wave(engine.ctx, ctypes.byref(d), a.data_ptr(), 0, *out, ctypes.byref(au2), None) == _capi.E_INVALID
    assert b'desc->ref' in L.serl_last_error()
    torch.cuda.synchronize()
    after = _state(env)
    np.testing.assert_array_equal(before[0], after[0])
    np.testing.assert_array_equal(before[1], after[1])


# ---- 8. nothing else moved -----------------------------------------------------------------------------------------------------------------
def test_default_env_still_runs_the_lane_kernels(engine):
    env = _venv(engine, 3, 'PHlab_attitude_nominal', 0.2, refs=_tables(3, 20, 3))
    assert env.kernel == 'lane' and not env._wave
    env.reset()
    env.step(torch.zeros(3, 3, dtype=torch.float32, device=env.device))
    info = (ctypes.c_int32 * 4)()
    assert engine.lib.serl_venv_last_info(engine.ctx, info) == 0 and info[0] == 12      # SERL_FAMILY_LANE

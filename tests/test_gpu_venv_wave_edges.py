"""The wave env kernels (one wavefront per env: serl_venv_reset_wave / _step_wave / _step_auto_wave, their _noise twins, serl_venv_rollout_wave /
_wave_noise; csrc/venv_wave.inc, venv_wave_rollout.inc) on the three batteries the lane kernels are held to, at ZERO tolerance:

  a, b  the scenarios of tests/env_glue.py (every terminator, cost term, threshold on and one ulp beyond, the time-out residue, the reward clip,
        actions beyond +-1, every fault row, incremental control, the 1 900-step dive) against the literal Python env -- the bodies of
        tests/test_gpu_env_glue.py with kernel='wave'; behind each flight the state buffer against the lane env's that flew the same;
  c     the model clock through tick 2000 on cg_timed and gust, in mid-episode and at a restart, against GlueEnv stepped by hand;
  d     the edge grid of the reference generator (tests/ref_spec_edges.py) -- the bodies of tests/test_gpu_ref_spec.py with kernel='wave';
  e     device-noise episodes replayed on the CPU oracle in every code variant -- tests/test_gpu_venv_noise_replay.py's _replay_case;
  f     sensor_bias / sensor_scale at the ABI of the wave noise entries, and those entries with the generator off against their namesakes.

Every wave copy of the env glue is another hand-written one, and every call moves the 19 states, the 29 bank words, the clock and t from the state buffer into
registers and LDS and back: the long flights far from trim are what exercises that round trip.  Every test asserts what ran (last_step_kernel == 'wave',
last_rollout_path == 'fused-wave').  tests/test_venv_wave_edges_host.py holds the case lists below to the batteries' own."""
import numpy as np
import pytest
import torch

import env_glue as G
import ref_spec_edges as X
import test_gpu_env_glue as E
import test_gpu_ref_spec as P
import test_gpu_venv_noise_replay as Q

pytestmark = pytest.mark.gpu
_np = E._np


def _same_buffers(lane, wave):
    """The Python env has no state buffer, and some of its words reach no output (the S-function work words among the 29 bank words): behind the same
    flight the wave env's buffer must be the lane env's, field for field but for the words test_gpu_venv_wave._same_state leaves out, and so the run buffers
    of an auto-reset env.  Behind the scenarios that is the round trip far from trim: at 60 deg of pitch, 75 deg of roll, 50 m, and 1 900 steps on."""
    from test_gpu_venv_wave import _same_state
    assert lane.last_step_kernel == 'lane' and wave.last_step_kernel == 'wave' and not lane._wave
    _same_state(lane, wave)
    if wave.auto_reset:
        for name in ('_run_return', '_run_length', '_cursor', '_ep_return', '_ep_length'):
            assert torch.equal(getattr(lane, name), getattr(wave, name)), name


# ---- a. the glue scenarios on serl_venv_step_wave / serl_venv_step_auto_wave -----------------------------------------------------------------------
STEP_CASES = [(key, auto) for key in E.STEP for auto in (False, True)]


@pytest.mark.parametrize('key,auto', STEP_CASES, ids=['%s-%s' % (E._id(k), 'auto' if a else 'step') for k, a in STEP_CASES])
def test_wave_step_kernels_on_the_scenarios(engine, key, auto):
    wave = E.step_case(engine, key, auto, kernel='wave')
    _same_buffers(E.step_case(engine, key, auto), wave)


# ---- b. the glue scenarios on serl_venv_rollout_wave ------------------------------------------------------------------------------------------------
ROLL_CASES = list(E.ROLL_CASES)      # ('lane32': the 7-32x3-3 actor, 'general': the one-layer hidden-16 actor; one wave kernel flies both)


@pytest.mark.parametrize('key,shape', ROLL_CASES, ids=['%s-%s' % (E._id(k), s) for k, s in ROLL_CASES])
def test_wave_rollout_kernel_on_the_scenarios(engine, key, shape):
    wave = E.roll_case(engine, key, shape, kernel='wave')
    _same_buffers(E.roll_case(engine, key, shape), wave)


# ---- c. the model clock through tick 2000 under the glue env ---------------------------------------------------------------------------------------
CLOCK_BUILDS = ('cg_timed', 'gust')
CLOCK_TICK0 = (1988, 1994, 1998, 1999, 2000)
CLOCK_ROWS, CLOCK_STEPS, CLOCK_T_MAX = 8, 20, 0.2
CLOCK_BIAS = np.array([[0.2, -0.1, 0.05], [-0.3, 0.2, 0.1], [0.1, 0.3, -0.2], [0.0, -0.25, 0.15], [0.4, 0.1, -0.1]], np.float32)
_CLOCK = {}


def _clock_inputs(build):
    """(reference tables [N, 8, 3], sensor-noise tables [N, 9, 7] or None, the actor's constant output f32 [N, 3], the sinusoid f64 [K, N, 3] added to it)"""
    from serl_amd import builds, refsignals as rs
    from oracle import rollout as R
    N = len(CLOCK_TICK0)
    refs = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=19)[:, :CLOCK_ROWS])
    assert np.isfinite(refs).all() and refs.shape == (N, CLOCK_ROWS, 3)
    sn = None
    if build == 'gust':      # the one of the two with a sensor model
        sn = np.stack([builds.sensor_noise_table(CLOCK_ROWS, np.random.RandomState(500 + e)) for e in range(N)])
    const = np.stack([R.activation('tanh', b) for b in CLOCK_BIAS]).astype(np.float32)
    k, e, c = np.meshgrid(np.arange(CLOCK_STEPS), np.arange(N), np.arange(3), indexing='ij')
    wave = 0.8 * np.sin(0.37 * k + 1.1 * e + 2.0 * c)      # (const + wave leaves [-1, 1] now and then: the sum is clipped)
    return refs, sn, const, wave


def _clock_flight(build):
    """the 20 steps of the 5 envs by GlueEnv, restarted by hand: a restart is a new GlueEnv with the carried error and the clock one tick per reset and one per
    step further on (test_gpu_env_glue._restart_obs).  Flown once per build, shared, never changed."""
    if build not in _CLOCK:
        refs, sn, const, wave = _clock_inputs(build)
        N, K = len(CLOCK_TICK0), CLOCK_STEPS
        out = dict(obs0=np.zeros((N, 7)), obs=np.zeros((K, N, 7)), final_obs=np.zeros((K, N, 7)), x=np.zeros((K, N, 12)), reward=np.zeros((K, N)),
                   done=np.zeros((K, N), bool), ticks=[])
        for e in range(N):
            mk = lambda err, tick: G.GlueEnv(build, G.ATTITUDE, False, None, refs[e], None if sn is None else sn[e], CLOCK_T_MAX, err0=err, tick0=tick)
            tick = CLOCK_TICK0[e]
            env = mk(None, tick)
            out['obs0'][e] = env.reset()
            n, starts = 0, [tick]
            for k in range(K):
                r = env.step(const[e], noise=wave[k, e])
                n += 1
                out['x'][k, e], out['reward'][k, e], out['done'][k, e] = r['x'], r['reward'], r['done']
                out['final_obs'][k, e] = out['obs'][k, e] = r['obs']
                if r['done']:
                    assert not r['fin'] and n == CLOCK_ROWS      # the table ends the episode: no terminator, no time-out
                    tick = tick + 1 + n
                    env = mk(list(env.err), tick)
                    out['obs'][k, e] = env.reset()
                    n = 0
                    starts.append(tick)
            out['ticks'].append(starts)
        # every env's clock passes tick 2000 inside the run: in mid-episode, or with the step its restart takes
        for e, starts in enumerate(out['ticks']):
            assert starts[0] <= 2000 < starts[0] + 3 + K, (e, starts)
        assert any(s < 2000 < s + 1 + CLOCK_ROWS for st in out['ticks'] for s in st) and any(2000 in st for st in out['ticks'])
        assert out['done'].sum(0).tolist() == [2] * N
        _CLOCK[build] = out
    return _CLOCK[build]


def _clock_env(engine, build):
    import serl_amd
    refs, sn, const, wave = _clock_inputs(build)
    env = serl_amd.CitationVecEnv(len(CLOCK_TICK0), mode=E.MODE_OF_BUILD[build], t_max=CLOCK_T_MAX, engine=engine, refs=refs,
                                  sensor_noise=False if sn is None else sn, auto_reset=True, kernel='wave')
    assert (env.build, env.max_steps) == (build, CLOCK_ROWS)
    obs0 = _np(env.reset(tick0=np.array(CLOCK_TICK0, np.int32)))
    assert env.last_step_kernel == 'wave'
    return env, obs0, const, wave


@pytest.mark.parametrize('build', CLOCK_BUILDS)
def test_wave_auto_step_across_the_clock_switch(engine, build):
    """serl_venv_step_auto_wave: f64 actions, the restarts inside the launch carry the error and the clock"""
    want = _clock_flight(build)
    env, obs0, const, wave = _clock_env(engine, build)
    acts = torch.from_numpy(np.clip(const[None].astype(np.float64) + wave, -1.0, 1.0)).to(env.device)
    assert acts.dtype == torch.float64 and bool((acts.abs() == 1.0).any())
    got = {k: [] for k in ('obs', 'final_obs', 'x', 'reward', 'done')}
    for k in range(CLOCK_STEPS):
        obs, rew, done, info = env.step(acts[k])
        for key, v in (('obs', obs), ('final_obs', info['final_obs']), ('x', info['x']), ('reward', rew), ('done', done)):
            got[key].append(_np(v).copy())
    assert env.last_step_kernel == 'wave'
    np.testing.assert_array_equal(obs0, want['obs0'], err_msg='obs0')
    for key in got:
        np.testing.assert_array_equal(np.stack(got[key]), want[key], err_msg=key)


@pytest.mark.parametrize('build', CLOCK_BUILDS)
def test_wave_rollout_across_the_clock_switch(engine, build):
    """serl_venv_rollout_wave: a zero-weight actor per env whose output is the script's constant, the sinusoid as its action-noise rows"""
    import serl_amd
    from oracle import rollout as R
    want = _clock_flight(build)
    env, obs0, const, wave = _clock_env(engine, build)
    N, K, H, L = len(CLOCK_TICK0), CLOCK_STEPS, 16, 1
    Pn = R.param_count(7, H, L, 3)
    w = np.zeros((N, (Pn + 3) // 4 * 4), np.float32)
    w[:, Pn - 3:Pn] = CLOCK_BIAS
    out = env.rollout(torch.from_numpy(w).to(env.device), K, spec=serl_amd.NetSpec(7, 3, H, L, 'tanh'), member_of_env=np.arange(N, dtype=np.int32),
                      action_noise=wave, transitions=True, path='fused')
    assert env.last_rollout_path == 'fused-wave'
    out = {k: _np(v) for k, v in out.items()}
    np.testing.assert_array_equal(out['obs'][0], want['obs0'], err_msg='obs0')
    np.testing.assert_array_equal(out['obs'][1:], want['obs'], err_msg='obs')
    for key in ('final_obs', 'x', 'reward', 'done'):
        np.testing.assert_array_equal(out[key], want[key], err_msg=key)
    np.testing.assert_array_equal(out['actions'], np.clip(const[None].astype(np.float64) + wave, -1.0, 1.0), err_msg='actions')


# ---- d. the reference generator's edge grid ---------------------------------------------------------------------------------------------------------
GEN_MODES = ['nominal', 'gust']
GEN_STEP_CASES = [(kernel_, kind, mode, t_max) for kernel_, kind in P.ENV_KINDS for mode in GEN_MODES for t_max in P.T_MAXES]
GEN_ROLL_CASES = [(which, kind, mode, t_max) for which in ('lane32', 'general') for kind in ('rows', 'shared', 'pool') for mode in GEN_MODES
                  for t_max in P.T_MAXES]
GEN_TAIL_CASES = ['step', 'auto', 'pool', 'general']


@pytest.mark.parametrize('kernel_,kind,mode,t_max', GEN_STEP_CASES, ids=['%s-%s-%s-%g' % c for c in GEN_STEP_CASES])
def test_env_step_returns_the_generated_reference(engine, kernel_, kind, mode, t_max):
    """serl_venv_step_wave / serl_venv_step_auto_wave: every sample tabulate_specs' bit for bit, no episode ends early, the pool's cursor"""
    P.step_ref_case(engine, kernel_, kind, mode, t_max, kernel='wave')


@pytest.mark.parametrize('which,kind,mode,t_max', GEN_ROLL_CASES, ids=['%s-%s-%s-%g' % c for c in GEN_ROLL_CASES])
def test_env_rollout_returns_the_generated_reference(engine, golden, which, kind, mode, t_max):
    """serl_venv_rollout_wave with the SERL50 golden actors ('lane32') and the hidden-72 actors ('general')"""
    P.rollout_ref_case(engine, golden, which, kind, mode, t_max, kernel='wave')


@pytest.mark.parametrize('what', GEN_TAIL_CASES)
def test_entries_past_n_are_not_read_by_the_env_kernels(engine, golden, what):
    P.tails_case(engine, golden, what, kernel='wave')


# ---- e. device-noise episodes replayed on the CPU oracle --------------------------------------------------------------------------------------------
# the modes of the lane tests (test_rollout_noise_ / test_rollout_general_noise_ / test_step_auto_noise_and_reset_noise_replay_on_the_oracle)
REPLAY_32 = ['noise', 'ice', 'cg-timed', 'gust', 'test', 'jr']
REPLAY_8 = ['gust', 'cg-timed', 'PHlab_symmetric_noise', 'PHlab_full_noise', 'PHlab_attitude_incremental', 'PHlab_symmetric_incremental',
            'PHlab_full_incremental']
REPLAY_LOOP = ['ice', 'cg-timed', 'test', 'PHlab_full_noise', 'PHlab_symmetric_incremental']
# (mode, hidden, layers, N, path): N = 70 is two groups of wavefronts across the 64-env padding of the state buffer
REPLAY_CASES = ([(m, 32, 3, 70, 'fused') for m in REPLAY_32] + [(m, 8, 1, 70, 'fused') for m in REPLAY_8] + [(m, 8, 1, 5, 'loop') for m in REPLAY_LOOP])
SWITCH_CASES = [(m, h, l, n, p) for m in ('cg-timed', 'gust') for h, l, n, p in ((32, 3, 70, 'fused'), (8, 1, 70, 'fused'), (8, 1, 5, 'loop'))]


def _replay(engine, mode, hidden, layers, N, path, clock0=None):
    ran = 'fused-wave' if path == 'fused' else 'loop'
    env = Q._replay_case(engine, mode, N, hidden, layers, path, ran, clock0=clock0, kernel='wave')
    assert env._wave and env.last_step_kernel == 'wave' and env.last_rollout_path == ran


@pytest.mark.parametrize('mode,hidden,layers,N,path', REPLAY_CASES, ids=['%s-%dx%d-%d-%s' % c for c in REPLAY_CASES])
def test_wave_noise_replays_on_the_oracle(engine, mode, hidden, layers, N, path):
    """serl_venv_rollout_wave_noise (path='fused'); serl_venv_step_auto_wave_noise + serl_venv_reset_wave_noise (path='loop')"""
    _replay(engine, mode, hidden, layers, N, path)


@pytest.mark.parametrize('mode,hidden,layers,N,path', SWITCH_CASES, ids=['%s-%dx%d-%d-%s' % c for c in SWITCH_CASES])
def test_wave_replay_across_the_clock_switch(engine, mode, hidden, layers, N, path):
    _replay(engine, mode, hidden, layers, N, path, clock0=Q._switch_clocks(N))


# ---- f. the free ABI parameters of the wave noise entries -------------------------------------------------------------------------------------------
def test_step_auto_wave_noise_applies_the_callers_bias_and_scale(engine):
    """serl_venv_reset_wave_noise and one serl_venv_step_auto_wave_noise step with BIAS / SCALE against the table path fed by the fill kernel"""
    Q.bias_and_scale_case(engine, wave=True)


def test_generator_off_reset_and_step_equal_their_namesakes(engine):
    """serl_venv_reset_wave_noise / serl_venv_step_auto_wave_noise with nz->sensor = 0 against serl_venv_reset_wave / serl_venv_step_auto_wave, state buffer included"""
    Q.generator_off_step_case(engine, wave=True)


@pytest.mark.parametrize('hidden,layers,path,ran', [(32, 3, 'fused', 'fused-wave'), (8, 1, 'fused', 'fused-wave'), (8, 1, 'loop', 'loop')])
def test_generator_off_rollout_equals_its_namesake(engine, hidden, layers, path, ran):
    """serl_venv_rollout_wave_noise with nz->sensor = nz->action = 0 and an action table against serl_venv_rollout_wave, key for key and in the env state"""
    Q.generator_off_rollout_case(engine, hidden, layers, path, ran, wave=True)

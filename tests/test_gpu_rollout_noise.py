"""Population rollouts with the sensor and exploration noise drawn inside the kernels (serl_rollout_noise; RolloutEngine.rollout
sensor_noise='device' / action_noise='device'; evaluate_pop(sensor_noise='device')) at ZERO tolerance.

The device path of a kernel family is held to the same family fed the tables `serl_amd.venv_noise` writes for the same keys, and those
tables go through the CPU oracle (same-libm flavour) as in tests/test_gpu_venv_noise_replay.py: fitness, lengths, length_t, cost steps,
action / state / reward traces and transition rows.  Lane launches fly lanes_per_wave = 4 (5 episodes: two wavefronts, one partial),
wave launches kernel='wave' (5 episodes: a partial workgroup); every launch asserts through last_rollout_info() which family ran.
Episodes are 0.5 s (51 steps) but where an episode has to outlive a crashed neighbour (3 s)."""
import ctypes
import numpy as np
import pytest
import torch

from actor_shapes import make_weights, _shape, spec_of, net_of

pytestmark = pytest.mark.gpu
SEED = 0x0DDBA11C0FFEE123
SD, CLIP = 0.3, 0.5
T_SHORT = 0.5
KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps', 'actions', 'states', 'rewards', 'transitions')
FAMILY_KW = {'lane': dict(lanes_per_wave=4), 'wave': dict(kernel='wave')}
ENV = np.array([7, 3, 3, 0, 1], np.int32)
EPISODE = np.array([0, 2, 2, 5, 0], np.int32)


def _np(t):
    return t.cpu().numpy()


def _refs(E, t_max=T_SHORT, seed=41):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(E, 2, 20, seed=seed)[:, :rs.n_steps_for(t_max)])
    assert np.isfinite(r).all()
    return r


def _err0(E):
    return (np.arange(E * 3).reshape(E, 3) % 7 - 3) * 2.0e-3


def _fly(engine, family, w, s, moe, refs, build='h2000_v90', t_max=T_SHORT, **kw):
    """one launch on `family`'s kernels -> numpy outputs (not synchronised by rollout(): a negative length is a result here)"""
    out = engine.rollout(torch.from_numpy(w), spec_of(s), moe, refs, build=build, t_max=t_max, traces=True, transitions=True, sync=False,
                         env_config=s['env_config'], incremental=s['incremental'], **FAMILY_KW[family], **kw)
    general = s['env_config'] != 0 or s['incremental']
    assert engine.last_rollout_info()['family'] == ('wavex' if general else family)
    torch.cuda.synchronize()
    return {k: _np(out[k]) for k in KEYS}


def _tables(engine, env, episode, T, sd=SD, clip=CLIP):
    import serl_amd
    sn = _np(serl_amd.venv_noise(SEED, env, episode, T + 1, 'sensor', engine=engine))
    an = _np(serl_amd.venv_noise(SEED, env, episode, T, 'action', noise_sd=sd, noise_clip=clip, engine=engine))
    assert sn.shape == (len(env), T + 1, 7) and an.shape == (len(env), T, 3)
    return sn, an


def _same(a, b, what='', rows=None):
    for k in KEYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        np.testing.assert_array_equal(x, y, err_msg='%s: %s' % (what, k))


def _same_as_oracle(g, o, what=''):
    """the oracle's traces are compared over the steps an episode flew"""
    for k in ('fitness', 'length_steps', 'length_t', 'cost_steps'):
        np.testing.assert_array_equal(g[k], o[k], err_msg='%s: oracle %s' % (what, k))
    for e, n in enumerate(np.abs(g['length_steps'])):
        for k in ('actions', 'states', 'rewards', 'transitions'):
            np.testing.assert_array_equal(g[k][e, :n], o[k][e, :n], err_msg='%s: oracle %s of episode %d' % (what, k, e))


def _device_table_oracle(engine, family, mode, s, w, moe, refs, *, t_max=T_SHORT, env=None, episode=None, sd=SD, clip=CLIP, err0=None, tick0=None,
                         sensor=True, action=True, oracle=True, what=''):
    """the device-noise launch, the same family on venv_noise's tables, the oracle on those tables -> (device, table, sensor table, action table)"""
    from serl_amd import builds
    from oracle import rollout as R
    E, T = len(moe), refs.shape[-2]
    build, row = builds.resolve_mode(mode)
    faults = None if row == builds.NOMINAL_ROW else [list(row)] * E
    env = np.arange(E, dtype=np.int32) if env is None else env
    episode = np.zeros(E, np.int32) if episode is None else episode
    sn, an = _tables(engine, env, episode, T, sd, clip)
    common = dict(build=build, t_max=t_max, faults=faults, err0=err0, tick0=tick0)
    nzkw = dict(noise_seed=SEED, noise_env=env, noise_episode=episode)
    if sensor:
        nzkw['sensor_noise'] = 'device'
    if action:
        nzkw.update(action_noise='device', noise_sd=sd, noise_clip=clip)
    dev = _fly(engine, family, w, s, moe, refs, **common, **nzkw)
    tab = _fly(engine, family, w, s, moe, refs, sensor_noise=sn if sensor else None, action_noise=an if action else None, **common)
    _same(dev, tab, what + ' device against table')
    if not oracle:
        return dev, tab, sn, an
    orc = R.rollout(w, net_of(s), moe, refs, build=build, faults=faults, err0=err0, tick0=tick0, action_noise=an if action else None,
                    sensor_noise=sn if sensor else None, t_max=t_max, traces=True, transitions=True, threads=min(8, E), env_config=s['env_config'],
                    incremental=s['incremental'], short_libm=True)
    _same_as_oracle(dev, orc, what)
    return dev, tab, sn, an


# the nominal code flies its own sensor-noise mode, the gust code too; the other three get the 'noise' sensor model through the low-level rollout
@pytest.mark.parametrize('mode', ['noise', 'ice', 'cg-timed', 'gust', 'test'])
@pytest.mark.parametrize('family', ['lane', 'wave'])
def test_device_path_equals_table_path_and_oracle(engine, family, mode):
    E = 5
    s = _shape(32, 3)
    w = np.ascontiguousarray(make_weights(s, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    refs = _refs(E)
    tick0 = 1975 + 6 * np.arange(E, dtype=np.int32) if mode in ('gust', 'cg-timed') else None      # the builds switch at tick 2000: inside these episodes
    dev, _, sn, an = _device_table_oracle(engine, family, mode, s, w, moe, refs, err0=_err0(E), tick0=tick0, what='%s %s' % (family, mode))
    assert (np.abs(dev['length_steps']) > 40).all() and np.isfinite(dev['states']).all()
    from serl_amd import builds
    quiet = _fly(engine, family, w, s, moe, refs, build=builds.resolve_mode(mode)[0], err0=_err0(E), tick0=tick0)
    assert (quiet['transitions'][:, 0, :7] != dev['transitions'][:, 0, :7]).any(-1).all(), 'a first observation carries no sensor noise'
    assert (quiet['fitness'] != dev['fitness']).all()
    assert (np.abs(an) == CLIP).any() and (np.abs(an) < CLIP).any()


@pytest.mark.parametrize('mode', ['PHlab_symmetric_nominal', 'PHlab_full_incremental'])
def test_wavex_device_path_equals_table_path_and_oracle(engine, mode):
    """the other env configurations (A = 1: only the first action column is used; rate control)"""
    from serl_amd import builds
    cfg, incr = builds.env_config(mode)
    s = _shape(8, 1, 'tanh', cfg, incr)
    E = 3
    w = np.ascontiguousarray(make_weights(s, 2, 5))
    moe = np.arange(E, dtype=np.int32) % 2
    dev, _, _, _ = _device_table_oracle(engine, 'wave', mode, s, w, moe, _refs(E), err0=_err0(E), what=mode)
    assert (np.abs(dev['length_steps']) > 40).all()


def _crashing_and_benign():
    """member 0: an output bias that saturates all three actions -- the aircraft leaves the attitude bounds long before 3 s; member 1: benign"""
    s = _shape(32, 3)
    w = np.ascontiguousarray(make_weights(s, 2, 7))
    P = 32 * 7 + 32 + 3 * (32 * 32 + 3 * 32) + 3 * 32 + 3
    w[0, P - 3:P] = 6.0
    return s, w


def test_lanes_of_one_wavefront_at_different_steps(engine):
    """one lane wavefront: an episode that ends early beside one that flies on -- the exploration noise entry is the LANE's step"""
    s, w = _crashing_and_benign()
    moe = np.array([0, 1], np.int32)
    refs = _refs(2, 3.0, seed=3)
    T = refs.shape[1]
    dev, tab, _, _ = _device_table_oracle(engine, 'lane', 'noise', s, w, moe, refs, t_max=3.0, what='crash beside benign')
    assert 0 < tab['length_steps'][0] < T // 2, 'the table path itself must end early'
    assert tab['length_steps'][1] == T
    np.testing.assert_array_equal(dev['length_steps'], tab['length_steps'])


def test_reference_table_shorter_than_the_episode(engine):
    """a reference table that ends before t_max: the length is negative and the draws stop with the table.  The oracle refuses such a table;
    it flies the whole one, and its first 37 steps are the comparison"""
    from oracle import rollout as R
    s = _shape(32, 3)
    w = np.ascontiguousarray(make_weights(s, 1, 9))
    moe = np.zeros(1, np.int32)
    full = _refs(1, 3.0)
    sn, an = _tables(engine, moe, moe, full.shape[1])
    orc = R.rollout(w, net_of(s), moe, full, action_noise=an, sensor_noise=sn, t_max=3.0, traces=True, transitions=True, short_libm=True)
    assert orc['length_steps'][0] > 37
    for family in ('lane', 'wave'):
        dev, _, _, _ = _device_table_oracle(engine, family, 'noise', s, w, moe, np.ascontiguousarray(full[:, :37]), t_max=3.0, oracle=False, what=family)
        assert dev['length_steps'][0] == -37
        for k in ('actions', 'states', 'rewards', 'transitions'):
            np.testing.assert_array_equal(dev[k][0], orc[k][0, :37], err_msg='%s: oracle %s' % (family, k))


def test_keys_not_positions_decide_the_draws(engine):
    s = _shape(32, 3)
    w = np.ascontiguousarray(make_weights(s, 3, 21))
    moe = np.array([0, 1, 1, 2, 0], np.int32)
    refs = _refs(5)
    refs[2] = refs[1]
    out = {}
    for family in ('lane', 'wave'):
        out[family], _, _, _ = _device_table_oracle(engine, family, 'noise', s, w, moe, refs, env=ENV, episode=EPISODE, what=family)
        for k in KEYS:
            np.testing.assert_array_equal(out[family][k][1], out[family][k][2], err_msg=k)
        assert len(set(out[family]['fitness'])) == 4
        perm = np.array([3, 0, 4, 2, 1])
        p = _fly(engine, family, w, s, moe[perm], np.ascontiguousarray(refs[perm]), sensor_noise='device', action_noise='device', noise_sd=SD,
                 noise_clip=CLIP, noise_seed=SEED, noise_env=ENV[perm], noise_episode=EPISODE[perm])
        for k in KEYS:
            np.testing.assert_array_equal(p[k], out[family][k][perm], err_msg='%s permuted: %s' % (family, k))
    _same(out['lane'], out['wave'], 'lane against wave')
    # the default keys are (e, 0): another realisation
    d = _fly(engine, 'lane', w, s, moe, refs, sensor_noise='device', action_noise='device', noise_sd=SD, noise_clip=CLIP, noise_seed=SEED)
    assert (d['fitness'][:4] != out['lane']['fitness'][:4]).all()
    np.testing.assert_array_equal(d['fitness'][4], _fly(engine, 'lane', w, s, moe, refs, sensor_noise='device', action_noise='device', noise_sd=SD,
                                                        noise_clip=CLIP, noise_seed=SEED, noise_env=np.arange(5, dtype=np.int32),
                                                        noise_episode=np.zeros(5, np.int32))['fitness'][4])


@pytest.mark.parametrize('family', ['lane', 'wave'])
def test_masks(engine, family):
    """sensor_row / noise_row < 0 switch an episode's draws off: the exploration-episode pattern"""
    s = _shape(32, 3)
    E = 5
    w = np.ascontiguousarray(make_weights(s, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    refs = _refs(E)
    T = refs.shape[1]
    srow, nrow = np.array([0, -1, 0, -1, 0], np.int32), np.array([-1, -1, -1, -1, 0], np.int32)
    dev = _fly(engine, family, w, s, moe, refs, sensor_noise='device', action_noise='device', noise_sd=SD, noise_clip=CLIP, noise_seed=SEED,
               sensor_row=srow, noise_row=nrow)
    sn, an = _tables(engine, np.arange(E, dtype=np.int32), np.zeros(E, np.int32), T)
    tab = _fly(engine, family, w, s, moe, refs, sensor_noise=sn, sensor_row=np.where(srow < 0, -1, np.arange(E)).astype(np.int32),
               action_noise=an, noise_row=np.where(nrow < 0, -1, np.arange(E)).astype(np.int32))
    _same(dev, tab, 'masked device against masked table')
    plain = _fly(engine, family, w, s, moe, refs)
    _same(dev, plain, 'masked episodes against no noise', rows=[1, 3])
    assert (dev['fitness'][[0, 2, 4]] != plain['fitness'][[0, 2, 4]]).all()
    sensor_only = _fly(engine, family, w, s, moe, refs, sensor_noise=sn)
    _same(dev, sensor_only, 'sensor noise, no exploration noise', rows=[0, 2])
    assert dev['fitness'][4] != sensor_only['fitness'][4]


@pytest.mark.parametrize('family', ['lane', 'wave'])
def test_action_noise_clip_and_zero_sd(engine, family):
    s = _shape(32, 3)
    E = 5
    w = np.ascontiguousarray(make_weights(s, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    refs = _refs(E)
    _, _, _, an = _device_table_oracle(engine, family, 'nominal', s, w, moe, refs, sd=2.0, clip=0.05, sensor=False, what='clip binds')
    assert (np.abs(an) == 0.05).mean() > 0.9 and (np.abs(an) < 0.05).any(), 'the clip must bind on most steps'
    # sd = 0: the table path with a zero table (the f64 action scaling; the no-noise path scales in f32)
    dev = _fly(engine, family, w, s, moe, refs, action_noise='device', noise_sd=0.0, noise_clip=0.5, noise_seed=SEED)
    tab = _fly(engine, family, w, s, moe, refs, action_noise=np.zeros((E, refs.shape[1], 3)))
    _same(dev, tab, 'sd = 0 against a zero table')


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def _prepared(engine, family, **kw):
    """a descriptor rollout() prepared and did not launch, with its outputs"""
    s = _shape(32, 3)
    E = 5
    w = np.ascontiguousarray(make_weights(s, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    return engine.rollout(torch.from_numpy(w), spec_of(s), moe, _refs(E), t_max=T_SHORT, traces=True, transitions=True, launch=False,
                          **FAMILY_KW[family], **kw)


def _nz(**kw):
    from serl_amd import _capi, builds
    bias, scale = builds.sensor_bias_scale()
    args = dict(seed=SEED, sensor=0, action=0, sensor_bias=(ctypes.c_double * 7)(*bias), sensor_scale=(ctypes.c_double * 7)(*scale), action_sd=SD,
                action_clip=CLIP)
    args.update(kw)
    return _capi.RolloutNoiseDesc(**args)


def _call(engine, prepared, nz):
    stream = ctypes.c_void_p(torch.cuda.current_stream(engine.device).cuda_stream)
    return engine.lib.serl_rollout_noise(engine.ctx, ctypes.byref(prepared['_desc']), None if nz is None else ctypes.byref(nz), stream)


@pytest.mark.parametrize('family', ['lane', 'wave'])
def test_generator_off_equals_serl_rollout(engine, family):
    """nz->sensor = nz->action = 0: the noise instantiation on the caller's tables against serl_rollout, in every output"""
    E, T = 5, _refs(5).shape[1]
    sn, an = _tables(engine, ENV, EPISODE, T)
    a, b = _prepared(engine, family, sensor_noise=sn, action_noise=an), _prepared(engine, family, sensor_noise=sn, action_noise=an)
    assert _call(engine, a, _nz()) == 0, engine.lib.serl_last_error()
    assert engine.last_rollout_info()['family'] == family
    stream = ctypes.c_void_p(torch.cuda.current_stream(engine.device).cuda_stream)
    assert engine.lib.serl_rollout(engine.ctx, ctypes.byref(b['_desc']), stream) == 0
    assert engine.last_rollout_info()['family'] == family
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert (a['length_steps'] != 0).all() and a['actions'].abs().max() > 0


def test_refusals_before_any_launch(engine):
    from serl_amd import _capi
    L = engine.lib
    E, T = 5, _refs(5).shape[1]
    sn, an = _tables(engine, ENV, EPISODE, T)

    def refused(p, nz, rc, word):
        assert _call(engine, p, nz) == rc, (word, L.serl_last_error())
        assert word in L.serl_last_error(), L.serl_last_error()
        torch.cuda.synchronize()
        assert not bool(p['fitness'].any()) and not bool(p['length_steps'].any()) and not bool(p['transitions'].any()), 'something was launched'

    p = _prepared(engine, 'wave')
    for hint in ('team', 'team2', 'team4', 'half', 'laneq'):
        p['_desc'].kernel_hint = _capi.KERNEL_HINTS[hint]
        refused(p, _nz(sensor=1, action=1), _capi.E_UNSUPPORTED, b'no noise instantiation')
    p['_desc'].kernel_hint = _capi.KERNEL_HINTS['wave']
    refused(p, None, _capi.E_INVALID, b'nz is NULL')
    refused(p, _nz(sensor=2), _capi.E_INVALID, b'0 or 1')
    for kw in (dict(action_sd=-1.0), dict(action_clip=-1.0), dict(action_sd=float('nan')), dict(action_clip=float('nan'))):
        refused(p, _nz(action=1, **kw), _capi.E_INVALID, b'action_sd')
    refused(_prepared(engine, 'wave', sensor_noise=sn), _nz(sensor=1), _capi.E_INVALID, b'sensor_noise together')
    refused(_prepared(engine, 'lane', action_noise=an), _nz(action=1), _capi.E_INVALID, b'action_noise together')
    p['_desc'].n_episodes = 0      # what serl_rollout refuses
    refused(p, _nz(sensor=1), _capi.E_INVALID, b'n_episodes')
    # a table beside the OTHER generator flag is served
    q = _prepared(engine, 'lane', action_noise=an)
    assert _call(engine, q, _nz(sensor=1)) == 0
    torch.cuda.synchronize()
    assert bool((q['length_steps'] != 0).all())


def test_python_argument_errors(engine):
    s = _shape(32, 3)
    w = torch.from_numpy(np.ascontiguousarray(make_weights(s, 1, 3)))
    base = dict(t_max=T_SHORT)
    fly = lambda **kw: engine.rollout(w, spec_of(s), [0, 0], _refs(2), **base, **kw)
    for kw in (dict(sensor_noise='host'), dict(sensor_noise='device'), dict(sensor_noise='device', noise_seed=-1),
               dict(action_noise='device', noise_seed=1), dict(action_noise='device', noise_seed=1, noise_sd=-0.1, noise_clip=1.0),
               dict(noise_sd=0.1, noise_clip=0.1), dict(noise_seed=1), dict(sensor_noise='device', noise_seed=1, noise_env=[0, 1, 2]),
               dict(sensor_noise='device', noise_seed=1, noise_episode=[0.5, 1.0]), dict(sensor_noise='device', noise_seed=1, sensor_row=[0]),
               dict(sensor_noise='device', noise_seed=1, kernel='team4'), dict(sensor_noise='device', noise_seed=1, kernel='laneq'),
               dict(sensor_noise='device', noise_seed=1, launch=False)):
        with pytest.raises(ValueError):
            fly(**kw)


# ---- evaluate_pop ------------------------------------------------------------------------------------------------------------------------------
def _pop_reference(engine, w, s, modes, num_evals, seed, t_max, noise_episode=0):
    """evaluate_pop on host tables: per build, RolloutEngine.rollout with venv_noise(seed, e, noise_episode) rows for the noisy episodes"""
    import serl_amd
    from serl_amd import builds, refsignals
    E = len(modes)
    moe = np.repeat(np.arange(E // num_evals, dtype=np.int32), num_evals)
    ref = refsignals.tabulate(*refsignals.base_reference(t_max), t_max)
    T = ref.shape[0]
    fit, ls, lt = np.zeros(E), np.zeros(E, np.int32), np.zeros(E)
    for b in sorted({builds.resolve_mode(m)[0] for m in modes}):
        idx = np.array([e for e in range(E) if builds.resolve_mode(modes[e])[0] == b])
        noisy = [e for e in idx if builds.has_sensor_noise(modes[e])]
        sn = _np(serl_amd.venv_noise(seed, np.array(noisy, np.int32), noise_episode, T + 1, 'sensor', engine=engine))
        pos = {e: j for j, e in enumerate(noisy)}
        o = engine.rollout(torch.from_numpy(w), spec_of(s), moe[idx], ref, build=b, t_max=t_max, sensor_noise=sn,
                           sensor_row=np.array([pos.get(e, -1) for e in idx], np.int32), kernel='wave')
        fit[idx], ls[idx], lt[idx] = _np(o['fitness']), _np(o['length_steps']), _np(o['length_t'])
    sh = lambda a: np.ascontiguousarray(a.reshape(E // num_evals, num_evals).T)
    return sh(fit), sh(ls), sh(lt)


@pytest.mark.parametrize('modes', [['noise'] * 4, ['noise', 'gust', 'gust', 'noise']], ids=['noise', 'noise+gust'])
def test_evaluate_pop_device_sensor_noise(engine, modes):
    import serl_amd
    s = _shape(32, 3)
    w = np.ascontiguousarray(make_weights(s, 2, 21))
    seed = 0x1234567890ABCDEF
    kw = dict(mode=modes if len(set(modes)) > 1 else modes[0], num_evals=2, t_max=1.0, spec=spec_of(s), engine=engine, sensor_noise='device')
    r = serl_amd.evaluate_pop(torch.from_numpy(w), seed=seed, **kw)
    assert engine.last_rollout_info()['family'] == 'wave' and r.noise_seed == seed
    fit, ls, lt = _pop_reference(engine, w, s, modes, 2, seed, 1.0)
    np.testing.assert_array_equal(r.returns, fit)
    np.testing.assert_array_equal(r.length_steps, ls)
    np.testing.assert_array_equal(r.length_t, lt)
    again = serl_amd.evaluate_pop(torch.from_numpy(w), seed=seed, **kw)
    np.testing.assert_array_equal(again.returns, r.returns)
    other = serl_amd.evaluate_pop(torch.from_numpy(w), seed=seed, noise_episode=1, **kw)
    assert (other.returns != r.returns).all()
    np.testing.assert_array_equal(other.returns, _pop_reference(engine, w, s, modes, 2, seed, 1.0, noise_episode=1)[0])
    drawn = serl_amd.evaluate_pop(torch.from_numpy(w), **kw)
    assert isinstance(drawn.noise_seed, int) and 0 <= drawn.noise_seed < 2**64 and drawn.noise_seed != seed
    for bad in (dict(sensor_noise='table'), dict(sensor_rng=np.random.RandomState(1)), dict(seed=-3), dict(kernel='team4'), dict(noise_episode=0.5)):
        with pytest.raises(ValueError):
            serl_amd.evaluate_pop(torch.from_numpy(w), **dict(kw, **bad))


def test_the_env_and_the_population_rollout_draw_the_same(engine):
    """CitationVecEnv's device noise and the population rollout's are one generator: env e's first episode is episode (e, 0)"""
    import serl_amd
    from serl_amd import refsignals as rs
    s = _shape(32, 3)
    N, K = 3, 20
    w = np.ascontiguousarray(make_weights(s, 3, 21))
    moe = np.arange(N, dtype=np.int32)
    specs = rs.ref_specs([rs.SmoothedStepSequence([0.0, 0.1 + 0.05 * e, 0.3], [5.0 - e, -3.0, 2.0 + e], 0.15) for e in range(N)],
                         [rs.SmoothedStepSequence([0.05, 0.2 + 0.03 * e], [4.0, -4.0 + e], 0.1) for e in range(N)], [0.2106] * N)
    env = serl_amd.CitationVecEnv(N, mode='noise', sensor_noise='device', seed=SEED, auto_reset=True, refs=specs, t_max=T_SHORT, engine=engine)
    env.reset()
    got = env.rollout(torch.from_numpy(w).to(env.device), K, spec=spec_of(s), member_of_env=moe, path='fused')
    assert env.last_rollout_path == 'fused' and not bool(got['done'].any())
    pop = _fly(engine, 'lane', w, s, moe, specs, sensor_noise='device', noise_seed=SEED, noise_env=np.arange(N, dtype=np.int32))
    tr = pop['transitions']
    obs, reward = _np(got['obs']), _np(got['reward'])
    for e in range(N):
        np.testing.assert_array_equal(obs[:K, e].astype(np.float32), tr[e, :K, :7])
        np.testing.assert_array_equal(obs[1:K + 1, e].astype(np.float32), tr[e, :K, 10:17])
        np.testing.assert_array_equal(reward[:, e], pop['rewards'][e, :K])

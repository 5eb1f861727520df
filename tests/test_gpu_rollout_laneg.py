"""The lane-per-episode population kernel for every actor shape (kernel='laneg': kernel_hint SERL_KERNEL_LANEG, csrc/family_laneg.hip and its device-noise
twin family_lanegn.hip -- every live lane runs lane_actor.h serl_actor_forward_lane_general over its own member's row) at ZERO tolerance.

Every launch asserts through last_rollout_info() that family 14 ('laneg') ran, and everything rollout() returns -- fitness, length_steps, length_t,
cost_steps, the action / state / reward traces, the transition rows -- is held bit for bit to the same call with kernel='wave' (one wavefront per
episode), to the same lanes_per_wave without the hint (the existing lane kernel: up to 64 wavefront-wide forward passes per env step) and to the CPU
oracle's same-libm flavour.  Flights are 0.5 .. 2 s.  The shapes are the smallest at which this forward can go wrong: hidden 4 (one 16-byte group, the
H - 4 clamp of serl_lane_rows), 20 (H % 16 != 0: the zero-padded LayerNorm block), 72 x 3, 96 x 3, 128 x 1, no hidden layer, 16 hidden layers at
hidden 8; each activation at least once."""
import numpy as np
import pytest
import torch

import actor_shapes as X
from test_gpu_rollout import ran, _oracle

pytestmark = pytest.mark.gpu
KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps', 'actions', 'states', 'rewards', 'transitions')
S72 = X._shape(72, 3)
SEED = 0x5EED1A9E0C0FFEE5
SD, CLIP = 0.3, 0.5


def _np(t):
    return t.cpu().numpy()


def _refs(E, t_max, seed=41):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(E, 2, 20, seed=seed)[:, :rs.n_steps_for(t_max)])
    assert np.isfinite(r).all()
    return r


def _fly(engine, flavour, w, s, moe, refs, lanes, **kw):
    """one launch -> numpy outputs.  flavour 'laneg': the hint with `lanes` lanes per wavefront; 'lane': the same lanes_per_wave without the hint;
    'wave': kernel='wave'.  The family that ran is asserted (not synchronised by rollout(): a negative length would be a result here)."""
    E = len(moe)
    call = {'laneg': dict(kernel='laneg', lanes_per_wave=lanes), 'lane': dict(lanes_per_wave=lanes), 'wave': dict(kernel='wave')}[flavour]
    out = engine.rollout(torch.from_numpy(w), X.spec_of(s), moe, refs, traces=True, transitions=True, sync=False, **call, **kw)
    if flavour == 'wave':
        ran(engine, 'wave')
    else:
        per = lanes if lanes > 0 else 64
        info = ran(engine, flavour, episodes_per_team=per, work_queue=False, actor_wavefronts=0, actor_streamed=True, launches=1)
        plan = engine.plan_rollout(X.spec_of(s), E, **call)
        assert info['workgroups'] == plan['workgroups'] and plan['workgroups'] * (plan['block'] // 64) >= -(-E // per)
        assert flavour == 'lane' or not plan['regroup']      # the hint streams the rows as they lie, at hidden 32 too
    torch.cuda.synchronize()
    return {k: _np(out[k]) for k in KEYS}


def _same(a, b, what):
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (what, k))


def _same_as_oracle(g, o, what):
    """the oracle's traces are compared over the steps an episode flew"""
    for k in ('fitness', 'length_steps', 'length_t', 'cost_steps'):
        np.testing.assert_array_equal(g[k], o[k], err_msg='%s: oracle %s' % (what, k))
    for e, n in enumerate(np.abs(g['length_steps'])):
        for k in ('actions', 'states', 'rewards', 'transitions'):
            np.testing.assert_array_equal(g[k][e, :n], o[k][e, :n], err_msg='%s: oracle %s of episode %d' % (what, k, e))


def _all_flavours(engine, w, s, moe, refs, lanes, what, oracle=True, **kw):
    """kernel='laneg' against kernel='wave', against the same lanes_per_wave without the hint and (oracle=True) against the CPU oracle -> the laneg outputs"""
    g = _fly(engine, 'laneg', w, s, moe, refs, lanes, **kw)
    assert (g['length_steps'] != 0).all(), what + ': an episode was not written'
    _same(g, _fly(engine, 'wave', w, s, moe, refs, lanes, **kw), what + ' against wave')
    _same(g, _fly(engine, 'lane', w, s, moe, refs, lanes if lanes > 0 else 64, **kw), what + ' against the lane kernel without the hint')
    if oracle:
        o = _oracle(w, X.net_of(s), moe, refs, traces=True, transitions=True, threads=min(8, len(moe)), **kw)
        _same_as_oracle(g, o, what)
    return g


SHAPES = [X._shape(4, 3), X._shape(20, 3, 'elu'), X._shape(72, 3), X._shape(96, 3, 'relu'), X._shape(128, 1), X._shape(32, 0, 'relu'), X._shape(8, 16, 'elu'),
          X._shape(32, 3)]


@pytest.mark.parametrize('s', SHAPES, ids=X.shape_id)
def test_shapes(engine, s):
    """5 episodes at 3 lanes per wavefront (two wavefronts, the second partly filled), every episode a member of its own, 1 s"""
    i = SHAPES.index(s)
    w = np.ascontiguousarray(X.make_weights(s, 5, 400 + i))
    moe = np.array([3, 0, 4, 1, 2], np.int32)
    refs = _refs(5, 1.0, seed=60 + i)
    g = _all_flavours(engine, w, s, moe, refs, 3, X.shape_id(s), t_max=1.0)
    assert (g['length_steps'] == refs.shape[1]).all()      # these actors fly the table out: every step of 1 s was compared
    X.check_actions_f64(s, w, moe, g['transitions'], g['length_steps'], X.shape_id(s))


@pytest.mark.parametrize('lanes,E', [(1, 3), (3, 5), (64, 70), (0, 70)], ids=['1x3', '3x5', '64x70', '0x70'])
def test_lane_geometry(engine, lanes, E):
    """episode counts that are no multiple of the lanes per wavefront (70 at 64: the last wavefront flies 6 lanes and its other 58 sit every pass out),
    every lane a member of its own (the weights tensor has exactly E rows), then all lanes one member; hidden 72 x 3, 0.5 s"""
    w = np.ascontiguousarray(X.make_weights(S72, E, 11)) if E <= 5 else np.ascontiguousarray(np.tile(X.make_weights(S72, 5, 11), (14, 1))[:E])
    if E > 5:      # 70 rows from 5 actors: every row its own output bias, so that no two members fly the same episode
        P = X.spec_of(S72).param_count
        w[:, P - 3:P] += (0.01 * np.arange(E)[:, None] * np.array([1.0, -1.0, 0.5])).astype(np.float32)
    refs = _refs(E, 0.5, seed=7)
    own = _all_flavours(engine, w, S72, np.arange(E, dtype=np.int32)[::-1].copy(), refs, lanes, 'own members %d x %d' % (lanes, E), oracle=E <= 5, t_max=0.5)
    assert len(set(own['fitness'].tolist())) == E
    info = engine.plan_rollout(X.spec_of(S72), E, kernel='laneg', lanes_per_wave=lanes)
    assert info['family'] == 'laneg' and info['lanes'] == (lanes or 64) and info['workgroups'] * (info['block'] // 64) == -(-E // (lanes or 64))
    one = _all_flavours(engine, w[2:3].copy(), S72, np.zeros(E, np.int32), refs, lanes, 'one member %d x %d' % (lanes, E), oracle=E <= 5, t_max=0.5)
    assert one['fitness'].shape == (E,)


def _crashing_and_benign():
    """72 x 3, four members: 0 and 2 carry an output bias that saturates the command (tanh(6) = 1 in all three / alternating signs) -- the CPU oracle
    alone ends their episodes on the env's bounds at steps 132 and 145 of 201 (2 s); 1 and 3 are benign and fly the table out"""
    w = np.ascontiguousarray(X.make_weights(S72, 4, 7))
    P = X.spec_of(S72).param_count
    w[0, P - 3:P] = 6.0
    w[2, P - 3:P] = [6.0, -6.0, 6.0]
    return w


def test_lanes_of_one_wavefront_at_different_steps(engine):
    """one wavefront of six live lanes whose episodes end at different steps: finished lanes sit the later passes out beside lanes that fly on"""
    w = _crashing_and_benign()
    moe = np.array([0, 1, 2, 3, 0, 1], np.int32)
    refs = _refs(6, 2.0, seed=3)
    T = refs.shape[1]
    o = _oracle(w, X.net_of(S72), moe, refs, t_max=2.0, threads=6)
    assert (o['length_steps'][[0, 2, 4]] < T).all() and (o['length_steps'][[0, 2, 4]] > 20).all() and (o['length_steps'][[1, 3, 5]] == T).all(), \
        'the oracle alone must end the saturated episodes early: %s' % o['length_steps']
    for lanes in (64, 3):
        g = _all_flavours(engine, w, S72, moe, refs, lanes, 'crash beside benign, %d lanes' % lanes, t_max=2.0)
        assert (g['length_steps'] < T).any() and (g['length_steps'] == T).any()
        np.testing.assert_array_equal(g['length_steps'], o['length_steps'])


@pytest.mark.parametrize('build', ['h2000_v90', 'ice', 'cg_timed', 'gust', 'test'])
def test_every_code_variant(engine, build):
    """each of the five code variants at 72 x 3; the time-switched builds (cg_timed, gust) start 25 .. 1 ticks in front of their switch at tick 2 000"""
    from serl_amd import builds
    E = 5
    w = np.ascontiguousarray(X.make_weights(S72, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    tick0 = 1975 + 6 * np.arange(E, dtype=np.int32) if build in ('gust', 'cg_timed') else None
    g = _all_flavours(engine, w, S72, moe, _refs(E, 1.0), 4, build, build=build, tick0=tick0, t_max=1.0)
    assert engine.last_rollout_info()['family'] == 'lane'      # (the last of the three flavours)
    _fly(engine, 'laneg', w, S72, moe, _refs(E, 1.0), 4, build=build, tick0=tick0, t_max=1.0)
    ran(engine, 'laneg', code=builds.CODE_IDS[builds.load(build)[1]['code']])
    assert np.isfinite(g['states']).all()


def test_fault_rows_carried_error_clock_and_generated_references(engine):
    """fault rows be / jr, err0 and tick0 given, and the reference generated in the kernel from serl_ref_spec rows (tables everywhere else)"""
    from serl_amd import refsignals as rs, builds
    E = 5
    w = np.ascontiguousarray(X.make_weights(S72, 5, 33))
    moe = np.arange(E, dtype=np.int32)
    rng = np.random.default_rng(19)
    faults = [builds.MODES[m][1] for m in ('be', 'jr', 'nominal', 'jr', 'be')]
    err0 = 0.05 * rng.standard_normal((E, 3))
    tick0 = rng.integers(0, 50_000, E).astype(np.int32)
    g = _all_flavours(engine, w, S72, moe, _refs(E, 1.0, seed=9), 3, 'fault rows, err0, tick0', faults=faults, err0=err0, tick0=tick0, t_max=1.0)
    plain = _fly(engine, 'laneg', w, S72, moe, _refs(E, 1.0, seed=9), 3, t_max=1.0)
    assert (g['fitness'] != plain['fitness']).all(), 'the fault rows / the carried error moved nothing'
    assert (g['transitions'][:, 0, :3] == err0.astype(np.float32)).all()
    th, ph = rs.training_references(E, 6, np.random.RandomState(5))      # (the draws of a 6 s episode: steps of 1 s, the first second of them is flown)
    specs = rs.ref_specs(th, ph, [0.2106] * E)
    by_spec = _all_flavours(engine, w, S72, moe, specs, 3, 'ref_spec rows', t_max=1.0)
    assert len(set(by_spec['fitness'].tolist())) == E and (by_spec['fitness'] != plain['fitness']).all()
    _all_flavours(engine, w, S72, moe, specs[:1], 64, 'one shared ref_spec row', t_max=1.0)


ENV = np.array([7, 3, 3, 0, 1], np.int32)
EPISODE = np.array([0, 2, 2, 5, 0], np.int32)


@pytest.mark.parametrize('s', [S72, X._shape(20, 1, 'elu')], ids=X.shape_id)
def test_noise_twin(engine, s):
    """sensor_noise='device' and action_noise='device' with per-episode keys on the hint: bit for bit the existing lane noise kernel (same lanes_per_wave, no
    hint), and the table path of the hint fed serl_amd.venv_noise's rows (which the oracle flies too); family 14 in both"""
    import serl_amd
    E = 5
    w = np.ascontiguousarray(X.make_weights(s, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    refs = _refs(E, 0.5)
    T = refs.shape[1]
    err0 = (np.arange(E * 3).reshape(E, 3) % 7 - 3) * 2.0e-3
    nz = dict(sensor_noise='device', action_noise='device', noise_sd=SD, noise_clip=CLIP, noise_seed=SEED, noise_env=ENV, noise_episode=EPISODE)
    dev = _fly(engine, 'laneg', w, s, moe, refs, 4, t_max=0.5, err0=err0, **nz)
    _same(dev, _fly(engine, 'lane', w, s, moe, refs, 4, t_max=0.5, err0=err0, **nz), 'device noise against the lane noise kernel')
    sn = _np(serl_amd.venv_noise(SEED, ENV, EPISODE, T + 1, 'sensor', engine=engine))
    an = _np(serl_amd.venv_noise(SEED, ENV, EPISODE, T, 'action', noise_sd=SD, noise_clip=CLIP, engine=engine))
    assert sn.shape == (E, T + 1, 7) and an.shape == (E, T, 3) and (np.abs(an) == CLIP).any() and (np.abs(an) < CLIP).any()
    _same(dev, _fly(engine, 'laneg', w, s, moe, refs, 4, t_max=0.5, err0=err0, sensor_noise=sn, action_noise=an), 'device noise against the table path')
    o = _oracle(w, X.net_of(s), moe, refs, t_max=0.5, err0=err0, sensor_noise=sn, action_noise=an, traces=True, transitions=True, threads=E)
    _same_as_oracle(dev, o, 'device noise')
    quiet = _fly(engine, 'laneg', w, s, moe, refs, 4, t_max=0.5, err0=err0)
    assert (quiet['fitness'] != dev['fitness']).all() and (quiet['transitions'][:, 0, :7] != dev['transitions'][:, 0, :7]).any(-1).all()
    # one generator only, masks, and 64 lanes with the default keys (env = the episode's index, episode 0)
    mask = np.array([0, -1, 0, 0, -1], np.int32)
    for kw in (dict(sensor_noise='device', noise_seed=SEED, sensor_row=mask), dict(action_noise='device', noise_sd=SD, noise_clip=CLIP, noise_seed=SEED, noise_row=mask)):
        a = _fly(engine, 'laneg', w, s, moe, refs, 64, t_max=0.5, **kw)
        _same(a, _fly(engine, 'lane', w, s, moe, refs, 64, t_max=0.5, **kw), 'masked device noise %s' % sorted(kw))
        _same(a, _fly(engine, 'wave', w, s, moe, refs, 64, t_max=0.5, **kw), 'masked device noise against wave %s' % sorted(kw))


def test_lanes_at_different_steps_with_device_noise(engine):
    """the exploration-noise entry is the LANE's step: the crashing members beside the benign ones, noise drawn in the kernel"""
    w = _crashing_and_benign()
    moe = np.array([0, 1, 2, 3], np.int32)
    refs = _refs(4, 2.0, seed=3)
    nz = dict(sensor_noise='device', action_noise='device', noise_sd=0.05, noise_clip=0.1, noise_seed=SEED)
    dev = _fly(engine, 'laneg', w, S72, moe, refs, 64, t_max=2.0, **nz)
    _same(dev, _fly(engine, 'wave', w, S72, moe, refs, 64, t_max=2.0, **nz), 'device noise, lanes at different steps, against wave')
    T = refs.shape[1]
    assert (dev['length_steps'][[0, 2]] < T).all() and (dev['length_steps'][[1, 3]] == T).all(), dev['length_steps']


def test_refusals_on_the_device_path(engine):
    """what the hint does not take raises with the library's text before any launch: the launch record still shows the previous launch"""
    import serl_amd
    from serl_amd import builds
    w = np.ascontiguousarray(X.make_weights(S72, 2, 1))
    _fly(engine, 'laneg', w, S72, np.arange(2, dtype=np.int32), _refs(2, 0.5), 2, t_max=0.5)
    before = ran(engine, 'laneg', episodes_per_team=2, workgroups=1)
    cfg, incr = builds.env_config('PHlab_symmetric_nominal')
    sym = X._shape(8, 1, 'tanh', cfg, incr)
    ws = np.ascontiguousarray(X.make_weights(sym, 2, 2))
    calls = [(ws, sym, dict(env_config=cfg, incremental=incr), 'env_config'),
             (ws, sym, dict(env_config=cfg, incremental=incr, sensor_noise='device', noise_seed=1), 'env_config')]
    att_inc = X._shape(8, 1, 'tanh', X.ATTITUDE, True)
    calls.append((np.ascontiguousarray(X.make_weights(att_inc, 2, 3)), att_inc, dict(incremental=True), 'incremental'))
    for wt, s, kw, limit in calls:
        for lanes in (0, 2):
            with pytest.raises(RuntimeError, match=r'\(-3\).*LANEG.*%s' % limit):
                engine.rollout(torch.from_numpy(wt), X.spec_of(s), [0, 1], _refs(2, 0.5), t_max=0.5, kernel='laneg', lanes_per_wave=lanes, **kw)
            assert engine.last_rollout_info() == before
    for H, L, limit in ((132, 1, 'hidden'), (30, 1, 'hidden'), (8, 17, 'num_layers')):
        spec = serl_amd.NetSpec(7, 3, H, L, 'tanh')
        with pytest.raises(RuntimeError, match=r'\(-3\).*LANEG.*%s' % limit):
            engine.rollout(torch.zeros(2, (spec.param_count + 3) // 4 * 4), spec, [0, 1], _refs(2, 0.5), t_max=0.5, kernel='laneg')
        assert engine.last_rollout_info() == before


def test_evaluate_pop_with_the_hint(engine):
    """evaluate_pop(kernel='laneg'): the keyword reaches every launch of a mixed-fault sweep (one launch per build, never serl_rollout_multi); results
    equal the default call's; with sensor_noise='device' the noise twin runs"""
    import serl_amd
    w = X.make_weights(S72, 5, 77)
    kw = dict(spec=X.spec_of(S72), num_evals=3, refs=_refs(1, 1.0)[0], t_max=1.0, engine=engine)
    a = serl_amd.evaluate_pop(torch.from_numpy(w), **kw)
    assert engine.last_rollout_info()['family'] != 'laneg'
    b = serl_amd.evaluate_pop(torch.from_numpy(w), kernel='laneg', lanes_per_wave=4, **kw)
    ran(engine, 'laneg', episodes_per_team=4, workgroups=4)
    for key in ('fitness', 'returns', 'smoothness', 'length_steps', 'length_t', 'cost_steps', 'pop_fitness'):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=key)
    assert a.champion == b.champion and a.worst == b.worst
    modes = ['nominal', 'ice', 'be'] * 5
    before = engine.multi_launches
    c = serl_amd.evaluate_pop(torch.from_numpy(w), mode=modes, **kw)
    d = serl_amd.evaluate_pop(torch.from_numpy(w), mode=modes, kernel='laneg', fused=True, **kw)
    ran(engine, 'laneg', episodes_per_team=64)
    assert engine.multi_launches == before
    np.testing.assert_array_equal(c.fitness, d.fitness)
    np.testing.assert_array_equal(c.length_steps, d.length_steps)
    e = serl_amd.evaluate_pop(torch.from_numpy(w), mode='noise', sensor_noise='device', seed=5, lanes_per_wave=4, **kw)
    ran(engine, 'lane')
    f = serl_amd.evaluate_pop(torch.from_numpy(w), mode='noise', sensor_noise='device', seed=5, lanes_per_wave=4, kernel='laneg', **kw)
    ran(engine, 'laneg', episodes_per_team=4)
    np.testing.assert_array_equal(e.fitness, f.fitness)
    assert (e.fitness != a.fitness).any()

"""kernel='laneg' over a REGROUPED copy of the weights (lane_weights='regrouped': C ABI serl_rollout_regrouped, csrc/family_lanegt.hip and its device-noise
twin family_lanegtn.hip -- every live lane runs lane_actor.h serl_actor_forward_lane_general_t over [ceil(P / 4)][members up to 64][4]) at ZERO tolerance.

Every launch asserts through last_rollout_info() that family 14 ('laneg') ran AND through last_rollout_weights() that it read a regrouped copy of the
expected padded members and groups; everything rollout() returns -- fitness, length_steps, length_t, cost_steps, the action / state / reward traces, the
transition rows -- is held bit for bit to the same call with kernel='laneg' on the rows, to kernel='wave' and to the CPU oracle's same-libm flavour.
Flights are 0.5 .. 2 s; the helpers are tests/test_gpu_rollout_laneg.py's."""
import numpy as np
import pytest
import torch

import actor_shapes as X
from test_gpu_rollout import ran, _oracle
from test_gpu_rollout_laneg import KEYS, S72, SEED, SD, CLIP, ENV, EPISODE, _np, _refs, _fly, _same, _same_as_oracle, _crashing_and_benign

pytestmark = pytest.mark.gpu


def _copy_of(w, s):
    """what last_rollout_weights() must say after a regrouped launch over the rows of `w`"""
    P = X.spec_of(s).param_count
    mpad, groups = -(-w.shape[0] // 64) * 64, -(-P // 4)
    return dict(regrouped=1, padded_members=mpad, groups=groups, bytes=mpad * groups * 16)


def _fly_t(engine, w, s, moe, refs, lanes, **kw):
    """one launch of kernel='laneg', lane_weights='regrouped' -> numpy outputs; the family and the copy are asserted (not synchronised by rollout())"""
    out = engine.rollout(torch.from_numpy(w), X.spec_of(s), moe, refs, traces=True, transitions=True, sync=False, kernel='laneg', lanes_per_wave=lanes,
                         lane_weights='regrouped', **kw)
    per = lanes if lanes > 0 else 64
    info = ran(engine, 'laneg', episodes_per_team=per, work_queue=False, actor_wavefronts=0, actor_streamed=True, launches=1)
    assert engine.last_rollout_weights() == _copy_of(w, s)
    plan = engine.plan_rollout(X.spec_of(s), len(moe), kernel='laneg', lanes_per_wave=lanes, lane_weights='regrouped', n_members=w.shape[0])
    assert plan['regroup'] and info['workgroups'] == plan['workgroups'] and plan['workgroups'] * (plan['block'] // 64) >= -(-len(moe) // per)
    torch.cuda.synchronize()
    return {k: _np(out[k]) for k in KEYS}


def _all(engine, w, s, moe, refs, lanes, what, oracle=True, **kw):
    """the regrouped launch against kernel='laneg' on the rows, against kernel='wave' and (oracle=True) the CPU oracle -> the regrouped outputs"""
    g = _fly_t(engine, w, s, moe, refs, lanes, **kw)
    assert (g['length_steps'] != 0).all(), what + ': an episode was not written'
    _same(g, _fly(engine, 'laneg', w, s, moe, refs, lanes, **kw), what + ' against laneg on the rows')
    assert engine.last_rollout_weights() == dict(regrouped=0, padded_members=0, groups=0, bytes=0)      # (the rows: no copy)
    _same(g, _fly(engine, 'wave', w, s, moe, refs, lanes, **kw), what + ' against wave')
    if oracle:
        _same_as_oracle(g, _oracle(w, X.net_of(s), moe, refs, traces=True, transitions=True, threads=min(8, len(moe)), **kw), what)
    return g


# hidden 4: one group per row and the H - 4 clamp; 4 x 0: P = 47, the zero-padded last group, no hidden layer; 20: H % 16 != 0; SERL10; the TD3 actor
# shape; the largest hidden; the largest layer count; the general forward at the hidden-32 shape.  Each activation at least once.
SHAPES = [X._shape(4, 3), X._shape(4, 0, 'relu'), X._shape(20, 3, 'elu'), X._shape(72, 3), X._shape(96, 3, 'relu'), X._shape(128, 1), X._shape(8, 16, 'elu'),
          X._shape(32, 3)]


@pytest.mark.parametrize('s', SHAPES, ids=X.shape_id)
def test_shapes(engine, s):
    """5 episodes at 3 lanes per wavefront (two wavefronts, the second partly filled), every episode a member of its own in permuted order, 1 s"""
    i = SHAPES.index(s)
    assert {x['activation'] for x in SHAPES} == {'tanh', 'relu', 'elu'} and X.spec_of(X._shape(4, 0)).param_count == 47
    w = np.ascontiguousarray(X.make_weights(s, 5, 500 + i))
    moe = np.array([3, 0, 4, 1, 2], np.int32)
    refs = _refs(5, 1.0, seed=70 + i)
    g = _all(engine, w, s, moe, refs, 3, X.shape_id(s), t_max=1.0)
    assert (g['length_steps'] == refs.shape[1]).all()      # these actors fly the table out: every step of 1 s was compared
    assert len(set(g['fitness'].tolist())) == 5
    X.check_actions_f64(s, w, moe, g['transitions'], g['length_steps'], X.shape_id(s))


def _many_members(M, seed=11):
    """M rows of 72 x 3 from 5 actors, every row its own output bias: no two members fly the same episode"""
    w = np.ascontiguousarray(np.tile(X.make_weights(S72, 5, seed), (-(-M // 5), 1))[:M])
    P = X.spec_of(S72).param_count
    w[:, P - 3:P] += (0.01 * np.arange(M)[:, None] * np.array([1.0, -1.0, 0.5])).astype(np.float32)
    return w


@pytest.mark.parametrize('lanes,E', [(1, 3), (3, 5), (64, 70), (0, 70)], ids=['1x3', '3x5', '64x70', '0x70'])
def test_lane_geometry_and_padding(engine, lanes, E):
    """every lane a member of its own (E members: 3 / 5 padded to 64, 70 to 128), then all episodes one member (1 member padded to 64); 72 x 3, 0.5 s"""
    w = _many_members(E)
    refs = _refs(E, 0.5, seed=7)
    own = _all(engine, w, S72, np.arange(E, dtype=np.int32)[::-1].copy(), refs, lanes, 'own members %d x %d' % (lanes, E), oracle=E <= 5, t_max=0.5)
    assert len(set(own['fitness'].tolist())) == E
    assert engine.plan_rollout(X.spec_of(S72), E, kernel='laneg', lanes_per_wave=lanes, lane_weights='regrouped')['lanes'] == (lanes or 64)
    one = _all(engine, w[2:3].copy(), S72, np.zeros(E, np.int32), refs, lanes, 'one member %d x %d' % (lanes, E), oracle=E <= 5, t_max=0.5)
    assert one['fitness'].shape == (E,)


def test_second_block_of_members_and_a_partly_filled_last_wavefront(engine):
    """65 members (padded to 128: member 64 is the first of the second block of 64) on 70 episodes at 64 lanes: the last wavefront flies 6 lanes, among
    them member 64, and its other 58 lanes sit every pass out"""
    w = _many_members(65)
    moe = (np.arange(70, dtype=np.int32) * 7) % 65
    moe[66] = 64
    assert set(moe.tolist()) == set(range(65)) and 64 in moe[64:]
    g = _all(engine, w, S72, moe, _refs(70, 0.5, seed=8), 64, '65 members, 70 episodes', oracle=False, t_max=0.5)
    assert _copy_of(w, S72)['padded_members'] == 128
    first = {}
    for e, m in enumerate(moe):      # episodes of one member with different references differ; the five episodes that repeat a member are compared to nothing here
        first.setdefault(int(m), g['fitness'][e])
    assert len(set(first.values())) == 65


def test_row_stride_larger_than_the_parameter_count(engine):
    """a weights tensor of P + 12 columns (a multiple of 4; the columns beyond P hold NaN: nothing may read them)"""
    w = np.ascontiguousarray(X.make_weights(S72, 5, 13))
    P = X.spec_of(S72).param_count
    wide = np.full((5, w.shape[1] + 12), np.nan, np.float32)
    wide[:, :P] = w[:, :P]
    assert wide.shape[1] % 4 == 0 and wide.shape[1] > (P + 3) // 4 * 4
    moe = np.array([4, 2, 0, 1, 3], np.int32)
    refs = _refs(5, 0.5, seed=5)
    g = _fly_t(engine, wide, S72, moe, refs, 3, t_max=0.5)
    assert np.isfinite(g['fitness']).all()
    _same(g, _fly_t(engine, w, S72, moe, refs, 3, t_max=0.5), 'wide rows against packed rows')
    _same(g, _fly(engine, 'laneg', wide, S72, moe, refs, 3, t_max=0.5), 'wide rows against laneg on the rows')
    _same_as_oracle(g, _oracle(w, X.net_of(S72), moe, refs, traces=True, transitions=True, threads=5, t_max=0.5), 'wide rows')


@pytest.mark.parametrize('build', ['h2000_v90', 'ice', 'cg_timed', 'gust', 'test'])
def test_every_code_variant_with_lanes_at_different_steps(engine, build):
    """each of the five code variants at 72 x 3 with two crashing and two benign members: lanes leave at different steps and sit the later passes out
    beside lanes that fly on; the time-switched builds (cg_timed, gust) start 25 .. 1 ticks in front of their switch at tick 2 000"""
    from serl_amd import builds
    w = _crashing_and_benign()
    moe = np.array([0, 1, 2, 3, 0, 1], np.int32)
    refs = _refs(6, 2.0, seed=3)
    T = refs.shape[1]
    tick0 = 1975 + 5 * np.arange(6, dtype=np.int32) if build in ('gust', 'cg_timed') else None
    for lanes in (64, 4):
        g = _all(engine, w, S72, moe, refs, lanes, '%s, %d lanes' % (build, lanes), oracle=lanes == 64, build=build, tick0=tick0, t_max=2.0)
        assert (g['length_steps'][[0, 2, 4]] < T).all() and (g['length_steps'][[0, 2, 4]] > 20).all() and (g['length_steps'][[1, 3, 5]] == T).all(), g['length_steps']
    _fly_t(engine, w, S72, moe, refs, 4, build=build, tick0=tick0, t_max=2.0)
    ran(engine, 'laneg', code=builds.CODE_IDS[builds.load(build)[1]['code']])


@pytest.mark.parametrize('s', [S72, X._shape(20, 1, 'elu')], ids=X.shape_id)
def test_noise_twin(engine, s):
    """sensor_noise='device' and action_noise='device' with per-episode keys on the regrouped noise kernel: bit for bit the row laneg noise launch and the
    table path of the regrouped kernel fed serl_amd.venv_noise's rows (which the oracle flies too); then one generator at a time under masks with a
    negative entry"""
    import serl_amd
    E = 5
    w = np.ascontiguousarray(X.make_weights(s, 3, 21))
    moe = np.arange(E, dtype=np.int32) % 3
    refs = _refs(E, 0.5)
    T = refs.shape[1]
    err0 = (np.arange(E * 3).reshape(E, 3) % 7 - 3) * 2.0e-3
    nz = dict(sensor_noise='device', action_noise='device', noise_sd=SD, noise_clip=CLIP, noise_seed=SEED, noise_env=ENV, noise_episode=EPISODE)
    dev = _fly_t(engine, w, s, moe, refs, 4, t_max=0.5, err0=err0, **nz)
    _same(dev, _fly(engine, 'laneg', w, s, moe, refs, 4, t_max=0.5, err0=err0, **nz), 'device noise against the row laneg noise launch')
    sn = _np(serl_amd.venv_noise(SEED, ENV, EPISODE, T + 1, 'sensor', engine=engine))
    an = _np(serl_amd.venv_noise(SEED, ENV, EPISODE, T, 'action', noise_sd=SD, noise_clip=CLIP, engine=engine))
    assert sn.shape == (E, T + 1, 7) and an.shape == (E, T, 3) and (np.abs(an) == CLIP).any() and (np.abs(an) < CLIP).any()
    _same(dev, _fly_t(engine, w, s, moe, refs, 4, t_max=0.5, err0=err0, sensor_noise=sn, action_noise=an), 'device noise against the table path')
    o = _oracle(w, X.net_of(s), moe, refs, t_max=0.5, err0=err0, sensor_noise=sn, action_noise=an, traces=True, transitions=True, threads=E)
    _same_as_oracle(dev, o, 'device noise')
    quiet = _fly_t(engine, w, s, moe, refs, 4, t_max=0.5, err0=err0)
    assert (quiet['fitness'] != dev['fitness']).all() and (quiet['transitions'][:, 0, :7] != dev['transitions'][:, 0, :7]).any(-1).all()
    mask = np.array([0, -1, 0, 0, -1], np.int32)
    for kw in (dict(sensor_noise='device', noise_seed=SEED, sensor_row=mask), dict(action_noise='device', noise_sd=SD, noise_clip=CLIP, noise_seed=SEED, noise_row=mask)):
        a = _fly_t(engine, w, s, moe, refs, 64, t_max=0.5, **kw)
        _same(a, _fly(engine, 'laneg', w, s, moe, refs, 64, t_max=0.5, **kw), 'masked device noise %s' % sorted(kw))
        _same(a, _fly(engine, 'wave', w, s, moe, refs, 64, t_max=0.5, **kw), 'masked device noise against wave %s' % sorted(kw))
    # lanes at different steps: the exploration-noise entry is the LANE's step
    wc = _crashing_and_benign()
    refs = _refs(4, 2.0, seed=3)
    nzc = dict(sensor_noise='device', action_noise='device', noise_sd=0.05, noise_clip=0.1, noise_seed=SEED)
    if s is S72:
        c = _fly_t(engine, wc, S72, np.arange(4, dtype=np.int32), refs, 64, t_max=2.0, **nzc)
        _same(c, _fly(engine, 'wave', wc, S72, np.arange(4, dtype=np.int32), refs, 64, t_max=2.0, **nzc), 'device noise, lanes at different steps, against wave')
        assert (c['length_steps'][[0, 2]] < refs.shape[1]).all() and (c['length_steps'][[1, 3]] == refs.shape[1]).all(), c['length_steps']


def test_more_launches_in_flight_than_ring_slots(engine):
    """six regrouped launches with different weights on two streams, not synchronised in between -- more than the four slots of the ring: a slot is handed
    on only behind the launch that read it.  Each result equals its own row launch"""
    E = 5
    moe = np.array([1, 4, 0, 3, 2], np.int32)
    refs = _refs(E, 1.0, seed=17)
    spec = X.spec_of(S72)
    ws = [np.ascontiguousarray(X.make_weights(S72, 5, 900 + i)) for i in range(6)]
    streams = [torch.cuda.Stream(engine.device), torch.cuda.Stream(engine.device)]
    torch.cuda.synchronize()
    outs = []
    for i, w in enumerate(ws):
        with torch.cuda.stream(streams[i % 2]):
            outs.append(engine.rollout(torch.from_numpy(w).to(engine.device), spec, moe, refs, traces=True, transitions=True, sync=False, kernel='laneg',
                                       lanes_per_wave=3, lane_weights='regrouped', concurrent_episodes=E, t_max=1.0))
        ran(engine, 'laneg', episodes_per_team=3)
        assert engine.last_rollout_weights() == _copy_of(w, S72)
    torch.cuda.synchronize()
    got = [{k: _np(o[k]) for k in KEYS} for o in outs]
    assert len({g['fitness'].tobytes() for g in got}) == 6
    for i, w in enumerate(ws):
        _same(got[i], _fly(engine, 'laneg', w, S72, moe, refs, 3, t_max=1.0), 'launch %d of six' % i)


def test_the_record_of_the_weights_follows_every_launch(engine):
    """last_rollout_weights(): 1 after a hidden-32 lane launch that regrouped on its own, zeros after a launch that regrouped nothing"""
    s32 = X._shape(32, 3)
    w = np.ascontiguousarray(X.make_weights(s32, 3, 5))
    moe = np.array([2, 0, 1], np.int32)
    refs = _refs(3, 0.5)
    _fly(engine, 'lane', w, s32, moe, refs, 3, t_max=0.5)
    assert engine.plan_rollout(X.spec_of(s32), 3, lanes_per_wave=3, n_members=3)['regroup']
    assert engine.last_rollout_weights() == _copy_of(w, s32)
    _fly(engine, 'wave', w, s32, moe, refs, 3, t_max=0.5)
    assert engine.last_rollout_weights() == dict(regrouped=0, padded_members=0, groups=0, bytes=0)
    _fly_t(engine, w, s32, moe, refs, 3, t_max=0.5)
    _fly(engine, 'laneg', w, s32, moe, refs, 3, t_max=0.5)
    assert engine.last_rollout_weights()['regrouped'] == 0


def test_refusals_reach_python_and_launch_nothing(engine):
    """what the entry does not take raises with the library's text before any launch: the launch records still show the previous launch"""
    import serl_amd
    from serl_amd import builds
    w = np.ascontiguousarray(X.make_weights(S72, 2, 1))
    _fly_t(engine, w, S72, np.arange(2, dtype=np.int32), _refs(2, 0.5), 2, t_max=0.5)
    before, copy = ran(engine, 'laneg', episodes_per_team=2, workgroups=1), engine.last_rollout_weights()
    assert copy == _copy_of(w, S72)
    cfg, incr = builds.env_config('PHlab_symmetric_nominal')
    sym = X._shape(8, 1, 'tanh', cfg, incr)
    ws = np.ascontiguousarray(X.make_weights(sym, 2, 2))
    calls = [(ws, sym, dict(env_config=cfg, incremental=incr), 'env_config'),
             (ws, sym, dict(env_config=cfg, incremental=incr, sensor_noise='device', noise_seed=1), 'env_config')]
    att_inc = X._shape(8, 1, 'tanh', X.ATTITUDE, True)
    calls.append((np.ascontiguousarray(X.make_weights(att_inc, 2, 3)), att_inc, dict(incremental=True), 'incremental'))
    for wt, s, kw, limit in calls:
        for lanes in (0, 2):
            with pytest.raises(RuntimeError, match=r'serl_rollout_regrouped failed \(-3\).*LANEG.*%s' % limit):
                engine.rollout(torch.from_numpy(wt), X.spec_of(s), [0, 1], _refs(2, 0.5), t_max=0.5, kernel='laneg', lanes_per_wave=lanes, lane_weights='regrouped', **kw)
            assert engine.last_rollout_info() == before and engine.last_rollout_weights() == copy
    for H, L, limit in ((132, 1, 'hidden'), (30, 1, 'hidden'), (8, 17, 'num_layers')):
        spec = serl_amd.NetSpec(7, 3, H, L, 'tanh')
        with pytest.raises(RuntimeError, match=r'\(-3\).*LANEG.*%s' % limit):
            engine.rollout(torch.zeros(2, (spec.param_count + 3) // 4 * 4), spec, [0, 1], _refs(2, 0.5), t_max=0.5, kernel='laneg', lane_weights='regrouped')
        assert engine.last_rollout_info() == before and engine.last_rollout_weights() == copy
    # the keyword without the kernel never reaches the library
    for kernel in ('wave', None, 'laneq'):
        with pytest.raises(ValueError, match="needs kernel='laneg'"):
            engine.rollout(torch.from_numpy(w), X.spec_of(S72), [0, 1], _refs(2, 0.5), t_max=0.5, kernel=kernel, lane_weights='regrouped')
    with pytest.raises(ValueError, match='lane_weights'):
        engine.rollout(torch.from_numpy(w), X.spec_of(S72), [0, 1], _refs(2, 0.5), t_max=0.5, kernel='laneg', lane_weights='groups')
    assert engine.last_rollout_info() == before and engine.last_rollout_weights() == copy
    # the entry itself refuses a hint that is not LANEG (the binding is called directly: rollout() never gets this far)
    import ctypes
    out = engine.rollout(torch.from_numpy(w), X.spec_of(S72), [0, 1], _refs(2, 0.5), t_max=0.5, kernel='wave', launch=False)
    rc = engine.lib.serl_rollout_regrouped(engine.ctx, ctypes.byref(out['_desc']), None, None)
    assert rc == -3 and 'only the LANEG kernels read a regrouped copy through this entry' in engine.lib.serl_last_error().decode()
    assert engine.last_rollout_info() == before and engine.last_rollout_weights() == copy


def test_evaluate_pop_with_the_keyword(engine):
    """evaluate_pop(kernel='laneg', lane_weights='regrouped'): the keyword reaches every launch of a mixed-fault sweep; results equal the default call's"""
    import serl_amd
    w = X.make_weights(S72, 5, 77)
    kw = dict(spec=X.spec_of(S72), num_evals=3, refs=_refs(1, 1.0)[0], t_max=1.0, engine=engine)
    a = serl_amd.evaluate_pop(torch.from_numpy(w), **kw)
    b = serl_amd.evaluate_pop(torch.from_numpy(w), kernel='laneg', lanes_per_wave=4, lane_weights='regrouped', **kw)
    ran(engine, 'laneg', episodes_per_team=4, workgroups=4)
    assert engine.last_rollout_weights() == _copy_of(w, S72)
    for key in ('fitness', 'returns', 'smoothness', 'length_steps', 'length_t', 'cost_steps', 'pop_fitness'):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=key)
    modes = ['nominal', 'ice', 'be'] * 5
    c = serl_amd.evaluate_pop(torch.from_numpy(w), mode=modes, **kw)
    d = serl_amd.evaluate_pop(torch.from_numpy(w), mode=modes, kernel='laneg', lane_weights='regrouped', **kw)
    ran(engine, 'laneg', episodes_per_team=64)
    assert engine.last_rollout_weights()['regrouped'] == 1
    np.testing.assert_array_equal(c.fitness, d.fitness)
    np.testing.assert_array_equal(c.length_steps, d.length_steps)
    e = serl_amd.evaluate_pop(torch.from_numpy(w), mode='noise', sensor_noise='device', seed=5, kernel='laneg', lanes_per_wave=4, **kw)
    f = serl_amd.evaluate_pop(torch.from_numpy(w), mode='noise', sensor_noise='device', seed=5, kernel='laneg', lanes_per_wave=4, lane_weights='regrouped', **kw)
    assert engine.last_rollout_weights()['regrouped'] == 1
    np.testing.assert_array_equal(e.fitness, f.fitness)
    assert (e.fitness != a.fitness).any()
    with pytest.raises(ValueError, match="needs kernel='laneg'"):
        serl_amd.evaluate_pop(torch.from_numpy(w), lane_weights='regrouped', **kw)

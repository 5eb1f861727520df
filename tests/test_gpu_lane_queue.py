"""The lane-per-episode kernels behind a work queue (kernel_hint SERL_KERNEL_LANEQ, rollout_variant.inc serl_rollout_laneq_kernel_<variant>): a lane whose
episode ends takes the next one from a device counter, and flies initialize()'s step in the model evaluation in which its neighbours fly an env step.  Every
episode must come out exactly as on the one-episode-per-team kernel -- zero tolerance on every returned tensor -- whichever lane flew it and whatever that
lane flew before.  The engines are made with SERL_LANEQ_WAVES set, so that a handful of episodes engage the queue; every case also asserts WHAT was launched
(serl_last_rollout_info: family, work_queue, workgroups, lanes per wavefront)."""
import os
import numpy as np
import pytest
import torch
import actor_shapes as X
from test_gpu_rollout import kernel, ran, _oracle, _spec, NET32, _mixed_length_population

pytestmark = pytest.mark.gpu
RESULTS = ('fitness', 'length_steps', 'length_t', 'cost_steps')
_engines = {}


def _engine(waves):
    """a RolloutEngine whose LANEQ launches have at most `waves` wavefronts (read once, when the context is made)"""
    if waves not in _engines:
        import serl_amd
        old = os.environ.get('SERL_LANEQ_WAVES')
        os.environ['SERL_LANEQ_WAVES'] = str(waves)
        try:
            _engines[waves] = serl_amd.RolloutEngine(0)
        finally:
            if old is None:
                del os.environ['SERL_LANEQ_WAVES']
            else:
                os.environ['SERL_LANEQ_WAVES'] = old
    return _engines[waves]


def _team(eng, *a, **kw):
    """the comparison partner: one episode per team of eight wavefronts"""
    out = eng.rollout(*a, kernel='team', **kw)
    ran(eng, 'team', 'teams', 'teamr', episodes_per_team=1, work_queue=False)
    return out


def _same(a, b, what, keys=None):
    """every tensor of two rollouts equal; traces and transitions up to each episode's length (rows beyond it are never written)"""
    ls = np.abs(a['length_steps'].cpu().numpy())
    for key in (keys or [k for k in a if torch.is_tensor(a[k])]):
        x, y = a[key].cpu().numpy(), b[key].cpu().numpy()
        if key in RESULTS:
            np.testing.assert_array_equal(x, y, err_msg='%s: %s' % (what, key))
        else:
            for e in range(len(ls)):
                np.testing.assert_array_equal(x[e, :ls[e]], y[e, :ls[e]], err_msg='%s: %s of episode %d' % (what, key, e))


def _ref6():
    from serl_amd import refsignals
    return refsignals.tabulate(*refsignals.base_reference(20), 20)[:refsignals.n_steps_for(6)]


def test_queue_engaged_nominal(golden):
    """8 lane slots (2 wavefronts x 4 lanes), 37 episodes: 29 of them wait in the queue.  Traces and stored transitions included; 16 episodes against the
    same-libm CPU oracle."""
    eng = _engine(2)
    w, bad = _mixed_length_population(golden, 13)
    n = 37
    moe = ((np.arange(n) * 5) % 13).astype(np.int32)
    ref = _ref6()
    kw = dict(t_max=6, traces=True, transitions=True)
    a = _team(eng, torch.from_numpy(w), _spec(NET32), moe, ref, **kw)
    b = eng.rollout(torch.from_numpy(w), _spec(NET32), moe, ref, kernel='laneq', lanes_per_wave=4, **kw)
    ran(eng, 'lane', work_queue=True, workgroups=2, episodes_per_team=4)
    ls = a['length_steps'].cpu().numpy()
    assert (ls < ls.max() // 2).sum() >= 4 and (ls == ls.max()).sum() >= 4 and ls.max() == ref.shape[0], 'the batch should mix early crashes and full flights: %s' % ls
    _same(a, b, 'laneq against team')
    pick = np.arange(0, 32, 2)
    o = _oracle(w, NET32, moe[pick], ref, t_max=6, traces=True, transitions=True, threads=16)
    for key in RESULTS:
        np.testing.assert_array_equal(b[key].cpu().numpy()[pick], o[key], err_msg='oracle: ' + key)
    for key in ('actions', 'states', 'rewards', 'transitions'):
        x = b[key].cpu().numpy()
        for j, e in enumerate(pick):
            np.testing.assert_array_equal(x[e, :ls[e]], o[key][j, :ls[e]], err_msg='oracle: %s of episode %d' % (key, e))


def test_every_code_variant_rereads_its_per_episode_rows(golden):
    """15 lane slots (3 wavefronts x 5 lanes), 70 episodes on the four configurations of test_lane_kernels_of_every_code_variant: a refilled lane must pick up
    ITS episode's fault row, member, reference (table row, or a spec row evaluated in the kernel), sensor- and action-noise rows, model clock and carried error."""
    from serl_amd import refsignals as rs, builds
    eng = _engine(3)
    w, bad = _mixed_length_population(golden, 13)
    rng = np.random.default_rng(23)
    n = 70
    moe = rng.integers(0, 13, n).astype(np.int32)
    T = rs.n_steps_for(6)
    ref = rs.synthetic_reference_tables(n, 3, 20, seed=5)[:, :T]
    th, ph = rs.training_references(n, 6, np.random.RandomState(5))
    specs = rs.ref_specs(th, ph, [0.2106] * n)
    noise = np.clip(0.3 * rng.standard_normal((n, T, 3)), -0.5, 0.5)
    sn = np.stack([builds.sensor_noise_table(T, np.random.RandomState(40 + e)) for e in range(n)])
    tick0 = rng.integers(0, 50_000, n).astype(np.int32)
    err0 = 0.05 * rng.standard_normal((n, 3))
    for build, r, kw in (('gust', ref, dict(action_noise=noise, sensor_noise=sn, tick0=tick0, traces='actions')),
                         ('cg_timed', specs, dict(tick0=tick0, err0=err0, transitions=True)),
                         ('test', ref, dict(sensor_noise=sn, traces=True)),
                         ('ice', specs, dict(faults=[builds.MODES[m][1] for m in ('be', 'jr', 'sa', 'se', 'nominal')] * 14, transitions=True))):
        a = _team(eng, torch.from_numpy(w), _spec(NET32), moe, r, build=build, t_max=6, **kw)
        b = eng.rollout(torch.from_numpy(w), _spec(NET32), moe, r, build=build, t_max=6, kernel='laneq', lanes_per_wave=5, **kw)
        ran(eng, 'lane', work_queue=True, workgroups=3, episodes_per_team=5, code=builds.CODE_IDS[builds.load(build)[1]['code']])
        _same(a, b, build)
        ls = np.abs(a['length_steps'].cpu().numpy())
        assert (ls < ls.max()).any() and (ls > 0).all(), build + ': some episodes should end early'


def test_rank_and_counter_edges_with_full_wavefronts(golden):
    """One wavefront of 64 lanes, 130 episodes.  Equal lengths: all 64 lanes ask in the same pass (ranks 0 .. 63 on one atomicAdd), then two lanes fly the tail
    and 62 draw beyond the end.  The outputs start as zeros and every episode of the team kernel has length_steps != 0, so equality shows that every episode
    was written, and by the right lane.  Then mixed lengths: lanes ask one or a few at a time."""
    eng = _engine(1)
    from serl_amd import refsignals
    n = 130
    shipped = golden('actors')['serl50'][:50]
    moe = (np.arange(n) % 50).astype(np.int32)
    ref = refsignals.tabulate(*refsignals.base_reference(20), 20)[:refsignals.n_steps_for(2)]
    a = _team(eng, torch.from_numpy(shipped), _spec(NET32), moe, ref, t_max=2)
    b = eng.rollout(torch.from_numpy(shipped), _spec(NET32), moe, ref, t_max=2, kernel='laneq')
    ran(eng, 'lane', work_queue=True, workgroups=1, episodes_per_team=64)
    ls = a['length_steps'].cpu().numpy()
    assert (ls == 201).all(), 'equal lengths are what makes all lanes ask together: %s' % ls
    assert (b['length_steps'].cpu().numpy() != 0).all()
    _same(a, b, 'equal lengths')
    w, bad = _mixed_length_population(golden, 13)
    moe = ((np.arange(n) * 5) % 13).astype(np.int32)
    a = _team(eng, torch.from_numpy(w), _spec(NET32), moe, _ref6(), t_max=6)
    b = eng.rollout(torch.from_numpy(w), _spec(NET32), moe, _ref6(), t_max=6, kernel='laneq', lanes_per_wave=0)
    ran(eng, 'lane', work_queue=True, workgroups=1, episodes_per_team=64)
    assert (b['length_steps'].cpu().numpy() != 0).all()
    _same(a, b, 'mixed lengths')


@pytest.mark.parametrize('n,queue,workgroups', [(1, False, 1), (7, False, 2), (8, False, 2), (9, True, 2)])
def test_boundaries_of_the_queue(golden, n, queue, workgroups):
    """8 lane slots: fewer episodes than slots, a partly filled last wavefront, exactly the slots (no queue, nobody refills), one more (a queue of one)."""
    eng = _engine(2)
    w, bad = _mixed_length_population(golden, 13)
    moe = ((np.arange(n) * 5 + 3) % 13).astype(np.int32)
    kw = dict(t_max=6, traces='actions', transitions=True)
    a = _team(eng, torch.from_numpy(w), _spec(NET32), moe, _ref6(), **kw)
    b = eng.rollout(torch.from_numpy(w), _spec(NET32), moe, _ref6(), kernel='laneq', lanes_per_wave=4, **kw)
    ran(eng, 'lane', work_queue=queue, workgroups=workgroups, episodes_per_team=4)
    c = eng.rollout(torch.from_numpy(w), _spec(NET32), moe, _ref6(), lanes_per_wave=4, **kw)
    ran(eng, 'lane', work_queue=False, workgroups=(n + 3) // 4, episodes_per_team=4)
    _same(a, b, 'laneq against team, %d episodes' % n)
    _same(c, b, 'laneq against the lane family, %d episodes' % n)


@pytest.mark.parametrize('H,L', [(64, 3), (72, 3)])
def test_another_actor_shape(H, L):
    """Actors that are not the SERL50 shape fly the wave-cooperative forward pass, one lane's episode after the other, on per-lane weight pointers that change
    when a lane is refilled (and a fresh lane's pass is skipped).  8 slots, 20 episodes, 5 members."""
    eng = _engine(2)
    s = X._shape(H, L)
    w = X.make_weights(s, 5, seed=300 + H)
    n = 20
    moe = ((np.arange(n) * 3) % 5).astype(np.int32)
    ref = X.references(n, t_max=3)
    kw = dict(t_max=3, traces='actions', transitions=True)
    a = _team(eng, torch.from_numpy(w), X.spec_of(s), moe, ref, **kw)
    b = eng.rollout(torch.from_numpy(w), X.spec_of(s), moe, ref, kernel='laneq', lanes_per_wave=4, **kw)
    ran(eng, 'lane', work_queue=True, workgroups=2, episodes_per_team=4)
    _same(a, b, 'hidden %d' % H)
    o = _oracle(w, X.net_of(s), moe[:4], ref[:4], t_max=3, threads=4)
    for key in RESULTS:
        np.testing.assert_array_equal(b[key].cpu().numpy()[:4], o[key], err_msg='oracle: ' + key)


def test_two_launches_in_flight(golden):
    """Two queue launches with different weights on two streams, nobody waiting on the host: each has a counter of its own (the ring of queue counters) and a
    regrouped copy of its weights (the ring of copies), and each is told the other's episodes, so that it takes its share of the wavefronts."""
    eng = _engine(2)
    w, bad = _mixed_length_population(golden, 13)
    rng = np.random.default_rng(31)
    ws = [w, w + rng.normal(0, 0.02, w.shape).astype(np.float32)]
    n = 37
    moe = ((np.arange(n) * 5) % 13).astype(np.int32)
    ref = _ref6()
    alone = []
    for wi in ws:
        alone.append(eng.rollout(torch.from_numpy(wi), _spec(NET32), moe, ref, t_max=6, kernel='laneq', lanes_per_wave=4))
        ran(eng, 'lane', work_queue=True, workgroups=2, episodes_per_team=4)
    assert not torch.equal(alone[0]['fitness'], alone[1]['fitness'])
    streams = [eng.side_stream(0), eng.side_stream(1)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    flying = []
    for i, wi in enumerate(ws):
        with torch.cuda.stream(streams[i]):
            flying.append(eng.rollout(torch.from_numpy(wi), _spec(NET32), moe, ref, t_max=6, kernel='laneq', lanes_per_wave=4, sync=False, concurrent_episodes=n))
        ran(eng, 'lane', work_queue=True, workgroups=1, episodes_per_team=4)      # (half of the two wavefronts each)
    torch.cuda.synchronize()
    for i in range(2):
        _same(alone[i], flying[i], 'launch %d in flight' % i, RESULTS)
    _same(_team(eng, torch.from_numpy(ws[1]), _spec(NET32), moe, ref, t_max=6), flying[1], 'in flight against team', RESULTS)


def test_refusals(golden):
    """The lane kernels exist for the attitude task only: SERL_E_UNSUPPORTED (-3), nothing launched, the launch record untouched."""
    import serl_amd
    eng = _engine(2)
    w = golden('actors')['serl50'][:3]
    eng.rollout(torch.from_numpy(w), _spec(NET32), np.arange(3), _ref6(), t_max=6, kernel='laneq', lanes_per_wave=4)
    before = ran(eng, 'lane', work_queue=False, workgroups=1, episodes_per_team=4)
    s = X._shape(32, 1, cfg=X.FULL)
    wf = X.make_weights(s, 2, seed=9)
    for lanes in (0, 4):
        with pytest.raises(RuntimeError, match=r'serl_rollout failed \(-3\)'):
            eng.rollout(torch.from_numpy(wf), X.spec_of(s), np.arange(2), _ref6(), t_max=6, kernel='laneq', lanes_per_wave=lanes, env_config=X.FULL)
        assert eng.last_rollout_info() == before
    with pytest.raises(RuntimeError, match=r'serl_dyn_open_loop failed \(-3\)'):
        eng.dynamics_open_loop(np.zeros((2, 3, 10)), kernel='laneq')
    assert eng.last_rollout_info() == before


def test_evaluate_pop_with_the_lane_queue(golden):
    """evaluate_pop(kernel='laneq'): the keyword reaches every launch; population fitness and champion equal the default call's."""
    import serl_amd
    eng = _engine(2)
    w, bad = _mixed_length_population(golden, 13)
    kw = dict(spec=_spec(NET32), num_evals=3, refs=_ref6(), t_max=6, engine=eng)
    a = serl_amd.evaluate_pop(torch.from_numpy(w), **kw)
    ran(eng, 'team')
    b = serl_amd.evaluate_pop(torch.from_numpy(w), kernel='laneq', lanes_per_wave=4, **kw)
    ran(eng, 'lane', work_queue=True, workgroups=2, episodes_per_team=4)
    np.testing.assert_array_equal(a.pop_fitness, b.pop_fitness)
    assert a.champion == b.champion and a.worst == b.worst
    for key in ('fitness', 'returns', 'smoothness', 'length_steps', 'length_t', 'cost_steps'):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=key)
    # a mixed-fault sweep: one launch per build (never serl_rollout_multi), each a queue launch on its share of the wavefronts
    modes = (['nominal', 'ice', 'be'] * 13)
    before = eng.multi_launches
    c = serl_amd.evaluate_pop(torch.from_numpy(w), mode=modes, **kw)
    d = serl_amd.evaluate_pop(torch.from_numpy(w), mode=modes, kernel='laneq', lanes_per_wave=4, fused=True, **kw)
    ran(eng, 'lane', work_queue=True, episodes_per_team=4)
    assert eng.multi_launches == before
    np.testing.assert_array_equal(c.fitness, d.fitness)
    np.testing.assert_array_equal(c.length_steps, d.length_steps)

"""tests/test_gpu_venv_wave_edges.py leaves nothing out: its case lists against the batteries' own (no GPU: the module is imported, none of its tests run)."""
import env_glue as G
import test_gpu_env_glue as E
import test_gpu_ref_spec as P
import test_gpu_venv_noise_replay as Q
import test_gpu_venv_wave_edges as W


def _params(test, name):
    """the values of the parametrize mark of `test` whose argument names are `name`: what pytest will run, not the list the mark was made from"""
    marks = [m for m in test.pytestmark if m.name == 'parametrize' and m.args[0] == name]
    assert len(marks) == 1, (test.__name__, name)
    return list(marks[0].args[1])


def test_every_scenario_flies_on_the_wave_step_kernels_both_ways():
    cases = _params(W.test_wave_step_kernels_on_the_scenarios, 'key,auto')
    assert cases and len(set(cases)) == len(cases)
    for auto in (False, True):
        keys = [k for k, a in cases if a is auto]
        assert set(keys) == set(E.STEP) and all(E.STEP[k] for k in keys)      # every key, none of them empty
        names = [s['name'] for k in keys for s in E.STEP[k]]
        assert sorted(names) == sorted(s['name'] for s in G.scenarios()), 'auto=%s' % auto


def test_every_fused_scenario_flies_on_the_wave_rollout_kernel():
    cases = _params(W.test_wave_rollout_kernel_on_the_scenarios, 'key,shape')
    assert cases and len(set(cases)) == len(cases)
    keys = {k for k, _ in cases}
    assert keys == set(E.ROLL) and all(E.ROLL[k] for k in keys)
    names = {s['name'] for k in keys for s in E.ROLL[k]}
    assert names == {s['name'] for s in G.scenarios() if s['fused']} and names
    for k in keys:      # the attitude task: the 7-32x3-3 actor and the one-layer hidden-16 one; the other configurations: the latter
        shapes = sorted(s for kk, s in cases if kk == k)
        assert shapes == (['general', 'lane32'] if (k[1], k[2]) == (G.ATTITUDE, False) else ['general']), k


def test_every_build_and_configuration_is_present():
    pairs = {(s['config'], s['incremental']) for s in G.scenarios()}
    assert len(pairs) == 6
    step = [k for k, _ in _params(W.test_wave_step_kernels_on_the_scenarios, 'key,auto')]
    roll = [k for k, _ in _params(W.test_wave_rollout_kernel_on_the_scenarios, 'key,shape')]
    for keys in (step, roll):
        assert {k[0] for k in keys} == set(E.MODE_OF_BUILD)
        assert {(k[1], k[2]) for k in keys} == pairs
    assert {k[3] for k in step} == {False, True} == {k[3] for k in roll}      # the long flights (the dive among them) too
    assert any(s['name'] == 'dive' for k in step if k[3] for s in E.STEP[k])
    assert {k[-1] for k in step} == {'f32', 'f64'}


def test_the_clock_cases_cross_the_switch_on_both_timed_builds():
    assert _params(W.test_wave_auto_step_across_the_clock_switch, 'build') == ['cg_timed', 'gust']
    assert _params(W.test_wave_rollout_across_the_clock_switch, 'build') == ['cg_timed', 'gust']
    assert W.CLOCK_TICK0 == (1988, 1994, 1998, 1999, 2000) and (W.CLOCK_ROWS, W.CLOCK_STEPS) == (8, 20)


def test_the_clock_flights_pass_tick_2000_and_depend_on_it():
    """the yardstick of the clock cases, flown here (GlueEnv needs no GPU): _clock_flight asserts the crossings itself; the same env started far from the
    switch flies other states, so a kernel that dropped the clock on the way through its registers would show"""
    import numpy as np
    for build in W.CLOCK_BUILDS:
        o = W._clock_flight(build)
        assert np.isfinite(o['x']).all() and np.isfinite(o['reward']).all() and o['done'][7].all() and o['done'][15].all()
        refs, sn, const, wave = W._clock_inputs(build)
        e = 4
        early = G.GlueEnv(build, G.ATTITUDE, False, None, refs[e], None if sn is None else sn[e], W.CLOCK_T_MAX, tick0=0)
        early.reset()
        x = [early.step(const[e], noise=wave[k, e])['x'] for k in range(W.CLOCK_ROWS)]
        assert not np.array_equal(np.array(x), o['x'][:W.CLOCK_ROWS, e]), build


def test_the_generator_cases_cover_the_lane_grid():
    lane = P.test_env_step_returns_the_generated_reference
    want = {(kn, kind, mode, t) for kn, kind in _params(lane, 'kernel_,kind') for mode in _params(lane, 'mode') for t in _params(lane, 't_max')}
    assert len(want) == len(P.ENV_KINDS) * 2 * len(P.T_MAXES) == 20
    got = _params(W.test_env_step_returns_the_generated_reference, 'kernel_,kind,mode,t_max')
    assert set(got) == want and len(got) == len(want)
    lane = P.test_env_rollout_returns_the_generated_reference
    want = {(w, kind, mode, t) for w in _params(lane, 'which') for kind in _params(lane, 'kind') for mode in _params(lane, 'mode')
            for t in _params(lane, 't_max')}
    got = _params(W.test_env_rollout_returns_the_generated_reference, 'which,kind,mode,t_max')
    assert set(got) == want and len(got) == len(want) == 24
    tails = _params(W.test_entries_past_n_are_not_read_by_the_env_kernels, 'what')
    assert {'step', 'auto', 'pool'} < set(tails) and set(tails) & {'lane32', 'general'}


def test_the_replay_cases_cover_the_lane_modes():
    got = _params(W.test_wave_noise_replays_on_the_oracle, 'mode,hidden,layers,N,path')
    want = ([(m, 32, 3, 70, 'fused') for m in _params(Q.test_rollout_noise_replays_on_the_oracle, 'mode')]
            + [(m, 8, 1, 70, 'fused') for m in _params(Q.test_rollout_general_noise_replays_on_the_oracle, 'mode')]
            + [(m, 8, 1, 5, 'loop') for m in _params(Q.test_step_auto_noise_and_reset_noise_replay_on_the_oracle, 'mode')])
    assert sorted(got) == sorted(want) and len(want) == 18
    lane = Q.test_replay_across_the_clock_switch
    want = [(m, h, l, n, p) for m in _params(lane, 'mode') for h, l, n, p, _ in _params(lane, 'hidden,layers,N,path,ran')]
    assert sorted(_params(W.test_wave_replay_across_the_clock_switch, 'mode,hidden,layers,N,path')) == sorted(want) and len(want) == 6

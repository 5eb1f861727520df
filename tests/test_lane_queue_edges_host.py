"""tests/test_gpu_lane_queue_edges.py flies what it claims: its case lists against the glue battery's own, and the written order of its group of 26 against
the flights of the Python env (no GPU: the module is imported, none of its tests run)."""
import numpy as np

import env_glue as G
import test_gpu_env_glue as E
import test_gpu_ref_spec as P
import test_gpu_lane_queue_edges as Q


def _params(test, name):
    """the values of the parametrize mark of `test` whose argument names are `name`: what pytest will run, not the list the mark was made from"""
    marks = [m for m in test.pytestmark if m.name == 'parametrize' and m.args[0] == name]
    assert len(marks) == 1, (test.__name__, name)
    return list(marks[0].args[1])


def _attitude(s):
    return (s['config'], s['incremental']) == (G.ATTITUDE, False)


def test_the_glue_cases_are_the_attitude_groups_of_the_fused_battery():
    keys = _params(Q.test_glue_scenarios_one_after_the_other_on_one_lane, 'key')
    want = [k for k in E.FUSED if (k[1], k[2]) == (G.ATTITUDE, False)]
    assert sorted(keys) == sorted(want) and len(keys) == len(set(keys)) == 11
    assert sorted(len(E.FUSED[k]) for k in keys) == [1] * 9 + [2, 26] and len(E.FUSED[Q.BIG]) == 26


def test_every_attitude_scenario_flies_first_and_behind_a_refill():
    flown, later = set(), set()
    for key in _params(Q.test_glue_scenarios_one_after_the_other_on_one_lane, 'key'):
        scs = Q.plan(key)
        assert {(s['build'], s['config'], s['incremental'], s['t_max']) for s in scs} == {(key[0], key[1], key[2], key[4])}
        names = [s.get('of', s['name']) for s in scs]
        flown |= set(names)
        later |= set(names[1:])
        if key != Q.BIG:
            assert set(names[1:]) == set(names), key      # the doubled groups: every scenario also behind a refill
    want = {s['name'] for s in G.scenarios() if s['fused'] and _attitude(s)}
    assert flown == want and len(want) == 37
    assert later == want - {Q.ORDER[0]}      # each of them on a lane that has flown an episode (but the one that opens the group of 26)


def test_the_cold_copy_differs_from_spec_noise_carry_in_clock_and_error_only():
    key = [k for k in Q.GROUPS if [s['name'] for s in Q.GROUPS[k]] == ['spec_noise_carry']][0]
    a, b, c = Q.plan(key)
    assert a is c and a['tick0'] == 1990 and a['err0'] and (b['tick0'], b['err0']) == (0, None)
    assert {k for k in a if a[k] is not b.get(k)} == {'name', 'err0', 'tick0'} and b['of'] == a['name']
    fa, fb = G.flown(a['name']), G.fly(b)
    assert not np.array_equal(fa['obs0'], fb['obs0']) and not np.array_equal(fa['states'], fb['states'])      # the error; the gust on the clock


def test_the_written_order_is_the_group_and_holds_every_hand_over():
    names = [s['name'] for s in E.FUSED[Q.BIG]]
    assert sorted(Q.ORDER) == sorted(names) and len(set(Q.ORDER)) == 26
    assert set(Q.TAIL) <= set(names)
    flights = Q.big_flights()
    assert [s['name'] for s, _ in flights] == list(Q.ORDER + Q.TAIL)
    where = Q.order_conditions(flights)
    twins = [s['name'] for s in E.FUSED[Q.BIG] if 'twin' in s]
    assert len(twins) == 14 and all(n.endswith(('_on', '_above')) for n in twins) and not [n for n in names if n.endswith(('_on', '_above')) and n not in twins]
    assert len(where) == 8 + 1, sorted(where)      # eight adjacent pairs, and the weak ninth: no twin opens the order
    assert sorted(flights[i][0]['name'] for i in where['every threshold twin behind a refill']) == sorted(twins)
    assert all(where.values()), [w for w, at in where.items() if not at]
    # within the 26 alone: everything but the second approach to zero_table
    where = Q.order_conditions(Q.big_flights(Q.ORDER))
    assert [w for w, at in where.items() if not at] == ['ended by phi (the state too), then zero_table']
    # the conditions are read off the flights: the unpadded scenarios' own flights say the same where the table is the launch's
    T = max(len(s['ref']) for s in E.FUSED[Q.BIG])
    for s, o in Q.big_flights():
        src = [x for x in G.scenarios() if x['name'] == s['name']][0]
        if len(src['ref']) == T:
            assert o is G.flown(s['name'])
        if src['ends'] in ('theta', 'phi'):
            assert o['length_steps'] == G.flown(s['name'])['length_steps'] > 0 and o['terms'][-1][G.TERMS.index(src['ends'])], s['name']
    # a checker that cannot fail checks nothing: the group's own order lacks hand-overs
    plain = Q.order_conditions(Q.big_flights(tuple(names)))
    assert not all(plain.values())


def test_the_clock_cases_start_on_both_sides_of_the_switch_and_depend_on_it():
    assert _params(Q.test_the_clock_is_reread_at_every_refill, 'build') == ['cg_timed', 'gust']
    assert Q.CLOCK_TICK0 == (1990, 0, 1995, 0, 50000, 1990) and Q.CLOCK_T_MAX == 0.6 and Q.CLOCK_NO_ERR0 == ('cg_timed',)
    for build in Q.CLOCK_BUILDS:
        scs, flights = Q.clock_flights(build)
        assert [s['tick0'] for s in scs] == list(Q.CLOCK_TICK0) and {s['build'] for s in scs} == {build}
        assert [s['err0'] is not None for s in scs] == ([False] * 6 if build in Q.CLOCK_NO_ERR0 else [True, False] * 3)
        errs = [np.abs(o['err']).max() for _, o in flights]
        assert min(errs) > 0.0      # every episode leaves an error behind: a refilled lane that kept it would start on another observation
        assert all(o['n'] == 61 and o['length_steps'] == 61 for _, o in flights)      # the time-out ends them: 0 <= tick0 + 61 crosses 2000 from 1990 and 1995
        assert Q.clock_yardsticks_differ(build), build
        x = [o['states'] for _, o in flights]
        assert not np.array_equal(x[0], x[2]) and not np.array_equal(x[2], x[4])      # 1990, 1995 and 50000 fly three different episodes


def test_the_generator_case_runs_both_t_max():
    assert _params(Q.test_queue_lanes_fly_the_edge_specs_like_their_table, 't_max') == list(P.T_MAXES) and len(set(P.T_MAXES)) == 2
    assert _params(P.test_fused_families_fly_the_edge_specs_like_their_table, 't_max') == list(P.T_MAXES)
    assert 'laneq' not in P.FAMILIES      # (the queue kernel's turn is the new file's)

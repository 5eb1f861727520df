"""The lane kernels behind the work queue (kernel_hint SERL_KERNEL_LANEQ: rollout_variant.inc serl_wave_episodes_q_<v>) on the two edge batteries of the
other fused kernels, at ZERO tolerance against the literal Python env (tests/env_glue.py) and the same-libm oracle.

serl_wave_episodes_q_ holds a second hand-written copy of the env-step glue, and it alone sets an episode up INSIDE the loop, on a lane that has flown one:
the `take` block re-points the fault row, the weights, the member, the reference, the spec row and both noise rows, re-runs cit_reset on a used context,
re-reads the clock and the carried error, zeroes t, fitness, k and cost_steps, and then flies initialize()'s step with sensor-noise row 0.
tests/test_gpu_lane_queue.py compares it with the team kernel on random populations, where nothing decides which episode follows which on a lane.  Here that
is the test's choice: with SERL_LANEQ_WAVES=1 and lanes_per_wave=1 the launch has ONE lane slot, which flies episodes 0, 1, 2, ... in index order (the
sequential geometry, asserted on every such launch).

  a  the glue scenarios of the attitude task (every FUSED group of tests/test_gpu_env_glue.py the queue kernel accepts), sequential geometry: the group of
     26 once in the written ORDER, whose adjacent pairs are the hand-overs a refill can get wrong, plus TAIL; every other group as its list and the list
     reversed in one launch, so that every scenario flies as a lane's first episode and behind a refill; spec_noise_carry around a cold copy of itself;
  b  (NOT HERE: the group of 26 on six lane slots, 2 wavefronts x 3 lanes with twenty episodes queued, per-lane and wave-cooperative actor.  The kernel
     as it is passed it, but a scratch build with one planted slip -- the noise pointers not nulled at a refill -- ended that launch with an illegal
     memory access whose cause the code does not show: a stale pointer still addresses a whole row of the launch's own tables.  Until the cause is
     known the case stays out; the one-lane wave-cooperative pass is therefore not flown here either.)
  c  the model clock of cg_timed and gust across six refills that put it before, far before and far behind the switch at tick 2000;
  d  the edge grid of the reference generator (tests/ref_spec_edges.py) on four lane slots: every refill changes the lane's serl_ref_spec row.

tests/test_lane_queue_edges_host.py holds the case lists and ORDER to what they claim (no GPU)."""
import numpy as np
import pytest

import env_glue as G
import test_gpu_env_glue as E
import test_gpu_ref_spec as P
from test_gpu_lane_queue import _engine
from test_gpu_rollout import ran

pytestmark = pytest.mark.gpu

# the FUSED groups the queue kernel accepts: the attitude task without incremental control (the others: test_gpu_lane_queue.test_refusals)
GROUPS = {key: scs for key, scs in E.FUSED.items() if (key[1], key[2]) == (G.ATTITUDE, False)}
BIG = ('h2000_v90', G.ATTITUDE, False, False, 20.0)
# The group of 26, one lane, in this order.  What each hand-over is there for (tests/test_lane_queue_edges_host.py checks it on the flights):
ORDER = ('nose_down',                  # a lane's first episode: 392 steps to theta < -60 deg
         'zero_table',                 # a trimmed flight on a context last at -60 deg of pitch; a terminator's end in front of a table's
         'aileron_pos',                # a table's end in front of a terminator's (phi)
         'fault_jr', 'reward_clip',    # the jammed rudder must not stay: reward_clip has no fault
         'fault_gain_clip', 'noise_clips',      # nor the elevator's gain and clip
         'bias_actor',                 # noise_row = -1 behind an episode with an action-noise row
         'theta_pos_on', 'theta_pos_above',
         'aileron_neg',                # sensor_row = -1 behind an episode with a sensor-noise row (60 deg on theta at step 5 of it)
         'phi_pos_on', 'phi_pos_above', 'fault_be', 'phi_neg_on', 'phi_neg_above', 'fault_sa', 'alpha_cost_on', 'alpha_cost_above', 'fault_se',
         'alpha_cost_neg_on', 'alpha_cost_neg_above', 'phi_cost_on', 'phi_cost_above', 'phi_cost_neg_on', 'phi_cost_neg_above')
# ... and behind the 26, once more: the trimmed flight on a context last at 75 deg of roll (zero_table comes once in ORDER, behind theta)
TAIL = ('aileron_neg', 'zero_table')
SEQ = dict(kernel='laneq', lanes_per_wave=1)


def _sequential(eng):
    """one lane slot: the launch's episodes fly one after the other, in index order"""
    ran(eng, 'lane', work_queue=True, workgroups=1, episodes_per_team=1)


def _by_name(key, names):
    scs = {s['name']: s for s in GROUPS[key]}
    return [scs[n] for n in names]


def cold(sc):
    """`sc` with no carried error and the model clock at 0, under a name of its own: flown by env_glue.fly as it is"""
    return dict(sc, name=sc['name'] + '_cold', of=sc['name'], err0=None, tick0=0)


def plan(key):
    """the episodes of the sequential launch of group `key`, in flying order"""
    scs = GROUPS[key]
    if key == BIG:
        return _by_name(key, ORDER + TAIL)
    assert len(scs) <= 2, key
    if [s['name'] for s in scs] == ['spec_noise_carry']:      # the clock and the error re-read in both directions across the gust switch
        return [scs[0], cold(scs[0]), scs[0]]
    return scs + scs[::-1]


def adjacent(flights, first, second):
    """[i]: episode i satisfies `first` and episode i + 1 `second`; flights = [(scenario as flown, its flight by the Python env)]"""
    return [i for i in range(len(flights) - 1) if first(*flights[i]) and second(*flights[i + 1])]


def order_conditions(flights):
    """{what: the places in `flights` where it holds}: the adjacent pairs the order exists for, read off the scenarios AS FLOWN (padded to the launch's
    table) and their flights by the Python env, not off their names"""
    theta = lambda s, o: o['length_steps'] > 0 and o['terms'][-1][G.TERMS.index('theta')] and abs(o['states'][-1, 7]) > 0.9 * G.MAX_THETA
    phi = lambda s, o: o['length_steps'] > 0 and o['terms'][-1][G.TERMS.index('phi')] and abs(o['states'][-1, 6]) > 0.9 * G.MAX_PHI
    named = lambda n: (lambda s, o: s['name'] == n)
    no_fault = lambda s, o: s['fault'] is None
    out = {
        'sensor row, then none': adjacent(flights, lambda s, o: s['sensor_noise'] is not None and np.any(s['sensor_noise'][:o['n'] + 1]), lambda s, o: s['sensor_noise'] is None),
        'action-noise row, then bias_actor': adjacent(flights, lambda s, o: s['kind'] == 'noise' and np.any(s['noise'][:o['n']]), lambda s, o: s['name'] == 'bias_actor' and s['kind'] != 'noise'),
        'fault_jr, then no fault': adjacent(flights, lambda s, o: s['name'] == 'fault_jr' and G.fault_row(s['fault'])[3] != 0.0, no_fault),
        'fault_gain_clip, then no fault': adjacent(flights, lambda s, o: s['name'] == 'fault_gain_clip' and G.fault_row(s['fault'])[0] != 1.0 and np.isfinite(G.fault_row(s['fault'])[1]), no_fault),
        'ended by theta (the state too), then zero_table': adjacent(flights, theta, named('zero_table')),
        'ended by phi (the state too), then zero_table': adjacent(flights, phi, named('zero_table')),
        'table exhausted, then a terminator': adjacent(flights, lambda s, o: o['length_steps'] < 0, lambda s, o: o['length_steps'] > 0 and o['fin'][-1]),
        'a terminator, then table exhausted': adjacent(flights, lambda s, o: o['length_steps'] > 0 and o['fin'][-1], lambda s, o: o['length_steps'] < 0),
    }
    # (the weak one, as the issue words it: no threshold twin flies only as a lane's first episode -- true of any order that does not open with a twin)
    twins = [i for i, (s, o) in enumerate(flights) if 'twin' in s]
    out['every threshold twin behind a refill'] = twins if twins and min(twins) > 0 else []
    return out


def big_flights(names=ORDER + TAIL):
    T = max(len(s['ref']) for s in GROUPS[BIG])
    return [E._expected(s, T) for s in _by_name(BIG, names)]


# ---- a. the glue battery, one lane ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', list(GROUPS), ids=[E._id(k) for k in GROUPS])
def test_glue_scenarios_one_after_the_other_on_one_lane(key):
    build, cfg, incr, _, t_max = key
    scs = plan(key)
    T = max(len(s['ref']) for s in scs)
    flights = [E._expected(s, T) for s in scs]
    if key == BIG:
        bad = [what for what, at in order_conditions(flights).items() if not at]
        assert not bad, 'the written order lacks: %s' % bad
    out = E.fused_case(_engine(1), scs, build, cfg, incr, t_max, SEQ, _sequential, what='laneq, one lane')
    names = [s['name'] for s in scs]
    if names[0] == 'timeout_exact':      # t == t_max exactly at k = 5, as a first episode and behind the refill: `>` for `>=` flies on
        for e, (s, o) in enumerate(flights):
            assert o['n'] == 6 and o['t'][4] == s['t_max'] and o['terms'][-1].tolist() == [True, False, False, False]
            assert out['length_steps'][e] == 6 and out['length_t'][e] == o['t'][5]
    if names[0] == 'timeout_residue':    # the accumulated t passes t_max by a residue: the penalty -200 (t_max - t) != 0, the same twice
        (s, o), n = flights[0], flights[0][1]['n']
        residue = -1.0 / G.DT * (s['t_max'] - o['t'][n - 2]) * 2.0
        assert o['terms'][-1][0] and o['t'][n - 2] > s['t_max'] and residue > 0.0
        assert out['rewards'][0, n - 1] == out['rewards'][1, n - 1] == o['rewards'][-1] and out['length_steps'].tolist() == [n, n]
    if names[0] == 'spec_noise_carry':
        assert not np.array_equal(flights[0][1]['states'], flights[1][1]['states']) and not np.array_equal(flights[0][1]['obs0'], flights[1][1]['obs0'])


# ---- c. the model clock across refills ------------------------------------------------------------------------------------------------------------
CLOCK_BUILDS = ('cg_timed', 'gust')
CLOCK_TICK0 = (1990, 0, 1995, 0, 50000, 1990)      # the switch at tick 2000: ahead by 10 steps, far ahead, ahead by 5, far ahead, long past, ahead by 10
CLOCK_T_MAX = 0.6
CLOCK_NO_ERR0 = ('cg_timed',)
_CLOCK = {}


def clock_plan(build):
    """six episodes of spec_noise_carry (its commands, generated reference, sensor noise on all seven columns) on `build`, each started on its tick.  gust:
    the carried error of the scenario on the even episodes, none on the odd ones.  cg_timed: none on any, and the launch is given NO table of carried errors
    (CLOCK_NO_ERR0: the descriptor's err0 is null), so that a refilled lane must zero the error its last episode left"""
    base = [s for s in G.scenarios() if s['name'] == 'spec_noise_carry'][0]
    assert base['t_max'] == CLOCK_T_MAX and base['fused']
    made = {}
    for i, tick in enumerate(CLOCK_TICK0):
        carried = i % 2 == 0 and build not in CLOCK_NO_ERR0
        if (tick, carried) not in made:
            made[tick, carried] = dict(base, name='clock_%s_%d%s' % (build, tick, '_err' if carried else ''), of=base['name'], build=build, tick0=tick,
                                       err0=base['err0'] if carried else None)
    return [made[tick, i % 2 == 0 and build not in CLOCK_NO_ERR0] for i, tick in enumerate(CLOCK_TICK0)]


def clock_flights(build):
    """(the six scenarios, [(scenario, its flight by the Python env)]): made and flown once per build, shared, never changed"""
    if build not in _CLOCK:
        scs = clock_plan(build)
        _CLOCK[build] = scs, [E._expected(s, len(s['ref'])) for s in scs]
    return _CLOCK[build]


def clock_yardsticks_differ(build):
    """the flight started 10 ticks ahead of the switch and the one started at tick 0 differ in their states: the case says something about the clock"""
    scs, flights = clock_flights(build)
    near, far = flights[0][1], E._expected(dict(scs[0], name=scs[0]['name'] + '_tick0', tick0=0), len(scs[0]['ref']))[1]
    assert scs[0]['tick0'] == 1990 and near['n'] == far['n']
    return not np.array_equal(near['states'], far['states'])


@pytest.mark.parametrize('build', CLOCK_BUILDS)
def test_the_clock_is_reread_at_every_refill(build):
    assert clock_yardsticks_differ(build)
    scs, _ = clock_flights(build)
    kw = dict(SEQ, err0=None) if build in CLOCK_NO_ERR0 else SEQ
    assert all(s['err0'] is None for s in scs) == (build in CLOCK_NO_ERR0)
    E.fused_case(_engine(1), scs, build, G.ATTITUDE, False, CLOCK_T_MAX, kw, _sequential, what='laneq, one lane, clock')


# ---- d. the reference generator -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t_max', P.T_MAXES)
def test_queue_lanes_fly_the_edge_specs_like_their_table(golden, t_max):
    """the 70 episodes of test_gpu_ref_spec on four lane slots, 66 queued: generated == the tabulate_specs table == zero tails == the oracle on KEYS"""
    P.fused_ref_case(_engine(1), golden, None, t_max, dict(kernel='laneq', lanes_per_wave=4),
                     lambda eng: ran(eng, 'lane', work_queue=True, workgroups=1, episodes_per_team=4), what='laneq, four lanes')

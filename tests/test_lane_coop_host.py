"""tests/lane_coop.py held to what it claims, without a GPU: the case table against the planner, the oracle flown on the table's inputs, the
conditions tests/test_gpu_lane_coop.py relies on, and five planted slips the comparison must reject (the convention of tests/nov64.py: a slip is
applied to a copy of the oracle's inputs or outputs, never to the kernel)."""
import numpy as np
import pytest

import actor_shapes as X
import lane_coop as C


def _plan(case):
    from serl_amd import evaluator
    env = {'SERL_LANEQ_WAVES': str(C.QUEUE_WAVES)} if case['kernel'] == 'laneq' else None
    return evaluator.plan_rollout(X.spec_of(case['s']), case['E'], caps=evaluator.planner_caps(256, env), lanes_per_wave=case['lanes'],
                                  kernel='laneq' if case['kernel'] == 'laneq' else None, n_members=min(case['E'], 5), noise=case['kernel'] == 'lanern')


def test_the_case_table():
    ids = [c['id'] for c in C.CASES]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)
    for c in C.CASES:      # the planner takes every case to the lane family, whose actor is wave-cooperative wherever hidden is not 32
        p = _plan(c)
        assert p['family'] == 'lane' and p['lanes'] == c['lanes'] and not p['regroup'] and c['s']['hidden'] != 32, (c['id'], p)
        assert p['work_queue'] == (c['kernel'] == 'laneq' and c['E'] > c['lanes']), (c['id'], p)
    # section 1: all 32 patterns of either generator, the 8 combinations; the same masks on the table kernels
    for kernel in C.KERNELS:
        m = C.select('mask', kernel)
        assert {c['sensor'] for c in m if c['action'] is None} == {c['action'] for c in m if c['sensor'] is None} and \
            len({c['sensor'] for c in m if c['action'] is None}) == 32, kernel
        assert all(c['s'] == C.S72 and c['E'] == 5 and c['lanes'] == 64 and c['t_max'] == 0.5 for c in m)
    both = [(c['sensor'], c['action']) for c in C.select('mask', 'lanern') if c['sensor'] is not None and c['action'] is not None]
    assert len(set(both)) == 8 and {m for pair in both for m in pair} == {C.MASK, C.ON, C.OFF, C.COMPLEMENT}
    # section 2: the whole grid on every kernel
    for kernel in C.KERNELS:
        assert {(c['lanes'], c['E']) for c in C.select('occ', kernel)} == {(l, e) for l in C.LANES for e in C.EPISODES}
        assert {c['crash'] for c in C.select('ends', kernel)} == {'first', 'last'}
    # section 3: every hidden width at 3 layers with MASK at 64 lanes under the generator; pairwise coverage of the product
    assert {c['s']['hidden'] for c in C.CASES if c['kernel'] == 'lanern' and c['s']['num_layers'] == 3 and c['sensor'] == C.MASK and c['lanes'] == 64
            and c['s']['activation'] == 'tanh'} == set(C.HIDDEN)
    sh = [c['s'] for c in C.select('shape')]
    for a, b, na, nb in (('hidden', 'num_layers', 7, 3), ('hidden', 'activation', 7, 3), ('num_layers', 'activation', 3, 3)):
        assert len({(s[a], s[b]) for s in sh}) == na * nb, (a, b)
    assert all(c['t_max'] == 0.5 for c in C.CASES if c['section'] != 'ends')


def _flown(case):
    inp = C.inputs(case)
    if case['kernel'] == 'lanern':
        C.stand_in_rows(case, inp)
    return inp, C.oracle(case, inp)


@pytest.fixture(scope='module')
def masked():
    """hidden 72 x 3, MASK on the sensor rows of pre-drawn tables"""
    case = C.BY_ID['mask-lane-H72_L3_tanh-E5-l64-snxnnx']
    return (case,) + _flown(case)


@pytest.fixture(scope='module')
def ends():
    case = C.BY_ID['ends-lane-H72_L3_tanh-E6-l64-snxnnx+-first']
    return (case,) + _flown(case)


def test_the_oracle_flies_the_table():
    """one case per kernel, section and hidden width (the GPU file flies them all): every episode written, finite, 50 steps unless it is a
    crashing member's; no output equals a guard sentinel"""
    seen = set()
    for c in C.CASES:
        key = (c['section'], c['kernel'], c['s']['hidden'], c['E'] > 5)
        if key in seen:
            continue
        seen.add(key)
        inp, o = _flown(c)
        assert (o['length_steps'] > 0).all() and all(np.isfinite(o[k]).all() for k in C.KEYS), c['id']
        if c['section'] != 'ends':
            assert inp['T'] == 51 and (o['length_steps'] == inp['T']).all(), (c['id'], o['length_steps'])
        for k in C.KEYS:
            sent = {np.dtype(np.float64): C.SENT_F64, np.dtype(np.float32): C.SENT_F32, np.dtype(np.int32): C.SENT_I32}[o[k].dtype]
            assert not (o[k] == sent).any(), (c['id'], k)
    assert {k[:2] for k in seen} == {(sec, ker) for sec in ('mask', 'occ', 'ends', 'shape') for ker in C.KERNELS} and {k[2] for k in seen} == set(C.HIDDEN)


def test_masked_and_unmasked_episodes_differ(masked):
    """MASK moves exactly the episodes it leaves noisy: against the all-off and the all-on flights of the same inputs"""
    case, inp, o = masked
    noisy = np.asarray(case['sensor']) == 0
    off = C.oracle(case, dict(inp, sr=np.full(5, -1, np.int32)))
    on = C.oracle(case, dict(inp, sr=(4 - np.arange(5)).astype(np.int32)))
    assert ((o['fitness'] != off['fitness']) == noisy).all() and ((o['fitness'] != on['fitness']) == ~noisy).all()
    acase = C.BY_ID['mask-lane-H72_L3_tanh-E5-l64-anxnnx']
    ainp, ao = _flown(acase)
    aoff = C.oracle(acase, dict(ainp, nr=np.full(5, -1, np.int32)))
    assert ((ao['fitness'] != aoff['fitness']) == noisy).all()
    assert len(set(o['fitness'].tolist())) == 5


def test_episodes_end_at_different_steps(ends):
    """the crashing member at episode 0 ends first, long before the benign lanes above it; at the last episode it ends while lower lanes fly on"""
    case, inp, o = ends
    T = inp['T']
    assert T == 201 and 20 < o['length_steps'][0] < T - 20 and (o['length_steps'][1:] == T).all(), o['length_steps']
    last = C.BY_ID['ends-lane-H72_L3_tanh-E6-l64-snxnnx+-last']
    _, ol = _flown(last)
    assert 20 < ol['length_steps'][-1] < T - 20 and (ol['length_steps'][:-1] == T).all(), ol['length_steps']


def _rejected(got, want, what):
    with pytest.raises(AssertionError):
        C.same_as_oracle(got, want, what)


def test_planted_slips_are_rejected(masked, ends):
    case, inp, o = masked
    C.same_as_oracle(o, C.oracle(case, inp), 'the oracle against itself')
    # 1. the mask shifted by one lane
    _rejected(C.oracle(case, dict(inp, sr=np.roll(inp['sr'], 1))), o, 'mask shifted')
    # 2. a weight row read at row + 1: the first hidden layer's matrix of every member, rows shifted by one
    H, S, L = 72, 7, 3
    w = inp['w'].copy()
    at = H * S + H
    W = w[:, at:at + H * H].reshape(-1, H, H)
    W[:] = np.roll(W, -1, axis=1)
    _rejected(C.oracle(case, dict(inp, w=w)), o, 'weight row + 1')
    #    ... and of ONE member, only its LAST row (the clamped row id of a partly filled second register)
    w = inp['w'].copy()
    w[2, at + (H - 1) * H:at + H * H] = w[2, at + (H - 2) * H:at + (H - 1) * H]
    _rejected(C.oracle(case, dict(inp, w=w)), o, 'last weight row clamped one early')
    # 3. noise entry k instead of k + 1 behind step k
    sn = inp['sn'].copy()
    sn[:, 2:] = inp['sn'][:, 1:-1]
    _rejected(C.oracle(case, dict(inp, sn=sn)), o, 'sensor entry k')
    acase = C.BY_ID['mask-lane-H72_L3_tanh-E5-l64-anxnnx']
    ainp, ao = _flown(acase)
    an = ainp['an'].copy()
    an[:, 1:] = ainp['an'][:, :-1]
    _rejected(C.oracle(acase, dict(ainp, an=an)), ao, 'action entry k - 1')
    # 4. the action of lane l delivered to lane l + 1: the stored actions of the first env step alone
    got = {k: v.copy() for k, v in o.items()}
    got['transitions'][:, 0, 7:10] = np.roll(o['transitions'][:, 0, 7:10], 1, axis=0)
    _rejected(got, o, 'action of the neighbour')
    # 5. a stale action kept for a finished lane's neighbour: episode 1 flies on the action of the step at which episode 0 ended
    ecase, einp, eo = ends
    n0 = int(eo['length_steps'][0])
    got = {k: v.copy() for k, v in eo.items()}
    got['actions'][1, n0] = eo['actions'][1, n0 - 1]
    got['transitions'][1, n0, 7:10] = eo['transitions'][1, n0 - 1, 7:10]
    assert (got['actions'][1, n0] != eo['actions'][1, n0]).any()
    _rejected(got, eo, 'stale action')
    # ... and one wrong value in the last step an episode flew, in each output, is seen; one behind an episode's end is not the oracle's to judge
    for k in ('actions', 'states', 'rewards', 'transitions'):
        got = {kk: v.copy() for kk, v in eo.items()}
        got[k][0, n0 - 1] = np.nextafter(got[k][0, n0 - 1], np.inf)
        _rejected(got, eo, k)
        got = {kk: v.copy() for kk, v in eo.items()}
        got[k][0, n0:] = 1.0
        C.same_as_oracle(got, eo, k + ' behind the end')

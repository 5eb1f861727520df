"""tests/env_glue.py on the CPU: every scenario ends where it declares and on that term alone, the list as a whole reaches every
termination term, every reachable cost term, both sides of every reward clip and every fault field; the literal Python env equals the C
oracle (same-libm flavour) bit for bit on every scenario the oracle can be fed; and each planted mistake changes the outputs of at least
one scenario -- so a kernel copy making the same slip cannot pass tests/test_gpu_env_glue.py.  Episodes are flown once per process
(env_glue.flown)."""
import numpy as np
import pytest
import env_glue as G

NAMES = [s['name'] for s in G.scenarios()]
BY_NAME = {s['name']: s for s in G.scenarios()}


@pytest.mark.parametrize('name', NAMES)
def test_scenario_ends_on_its_declared_term_alone(name):
    sc, o = BY_NAME[name], G.flown(name)
    terms, n = o['terms'], o['n']
    assert not terms[:-1].any(), '%s: a termination term is true before the last step: %s' % (name, np.argwhere(terms[:-1])[:3])
    last = {t for t, v in zip(G.TERMS, terms[-1]) if v}
    if sc['ends'] == 'table':
        assert not last and o['length_steps'] == -len(sc['ref']) and not o['fin'].any()
    elif name == 'timeout_and_phi':      # the one scenario with two terms on one step
        assert last == {'time', 'phi'} and o['length_steps'] == n
    else:
        assert last == {sc['ends']} and o['length_steps'] == n
    assert o['fin'][-1] == (sc['ends'] != 'table') and not o['fin'][:-1].any()
    occurred = {c for i, c in enumerate(G.COSTS) if o['costs'][:, i].any()}
    assert occurred == set(sc['costs']), '%s: cost terms %s, declared %s' % (name, occurred, sc['costs'])
    assert o['cost_steps'] == int(o['costs'].any(axis=1).sum()) == int(o['cost'].sum())
    # the penalty is taken at the pre-increment t: -200 * (t_max - t_{n-1})
    if sc['ends'] != 'table':
        t_pre = 0.0
        for _ in range(n - 1):
            t_pre += G.DT
        r = float(o['rewards'][-1])
        A = sc['A']
        base = -sum(abs(min(max(v, -1.0), 1.0)) for v in o['scaled'][-1][:A]) / A
        assert r == base + -100.0 * (sc['t_max'] - t_pre) * 2.0
    assert np.isfinite(o['states']).all() and np.isfinite(o['rewards']).all()


def test_the_issue_s_table_of_crossings():
    """first indices on h2000_v90 under commands of exactly +-10 deg"""
    def first_cost(name, c):
        return int(np.argmax(G.flown(name)['costs'][:, G.COSTS.index(c)]))
    assert (first_cost('nose_up', 'alpha'), G.flown('nose_up')['n'] - 1) == (57, 709)
    assert G.flown('nose_down')['n'] - 1 == 391 and G.flown('nose_down')['states'][-1, 7] < -G.MAX_THETA
    for name in ('aileron_pos', 'aileron_neg', 'aileron_cg_timed', 'aileron_gust', 'aileron_test'):
        assert (first_cost(name, 'phi'), G.flown(name)['n'] - 1) == (10, 164), name
    assert (first_cost('rudder', 'phi'), G.flown('rudder')['n'] - 1) == (85, 1018)
    assert G.flown('dive')['n'] - 1 == 1868
    # executed commands of exactly +-10 deg
    assert (np.abs(G.flown('nose_up')['actions'][:, 0]) == 10.0 * G.D2R).all()


def test_exact_threshold_twins_differ_exactly_as_declared():
    seen = set()
    for name in NAMES:
        if not name.endswith('_on'):
            continue
        a, b = BY_NAME[name], BY_NAME[name[:-3] + '_above']
        term, is_cost, k, _ = a['twin']
        assert b['twin'] == (term, is_cost, k, True)
        oa, ob = G.flown(a['name']), G.flown(b['name'])
        col = {'theta': 7, 'phi': 6, 'alpha': 4}[term]
        va, vb = abs(oa['states'][k, col]), abs(ob['states'][k, col])
        assert vb == np.nextafter(va, np.inf), (name, va, vb)
        if is_cost:
            thr = {'alpha': G.ALPHA_COST, 'phi': G.PHI_COST}[term]
            assert G.R2D * va == thr and G.R2D * vb > thr
            i = G.COSTS.index(term)
            assert not oa['costs'][k, i] and ob['costs'][k, i] and oa['cost'][k] == 0 and ob['cost'][k] == 1
            assert oa['n'] == ob['n'] and oa['cost_steps'] + 1 == ob['cost_steps']
        else:
            thr = {'theta': G.MAX_THETA, 'phi': G.MAX_PHI}[term]
            assert va == thr
            i = G.TERMS.index(term)
            assert not oa['terms'][k, i] and ob['terms'][k, i]
            assert ob['n'] == k + 1 and oa['n'] == len(a['ref']) and oa['length_steps'] < 0 < ob['length_steps']
        # up to step k the twins are the same flight
        np.testing.assert_array_equal(oa['states'][:k], ob['states'][:k])
        seen.add((term, is_cost, bool(np.sign(oa['states'][k, col]) > 0)))
    assert seen == {(t, c, s) for t, c in (('theta', False), ('phi', False), ('alpha', True), ('phi', True)) for s in (True, False)}


def test_the_list_reaches_every_branch():
    ended = {BY_NAME[n]['ends'] for n in NAMES}
    assert ended == set(G.TERMS) | {'table'}
    # each term true at a last step in each configuration it is declared for
    for cfg in (G.ATTITUDE, G.SYMMETRIC, G.FULL):
        assert {'theta', 'time'} <= {s['ends'] for s in G.scenarios() if s['config'] == cfg}
    costs = set()
    for n in NAMES:
        costs |= {c for i, c in enumerate(G.COSTS) if G.flown(n)['costs'][:, i].any()}
    assert costs == {'alpha', 'phi'}      # `V < V0 / 3` is not reachable (env_glue: SPEED_SEARCH); covered on its false side only
    assert min(G.SPEED_SEARCH.values()) > 30.0
    for n in NAMES:
        assert (G.flown(n)['states'][:, 3] >= G.flown(n)['V0'] / 3.0).all()
    # both sides of the reward clip, per channel
    o, marks = G.flown('reward_clip'), BY_NAME['reward_clip']['marks']
    assert sorted((i, w) for _, i, w in marks) == sorted((i, w) for i in range(3) for w in (1.0, np.nextafter(1.0, np.inf), -1.0))
    for k, i, want in marks:
        assert o['scaled'][k, i] == want
    clipped = np.abs(np.concatenate([G.flown(n)['scaled'].ravel() for n in NAMES]))
    assert (clipped > 1.0).any() and (clipped < 1.0).any()
    # every fault field bites: the plant's command differs from the env's
    for f, col in (('be', 0), ('se', 0), ('gain_clip', 0), ('sa', 1), ('jr', 2)):
        o = G.flown('fault_' + f)
        assert (o['cmd'][:, col] != o['actions'][:, col]).any(), f
        other = [c for c in range(3) if c != col]
        np.testing.assert_array_equal(o['cmd'][:, other], o['actions'][:, other])
    o = G.flown('fault_se')
    clip = float(np.deg2rad(2.5))
    assert (o['cmd'][:, 0] == clip).any() and (o['cmd'][:, 0] == -clip).any() and (np.abs(o['cmd'][:, 0]) < clip).any()
    o = G.flown('fault_gain_clip')
    assert (np.abs(o['cmd'][:, 0]) == clip).any() and ((np.abs(o['cmd'][:, 0]) < clip) & (o['cmd'][:, 0] == 0.3 * o['actions'][:, 0])).any()
    # incremental control drives last_u past the deflection bound; actions of exactly +-1 and clipped sums
    assert np.abs(G.flown('incr_rates')['actions']).max() > 10.0 * G.D2R
    tr = G.flown('noise_clips')['transitions']
    assert (tr[:, 7:10] == 1.0).any() and (tr[:, 7:10] == -1.0).any() and (np.abs(tr[:, 7:10]) < 1.0).any()
    assert np.abs(G.flown('f64_beyond')['actions']).max() > 10.0 * G.D2R
    # time-outs: a penalty residue, none, and a crossing on the time-out's step
    assert G.flown('timeout_residue')['length_t'] > 0.6 and G.flown('timeout_residue')['n'] == 61
    assert G.flown('timeout_exact')['n'] == 6
    kinds = {s['kind'] for s in G.scenarios()}
    assert kinds == {'noise', 'f32', 'f64'}
    assert {(s['config'], s['incremental']) for s in G.scenarios()} == {(c, i) for c in (0, 1, 2) for i in (False, True)}


def oracle_of(sc, n):
    """the C oracle on scenario `sc`.  It refuses a table that ends before the episode does, so a `table` scenario is flown on its table
    padded to the time-out: the first n steps see the same inputs"""
    from oracle import rollout as R
    S, A = sc['S'], sc['A']
    net = dict(state_dim=S, action_dim=A, hidden=32, num_layers=3, activation='tanh')
    w = np.zeros((1, R.param_count(S, 32, 3, A)), np.float32)
    w[0, -A:] = sc['bias'][:A]
    T = len(sc['ref'])
    Tp = max(T, G.n_steps_for(sc['t_max'])) if sc['ends'] == 'table' else T

    def pad(a, rows):
        return np.concatenate([a, np.zeros((rows - len(a),) + a.shape[1:])]) if a is not None and rows > len(a) else a
    kw = {}
    if sc['kind'] == 'noise':
        kw['action_noise'] = pad(sc['noise'], Tp)[None]
    if sc['sensor_noise'] is not None:
        kw['sensor_noise'] = pad(sc['sensor_noise'], Tp + 1)[None]
    if sc['err0'] is not None:
        kw['err0'] = [sc['err0']]
    if sc['tick0'] is not None:
        kw['tick0'] = [sc['tick0']]
    return R.rollout(w, net, [0], pad(sc['ref'], Tp)[None], build=sc['build'], faults=[G.fault_row(sc['fault'])], t_max=sc['t_max'],
                     traces=True, transitions=True, env_config=sc['config'], incremental=sc['incremental'], short_libm=True, **kw)


@pytest.mark.parametrize('name', [s['name'] for s in G.scenarios() if s['fused']])
def test_python_env_equals_the_c_oracle_bit_for_bit(name):
    sc, o = BY_NAME[name], G.flown(name)
    n = o['n']
    c = oracle_of(sc, n)
    A = sc['A']
    np.testing.assert_array_equal(c['states'][0, :n], o['states'])
    np.testing.assert_array_equal(c['actions'][0, :n, :A], o['actions'][:, :A])
    np.testing.assert_array_equal(c['rewards'][0, :n], o['rewards'])
    np.testing.assert_array_equal(c['transitions'][0, :n], o['transitions'])
    if sc['ends'] != 'table':
        assert c['length_steps'][0] == o['length_steps'] == n
        assert c['fitness'][0] == o['fitness'] and c['length_t'][0] == o['length_t'] and c['cost_steps'][0] == o['cost_steps']
    else:
        assert c['length_steps'][0] > n


def test_generated_reference_of_the_spec_scenario_is_its_table():
    from serl_amd import refsignals as rs
    sc = BY_NAME['spec_noise_carry']
    np.testing.assert_array_equal(rs.tabulate_specs(sc['spec'], sc['t_max'])[0], sc['ref'])
    assert len(sc['ref']) == rs.n_steps_for(sc['t_max']) == G.n_steps_for(sc['t_max'])


# the scenarios that must notice each planted mistake (at least one of them)
DETECTORS = {
    'gt_time': ['timeout_exact'], 'ge_theta': ['theta_pos_on', 'theta_neg_full_on', 'theta_pos_sym_on'], 'ge_phi': ['phi_pos_on', 'phi_neg_on'],
    'ge_alpha_cost': ['alpha_cost_on', 'alpha_cost_neg_on'], 'ge_phi_cost': ['phi_cost_on', 'phi_cost_neg_on'],
    't_after': ['timeout_residue', 'timeout_exact', 'timeout_sym'], 'div3': ['timeout_sym', 'incr_sym'], 'noclip': ['reward_clip'],
    'penalty_sign': ['timeout_residue', 'aileron_pos'], 'gain_after_clip': ['fault_gain_clip'], 'nojam': ['fault_jr'],
    'noise_x3': ['spec_noise_carry', 'alpha_cost_above'], 'rate_nodt': ['timeout_sym_incr', 'incr_rates'], 'maxphi_deg': ['phi_cost_above', 'aileron_pos'],
    'no_last_u': ['timeout_full_incr', 'timeout_sym_incr'], 'scale_f64': ['bias_actor', 'f32_script'],
}
KEYS = ('states', 'actions', 'rewards', 'transitions', 'obs', 'cost', 'fin')


def _differs(a, b):
    if a['n'] != b['n'] or a['length_steps'] != b['length_steps'] or a['fitness'] != b['fitness'] or a['cost_steps'] != b['cost_steps']:
        return True
    return any(not np.array_equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize('bug', G.BUGS)
def test_planted_mistake_changes_a_scenario(bug):
    noticed = [n for n in DETECTORS[bug] if _differs(G.flown(n), G.fly(BY_NAME[n], bug))]
    print(bug, 'noticed by', noticed)
    assert noticed, '%s: none of %s changed' % (bug, DETECTORS[bug])
    if bug.startswith('ge_') or bug == 'gt_time':      # the exact-threshold scenarios: every one of them
        assert noticed == DETECTORS[bug]


def test_every_detector_is_flown_by_the_gpu_tests():
    """the three step-kernel-only scenarios aside, every detector runs in a fused kernel too"""
    assert set(DETECTORS) == set(G.BUGS)
    for bug, names in DETECTORS.items():
        assert any(BY_NAME[n]['fused'] for n in names), bug


@pytest.mark.parametrize('bug', G.BUGS_BLIND)
def test_blind_spots_are_what_the_module_says(bug):
    """`<=` for `<` on h and V: no scenario can notice (no sensor noise on x[9], x[3]); h is still crossed, from 50.2 to 49.7"""
    o = G.flown('dive')
    assert o['states'][-2, 9] > G.H_MIN > o['states'][-1, 9]
    assert not _differs(o, G.fly(BY_NAME['dive'], bug))

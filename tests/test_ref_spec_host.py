"""The reference generator's host side (no GPU): refsignals.tabulate_specs -- the float64 restatement every kernel is held to bit for bit
-- against the longdouble reference over the edge grid of tests/ref_spec_edges.py, the calibration of its tolerance, planted mistakes,
the CPU oracle's generator against its own table, and the contract refsignals.check_specs enforces."""
import os
import numpy as np
import pytest
import ref_spec_edges as X
from serl_amd import refsignals as rs

NET32 = dict(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation='tanh')
T_MAXES = [X.T_MAX, X.T_MAX_GATED]


@pytest.fixture(scope='module')
def tables():
    rows = X.specs()
    return rows, {tm: rs.tabulate_specs(rows, tm) for tm in T_MAXES}


def test_the_grid_is_what_it_says():
    rows = X.specs()
    t = rs.env_times(rs.n_steps_for(X.T_MAX_GATED))
    assert sorted({int(n) for n in rows['n_theta']} | {int(n) for n in rows['n_phi']}) == [0, 1, 2, 3, 4, 7, 8]
    by = dict(zip(X.NAMES, rows))
    assert (by['eight_none']['n_theta'], by['eight_none']['n_phi']) == (8, 0) and (by['none_eight']['n_theta'], by['none_eight']['n_phi']) == (0, 8)
    # a step ON an accumulated time that is not k * 0.01, and one ulp to either side of it
    tk = t[X.K_OFF]
    assert by['at_tk']['t_theta'][0] == tk != X.K_OFF * 0.01 and by['below_tk']['t_theta'][0] < tk < by['above_tk']['t_theta'][0]
    assert np.nextafter(by['below_tk']['t_theta'][0], 1.0) == tk == np.nextafter(by['above_tk']['t_theta'][0], -1.0)
    assert by['at_k_dt']['t_theta'][0] == 12 * 0.01 != t[12] and by['at_k_dt']['t_phi'][1] == 10 * 0.01 != t[10]
    # the blend argument lands on the branch points of det_cospi at a sample
    assert t[7] / by['s_14_12']['w_theta'] == 0.25 and t[9] / by['s_14_12']['w_phi'] == 0.5
    assert t[X._K34] / by['s_34_1']['w_theta'] == 0.75 and t[11] / by['s_34_1']['w_phi'] == 1.0
    assert (-0.05 - 0.0) / -by['before_0']['w_theta'] == 0.25                               # partly blended at t = 0
    assert by['w_1e-6']['w_theta'] == 1e-6 and by['w_1e300']['w_phi'] == 1e300 and by['w_short']['w_theta'] < 0.01
    assert by['cut_off']['w_theta'] > by['cut_off']['t_theta'][1] - by['cut_off']['t_theta'][0]
    assert by['after_end']['t_theta'][1] > t[-1] and by['after_end']['t_phi'][0] > t[-1]
    assert np.abs(by['big']['a_theta'][:4]).max() == 1e3 and np.signbit(by['zeros']['a_theta'][1]) and not by['zeros']['a_theta'][:3].any()
    assert len(set(rows['trim_deg'])) >= 4 and (rows['trim_deg'] < 0).any() and (rows['trim_deg'] == 0).any()
    # the unused tails are NaN, and the rows still pass the contract
    for nk, _, tk_, ak in X.CHANNELS:
        for r in rows:
            assert np.isnan(r[tk_][r[nk]:]).all() and np.isnan(r[ak][r[nk]:]).all() and np.isfinite(r[tk_][:r[nk]]).all()
    # the seven / eight step channels reach their last level inside the episode (the last sample of T_MAX is the accumulated
    # 0.6000000000000003 > 0.6: its trim is gated off already)
    tab = rs.tabulate_specs(rows, X.T_MAX)
    assert t[60] > X.T_MAX
    for name, amp in (('seven', 2.0), ('eight', -2.0)):
        assert tab[X.NAMES.index(name), -2, 0] == (amp + by[name]['trim_deg']) * (np.pi / 180.0)
        assert tab[X.NAMES.index(name), -1, 0] == amp * (np.pi / 180.0)


@pytest.mark.parametrize('t_max', T_MAXES)
def test_tabulate_specs_against_the_longdouble_reference(tables, t_max):
    """every case within TOL; TOL is 4 x the worst case measured here (the figures in tests/ref_spec_edges.py)"""
    rows, tab = tables
    t = rs.env_times(rs.n_steps_for(t_max))
    assert tab[t_max].shape == (len(X.EDGES), len(t), 3)
    errs = {c.name: X.check(tab[t_max][i], c, t, t_max, 'tabulate_specs') for i, c in enumerate(X.EDGES)}
    print(' '.join('%s %.3f' % kv for kv in errs.items()))
    worst = max(errs.values())
    assert 0.9 * X.TOL <= 4.0 * worst <= X.TOL, 'TOL = %.3g is not 4 x the measured worst case %.4g' % (X.TOL, worst)
    if t_max == X.T_MAX_GATED:      # the last sample lies beyond t_max: no trim there, and a trim on the sample before
        none = tab[t_max][X.NAMES.index('none')]
        assert t[-1] > t_max >= t[-2] and none[-1, 0] == 0.0 and none[-2, 0] == 0.22 * (np.pi / 180.0)


def test_planted_mistakes_exceed_the_tolerance(tables):
    """`>` for `>=`, prev not updated, the blend not clamped at 1: each is caught by several cases, by many orders of magnitude -- and the
    scalar generator they are planted in is tabulate_specs bit for bit without them"""
    rows, tab = tables
    for t_max in T_MAXES:
        t = rs.env_times(rs.n_steps_for(t_max))
        caught = {b: [] for b in X.BUGS}
        for i, c in enumerate(X.EDGES):
            np.testing.assert_array_equal(X.generator(rows[i], t, t_max), tab[t_max][i], err_msg=c.name)
            for b in X.BUGS:
                e = X.error_in_units(X.generator(rows[i], t, t_max, b), c, t, t_max)
                if not e <= X.TOL:
                    assert e > 1e6 * X.TOL, (b, c.name, e)
                    caught[b].append(c.name)
        print(caught)
        assert {'at_tk', 'tie3', 'cut_off'} <= set(caught['gt']) and 'below_tk' not in caught['gt'] and 'above_tk' not in caught['gt']
        assert len(caught['prev']) >= 15 and len(caught['clamp']) >= 15


@pytest.mark.parametrize('short_libm', [False, True], ids=['glibc', 'same-libm'])
@pytest.mark.parametrize('t_max', T_MAXES)
def test_oracle_generator_equals_its_table(tables, t_max, short_libm):
    """the oracle's generator inside the episode loop == tabulate_specs fed as a table, bit for bit, on the 70-episode batch of the GPU
    tests; NaN tails == zero tails; and the episodes are not trivially short"""
    from oracle import rollout as R
    rows, tab = tables
    w = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'actors.npz'))['serl50']
    idx = X.cycled()
    moe = np.arange(X.N_ENVS) % len(w)
    kw = dict(t_max=t_max, traces=True, short_libm=short_libm, threads=4)
    a = R.rollout(w, NET32, moe, rows[idx], **kw)
    b = R.rollout(w, NET32, moe, np.ascontiguousarray(tab[t_max][idx]), **kw)
    z = R.rollout(w, NET32, moe, X.specs(tail=0.0)[idx], **kw)
    assert (a['length_steps'] == rs.n_steps_for(t_max)).mean() >= 0.5
    for key in ('fitness', 'length_steps', 'length_t', 'cost_steps', 'actions', 'states', 'rewards'):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_array_equal(a[key], z[key], err_msg=key + ' (zero tails)')
    assert np.isfinite(a['fitness']).all() and len(set(a['fitness'])) > len(X.EDGES)


# ---- the contract -----------------------------------------------------------------------------------------------------------------------
def _row(**kv):
    r = rs.ref_specs([rs.SmoothedStepSequence([0.0, 0.1, 0.2], [1.0, 2.0, 3.0], 0.1)], [rs.SmoothedStepSequence([0.0], [1.0], 0.1)])
    for k, v in kv.items():
        if isinstance(v, tuple):
            r[k][0, v[0]] = v[1]
        else:
            r[k][0] = v
    return r


BAD_ROWS = [('n_theta', dict(n_theta=9)), ('n_phi', dict(n_phi=-1)), ('w_theta', dict(w_theta=0.0)), ('w_theta', dict(w_theta=-0.0)),
            ('w_phi', dict(w_phi=-1.0)), ('w_phi', dict(w_phi=np.inf)), ('w_theta', dict(w_theta=np.nan)),
            ('t_theta', dict(t_theta=(1, -0.1))), ('t_theta', dict(t_theta=(2, np.nextafter(0.1, 0.0)))), ('t_theta', dict(t_theta=(0, np.nan))),
            ('t_phi', dict(t_phi=(0, np.inf))), ('a_theta', dict(a_theta=(2, np.nan))), ('a_phi', dict(a_phi=(0, -np.inf))),
            ('trim_deg', dict(trim_deg=np.nan))]


@pytest.mark.parametrize('field,kv', BAD_ROWS, ids=['%s-%d' % (f, i) for i, (f, _) in enumerate(BAD_ROWS)])
def test_check_specs_refuses(field, kv):
    rs.check_specs(_row())
    with pytest.raises(ValueError, match=field):
        rs.check_specs(_row(**kv))
    # among good rows too, and naming the row
    rows = np.concatenate([_row(), _row(), _row(**kv)])
    with pytest.raises(ValueError, match=r'%s: row 2\b' % field):
        rs.check_specs(rows)
    with pytest.raises(ValueError, match=field):      # the env refuses hand-made rows before it touches a device
        import serl_amd
        serl_amd.CitationVecEnv(1, t_max=X.T_MAX, refs=_row(**kv))


def test_check_specs_accepts():
    rs.check_specs(_row(t_theta=(1, 0.0)))                                   # ties are legal
    rs.check_specs(_row(t_theta=(2, 0.1)))
    rs.check_specs(_row(n_theta=2, t_theta=(2, np.nan), a_theta=(2, np.nan)))      # entries past n are not read
    rs.check_specs(_row(n_theta=0, n_phi=0))
    rs.check_specs(_row(w_theta=5e-324, w_phi=1e300))
    assert rs.check_specs(X.specs()).shape == (len(X.EDGES),)
    with pytest.raises(ValueError, match='REF_SPEC_DTYPE'):
        rs.check_specs(np.zeros(2, dtype=[('n_theta', np.int32)]))
    rows = rs.ref_specs(*rs.training_references(5, 5, np.random.RandomState(2)), 0.2106)      # t_max < 6: width 1e-6
    assert (rows['w_theta'] == 1e-6).all()


def test_ref_specs_refuses_what_the_kernel_would_read_differently():
    """The two places where the literal SmoothedStepSequence and the kernels' generator part, pinned as documented behaviour: width 0
    (NaN at the sample on the step against the level) and decreasing step times (prev of the step listed before against prev of the step
    hit last: a whole level).  ref_specs refuses both with a message naming the field; ties stay legal."""
    S = rs.SmoothedStepSequence
    ok = S([0.0], [1.0], 0.1)
    t = rs.env_times(rs.n_steps_for(X.T_MAX))
    # width 0
    w0 = S([0.0, 0.2], [3.0, -2.0], 0.0)
    with np.errstate(all='ignore'):
        lit = w0(t)
    assert np.isnan(lit[0]) and lit[1] == 3.0
    row = _row(); row['n_theta'], row['w_theta'] = 2, 0.0; row['t_theta'][0, :2] = [0.0, 0.2]; row['a_theta'][0, :2] = [3.0, -2.0]; row['trim_deg'] = 0.0
    gen = X.generator(row[0], t, X.T_MAX)
    assert gen[0, 0] == 3.0 * (np.pi / 180.0) and np.isfinite(gen).all()
    with np.errstate(all='ignore'):
        np.testing.assert_array_equal(rs.tabulate_specs(row, X.T_MAX)[0], gen)      # tabulate_specs is the kernel's clamp, not np.minimum
    for w in (0.0, -0.0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match='w_theta'):
            rs.ref_specs([S([0.0, 0.2], [3.0, -2.0], w)], [ok])
        with pytest.raises(ValueError, match='w_phi'):
            rs.ref_specs([ok], [S([0.0, 0.2], [3.0, -2.0], w)])
    # decreasing times
    dec = S([0.3, 0.1, 0.2], [5.0, -4.0, 2.0], 0.2)
    row = _row(); row['w_theta'] = 0.2; row['t_theta'][0, :3] = dec.times; row['a_theta'][0, :3] = dec.amps; row['trim_deg'] = 0.0
    k = 15                                                # t = 0.15: the literal form blends from 5 (the step listed before), the kernel from 0
    lit, gen = np.deg2rad(dec(t)), X.generator(row[0], t, X.T_MAX)[:, 0]
    assert abs(t[k] - 0.15) < 1e-15 and abs(lit[k] - gen[k]) > np.deg2rad(4.0)
    with pytest.raises(ValueError, match='t_theta'):
        rs.ref_specs([dec], [ok])
    with pytest.raises(ValueError, match='t_phi'):
        rs.ref_specs([ok], [dec])
    with pytest.raises(ValueError, match='max 8'):
        rs.ref_specs([S(np.arange(9) * 0.1, np.ones(9), 0.1)], [ok])
    tie = rs.ref_specs([S([0.1, 0.1, 0.1], [1.0, 2.0, 3.0], 0.05)], [ok])
    np.testing.assert_allclose(rs.tabulate_specs(tie, X.T_MAX)[0], rs.tabulate(S([0.1, 0.1, 0.1], [1.0, 2.0, 3.0], 0.05), ok, X.T_MAX), rtol=0, atol=1e-16)

"""The in-kernel reference generator (serl_ref_spec: det_cospi / serl_ref_channel / serl_ref_generate of rollout_device.h) in every kernel it
is compiled into, on the edge grid of tests/ref_spec_edges.py.

The env kernels (serl_venv_step, serl_venv_step_auto, serl_venv_rollout, serl_venv_rollout_general) return the reference sample itself:
it must be the row of refsignals.tabulate_specs for the env's current spec and episode time BIT FOR BIT, and within TOL of the longdouble
reference -- through a restart, with per-env rows, one shared row and a pool of two rows per env, at t_max = 0.6 and 0.605, on the
nominal and a time-switched build.  The five fused rollout families do not return it: there the edge specs must fly exactly like their
table (fitness, lengths, actions, states), like the oracle and like each other.  Entries past n may hold NaN: no output moves.
70 envs / episodes (one full wavefront and a partial one), the cases cycled over them; every episode is 61 or 62 steps."""
import numpy as np
import pytest
import torch
import ref_spec_edges as X
from actor_shapes import make_weights, _shape, spec_of
from test_gpu_rollout import kernel, _oracle, _spec, NET32

pytestmark = pytest.mark.gpu
N = X.N_ENVS
T_MAXES = [X.T_MAX, X.T_MAX_GATED]
AFTER = 5                       # steps flown after the (last) restart
S72 = _shape(72, 3)


def _np(t):
    return t.cpu().numpy()


_TAB = {}


def _tab(t_max):
    """tabulate_specs of the grid, once per t_max: (rows with NaN tails, table [case, T, 3], env times)"""
    if t_max not in _TAB:
        from serl_amd import refsignals as rs
        rows = X.specs()
        _TAB[t_max] = rows, rs.tabulate_specs(rows, t_max), rs.env_times(rs.n_steps_for(t_max))
    return _TAB[t_max]


def _layout(kind):
    """case index of (env, episode) -> [N, episodes]: per-env rows (every episode the same), one shared row, or a pool of two rows"""
    if kind == 'shared':
        return np.full((N, 1), X.NAMES.index('eight'))
    if kind == 'pool':
        return np.stack([X.cycled(), X.cycled(shift=7)], axis=1)
    return X.cycled()[:, None]


def _make_env(engine, kind, auto, mode, t_max, tail=np.nan, kernel='lane'):
    import serl_amd
    rows = X.specs(tail=tail)
    lay = _layout(kind)
    if kind == 'pool':      # made to draw (refs=None); the reset is given rows, so it draws nothing, and the pool tensor is written after it
        env = serl_amd.CitationVecEnv(N, mode=mode, t_max=t_max, engine=engine, auto_reset=True, ref_pool=2, kernel=kernel)
        env.reset(refs=np.ascontiguousarray(rows[lay[:, 0]]))
        pool = np.ascontiguousarray(rows[lay]).view(np.uint8).reshape(N, 2, -1)
        assert env._pool.shape == pool.shape
        env._pool.copy_(torch.from_numpy(pool))
    else:
        given = rows[lay[:1, 0]] if kind == 'shared' else rows[lay[:, 0]]      # (one row: stride 0)
        env = serl_amd.CitationVecEnv(N, mode=mode, t_max=t_max, engine=engine, auto_reset=auto, refs=np.ascontiguousarray(given), kernel=kernel)
        assert env._spec_shared == (kind == 'shared')
        env.reset()
    from serl_amd import refsignals as rs
    assert env.max_steps == rs.n_steps_for(t_max) and env.last_step_kernel == kernel
    return env, lay


def _episodes(kind):
    return 2 if kind == 'pool' else 1      # restarts to fly before the last AFTER steps: the pool's cursor is back on row 0 after two


def _check_refs(ref, t, done, lay, t_max, what, full=0.5):
    """ref [K, N, 3], t [K, N], done [K, N] of K consecutive steps that began with fresh episodes: every sample is the tabulate_specs row of
    the env's current spec (lay[e, episode % R]) at its episode time bit for bit, the time the accumulated one, and every finished
    episode within TOL of the longdouble reference"""
    from serl_amd import refsignals as rs
    rows, tab, times = _tab(t_max)
    after = rs.env_times(len(times) + 1)[1:]      # info['t'] is the time after the step
    K = len(ref)
    k_e, epi = np.zeros(N, np.int64), np.zeros(N, np.int64)
    want, want_t = np.empty_like(ref), np.empty_like(t)
    ends = []
    for k in range(K):
        case = lay[np.arange(N), epi % lay.shape[1]]
        assert (k_e < len(times)).all(), '%s: an episode outlived its %d steps' % (what, len(times))
        want[k], want_t[k] = tab[case, k_e], after[k_e]
        for e in np.nonzero(done[k])[0]:
            ends.append((e, case[e], k - k_e[e], k + 1))
        k_e = np.where(done[k], 0, k_e + 1)
        epi = epi + done[k]
    np.testing.assert_array_equal(t, want_t, err_msg=what + ': env time')
    bad = np.nonzero((ref != want).any(axis=2))
    assert not len(bad[0]), '%s: %d samples differ from tabulate_specs, the first at step %d env %d (%s): %r against %r' % (
        what, len(bad[0]), bad[0][0], bad[1][0], X.NAMES[lay[bad[1][0], 0]], ref[bad[0][0], bad[1][0]], want[bad[0][0], bad[1][0]])
    assert len(ends) >= N * _n_restarts(lay, K, len(times)), '%s: only %d episodes ended' % (what, len(ends))
    lengths = np.array([b - a for _, _, a, b in ends])
    assert (lengths == len(times)).mean() >= full, '%s: episodes end early: %s' % (what, np.bincount(lengths))
    worst = 0.0
    for e, c, a, b in ends:
        worst = max(worst, X.check(ref[a:b, e], X.EDGES[c], times[:b - a], t_max, '%s env %d' % (what, e)))
    return worst, epi


def _n_restarts(lay, K, T):
    return (K - AFTER) // T


def _walk(env, kind, t_max, keys=('ref', 't'), kernel='lane'):
    """zero actions through one episode (the pool: two) plus the restart and AFTER steps of the next; the plain env is reset as documented;
    every step and reset must have run on the `kernel` family"""
    from serl_amd import refsignals as rs
    K = _episodes(kind) * rs.n_steps_for(t_max) + AFTER
    act = torch.zeros(N, 3, device=env.device)
    rec = {k: [] for k in keys + ('done', 'obs', 'reward')}
    for _ in range(K):
        obs, rew, done, info = env.step(act)
        for k in keys:
            rec[k].append(info[k].clone())
        rec['done'].append(done.clone()); rec['obs'].append(obs.clone()); rec['reward'].append(rew.clone())
        assert env.last_step_kernel == kernel
        if not env.auto_reset and bool(done.any()):
            env.reset(done)
            assert env.last_step_kernel == kernel
    return {k: np.stack([_np(v) for v in vs]) for k, vs in rec.items()}


ENV_KINDS = [('step', 'rows'), ('step', 'shared'), ('auto', 'rows'), ('auto', 'shared'), ('auto', 'pool')]


@pytest.mark.parametrize('t_max', T_MAXES)
@pytest.mark.parametrize('mode', ['nominal', 'gust'])
@pytest.mark.parametrize('kernel_,kind', ENV_KINDS, ids=['%s-%s' % k for k in ENV_KINDS])
def test_env_step_returns_the_generated_reference(engine, kernel_, kind, mode, t_max):
    """serl_venv_step / serl_venv_step_auto: info['ref'] of every step, through the restart (the pool: until its cursor is back on row 0)"""
    step_ref_case(engine, kernel_, kind, mode, t_max)


def step_ref_case(engine, kernel_, kind, mode, t_max, kernel='lane'):
    np.random.seed(5)      # (gust: the sensor-noise tables the resets draw)
    env, lay = _make_env(engine, kind, kernel_ == 'auto', mode, t_max, kernel=kernel)
    o = _walk(env, kind, t_max, kernel=kernel)
    worst, epi = _check_refs(o['ref'], o['t'], o['done'], lay, t_max, '%s %s %s %g' % (kernel_, kind, mode, t_max), full=1.0)
    print('worst %.3f units' % worst)
    assert np.isfinite(o['obs']).all() and np.isfinite(o['reward']).all()
    if kind == 'pool':
        assert (epi == 2).all() and (_np(env._cursor) == 0).all()          # row 0, row 1, and row 0 again for the last AFTER steps
        assert (lay[:, 0] != lay[:, 1]).all()


def _actor(engine, golden, which, kernel='lane'):
    """(weights, spec, members, the path rollout(path='fused') must report): on a wave env both shapes run the one wave rollout kernel"""
    if which == 'lane32':
        w = np.ascontiguousarray(golden('actors')['serl50'])
        return torch.from_numpy(w).to(engine.device), _spec(NET32), len(w), 'fused-wave' if kernel == 'wave' else 'fused'
    w = np.ascontiguousarray(make_weights(S72, 5, 31))
    return torch.from_numpy(w).to(engine.device), spec_of(S72), len(w), 'fused-wave' if kernel == 'wave' else 'fused-general'


def _rollout(engine, golden, which, kind, mode, t_max, tail=np.nan, kernel='lane'):
    from serl_amd import refsignals as rs
    env, lay = _make_env(engine, kind, True, mode, t_max, tail, kernel)
    w, spec, M, path = _actor(engine, golden, which, kernel)
    K = _episodes(kind) * rs.n_steps_for(t_max) + AFTER
    out = env.rollout(w, K, spec=spec, member_of_env=np.arange(N, dtype=np.int32) % M, transitions=True, path='fused')
    assert env.last_rollout_path == path
    return env, lay, {k: _np(v) for k, v in out.items()}


@pytest.mark.parametrize('t_max', T_MAXES)
@pytest.mark.parametrize('mode', ['nominal', 'gust'])
@pytest.mark.parametrize('kind', ['rows', 'shared', 'pool'])
@pytest.mark.parametrize('which', ['lane32', 'general'])
def test_env_rollout_returns_the_generated_reference(engine, golden, which, kind, mode, t_max):
    """serl_venv_rollout (the SERL50 shape: the lane-32 kernel) and serl_venv_rollout_general (hidden 72): 'ref' [K, N, 3] of one launch
    that flies an episode, restarts and flies on -- the actor in the loop, so the reference also feeds back into the flight"""
    rollout_ref_case(engine, golden, which, kind, mode, t_max)


def rollout_ref_case(engine, golden, which, kind, mode, t_max, kernel='lane'):
    np.random.seed(5)
    env, lay, o = _rollout(engine, golden, which, kind, mode, t_max, kernel=kernel)
    worst, epi = _check_refs(o['ref'], o['t'], o['done'], lay, t_max, '%s %s %s %g' % (which, kind, mode, t_max))
    print('worst %.3f units' % worst)
    assert np.isfinite(o['obs']).all() and np.isfinite(o['reward']).all()
    if kind == 'pool':
        assert (_np(env._cursor) == epi % 2).all()


@pytest.mark.parametrize('what', ['step', 'auto', 'pool', 'lane32', 'general'])
def test_entries_past_n_are_not_read_by_the_env_kernels(engine, golden, what):
    """NaN against zero in the unused tails of t_* / a_*: every output of every step bit for bit"""
    tails_case(engine, golden, what)


def tails_case(engine, golden, what, kernel='lane'):
    runs = []
    for tail in (np.nan, 0.0):
        if what in ('lane32', 'general'):
            _, _, o = _rollout(engine, golden, what, 'pool', 'nominal', X.T_MAX, tail, kernel)
        else:
            env, _ = _make_env(engine, 'pool' if what == 'pool' else 'rows', what != 'step', 'nominal', X.T_MAX, tail, kernel)
            o = _walk(env, 'pool' if what == 'pool' else 'rows', X.T_MAX, keys=('ref', 't', 'x', 'cost'), kernel=kernel)
        runs.append(o)
    assert set(runs[0]) == set(runs[1]) and np.isfinite(runs[0]['ref']).all()
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


# ---- the fused rollout families -------------------------------------------------------------------------------------------------------
FAMILIES = ['team', 'wave', 4, 'half', 'team2']
KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps', 'actions', 'states', 'rewards')
_ORACLE = {}


def _batch(golden, t_max):
    """the 70 episodes (SERL50 golden actors, the cases cycled) and their flight by the CPU oracle, once per t_max"""
    if t_max not in _ORACLE:
        from serl_amd import refsignals as rs
        w = np.ascontiguousarray(golden('actors')['serl50'])
        moe = np.arange(N) % len(w)
        idx = X.cycled()
        o = _oracle(w, NET32, moe, X.specs()[idx], t_max=t_max, traces=True, threads=8)
        assert (o['length_steps'] == rs.n_steps_for(t_max)).mean() >= 0.5, 'trivially short episodes: %s' % o['length_steps']
        _ORACLE[t_max] = w, moe, idx, o
    return _ORACLE[t_max]


@pytest.mark.parametrize('t_max', T_MAXES)
@pytest.mark.parametrize('kern', FAMILIES, ids=[str(k) for k in FAMILIES])
def test_fused_families_fly_the_edge_specs_like_their_table(engine, golden, kern, t_max):
    """team, wave, lane (4 per wavefront), two episodes per wavefront, two per team: generated == the tabulate_specs table == zero tails
    == the oracle, bit for bit (across families: through the oracle)"""
    fused_ref_case(engine, golden, kern, t_max)


def fused_ref_case(engine, golden, kern, t_max, launch_kw=None, check_ran=lambda eng: None, what=None):
    """the 70 episodes of _batch on `engine` under the hint `kern` (an int: that many lanes per wavefront; None: no hint); launch_kw: further keywords
    of every rollout (kernel=, lanes_per_wave=), check_ran(engine) behind each of the three launches; what: the label of the messages (default: kern)"""
    what = kern if what is None else what
    w, moe, idx, o = _batch(golden, t_max)
    rows, tab, _ = _tab(t_max)
    lanes = kern if isinstance(kern, int) else 0
    kw = dict(t_max=t_max, traces=True, lanes_per_wave=lanes)
    kw.update(launch_kw or {})
    wt = torch.from_numpy(w)
    with kernel(kern, engine):
        a = engine.rollout(wt, _spec(NET32), moe, rows[idx], **kw)
        check_ran(engine)
        b = engine.rollout(wt, _spec(NET32), moe, np.ascontiguousarray(tab[idx]), **kw)
        check_ran(engine)
        z = engine.rollout(wt, _spec(NET32), moe, X.specs(tail=0.0)[idx], **kw)
        check_ran(engine)
    for key in KEYS:
        got = _np(a[key])
        np.testing.assert_array_equal(got, _np(b[key]), err_msg='%s: %s, generated against its table' % (what, key))
        np.testing.assert_array_equal(got, _np(z[key]), err_msg='%s: %s, NaN against zero tails' % (what, key))
        np.testing.assert_array_equal(got, o[key], err_msg='%s: %s against the oracle' % (what, key))
    assert np.isfinite(_np(a['fitness'])).all()


def test_hand_made_rows_are_refused_before_any_device_work(engine, golden):
    """check_specs at the host entry points: the evaluator, the env's constructor and reset(refs=...)"""
    import serl_amd
    rows = X.specs()[X.cycled()]
    bad_w, bad_t = rows.copy(), rows.copy()
    bad_w['w_phi'][3] = 0.0
    i = X.NAMES.index('seven')
    bad_t['t_theta'][i, 2] = bad_t['t_theta'][i, 1] - 1e-9
    w = golden('actors')['serl50'][:1]
    engine.rollout(torch.from_numpy(w), _spec(NET32), np.zeros(N, np.int32), rows, t_max=X.T_MAX)
    before = engine.last_rollout_info()
    env = serl_amd.CitationVecEnv(N, t_max=X.T_MAX, engine=engine, refs=rows)
    env.reset()
    state = env._state.clone(), env._spec.clone()
    for bad, field in ((bad_w, 'w_phi'), (bad_t, 't_theta')):
        with pytest.raises(ValueError, match=field):
            engine.rollout(torch.from_numpy(w), _spec(NET32), np.zeros(N, np.int32), bad, t_max=X.T_MAX)
        with pytest.raises(ValueError, match=field):
            serl_amd.CitationVecEnv(N, t_max=X.T_MAX, engine=engine, refs=bad)
        with pytest.raises(ValueError, match=field):
            env.reset(refs=bad)
    assert engine.last_rollout_info() == before
    assert torch.equal(env._state, state[0]) and torch.equal(env._spec, state[1])

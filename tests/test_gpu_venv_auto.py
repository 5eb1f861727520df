"""Auto-reset inside the step of the vector env (C ABI serl_venv_step_auto, CitationVecEnv(auto_reset=True)) on the GPU.

The yardstick is the existing API, which tests/test_gpu_venv.py pins to the oracle: a `manual` env (auto_reset=False) runs the
documented loop -- `step`, then `reset(done)` -- beside an `auto` env on the same actions, and every output of every step must be
equal bit for bit (assert_array_equal: there is no tolerance).  Episodes are a handful of steps (t_max = 0.05 s) so that every env
restarts several times within a few dozen launches.

The pool test cannot use t_max = 0.05: refsignals.training_references has no sequence shorter than t_max // 5 = 1 s per level
(at 0.05 s it produces 50 001 levels, which serl_ref_spec refuses), for the existing env as well.  It uses t_max = 5, the shortest
episode for which the draw exists."""
import ctypes
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T_SHORT = 0.05
STEP_KEYS = ('reward', 'done', 'x', 'ref', 't', 'cost')


def _venv(n, mode, t_max, engine, **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(n, mode=mode, t_max=t_max, engine=engine, **kw)


def _tables(N, t_max, seed, A=3):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rs.n_steps_for(t_max)])
    if A == 1:
        r[:, :, 1:] = 0.0
    assert np.isfinite(r).all()
    return r


def _actions(steps, N, A, seed, dtype=torch.float32):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return ((torch.rand(steps, N, A, generator=g, dtype=torch.float64) * 2 - 1) * 0.6).to(dtype)


class Pair:
    """A manual and an auto env side by side; every step is recorded on the device (no synchronisation in the loop unless
    `next_refs` needs the finished envs) and compared afterwards."""

    def __init__(self, manual, auto):
        assert not manual.auto_reset and auto.auto_reset and manual.n_envs == auto.n_envs
        self.m, self.a, self.rec = manual, auto, []
        dev, N = auto.device, auto.n_envs
        self.acc = torch.zeros(N, dtype=torch.float64, device=dev)       # device accumulator ret = ret + reward of the running episodes
        self.cnt = torch.zeros(N, dtype=torch.int32, device=dev)

    def reset(self, mask=None, **kw):
        om, oa = self.m.reset(mask, **kw), self.a.reset(mask, **kw)
        np.testing.assert_array_equal(oa.cpu().numpy(), om.cpu().numpy(), err_msg='explicit reset')
        if mask is None:
            self.acc.zero_(); self.cnt.zero_()
        else:
            self.acc.masked_fill_(mask, 0); self.cnt.masked_fill_(mask, 0)

    def step(self, act, next_refs=None):
        obs_a, rew_a, done_a, info_a = self.a.step(act)
        r = {'a_obs': obs_a.clone(), 'a_reward': rew_a.clone(), 'a_done': done_a.clone()}
        for k in ('x', 'ref', 't', 'cost', 'final_obs', 'episode_return', 'episode_length'):
            r['a_' + k] = info_a[k].clone()
        obs_m, rew_m, done_m, info_m = self.m.step(act)
        r.update(m_obs=obs_m.clone(), m_reward=rew_m.clone(), m_done=done_m.clone())
        for k in ('x', 'ref', 't', 'cost'):
            r['m_' + k] = info_m[k].clone()
        self.acc = self.acc + rew_m
        self.cnt = self.cnt + 1
        r['acc'], r['cnt'] = self.acc.clone(), self.cnt.clone()
        done = r['m_done']
        self.acc = torch.where(done, torch.zeros_like(self.acc), self.acc)
        self.cnt = torch.where(done, torch.zeros_like(self.cnt), self.cnt)
        kw = {}
        if next_refs is not None:
            rows = next_refs(done.cpu().numpy())
            if rows is not None:
                kw['refs'] = rows
        r['m_reset_obs'] = self.m.reset(done, **kw).clone()          # the documented loop: only the finished envs
        self.rec.append(r)

    def arrays(self):
        return {k: np.stack([r[k].cpu().numpy() for r in self.rec]) for k in self.rec[0]}


def _compare(o):
    """auto against manual, every step: the outputs of the terminal step, the terminal observation, the restarted observation"""
    for k in STEP_KEYS:
        np.testing.assert_array_equal(o['a_' + k], o['m_' + k], err_msg=k)
    np.testing.assert_array_equal(o['a_final_obs'], o['m_obs'], err_msg='final_obs against the manual step obs')
    np.testing.assert_array_equal(o['a_obs'], o['m_reset_obs'], err_msg='obs against the manual reset(done)')


def _compare_statistics(o):
    done = o['m_done']
    np.testing.assert_array_equal(o['a_episode_return'][done], o['acc'][done])
    np.testing.assert_array_equal(o['a_episode_length'][done], o['cnt'][done])
    assert (o['cnt'][done] > 0).all()
    # where not done: unchanged from the previous step
    keep = ~done[1:]
    np.testing.assert_array_equal(o['a_episode_return'][1:][keep], o['a_episode_return'][:-1][keep])
    np.testing.assert_array_equal(o['a_episode_length'][1:][keep], o['a_episode_length'][:-1][keep])


# ---- 1 / 2. equivalence with given references, and the episode statistics of the same run -------------------------------------------
_RUNS = {}


def _staggered_run(engine, mode, refkind):
    key = (mode, refkind)
    if key in _RUNS:
        return _RUNS[key]
    from serl_amd import builds, refsignals as rs
    N = 70
    T = rs.n_steps_for(T_SHORT)
    if refkind == 'table':
        refs = _tables(N, T_SHORT, 41)
        assert refs.shape == (N, T, 3)
    else:
        refs = rs.ref_specs(*rs.training_references(1, 20, np.random.RandomState(8)), 0.2106)
    kw = {}
    if builds.has_sensor_noise(mode):
        kw['sensor_noise'] = np.stack([builds.sensor_noise_table(T, np.random.RandomState(300 + e)) for e in range(N)])
    p = Pair(_venv(N, mode, T_SHORT, engine, refs=refs, **kw), _venv(N, mode, T_SHORT, engine, refs=refs, auto_reset=True, **kw))
    assert p.a.max_steps == p.m.max_steps == T
    dev = p.a.device
    acts = _actions(3 + 4 * T, N, 3, seed=7).to(dev)
    e = torch.arange(N, device=dev)
    # stagger: reset all, two steps, reset every third env, one step, reset every fifth
    p.reset()
    p.step(acts[0]); p.step(acts[1])
    p.reset(e % 3 == 0)
    p.step(acts[2])
    p.reset(e % 5 == 0)
    p.rec.clear()
    for k in range(4 * T):
        p.step(acts[3 + k])
    _RUNS[key] = o = p.arrays()
    return o


MODES = ['nominal', 'cg-timed', 'gust']


@pytest.mark.parametrize('refkind', ['table', 'spec'])
@pytest.mark.parametrize('mode', MODES)
def test_equivalence_with_given_references(engine, mode, refkind):
    o = _staggered_run(engine, mode, refkind)
    done = o['m_done']
    per_step = done.sum(1)
    assert (per_step == 0).any(), 'no step without a finish'
    assert ((per_step > 0) & (per_step < done.shape[1])).any(), 'no step on which a strict subset finishes'
    assert (done.sum(0) >= 3).all(), 'fewer than three restarts of some env'
    _compare(o)
    assert np.isfinite(o['a_obs']).all() and np.isfinite(o['a_reward']).all()


@pytest.mark.parametrize('refkind', ['table', 'spec'])
@pytest.mark.parametrize('mode', MODES)
def test_episode_statistics(engine, mode, refkind):
    o = _staggered_run(engine, mode, refkind)
    assert o['m_done'].any() and not o['m_done'].all()
    _compare_statistics(o)


# ---- 3. the pool of drawn references: rows j % R, wrapping ----------------------------------------------------------------------------
def test_reference_pool_wraps(engine):
    from serl_amd import refsignals as rs
    N, R, t_max, seed, EPIS = 6, 2, 5, 1234, 3
    np.random.seed(seed)
    auto = _venv(N, 'nominal', t_max, engine, refs=None, auto_reset=True, ref_pool=R)
    obs_a = auto.reset().clone()
    after_reset = np.random.get_state()
    np.random.seed(seed)
    specs = rs.ref_specs(*rs.training_references(N * R, t_max, np.random, n_actions=3), theta_trim_deg=auto._trim).reshape(N, R)
    after_draw = np.random.get_state()
    assert after_reset[0] == after_draw[0] and after_reset[2:] == after_draw[2:]
    np.testing.assert_array_equal(after_reset[1], after_draw[1])
    assert not (specs[:, 0] == specs[:, 1]).any()                    # the rows differ: a wrong row shows
    manual = _venv(N, 'nominal', t_max, engine, refs=np.ascontiguousarray(specs[:, 0]))
    np.testing.assert_array_equal(manual.reset().cpu().numpy(), obs_a.cpu().numpy())
    p = Pair(manual, auto)
    epi = np.zeros(N, np.int64)

    def next_refs(done):
        idx = np.nonzero(done)[0]
        if not len(idx):
            return None
        epi[idx] += 1
        return np.ascontiguousarray(specs[idx, epi[idx] % R])
    steps = EPIS * auto.max_steps
    acts = _actions(steps, N, 3, seed=11).to(auto.device)
    for k in range(steps):
        p.step(acts[k], next_refs)
    o = p.arrays()
    assert (o['m_done'].sum(0) >= EPIS).all()                       # three episodes each: the pool of two has wrapped
    _compare(o)
    _compare_statistics(o)
    # the references differ between the episodes of an env: row 1 flown in the second, row 0 again in the third
    first = [int(np.argmax(o['m_done'][:, e])) for e in range(N)]
    assert any(not np.array_equal(o['a_ref'][:first[e] + 1, e], o['a_ref'][first[e] + 1:2 * first[e] + 2, e]) for e in range(N))


# ---- 4. the env configurations and rate control --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['PHlab_symmetric_nominal', 'PHlab_full_nominal', 'PHlab_attitude_incremental', 'PHlab_full_incremental'])
def test_configurations(engine, name):
    from serl_amd import builds, refsignals as rs
    N = 3
    S, A = builds.env_dims(*builds.env_config(name))
    T = rs.n_steps_for(T_SHORT)
    refs = _tables(N, T_SHORT, 43, A)
    p = Pair(_venv(N, name, T_SHORT, engine, refs=refs), _venv(N, name, T_SHORT, engine, refs=refs, auto_reset=True))
    assert (p.a.state_dim, p.a.action_dim) == (S, A)
    p.reset()
    acts = _actions(2 * T, N, A, seed=5).to(p.a.device)
    for k in range(2 * T):
        p.step(acts[k])
    o = p.arrays()
    assert o['a_obs'].shape[1:] == (N, S) and o['a_final_obs'].shape[1:] == (N, S)
    assert (o['m_done'].sum(0) == 2).all()
    _compare(o)
    _compare_statistics(o)
    if p.a.incremental:      # the restarted observation carries last_u = 0, the terminal one the integrated command
        done = o['m_done']
        assert (o['a_obs'][done][:, S - A:] == 0.0).all()
        assert (o['a_final_obs'][done][:, S - A:] != 0.0).any()


# ---- 5. a never-reset env stays frozen; f64 actions -----------------------------------------------------------------------------------
def test_never_reset_env_is_frozen(engine):
    env = _venv(3, 'nominal', T_SHORT, engine, refs=_tables(3, T_SHORT, 44), auto_reset=True)
    before = [b.clone() for b in (env._state, env._run_return, env._run_length, env._cursor, env._ep_return, env._ep_length)]
    for _ in range(2):
        obs, rew, done, info = env.step(torch.full((3, 3), 0.3, device=env.device))
        assert done.all() and (rew == 0).all()
        np.testing.assert_array_equal(info['final_obs'].cpu().numpy(), obs.cpu().numpy())
    for b, a in zip(before, (env._state, env._run_return, env._run_length, env._cursor, env._ep_return, env._ep_length)):
        assert torch.equal(a, b)


def test_f64_actions(engine):
    from serl_amd import refsignals as rs
    N, T = 5, rs.n_steps_for(T_SHORT)
    refs = _tables(N, T_SHORT, 45)
    p = Pair(_venv(N, 'nominal', T_SHORT, engine, refs=refs), _venv(N, 'nominal', T_SHORT, engine, refs=refs, auto_reset=True))
    p.reset()
    acts = (_actions(2 * T, N, 3, seed=9, dtype=torch.float64) * 2.5).to(p.a.device)      # outside [-1, 1] too: not clipped
    f32 = acts.float().double()
    assert (acts != f32).any()                                                         # not representable in f32: the f64 path shows
    for k in range(2 * T):
        p.step(acts[k])
    o = p.arrays()
    assert (o['m_done'].sum(0) == 2).all()
    _compare(o)
    _compare_statistics(o)


# ---- 6. bad arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(engine):
    from serl_amd import _capi, refsignals as rs
    N = 4
    refs = _tables(N, T_SHORT, 46)
    p = Pair(_venv(N, 'nominal', T_SHORT, engine, refs=refs), _venv(N, 'nominal', T_SHORT, engine, refs=refs, auto_reset=True))
    p.reset()
    env, dev = p.a, p.a.device
    L, ctx = engine.lib, engine.ctx
    act = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    state0 = env._state.clone()

    def call(d, au, actions=act, f64=0, obs=env._obs, reward=env._reward, done=env._done):
        ptr = lambda t: None if t is None else t.data_ptr()
        return L.serl_venv_step_auto(ctx, ctypes.byref(d), ptr(actions), f64, ptr(obs), ptr(reward), ptr(done), None, None, None, None,
                                     ctypes.byref(au), None)
    good_d, good_au = _capi.VenvDesc.from_buffer_copy(env.desc), _capi.VenvAutoDesc.from_buffer_copy(env.auto_desc)
    for field in ('final_obs', 'ep_return', 'ep_length', 'run_return', 'run_length', 'cursor'):
        au = _capi.VenvAutoDesc.from_buffer_copy(env.auto_desc)
        setattr(au, field, None)
        assert call(good_d, au) == _capi.E_INVALID, field
    for kw in (dict(obs=None), dict(reward=None), dict(done=None), dict(actions=None), dict(f64=2), dict(f64=-1)):
        assert call(good_d, good_au, **kw) == _capi.E_INVALID, kw
    pool = torch.zeros(N, 2, rs.REF_SPEC_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    au = _capi.VenvAutoDesc.from_buffer_copy(env.auto_desc)
    au.ref_pool, au.pool_rows = pool.data_ptr(), 2
    assert call(good_d, au) == _capi.E_INVALID                       # a pool together with desc->ref
    assert b'desc->ref' in L.serl_last_error()
    d = _capi.VenvDesc.from_buffer_copy(env.desc)
    d.ref, d.ref_stride = None, 0
    for rows in (0, -1):
        au.pool_rows = rows
        assert call(d, au) == _capi.E_INVALID, rows
        assert b'pool_rows' in L.serl_last_error()
    torch.cuda.synchronize()
    assert torch.equal(env._state, state0)                           # nothing was launched
    with pytest.raises(ValueError):
        env.step(torch.zeros(N, 2, device=dev))
    with pytest.raises(ValueError):
        env.step(torch.zeros(N + 1, 3, device=dev))
    with pytest.raises(ValueError):
        env.step(torch.zeros(N, 3))                                  # host tensor
    with pytest.raises(ValueError):
        _venv(N, 'nominal', T_SHORT, engine, refs=refs, auto_reset=True, ref_pool=0)
    # a following good call still matches
    acts = _actions(8, N, 3, seed=3).to(dev)
    for k in range(8):
        p.step(acts[k])
    o = p.arrays()
    assert o['m_done'].any()
    _compare(o)

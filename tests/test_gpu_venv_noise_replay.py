"""Device-noise episodes of CitationVecEnv flown again on the CPU oracle (same-libm flavour), at ZERO tolerance, in every code variant.

What the feature promises is replay: from `noise_seed`, the env index and the episode ordinal, `serl_amd.venv_noise` writes out the sensor and
exploration noise an episode saw, and the oracle, fed those tables, the carried error and the model clock, flies the same episode bit for bit.
Here that is done for every episode of a run with restarts inside the launches, an explicit partial reset between two launches (an episode
abandoned without a step), a restart on a launch's last step and a trailing partial episode -- tests/noise_replay.py finds the episodes --
through all four noise entry points: serl_venv_rollout_noise, serl_venv_rollout_general_noise, and serl_venv_step_auto_noise +
serl_venv_reset_noise behind path='loop'.  Episodes are six steps (t_max = 0.05 s, table references); N = 70 is one full and one partial
wavefront.  Then the free parameters of the C ABI the Python defaults never move (sensor_bias / sensor_scale), and the header's promise that
the noise entry points with the generator off compute what their namesakes compute."""
import ctypes
import numpy as np
import pytest
import torch

import noise_replay
from actor_shapes import make_weights, _shape, spec_of, net_of

pytestmark = pytest.mark.gpu
T_SHORT = 0.05
SEED = 0x5EED0123456789AB
SD, CLIP = 0.3, 0.5
K1, K2 = 12, 8
EP = 6                  # steps of an episode
MEMBERS = 3
THREADS = 16


def _np(t):
    return t.cpu().numpy()


def _tables(N, seed=41):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rs.n_steps_for(T_SHORT)])
    assert np.isfinite(r).all() and r.shape[1] == EP
    return r


def _shape_of(mode, hidden, layers):
    from serl_amd import builds
    cfg, incr = builds.env_config(mode)
    return _shape(hidden, layers, 'tanh', cfg, incr)


def _record(engine, mode, N, s, path, clock0=None, kernel='lane'):
    """the run: reset(), 12 steps, reset(every third env), 8 steps -> the env, the joined recording, the observations of the two resets
    (clock0: the first reset starts the model clocks there instead of at 0)"""
    import serl_amd
    refs = _tables(N)
    env = serl_amd.CitationVecEnv(N, mode, t_max=T_SHORT, refs=refs, engine=engine, auto_reset=True, seed=SEED, sensor_noise='device',
                                  kernel=kernel)
    assert (env.state_dim, env.action_dim) == (s['state_dim'], s['action_dim']) and env.max_steps == EP
    dev = env.device
    w = np.ascontiguousarray(make_weights(s, MEMBERS, 21))
    wt = torch.from_numpy(w).to(dev)
    moe = np.arange(N, dtype=np.int32) % MEMBERS
    third = torch.arange(N, device=dev) % 3 == 0
    roll = lambda K: env.rollout(wt, K, spec=spec_of(s), member_of_env=moe, action_noise='device', noise_sd=SD, noise_clip=CLIP,
                                 transitions=True, path=path)
    reset_obs = [_np(env.reset(tick0=clock0)).copy()]
    assert env.last_step_kernel == kernel
    p1 = {k: _np(v) for k, v in roll(K1).items()}
    ran = env.last_rollout_path
    reset_obs.append(_np(env.reset(third)).copy())
    p2 = {k: _np(v) for k, v in roll(K2).items()}
    assert env.last_rollout_path == ran
    np.testing.assert_array_equal(p1['obs'][0], reset_obs[0])
    np.testing.assert_array_equal(p2['obs'][0], reset_obs[1])
    rec = {k: np.concatenate([p1[k], p2[k]]) for k in p1 if k != 'obs'}
    rec['obs_after'] = np.concatenate([p1['obs'][1:], p2['obs'][1:]])
    return env, refs, w, moe, _np(third), rec, reset_obs, ran


def _noise_free_twin(engine, mode, N, refs, third, rec, clock0=None, kernel='lane'):
    """the observations of an env without sensor noise on the recorded actions (the noise is added to what the model returns and never
    fed back, so the twin flies the same states)"""
    import serl_amd
    twin = serl_amd.CitationVecEnv(N, mode, t_max=T_SHORT, refs=refs, engine=engine, auto_reset=True, sensor_noise=False, kernel=kernel)
    acts = torch.from_numpy(rec['actions']).to(twin.device)
    twin.reset(tick0=clock0)
    obs = []
    for k in range(K1 + K2):
        if k == K1:
            twin.reset(torch.from_numpy(third).to(twin.device))
        obs.append(_np(twin.step(acts[k])[0]).copy())
    assert twin.last_step_kernel == kernel
    return np.stack(obs)


# The time-switched builds change at model time 20 s (clock tick 2000: cg_timed shifts its centre of gravity, gust starts blowing) and nowhere near
# the ticks 0 .. 24 a run from a fresh env reaches.  Started from these clocks, 1978 .. 2001 spread over the envs, every env crosses tick 2000
# inside the run -- in the middle of an episode, at a restart, behind the explicit reset (env 0, also of five) --, so an episode restarted with
# another clock is another episode.
def _switch_clocks(N):
    return 1978 + (np.arange(N) * 5 + 3) % 24


def _replay_case(engine, mode, N, hidden, layers, path, want_path, clock0=None, kernel='lane'):
    """-> the env that flew (made with kernel=`kernel`)"""
    import serl_amd
    from serl_amd import builds
    from oracle import rollout as R
    s = _shape_of(mode, hidden, layers)
    S, A = s['state_dim'], s['action_dim']
    env, refs, w, moe, third, rec, reset_obs, ran = _record(engine, mode, N, s, path, clock0, kernel)
    assert ran == want_path
    K = K1 + K2
    done = rec['done']
    eps = noise_replay.episodes(done, [(0, None), (K1, third)], clock0=clock0)
    _, kin = noise_replay.ordinals(done, eps)
    np.testing.assert_array_equal(_np(env.noise_episode), noise_replay.starts(eps, N))
    build, row = builds.resolve_mode(mode)
    assert build == env.build
    compared_rows, compared_eps, completed = 0, 0, np.zeros(N, np.int64)
    clip_bites, late_clock, clock_matters = False, False, False
    for o in sorted({ep.ordinal for ep in eps}):
        batch = [ep for ep in eps if ep.ordinal == o]
        idx = np.array([ep.env for ep in batch])
        sn = _np(serl_amd.venv_noise(SEED, idx, o, EP + 1, 'sensor', engine=engine))
        an = _np(serl_amd.venv_noise(SEED, idx, o, EP, 'action', noise_sd=SD, noise_clip=CLIP, engine=engine))
        assert sn.shape == (len(batch), EP + 1, 7) and an.shape == (len(batch), EP, 3)
        err0 = np.zeros((len(batch), 3))
        for i, ep in enumerate(batch):      # the error of the env's last step before the start: reference row of that step minus (theta, phi, beta)
            if ep.err_row >= 0:
                r = ep.err_row
                err0[i, :A] = (refs[ep.env, kin[r, ep.env]] - rec['x'][r, ep.env][[7, 6, 5]])[:A]
        orc = R.rollout(w, net_of(s), moe[idx], refs[idx], build=build, faults=None if row == builds.NOMINAL_ROW else [list(row)] * len(batch),
                        err0=err0, tick0=[ep.tick0 for ep in batch], action_noise=an, sensor_noise=sn, t_max=T_SHORT, traces=True,
                        transitions=True, threads=min(THREADS, len(batch)), env_config=s['env_config'], incremental=s['incremental'],
                        short_libm=True)
        assert (orc['length_steps'] == EP).all()
        if clock0 is not None:      # the same episodes one tick behind: the clock is not a spectator
            kw = dict(build=build, err0=err0, tick0=[ep.tick0 - 1 for ep in batch], action_noise=an, sensor_noise=sn, t_max=T_SHORT, traces=True,
                      threads=min(THREADS, len(batch)), short_libm=True)
            clock_matters = clock_matters or not np.array_equal(R.rollout(w, net_of(s), moe[idx], refs[idx], **kw)['states'], orc['states'])
        for i, ep in enumerate(batch):
            e, n, rows = ep.env, ep.n, slice(ep.row0, ep.row0 + ep.n)
            what = 'env %d ordinal %d rows %d .. %d' % (e, o, ep.row0, ep.row0 + n - 1)
            assert ep.k0 == 0 and n <= EP and ep.finished == (n == EP), what
            first = reset_obs[ep.obs0[1]][e] if ep.obs0[0] == 'reset' else rec['obs_after'][ep.obs0[1], e]
            np.testing.assert_array_equal(first.astype(np.float32), orc['transitions'][i, 0, :S], err_msg=what + ': first observation')
            np.testing.assert_array_equal(rec['transitions'][rows, e], orc['transitions'][i, :n], err_msg=what + ': transitions')
            np.testing.assert_array_equal(rec['x'][rows, e], orc['states'][i, :n], err_msg=what + ': x')
            np.testing.assert_array_equal(rec['reward'][rows, e], orc['rewards'][i, :n], err_msg=what + ': reward')
            if ep.finished:
                last = ep.row0 + n - 1
                assert rec['ep_return'][last, e] == orc['fitness'][i] and rec['ep_length'][last, e] == EP, what
                completed[e] += 1
            compared_rows += n
            compared_eps += 1
            clip_bites = clip_bites or bool((np.abs(an[i, :n, :A]) == CLIP).any())
            late_clock = late_clock or ep.tick0 > 0
    # ---- the comparison above was not empty
    assert (completed >= 3).all(), 'an env completed fewer than three episodes'
    left_out = 1.0 - compared_rows / float(K * N)
    assert left_out == 0.0 and compared_eps == len(eps), (left_out, compared_eps, len(eps))
    assert any(ep.n == 0 for ep in eps) and any(0 < ep.n < EP for ep in eps)      # the abandoned episode, the trailing one
    assert done.sum(0).min() == 3                                                    # three restarts inside the launches
    assert clip_bites, 'the action clip never bites'
    assert late_clock, 'no compared episode started with a running model clock'
    assert clock0 is None or clock_matters, 'the episodes do not depend on the model clock'
    a = rec['actions']
    print('%s %s: %d episodes, |action| < 1 in %.3f of the entries' % (mode, ran, len(eps), (np.abs(a) < 1.0).mean()))
    assert (np.abs(a) <= 1.0).all() and (np.abs(a) < 1.0).any(), 'every action is at +-1'
    assert not np.array_equal(a[:, 0], a[:, 1])
    quiet = _noise_free_twin(engine, mode, N, refs, third, rec, clock0, kernel)
    assert (quiet != rec['obs_after']).any(-1).all(), 'an observation carries no sensor noise'
    assert np.isfinite(rec['obs_after']).all() and np.isfinite(rec['reward']).all()
    return env


@pytest.mark.parametrize('mode', ['noise', 'ice', 'cg-timed', 'gust', 'test', 'jr'])
def test_rollout_noise_replays_on_the_oracle(engine, mode):
    """serl_venv_rollout_noise (hidden 32 x 3, the attitude task)"""
    _replay_case(engine, mode, 70, 32, 3, 'fused', 'fused')


@pytest.mark.parametrize('mode', ['gust', 'cg-timed', 'PHlab_symmetric_noise', 'PHlab_full_noise', 'PHlab_attitude_incremental',
                                  'PHlab_symmetric_incremental', 'PHlab_full_incremental'])
def test_rollout_general_noise_replays_on_the_oracle(engine, mode):
    """serl_venv_rollout_general_noise (hidden 8 x 1).  The incremental modes have no sensor model of their own: sensor_noise='device' adds
    the generator's addends there as a table would"""
    _replay_case(engine, mode, 70, 8, 1, 'fused', 'fused-general')


@pytest.mark.parametrize('mode', ['ice', 'cg-timed', 'test', 'PHlab_full_noise', 'PHlab_symmetric_incremental'])
def test_step_auto_noise_and_reset_noise_replay_on_the_oracle(engine, mode):
    """serl_venv_step_auto_noise + serl_venv_reset_noise: the step loop of a device-noise env"""
    _replay_case(engine, mode, 5, 8, 1, 'loop', 'loop')


@pytest.mark.parametrize('mode', ['cg-timed', 'gust'])
@pytest.mark.parametrize('hidden,layers,N,path,ran', [(32, 3, 70, 'fused', 'fused'), (8, 1, 70, 'fused', 'fused-general'), (8, 1, 5, 'loop', 'loop')])
def test_replay_across_the_clock_switch(engine, mode, hidden, layers, N, path, ran):
    """the time-switched builds started just in front of their switch: the clock every restart carries on decides what the episode flies"""
    _replay_case(engine, mode, N, hidden, layers, path, ran, clock0=_switch_clocks(N))


# ---- sensor_bias / sensor_scale at the ABI ---------------------------------------------------------------------------------------------------
# a zero scale (r), a negative scale (q, beta), a zero bias (q, phi), a large bias (p: observed only, no bound reads it)
BIAS = (1.0e3, 0.0, 3.0e-5, -7.25, 1.8e-3, 0.0, 4.0e-3)
SCALE = (6.3e-4, -2.0, 0.0, 4.0e-10, -2.7e-4, 3.2e-5, 0.125)


def _nz(env=None, sensor=0):
    from serl_amd import _capi
    return _capi.VenvNoiseDesc(seed=SEED, episode_count=None if env is None else env.noise_episode.data_ptr(), sensor=sensor,
                               sensor_bias=(ctypes.c_double * 7)(*BIAS), sensor_scale=(ctypes.c_double * 7)(*SCALE))


def _fill(engine, nz, mode, W, env, episode, entry0, entries):
    dev = engine.device
    cols = [torch.as_tensor(np.asarray(v), dtype=torch.int32).to(dev).contiguous() for v in (env, episode, entry0)]
    out = torch.full((len(cols[0]), entries, W), 9.0, dtype=torch.float64, device=dev)
    rc = engine.lib.serl_venv_noise_fill(engine.ctx, ctypes.byref(nz), mode, len(cols[0]), cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(),
                                         entries, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, engine.lib.serl_last_error()
    torch.cuda.synchronize()
    return _np(out)


def test_fill_applies_the_callers_bias_and_scale(engine):
    """mode 2 = bias + scale * z of mode 1, the product rounded before the sum, for a row that is not the Python default; 70 rows whose
    entries start near 0 and near 8000"""
    r = np.arange(70)
    env, episode = (r * 937 + 3) % 65536, (r * 7) % 50
    entry0 = np.where(r % 2 == 0, r % 5, 7990 + r % 11)
    assert entry0.min() == 0 and entry0.max() == 8000
    nz = _nz()
    z = _fill(engine, nz, 1, 7, env, episode, entry0, 8)
    got = _fill(engine, nz, 2, 7, env, episode, entry0, 8)
    np.testing.assert_array_equal(got, np.array(BIAS) + np.array(SCALE) * z)
    assert (got[..., 2] == BIAS[2]).all() and (got[..., 0] > 999.0).all() and np.abs(z).max() > 2.0
    from serl_amd import builds
    assert not np.array_equal(got, builds.sensor_terms(z))


def test_step_auto_noise_applies_the_callers_bias_and_scale(engine):
    """reset and one serl_venv_step_auto_noise step with that row against the table path fed by the fill kernel with the same row"""
    bias_and_scale_case(engine)


def bias_and_scale_case(engine, wave=False):
    """wave: serl_venv_reset_wave_noise / serl_venv_step_auto_wave_noise, still against the lane kernels' table path"""
    import serl_amd
    N = 70
    refs = _tables(N)
    D = serl_amd.CitationVecEnv(N, 'noise', t_max=T_SHORT, refs=refs, engine=engine, auto_reset=True, seed=SEED, sensor_noise='device',
                                kernel='wave' if wave else 'lane')
    D._nz_desc = lambda *a, **kw: _nz(D, sensor=1)
    table = _fill(engine, _nz(), 2, 7, np.arange(N), np.zeros(N), np.zeros(N), EP + 1)
    Tb = serl_amd.CitationVecEnv(N, 'noise', t_max=T_SHORT, refs=refs, engine=engine, sensor_noise=table)
    od, ot = D.reset(), Tb.reset()
    assert D.last_step_kernel == ('wave' if wave else 'lane') and Tb.last_step_kernel == 'lane'
    assert torch.equal(od, ot)
    assert (_np(od)[:, 3] > 999.0).all()                    # p carries the large bias
    g = torch.Generator(device='cpu').manual_seed(9)
    a = ((torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.6).to(D.device)
    od, rd, dd, idd = D.step(a)
    ot, rt, dt, itt = Tb.step(a)
    assert D.last_step_kernel == ('wave' if wave else 'lane') and Tb.last_step_kernel == 'lane'
    assert torch.equal(od, ot) and torch.equal(rd, rt) and torch.equal(dd, dt) and not bool(dd.any())
    for key in ('x', 'ref', 't', 'cost'):
        assert torch.equal(idd[key], itt[key]), key
    x = _np(idd['x'])
    assert (x[:, 0] > 999.0).all() and np.isfinite(x).all()
    np.testing.assert_array_equal(_np(D.noise_episode), np.ones(N))


# ---- generator off: the noise entry points compute what their namesakes compute ------------------------------------------------------------
def _pair(engine, N, wave=False):
    """a gust env with a generator state that draws nothing from it (seed= only: a sensor table, action tables), and one without;
    wave: both on the wave kernels"""
    import serl_amd
    from serl_amd import builds
    tab = np.stack([builds.sensor_noise_table(EP, np.random.RandomState(300 + e)) for e in range(N)])
    kw = dict(t_max=T_SHORT, refs=_tables(N), engine=engine, auto_reset=True, sensor_noise=tab, kernel='wave' if wave else 'lane')
    a, b = serl_amd.CitationVecEnv(N, 'gust', seed=SEED, **kw), serl_amd.CitationVecEnv(N, 'gust', **kw)
    assert a.noise_episode is not None and not a._dev_sensor and b.noise_episode is None
    return a, b


def _same_state(a, b):
    for name in ('_state', '_run_return', '_run_length', '_cursor', '_ep_return', '_ep_length'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_generator_off_reset_and_step_equal_their_namesakes(engine):
    """serl_venv_reset_noise / serl_venv_step_auto_noise with nz->sensor = 0 against serl_venv_reset / serl_venv_step_auto"""
    generator_off_step_case(engine)


def generator_off_step_case(engine, wave=False):
    N = 70
    a, b = _pair(engine, N, wave)
    dev = a.device
    third = torch.arange(N, device=dev) % 3 == 0
    g = torch.Generator(device='cpu').manual_seed(9)
    acts = ((torch.rand(K1 + K2, N, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.6).to(dev)
    want = np.ones(N, np.int64)
    assert torch.equal(a.reset(), b.reset())
    np.testing.assert_array_equal(_np(a.noise_episode), want)
    for k in range(K1 + K2):
        if k == 3:
            assert torch.equal(a.reset(third), b.reset(third))
            want += _np(third)
            np.testing.assert_array_equal(_np(a.noise_episode), want)
        oa, ra, da, ia = a.step(acts[k] if k % 2 else acts[k].float())
        ob, rb, db, ib = b.step(acts[k] if k % 2 else acts[k].float())
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert a.last_step_kernel == b.last_step_kernel == ('wave' if wave else 'lane')
        assert ia.keys() == ib.keys()
        for key in ia:
            assert torch.equal(ia[key], ib[key]), (k, key)
        want += _np(da)
        np.testing.assert_array_equal(_np(a.noise_episode), want)
    _same_state(a, b)
    assert (want == 4).all()      # reset, three restarts (rows 5, 11, 17); every third env: reset, reset, two restarts (rows 8, 14)


@pytest.mark.parametrize('hidden,layers,path,ran', [(32, 3, 'fused', 'fused'), (8, 1, 'fused', 'fused-general'), (8, 1, 'loop', 'loop')])
def test_generator_off_rollout_equals_its_namesake(engine, hidden, layers, path, ran):
    """serl_venv_rollout_noise / _rollout_general_noise with nz->sensor = nz->action = 0 and an action table against serl_venv_rollout /
    _rollout_general, key for key and in the env state.  The step loop of an env with a generator state runs the kernels' forward where
    the other env runs torch's (serl_amd/venv.py), so the 'loop' case flies a zero actor, whose action is 0 in both: what is compared is
    serl_venv_step_auto_noise against serl_venv_step_auto on the table's actions."""
    generator_off_rollout_case(engine, hidden, layers, path, ran)


def generator_off_rollout_case(engine, hidden, layers, path, ran, wave=False):
    N = 70 if path == 'fused' else 5
    a, b = _pair(engine, N, wave)
    dev = a.device
    s = _shape(hidden, layers)
    w = torch.from_numpy(np.ascontiguousarray(make_weights(s, MEMBERS, 5))).to(dev)
    if path == 'loop':
        w = torch.zeros_like(w)
    moe = np.arange(N, dtype=np.int32) % MEMBERS
    g = torch.Generator(device='cpu').manual_seed(50)
    noise = (torch.randn(K1 + K2, N, 3, generator=g, dtype=torch.float64) * 0.4).to(dev)
    third = torch.arange(N, device=dev) % 3 == 0
    assert torch.equal(a.reset(), b.reset())
    want = np.ones(N, np.int64)
    for lo, hi in ((0, K1), (K1, K1 + K2)):
        if lo:
            assert torch.equal(a.reset(third), b.reset(third))
            want += _np(third)
        kw = dict(spec=spec_of(s), member_of_env=moe, action_noise=noise[lo:hi], transitions=True, path=path)
        oa, ob = a.rollout(w, hi - lo, **kw), b.rollout(w, hi - lo, **kw)
        assert a.last_rollout_path == b.last_rollout_path == ran and oa.keys() == ob.keys()
        for key in oa:
            assert torch.equal(oa[key], ob[key]), key
        _same_state(a, b)
        want += _np(oa['done']).sum(0)
        np.testing.assert_array_equal(_np(a.noise_episode), want)
        assert oa['actions'].abs().max() > 0 and bool((oa['actions'].abs() < 1).any())
    assert want.min() == 4 and want.max() == 5

"""Sensor and exploration noise drawn inside the env kernels (serl_venv_*_noise, serl_venv_noise_fill; CitationVecEnv(sensor_noise='device'),
rollout(action_noise='device'), serl_amd.venv_noise) on the GPU.

The generator is checked bottom-up: its bits against the host export (which tests/test_rng_host.py holds to a NumPy restatement of
Philox4x32-10), its normals against that restatement continued in long double, its addends exactly, its statistics; then the env kernels
against the TABLE path at zero tolerance -- an env without auto-reset that is refilled at every reset with the table serl_venv_noise_fill
writes for the episode the restarted env will fly -- and the rollout kernels against the fill kernel and against each other.
Episodes are six steps (t_max = 0.05 s, table references), 20 steps give three restarts per env; N = 70 covers a partial wavefront."""
import ctypes
import numpy as np
import pytest
import torch

import noise_replay
import rng_ref
from actor_shapes import make_weights, _shape, spec_of

pytestmark = pytest.mark.gpu
T_SHORT = 0.05
SEED = 0x5EED0123456789AB
SD, CLIP = 0.3, 0.5
STEPS = 20


def _np(t):
    return t.cpu().numpy()


def _tables(N, seed=41):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rs.n_steps_for(T_SHORT)])
    assert np.isfinite(r).all() and r.shape[1] == 6
    return r


def _dev_env(N, mode, engine, seed=SEED, **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(N, mode=mode, t_max=T_SHORT, refs=_tables(N), engine=engine, auto_reset=True, seed=seed, **kw)


def _actions(steps, N, A, dev, seed=9):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return ((torch.rand(steps, N, A, generator=g, dtype=torch.float64) * 2 - 1) * 0.6).to(dev)


def _fill(engine, kind, env, episode, entries, entry0=0, seed=SEED, **kw):
    import serl_amd
    return _np(serl_amd.venv_noise(seed, env, episode, entries, kind, entry0=entry0, engine=engine, **kw))


@pytest.fixture(scope='module')
def grid70():
    """70 rows x 8 entries with distinct env / episode / entry0 (read-only)"""
    r = np.arange(70)
    return dict(env=(r * 937 + 3) % 65536, episode=(r * 7) % 50, entry0=(r * 13) % 2000)


# ---- 1. bits -----------------------------------------------------------------------------------------------------------------------------
def test_fill_words_equal_the_host_export(engine, grid70):
    L = engine.lib
    got = _fill(engine, 'bits', grid70['env'], grid70['episode'], 8, grid70['entry0']).view(np.uint32)
    assert got.shape == (70, 8, 24)
    out = (ctypes.c_uint32 * 4)()
    want = np.zeros_like(got)
    for i in range(70):
        for j in range(8):
            for b in range(6):
                stream, block = (0, b) if b < 4 else (1, b - 4)
                L.serl_host_philox(SEED, int(grid70['env'][i]), int(grid70['episode'][i]), int(grid70['entry0'][i]) + j, stream << 16 | block, out)
                want[i, j, 4 * b:4 * b + 4] = list(out)
    np.testing.assert_array_equal(got, want)
    # ... and the restatement, vectorised
    for b in range(6):
        stream, block = (0, b) if b < 4 else (1, b - 4)
        ref = rng_ref.words(SEED, grid70['env'][:, None], grid70['episode'][:, None], grid70['entry0'][:, None] + np.arange(8)[None], stream, block)
        np.testing.assert_array_equal(got[..., 4 * b:4 * b + 4], ref)


# ---- 2. normals --------------------------------------------------------------------------------------------------------------------------
def test_fill_normals_against_the_long_double_restatement(engine, grid70):
    """|gpu - ref| <= 8 * 2^-52 * max(r, 1), r = the pair's radius sqrt(-2 log u0).  The 8 is the sum of the device library's documented
    bounds, doubled: log 1 ulp, halved by the root, plus the root's 0.5 (1 ulp of r), sincospi 2 ulp of 1 (times r), the product 0.5 -- 3.5 ulp
    of r, and in front of them nothing: the uniforms are exact.  Relative to the radius, not to z: cos passes through zero.  The action
    stream's normals (fill mode 3 with sd = 1 and a clip beyond every normal) are held to the same bound."""
    env, ep, e0 = grid70['env'][:, None], grid70['episode'][:, None], grid70['entry0'][:, None] + np.arange(8)[None]
    got = _fill(engine, 'normal', grid70['env'], grid70['episode'], 8, grid70['entry0'])
    ref, rad = rng_ref.normals(SEED, env, ep, e0, rng_ref.SENSOR, 4)
    err = np.abs(got.astype(np.longdouble) - ref[..., :7])
    bound = 8 * np.longdouble(2.0) ** -52 * np.maximum(rad[..., :7], 1)
    print('normals: max |gpu - ref| / (2^-52 max(r, 1)) =', float((err / (bound / 8)).max()))
    assert (err <= bound).all()
    assert np.abs(got).max() > 2.0 and np.isfinite(got).all()
    got = _fill(engine, 'action', grid70['env'], grid70['episode'], 8, grid70['entry0'], noise_sd=1.0, noise_clip=1e300)
    ref, rad = rng_ref.normals(SEED, env, ep, e0, rng_ref.ACTION, 2)
    err = np.abs(got.astype(np.longdouble) - ref[..., :3])
    assert (err <= 8 * np.longdouble(2.0) ** -52 * np.maximum(rad[..., :3], 1)).all()


# ---- 3. addends --------------------------------------------------------------------------------------------------------------------------
def test_fill_addends_are_exact(engine, grid70):
    from serl_amd import builds
    a = (grid70['env'], grid70['episode'], 8, grid70['entry0'])
    z = _fill(engine, 'normal', *a)
    np.testing.assert_array_equal(_fill(engine, 'sensor', *a), builds.sensor_terms(z))
    za = _fill(engine, 'action', *a, noise_sd=1.0, noise_clip=1e300)      # 1.0 z clipped nowhere: the action stream's normals themselves
    assert np.abs(za).max() > CLIP / SD                                    # (the clip below bites)
    np.testing.assert_array_equal(_fill(engine, 'action', *a, noise_sd=SD, noise_clip=CLIP), np.clip(SD * za, -CLIP, CLIP))
    np.testing.assert_array_equal(_fill(engine, 'action', *a, noise_sd=SD, noise_clip=0.0), np.zeros_like(za))
    assert not np.array_equal(za, z[..., :3])                              # two streams


# ---- 4. statistics -----------------------------------------------------------------------------------------------------------------------
def test_normals_are_standard_and_uncorrelated(engine):
    R, E = 4096, 64
    z = _fill(engine, 'normal', np.arange(R), 0, E)
    assert z.shape == (R, E, 7)

    def standard(v):
        n = v.size
        assert abs(v.mean()) <= 5 / np.sqrt(n), (v.mean(), n)
        assert abs(v.var() - 1) <= 5 * np.sqrt(2 / n), (v.var(), n)
    standard(z)
    for c in range(7):
        standard(z[..., c])
    flat = np.ascontiguousarray(z.reshape(-1, 7))
    assert len(np.unique(flat.view([('', flat.dtype)] * 7))) == R * E       # no two 7-vectors are equal
    for a, b in ((z[:, :-1], z[:, 1:]), (z[:-1], z[1:])):                   # entry j against j + 1, env e against e + 1
        n = a.size
        assert abs((a * b).mean()) <= 5 / np.sqrt(n), ((a * b).mean(), n)
    # another episode and another seed are other draws
    assert not np.array_equal(z[:8], _fill(engine, 'normal', np.arange(8), 1, E))
    assert not np.array_equal(z[:8], _fill(engine, 'normal', np.arange(8), 0, E, seed=SEED + 1))


# ---- 5. the sensor path, bit for bit against the table path ---------------------------------------------------------------------------------
def _against_the_table_path(engine, mode, N):
    import serl_amd
    D = _dev_env(N, mode, engine, sensor_noise='device')
    assert D.noise_seed == SEED and D._noise is None and D.desc.sensor_noise is None
    T1 = D.max_steps + 1
    dev, A = D.device, D.action_dim
    allenv = torch.arange(N, device=dev)
    table = lambda idx, ordinal: serl_amd.venv_noise(SEED, idx, ordinal, T1, 'sensor', engine=engine)
    T = serl_amd.CitationVecEnv(N, mode=mode, t_max=T_SHORT, refs=_tables(N), engine=engine,
                                sensor_noise=table(allenv, torch.zeros(N, dtype=torch.int64, device=dev)))
    starts = np.ones(N, np.int64)                       # episode starts of every env
    assert torch.equal(D.reset(), T.reset())
    np.testing.assert_array_equal(_np(D.noise_episode), starts)
    acts = _actions(STEPS, N, A, dev)
    ret, length = np.zeros(N), np.zeros(N, np.int64)
    restarts = 0
    for k in range(STEPS):
        if k == 2:      # an explicit reset of every third env on both: it counts as a start and clears the running return
            third = allenv % 3 == 0
            idx = torch.nonzero(third).reshape(-1)
            od = D.reset(third).clone()
            ot = T.reset(third, sensor_noise=table(idx, torch.from_numpy(starts).to(dev)[idx]))
            assert torch.equal(od, ot)
            starts[_np(third)] += 1
            ret[_np(third)], length[_np(third)] = 0.0, 0
            np.testing.assert_array_equal(_np(D.noise_episode), starts)
        od, rd, dd, idd = D.step(acts[k])
        ot, rt, dt, itt = T.step(acts[k])
        assert torch.equal(rd, rt) and torch.equal(dd, dt), k
        for key in ('x', 'ref', 't', 'cost'):
            assert torch.equal(idd[key], itt[key]), (k, key)
        assert torch.equal(idd['final_obs'], ot), k                     # the terminal-aware observation is the table env's
        ret = ret + _np(rt)
        length += 1
        done = _np(dt)
        np.testing.assert_array_equal(_np(idd['episode_return'])[done], ret[done])
        np.testing.assert_array_equal(_np(idd['episode_length'])[done], length[done])
        if done.any():      # the table env is restarted by hand, with the table of the episode ordinal the restarted env will have
            idx = torch.nonzero(dt).reshape(-1)
            ot = T.reset(dt, sensor_noise=table(idx, torch.from_numpy(starts).to(dev)[idx]))
            starts[done] += 1
            ret[done], length[done] = 0.0, 0
            restarts += int(done.sum())
        assert torch.equal(od, ot), k
        np.testing.assert_array_equal(_np(D.noise_episode), starts)
    assert restarts >= 3 * N and (_np(idd['x'])[:, :3] != 0).all()
    return D


def test_sensor_noise_equals_the_table_path_mode_noise(engine):
    _against_the_table_path(engine, 'noise', 70)


def test_sensor_noise_equals_the_table_path_mode_gust(engine):
    _against_the_table_path(engine, 'gust', 5)


def test_sensor_noise_equals_the_table_path_symmetric_task(engine):
    D = _against_the_table_path(engine, 'PHlab_symmetric_noise', 5)
    assert (D.state_dim, D.action_dim) == (2, 1)


# ---- 6. restarted episodes differ ----------------------------------------------------------------------------------------------------------
def test_restarted_episodes_get_a_realisation_of_their_own(engine):
    """Same actions, same references: on the table path a restarted episode sees the first one's noise again and ends in the same x; with the
    generator it does not.  (The defect this feature removes: without it the first half of this test has nothing to run.)"""
    import serl_amd
    from serl_amd import builds
    N = 5
    D = _dev_env(N, 'noise', engine, sensor_noise='device')
    tab = np.stack([builds.sensor_noise_table(D.max_steps, np.random.RandomState(300 + e)) for e in range(N)])
    Tb = serl_amd.CitationVecEnv(N, mode='noise', t_max=T_SHORT, refs=_tables(N), engine=engine, auto_reset=True, sensor_noise=tab)
    a = torch.zeros(N, 3, dtype=torch.float64, device=D.device)
    ends = {}
    for name, env in (('device', D), ('table', Tb)):
        env.reset()
        xs = []
        for k in range(12):
            _, _, done, info = env.step(a)
            if k in (5, 11):
                assert bool(done.all())
                xs.append(_np(info['x']).copy())
        ends[name] = xs
    np.testing.assert_array_equal(ends['table'][0], ends['table'][1])
    assert (ends['device'][0][:, :3] != ends['device'][1][:, :3]).all()
    assert np.array_equal(_np(D.noise_episode), np.full(N, 3))


# ---- 7. action noise, exact ----------------------------------------------------------------------------------------------------------------
def _ordinals(done, first):
    """(episode ordinal, in-episode step) of every [k, e] from the done flags, for envs whose running episode has ordinal `first` at step 0"""
    first = np.array(first, np.int64)      # (tests/noise_replay.py: envs that fly that episode at row 0, `first + 1` starts counted)
    return noise_replay.ordinals(done, noise_replay.episodes(done, count0=first + 1, live0=np.ones(len(first), bool), clock0=np.ones(len(first))))


@pytest.mark.parametrize('hidden,layers,ask,path', [(32, 3, 'fused', 'fused'), (8, 1, 'fused', 'fused-general'), (32, 3, 'loop', 'loop'),
                                                    (8, 1, 'loop', 'loop')])
def test_action_noise_of_a_zero_actor_is_the_fill_kernels(engine, hidden, layers, ask, path):
    N = 70
    env = _dev_env(N, 'nominal', engine, seed=SEED if hidden == 8 else None)      # (hidden 32: the first device-noise rollout starts the generator)
    s = _shape(hidden, layers)
    spec = spec_of(s)
    w = torch.zeros(1, (spec.param_count + 3) // 4 * 4, dtype=torch.float32, device=env.device)
    mask = torch.ones(N, dtype=torch.bool, device=env.device)
    mask[[3, 64]] = False                                                          # two envs that are never reset stay frozen
    env.reset(mask)
    out = env.rollout(w, STEPS, spec=spec, action_noise='device', noise_sd=SD, noise_clip=CLIP, path=ask)
    assert env.last_rollout_path == path
    seed = env.noise_seed
    assert seed == SEED or hidden == 32
    act, done = _np(out['actions']), _np(out['done'])
    live = _np(mask)
    ordinal, kin = _ordinals(done[:, live], np.zeros(int(live.sum())))
    assert ordinal.max() == 3 and kin.max() == 5
    e = np.broadcast_to(np.nonzero(live)[0][None], ordinal.shape)
    want = _fill(engine, 'action', e.reshape(-1), ordinal.reshape(-1), 1, kin.reshape(-1), seed=seed, noise_sd=SD, noise_clip=CLIP)
    np.testing.assert_array_equal(act[:, live], want.reshape(STEPS, -1, 3))       # clip(0 + addend, -1, 1) = the addend: |addend| <= 0.5
    assert (act[:, ~live] == 0).all() and done[:, ~live].all()
    assert (np.abs(act[:, live]) == CLIP).any() and (act[:, live] != 0).all()
    np.testing.assert_array_equal(_np(env.noise_episode), np.where(live, 4, 0 if hidden == 8 else 1))


# ---- 8. the paths agree ----------------------------------------------------------------------------------------------------------------------
def _actor(kind, dev, golden):
    if kind == 'serl50':
        import serl_amd
        w = np.zeros((1, 3716), np.float32)
        w[0, :3715] = golden('actors')['serl50'][18]
        return torch.from_numpy(w).to(dev), serl_amd.NetSpec(7, 3, 32, 3, 'tanh'), 'fused'
    s = _shape(8, 2)
    return torch.from_numpy(np.ascontiguousarray(make_weights(s, 1, 11))).to(dev), spec_of(s), 'fused-general'


def _roll(env, w, spec, K, path):
    return env.rollout(w, K, spec=spec, action_noise='device', noise_sd=SD, noise_clip=CLIP, transitions=True, path=path)


@pytest.mark.parametrize('kind', ['serl50', 'hidden8'])
def test_actor_forward_entry_equals_the_kernels_actions(engine, golden, kind):
    """serl_venv_actor_forward on the observations a fused rollout recorded gives the actions it recorded (no action noise: (double)act)"""
    from serl_amd import _capi
    N = 70
    env = _dev_env(N, 'noise', engine, sensor_noise='device')
    w, spec, path = _actor(kind, env.device, golden)
    w = torch.cat([w, w.flip(1)])                                   # two members
    moe = torch.arange(N, dtype=torch.int32, device=env.device) % 2
    env.reset()
    out = env.rollout(w, STEPS, spec=spec, member_of_env=moe, path='fused')
    assert env.last_rollout_path == path
    fd = _capi.VenvRolloutDesc(state_dim=7, action_dim=3, hidden=spec.hidden, num_layers=spec.num_layers, activation=spec.activation_id, n_members=2,
                               weights=w.data_ptr(), weight_stride=w.stride(0), member_of_env=moe.data_ptr())
    for k in (0, 7, STEPS - 1):
        a = torch.full((N, 3), 9.0, dtype=torch.float32, device=env.device)
        o = out['obs'][k].contiguous()
        assert engine.lib.serl_venv_actor_forward(engine.ctx, ctypes.byref(fd), N, o.data_ptr(), a.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(a.double(), out['actions'][k]), k
    assert out['actions'].abs().max() > 0


@pytest.mark.parametrize('kind', ['serl50', 'hidden8'])
def test_two_segments_equal_one_rollout(engine, golden, kind):
    """rollout(12) then rollout(8) on an identically seeded env equals rollout(20): the action entry is the env's in-episode step, the sensor
    entry k + 1, the ordinal is carried in noise_episode"""
    N = 70
    a, b = (_dev_env(N, 'noise', engine, sensor_noise='device') for _ in range(2))
    w, spec, path = _actor(kind, a.device, golden)
    assert torch.equal(a.reset(), b.reset())
    whole = _roll(a, w, spec, STEPS, 'fused')
    assert a.last_rollout_path == path
    p1 = {k: v.clone() for k, v in _roll(b, w, spec, 12, 'fused').items()}
    p2 = _roll(b, w, spec, 8, 'fused')
    assert torch.equal(p1['obs'][12], p2['obs'][0])
    for key in whole:
        joined = torch.cat([p1[key], p2[key][1:] if key == 'obs' else p2[key]])
        assert torch.equal(whole[key], joined), key
    assert whole['done'].any() and not whole['done'].all() and (whole['actions'].abs() <= 1).all()
    assert torch.equal(a.noise_episode, b.noise_episode) and torch.equal(a._state, b._state)


@pytest.mark.parametrize('kind', ['serl50', 'hidden8'])
def test_fused_equals_loop(engine, golden, kind):
    """path='fused' against path='loop' on identically seeded envs, key for key at zero tolerance (device sensor and action noise).  On a
    device-noise env the step loop runs the kernels' own forward (serl_venv_actor_forward) and takes its addends from serl_venv_noise_fill;
    with torch's forward, as on every other env, the first action already differs by 5.07e-07 (serl50) / 5.96e-08 (hidden8) and the
    closed loop carries that along (measured on an MI355X: actions up to 1.67e-06 / 1.64e-07 apart over these 20 steps).  The figures are
    printed before the assertion."""
    N = 70
    a, b = (_dev_env(N, 'noise', engine, sensor_noise='device') for _ in range(2))
    w, spec, path = _actor(kind, a.device, golden)
    a.reset(); b.reset()
    fused = _roll(a, w, spec, STEPS, 'fused')
    loop = _roll(b, w, spec, STEPS, 'loop')
    assert (a.last_rollout_path, b.last_rollout_path) == (path, 'loop') and fused.keys() == loop.keys()
    for key in fused:
        f, l = _np(fused[key]).astype(np.float64), _np(loop[key]).astype(np.float64)
        print('%s %s: max |fused - loop| = %.3g, differing elements %d of %d' % (kind, key, np.abs(f - l).max(), int((f != l).sum()), f.size))
    for key in fused:
        np.testing.assert_array_equal(_np(fused[key]), _np(loop[key]), err_msg=key)


# ---- 9. no existing behaviour moved ------------------------------------------------------------------------------------------------------------
def test_the_table_path_is_untouched_by_a_device_noise_env_on_the_same_engine(engine):
    import serl_amd
    from serl_amd import builds
    N = 70
    tab = np.stack([builds.sensor_noise_table(6, np.random.RandomState(300 + e)) for e in range(N)])
    acts = _actions(STEPS, N, 3, engine.device)
    s = _shape(32, 3)
    w = torch.from_numpy(np.ascontiguousarray(make_weights(s, 1, 5))).to(engine.device)

    def run():
        env = serl_amd.CitationVecEnv(N, mode='noise', t_max=T_SHORT, refs=_tables(N), engine=engine, auto_reset=True, sensor_noise=tab)
        assert env.noise_seed is None and env.noise_episode is None
        rec = [env.reset().clone()]
        for k in range(8):
            obs, rew, done, info = env.step(acts[k])
            rec += [obs.clone(), rew.clone(), done.clone(), info['x'].clone(), info['episode_return'].clone()]
        out = env.rollout(w, 12, spec=spec_of(s), transitions=True)
        assert env.last_rollout_path == 'fused'
        return rec + [out[k] for k in sorted(out)], env._state.clone()
    before, state0 = run()
    D = _dev_env(N, 'noise', engine, sensor_noise='device')
    D.reset()
    for k in range(8):
        D.step(acts[k])
    D.rollout(w, 12, spec=spec_of(s), action_noise='device', noise_sd=SD, noise_clip=CLIP)
    after, state1 = run()
    assert len(before) == len(after) and torch.equal(state0, state1)
    for x, y in zip(before, after):
        assert torch.equal(x, y)

"""The step-wise vector env on the GPU (C ABI v9 serl_venv_reset / serl_venv_step, serl_amd.CitationVecEnv) against the CPU oracle in its
same-libm flavour, at ZERO tolerance: oracle episodes are flown first (closed loop, traces and transitions), then their f32 actions are
fed to the env step by step and every output of every step must be the oracle's, bit for bit."""
import os, subprocess, sys
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET32 = dict(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation='tanh')
THREADS = 16


def _oracle(*a, **kw):
    from oracle import rollout as R
    return R.rollout(*a, short_libm=True, threads=THREADS, **kw)


def _venv(n, mode, t_max, engine, **kw):
    import serl_amd
    return serl_amd.CitationVecEnv(n, mode=mode, t_max=t_max, engine=engine, **kw)


def _tables(N, t_max, seed):
    """per-env reference tables for an episode of t_max seconds: the first rows of 20 s tables (the short-t_max signals of refsignals
    would blend over a width t_max // 10 = 0)"""
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(N, 2, 20, seed=seed)[:, :rs.n_steps_for(t_max)])
    assert np.isfinite(r).all()
    return r


def _base(t_max):
    from serl_amd import refsignals as rs
    return np.ascontiguousarray(rs.tabulate(*rs.base_reference(20), 20)[:rs.n_steps_for(t_max)])


def _replay(env, o, S, A, reset_kw=None, first_reset=True):
    """Feed the oracle's transitions' f32 actions to `env` (one oracle episode per env) and check every step at zero tolerance."""
    N, T = env.n_envs, o['transitions'].shape[1]
    tr = o['transitions']
    L = o['length_steps']
    assert (L > 0).all()
    dev = env.device
    acts = torch.from_numpy(np.ascontiguousarray(tr[:, :, S:S + A].transpose(1, 0, 2))).to(dev)        # [T, N, A] f32
    obs0 = env.reset(**(reset_kw or {})).cpu().numpy() if first_reset else None
    if obs0 is not None:
        np.testing.assert_array_equal(obs0.astype(np.float32), tr[:, 0, :S])
    Tm = int(L.max()) + 2      # two steps past the last `done`: those envs must be frozen
    rec = {k: torch.zeros((Tm,) + s, dtype=dt, device=dev) for k, s, dt in
           (('obs', (N, S), torch.float64), ('reward', (N,), torch.float64), ('done', (N,), torch.bool), ('x', (N, 12), torch.float64),
            ('ref', (N, 3), torch.float64), ('t', (N,), torch.float64), ('cost', (N,), torch.int32))}
    for k in range(Tm):
        a = acts[k] if k < T else torch.zeros(N, A, dtype=torch.float32, device=dev)
        obs, rew, done, info = env.step(a)
        rec['obs'][k].copy_(obs); rec['reward'][k].copy_(rew); rec['done'][k].copy_(done)
        for key in ('x', 'ref', 't', 'cost'):
            rec[key][k].copy_(info[key])
    rec = {k: v.cpu().numpy() for k, v in rec.items()}
    for e in range(N):
        n = int(L[e])
        np.testing.assert_array_equal(rec['x'][:n, e], o['states'][e, :n], err_msg='env %d: x' % e)
        np.testing.assert_array_equal(rec['reward'][:n, e], o['rewards'][e, :n], err_msg='env %d: reward' % e)
        np.testing.assert_array_equal(rec['obs'][:n, e].astype(np.float32), tr[e, :n, S + A:2 * S + A], err_msg='env %d: next obs' % e)
        np.testing.assert_array_equal(rec['cost'][:n, e], tr[e, :n, 2 * S + A + 2].astype(np.int32), err_msg='env %d: cost' % e)
        d = rec['done'][:, e]
        assert not d[:n - 1].any() and d[n - 1:].all(), 'env %d: done first rises at %d, not %d' % (e, int(np.argmax(d)) + 1, n)
        assert rec['t'][n - 1, e] == o['length_t'][e]
        fit = 0.0
        for r in rec['reward'][:n, e]:
            fit += r
        assert fit == o['fitness'][e], (e, fit, o['fitness'][e])
        # frozen after done: last obs / x / ref / t / cost, reward 0
        for k in range(n, Tm):
            assert rec['reward'][k, e] == 0.0
            for key in ('obs', 'x', 'ref', 't', 'cost'):
                np.testing.assert_array_equal(rec[key][k, e], rec[key][n - 1, e], err_msg='env %d: %s after done' % (e, key))
        # env.last_u: the executed command of the oracle from the f32 action (scale_action in f32 then f64) -- for rate control the
        # observation's tail is last_u itself
        u = o['actions'][e, :n, :A]
        if env.incremental:
            np.testing.assert_array_equal(rec['obs'][:n, e, S - A:], u, err_msg='env %d: last_u' % e)
        else:
            bound = 10.0 * (3.14159265358979323846 / 180.0)
            s = (np.float32(0.5) * (tr[e, :n, S:S + A] + np.float32(1.0))).astype(np.float32)
            np.testing.assert_array_equal(-bound + s.astype(np.float64) * (bound - -bound), u, err_msg='env %d: last_u' % e)
    return rec


# ---- 1. closed-loop oracle episodes replayed, attitude task, every code variant -------------------------------------------------------
VARIANTS = [('nominal', 'h2000_v90', None), ('ice', 'ice', None), ('cg-timed', 'cg_timed', None), ('gust', 'gust', 'noise'),
            ('test', 'test', None), ('noise', 'h2000_v90', 'noise'), ('be', 'h2000_v90', 'be'), ('jr', 'h2000_v90', 'jr'),
            ('sa', 'h2000_v90', 'sa'), ('se', 'h2000_v90', 'se')]


@pytest.mark.parametrize('mode,build,extra', VARIANTS)
def test_replay_of_oracle_episodes_attitude(engine, golden, mode, build, extra):
    from serl_amd import builds, refsignals as rs
    E = 64 if extra in (None, 'noise') else 16
    w = golden('actors')['serl50']
    moe = np.arange(E) % len(w)
    refs = rs.synthetic_reference_tables(E, 3, 20, seed=11 + len(mode))
    T = refs.shape[1]
    kw, env_kw = {}, {}
    if extra == 'noise':
        sn = np.stack([builds.sensor_noise_table(T, np.random.RandomState(100 + e)) for e in range(E)])
        kw['sensor_noise'] = env_kw['sensor_noise'] = sn
    elif extra is not None:
        kw['faults'] = [extra] * E
    o = _oracle(w, NET32, moe, refs, build=build, t_max=20, traces=True, transitions=True, **kw)
    env = _venv(E, mode, 20, engine, refs=refs, **env_kw)
    assert env.build == build and (env.state_dim, env.action_dim) == (7, 3)
    _replay(env, o, 7, 3)


# ---- 2. the other env configurations and rate control, table and generated references ---------------------------------------------
CONFIGS = [('sym', 'PHlab_symmetric_nominal'), ('sym_inc_n', 'PHlab_symmetric_incremental'), ('full', 'PHlab_full_nominal'),
           ('full_inc_n', 'PHlab_full_incremental'), ('att_inc', 'PHlab_attitude_incremental')]


@pytest.mark.parametrize('refkind', ['table', 'spec'])
@pytest.mark.parametrize('case,name', CONFIGS)
def test_replay_of_oracle_episodes_configurations(engine, golden, case, name, refkind):
    from serl_amd import builds, refsignals as rs
    from test_oracle_rollout import config_case
    g = golden('config')
    cfg, incr, net, _, _, _ = config_case(g, case)
    assert builds.env_config(name) == (cfg, bool(incr))
    S, A = net['state_dim'], net['action_dim']
    E = 24
    rng = np.random.default_rng(5)
    w = np.repeat(g[case + '_w'][None], E, 0)
    w[1:] += rng.normal(0, 0.05, w[1:].shape).astype(np.float32)
    if refkind == 'table':
        refs = rs.synthetic_reference_tables(E, 2, 20, seed=21)
        if A == 1:
            refs[:, :, 1:] = 0.0
    else:
        refs = rs.ref_specs(*rs.training_references(E, 20, np.random.RandomState(8), n_actions=A), 0.2106 if A == 3 else 0.22)
    o = _oracle(w, net, np.arange(E), refs, t_max=20, traces=True, transitions=True, env_config=cfg, incremental=incr)
    env = _venv(E, name, 20, engine, refs=refs)
    assert (env.state_dim, env.action_dim) == (S, A)
    _replay(env, o, S, A)


# ---- 3. f64 actions (outside [-1, 1] too) against the open-loop dynamics and the env glue restated in tests/env_glue.py ----------------
@pytest.mark.parametrize('mode', ['PHlab_attitude_nominal', 'PHlab_attitude_incremental'])
def test_f64_actions_against_the_dynamics(engine, mode):
    import env_glue as G
    from serl_amd import refsignals as rs
    N, t_max = 6, 3.0
    T = rs.n_steps_for(t_max)
    refs = _tables(N, t_max, 3)
    rng = np.random.default_rng(17)
    acts = rng.uniform(-1.25, 1.25, (T + 3, N, 3)) * np.array([0.3, 0.2, 0.2])
    acts[:, 0] *= 4.0       # env 0: far outside [-1, 1] (not clipped by the env)
    env = _venv(N, mode, t_max, engine, refs=refs)
    incr = env.incremental
    obs0 = env.reset().cpu().numpy()
    out = []
    for k in range(T + 3):
        obs, rew, done, info = env.step(torch.from_numpy(acts[k]).to(env.device))
        out.append([obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), info['x'].cpu().numpy(), info['t'].cpu().numpy(),
                    info['cost'].cpu().numpy()])
    for e in range(N):
        py = G.GlueEnv('h2000_v90', G.ATTITUDE, incr, None, refs[e], None, t_max)      # the literal Python env (tests/env_glue.py)
        np.testing.assert_array_equal(obs0[e], np.array(py.reset()))
        n = None
        for k in range(T + 3):
            o_, r_, d_, x_, t_, c_ = (v[e] for v in out[k])
            if n is not None:       # frozen
                assert d_ and r_ == 0.0 and t_ == py.t
                continue
            r = py.step(np.asarray(acts[k, e], dtype=np.float64))
            np.testing.assert_array_equal(x_, np.array(r['x']), err_msg='env %d step %d' % (e, k))
            np.testing.assert_array_equal(o_, np.array(r['obs']), err_msg='env %d step %d' % (e, k))
            assert r_ == r['reward'] and c_ == r['cost'] and t_ == r['t'], (e, k, r_, r['reward'])
            assert bool(d_) == (r['fin'] or k + 1 >= T), (e, k)
            if d_:
                n = k + 1
        assert n is not None


# ---- 4. re-used envs: three episodes each, partial resets, the carried error and model clock ----------------------------------------
@pytest.mark.parametrize('mode,build', [('cg-timed', 'cg_timed'), ('gust', 'gust')])
def test_reuse_of_envs_with_partial_resets(engine, golden, mode, build):
    from serl_amd import builds, refsignals as rs
    N, t_max, EPIS = 16, 3.0, 3
    w = golden('actors')['serl50']
    T = rs.n_steps_for(t_max)
    noisy = builds.has_sensor_noise(mode)
    refs = [_tables(N, t_max, 30 + j) for j in range(EPIS)]
    sn = [np.stack([builds.sensor_noise_table(T, np.random.RandomState(1000 * j + e)) for e in range(N)]) if noisy else None
          for j in range(EPIS)]
    # the oracle first: episode j of env i starts from the error and the clock episode j - 1 left (one tick per reset, one per step)
    err0, tick0, orc = np.zeros((N, 3)), np.zeros(N, np.int64), []
    for j in range(EPIS):
        moe = (np.arange(N) * 3 + j) % len(w)
        kw = dict(sensor_noise=sn[j]) if noisy else {}
        o = _oracle(w, NET32, moe, refs[j], build=build, t_max=t_max, traces=True, transitions=True, err0=err0, tick0=tick0, **kw)
        orc.append(o)
        L = o['length_steps']
        assert (L > 0).all()
        for i in range(N):
            err0[i] = refs[j][i, L[i] - 1] - o['states'][i, L[i] - 1][[7, 6, 5]]
        tick0 = tick0 + 1 + L
    env = _venv(N, mode, t_max, engine, refs=refs[0], **(dict(sensor_noise=sn[0]) if noisy else {}))
    dev = env.device
    start = np.where(np.arange(N) % 2 == 0, 0, 41)        # odd envs start 41 steps later: every later reset is a partial one
    epi = np.full(N, -1)
    k = np.zeros(N, np.int64)
    got = [[dict(x=[], r=[], o=[]) for _ in range(N)] for _ in range(EPIS)]
    for step in range(10 * T):
        due = np.array([(epi[i] < 0 and step == start[i]) or (epi[i] >= 0 and epi[i] < EPIS - 1 and k[i] >= orc[epi[i]]['length_steps'][i])
                        for i in range(N)])
        if due.any():
            idx = np.nonzero(due)[0]
            epi[idx] += 1
            k[idx] = 0
            j_of = epi[idx]
            rr = np.stack([refs[j][i] for i, j in zip(idx, j_of)])
            kw = dict(sensor_noise=np.stack([sn[j][i] for i, j in zip(idx, j_of)])) if noisy else {}
            obs = env.reset(torch.from_numpy(due).to(dev), refs=rr, **kw).cpu().numpy()
            for i, j in zip(idx, j_of):
                np.testing.assert_array_equal(obs[i].astype(np.float32), orc[j]['transitions'][i, 0, :7], err_msg='obs0 env %d episode %d' % (i, j))
        if (epi == EPIS - 1).all() and all(k[i] >= orc[EPIS - 1]['length_steps'][i] for i in range(N)):
            break
        a = np.zeros((N, 3), np.float32)
        for i in range(N):
            if epi[i] >= 0 and k[i] < orc[epi[i]]['length_steps'][i]:
                a[i] = orc[epi[i]]['transitions'][i, k[i], 7:10]
        obs, rew, done, info = env.step(torch.from_numpy(a).to(dev))
        obs, rew, x = obs.cpu().numpy(), rew.cpu().numpy(), info['x'].cpu().numpy()
        for i in range(N):
            if epi[i] >= 0 and k[i] < orc[epi[i]]['length_steps'][i]:
                g = got[epi[i]][i]
                g['x'].append(x[i]); g['r'].append(rew[i]); g['o'].append(obs[i])
                k[i] += 1
    for j in range(EPIS):
        o = orc[j]
        for i in range(N):
            n = int(o['length_steps'][i])
            g = got[j][i]
            assert len(g['r']) == n, (j, i)
            np.testing.assert_array_equal(np.array(g['x']), o['states'][i, :n], err_msg='env %d episode %d: x' % (i, j))
            np.testing.assert_array_equal(np.array(g['r']), o['rewards'][i, :n], err_msg='env %d episode %d: reward' % (i, j))
            np.testing.assert_array_equal(np.array(g['o']).astype(np.float32), o['transitions'][i, :n, 10:17])


# ---- 5. an env's results do not depend on the batch around it, nor on the process -------------------------------------------------
def _batch_outputs(engine, N, pos, acts_i, t_max=3.0, seed=0):
    env = _venv(N, 'nominal', t_max, engine, refs=_base(t_max))
    g = torch.Generator(device='cpu').manual_seed(seed)
    out = []
    env.reset()
    for k in range(len(acts_i)):
        a = torch.rand(N, 3, generator=g, dtype=torch.float32) * 2 - 1
        a[pos] = torch.from_numpy(acts_i[k])
        obs, rew, done, info = env.step(a.to(env.device))
        out.append(np.concatenate([obs[pos].cpu().numpy(), rew[pos:pos + 1].cpu().numpy(), info['x'][pos].cpu().numpy(),
                                   done[pos:pos + 1].cpu().numpy().astype(np.float64)]))
    return np.stack(out)


def test_independence_of_the_batch(engine):
    rng = np.random.default_rng(2)
    acts = (rng.uniform(-1, 1, (301, 3)) * 0.4).astype(np.float32)
    alone = _batch_outputs(engine, 1, 0, acts)
    for N, pos in ((4096, 0), (4096, 4095), (4096, 1234), (300, 77)):
        np.testing.assert_array_equal(_batch_outputs(engine, N, pos, acts, seed=N + pos), alone, err_msg='N %d position %d' % (N, pos))


DIGEST_SCRIPT = r'''
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import serl_amd
from serl_amd import refsignals as rs
N, t_max = 4096, 20.0
specs = rs.ref_specs(*rs.training_references(N, t_max, np.random.RandomState(5)), 0.2106)
env = serl_amd.CitationVecEnv(N, mode='gust', t_max=t_max, refs=specs, sensor_noise=False)
g = torch.Generator(device='cpu').manual_seed(9)
h = hashlib.sha256()
h.update(env.reset().cpu().numpy().tobytes())
for k in range(rs.n_steps_for(2.0)):
    obs, rew, done, info = env.step((torch.rand(N, 3, generator=g, dtype=torch.float64) * 2 - 1).to(env.device))
    for v in (obs, rew, done, info['x'], info['t'], info['cost']):
        h.update(v.cpu().numpy().tobytes())
print('DIGEST', h.hexdigest())
'''


def test_two_processes_give_identical_digests(engine):
    digests = []
    for _ in range(2):
        r = subprocess.run([sys.executable, '-c', DIGEST_SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        digests.append([l for l in r.stdout.splitlines() if l.startswith('DIGEST')][0])
    assert digests[0] == digests[1], digests


# ---- 6. frozen done envs, the end of the tables, bad arguments --------------------------------------------------------------------
def test_done_envs_are_frozen_and_the_tables_are_not_read_past_their_end(engine):
    from serl_amd import builds, refsignals as rs
    t_max = 0.5
    T = rs.n_steps_for(t_max)
    dev = engine.device
    # the table of a single env, followed in memory by NaN rows: a read past max_steps would show in reward / obs
    big = torch.full((1, T + 4, 3), float('nan'), dtype=torch.float64, device=dev)
    big[0, :T] = torch.from_numpy(_base(t_max)).to(dev)
    nbig = torch.full((1, T + 4, 7), float('nan'), dtype=torch.float64, device=dev)
    nbig[0, :T + 1] = torch.from_numpy(builds.sensor_noise_table(T, np.random.RandomState(1))).to(dev)
    ref, noise = big[:, :T], nbig[:, :T + 1]
    assert ref.is_contiguous() and noise.is_contiguous()
    env = _venv(1, 'noise', t_max, engine, refs=ref, sensor_noise=noise)
    assert env._ref.data_ptr() == big.data_ptr() and env._noise.data_ptr() == nbig.data_ptr()
    env.reset()
    a = torch.zeros(1, 3, dtype=torch.float32, device=dev)
    rows = []
    for k in range(T + 10):
        obs, rew, done, info = env.step(a)
        rows.append((obs.cpu().numpy().copy(), float(rew[0]), bool(done[0]), info['x'].cpu().numpy().copy(), float(info['t'][0]),
                     info['ref'].cpu().numpy().copy()))
    first = [k for k, r in enumerate(rows) if r[2]][0]
    assert first == T - 1                                  # flown to t_max: done at the last row of the table
    assert rows[first][4] == rs.env_times(T + 1)[T]
    for r in rows:
        assert np.isfinite(r[0]).all() and np.isfinite(r[1]) and np.isfinite(r[3]).all() and np.isfinite(r[5]).all()
    for r in rows[first + 1:]:
        assert r[2] and r[1] == 0.0 and r[4] == rows[first][4]
        np.testing.assert_array_equal(r[0], rows[first][0]); np.testing.assert_array_equal(r[3], rows[first][3])
    # a shorter table than t_max needs: done when it ends, frozen behind it
    env2 = _venv(1, 'nominal', 3.0, engine, refs=big[0, :20])
    env2.reset()
    d = [bool(env2.step(a)[2][0]) for _ in range(25)]
    assert d.index(True) == 19 and all(d[19:])
    assert np.isfinite(env2._obs.cpu().numpy()).all()
    # a never-reset env is not running: done, reward 0
    env3 = _venv(3, 'nominal', 20, engine)
    obs, rew, done, _ = env3.step(torch.zeros(3, 3, device=dev))
    assert done.all() and (rew == 0).all()
    # reset of a subset: the others keep running
    env3.reset()
    for _ in range(5):
        env3.step(torch.zeros(3, 3, device=dev))
    before = env3._obs.clone()
    obs = env3.reset(torch.tensor([False, True, False], device=dev))
    np.testing.assert_array_equal(obs[[0, 2]].cpu().numpy(), before[[0, 2]].cpu().numpy())
    assert not env3.step(torch.zeros(3, 3, device=dev))[2].any()


def test_bad_arguments(engine):
    import ctypes
    from serl_amd import _capi
    dev = engine.device
    env = _venv(8, 'PHlab_symmetric_nominal', 20, engine)
    env.reset()
    with pytest.raises(ValueError):
        env.step(torch.zeros(8, 3, device=dev))                       # symmetric: one action
    with pytest.raises(ValueError):
        env.step(torch.zeros(8, 1, device=dev, dtype=torch.int32))
    with pytest.raises(ValueError):
        env.step(torch.zeros(8, 1))                                   # host tensor
    with pytest.raises(ValueError):
        env.reset(torch.zeros(7, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        _venv(0, 'nominal', 1.0, engine)
    L, ctx = engine.lib, engine.ctx
    obs = torch.zeros(8, 2, dtype=torch.float64, device=dev)
    good = _capi.VenvDesc.from_buffer_copy(env.desc)
    assert L.serl_venv_reset(ctx, ctypes.byref(good), None, obs.data_ptr(), None) == 0
    torch.cuda.synchronize()
    for field, value in (('state_dim', 7), ('action_dim', 3), ('env_config', 3), ('build_slot', -1), ('state', None), ('n_envs', 0),
                         ('max_steps', 0), ('t_max', 0.0), ('ref_spec', None), ('ref_spec_stride', 2)):
        d = _capi.VenvDesc.from_buffer_copy(env.desc)
        setattr(d, field, value)
        assert L.serl_venv_reset(ctx, ctypes.byref(d), None, obs.data_ptr(), None) == -1, field
        assert L.serl_venv_step(ctx, ctypes.byref(d), obs.data_ptr(), 1, obs.data_ptr(), obs.data_ptr(), obs.data_ptr(), None, None, None,
                                None, None) == -1, field
    assert L.serl_venv_step(ctx, ctypes.byref(good), obs.data_ptr(), 2, obs.data_ptr(), obs.data_ptr(), obs.data_ptr(), None, None, None,
                            None, None) == -1
    assert L.serl_venv_step(ctx, ctypes.byref(good), None, 0, obs.data_ptr(), obs.data_ptr(), obs.data_ptr(), None, None, None,
                            None, None) == -1
    assert L.serl_venv_reset(ctx, ctypes.byref(good), None, None, None) == -1

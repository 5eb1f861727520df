"""serl_td3_train -- a chain of TD3 updates in one launch -- against the float64 contract of tests/td3_64.py over a covering grid of
shapes and schedules, and its invariants: n_updates = 0, two calls against one, several learners in one launch, what it may read and
write, refusals, TD3.train on the fused path."""
import ctypes
import functools
import random
import types
import numpy as np
import pytest
import torch
import td3_64 as T

pytestmark = pytest.mark.gpu
ACT = {'tanh': 0, 'elu': 1, 'relu': 2}


@functools.lru_cache(maxsize=None)
def _case(c, seed=None):
    d = T.make_case(c, seed)
    return d, T.td3_literal(d)


class Launch:
    """device buffers of K learners of one shape and one serl_td3_train call on rows 1 .. K of every per-learner array (row 0 and row
    K + 1 are guards); strides leave extra columns behind every row"""

    def __init__(self, engine, cases, n=None, extra=5, nan_pad=True, steps0=(0, 0)):
        from serl_amd import _capi
        self.L = _capi.lib()
        self.engine, self.cases = engine, cases
        d0 = cases[0]
        K = self.K = len(cases)
        S, A, B = d0['S'], d0['A'], d0['B']
        self.n = d0['n'] if n is None else n
        n_all = d0['n']
        self.Pa, self.Pc = len(d0['actor']), len(d0['critic'])
        assert self.Pc == self.L.serl_td3_param_count(S, A)
        dev = self.dev = engine.device
        self.sa, self.sc = self.Pa + extra, self.Pc + extra
        host = {}
        for k, P, st in (('actor', self.Pa, self.sa), ('actor_target', self.Pa, self.sa), ('actor_m', self.Pa, self.sa), ('actor_v', self.Pa, self.sa),
                         ('critic', self.Pc, self.sc), ('critic_target', self.Pc, self.sc), ('critic_m', self.Pc, self.sc), ('critic_v', self.Pc, self.sc)):
            a = np.full((K + 2, st), 7.25, np.float32)
            for i, d in enumerate(cases):
                a[1 + i, :P] = d[k] if k in d else 0.0
            host[k] = a
        W = 2 * S + A + 3
        cap = T.RING_ROWS + 1                       # the last ring row is NaN: every unused slot column names it
        ring = np.full((K, cap, W), np.nan, np.float32)
        cols = B + 3
        slots = np.full((K, n_all, cols), cap - 1, np.int32)
        tn = np.zeros((K, n_all, B, A), np.float32)
        cn = np.zeros((K, max(d0['n_actor'], 1), B, S), np.float32)
        for i, d in enumerate(cases):
            ring[i, :T.RING_ROWS] = d['ring']
            slots[i, :, :B] = d['slots']
            tn[i] = d['tn']
            if d['caps']:
                cn[i, :d['n_actor']] = d['cn']
        host.update(ring=ring, slots=slots, tn=tn, cn=cn)
        host['steps'] = np.tile(np.array(steps0, np.int32), (K + 2, 1))
        host['td'] = np.full((K + 2, n_all + 2), -3.5, np.float32)
        host['pg'] = np.full((K + 2, n_all + 2), -3.5, np.float32)
        self.host = host
        self.t = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
        self.wb = int(self.L.serl_td3_work_bytes(K, S, A, d0['H'], d0['L'], B))
        assert self.wb > 0
        self.work = torch.full((self.wb // 4 + 8,), float('nan'), dtype=torch.float32, device=dev)

    def desc(self, n, it0, u0=0, k0=0, first=0, K=None):
        """descriptor of n updates starting at update u0 (actor update k0) of the tables, for learners first .. first + K"""
        from serl_amd import _capi
        d0, t = self.cases[0], self.t
        K = self.K if K is None else K
        p = lambda x, *idx: x[idx].data_ptr()
        return _capi.Td3Desc(
            state_dim=d0['S'], action_dim=d0['A'], hidden=d0['H'], num_layers=d0['L'], activation=ACT[d0['act']], n_learners=K, batch=d0['B'],
            n_updates=n, capacity=t['ring'].shape[1], slot_cols=t['slots'].shape[2], policy_update_freq=d0['freq'], iteration0=it0,
            update_actor_target=int(d0['uat']), lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP,
            lambda_s=T.CAPS['lambda_s'], lambda_t=T.CAPS['lambda_t'], eps_sd=T.CAPS['eps_sd'], max_grad_norm=T.MAX_NORM,
            actor=p(t['actor'], 1 + first), actor_target=p(t['actor_target'], 1 + first), actor_m=p(t['actor_m'], 1 + first),
            actor_v=p(t['actor_v'], 1 + first), actor_stride=self.sa, critic=p(t['critic'], 1 + first),
            critic_target=p(t['critic_target'], 1 + first), critic_m=p(t['critic_m'], 1 + first), critic_v=p(t['critic_v'], 1 + first),
            critic_stride=self.sc, adam_steps=p(t['steps'], 1 + first), ring=p(t['ring'], first), ring_stride=t['ring'].stride(0),
            slots=p(t['slots'], first, u0), slots_stride=t['slots'].stride(0), target_noise=p(t['tn'], first, u0), noise_stride=t['tn'].stride(0),
            caps_noise=p(t['cn'], first, k0) if d0['caps'] else None, caps_stride=t['cn'].stride(0), td_loss=p(t['td'], 1 + first, u0),
            pg_loss=p(t['pg'], 1 + first, u0), loss_stride=t['td'].stride(0), work=self.work.data_ptr(), work_bytes=self.wb)

    def run(self, **kw):
        d0 = self.cases[0]
        kw.setdefault('n', self.n)
        kw.setdefault('it0', d0['it0'])
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        rc = self.L.serl_td3_train(self.engine.ctx, ctypes.byref(self.desc(**kw)), stream)
        torch.cuda.synchronize()
        return rc

    def out(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def result(self, o, i):
        """learner i of out() as the dict td3_64.check takes"""
        r = {k: o[k][1 + i, :(self.Pa if k.startswith('actor') else self.Pc)] for k in T.ROWS + T.MOMENTS}
        n = self.cases[0]['n']
        r['td'], r['pg'] = o['td'][1 + i, :n], o['pg'][1 + i, :n]
        return r

    def assert_guards(self, o, n=None):
        """columns past the rows, the guard learners, loss entries from n on, pg entries of non-actor updates: as given"""
        h, d0 = self.host, self.cases[0]
        n = self.n if n is None else n
        for k in T.ROWS + T.MOMENTS:
            P = self.Pa if k.startswith('actor') else self.Pc
            np.testing.assert_array_equal(o[k][:, P:], h[k][:, P:], err_msg=k)
            np.testing.assert_array_equal(o[k][[0, -1]], h[k][[0, -1]], err_msg=k)
        for k in ('td', 'pg'):
            np.testing.assert_array_equal(o[k][:, n:], h[k][:, n:], err_msg=k)
            np.testing.assert_array_equal(o[k][[0, -1]], h[k][[0, -1]], err_msg=k)
        np.testing.assert_array_equal(o['steps'][[0, -1]], h['steps'][[0, -1]])
        for u in range(n):
            if (d0['it0'] + u + 1) % d0['freq'] != 0:
                assert (o['pg'][1:-1, u] == -3.5).all(), u
            else:
                assert (o['pg'][1:-1, u] != -3.5).all(), u
        for k in ('ring', 'slots', 'tn', 'cn'):
            np.testing.assert_array_equal(o[k], h[k], err_msg=k)


@pytest.mark.parametrize('c', T.CASES, ids=T.case_id)
def test_td3_kernel_vs_float64(engine, c):
    """one learner per case of the grid: rows, targets, moments, td_loss[0] and the first pg_loss against the float64 run; the norm clip
    is active in every critic step of a 'big' case and in none of a 'small' one; NaN ring rows and unused slot columns are never read"""
    d, ref = _case(c)
    assert all(ref['clip_c']) if d['rew'] == 'big' else not any(ref['clip_c']), ref['clip_c']
    la = Launch(engine, [d])
    assert la.run() == 0
    o = la.out()
    T.check(la.result(o, 0), ref, d, T.case_id(c))
    la.assert_guards(o)
    n_act = d['n_actor']
    np.testing.assert_array_equal(o['steps'][1], [d['n'], n_act])
    got = la.result(o, 0)
    np.testing.assert_allclose(got['td'], ref['td'], rtol=2e-3, atol=1e-5)


def test_td3_zero_updates_is_a_noop(engine):
    d, _ = _case(T.CASES[0])
    la = Launch(engine, [d], n=0)
    assert la.run() == 0
    o = la.out()
    for k, v in la.host.items():
        np.testing.assert_array_equal(o[k], v, err_msg=k)


@pytest.mark.parametrize('c', [T.CASES[0], T.CASES[2]], ids=T.case_id)
def test_td3_two_calls_equal_one(engine, c):
    """n1 updates, then the remaining ones with iteration0 advanced and the Adam counts carried: bit for bit the single call"""
    d, _ = _case(c)
    one = Launch(engine, [d])
    assert one.run() == 0
    a = one.out()
    n1 = 7
    k1 = sum(1 for u in range(n1) if (d['it0'] + u + 1) % d['freq'] == 0)
    two = Launch(engine, [d])
    assert two.run(n=n1) == 0
    assert two.run(n=d['n'] - n1, it0=d['it0'] + n1, u0=n1, k0=k1) == 0
    b = two.out()
    for k in T.ROWS + T.MOMENTS + ('td', 'pg', 'steps'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_td3_three_learners_equal_three_launches(engine):
    """three learners (different rows, rings, draws) in one launch against one launch each, bit for bit; each within the bound"""
    c = T.CASES[10]
    cases = [_case(c, seed)[0] for seed in (None, 21, 22)]
    la = Launch(engine, cases)
    assert la.run() == 0
    o = la.out()
    la.assert_guards(o)
    for i, d in enumerate(cases):
        T.check(la.result(o, i), _case(c, (None, 21, 22)[i])[1], d, 'learner %d' % i)
        solo = Launch(engine, cases)
        assert solo.run(first=i, K=1) == 0
        s = solo.out()
        for k in T.ROWS + T.MOMENTS + ('td', 'pg', 'steps'):
            np.testing.assert_array_equal(s[k][1 + i], o[k][1 + i], err_msg='%s learner %d' % (k, i))
            others = [j for j in range(5) if j != 1 + i]
            np.testing.assert_array_equal(s[k][others], solo.host[k][others], err_msg=k)


def test_td3_refusals(engine):
    """shapes outside the compiled range: SERL_E_UNSUPPORTED, work_bytes 0, nothing written; bad arguments: SERL_E_INVALID"""
    from serl_amd import _capi
    d, _ = _case(T.CASES[3])
    la = Launch(engine, [d])
    L = la.L
    stream = ctypes.c_void_p(torch.cuda.current_stream(la.dev).cuda_stream)
    for field, v in (('hidden', 132), ('hidden', 6), ('num_layers', 5), ('state_dim', 17), ('action_dim', 5), ('batch', 129)):
        desc = la.desc(la.n, d['it0'])
        setattr(desc, field, v)
        desc.slot_cols = 200
        assert L.serl_td3_train(engine.ctx, ctypes.byref(desc), stream) == _capi.E_UNSUPPORTED, field
    assert L.serl_td3_work_bytes(1, 7, 3, 132, 3, 86) == 0 and L.serl_td3_work_bytes(1, 7, 3, 72, 3, 129) == 0
    for field, v in (('actor', None), ('slots', None), ('work', None), ('n_updates', -1), ('policy_update_freq', 0), ('activation', 3),
                     ('capacity', 0), ('n_learners', 0), ('work_bytes', 16), ('slot_cols', 2), ('lr', 0.0), ('tau', 1.5)):
        desc = la.desc(la.n, d['it0'])
        setattr(desc, field, v)
        assert L.serl_td3_train(engine.ctx, ctypes.byref(desc), stream) == _capi.E_INVALID, field
    torch.cuda.synchronize()
    o = la.out()
    for k, v in la.host.items():
        np.testing.assert_array_equal(o[k], v, err_msg=k)


def _args(S, A, H, L, act, B, dev, caps=True):
    return types.SimpleNamespace(state_dim=S, action_dim=A, hidden_size=H, num_layers=L, activation_actor=act, device=dev, individual_bs=400,
                                 lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP, policy_update_freq=2,
                                 use_caps=caps, batch_size=B)


def test_td3_train_fused_path_and_fallback(engine):
    """TD3.train on a device ring takes the fused path and agrees with the eager loop on the same draws (both f32: twice the bound
    apart); a shape the kernel is not compiled for (hidden 130) falls back to the eager loop"""
    import serl_amd
    from serl_amd.actor import pack_actor, pack_critic
    dev = engine.device
    d, _ = _case(T.CASES[0])
    res = {}
    for fused in (True, False):
        torch.manual_seed(5)
        t = serl_amd.TD3(_args(7, 3, 72, 3, 'tanh', 86, 'cpu'), engine)
        ring = serl_amd.DeviceReplay(400, dev, engine, 7, 3)
        ring.append_rows(torch.from_numpy(d['ring']))
        w0 = pack_actor(t.actor).numpy().astype(np.float64), pack_critic(t.critic).numpy().astype(np.float64)
        out = t.train(ring, 14, iteration0=3, rng=random.Random(3), generator=torch.Generator().manual_seed(9), fused=fused)
        assert t.last_path == ('fused' if fused else 'eager')
        res[fused] = (pack_actor(t.actor).numpy().astype(np.float64), pack_critic(t.critic).numpy().astype(np.float64), out, w0)
    for k, name in ((0, 'actor'), (1, 'critic')):
        moved = np.abs(res[False][k] - res[False][3][k]).max()
        assert moved > T.MIN_MOVED
        err = np.abs(res[True][k] - res[False][k]).max()
        print('TD3_TRAIN %s |fused - eager| %.3g moved %.4f' % (name, err, moved))
        assert err <= 2 * T.TOL_REL['tanh'] * moved + T.TOL_ABS
    assert abs(res[True][2]['TD_loss'] - res[False][2]['TD_loss']) <= 1e-3 * abs(res[False][2]['TD_loss']) + 1e-6
    t = serl_amd.TD3(_args(7, 3, 130, 1, 'tanh', 16, 'cpu'), engine)
    ring = serl_amd.DeviceReplay(400, dev, engine, 7, 3)
    ring.append_rows(torch.from_numpy(d['ring']))
    assert not t.fused_supported(dev)
    out = t.train(ring, 3, iteration0=0, rng=random.Random(1), generator=torch.Generator().manual_seed(1))
    assert t.last_path == 'eager' and np.isfinite(out['TD_loss'])


def test_td3_golden_chain_on_the_kernel(engine, golden):
    """the chains the reference's own TD3 ran (tests/golden/td3_update.npz) once on the kernel"""
    g = golden('td3_update')
    for tag in ('a', 'b'):
        d, ref = golden_case(g, tag)
        la = Launch(engine, [d])
        assert la.run() == 0
        o = la.out()
        got = la.result(o, 0)
        dev, moved = T.deviations({k: got[k] for k in T.ROWS + T.MOMENTS}, dict(ref, **{k: got[k] for k in T.MOMENTS}), d)
        print('TD3_GOLDEN %s %s' % (tag, {k: '%.2g' % dev[k] for k in T.ROWS}))
        for k in T.ROWS:
            assert dev[k] <= 2 * T.TOL_REL[d['act']] + T.TOL_ABS / moved[k.split('_')[0]], (tag, k, dev[k])
        np.testing.assert_allclose(got['td'], ref['td'], rtol=5e-3, atol=1e-5)


def golden_case(g, tag):
    """a case dict (td3_64.make_case's keys) and the reference's results from the golden arrays of one chain"""
    S, A, H, L, B, freq, it0, n, caps, uat, act_id = (int(x) for x in g[tag + '_shape'])
    act = ('tanh', 'elu', 'relu')[act_id]
    pg = g[tag + '_pg'].astype(np.float64)
    d = dict(S=S, A=A, H=H, L=L, act=act, B=B, freq=freq, it0=it0, n=n, caps=bool(caps), uat=bool(uat), rew='golden',
             n_actor=int((~np.isnan(pg)).sum()), actor=g[tag + '_actor0'], actor_target=g[tag + '_actor_target0'], critic=g[tag + '_critic0'],
             critic_target=g[tag + '_critic_target0'], ring=g[tag + '_ring'], slots=g[tag + '_slots'], tn=g[tag + '_tn'],
             cn=g[tag + '_cn'] if caps else None)
    ref = {k: g[tag + '_' + k].astype(np.float64) for k in T.ROWS}
    ref.update(td=g[tag + '_td'].astype(np.float64), pg=pg)
    return d, ref

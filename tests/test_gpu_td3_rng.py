"""serl_td3_train_rng -- the fused TD3 learner with its minibatch slots and its noise drawn inside the kernel (csrc/serl_rng.h) -- against
serl_td3_train / serl_td3_train_mfma fed the tables serl_td3_rng_fill writes for the same (seed, learner, iteration), bit for bit in every
array the kernels write; split and learner invariance; what the fill kernel writes against the host's restatement of the generator;
refusals; TD3.train(draws='device') against a twin learner on the host path with the replayed draws."""
import ctypes
import functools
import random
import numpy as np
import pytest
import torch
import td3_64 as T
import test_gpu_td3 as G

pytestmark = pytest.mark.gpu
OUT = T.ROWS + T.MOMENTS + ('td', 'pg', 'steps')
SEED = 0x9E3779B97F4A7C15
N = 6
# (S, A, B, n_rows, capacity): the default minibatch in a part-filled ring; the smallest of everything; a full ring drawn whole (a permutation,
# both halves of the slot wavefront full); one sample past a multiple of 16 in a small ring (many Floyd collisions); one past 32 in a big one
SHAPES = [(7, 3, 86, 300, 512), (1, 1, 1, 1, 1), (16, 4, 128, 128, 128), (5, 2, 17, 40, 64), (7, 3, 33, 1000, 1000)]
# (caps, policy_update_freq, iteration0): freq 2 from 0 (actor updates at u = 1, 3, 5) and from 1 (u = 0, 2, 4: the CAPS block index starts
# at the first update); CAPS off; every update an actor update; every third
SCHEDULES = [(1, 2, 0), (1, 2, 1), (0, 2, 0), (1, 1, 0), (1, 3, 0)]


@functools.lru_cache(maxsize=None)
def _weights(S, A, H, B):
    return T.make_case((S, A, H, 1, 'tanh', B, 2, 0, 6, 1, 1, 'small'))


@functools.lru_cache(maxsize=None)
def _ring(S, A, n_rows, capacity):
    """rows [0, n_rows) like td3_64.make_case's ring; NaN from n_rows on: a slot outside the filled part shows in every output"""
    rng = np.random.default_rng(1000 * S + 100 * A + n_rows)
    ring = np.full((capacity, 2 * S + A + 3), np.nan, np.float32)
    st = rng.standard_normal((n_rows, S)) * rng.uniform(0.3, 1.5, S)
    ring[:n_rows, :S] = st
    ring[:n_rows, S:S + A] = rng.uniform(-1, 1, (n_rows, A))
    ring[:n_rows, S + A:2 * S + A] = st + 0.1 * rng.standard_normal((n_rows, S))
    ring[:n_rows, 2 * S + A] = (-0.5 + 0.4 * rng.standard_normal(n_rows)) * 0.1
    ring[:n_rows, 2 * S + A + 1] = rng.random(n_rows) < 0.15
    ring[:n_rows, 2 * S + A + 2] = rng.random(n_rows) < 0.3
    return ring


class Launch:
    """device buffers of K learners of one shape on one shared ring, rows 1 .. K of every per-learner array (row 0 and row K + 1 are
    guards), and calls of the generator entry and of the table entries on them"""

    def __init__(self, engine, shape, H, K=1, n=N):
        from serl_amd import _capi
        self.C, self.L, self.engine, self.dev = _capi, _capi.lib(), engine, engine.device
        self.S, self.A, self.B, self.n_rows, self.cap = shape
        self.H, self.K, self.n = H, K, n
        S, A, B = self.S, self.A, self.B
        host = {}
        for i in range(K):
            d = _weights(S, A, H, B) if i == 0 else T.make_case((S, A, H, 1, 'tanh', B, 2, 0, 6, 1, 1, 'small'), seed=40 + i)
            for k in T.ROWS + T.MOMENTS:
                P = len(d[k.split('_')[0]])
                host.setdefault(k, np.full((K + 2, P + 5), 7.25, np.float32))[1 + i, :P] = d[k] if k in d else 0.0
        self.Pa, self.Pc = len(d['actor']), len(d['critic'])
        host['ring'] = _ring(S, A, self.n_rows, self.cap)
        host['steps'] = np.zeros((K + 2, 2), np.int32)
        host['td'] = np.full((K + 2, n + 2), -3.5, np.float32)
        host['pg'] = np.full((K + 2, n + 2), -3.5, np.float32)
        self.host = host
        self.t = {k: torch.from_numpy(v).to(self.dev) for k, v in host.items()}
        self.wb = int(self.L.serl_td3_work_bytes(K, S, A, H, 1, B))
        assert self.wb > 0
        self.work = torch.full((self.wb // 4 + 8,), float('nan'), dtype=torch.float32, device=self.dev)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def desc(self, n, it0, freq, u0=0, first=0, K=None, tables=None):
        t = self.t
        K = self.K if K is None else K
        p = lambda x, *idx: x[idx].data_ptr()
        sl, tn, cn = tables if tables is not None else (None, None, None)
        return self.C.Td3Desc(
            state_dim=self.S, action_dim=self.A, hidden=self.H, num_layers=1, activation=0, n_learners=K, batch=self.B, n_updates=n,
            capacity=self.cap, slot_cols=self.B if tables is not None else 0, policy_update_freq=freq, iteration0=it0, update_actor_target=1, lr=T.LR,
            gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP, lambda_s=T.CAPS['lambda_s'], lambda_t=T.CAPS['lambda_t'],
            eps_sd=T.CAPS['eps_sd'], max_grad_norm=T.MAX_NORM, actor=p(t['actor'], 1 + first), actor_target=p(t['actor_target'], 1 + first),
            actor_m=p(t['actor_m'], 1 + first), actor_v=p(t['actor_v'], 1 + first), actor_stride=t['actor'].stride(0),
            critic=p(t['critic'], 1 + first), critic_target=p(t['critic_target'], 1 + first), critic_m=p(t['critic_m'], 1 + first),
            critic_v=p(t['critic_v'], 1 + first), critic_stride=t['critic'].stride(0), adam_steps=p(t['steps'], 1 + first), ring=t['ring'].data_ptr(),
            ring_stride=0, slots=sl.data_ptr() if sl is not None else None, slots_stride=0, target_noise=tn.data_ptr() if tn is not None else None,
            noise_stride=0, caps_noise=cn.data_ptr() if cn is not None else None, caps_stride=0, td_loss=p(t['td'], 1 + first, u0),
            pg_loss=p(t['pg'], 1 + first, u0), loss_stride=t['td'].stride(0), work=self.work.data_ptr(), work_bytes=self.wb)

    def rng_desc(self, caps, dense=0, learner0=0, seed=SEED, n_rows=None):
        return self.C.Td3RngDesc(seed=seed, n_rows=self.n_rows if n_rows is None else n_rows, learner0=learner0, dense=dense, caps=caps)

    def run_rng(self, caps, freq, it0, dense=0, learner0=0, n=None, **kw):
        rc = self.L.serl_td3_train_rng(self.engine.ctx, ctypes.byref(self.desc(self.n if n is None else n, it0, freq, **kw)),
                                       ctypes.byref(self.rng_desc(caps, dense, learner0)), self.stream())
        torch.cuda.synchronize()
        return rc

    def fill(self, caps, freq, it0, learner0=0, learner=0, n=None):
        """serl_td3_rng_fill -> (slots, target_noise, caps_noise or None) on the device"""
        n = self.n if n is None else n
        k = (it0 + n) // freq - it0 // freq
        sl = torch.full((n, self.B), -9, dtype=torch.int32, device=self.dev)
        tn = torch.full((n, self.B, self.A), float('nan'), device=self.dev)
        cn = torch.full((max(k, 1), self.B, self.S), float('nan'), device=self.dev) if caps else None
        rc = self.L.serl_td3_rng_fill(self.engine.ctx, ctypes.byref(self.rng_desc(caps, 0, learner0)), learner, self.S, self.A, self.B, it0, n, freq,
                                      sl.data_ptr(), tn.data_ptr(), cn.data_ptr() if caps else None, self.stream())
        torch.cuda.synchronize()
        assert rc == 0
        return sl, tn, (cn[:k] if caps else None)

    def run_tables(self, tables, freq, it0, dense=0, n=None, **kw):
        fn = self.L.serl_td3_train_mfma if dense else self.L.serl_td3_train
        rc = fn(self.engine.ctx, ctypes.byref(self.desc(self.n if n is None else n, it0, freq, tables=tables, **kw)), self.stream())
        torch.cuda.synchronize()
        return rc

    def out(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def assert_guards(self, o):
        h = self.host
        for k in T.ROWS + T.MOMENTS:
            P = self.Pa if k.startswith('actor') else self.Pc
            np.testing.assert_array_equal(o[k][:, P:], h[k][:, P:], err_msg=k)
            np.testing.assert_array_equal(o[k][[0, -1]], h[k][[0, -1]], err_msg=k)
        for k in ('td', 'pg', 'steps'):
            np.testing.assert_array_equal(o[k][[0, -1]], h[k][[0, -1]], err_msg=k)
        np.testing.assert_array_equal(o['ring'], h['ring'])


def _same(a, b, what=''):
    for k in OUT:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s %s' % (what, k))


def _finite_and_moved(la, o, caps, freq, it0):
    """no NaN anywhere (the ring's rows from n_rows on were never read), the rows moved, and the losses sit where the schedule puts them"""
    n = la.n
    actor_updates = [u for u in range(n) if (it0 + u + 1) % freq == 0]
    for i in range(1, la.K + 1):
        for k in T.ROWS + T.MOMENTS:
            P = la.Pa if k.startswith('actor') else la.Pc
            assert np.isfinite(o[k][i, :P]).all(), k
        assert np.isfinite(o['td'][i, :n]).all() and (o['td'][i, n:] == -3.5).all()
        for u in range(n):
            assert (o['pg'][i, u] != -3.5) == (u in actor_updates), u
        assert np.isfinite(o['pg'][i, actor_updates]).all()
        np.testing.assert_array_equal(o['steps'][i], [n, len(actor_updates)])
        assert np.abs(o['critic'][i, :la.Pc] - la.host['critic'][i, :la.Pc]).max() > 0
        if actor_updates:
            assert np.abs(o['actor'][i, :la.Pa] - la.host['actor'][i, :la.Pa]).max() > 0


@pytest.mark.parametrize('sched', SCHEDULES, ids=lambda s: 'caps%d_f%d_i%d' % s)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'S%dA%d_B%d_r%d_c%d' % s)
def test_generator_kernels_equal_table_kernels_on_the_replayed_tables(engine, shape, sched):
    """both dense flavours: every array serl_td3_train_rng writes equals what serl_td3_train / _mfma write from serl_td3_rng_fill's tables"""
    caps, freq, it0 = sched
    H = 8 if SHAPES.index(shape) % 2 == 0 else 12
    res = {}
    for dense in (0, 1):
        g = Launch(engine, shape, H)
        assert g.run_rng(caps, freq, it0, dense) == 0, g.L.serl_last_error()
        o = g.out()
        g.assert_guards(o)
        _finite_and_moved(g, o, caps, freq, it0)
        tb = Launch(engine, shape, H)
        tables = tb.fill(caps, freq, it0)
        sl = tables[0].cpu().numpy()
        assert sl.min() >= 0 and sl.max() < g.n_rows and all(len(set(r.tolist())) == g.B for r in sl)
        assert tb.run_tables(tables, freq, it0, dense) == 0, tb.L.serl_last_error()
        _same(o, tb.out(), 'dense %d' % dense)
        res[dense] = o
    _same(res[0], res[1], 'valu against mfma')


def test_split_invariance_and_zero_updates(engine):
    """6 updates in one call equal 2 + 4 (iteration0 advanced, Adam counts carried); 0 updates leave every buffer as it was"""
    shape, (caps, freq, it0) = SHAPES[0], (1, 2, 1)
    for dense in (0, 1):
        one = Launch(engine, shape, 8)
        assert one.run_rng(caps, freq, it0, dense) == 0
        two = Launch(engine, shape, 8)
        assert two.run_rng(caps, freq, it0, dense, n=2) == 0
        assert two.run_rng(caps, freq, it0 + 2, dense, n=4, u0=2) == 0
        _same(one.out(), two.out(), 'dense %d' % dense)
        z = Launch(engine, shape, 8)
        assert z.run_rng(caps, freq, it0, dense, n=0) == 0
        o = z.out()
        for k, v in z.host.items():
            np.testing.assert_array_equal(o[k], v, err_msg=k)
        assert torch.isnan(z.work).all()


def test_two_learners_equal_two_launches(engine):
    """n_learners 2 with learner0 5 against single-learner calls with learner0 5 and 6; the two learners draw different slots"""
    shape, (caps, freq, it0) = SHAPES[3], (1, 2, 0)
    both = Launch(engine, shape, 12, K=2)
    assert both.run_rng(caps, freq, it0, 0, learner0=5) == 0
    o = both.out()
    both.assert_guards(o)
    _finite_and_moved(both, o, caps, freq, it0)
    for i in (0, 1):
        solo = Launch(engine, shape, 12, K=2)
        assert solo.run_rng(caps, freq, it0, 0, learner0=5 + i, first=i, K=1) == 0
        s = solo.out()
        for k in OUT:
            np.testing.assert_array_equal(s[k][1 + i], o[k][1 + i], err_msg='%s learner %d' % (k, i))
            np.testing.assert_array_equal(s[k][2 - i], solo.host[k][2 - i], err_msg=k)
        a = both.fill(caps, freq, it0, learner0=5, learner=i)
        b = both.fill(caps, freq, it0, learner0=5 + i, learner=0)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    s5, s6 = both.fill(caps, freq, it0, learner0=5)[0], both.fill(caps, freq, it0, learner0=6)[0]
    assert (s5 != s6).any()


def _words(L, seed, c0, c1, c2, c3):
    w = (ctypes.c_uint32 * 4)()
    L.serl_host_philox(seed, c0, c1, c2, c3, w)
    return list(w)


def test_fill_against_the_host(engine):
    """slots row for row against serl_host_td3_slots; CAPS uniforms exactly and target normals to 1e-6 max(1, |z|) against the host's
    Philox words (f64 Box-Muller in numpy: a few ulp of libm plus one rounding to f32)"""
    la = Launch(engine, SHAPES[0], 8)
    S, A, B = la.S, la.A, la.B
    freq, it0, learner = 2, 1, 3
    sl, tn, cn = (x.cpu().numpy() for x in la.fill(1, freq, it0, learner0=learner))
    assert cn.shape == (3, B, S) and tn.shape == (N, B, A)
    k = 0
    for u in range(N):
        it = it0 + u + 1
        want = np.zeros(B, np.int32)
        assert la.L.serl_host_td3_slots(SEED, learner, it, la.n_rows, B, want.ctypes.data) == 0
        np.testing.assert_array_equal(sl[u], want, err_msg='update %d' % u)
        w = np.array([[_words(la.L, SEED, learner, it, b, (3 << 16) | blk) for blk in range(2)] for b in range(B)], dtype=np.uint64)
        kk = (w[..., 0::2] << np.uint64(20)) | (w[..., 1::2] >> np.uint64(12))
        uni = (2.0 * kk.astype(np.float64) + 1.0) * 2.0**-53
        r = np.sqrt(-2.0 * np.log(uni[..., 0]))
        z = np.stack([r * np.cos(2 * np.pi * uni[..., 1]), r * np.sin(2 * np.pi * uni[..., 1])], -1).reshape(B, 4)[:, :A]
        err = np.abs(tn[u].astype(np.float64) - z) / np.maximum(1.0, np.abs(z))
        assert err.max() <= 1e-6, (u, err.max())
        if it % freq == 0:
            cw = np.array([[_words(la.L, SEED, learner, it, b, (4 << 16) | blk) for blk in range(4)] for b in range(B)], dtype=np.uint32).reshape(B, 16)
            np.testing.assert_array_equal(cn[k], ((cw >> 8).astype(np.float32) * np.float32(2.0**-24))[:, :S], err_msg='update %d' % u)
            k += 1
    assert k == 3 and cn.min() >= 0.0 and cn.max() < 1.0


def test_fill_moments_of_the_target_normals(engine):
    """86 x 3 x 2 000 standard normals: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N)"""
    la = Launch(engine, SHAPES[0], 8)
    _, tn, cn = la.fill(1, 2, 0, n=2000)
    z = tn.cpu().numpy().astype(np.float64).reshape(-1)
    n = z.size
    assert n == 86 * 3 * 2000 and np.isfinite(z).all()
    print('TD3_RNG normals mean %.3g var - 1 %.3g' % (z.mean(), z.var() - 1.0))
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    u = cn.cpu().numpy().astype(np.float64).reshape(-1)
    assert u.size == 86 * 7 * 1000 and abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / u.size)


def test_refusals_launch_nothing(engine):
    """every new SERL_E_INVALID case, the refusals of serl_td3_train that still apply, and those that no longer do (NULL tables)"""
    la = Launch(engine, SHAPES[0], 8)
    C, L = la.C, la.L
    call = lambda d, r: L.serl_td3_train_rng(engine.ctx, ctypes.byref(d), ctypes.byref(r) if r is not None else None, la.stream())
    d = la.desc(N, 0, 2)
    assert d.slots is None and d.target_noise is None and d.caps_noise is None and d.slot_cols == 0
    assert call(d, None) == C.E_INVALID
    for field, v in (('n_rows', la.B - 1), ('n_rows', la.cap + 1), ('n_rows', -1), ('dense', 2), ('dense', -1), ('caps', 2), ('caps', -1)):
        r = la.rng_desc(1)
        setattr(r, field, v)
        assert call(d, r) == C.E_INVALID, field
    for field, v in (('actor', None), ('ring', None), ('work', None), ('n_updates', -1), ('policy_update_freq', 0), ('activation', 3),
                     ('capacity', 0), ('n_learners', 0), ('work_bytes', 16), ('lr', 0.0), ('tau', 1.5)):
        d = la.desc(N, 0, 2)
        setattr(d, field, v)
        assert call(d, la.rng_desc(1)) == C.E_INVALID, field
    for field, v in (('hidden', 132), ('hidden', 6), ('num_layers', 5), ('state_dim', 17), ('action_dim', 5), ('batch', 129)):
        d = la.desc(N, 0, 2)
        setattr(d, field, v)
        assert call(d, la.rng_desc(1)) == C.E_UNSUPPORTED, field
        assert call(d, None) == C.E_UNSUPPORTED, field                 # (the generator's descriptor is looked at last)
    torch.cuda.synchronize()
    o = la.out()
    for k, v in la.host.items():
        np.testing.assert_array_equal(o[k], v, err_msg=k)
    assert torch.isnan(la.work).all()
    sl = torch.zeros(N, la.B, dtype=torch.int32, device=la.dev)
    tn = torch.zeros(N, la.B, la.A, device=la.dev)
    fill = lambda r, *a: L.serl_td3_rng_fill(engine.ctx, ctypes.byref(r), *a, sl.data_ptr(), tn.data_ptr(), None, la.stream())
    assert fill(la.rng_desc(1), 0, la.S, la.A, la.B, 0, N, 2) == 0
    for a in ((0, 17, la.A, la.B, 0, N, 2), (0, la.S, 5, la.B, 0, N, 2), (0, la.S, la.A, 129, 0, N, 2), (0, la.S, la.A, 0, 0, N, 2),
              (-1, la.S, la.A, la.B, 0, N, 2), (0, la.S, la.A, la.B, -1, N, 2), (0, la.S, la.A, la.B, 0, -1, 2), (0, la.S, la.A, la.B, 0, N, 0)):
        assert fill(la.rng_desc(1), *a) == C.E_INVALID, a
    assert fill(la.rng_desc(1, n_rows=la.B - 1), 0, la.S, la.A, la.B, 0, N, 2) == C.E_INVALID
    torch.cuda.synchronize()


def _state(t):
    from serl_amd.actor import pack_actor, pack_critic
    from serl_amd.td3 import _pack_adam
    am, av, asteps = _pack_adam(t.actor_optim, list(t.actor.parameters()))
    cm, cv, csteps = _pack_adam(t.critic_optim, list(t.critic.parameters()))
    return dict(actor=pack_actor(t.actor).numpy(), actor_target=pack_actor(t.actor_target).numpy(), critic=pack_critic(t.critic).numpy(),
                critic_target=pack_critic(t.critic_target).numpy(), actor_m=am.numpy(), actor_v=av.numpy(), critic_m=cm.numpy(), critic_v=cv.numpy(),
                steps=np.array([csteps, asteps]))


@pytest.mark.parametrize('dense', ['valu', 'mfma'])
def test_td3_train_draws_device(engine, monkeypatch, dense):
    """TD3.train(draws='device', seed=s) touches neither python's `random` nor the generator, reports its path, and equals a twin learner
    on the host path whose sample_many / draw_noise return serl_amd.td3_draws' tables; seeds differ, a seed repeats"""
    import serl_amd
    from serl_amd import td3 as td3_mod
    dev = engine.device
    S, A, H, B, n, it0, rows = 7, 3, 12, 17, 6, 3, 40
    ring_rows = torch.from_numpy(_ring(S, A, rows, rows))

    def learner():
        torch.manual_seed(5)
        t = serl_amd.TD3(G._args(S, A, H, 1, 'tanh', B, 'cpu'), engine)
        ring = serl_amd.DeviceReplay(64, dev, engine, S, A)
        ring.append_rows(ring_rows)
        return t, ring

    def device_run(seed):
        t, ring = learner()
        gen = torch.Generator().manual_seed(9)
        m0, g0 = random.getstate(), gen.get_state().clone()
        out = t.train(ring, n, iteration0=it0, generator=gen, draws='device', seed=seed, learner=2, dense=dense)
        assert random.getstate() == m0 and torch.equal(gen.get_state(), g0)
        assert t.last_path == ('fused-mfma-rng' if dense == 'mfma' else 'fused-rng') and t.last_table_bytes == 0
        assert np.isfinite(out['TD_loss']) and np.isfinite(out['PG_obj'])
        return _state(t), out

    a, out_a = device_run(77)
    a2, out_a2 = device_run(77)
    b, _ = device_run(78)
    for k in a:
        np.testing.assert_array_equal(a[k], a2[k], err_msg=k)
    assert out_a == out_a2
    assert (a['critic'] != b['critic']).any() and (a['actor'] != b['actor']).any()
    np.testing.assert_array_equal(a['steps'], [n, 3])

    sl, tn, cn = serl_amd.td3_draws(engine, seed=77, learner=2, iteration0=it0, n_updates=n, batch=B, n_rows=rows, state_dim=S, action_dim=A,
                                    policy_update_freq=2, caps=True, device=dev)
    assert sl.shape == (n, B) and tn.shape == (n, B, A) and cn.shape == (3, B, S) and int(sl.max()) < rows
    monkeypatch.setattr(td3_mod._replay, 'sample_many', lambda n_, k_, calls, rng=None: sl.cpu().numpy())
    monkeypatch.setattr(td3_mod, 'draw_noise', lambda *a_, **kw_: (tn.cpu(), cn.cpu()))
    t, ring = learner()
    out_h = t.train(ring, n, iteration0=it0, dense=dense)
    assert t.last_path == ('fused-mfma' if dense == 'mfma' else 'fused') and t.last_table_bytes > 0
    h = _state(t)
    for k in a:
        np.testing.assert_array_equal(a[k], h[k], err_msg=k)
    assert out_a == out_h

"""serl_td3_train_big -- the fused TD3 learner on minibatches of up to 512 rows, walked in chunks of 128 samples: one chunk against the
kernels it generalises (bit for bit), several chunks against the float64 contract of tests/td3_64.py with its tolerances as they stand,
mfma against valu and in-kernel draws against serl_td3_rng_fill_big's tables (bit for bit), the invariants the other TD3 kernels have,
the refusals, and TD3.train with batch_size 256."""
import ctypes
import functools
import random
import numpy as np
import pytest
import torch
import td3_64 as T
import td3_big as TB
import test_gpu_td3 as G
import test_gpu_td3_rng as R

pytestmark = pytest.mark.gpu
OUT = T.ROWS + T.MOMENTS + ('td', 'pg', 'steps')
SEED = 0x9E3779B97F4A7C15


@functools.lru_cache(maxsize=None)
def _big(c, seed=None):
    d = TB.make_case(c, seed)
    return d, T.td3_literal(d)


@functools.lru_cache(maxsize=None)
def _small(c):
    return T.make_case(c)


class Launch:
    """device buffers of K learners of one shape, rows 1 .. K of every per-learner array (row 0 and row K + 1 are guards, strides leave
    columns behind every row), and one call of serl_td3_train_big or of an older entry on them.  The ring holds the first n_rows rows of
    the case's and NaN behind them (at least one row, unless full=True); unused slot columns name the last, NaN, row; the workspace is
    NaN-filled and has eight floats past its end."""

    def __init__(self, engine, cases, n=None, extra=5, n_rows=None, full=False):
        from serl_amd import _capi
        self.C, self.L = _capi, _capi.lib()
        self.engine, self.cases, self.dev = engine, cases, engine.device
        d0 = cases[0]
        K = self.K = len(cases)
        S, A, B = d0['S'], d0['A'], d0['B']
        self.n = d0['n'] if n is None else n
        n_all = d0['n']
        self.Pa, self.Pc = len(d0['actor']), len(d0['critic'])
        self.sa, self.sc = self.Pa + extra, self.Pc + extra
        host = {}
        for k, P, st in (('actor', self.Pa, self.sa), ('actor_target', self.Pa, self.sa), ('actor_m', self.Pa, self.sa), ('actor_v', self.Pa, self.sa),
                         ('critic', self.Pc, self.sc), ('critic_target', self.Pc, self.sc), ('critic_m', self.Pc, self.sc), ('critic_v', self.Pc, self.sc)):
            a = np.full((K + 2, st), 7.25, np.float32)
            for i, d in enumerate(cases):
                a[1 + i, :P] = d[k] if k in d else 0.0
            host[k] = a
        self.n_rows = d0['ring'].shape[0] if n_rows is None else n_rows
        cap = self.cap = self.n_rows if full else d0['ring'].shape[0] + 1
        ring = np.full((K, cap, 2 * S + A + 3), np.nan, np.float32)
        slots = np.full((K, n_all, B + 3), cap - 1, np.int32)
        tn = np.zeros((K, n_all, B, A), np.float32)
        cn = np.zeros((K, max(d0['n_actor'], 1), B, S), np.float32)
        for i, d in enumerate(cases):
            ring[i, :self.n_rows] = d['ring'][:self.n_rows]
            slots[i, :, :B] = d['slots']
            tn[i] = d['tn']
            if d['caps']:
                cn[i, :d['n_actor']] = d['cn']
        host.update(ring=ring, slots=slots, tn=tn, cn=cn)
        host['steps'] = np.zeros((K + 2, 2), np.int32)
        host['td'] = np.full((K + 2, n_all + 2), -3.5, np.float32)
        host['pg'] = np.full((K + 2, n_all + 2), -3.5, np.float32)
        self.host = host
        self.t = {k: torch.from_numpy(v).to(self.dev) for k, v in host.items()}
        self.wb = int(self.L.serl_td3_big_work_bytes(K, S, A, d0['H'], d0['L'], B))
        assert self.wb > 0
        self.work = torch.full((self.wb // 4 + 8,), float('nan'), dtype=torch.float32, device=self.dev)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def desc(self, n=None, it0=None, u0=0, k0=0, first=0, K=None, tables=None, no_tables=False):
        """n updates from update u0 (actor update k0) of the tables, learners first .. first + K; tables = (slots, tn, cn) of a fill
        replace the case's (one learner, no spare columns); no_tables: the table fields are NULL / 0 (the generator's calls)"""
        d0, t = self.cases[0], self.t
        K = self.K if K is None else K
        n = self.n if n is None else n
        it0 = d0['it0'] if it0 is None else it0
        p = lambda x, *idx: x[idx].data_ptr()
        sl, tn, cn, cols = p(t['slots'], first, u0), p(t['tn'], first, u0), p(t['cn'], first, k0) if d0['caps'] else None, t['slots'].shape[2]
        strides = (t['slots'].stride(0), t['tn'].stride(0), t['cn'].stride(0))
        if tables is not None:
            sl, tn, cn, cols, strides = tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr() if tables[2] is not None else None, d0['B'], (0, 0, 0)
        if no_tables:
            sl, tn, cn, cols, strides = None, None, None, 0, (0, 0, 0)
        return self.C.Td3Desc(
            state_dim=d0['S'], action_dim=d0['A'], hidden=d0['H'], num_layers=d0['L'], activation=G.ACT[d0['act']], n_learners=K, batch=d0['B'],
            n_updates=n, capacity=self.cap, slot_cols=cols, policy_update_freq=d0['freq'], iteration0=it0,
            update_actor_target=int(d0['uat']), lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP,
            lambda_s=T.CAPS['lambda_s'], lambda_t=T.CAPS['lambda_t'], eps_sd=T.CAPS['eps_sd'], max_grad_norm=T.MAX_NORM,
            actor=p(t['actor'], 1 + first), actor_target=p(t['actor_target'], 1 + first), actor_m=p(t['actor_m'], 1 + first),
            actor_v=p(t['actor_v'], 1 + first), actor_stride=self.sa, critic=p(t['critic'], 1 + first),
            critic_target=p(t['critic_target'], 1 + first), critic_m=p(t['critic_m'], 1 + first), critic_v=p(t['critic_v'], 1 + first),
            critic_stride=self.sc, adam_steps=p(t['steps'], 1 + first), ring=p(t['ring'], first), ring_stride=t['ring'].stride(0),
            slots=sl, slots_stride=strides[0], target_noise=tn, noise_stride=strides[1], caps_noise=cn, caps_stride=strides[2],
            td_loss=p(t['td'], 1 + first, u0), pg_loss=p(t['pg'], 1 + first, u0), loss_stride=t['td'].stride(0), work=self.work.data_ptr(),
            work_bytes=self.wb)

    def rng_desc(self, dense=0, learner0=0, seed=SEED):
        return self.C.Td3RngDesc(seed=seed, n_rows=self.n_rows, learner0=learner0, dense=dense, caps=int(self.cases[0]['caps']))

    def run(self, entry='big', dense=0, gen=False, learner0=0, **kw):
        """entry 'big': serl_td3_train_big; 'old': serl_td3_train / _mfma / _rng.  gen: the in-kernel generator instead of the tables"""
        d = self.desc(no_tables=gen, **kw)
        rd = self.rng_desc(dense, learner0) if gen else None
        if entry == 'big':
            bd = self.C.Td3BigDesc(rng=ctypes.pointer(rd) if gen else None, dense=dense)
            rc = self.L.serl_td3_train_big(self.engine.ctx, ctypes.byref(d), ctypes.byref(bd), self.stream())
        elif gen:
            rc = self.L.serl_td3_train_rng(self.engine.ctx, ctypes.byref(d), ctypes.byref(rd), self.stream())
        else:
            rc = (self.L.serl_td3_train_mfma if dense else self.L.serl_td3_train)(self.engine.ctx, ctypes.byref(d), self.stream())
        torch.cuda.synchronize()
        return rc

    def fill(self, it0=None, n=None, learner0=0, learner=0):
        """serl_td3_rng_fill_big -> (slots, target_noise, caps_noise or None) on the device"""
        d0 = self.cases[0]
        n = self.n if n is None else n
        it0 = d0['it0'] if it0 is None else it0
        S, A, B, freq = d0['S'], d0['A'], d0['B'], d0['freq']
        k = (it0 + n) // freq - it0 // freq
        sl = torch.full((n, B), -9, dtype=torch.int32, device=self.dev)
        tn = torch.full((n, B, A), float('nan'), device=self.dev)
        cn = torch.full((max(k, 1), B, S), float('nan'), device=self.dev) if d0['caps'] else None
        rc = self.L.serl_td3_rng_fill_big(self.engine.ctx, ctypes.byref(self.rng_desc(0, learner0)), learner, S, A, B, it0, n, freq, sl.data_ptr(),
                                          tn.data_ptr(), cn.data_ptr() if cn is not None else None, self.stream())
        torch.cuda.synchronize()
        assert rc == 0, self.L.serl_last_error()
        return sl, tn, (cn[:k] if cn is not None else None)

    def out(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def result(self, o, i):
        r = {k: o[k][1 + i, :(self.Pa if k.startswith('actor') else self.Pc)] for k in T.ROWS + T.MOMENTS}
        n = self.cases[0]['n']
        r['td'], r['pg'] = o['td'][1 + i, :n], o['pg'][1 + i, :n]
        return r

    def assert_guards(self, o, n=None):
        """columns past the rows, the guard learners, loss entries from n on, pg entries of non-actor updates, every input: as given"""
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
            assert ((o['pg'][1:-1, u] == -3.5) == ((d0['it0'] + u + 1) % d0['freq'] != 0)).all(), u
        for k in ('ring', 'slots', 'tn', 'cn'):
            np.testing.assert_array_equal(o[k], h[k], err_msg=k)
        assert torch.isnan(self.work[-8:]).all()

    def assert_untouched(self):
        o = self.out()
        for k, v in self.host.items():
            np.testing.assert_array_equal(o[k], v, err_msg=k)
        assert torch.isnan(self.work).all()


def _same(a, b, what=''):
    for k in OUT:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s %s' % (what, k))


# ---- 1. one chunk equals the old kernels ------------------------------------------------------------------------------------------------
# B = 1, 86, 128 with CAPS on and off (td3_64.CASES where it has the pair; B = 1 with CAPS and B = 128 without are added)
ONE_CHUNK = [(7, 3, 20, 1, 'tanh', 1, 2, 0, 13, 1, 1, 'small'), T.CASES[5], T.CASES[0], T.CASES[8], T.CASES[1], (7, 3, 72, 3, 'relu', 128, 2, 0, 13, 0, 1, 'small')]


@pytest.mark.parametrize('gen', [False, True], ids=['tables', 'rng'])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('c', ONE_CHUNK, ids=T.case_id)
def test_one_chunk_equals_the_old_kernel(engine, c, dense, gen):
    """B = 1, 86, 128: every array serl_td3_train_big writes is bit for bit that of serl_td3_train / _mfma / _rng on the same inputs"""
    d = _small(c)
    assert d['B'] in (1, 86, 128)
    old, new = Launch(engine, [d]), Launch(engine, [d])
    assert new.wb == old.L.serl_td3_work_bytes(1, d['S'], d['A'], d['H'], d['L'], d['B'])
    assert old.run('old', dense, gen) == 0, old.L.serl_last_error()
    assert new.run('big', dense, gen) == 0, new.L.serl_last_error()
    a, b = old.out(), new.out()
    new.assert_guards(b)
    np.testing.assert_array_equal(b['steps'][1], [d['n'], d['n_actor']])
    assert np.isfinite(new.result(b, 0)['td']).all() and np.abs(b['critic'][1, :new.Pc] - new.host['critic'][1, :new.Pc]).max() > 0
    _same(a, b, T.case_id(c))


# ---- 2. + 3. several chunks against float64; mfma equals valu ------------------------------------------------------------------------
@pytest.mark.parametrize('c', TB.CASES, ids=T.case_id)
def test_chunks_vs_float64_and_mfma_equals_valu(engine, c):
    """rows, targets, moments, td_loss[0] and the first pg_loss against the float64 run within td3_64.check's bounds, td_loss within
    rtol 2e-3 / atol 1e-5, in both dense flavours; the two flavours bit for bit equal; NaN ring rows, unused slot columns, guards untouched"""
    d, ref = _big(c)
    assert all(ref['clip_c']) if d['rew'] == 'big' else not any(ref['clip_c']), ref['clip_c']
    res = {}
    for dense in (0, 1):
        la = Launch(engine, [d])
        assert la.run('big', dense) == 0, la.L.serl_last_error()
        o = res[dense] = la.out()
        got = la.result(o, 0)
        T.check(got, ref, d, '%s dense %d' % (T.case_id(c), dense))
        print('TD3_BIG td max rel %.3g' % np.max(np.abs(got['td'] - ref['td']) / np.maximum(np.abs(ref['td']), 1e-30)))
        np.testing.assert_allclose(got['td'], ref['td'], rtol=2e-3, atol=1e-5)
        la.assert_guards(o)
        np.testing.assert_array_equal(o['steps'][1], [d['n'], d['n_actor']])
    _same(res[0], res[1], 'valu against mfma')


# ---- 4. generator equals tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('full', [True, False], ids=['full', 'part'])
@pytest.mark.parametrize('c', [c for c in TB.CASES if c[5] in (129, 300, 512) and c[:5] == TB.SHAPES[0]], ids=T.case_id)
def test_generator_equals_tables(engine, c, full):
    """in-kernel draws against serl_td3_train_big on serl_td3_rng_fill_big's tables, both flavours, on a full ring (n_rows = capacity =
    600) and on 600 filled rows with NaN behind them; the fill's slots are serl_host_td3_slots' row for row"""
    d, _ = _big(c)
    B, n_rows = d['B'], 600
    res = {}
    for dense in (0, 1):
        g = Launch(engine, [d], n_rows=n_rows, full=full)
        assert g.run('big', dense, gen=True, learner0=3) == 0, g.L.serl_last_error()
        o = res[dense] = g.out()
        g.assert_guards(o)
        for k in OUT:
            assert np.isfinite(o[k][1]).all() or k == 'pg', k
        tb = Launch(engine, [d], n_rows=n_rows, full=full)
        tables = tb.fill(learner0=3)
        sl = tables[0].cpu().numpy()
        for u in range(d['n']):
            want = np.zeros(B, np.int32)
            assert g.L.serl_host_td3_slots(SEED, 3, d['it0'] + u + 1, n_rows, B, want.ctypes.data) == 0
            np.testing.assert_array_equal(sl[u], want, err_msg='update %d' % u)
        assert tb.run('big', dense, tables=tables) == 0, tb.L.serl_last_error()
        _same(o, tb.out(), 'dense %d' % dense)
    _same(res[0], res[1], 'valu against mfma')


# ---- 5. the invariants the other TD3 kernels have ---------------------------------------------------------------------------------
@pytest.mark.parametrize('gen', [False, True], ids=['tables', 'rng'])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
def test_two_calls_equal_one_and_zero_updates(engine, dense, gen):
    c = TB.CASES[12]                        # B = 300
    d, _ = _big(c)
    one = Launch(engine, [d])
    assert one.run('big', dense, gen) == 0
    n1 = 5
    k1 = sum(1 for u in range(n1) if (d['it0'] + u + 1) % d['freq'] == 0)
    two = Launch(engine, [d])
    assert two.run('big', dense, gen, n=n1) == 0
    assert two.run('big', dense, gen, n=d['n'] - n1, it0=d['it0'] + n1, u0=n1, k0=k1) == 0
    _same(one.out(), two.out())
    z = Launch(engine, [d])
    assert z.run('big', dense, gen, n=0) == 0
    z.assert_untouched()


def test_two_learners_equal_two_launches(engine):
    c = TB.CASES[9]                         # B = 257
    cases = [_big(c, seed)[0] for seed in (None, 31)]
    for gen in (False, True):
        both = Launch(engine, cases)
        assert both.run('big', 1, gen, learner0=5) == 0
        o = both.out()
        both.assert_guards(o)
        for i in (0, 1):
            solo = Launch(engine, cases)
            assert solo.run('big', 1, gen, learner0=5 + i, first=i, K=1) == 0
            s = solo.out()
            for k in OUT:
                np.testing.assert_array_equal(s[k][1 + i], o[k][1 + i], err_msg='%s learner %d' % (k, i))
                np.testing.assert_array_equal(s[k][2 - i], solo.host[k][2 - i], err_msg=k)
        assert (o['critic'][1] != o['critic'][2]).any()


# ---- 6. refusals, each before any launch -------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(engine):
    d, _ = _big(TB.CASES[6])                # B = 256
    la = Launch(engine, [d])
    C, L = la.C, la.L
    big = lambda desc, bd: L.serl_td3_train_big(engine.ctx, ctypes.byref(desc), ctypes.byref(bd) if bd is not None else None, la.stream())
    tables, rd = C.Td3BigDesc(rng=None, dense=0), la.rng_desc(0)
    gen = C.Td3BigDesc(rng=ctypes.pointer(rd), dense=0)
    for bd in (tables, gen):
        x = la.desc(); x.batch = 513; x.slot_cols = 600
        assert big(x, bd) == C.E_UNSUPPORTED
        x = la.desc(); x.work_bytes = la.wb - 1
        assert big(x, bd) == C.E_INVALID
        for field, v in (('hidden', 132), ('num_layers', 5), ('state_dim', 17), ('action_dim', 5)):
            x = la.desc(); setattr(x, field, v)
            assert big(x, bd) == C.E_UNSUPPORTED, field
        for field, v in (('actor', None), ('work', None), ('n_updates', -1), ('policy_update_freq', 0), ('capacity', 0), ('lr', 0.0)):
            x = la.desc(); setattr(x, field, v)
            assert big(x, bd) == C.E_INVALID, field
    x = la.desc(); x.slot_cols = d['B'] - 1
    assert big(x, tables) == C.E_INVALID
    assert big(la.desc(), None) == C.E_INVALID
    assert big(la.desc(), C.Td3BigDesc(rng=None, dense=2)) == C.E_INVALID
    assert big(la.desc(no_tables=True), C.Td3BigDesc(rng=ctypes.pointer(la.rng_desc(1)), dense=0)) == C.E_INVALID        # the two dense disagree
    assert big(la.desc(no_tables=True), tables) == C.E_INVALID                                                          # NULL tables without a generator
    bad = la.rng_desc(0); bad.n_rows = d['B'] - 1
    assert big(la.desc(no_tables=True), C.Td3BigDesc(rng=ctypes.pointer(bad), dense=0)) == C.E_INVALID
    # the old entries still refuse a minibatch of 129 rows
    x = la.desc(); x.batch = 129
    assert L.serl_td3_train(engine.ctx, ctypes.byref(x), la.stream()) == C.E_UNSUPPORTED
    assert L.serl_td3_train_mfma(engine.ctx, ctypes.byref(x), la.stream()) == C.E_UNSUPPORTED
    assert L.serl_td3_train_rng(engine.ctx, ctypes.byref(x), ctypes.byref(rd), la.stream()) == C.E_UNSUPPORTED
    assert L.serl_td3_work_bytes(1, d['S'], d['A'], d['H'], d['L'], 129) == 0
    sl, tn = torch.zeros(2, 513, dtype=torch.int32, device=la.dev), torch.zeros(2, 513, d['A'], device=la.dev)
    assert L.serl_td3_rng_fill(engine.ctx, ctypes.byref(rd), 0, d['S'], d['A'], 129, 0, 2, 2, sl.data_ptr(), tn.data_ptr(), None, la.stream()) == C.E_INVALID
    assert L.serl_td3_rng_fill_big(engine.ctx, ctypes.byref(rd), 0, d['S'], d['A'], 513, 0, 2, 2, sl.data_ptr(), tn.data_ptr(), None, la.stream()) == C.E_INVALID
    torch.cuda.synchronize()
    la.assert_untouched()
    assert int(sl.abs().max()) == 0 and float(tn.abs().max()) == 0.0


# ---- 7. through TD3.train ---------------------------------------------------------------------------------------------------------
def test_td3_train_batch_256(engine, monkeypatch):
    """batch_size 256: fused=True, dense='mfma' and draws='device' run the kernel and say so; the default call stays the eager loop;
    draws='device' equals the raw entry bit for bit; td3_draws(batch 256) replays it on the table path"""
    import serl_amd
    from serl_amd import td3 as td3_mod
    dev = engine.device
    S, A, H, Lh, B, n, it0, rows = 7, 3, 72, 3, 256, 13, 3, 600
    n_act = (it0 + n) // 2 - it0 // 2          # actor updates: iterations 4, 6, .. 16
    d0, _ = _big(TB.CASES[6])
    ring_rows = torch.from_numpy(d0['ring'][:rows])

    def learner():
        torch.manual_seed(5)
        t = serl_amd.TD3(G._args(S, A, H, Lh, 'tanh', B, 'cpu'), engine)
        ring = serl_amd.DeviceReplay(700, dev, engine, S, A)
        ring.append_rows(ring_rows)
        return t, ring

    t, ring = learner()
    assert t.fused_big_supported(dev) and not t.fused_supported(dev)
    start = R._state(t)
    t.train(ring, 2, iteration0=0, rng=random.Random(1), generator=torch.Generator().manual_seed(1))
    assert t.last_path == 'eager'
    res = {}
    for key, kw, path in (('valu', dict(fused=True), 'fused-big'), ('mfma', dict(dense='mfma'), 'fused-mfma-big')):
        t, ring = learner()
        out = t.train(ring, n, iteration0=it0, rng=random.Random(3), generator=torch.Generator().manual_seed(9), **kw)
        assert t.last_path == path and t.last_table_bytes > 0 and np.isfinite(out['TD_loss']) and np.isfinite(out['PG_obj'])
        res[key] = R._state(t)
    for k in res['valu']:
        np.testing.assert_array_equal(res['valu'][k], res['mfma'][k], err_msg=k)
    t, ring = learner()
    gen = torch.Generator().manual_seed(9)
    m0, g0 = random.getstate(), gen.get_state().clone()
    out_a = t.train(ring, n, iteration0=it0, generator=gen, draws='device', seed=77, learner=2)
    assert random.getstate() == m0 and torch.equal(gen.get_state(), g0)
    assert t.last_path == 'fused-big-rng' and t.last_table_bytes == 0
    a = R._state(t)
    np.testing.assert_array_equal(a['steps'], [n, n_act])
    # the raw entry on the same rows, ring and generator
    case = dict(S=S, A=A, H=H, L=Lh, act='tanh', B=B, freq=2, it0=it0, n=n, caps=True, uat=True, n_actor=n_act, ring=d0['ring'],
                slots=np.zeros((n, B), np.int32), tn=np.zeros((n, B, A), np.float32), cn=np.zeros((n_act, B, S), np.float32),
                **{k: start[k] for k in T.ROWS})
    la = Launch(engine, [case], n_rows=rows)
    d = la.desc(no_tables=True)
    rd = la.C.Td3RngDesc(seed=77, n_rows=rows, learner0=2, dense=0, caps=1)
    bd = la.C.Td3BigDesc(rng=ctypes.pointer(rd), dense=0)
    assert la.L.serl_td3_train_big(engine.ctx, ctypes.byref(d), ctypes.byref(bd), la.stream()) == 0, la.L.serl_last_error()
    torch.cuda.synchronize()
    o = la.out()
    for k in T.ROWS + T.MOMENTS:
        np.testing.assert_array_equal(a[k], o[k][1, :len(a[k])], err_msg=k)
    np.testing.assert_array_equal(a['steps'], o['steps'][1])
    assert out_a['TD_loss'] == float(np.median(o['td'][1, :n]))
    # td3_draws writes the tables of the same call: the host path fed with them ends in the same place
    sl, tn, cn = serl_amd.td3_draws(engine, seed=77, learner=2, iteration0=it0, n_updates=n, batch=B, n_rows=rows, state_dim=S, action_dim=A,
                                    policy_update_freq=2, caps=True, device=dev)
    assert sl.shape == (n, B) and tn.shape == (n, B, A) and cn.shape == (n_act, B, S) and int(sl.max()) < rows
    monkeypatch.setattr(td3_mod._replay, 'sample_many', lambda n_, k_, calls, rng=None: sl.cpu().numpy())
    monkeypatch.setattr(td3_mod, 'draw_noise', lambda *a_, **kw_: (tn.cpu(), cn.cpu()))
    t, ring = learner()
    out_h = t.train(ring, n, iteration0=it0, fused=True)
    assert t.last_path == 'fused-big'
    h = R._state(t)
    for k in a:
        np.testing.assert_array_equal(a[k], h[k], err_msg=k)
    assert out_a == out_h

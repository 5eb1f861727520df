"""serl_td3_train_mfma -- the fused TD3 learner with its dense phases on the f32 matrix cores -- against serl_td3_train, bit for bit:
the grid of tests/td3_64.py (and the float64 contract on it), shapes at the edges of the 16 x 16 x 4 blocks that the grid misses, the
launch invariants and refusals of tests/test_gpu_td3.py on the new entry, a launch behind NaN-filled LDS, and TD3.train(dense='mfma')."""
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


class MfmaLaunch(G.Launch):
    """Launch whose run() calls serl_td3_train_mfma (same buffers, guards and NaN-filled workspace)"""

    def run(self, **kw):
        d0 = self.cases[0]
        kw.setdefault('n', self.n)
        kw.setdefault('it0', d0['it0'])
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        rc = self.L.serl_td3_train_mfma(self.engine.ctx, ctypes.byref(self.desc(**kw)), stream)
        torch.cuda.synchronize()
        return rc


@functools.lru_cache(maxsize=None)
def _edge(c):
    return T.make_case(c)


@functools.lru_cache(maxsize=None)
def _valu(engine, c):
    """the scalar kernel's result on a case of the grid or of EDGES (run once, shared, never modified)"""
    la = G.Launch(engine, [G._case(c)[0] if c in T.CASES else _edge(c)])
    assert la.run() == 0
    return la.out()


def _same(a, b, what=''):
    for k in OUT:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s %s' % (what, k))


@pytest.mark.parametrize('c', T.CASES, ids=T.case_id)
def test_mfma_equals_valu_on_the_grid(engine, c):
    """every case of the grid: rows, moments, losses and Adam counts of the matrix-core kernel equal the scalar kernel's bit for bit,
    and meet the float64 contract on their own; guards, NaN ring rows, unused slot columns untouched"""
    d, ref = G._case(c)
    la = MfmaLaunch(engine, [d])
    assert la.run() == 0
    o = la.out()
    _same(o, _valu(engine, c), T.case_id(c))
    T.check(la.result(o, 0), ref, d, 'mfma ' + T.case_id(c))
    la.assert_guards(o)
    np.testing.assert_array_equal(o['steps'][1], [d['n'], d['n_actor']])


# hidden 20: one full block of rows and a block of 4; 36: two and 4; 100: six and 4, K of the output layer's gradient in four column
# pairs; 128 with (1, 1): K = 1, N = 1 and every block full, all four groups of samples; hidden 4, B 1: one row block of 4, one sample.
# B 17 and 33: one sample into the second group of 32 / the second block of 16 reduced over (B4 = 20, 36).
#   (S, A, H, L, activation, B, freq, iteration0, n_updates, caps, update_actor_target, rewards)
EDGES = [(7, 3, 20, 1, 'tanh', 17, 2, 0, 6, 1, 1, 'small'), (7, 3, 36, 2, 'elu', 33, 2, 0, 6, 1, 0, 'small'),
         (16, 4, 100, 1, 'relu', 86, 2, 0, 6, 0, 1, 'small'), (1, 1, 128, 4, 'tanh', 128, 2, 0, 6, 1, 1, 'big'),
         (16, 4, 4, 0, 'elu', 1, 2, 0, 6, 1, 1, 'small')]


@pytest.mark.parametrize('c', EDGES, ids=T.case_id)
def test_mfma_equals_valu_at_the_tile_edges(engine, c):
    d = _edge(c)
    la = MfmaLaunch(engine, [d])
    assert la.run() == 0
    o = la.out()
    v = _valu(engine, c)
    _same(o, v, T.case_id(c))
    la.assert_guards(o)
    assert np.isfinite(o['actor'][1, :la.Pa]).all() and np.isfinite(o['critic'][1, :la.Pc]).all()
    assert np.abs(o['actor'][1, :la.Pa] - d['actor']).max() > 0 and np.abs(o['critic'][1, :la.Pc] - d['critic']).max() > 0


@pytest.mark.parametrize('c', [T.CASES[0], T.CASES[2]], ids=T.case_id)
def test_mfma_two_calls_equal_one(engine, c):
    """n1 updates, then the remaining ones with iteration0 advanced and the Adam counts carried: bit for bit the single call"""
    d, _ = G._case(c)
    one = MfmaLaunch(engine, [d])
    assert one.run() == 0
    a = one.out()
    n1 = 7
    k1 = sum(1 for u in range(n1) if (d['it0'] + u + 1) % d['freq'] == 0)
    two = MfmaLaunch(engine, [d])
    assert two.run(n=n1) == 0
    assert two.run(n=d['n'] - n1, it0=d['it0'] + n1, u0=n1, k0=k1) == 0
    _same(a, two.out())


def test_mfma_three_learners_equal_three_launches(engine):
    """three learners (different rows, rings, draws) in one launch against one launch each, bit for bit, guards intact"""
    c = T.CASES[10]
    cases = [G._case(c, seed)[0] for seed in (None, 21, 22)]
    la = MfmaLaunch(engine, cases)
    assert la.run() == 0
    o = la.out()
    la.assert_guards(o)
    for i, d in enumerate(cases):
        T.check(la.result(o, i), G._case(c, (None, 21, 22)[i])[1], d, 'mfma learner %d' % i)
        solo = MfmaLaunch(engine, cases)
        assert solo.run(first=i, K=1) == 0
        s = solo.out()
        for k in OUT:
            np.testing.assert_array_equal(s[k][1 + i], o[k][1 + i], err_msg='%s learner %d' % (k, i))
            others = [j for j in range(5) if j != 1 + i]
            np.testing.assert_array_equal(s[k][others], solo.host[k][others], err_msg=k)


def test_mfma_refusals_and_zero_updates(engine):
    """the lists of test_td3_refusals on the new entry: the same return codes, nothing written; n_updates = 0 is a no-op"""
    from serl_amd import _capi
    d, _ = G._case(T.CASES[3])
    la = MfmaLaunch(engine, [d])
    L = la.L
    stream = ctypes.c_void_p(torch.cuda.current_stream(la.dev).cuda_stream)
    for field, v in (('hidden', 132), ('hidden', 6), ('num_layers', 5), ('state_dim', 17), ('action_dim', 5), ('batch', 129)):
        desc = la.desc(la.n, d['it0'])
        setattr(desc, field, v)
        desc.slot_cols = 200
        assert L.serl_td3_train_mfma(engine.ctx, ctypes.byref(desc), stream) == _capi.E_UNSUPPORTED, field
    for field, v in (('actor', None), ('slots', None), ('work', None), ('n_updates', -1), ('policy_update_freq', 0), ('activation', 3),
                     ('capacity', 0), ('n_learners', 0), ('work_bytes', 16), ('slot_cols', 2), ('lr', 0.0), ('tau', 1.5)):
        desc = la.desc(la.n, d['it0'])
        setattr(desc, field, v)
        assert L.serl_td3_train_mfma(engine.ctx, ctypes.byref(desc), stream) == _capi.E_INVALID, field
    assert la.run(n=0) == 0
    o = la.out()
    for k, v in la.host.items():
        np.testing.assert_array_equal(o[k], v, err_msg=k)
    assert torch.isnan(la.work).all()


def test_mfma_behind_nan_filled_lds(engine):
    """Best effort: 512 learners x 1 update of the scalar kernel at hidden 128, B 128 with NaN parameters leave NaN in both LDS tiles
    of every CU they ran on; the smallest case (hidden 4, K = 2 and 4, N = 1, B 3) on the matrix-core entry right behind them must
    still equal its scalar result.  A k slot, a row or a sample of a block whose operand was masked on one side only would multiply
    0 x NaN here.  LDS contents surviving from one launch to the next is not guaranteed by anything, so this test can expose a
    half-masked tail but cannot prove there is none; the NaN-filled workspace of every Launch is the firm check."""
    c = T.CASES[3]
    want = _valu(engine, c)
    big = T.make_case((16, 4, 128, 0, 'tanh', 128, 1, 0, 1, 1, 1, 'small'))
    for k in T.ROWS:
        big[k] = np.full_like(big[k], np.nan)
    fill = G.Launch(engine, [big] * 512, extra=0)
    assert fill.run() == 0
    assert np.isnan(fill.out()['critic'][1:-1]).all()
    la = MfmaLaunch(engine, [G._case(c)[0]])
    assert la.run() == 0
    o = la.out()
    _same(o, want)
    assert np.isfinite(o['actor'][1, :la.Pa]).all() and np.isfinite(o['td'][1, :la.n]).all()


def test_td3_train_dense_mfma(engine):
    """TD3.train(ring, 14, iteration0=3, dense='mfma') reports 'fused-mfma' and leaves actor, critic, both targets and the losses
    exactly as dense='valu' does from the same seeds"""
    import serl_amd
    from serl_amd.actor import pack_actor, pack_critic
    dev = engine.device
    d, _ = G._case(T.CASES[0])
    res = {}
    for dense in ('valu', 'mfma'):
        torch.manual_seed(5)
        t = serl_amd.TD3(G._args(7, 3, 72, 3, 'tanh', 86, 'cpu'), engine)
        ring = serl_amd.DeviceReplay(400, dev, engine, 7, 3)
        ring.append_rows(torch.from_numpy(d['ring']))
        w0 = pack_actor(t.actor).numpy().copy()
        out = t.train(ring, 14, iteration0=3, rng=random.Random(3), generator=torch.Generator().manual_seed(9), dense=dense)
        assert t.last_path == ('fused-mfma' if dense == 'mfma' else 'fused')
        res[dense] = (pack_actor(t.actor).numpy(), pack_actor(t.actor_target).numpy(), pack_critic(t.critic).numpy(),
                      pack_critic(t.critic_target).numpy(), out)
        assert np.abs(res[dense][0] - w0).max() > T.MIN_MOVED
    for k in range(4):
        np.testing.assert_array_equal(res['mfma'][k], res['valu'][k])
    assert res['mfma'][4] == res['valu'][4] and np.isfinite(res['mfma'][4]['TD_loss']) and np.isfinite(res['mfma'][4]['PG_obj'])
    with pytest.raises(ValueError):
        t.train(ring, 14, iteration0=3, dense='mfma', fused=False)

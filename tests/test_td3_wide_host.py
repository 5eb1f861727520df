"""serl_td3_train_wide without a GPU: the layout of serl_td3_wide_desc, serl_td3_wide_work_bytes against the header's formula, the
argument errors of TD3.train(chunks=...), and the order in which workgroup 0 adds the chunks' partial actor gradients, restated in
float32: it is the chunked kernel's running sum bit for bit, and adding a chunk's main and CAPS passes to each other first is not."""
import ctypes
import random
import numpy as np
import pytest
import torch
import td3_64 as T
import td3_big as TB
import test_td3_big_host as BH


@pytest.fixture(scope='module')
def L():
    from serl_amd import _capi
    return _capi.lib()


def test_wide_layout_matches_the_ctypes_struct(L):
    from serl_amd import _capi
    want = _capi.expected_td3_wide_layout()
    got = (ctypes.c_int32 * (len(want) + 2))()
    assert L.serl_td3_wide_layout(got, len(got)) == len(want) == 5
    assert list(got)[:len(want)] == want == [24, 0, 8, 16, 20]
    assert L.serl_td3_wide_layout(None, 0) == len(want)
    assert L.serl_abi_version() == _capi.ABI_VERSION == 9
    for f in ('serl_td3_train_wide', 'serl_td3_wide_layout', 'serl_td3_wide_work_bytes'):
        assert f in _capi.EXPORTS and getattr(L, f)


def test_wide_work_bytes_follow_the_formula(L):
    """big + n_learners * (G * (3 gf + 4) * 4 + 16) with gf = max(actor, critic parameters) rounded up to 4; 0 exactly where big is 0"""
    wide, big = L.serl_td3_wide_work_bytes, L.serl_td3_big_work_bytes
    for S, A, H, Lh in ((7, 3, 72, 3), (2, 1, 4, 0), (16, 4, 128, 4), (1, 1, 4, 0)):
        gf = (max(L.serl_param_count(S, H, Lh, A), L.serl_td3_param_count(S, A)) + 3) & ~3
        for B in (1, 86, 128, 129, 256, 257, 384, 385, 512):
            G = (B + 127) // 128
            for K in (1, 3):
                w = wide(K, S, A, H, Lh, B)
                assert w == big(K, S, A, H, Lh, B) + K * (G * (3 * gf + 4) * 4 + 16) and w % 16 == 0, (S, A, H, Lh, B, K)
    for args in ((1, 7, 3, 72, 3, 0), (1, 7, 3, 72, 3, 513), (1, 7, 3, 72, 3, -1), (0, 7, 3, 72, 3, 256), (1, 7, 3, 132, 3, 256), (1, 7, 3, 6, 3, 256),
                 (1, 7, 3, 72, 5, 256), (1, 17, 3, 72, 3, 256), (1, 7, 5, 72, 3, 256), (1, 0, 3, 72, 3, 256)):
        assert big(*args) == 0 and wide(*args) == 0, args


def test_refusals_need_no_device(L):
    from serl_amd import _capi
    d = _capi.Td3Desc()
    st = (ctypes.c_int32 * 1)()
    ok = _capi.Td3WideDesc(rng=None, status=ctypes.addressof(st), dense=0)
    assert L.serl_td3_train_wide(None, ctypes.byref(d), None, None) == _capi.E_INVALID
    assert L.serl_td3_train_wide(None, ctypes.byref(d), ctypes.byref(_capi.Td3WideDesc(rng=None, status=None, dense=0)), None) == _capi.E_INVALID
    assert b'status' in L.serl_last_error()
    assert L.serl_td3_train_wide(None, ctypes.byref(d), ctypes.byref(_capi.Td3WideDesc(rng=None, status=ctypes.addressof(st), dense=2)), None) == _capi.E_INVALID
    assert L.serl_td3_train_wide(None, ctypes.byref(d), ctypes.byref(ok), None) == _capi.E_INVALID      # NULL context


@pytest.mark.parametrize('B', [86, 256, 512])
def test_train_chunks_argument_errors_come_before_any_draw(B):
    """an unknown `chunks` and chunks='parallel' with fused=False are ValueErrors, chunks='parallel' without a GPU a RuntimeError, each
    raised with `rng`, `generator` and python's global stream untouched; the default is 'serial': the eager loop as before"""
    from serl_amd import td3 as td3_mod
    t, ring = BH._learner(B)
    assert not t.fused_wide_supported('cpu') and td3_mod.CHUNKS == ('serial', 'parallel')
    rng, gen = random.Random(3), torch.Generator().manual_seed(9)
    s0, g0, m0 = rng.getstate(), gen.get_state().clone(), random.getstate()
    for err, kw in ((ValueError, dict(chunks='wide')), (ValueError, dict(chunks=None)), (ValueError, dict(chunks='parallel', fused=False)),
                    (RuntimeError, dict(chunks='parallel')), (RuntimeError, dict(chunks='parallel', fused=True)),
                    (RuntimeError, dict(chunks='parallel', dense='mfma')), (RuntimeError, dict(chunks='parallel', draws='device', seed=1))):
        with pytest.raises(err):
            t.train(ring, 3, iteration0=0, rng=rng, generator=gen, **kw)
        assert rng.getstate() == s0 and torch.equal(gen.get_state(), g0) and random.getstate() == m0, kw
    out = t.train(ring, 2, iteration0=0, rng=rng, generator=gen, chunks='serial')
    assert t.last_path == 'eager' and np.isfinite(out['TD_loss'])
    assert td3_mod._names('valu', wide=True) == ('serl_td3_train_wide', 'fused-wide')
    assert td3_mod._names('mfma', big=True, rng=True, wide=True) == ('serl_td3_train_wide', 'fused-mfma-wide-rng')
    assert td3_mod._names('mfma', big=True, rng=True) == ('serl_td3_train_big', 'fused-mfma-big-rng')


# ---- the reduce order, in float32 ------------------------------------------------------------------------------------------------------
def actor_partials32(d):
    """The first actor update of case d at its starting weights, in float32 as TB.td3_chunked32 computes a chunk: per chunk of 128
    samples the actor gradient of the main pass (-Q / B and the temporal CAPS term) and of the spatial CAPS pass, separately, each scaled
    by the minibatch's 1 / B and 1 / (B A).  -> [(main, caps)] per chunk, float32 arrays"""
    S, A, H, Lh, B = d['S'], d['A'], d['H'], d['L'], d['B']
    act = {'tanh': torch.tanh, 'elu': torch.nn.functional.elu, 'relu': lambda v: torch.nn.functional.leaky_relu(v, 0.01)}[d['act']]

    def taker(w):
        off = [0]

        def take(*shape):
            k = int(np.prod(shape))
            v = w[off[0]:off[0] + k].view(shape)
            off[0] += k
            return v
        return take

    def lnorm(y, g, be):
        return g * (y - y.mean(-1, keepdim=True)) / (y.std(-1, keepdim=True) + 1e-6) + be

    def actor_f(w, x):
        take = taker(w)
        W, b = take(H, S), take(H)
        h = act(x @ W.T + b)
        for _ in range(Lh):
            W, b, g, be = take(H, H), take(H), take(H), take(H)
            h = act(lnorm(h @ W.T + b, g, be))
        W, b = take(A, H), take(A)
        return torch.tanh(h @ W.T + b)

    def q1_f(w, x):
        take = taker(w[:w.numel() // 2])
        W, b, g, be = take(T.HC, S + A), take(T.HC), take(T.HC), take(T.HC)
        h = act(lnorm(x @ W.T + b, g, be))
        W, b, g, be = take(T.HC, T.HC), take(T.HC), take(T.HC), take(T.HC)
        h = act(lnorm(h @ W.T + b, g, be))
        W, b = take(1, T.HC), take(1)
        return h @ W.T + b

    t32 = lambda k: torch.from_numpy(np.asarray(d[k], np.float32)).clone()
    wa, wc, ring, cn = t32('actor').requires_grad_(True), t32('critic'), t32('ring'), t32('cn')
    rows = ring[torch.from_numpy(d['slots'][0].astype(np.int64))]
    out = []
    for b0 in range(0, B, TB.CHUNK):
        r = rows[b0:b0 + TB.CHUNK]
        state, action = r[:, :S], r[:, S:S + A]
        a_now = actor_f(wa, state)
        main = -q1_f(wc, torch.cat((state, a_now), 1)).sum() / B + T.CAPS['lambda_t'] * ((action - a_now) ** 2).sum() / (B * A)
        bar = actor_f(wa, state + cn[0, b0:b0 + TB.CHUNK] * T.CAPS['eps_sd'])
        caps = T.CAPS['lambda_s'] * ((action - bar) ** 2).sum() / (B * A)
        out.append(tuple(torch.autograd.grad(x, wa)[0].numpy().copy() for x in (main, caps)))
    return out


def chunked_sum(parts):
    """serl_td3_train_big: one vector; chunk 0's main pass writes it, every later pass adds its finished partial sum to what is there"""
    g = None
    for main, caps in parts:
        g = main.copy() if g is None else g + main
        g = g + caps
    return g


def reduced_sum(parts, slip=False):
    """serl_td3_train_wide's workgroup 0, from the partial vectors the workgroups left: M0 + C0 + M1 + C1 + .. left to right.
    slip: a chunk's main and CAPS passes added to each other first -- what one partial vector per workgroup would give"""
    if slip:
        g = parts[0][0] + parts[0][1]
        for main, caps in parts[1:]:
            g = g + (main + caps)
        return g
    g = parts[0][0] + parts[0][1]
    for main, caps in parts[1:]:
        g = g + main
        g = g + caps
    return g


CAPS_CASES = [c for c in TB.CASES if c[9] and c[:5] == TB.SHAPES[0]]


@pytest.mark.parametrize('c', CAPS_CASES, ids=T.case_id)
def test_reduce_order_is_the_chunked_order_and_the_slip_is_seen(c):
    """with CAPS on, on cases tests/test_gpu_td3_wide.py compares bit for bit: the stated reduce order gives the chunked kernel's sum
    exactly; main + CAPS added inside the chunk first changes at least one bit of the actor gradient, so that comparison sees it"""
    d = TB.make_case(c)
    parts = actor_partials32(d)
    assert len(parts) == (d['B'] + 127) // 128 >= 2 and all(p.dtype == np.float32 for pair in parts for p in pair)
    want = chunked_sum(parts)
    np.testing.assert_array_equal(reduced_sum(parts), want)
    slipped = reduced_sum(parts, slip=True)
    assert (slipped.view(np.uint32) != want.view(np.uint32)).any()
    np.testing.assert_allclose(slipped, want, rtol=1e-4, atol=1e-7)


def test_the_caps_cases_are_on_the_gpu_grid():
    assert len(CAPS_CASES) >= 3 and {c[5] for c in CAPS_CASES} <= set(TB.BATCHES)

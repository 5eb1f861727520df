"""serl_td3_train_big without a GPU: the layout of serl_td3_big_desc, the table of serl_td3_big_work_bytes, the slot draw at minibatches
of more than 128 rows against its definition, the argument errors of TD3.train for such a minibatch, and the cases of
tests/test_gpu_td3_big.py chosen on the CPU: float32 torch meets td3_64's bound on each, the slips a chunk loop invites do not."""
import ctypes
import functools
import random
import types
import numpy as np
import pytest
import torch
import td3_64 as T
import td3_big as TB


@pytest.fixture(scope='module')
def L():
    from serl_amd import _capi
    return _capi.lib()


def test_big_layout_matches_the_ctypes_struct(L):
    from serl_amd import _capi
    want = _capi.expected_td3_big_layout()
    got = (ctypes.c_int32 * (len(want) + 2))()
    assert L.serl_td3_big_layout(got, len(got)) == len(want) == 4
    assert list(got)[:len(want)] == want == [16, 0, 8, 12]
    assert L.serl_td3_big_layout(None, 0) == len(want)
    assert L.serl_abi_version() == _capi.ABI_VERSION == 9
    for f in ('serl_td3_train_big', 'serl_td3_big_layout', 'serl_td3_big_work_bytes', 'serl_td3_rng_fill_big'):
        assert f in _capi.EXPORTS and getattr(L, f)


def test_big_work_bytes_table(L):
    big, old = L.serl_td3_big_work_bytes, L.serl_td3_work_bytes
    for B in (1, 86, 128):
        assert big(1, 7, 3, 72, 3, B) == old(1, 7, 3, 72, 3, B) > 0
    one = big(1, 7, 3, 72, 3, 128)
    chunk = big(1, 7, 3, 72, 3, 129) - one                  # inputs and tapes of one more chunk
    assert chunk > 0 and chunk % 4 == 0
    for B, chunks in ((129, 2), (256, 2), (257, 3), (384, 3), (385, 4), (512, 4)):
        assert big(1, 7, 3, 72, 3, B) == one + (chunks - 1) * chunk, B
        assert big(3, 7, 3, 72, 3, B) == 3 * big(1, 7, 3, 72, 3, B)
    assert big(1, 16, 4, 128, 4, 512) > 0 and big(1, 1, 1, 4, 0, 512) > 0
    assert big(1, 7, 3, 72, 3, 0) == 0 and big(1, 7, 3, 72, 3, 513) == 0 and big(1, 7, 3, 72, 3, -1) == 0 and big(0, 7, 3, 72, 3, 256) == 0
    for shape in ((7, 3, 132, 3), (7, 3, 6, 3), (7, 3, 72, 5), (17, 3, 72, 3), (7, 5, 72, 3), (0, 3, 72, 3)):
        assert old(1, *shape, 86) == 0 and big(1, *shape, 256) == 0, shape
    assert old(1, 7, 3, 72, 3, 129) == 0 and old(1, 7, 3, 72, 3, 512) == 0


def _words(L, seed, c0, c1, c2, c3):
    w = (ctypes.c_uint32 * 4)()
    L.serl_host_philox(seed, c0, c1, c2, c3, w)
    return list(w)


@pytest.mark.parametrize('B,n_rows', [(129, 129), (129, 640), (300, 301), (300, 5000), (512, 512), (512, 640)])
def test_slot_draw_follows_its_definition_past_128(L, B, n_rows):
    """Floyd's algorithm recomputed literally from serl_host_philox words (stream 2, block 0, index = step): a full ring is a permutation"""
    seed, learner, it = 0x1234567890ABCDEF, 3, 17
    out = np.zeros(B, np.int32)
    assert L.serl_host_td3_slots(seed, learner, it, n_rows, B, out.ctypes.data) == 0
    want = []
    for i in range(B):
        j = n_rows - B + i
        w = _words(L, seed, learner, it, i, 2 << 16)
        t = (((w[0] << 32) | w[1]) * (j + 1)) >> 64
        want.append(j if t in want else t)
    assert out.tolist() == want
    assert len(set(want)) == B and min(want) >= 0 and max(want) < n_rows
    if B == n_rows:
        assert sorted(want) == list(range(B))


def test_refusals_need_no_device(L):
    """NULL and out-of-range arguments of the new entries are refused before the context is looked at"""
    from serl_amd import _capi
    d = _capi.Td3Desc()
    bd = _capi.Td3BigDesc(rng=None, dense=0)
    assert L.serl_td3_train_big(None, ctypes.byref(d), ctypes.byref(bd), None) == _capi.E_INVALID
    assert L.serl_td3_train_big(None, ctypes.byref(d), None, None) == _capi.E_INVALID
    bd.dense = 2
    assert L.serl_td3_train_big(None, ctypes.byref(d), ctypes.byref(bd), None) == _capi.E_INVALID
    rd = _capi.Td3RngDesc(seed=1, n_rows=600, learner0=0, dense=0, caps=1)
    assert L.serl_td3_rng_fill_big(None, ctypes.byref(rd), 0, 7, 3, 256, 0, 4, 2, None, None, None, None) == _capi.E_INVALID


def _learner(B):
    import serl_amd
    args = types.SimpleNamespace(state_dim=7, action_dim=3, hidden_size=8, num_layers=1, activation_actor='tanh', device='cpu', individual_bs=700,
                                 lr=1e-3, gamma=0.98, tau=0.05, noise_sd=0.2, noise_clip=0.3, policy_update_freq=2, use_caps=True, batch_size=B)
    t = serl_amd.TD3(args)
    ring = serl_amd.DeviceReplay(700, 'cpu', None, 7, 3)
    ring.append_rows(torch.randn(640, 2 * 7 + 3 + 3))
    return t, ring


@pytest.mark.parametrize('B', [129, 256, 512])
def test_train_large_batch_argument_errors_come_before_any_draw(B):
    """without a GPU fused=True, dense='mfma' and draws='device' are RuntimeErrors for a large minibatch, raised with `rng`, `generator` and
    python's global stream untouched; the default call is the eager loop as before"""
    t, ring = _learner(B)
    assert not t.fused_supported('cpu') and not t.fused_big_supported('cpu')
    rng, gen = random.Random(3), torch.Generator().manual_seed(9)
    s0, g0, m0 = rng.getstate(), gen.get_state().clone(), random.getstate()
    for kw in (dict(fused=True), dict(dense='mfma'), dict(draws='device', seed=1), dict(draws='device', seed=1, dense='mfma'), dict(fused=True, dense='mfma')):
        with pytest.raises(RuntimeError):
            t.train(ring, 3, iteration0=0, rng=rng, generator=gen, **kw)
        assert rng.getstate() == s0 and torch.equal(gen.get_state(), g0) and random.getstate() == m0, kw
    out = t.train(ring, 2, iteration0=0, rng=rng, generator=gen)
    assert t.last_path == 'eager' and np.isfinite(out['TD_loss'])
    assert rng.getstate() != s0


def test_group_still_refuses_a_large_batch():
    import serl_amd
    t, ring = _learner(256)
    with pytest.raises(RuntimeError):
        serl_amd.TD3Group([t]).train([ring], 2, iteration0=0, seed=1)


# ---- the cases of the GPU test, chosen on the CPU ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(c):
    d = TB.make_case(c)
    return d, T.td3_literal(d)


def test_grid_covers_the_chunk_paths():
    assert sorted({c[5] for c in TB.CASES}) == [129, 192, 256, 257, 300, 512]
    for B in TB.BATCHES:
        assert {c[:5] for c in TB.CASES if c[5] == B} == set(TB.SHAPES)
        assert {c[11] for c in TB.CASES if c[5] == B} == {'big', 'small'}
    assert {c[9] for c in TB.CASES} == {0, 1} and {c[10] for c in TB.CASES} == {0, 1} and {c[6] for c in TB.CASES} == {2, 3}
    d = TB.make_case(TB.CASES[0])
    assert d['ring'].shape[0] == TB.RING_ROWS and (d['slots'][:, 128:] >= TB.RING_ROWS - TB.LOUD_ROWS).all() and (d['slots'][:, :128] < 480).all()
    assert all(len(set(r.tolist())) == d['B'] for r in d['slots'])


@pytest.mark.parametrize('c', TB.CASES, ids=T.case_id)
def test_float32_meets_the_bound_and_the_slips_do_not(c):
    """td3_literal in float32 and the chunked summation in float32 pass td3_64.check against the float64 run (so the bound can be met
    at these shapes); the norm clip is active in every critic step of a 'big' case and in none of a 'small' one; each planted slip --
    the last chunk's gradient dropped, the means divided by 128, the padding of a partial chunk let into the sums -- fails the check"""
    d, ref = _case(c)
    assert all(ref['clip_c']) if d['rew'] == 'big' else not any(ref['clip_c']), ref['clip_c']
    T.check(T.td3_literal(d, dtype=torch.float32), ref, d, 'float32 torch ' + T.case_id(c))
    T.check(TB.td3_chunked32(d), ref, d, 'chunked float32 ' + T.case_id(c))
    for slip in TB.SLIPS:
        if TB.slip_applies(d, slip):
            with pytest.raises(AssertionError):
                T.check(TB.td3_chunked32(d, slip), ref, d, '%s %s' % (slip, T.case_id(c)))

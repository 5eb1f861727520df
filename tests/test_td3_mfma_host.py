"""serl_td3_train_mfma and TD3.train(dense=...) as far as they go without a GPU: the export, the refusals that need no device, the
keyword's validation before any draw, and the ABI left as it was."""
import ctypes
import os
import random
import re
import types
import numpy as np
import pytest
import torch
import td3_64 as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(S, A, H, L, act, B, caps=True):
    return types.SimpleNamespace(state_dim=S, action_dim=A, hidden_size=H, num_layers=L, activation_actor=act, device='cpu', individual_bs=300,
                                 lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP, policy_update_freq=2,
                                 use_caps=caps, batch_size=B)


def test_library_exports_the_mfma_entry():
    from serl_amd import _capi
    L = _capi.lib()
    assert 'serl_td3_train_mfma' in _capi.EXPORTS and hasattr(L, 'serl_td3_train_mfma')
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert re.search(r'int serl_td3_train_mfma\(serl_ctx \*ctx, const serl_td3_desc \*desc, void \*stream\);', hdr)
    assert 'bit for bit' in hdr[hdr.index('int serl_td3_train('):hdr.index('int serl_td3_train_mfma(')]


def test_abi_version_and_layout_are_unchanged():
    from serl_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert re.search(r'#define SERL_ABI_VERSION 9\b', hdr) and L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == len(_capi.expected_layout()) == 62
    want = _capi.expected_td3_layout()
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_td3_layout(got, len(want)) == len(want) and list(got) == want
    # the workspace: gradients (the longer row, rounded up to 4) | four inputs [20][128] | the tapes of the actor and of a critic twin
    S, A, H, Ly = 7, 3, 72, 3
    grads = (max(T.actor_param_count(S, A, H, Ly), T.critic_param_count(S, A)) + 3) & ~3
    tape = lambda layers, width: (2 * layers * width + layers) * 128
    assert L.serl_td3_work_bytes(1, S, A, H, Ly, 86) == 4 * (grads + 4 * 20 * 128 + tape(Ly + 2, H) + tape(3, 64))


def test_null_and_bad_arguments_are_refused_like_serl_td3_train():
    """a NULL context or descriptor: SERL_E_INVALID; and without a device the same descriptors get the same code from both entries"""
    from serl_amd import _capi
    L = _capi.lib()
    assert L.serl_td3_train_mfma(None, None, None) == _capi.E_INVALID
    assert 'serl_td3_train_mfma' in L.serl_last_error().decode()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def desc(**kw):
        d = _capi.Td3Desc(state_dim=7, action_dim=3, hidden=72, num_layers=3, activation=0, n_learners=1, batch=86, n_updates=2, capacity=100,
                          slot_cols=86, policy_update_freq=2, iteration0=0, update_actor_target=1, lr=1e-3, gamma=0.99, tau=0.005, noise_sd=0.2,
                          noise_clip=0.5, lambda_s=0.5, lambda_t=0.1, eps_sd=0.05, max_grad_norm=10.0, actor=p, actor_target=p, actor_m=p, actor_v=p,
                          actor_stride=20000, critic=p, critic_target=p, critic_m=p, critic_v=p, critic_stride=11000, adam_steps=p, ring=p,
                          slots=p, target_noise=p, caps_noise=p, td_loss=p, pg_loss=p, loss_stride=2, work=p, work_bytes=1 << 30)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    ctx = ctypes.c_void_p(buf.ctypes.data)          # never dereferenced: every call below is refused by the argument checks
    assert L.serl_td3_train_mfma(None, ctypes.byref(desc()), None) == _capi.E_INVALID
    assert L.serl_td3_train_mfma(ctx, None, None) == _capi.E_INVALID
    for kw in (dict(actor=None), dict(work=None), dict(state_dim=0), dict(activation=3), dict(n_updates=-1), dict(slot_cols=85), dict(lr=0.0),
               dict(tau=1.5), dict(actor_stride=100), dict(loss_stride=1), dict(work_bytes=8), dict(ring_stride=-1), dict(lr=float('nan')),
               dict(hidden=132), dict(hidden=70), dict(num_layers=5), dict(state_dim=17), dict(action_dim=5), dict(batch=129, slot_cols=129),
               dict(hidden=132, actor=None), dict(hidden=132, work_bytes=8)):          # (the last two: which refusal comes first)
        rc = L.serl_td3_train(ctx, ctypes.byref(desc(**kw)), None)
        assert rc in (_capi.E_INVALID, _capi.E_UNSUPPORTED), kw
        assert L.serl_td3_train_mfma(ctx, ctypes.byref(desc(**kw)), None) == rc, kw


def test_train_rejects_an_unknown_dense_before_any_draw():
    """dense='tensor', and dense='mfma' with fused=False: ValueError with the states of `rng` and `generator` as they were; the
    default dense='valu' on a CPU ring still runs the eager loop"""
    import serl_amd
    d = T.make_case((7, 3, 32, 2, 'elu', 24, 2, 3, 13, 1, 1, 'small'))
    torch.manual_seed(3)
    t = serl_amd.TD3(_args(7, 3, 32, 2, 'elu', 24), None)
    ring = serl_amd.DeviceReplay(300, 'cpu', None, 7, 3)
    ring.append_rows(torch.from_numpy(d['ring']))
    rng, gen = random.Random(11), torch.Generator().manual_seed(12)
    s0, g0 = rng.getstate(), gen.get_state().clone()
    for kw in (dict(dense='tensor'), dict(dense='MFMA'), dict(dense=None), dict(dense='mfma', fused=False)):
        with pytest.raises(ValueError):
            t.train(ring, 5, iteration0=3, rng=rng, generator=gen, **kw)
        assert rng.getstate() == s0 and torch.equal(gen.get_state(), g0), kw
    assert t.last_path is None
    with pytest.raises(RuntimeError):               # no device here: the kernel cannot run, and 'mfma' never means the eager loop
        t.train(ring, 5, iteration0=3, rng=rng, generator=gen, dense='mfma')
    assert rng.getstate() == s0 and torch.equal(gen.get_state(), g0)
    out = t.train(ring, 5, iteration0=3, rng=rng, generator=gen, dense='valu')
    assert t.last_path == 'eager' and np.isfinite(out['TD_loss'])
    assert rng.getstate() != s0 and not torch.equal(gen.get_state(), g0)

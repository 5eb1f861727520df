"""The host side of the fused TD3 learner's in-kernel draws (serl_td3_train_rng, csrc/serl_rng.h): the descriptor's layout, the slot
draw compiled for the host (serl_host_td3_slots: Floyd's algorithm on Philox words) -- distinct rows, in range, a function of its
arguments, uniform over the subsets -- and the argument errors of TD3.train(draws=...), which come before any draw."""
import ctypes
import itertools
import random
import types
import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def L():
    from serl_amd import _capi
    return _capi.lib()


def slots(L, seed, learner, iteration, n_rows, B):
    out = np.full(B + 2, -7, np.int32)
    assert L.serl_host_td3_slots(seed, learner, iteration, n_rows, B, out[1:].ctypes.data) == 0
    assert out[0] == -7 and out[-1] == -7
    return out[1:-1].copy()


def test_rng_layout_matches_the_ctypes_struct(L):
    from serl_amd import _capi
    want = _capi.expected_td3_rng_layout()
    got = (ctypes.c_int32 * (len(want) + 2))()
    n = L.serl_td3_rng_layout(got, len(want) + 2)
    assert n == len(want) == 6 and list(got)[:n] == want
    assert want == [24, 0, 8, 12, 16, 20]
    assert L.serl_td3_rng_layout(None, 0) == n


@pytest.mark.parametrize('B', [1, 17, 128])
def test_full_ring_is_a_permutation(L, B):
    for it in (1, 2, 77):
        assert sorted(slots(L, 12345, 0, it, B, B)) == list(range(B))


@pytest.mark.parametrize('n_rows,B', [(2, 1), (129, 128), (1000000, 86)])
def test_rows_distinct_and_in_range(L, n_rows, B):
    seen = set()
    for it in range(1, 40):
        s = slots(L, 2**63 + 11, 3, it, n_rows, B)
        assert len(set(s.tolist())) == B and s.min() >= 0 and s.max() < n_rows
        seen.add(tuple(s))
    assert len(seen) > 1


def test_iterations_and_learners_differ_and_the_draw_is_pure(L):
    a = slots(L, 99, 0, 1, 1000, 86)
    np.testing.assert_array_equal(a, slots(L, 99, 0, 1, 1000, 86))
    assert (a != slots(L, 99, 0, 2, 1000, 86)).any()
    assert (a != slots(L, 99, 1, 1, 1000, 86)).any()
    assert (a != slots(L, 100, 0, 1, 1000, 86)).any()
    assert (a != slots(L, 99 + 2**32, 0, 1, 1000, 86)).any()            # the high word of the seed is part of the key


def test_slot_draw_follows_its_definition(L):
    """Floyd's algorithm as include/serl_amd.h states it, recomputed from serl_host_philox words in python integers"""
    seed, learner, it, n_rows, B = 0x123456789ABCDEF, 4, 9, 50, 33
    w = (ctypes.c_uint32 * 4)()
    want = []
    for i in range(B):
        j = n_rows - B + i
        L.serl_host_philox(seed, learner, it, i, (2 << 16) | 0, w)
        t = (((w[0] << 32) | w[1]) * (j + 1)) >> 64
        want.append(j if t in want else t)
    assert slots(L, seed, learner, it, n_rows, B).tolist() == want
    assert len(set(want)) == B and any(want[i] == n_rows - B + i for i in range(B))     # (the collision branch is taken at this size)


def test_host_slots_refusals(L):
    from serl_amd import _capi
    out = np.zeros(4, np.int32)
    assert L.serl_host_td3_slots(1, 0, 1, 3, 4, out.ctypes.data) == _capi.E_INVALID
    assert L.serl_host_td3_slots(1, 0, 1, 3, 0, out.ctypes.data) == _capi.E_INVALID
    assert L.serl_host_td3_slots(1, 0, 1, 3, 2, None) == _capi.E_INVALID
    assert (out == 0).all()


def test_uniform_over_rows_and_subsets(L):
    """n_rows 8, B 3, 20 000 iterations: every row's inclusion frequency within 5 binomial standard deviations of 3 / 8
    (5 sqrt(3/8 * 5/8 / 20000) = 0.0171), and every one of the 56 subsets occurs"""
    n, rows = 20000, 8
    count = np.zeros(rows)
    subsets = set()
    for it in range(1, n + 1):
        s = slots(L, 20261019, 0, it, rows, 3)
        count[s] += 1
        subsets.add(frozenset(s.tolist()))
    freq = count / n
    print('TD3_RNG inclusion frequencies', freq, 'subsets', len(subsets))
    assert np.abs(freq - 3 / 8).max() <= 0.0172, freq
    assert subsets == {frozenset(c) for c in itertools.combinations(range(rows), 3)}


def _learner(B=16, H=8):
    import serl_amd
    a = types.SimpleNamespace(state_dim=7, action_dim=3, hidden_size=H, num_layers=1, activation_actor='tanh', device='cpu', individual_bs=64,
                              lr=1e-3, gamma=0.98, tau=0.05, noise_sd=0.2, noise_clip=0.3, policy_update_freq=2, use_caps=True, batch_size=B)
    t = serl_amd.TD3(a, None)
    ring = serl_amd.DeviceReplay(64, 'cpu', None, 7, 3)
    ring.append_rows(torch.zeros(32, 2 * 7 + 3 + 3))
    return t, ring


def test_train_draws_argument_errors_come_before_any_draw():
    """an unknown draws, draws='device' without a seed / with fused=False / with a seed or learner out of range: ValueError; on a device the
    kernel does not run (a CPU ring): RuntimeError, never the eager loop -- python's `random`, `rng` and the generator as they were"""
    t, ring = _learner()
    assert len(ring) == 32
    rng, gen = random.Random(4), torch.Generator().manual_seed(4)
    s0, g0, m0 = rng.getstate(), gen.get_state().clone(), random.getstate()
    for kw, err in ((dict(draws='gpu'), ValueError), (dict(draws='device'), ValueError), (dict(draws='device', seed=1, fused=False), ValueError),
                    (dict(draws='device', seed=-1), ValueError), (dict(draws='device', seed=2**64), ValueError),
                    (dict(draws='device', seed=1.5), ValueError), (dict(draws='device', seed=1, learner=-1), ValueError),
                    (dict(draws='device', seed=1), RuntimeError), (dict(draws='device', seed=1, dense='mfma'), RuntimeError),
                    (dict(draws='device', seed=1, fused=True), RuntimeError)):
        with pytest.raises(err):
            t.train(ring, 4, iteration0=0, rng=rng, generator=gen, **kw)
        assert rng.getstate() == s0 and torch.equal(gen.get_state(), g0) and random.getstate() == m0, kw
        assert t.last_path is None
    out = t.train(ring, 2, iteration0=0, rng=rng, generator=gen)            # the default still draws on the host and runs
    assert t.last_path == 'eager' and np.isfinite(out['TD_loss']) and rng.getstate() != s0 and not torch.equal(gen.get_state(), g0)

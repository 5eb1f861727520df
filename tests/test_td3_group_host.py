"""The host side of a group of TD3 learners in one launch (serl_td3_train_group, serl_amd.TD3Group): the layout of the two new structs
against their ctypes mirrors with everything older where it was, and every argument error of TD3Group, raised before any device work --
the rings here are stubs on the CPU, where the only thing train() can do after its checks is refuse."""
import copy
import ctypes
import types
import pytest
import torch


@pytest.fixture(scope='module')
def L():
    from serl_amd import _capi
    return _capi.lib()


def test_group_layout_matches_the_ctypes_structs(L):
    from serl_amd import _capi
    want = _capi.expected_td3_group_layout()
    got = (ctypes.c_int32 * (len(want) + 2))()
    n = L.serl_td3_group_layout(got, len(want) + 2)
    assert n == len(want) == 24 and list(got)[:n] == want
    # the row: ring, seed, seven i32 and a pad, eight f32; the descriptor: two pointers, dense, caps
    assert want == [80, 0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 24, 0, 8, 16, 20]
    assert L.serl_td3_group_layout(None, 0) == n
    assert ctypes.sizeof(_capi.Td3LearnerRow) % 8 == 0
    assert 'serl_td3_train_group' in _capi.EXPORTS and 'serl_td3_group_layout' in _capi.EXPORTS and hasattr(L, 'serl_td3_train_group')


def test_nothing_older_has_moved(L):
    from serl_amd import _capi
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    for fn, want in ((L.serl_td3_layout, _capi.expected_td3_layout()), (L.serl_td3_rng_layout, _capi.expected_td3_rng_layout())):
        got = (ctypes.c_int32 * len(want))()
        assert fn(got, len(want)) == len(want) and list(got) == want
    assert _capi.expected_td3_rng_layout() == [24, 0, 8, 12, 16, 20]
    assert ctypes.sizeof(_capi.Td3Desc) == 288 and _capi.Td3Desc.work_bytes.offset == 280


def test_launch_wide_refusals_need_no_device(L):
    """a NULL context or descriptor is refused before anything else, like serl_td3_train_rng"""
    from serl_amd import _capi
    g = _capi.Td3GroupDesc()
    assert L.serl_td3_train_group(None, ctypes.byref(_capi.Td3Desc()), ctypes.byref(g), None) == _capi.E_INVALID
    assert b'serl_td3_train_group' in L.serl_last_error()


def _args(**kw):
    a = dict(state_dim=7, action_dim=3, hidden_size=8, num_layers=1, activation_actor='tanh', device='cpu', individual_bs=64, lr=1e-3, gamma=0.98,
             tau=0.05, noise_sd=0.2, noise_clip=0.3, policy_update_freq=2, use_caps=True, batch_size=16)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _learner(engine=None, **kw):
    import serl_amd
    return serl_amd.TD3(_args(**kw), engine)


def _ring(rows=32, S=7, A=3, capacity=64):
    import serl_amd
    ring = serl_amd.DeviceReplay(capacity, 'cpu', None, S, A)
    if rows:
        ring.append_rows(torch.zeros(rows, 2 * S + A + 3))
    return ring


def test_group_init_names_the_first_differing_field():
    import serl_amd
    assert serl_amd.TD3Group is serl_amd.td3.TD3Group and 'TD3Group' in serl_amd.__all__
    with pytest.raises(ValueError, match='no learners'):
        serl_amd.TD3Group([])
    with pytest.raises(ValueError, match='not a serl_amd.TD3'):
        serl_amd.TD3Group([_learner(), object()])
    for kw, field in ((dict(state_dim=6), 'state_dim'), (dict(action_dim=2), 'action_dim'), (dict(hidden_size=12), 'hidden_size'),
                      (dict(num_layers=2), 'num_layers'), (dict(activation_actor='elu'), 'activation_actor'), (dict(batch_size=17), 'batch_size'),
                      (dict(use_caps=False), 'use_caps'), (dict(hidden_size=12, batch_size=17), 'hidden_size'),
                      (dict(state_dim=6, use_caps=False), 'state_dim')):
        with pytest.raises(ValueError, match='learner 2 differs from learner 0 in %s' % field):
            serl_amd.TD3Group([_learner(), _learner(), _learner(**kw)])
    with pytest.raises(ValueError, match='learner 1 differs from learner 0 in device'):
        serl_amd.TD3Group([_learner(types.SimpleNamespace(device='cuda:0', ctx=None)), _learner(types.SimpleNamespace(device='cuda:1', ctx=None))])
    g = serl_amd.TD3Group([_learner(), _learner(activation_actor='TANH', lr=3e-4, gamma=0.9, policy_update_freq=3)])
    assert len(g) == 2          # hyper-parameters may differ; the activation's spelling does not count


BAD_TRAIN = [
    (dict(replays=1), 'rings for'), (dict(replays=3), 'rings for'),
    (dict(n_updates=[4]), 'n_updates'), (dict(n_updates=[4, 4, 4]), 'n_updates'), (dict(iteration0=[0, 1, 2]), 'iteration0'),
    (dict(seed=[1]), 'seed'), (dict(key=[0, 1, 2]), 'key'), (dict(champion_target=[True]), 'champion_target'),
    (dict(ring1=dict(S=6)), 'learner 1: the ring holds rows'), (dict(ring1=dict(A=2)), 'learner 1: the ring holds rows'),
    (dict(ring1=dict(rows=15)), 'learner 1: 15 rows in the ring'), (dict(ring1=dict(rows=0)), 'learner 1: 0 rows in the ring'),
    (dict(n_updates=-1), 'learner 0: n_updates'), (dict(n_updates=[4, -2]), 'learner 1: n_updates'), (dict(n_updates=2.5), 'n_updates'),
    (dict(iteration0=-1), 'learner 0: iteration0'), (dict(iteration0=[0, 2**31 - 5]), 'learner 1: iteration0'),
    (dict(seed=-1), 'seed'), (dict(seed=[1, 2**64]), 'learner 1'), (dict(seed=1.5), 'seed'), (dict(seed=None), 'seed'),
    (dict(key=[0, -1]), 'learner 1: key'), (dict(key=[2**31 - 1, 0]), 'learner 0: key'), (dict(key=[0, 1.0]), 'learner 1: key'),
    (dict(seed=[5, 6], key=[3, 3]), None), (dict(seed=[5, 5], key=[3, 3]), 'learners 0 and 1 share'),
    (dict(seed=5, key=7), 'share'),
    (dict(dense='fast'), 'dense'), (dict(dense=None), 'dense'),
]


@pytest.mark.parametrize('case', BAD_TRAIN, ids=lambda c: '-'.join('%s=%s' % kv for kv in c[0].items()).replace(' ', ''))
def test_group_train_value_errors_come_before_any_device_work(case, monkeypatch):
    """wrong lengths, ring dims, a ring below one minibatch, negative counts, seeds and keys out of range, a shared (seed, key), an unknown
    dense: ValueError with the learners untouched.  The rings are on the CPU and the learners have no engine, so a check that came after
    device work could not have been reached; (seed [5, 6], key [3, 3]) is the one row here that is fine and ends at the device check."""
    import serl_amd
    from serl_amd import _capi
    kw, msg = case
    kw = dict(kw)
    learners = [_learner(), _learner(lr=2e-3)]
    before = [copy.deepcopy(t.actor.state_dict()) for t in learners]
    group = serl_amd.TD3Group(learners)
    n_rings = kw.pop('replays', 2)
    rings = [_ring() for _ in range(n_rings)]
    if 'ring1' in kw:
        rings[1] = _ring(**kw.pop('ring1'))
    monkeypatch.setattr(_capi, 'lib', lambda: pytest.fail('the library was reached'))
    call = dict(n_updates=4, iteration0=0, seed=[1, 2])
    call.update(kw)
    n_updates = call.pop('n_updates')
    with pytest.raises(ValueError if msg is not None else RuntimeError, match=msg):
        group.train(rings, n_updates, **call)
    for t, b in zip(learners, before):
        assert t.last_path is None and all(torch.equal(v, b[k]) for k, v in t.actor.state_dict().items())


def test_group_train_without_a_gpu_is_an_error_not_the_eager_loop():
    """valid arguments on CPU rings: RuntimeError (TD3.train would loop update_parameters here); so does a shape the kernel is not compiled
    for -- its work size is 0 -- wherever the rings are"""
    import serl_amd
    for kw in (dict(), dict(hidden_size=6)):
        learners = [_learner(**kw), _learner(**kw)]
        before = [copy.deepcopy(t.critic.state_dict()) for t in learners]
        group = serl_amd.TD3Group(learners)
        for dense in ('valu', 'mfma'):
            with pytest.raises(RuntimeError, match='no eager fall-back'):
                group.train([_ring(), _ring()], [4, 0], iteration0=[0, 3], seed=9, dense=dense)
        for t, b in zip(learners, before):
            assert t.last_path is None and all(torch.equal(v, b[k]) for k, v in t.critic.state_dict().items())
    from serl_amd import _capi
    assert _capi.lib().serl_td3_work_bytes(2, 7, 3, 6, 1, 16) == 0

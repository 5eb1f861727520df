"""The host side of groups of TD3 learners on minibatches of up to 512 rows (serl_td3_train_group_big, serl_td3_train_group_wide,
TD3Group.train(chunks=...)): the two new symbols with nothing older moved, their refusals without a device, the time-out codes a wide
group reports in the row status, and the argument errors of TD3Group.train -- on stub CPU rings, as tests/test_td3_group_host.py builds
them, where the only thing train() can do after its checks is refuse the device."""
import copy
import ctypes
import pytest
import torch
import test_td3_group_host as GH

ENTRIES = ('serl_td3_train_group_big', 'serl_td3_train_group_wide')


@pytest.fixture(scope='module')
def L():
    from serl_amd import _capi
    return _capi.lib()


def test_the_library_exports_both_entries(L):
    from serl_amd import _capi
    for f in ENTRIES:
        assert f in _capi.EXPORTS and getattr(L, f)
        assert getattr(L, f).argtypes == L.serl_td3_train_group.argtypes and getattr(L, f).restype is ctypes.c_int


def test_nothing_older_has_moved(L):
    """two symbols and four enumerators more: the ABI version and every TD3 layout are where they were"""
    from serl_amd import _capi
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION and all(f in _capi.EXPORTS for f in ENTRIES)
    for fn, want, literal in ((L.serl_td3_group_layout, _capi.expected_td3_group_layout(),
                               [80, 0, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68, 72, 76, 24, 0, 8, 16, 20]),
                              (L.serl_td3_big_layout, _capi.expected_td3_big_layout(), [16, 0, 8, 12]),
                              (L.serl_td3_wide_layout, _capi.expected_td3_wide_layout(), [24, 0, 8, 16, 20])):
        got = (ctypes.c_int32 * (len(want) + 2))()
        assert fn(got, len(got)) == len(want) and list(got)[:len(want)] == want == literal
    assert ctypes.sizeof(_capi.Td3Desc) == 288 and ctypes.sizeof(_capi.Td3LearnerRow) == 80 and ctypes.sizeof(_capi.Td3GroupDesc) == 24


@pytest.mark.parametrize('entry', ENTRIES)
def test_refusals_need_no_device(L, entry):
    """a NULL context or descriptor is E_INVALID before anything else, and the message names the entry"""
    from serl_amd import _capi
    fn, g = getattr(L, entry), _capi.Td3GroupDesc()
    assert fn(None, ctypes.byref(_capi.Td3Desc()), ctypes.byref(g), None) == _capi.E_INVALID
    assert entry.encode() + b':' in L.serl_last_error()
    assert L.serl_td3_train_group(None, ctypes.byref(_capi.Td3Desc()), ctypes.byref(g), None) == _capi.E_INVALID
    assert entry.encode() not in L.serl_last_error()
    assert fn(None, None, ctypes.byref(g), None) == _capi.E_INVALID
    assert entry.encode() + b':' in L.serl_last_error()


def test_time_out_codes_are_distinct_from_the_row_checks():
    from serl_amd import _capi
    rows, wide = _capi.TD3_ROW_STATUS, _capi.TD3_WIDE_STATUS
    assert sorted(wide) == [0, 1, 2, 3, 4] and set(range(7)) <= set(rows)
    assert _capi.TD3_ROW_TIMEOUTS == (17, 18, 19, 20) and sorted(rows) == list(range(7)) + [17, 18, 19, 20]
    for s, code in zip((1, 2, 3, 4), _capi.TD3_ROW_TIMEOUTS):
        assert code > 6 and 'hand-over %s' % 'ABCD'[s - 1] in rows[code] and 'ran out of time' in rows[code]
        assert wide[s] in rows[code]
    assert len(set(rows.values())) == len(rows)


def test_names_of_the_group_launches():
    from serl_amd import td3 as M
    assert M._names('valu', group=True) == ('serl_td3_train_group', 'fused-group-rng')
    assert M._names('mfma', group=True) == ('serl_td3_train_group', 'fused-mfma-group-rng')
    assert M._names('valu', big=True, group=True) == ('serl_td3_train_group_big', 'fused-big-group-rng')
    assert M._names('mfma', big=True, group=True) == ('serl_td3_train_group_big', 'fused-mfma-big-group-rng')
    assert M._names('valu', group=True, wide=True) == ('serl_td3_train_group_wide', 'fused-wide-group-rng')
    assert M._names('mfma', big=True, group=True, wide=True) == ('serl_td3_train_group_wide', 'fused-mfma-wide-group-rng')


def _group(batch_size, K=2):
    import serl_amd
    learners = [GH._learner(batch_size=batch_size, lr=1e-3 * (1 + i)) for i in range(K)]
    return serl_amd.TD3Group(learners), learners, [GH._ring(rows=batch_size + 3, capacity=batch_size + 8) for _ in range(K)]


def _untouched(learners, before):
    for t, b in zip(learners, before):
        assert t.last_path is None and all(torch.equal(v, b[k]) for k, v in t.critic.state_dict().items())


@pytest.mark.parametrize('B', [16, 129, 512])
def test_an_unknown_chunks_is_a_value_error(B, monkeypatch):
    from serl_amd import _capi
    group, learners, rings = _group(B)
    before = [copy.deepcopy(t.critic.state_dict()) for t in learners]
    monkeypatch.setattr(_capi, 'lib', lambda: pytest.fail('the library was reached'))
    for chunks in ('diagonal', None, 'Serial', 1):
        with pytest.raises(ValueError, match='chunks'):
            group.train(rings, 3, iteration0=0, seed=[1, 2], chunks=chunks)
    _untouched(learners, before)


@pytest.mark.parametrize('dense', ['valu', 'mfma'])
@pytest.mark.parametrize('chunks', ['serial', 'parallel'])
@pytest.mark.parametrize('B', [129, 300, 512])
def test_a_large_batch_passes_the_argument_checks_and_ends_at_the_device(B, chunks, dense):
    """batch_size above 128 is no longer 'this shape': on CPU rings the call gets past every argument check and is refused for the device,
    naming the entry it would have launched, with no learner touched"""
    group, learners, rings = _group(B)
    before = [copy.deepcopy(t.critic.state_dict()) for t in learners]
    entry = 'serl_td3_train_group_wide' if chunks == 'parallel' else 'serl_td3_train_group_big'
    with pytest.raises(RuntimeError, match='%s runs on one CUDA device.*rings are on cpu.*no eager fall-back' % entry) as e:
        group.train(rings, [3, 0], iteration0=[0, 4], seed=9, dense=dense, chunks=chunks)
    assert 'does not run this shape' not in str(e.value)
    _untouched(learners, before)


def test_small_batches_name_their_entries_too():
    group, learners, rings = _group(16)
    with pytest.raises(RuntimeError, match='serl_td3_train_group runs on one CUDA device'):
        group.train(rings, 3, iteration0=0, seed=[1, 2])
    with pytest.raises(RuntimeError, match='serl_td3_train_group_wide runs on one CUDA device'):
        group.train(rings, 3, iteration0=0, seed=[1, 2], chunks='parallel')


@pytest.mark.parametrize('chunks', ['serial', 'parallel'])
@pytest.mark.parametrize('case', [c for c in GH.BAD_TRAIN if c[1] is not None and 'ring1' not in c[0]],
                         ids=lambda c: '-'.join('%s=%s' % kv for kv in c[0].items()).replace(' ', ''))
def test_the_existing_value_errors_still_come_first(case, chunks, monkeypatch):
    """every argument error of tests/test_td3_group_host.py at batch_size 129 with either `chunks`: the ValueError it was, before the
    device is looked at"""
    from serl_amd import _capi
    kw, msg = dict(case[0]), case[1]
    group, learners, _ = _group(129)
    before = [copy.deepcopy(t.critic.state_dict()) for t in learners]
    rings = [GH._ring(rows=140, capacity=150) for _ in range(kw.pop('replays', 2))]
    monkeypatch.setattr(_capi, 'lib', lambda: pytest.fail('the library was reached'))
    call = dict(n_updates=4, iteration0=0, seed=[1, 2], chunks=chunks)
    call.update(kw)
    n_updates = call.pop('n_updates')
    with pytest.raises(ValueError, match=msg):
        group.train(rings, n_updates, **call)
    _untouched(learners, before)


def test_a_ring_below_one_large_minibatch_is_a_value_error():
    group, learners, rings = _group(129)
    rings[1] = GH._ring(rows=128, capacity=150)
    for chunks in ('serial', 'parallel'):
        with pytest.raises(ValueError, match='learner 1: 128 rows in the ring, minibatches of 129'):
            group.train(rings, 3, iteration0=0, seed=[1, 2], chunks=chunks)
    with pytest.raises(ValueError, match='chunks'):          # ... and an unknown `chunks` comes before it
        group.train(rings, 3, iteration0=0, seed=[1, 2], chunks='diagonal')

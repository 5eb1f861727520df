"""K policy-driven env steps in one launch (serl_venv_rollout, CitationVecEnv.rollout) without a GPU: the exports, the layout of
serl_venv_rollout_desc against its ctypes mirror and the header, the ABI that must not have moved, the argument checks of the C entry
that fail before the context is read, and the argument checks of CitationVecEnv.rollout that need no device."""
import ctypes, os, re
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()                    # raises when a ctypes mirror differs from the library's layout self-checks


def test_rollout_layout_equals_the_ctypes_mirror():
    from serl_amd import _capi
    L = _lib()
    for f in ('serl_venv_rollout', 'serl_venv_rollout_layout'):
        assert f in _capi.EXPORTS and hasattr(L, f)
    D = _capi.VenvRolloutDesc
    want = _capi.expected_venv_rollout_layout()
    assert want == [ctypes.sizeof(D)] + [getattr(D, f).offset for f, _ in D._fields_]
    assert L.serl_venv_rollout_layout(None, 0) == len(want) == 25
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_venv_rollout_layout(got, len(want)) == len(want)
    assert list(got) == want
    short = (ctypes.c_int32 * 3)(-1, -1, -1)           # a short buffer is filled as far as it goes
    assert L.serl_venv_rollout_layout(short, 2) == len(want) and list(short) == want[:2] + [-1]


def test_header_members_equal_the_mirror():
    from serl_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    body = re.search(r'typedef struct serl_venv_rollout_desc \{(.*?)\} serl_venv_rollout_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[;,]', body)
    assert names == [f for f, _ in _capi.VenvRolloutDesc._fields_], names


def test_the_abi_has_not_moved():
    from serl_amd import _capi
    L = _lib()
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    want = _capi.expected_venv_auto_layout()
    assert L.serl_venv_auto_layout(None, 0) == len(want) == 10
    got = (ctypes.c_int32 * 10)()
    L.serl_venv_auto_layout(got, 10)
    assert list(got) == want == [64, 0, 8, 16, 24, 32, 40, 48, 56, 60]
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert int(re.search(r'#define SERL_ABI_VERSION (\d+)', hdr).group(1)) == 9


def test_rollout_refuses_bad_descriptors_before_reading_the_context():
    """serl_venv_rollout checks its three descriptors before serl_venv_check reads the context, and this test relies on that order: the
    context here is a pointer that is never dereferenced.  What lies behind serl_venv_check needs a real context (GPU suite)."""
    from serl_amd import _capi
    L = _lib()
    E = _capi.E_INVALID
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p -= p % 16                                        # (never read: only its alignment is looked at)
    ctx = ctypes.c_void_p(8)

    def desc(**kw):
        d = dict(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1)
        d.update(kw)
        return _capi.VenvDesc(**d)

    def ro(**kw):
        d = dict(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation=0, n_members=1, weights=p, weight_stride=3716,
                 n_steps=5, obs=p)
        d.update(kw)
        return _capi.VenvRolloutDesc(**d)

    def call(c, d, au, r):
        ref = lambda s: None if s is None else ctypes.byref(s)
        return L.serl_venv_rollout(c, ref(d), ref(au), ref(r), None)
    au = _capi.VenvAutoDesc(run_return=p, run_length=p, cursor=p)
    assert call(None, desc(), au, ro()) == E and b'NULL' in L.serl_last_error()
    assert call(ctx, None, au, ro()) == E
    assert call(ctx, desc(), None, ro()) == E and b'NULL' in L.serl_last_error()
    assert call(ctx, desc(), au, None) == E
    for kw, word in ((dict(obs=None), b'obs'), (dict(weights=None), b'weights'), (dict(n_steps=0), b'n_steps'), (dict(n_steps=-3), b'n_steps'),
                     (dict(n_members=0), b'n_members'), (dict(hidden=72), b'hidden 32'), (dict(hidden=64), b'hidden 32'),
                     (dict(state_dim=13), b'hidden 32'), (dict(action_dim=1), b'hidden 32'), (dict(num_layers=-1), b'num_layers'),
                     (dict(activation=3), b'activation'), (dict(weight_stride=3715), b'weight_stride'), (dict(weight_stride=100), b'weight_stride'),
                     (dict(weights=p + 4), b'aligned')):
        assert call(ctx, desc(), au, ro(**kw)) == E, kw
        assert word in L.serl_last_error(), (kw, L.serl_last_error())
    for kw in (dict(env_config=1, state_dim=2, action_dim=1), dict(env_config=2, state_dim=13), dict(incremental=1, state_dim=10)):
        assert call(ctx, desc(**kw), au, ro()) == E, kw
        assert b'attitude' in L.serl_last_error()
    for field in ('run_return', 'run_length', 'cursor'):
        a2 = _capi.VenvAutoDesc(run_return=p, run_length=p, cursor=p)
        setattr(a2, field, None)
        assert call(ctx, desc(), a2, ro()) == E and b'cursor' in L.serl_last_error()
    a2 = _capi.VenvAutoDesc(run_return=p, run_length=p, cursor=p, ref_pool=p, pool_rows=0)
    assert call(ctx, desc(), a2, ro()) == E and b'pool_rows' in L.serl_last_error()
    a2.pool_rows = 2
    assert call(ctx, desc(ref=p), a2, ro()) == E and b'desc->ref' in L.serl_last_error()
    assert L.serl_param_count(7, 32, 3, 3) == 3715


class _Args:
    state_dim, action_dim, hidden_size, num_layers, activation_actor = 7, 3, 32, 2, 'tanh'


def _bare_env(**kw):
    """A CitationVecEnv that never touched a device: only what rollout()'s argument checks read."""
    import serl_amd
    env = object.__new__(serl_amd.CitationVecEnv)
    env.n_envs, env.state_dim, env.action_dim, env.auto_reset, env.device = 6, 7, 3, True, torch.device('cuda', 0)
    env.env_config, env.incremental = 0, False
    for k, v in kw.items():
        setattr(env, k, v)
    return env


def test_rollout_validates_its_arguments_before_any_device_work():
    import serl_amd
    assert callable(serl_amd.CitationVecEnv.rollout) and serl_amd.CitationVecEnv.last_rollout_path is None
    actor = serl_amd.Actor(_Args())
    with pytest.raises(ValueError, match='auto_reset'):
        _bare_env(auto_reset=False).rollout(actor, 5)
    env = _bare_env()
    for n in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='n_steps'):
            env.rollout(actor, n)
    with pytest.raises(ValueError, match='spec'):
        env.rollout(torch.zeros(1, 3716), 5)                                   # packed weights without a NetSpec
    with pytest.raises(ValueError, match='packed weights on cpu'):
        env.rollout(torch.zeros(1, 3716), 5, spec=actor.spec)                   # ... on the wrong device
    with pytest.raises(ValueError, match='empty'):
        env.rollout([], 5)
    with pytest.raises(ValueError, match='member_of_env'):
        env.rollout(actor, 5, member_of_env=np.zeros(5, np.int32))
    with pytest.raises(ValueError, match='action_noise'):
        env.rollout(actor, 5, action_noise=np.zeros((4, 6, 3)))
    with pytest.raises(ValueError, match='does not fit the env'):
        _bare_env(state_dim=13).rollout(actor, 5)
    # the shapes the kernel takes
    NetSpec = serl_amd.NetSpec
    assert env.fused_rollout_ok(NetSpec(7, 3, 32, 0, 'relu')) and env.fused_rollout_ok(NetSpec(7, 3, 32, 3, 'tanh'))
    assert not env.fused_rollout_ok(NetSpec(7, 3, 72, 3, 'tanh')) and not _bare_env(incremental=True).fused_rollout_ok(NetSpec(7, 3, 32, 3, 'tanh'))
    assert not _bare_env(env_config=2).fused_rollout_ok(NetSpec(7, 3, 32, 3, 'tanh'))

"""serl_venv_rollout_general / CitationVecEnv.rollout(path=...) without a GPU: the export and its ctypes signature, the ABI and the
three descriptor layouts that must not have moved, the descriptor checks of the C entry that fail before the context is read, which
shapes `fused_general_ok` takes, and the validation of `path` before any device work."""
import ctypes, os, re
import pytest
import torch

from actor_shapes import _shape, spec_of, ATTITUDE, SYMMETRIC, FULL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()


def test_the_symbol_and_its_signature():
    from serl_amd import _capi
    L = _lib()
    assert 'serl_venv_rollout_general' in _capi.EXPORTS and hasattr(L, 'serl_venv_rollout_general')
    f = L.serl_venv_rollout_general
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.POINTER(_capi.VenvDesc), ctypes.POINTER(_capi.VenvAutoDesc),
                                ctypes.POINTER(_capi.VenvRolloutDesc), ctypes.c_void_p]
    assert list(f.argtypes) == list(L.serl_venv_rollout.argtypes)
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert re.search(r'int serl_venv_rollout_general\(serl_ctx \*ctx, const serl_venv_desc \*desc, const serl_venv_auto_desc \*au, '
                     r'const serl_venv_rollout_desc \*ro,\s+void \*stream\);', hdr)


def test_the_abi_and_the_layouts_have_not_moved():
    """the values the parent commit returns, written out"""
    from serl_amd import _capi
    L = _lib()
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    got = (ctypes.c_int32 * 10)()
    assert L.serl_venv_auto_layout(got, 10) == 10
    assert list(got) == [64, 0, 8, 16, 24, 32, 40, 48, 56, 60]
    got = (ctypes.c_int32 * 25)()
    assert L.serl_venv_rollout_layout(got, 25) == 25
    assert list(got) == [160, 0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 52, 56, 64, 72, 80, 88, 96, 104, 112, 120, 128, 136, 144, 152]
    assert list(got) == _capi.expected_venv_rollout_layout()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert int(re.search(r'#define SERL_ABI_VERSION (\d+)', hdr).group(1)) == 9


def test_general_entry_refuses_bad_descriptors_before_reading_the_context():
    """as tests/test_venv_rollout_host.py: the context is a pointer that is never dereferenced"""
    from serl_amd import _capi
    L = _lib()
    EI, EU = _capi.E_INVALID, _capi.E_UNSUPPORTED
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p -= p % 16
    ctx = ctypes.c_void_p(8)
    P = L.serl_param_count(7, 72, 3, 3)
    assert P == 16995

    def desc(**kw):
        d = dict(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1)
        d.update(kw)
        return _capi.VenvDesc(**d)

    def ro(**kw):
        d = dict(state_dim=7, action_dim=3, hidden=72, num_layers=3, activation=0, n_members=1, weights=p, weight_stride=P + 1, n_steps=5, obs=p)
        d.update(kw)
        return _capi.VenvRolloutDesc(**d)

    def call(c, d, au, r):
        ref = lambda s: None if s is None else ctypes.byref(s)
        return L.serl_venv_rollout_general(c, ref(d), ref(au), ref(r), None)
    au = _capi.VenvAutoDesc(run_return=p, run_length=p, cursor=p)
    assert call(None, desc(), au, ro()) == EI and b'NULL' in L.serl_last_error()
    assert call(ctx, None, au, ro()) == EI and call(ctx, desc(), None, ro()) == EI and call(ctx, desc(), au, None) == EI
    for kw, rc, word in ((dict(obs=None), EI, b'obs'), (dict(weights=None), EI, b'weights'), (dict(n_steps=0), EI, b'n_steps'),
                         (dict(n_members=0), EI, b'n_members'), (dict(hidden=30), EU, b'hidden'), (dict(hidden=132), EU, b'hidden'),
                         (dict(hidden=0), EU, b'hidden'), (dict(hidden=2), EU, b'hidden'), (dict(num_layers=17), EU, b'num_layers'),
                         (dict(num_layers=-1), EU, b'num_layers'), (dict(activation=3), EI, b'activation'), (dict(activation=-1), EI, b'activation'),
                         (dict(state_dim=13), EI, b'env configuration'), (dict(action_dim=1), EI, b'env configuration'),
                         (dict(weight_stride=P - 3), EI, b'weight_stride'), (dict(weight_stride=P + 3), EI, b'weight_stride'),
                         (dict(weights=p + 4), EI, b'aligned')):
        assert call(ctx, desc(), au, ro(**kw)) == rc, kw
        assert word in L.serl_last_error() and b'serl_venv_rollout_general' in L.serl_last_error(), (kw, L.serl_last_error())
    assert call(ctx, desc(env_config=3), au, ro()) == EI and b'env_config' in L.serl_last_error()
    # the actor must fit the env configuration of the ENV descriptor
    assert call(ctx, desc(env_config=1, state_dim=2, action_dim=1), au, ro()) == EI and b'env configuration' in L.serl_last_error()
    assert call(ctx, desc(incremental=1, state_dim=10), au, ro()) == EI and b'env configuration' in L.serl_last_error()
    for field in ('run_return', 'run_length', 'cursor'):
        a2 = _capi.VenvAutoDesc(run_return=p, run_length=p, cursor=p)
        setattr(a2, field, None)
        assert call(ctx, desc(), a2, ro()) == EI and b'cursor' in L.serl_last_error()
    a2 = _capi.VenvAutoDesc(run_return=p, run_length=p, cursor=p, ref_pool=p, pool_rows=0)
    assert call(ctx, desc(), a2, ro()) == EI and b'pool_rows' in L.serl_last_error()
    # serl_venv_rollout keeps refusing what it refused
    assert L.serl_venv_rollout(ctx, ctypes.byref(desc()), ctypes.byref(au), ctypes.byref(ro()), None) == EI and b'hidden 32' in L.serl_last_error()


def _bare_env(cfg=ATTITUDE, incr=False):
    """A CitationVecEnv that never touched a device: only what rollout()'s argument checks read (tests/test_venv_rollout_host.py)."""
    import serl_amd
    from serl_amd import builds
    env = object.__new__(serl_amd.CitationVecEnv)
    env.n_envs, env.auto_reset, env.device = 6, True, torch.device('cuda', 0)
    env.env_config, env.incremental = cfg, bool(incr)
    env.state_dim, env.action_dim = builds.env_dims(cfg, incr)
    return env


SUBSET = ([_shape(H, 3) for H in (4, 20, 72, 96, 128)] + [_shape(12, 0), _shape(128, 0), _shape(8, 16), _shape(100, 3)]
          + [_shape(72, 3, 'elu'), _shape(72, 3, 'relu')]
          + [_shape(32, 2, 'elu', ATTITUDE, True), _shape(12, 2, 'tanh', SYMMETRIC), _shape(8, 1, 'tanh', SYMMETRIC, True),
             _shape(72, 3, 'relu', FULL), _shape(48, 3, 'tanh', FULL, True)])


def test_fused_general_ok():
    import serl_amd
    NetSpec = serl_amd.NetSpec
    for s in SUBSET:
        env = _bare_env(s['env_config'], s['incremental'])
        assert env.fused_general_ok(spec_of(s)), s
        assert not env.fused_rollout_ok(spec_of(s)), s                    # none of them is the lane-32 kernel's
    env = _bare_env()
    assert env.fused_general_ok(NetSpec(7, 3, 32, 3, 'tanh')) and env.fused_rollout_ok(NetSpec(7, 3, 32, 3, 'tanh'))
    for H, L in ((30, 1), (132, 1), (2, 1), (0, 1), (6, 3), (72, 17), (72, -1)):
        assert not env.fused_general_ok(NetSpec(7, 3, H, L, 'tanh')), (H, L)
    assert not env.fused_general_ok(NetSpec(13, 3, 72, 3, 'tanh')) and not env.fused_general_ok(NetSpec(2, 1, 72, 3, 'tanh'))
    assert _bare_env(FULL).fused_general_ok(NetSpec(13, 3, 72, 3, 'tanh')) and not _bare_env(FULL, True).fused_general_ok(NetSpec(13, 3, 72, 3, 'tanh'))
    assert _bare_env(SYMMETRIC, True).fused_general_ok(NetSpec(3, 1, 72, 3, 'tanh'))


class _Args:
    state_dim, action_dim, hidden_size, num_layers, activation_actor = 7, 3, 30, 1, 'tanh'


def test_path_is_validated_before_any_device_work():
    import serl_amd
    env = _bare_env()                                                     # (any device work would fail: the env has no buffers)
    actor = serl_amd.Actor(_Args())
    assert serl_amd.CitationVecEnv.ROLLOUT_PATHS == ('auto', 'fused', 'loop')
    for bad in ('bogus', '', None, 'FUSED', 'fused-general'):
        with pytest.raises(ValueError, match='path'):
            env.rollout(actor, 5, path=bad)
    with pytest.raises(ValueError, match="path='fused'"):
        env.rollout(actor, 5, path='fused')                               # hidden 30: no kernel takes it
    # the other argument checks still come first-hand with a path given
    with pytest.raises(ValueError, match='n_steps'):
        env.rollout(actor, 0, path='fused')
    with pytest.raises(ValueError, match='auto_reset'):
        e2 = _bare_env(); e2.auto_reset = False
        e2.rollout(actor, 5, path='loop')

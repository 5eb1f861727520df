"""The wave rollout entries (serl_venv_rollout_wave / _wave_noise, CitationVecEnv.rollout(path='fused') on a wave env) without a GPU: the exports and
their signatures, the refusals that come before any device work, and the ABI and the Python surface that must not have moved."""
import ctypes, os, re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [('serl_venv_rollout_wave', 'serl_venv_rollout_general'), ('serl_venv_rollout_wave_noise', 'serl_venv_rollout_general_noise')]


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()


def test_exports_and_header():
    from serl_amd import _capi
    L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    args = lambda name: re.sub(r'\s+', ' ', re.search(r'^int %s\((.*?)\);' % name, hdr, re.M | re.S).group(1))
    for wave, general in PAIRS:
        assert wave in _capi.EXPORTS and hasattr(L, wave)
        assert re.search(r'^int %s\(' % wave, hdr, re.M), wave
        assert args(wave) == args(general), wave
        assert getattr(L, wave).argtypes == getattr(L, general).argtypes and getattr(L, wave).argtypes is not None


def test_the_build_has_a_unit_of_its_own_per_code_variant():
    from serl_amd import build
    assert 'venvwr' in build.FAMILIES and 'venvw' in build.FAMILIES
    for code, v in enumerate(build.VARIANTS):
        assert build.UNITS['rollout_venvwr_' + v] == ('family_venvwr.hip', ['-DSERL_DYN=%d' % code])
        assert build.UNITS['rollout_venvw_' + v] == ('family_venvw.hip', ['-DSERL_DYN=%d' % code])
    assert os.path.exists(os.path.join(build.CSRC, 'family_venvwr.hip'))


def test_the_abi_has_not_moved():
    from serl_amd import _capi
    L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert int(re.search(r'#define SERL_ABI_VERSION (\d+)', hdr).group(1)) == 9
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    for name, want in (('serl_venv_auto_layout', _capi.expected_venv_auto_layout()), ('serl_venv_rollout_layout', _capi.expected_venv_rollout_layout()),
                       ('serl_venv_noise_layout', _capi.expected_venv_noise_layout())):
        got = (ctypes.c_int32 * len(want))()
        assert getattr(L, name)(got, len(want)) == len(want) and list(got) == want, name
    assert _capi.FAMILIES[10] == 'wave' and len(_capi.FAMILIES) == 14      # no family added: the launch is recorded as SERL_FAMILY_WAVE


def test_refusals_before_any_launch():
    """the descriptor checks of serl_venv_rollout_general[_noise], in its order, none of which reads the context"""
    from serl_amd import _capi
    L = _lib()
    ctx = ctypes.c_void_p(8)      # never dereferenced by these checks
    buf = (ctypes.c_float * 32768)()
    base = ctypes.addressof(buf)
    wts = base + (-base) % 16
    d = _capi.VenvDesc(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1)
    run = ctypes.cast((ctypes.c_double * 8)(), ctypes.c_void_p)
    au = _capi.VenvAutoDesc(run_return=run, run_length=run, cursor=run)

    def rdesc(**over):
        kw = dict(state_dim=7, action_dim=3, hidden=72, num_layers=3, activation=0, n_members=1, weights=wts, weight_stride=24000, n_steps=3, obs=run)
        kw.update(over)
        return _capi.VenvRolloutDesc(**kw)

    def call(rd, dd=d, aa=au, c=ctx):
        return L.serl_venv_rollout_wave(c, None if dd is None else ctypes.byref(dd), None if aa is None else ctypes.byref(aa),
                                        None if rd is None else ctypes.byref(rd), None)
    assert call(rdesc(), c=None) == _capi.E_INVALID and b'serl_venv_rollout_wave' in L.serl_last_error()
    assert call(rdesc(), dd=None) == _capi.E_INVALID and call(rdesc(), aa=None) == _capi.E_INVALID and call(None) == _capi.E_INVALID
    P = L.serl_param_count(7, 72, 3, 3)
    cases = [(dict(obs=None), _capi.E_INVALID, b'obs'), (dict(weights=None), _capi.E_INVALID, b'weights'), (dict(n_steps=0), _capi.E_INVALID, b'n_steps'),
             (dict(n_members=0), _capi.E_INVALID, b'n_members'), (dict(state_dim=13), _capi.E_INVALID, b'state_dim'),
             (dict(action_dim=1), _capi.E_INVALID, b'action_dim'), (dict(hidden=132), _capi.E_UNSUPPORTED, b'hidden'),
             (dict(hidden=30), _capi.E_UNSUPPORTED, b'hidden'), (dict(hidden=0), _capi.E_UNSUPPORTED, b'hidden'),
             (dict(num_layers=17), _capi.E_UNSUPPORTED, b'num_layers'), (dict(num_layers=-1), _capi.E_UNSUPPORTED, b'num_layers'),
             (dict(activation=3), _capi.E_INVALID, b'activation'), (dict(weight_stride=P - 3), _capi.E_INVALID, b'weight_stride'),
             (dict(weight_stride=P + 3), _capi.E_INVALID, b'weight_stride'), (dict(weights=wts + 4), _capi.E_INVALID, b'16-byte')]
    for over, code, word in cases:
        for name in ('serl_venv_rollout_wave', 'serl_venv_rollout_general'):      # the same refusal, the same code, from either entry
            rd = rdesc(**over)
            assert getattr(L, name)(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), None) == code, (name, over)
            err = L.serl_last_error()
            assert name.encode() + b':' in err and word in err, (name, over, err)
    for field in ('run_return', 'run_length', 'cursor'):
        a2 = _capi.VenvAutoDesc.from_buffer_copy(au)
        setattr(a2, field, None)
        assert call(rdesc(), aa=a2) == _capi.E_INVALID and b'run_return' in L.serl_last_error(), field
    a2 = _capi.VenvAutoDesc.from_buffer_copy(au)
    a2.ref_pool, a2.pool_rows = run, 0
    assert call(rdesc(), aa=a2) == _capi.E_INVALID and b'pool_rows' in L.serl_last_error()
    d2 = _capi.VenvDesc.from_buffer_copy(d)
    d2.ref, a2.pool_rows = run, 2
    assert call(rdesc(), dd=d2, aa=a2) == _capi.E_INVALID and b'desc->ref' in L.serl_last_error()
    # the noise entry: what serl_venv_rollout_general_noise refuses in `nz`, before anything else
    nz = _capi.VenvNoiseDesc()
    rd = rdesc()
    f = L.serl_venv_rollout_wave_noise
    assert f(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), None, None) == _capi.E_INVALID and b'nz is NULL' in L.serl_last_error()
    assert f(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), ctypes.byref(nz), None) == _capi.E_INVALID
    assert b'serl_venv_rollout_wave_noise' in L.serl_last_error() and b'episode_count' in L.serl_last_error()
    nz = _capi.VenvNoiseDesc(episode_count=run, action=1, action_sd=0.1, action_clip=0.2)
    rd = rdesc(action_noise=run)
    assert f(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), ctypes.byref(nz), None) == _capi.E_INVALID and b'action_noise' in L.serl_last_error()
    nz = _capi.VenvNoiseDesc(episode_count=run, action=1, action_sd=-1.0, action_clip=0.2)
    rd = rdesc()
    assert f(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), ctypes.byref(nz), None) == _capi.E_INVALID and b'action_sd' in L.serl_last_error()
    nz = _capi.VenvNoiseDesc(episode_count=run)
    rd = rdesc(hidden=132)
    assert f(ctx, ctypes.byref(d), ctypes.byref(au), ctypes.byref(rd), ctypes.byref(nz), None) == _capi.E_UNSUPPORTED


def _bare(cfg=0, incr=False, S=7, A=3, wave=True):
    from serl_amd import venv
    env = venv.CitationVecEnv.__new__(venv.CitationVecEnv)
    env.env_config, env.incremental, env.state_dim, env.action_dim = cfg, incr, S, A
    env.auto_reset, env.n_envs, env._wave, env.kernel = True, 4, wave, 'wave' if wave else 'lane'
    return env


def test_python_surface():
    import serl_amd
    from serl_amd import venv
    assert venv.CitationVecEnv.ROLLOUT_PATHS == ('auto', 'fused', 'loop')
    assert venv.CitationVecEnv.last_rollout_path is None
    att, sym, full_inc = _bare(), _bare(1, False, 2, 1), _bare(2, True, 16, 3)
    shapes = [(7, 3, 32, 3), (7, 3, 32, 0), (7, 3, 64, 1), (7, 3, 72, 3), (7, 3, 96, 2), (7, 3, 128, 1), (7, 3, 4, 0), (7, 3, 32, 16), (7, 3, 132, 1),
              (7, 3, 30, 1), (7, 3, 0, 1), (7, 3, 32, 17), (7, 3, 128, 16), (2, 1, 12, 2), (2, 1, 32, 3), (16, 3, 48, 3), (13, 3, 72, 3), (10, 3, 32, 2)]
    seen = set()
    for env in (att, sym, full_inc):
        for S, A, H, Lr in shapes:
            spec = serl_amd.NetSpec(S, A, H, Lr, 'tanh')
            assert env.fused_wave_ok(spec) == env.fused_general_ok(spec), (S, A, H, Lr)
            seen.add(env.fused_wave_ok(spec))
    assert seen == {True, False}
    assert att.fused_wave_ok(serl_amd.NetSpec(7, 3, 32, 3, 'tanh')) and att.fused_rollout_ok(serl_amd.NetSpec(7, 3, 32, 3, 'tanh'))      # the lane-32 shape is included


def test_arguments_are_checked_before_the_kernel_family_is_looked_at():
    """a bare env without `_wave` (tests build such envs with __new__): the path and the arguments are refused first"""
    import serl_amd
    import torch
    from serl_amd import venv
    env = venv.CitationVecEnv.__new__(venv.CitationVecEnv)
    env.env_config, env.incremental, env.state_dim, env.action_dim, env.auto_reset, env.n_envs = 0, False, 7, 3, True, 4
    env.device = torch.device('cpu')
    assert not hasattr(env, '_wave')
    w = torch.zeros(1, 4000)
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    with pytest.raises(ValueError, match='path'):
        env.rollout(w, 3, spec=spec, path='fused-wave')
    with pytest.raises(ValueError, match='n_steps'):
        env.rollout(w, 0, spec=spec, path='fused')
    with pytest.raises(ValueError, match="path='fused'"):
        env.rollout(torch.zeros(1, 4000), 3, spec=serl_amd.NetSpec(7, 3, 30, 1, 'tanh'), path='fused')
    with pytest.raises(ValueError, match='does not fit'):
        env.rollout(w, 3, spec=serl_amd.NetSpec(2, 1, 32, 3, 'tanh'), path='fused')
    with pytest.raises(ValueError, match='member_of_env'):
        env.rollout(w, 3, spec=spec, member_of_env=[0, 0], path='fused')

"""The wave path of the step-wise env (serl_venv_*_wave, CitationVecEnv(kernel=...)) without a GPU: the exports, the refusals that come before any
device work, and the ABI that must not have moved."""
import ctypes, os, re
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_ENTRIES = ['serl_venv_reset_wave', 'serl_venv_step_wave', 'serl_venv_step_auto_wave', 'serl_venv_reset_wave_noise',
                'serl_venv_step_auto_wave_noise']


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()


def test_exports_and_header():
    from serl_amd import _capi
    L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    for f in WAVE_ENTRIES + ['serl_venv_last_info']:
        assert f in _capi.EXPORTS and hasattr(L, f)
        assert re.search(r'^int %s\(' % f, hdr, re.M), f
    for f in WAVE_ENTRIES:      # the argument list of the namesake
        lane = f.replace('_wave', '')
        args = lambda name: re.sub(r'\s+', ' ', re.search(r'^int %s\((.*?)\);' % name, hdr, re.M | re.S).group(1))
        assert args(f) == args(lane), f
        assert getattr(L, f).argtypes == getattr(L, lane).argtypes


def test_bad_kernel_is_a_value_error_before_any_device_work():
    import serl_amd
    for bad in ('team', 'Wave', None, 1, ''):
        with pytest.raises(ValueError, match='kernel'):
            serl_amd.CitationVecEnv(4, kernel=bad)
    from serl_amd import venv
    assert venv.KERNELS == ('lane', 'wave', 'auto') and isinstance(venv.WAVE_MAX_ENVS, int) and venv.WAVE_MAX_ENVS >= 0


def test_wave_env_raises_without_a_gpu():
    import serl_amd
    if torch.cuda.is_available():
        pytest.skip('a GPU is present: tests/test_gpu_venv_wave.py constructs the env')
    with pytest.raises(RuntimeError, match='needs a ROCm GPU'):
        serl_amd.CitationVecEnv(4, kernel='wave')


def test_refusals_before_any_launch():
    """what needs no context: NULL descriptors, pool_rows, a pool together with desc->ref, a NULL nz -- in the namesakes' order, before serl_venv_check
    reads the context (tests/test_venv_auto_host.py relies on the same order); actions_f64 needs a context: tests/test_gpu_venv_wave.py"""
    from serl_amd import _capi
    L = _lib()
    d = _capi.VenvDesc(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1)
    au = _capi.VenvAutoDesc()
    nz = _capi.VenvNoiseDesc()
    nul = (None,) * 7
    ctx = ctypes.c_void_p(8)      # never dereferenced by these checks
    assert L.serl_venv_reset_wave(None, ctypes.byref(d), None, None, None) == _capi.E_INVALID
    assert L.serl_venv_reset_wave(ctx, None, None, None, None) == _capi.E_INVALID
    assert L.serl_venv_step_wave(None, ctypes.byref(d), None, 0, *nul, None) == _capi.E_INVALID
    assert L.serl_venv_step_wave(ctx, None, None, 0, *nul, None) == _capi.E_INVALID
    assert b'serl_venv_step_wave' in L.serl_last_error()
    assert L.serl_venv_step_auto_wave(None, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert L.serl_venv_step_auto_wave(ctx, None, None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert L.serl_venv_step_auto_wave(ctx, ctypes.byref(d), None, 0, *nul, None, None) == _capi.E_INVALID
    assert L.serl_venv_reset_wave_noise(ctx, ctypes.byref(d), None, None, None, None) == _capi.E_INVALID
    assert b'nz is NULL' in L.serl_last_error()
    assert L.serl_venv_reset_wave_noise(ctx, ctypes.byref(d), None, None, ctypes.byref(nz), None) == _capi.E_INVALID
    assert b'episode_count' in L.serl_last_error()
    assert L.serl_venv_step_auto_wave_noise(ctx, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None, None) == _capi.E_INVALID
    assert b'nz is NULL' in L.serl_last_error()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for pool_rows, word in ((0, b'pool_rows'), (2, b'desc->ref')):
        au = _capi.VenvAutoDesc(ref_pool=p, pool_rows=pool_rows)
        d.ref = p
        assert L.serl_venv_step_auto_wave(ctx, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
        if pool_rows:
            assert word in L.serl_last_error()
    d.ref = None
    au = _capi.VenvAutoDesc(ref_pool=p, pool_rows=0)
    assert L.serl_venv_step_auto_wave(ctx, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert b'pool_rows' in L.serl_last_error()
    assert L.serl_venv_last_info(None, None) == _capi.E_INVALID


def test_the_abi_has_not_moved():
    from serl_amd import _capi
    L = _lib()
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    for name, want in (('serl_venv_auto_layout', _capi.expected_venv_auto_layout()), ('serl_venv_rollout_layout', _capi.expected_venv_rollout_layout()),
                       ('serl_venv_noise_layout', _capi.expected_venv_noise_layout())):
        got = (ctypes.c_int32 * len(want))()
        assert getattr(L, name)(got, len(want)) == len(want) and list(got) == want, name
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    from serl_amd import venv
    import inspect
    assert inspect.signature(venv.CitationVecEnv.__init__).parameters['kernel'].default == 'lane'

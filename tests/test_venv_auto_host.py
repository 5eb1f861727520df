"""Auto-reset inside the step of the vector env (serl_venv_step_auto, CitationVecEnv(auto_reset=True)) without a GPU: the export, the
layout of serl_venv_auto_desc against its ctypes mirror and the header, the ABI that must not have moved, argument checks that fail
before any device work, and the refusal to run without a GPU."""
import ctypes, os, re
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()                    # raises when a ctypes mirror differs from the library's layout self-checks


def test_auto_layout_equals_the_ctypes_mirror():
    from serl_amd import _capi
    L = _lib()
    for f in ('serl_venv_step_auto', 'serl_venv_auto_layout'):
        assert f in _capi.EXPORTS and hasattr(L, f)
    want = _capi.expected_venv_auto_layout()
    assert want == [ctypes.sizeof(_capi.VenvAutoDesc)] + [getattr(_capi.VenvAutoDesc, f).offset for f, _ in _capi.VenvAutoDesc._fields_]
    assert L.serl_venv_auto_layout(None, 0) == len(want)
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_venv_auto_layout(got, len(want)) == len(want)
    assert list(got) == want
    short = (ctypes.c_int32 * 3)(-1, -1, -1)           # a short buffer is filled as far as it goes
    assert L.serl_venv_auto_layout(short, 2) == len(want) and list(short) == want[:2] + [-1]


def test_header_members_equal_the_mirror():
    from serl_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    body = re.search(r'typedef struct serl_venv_auto_desc \{(.*?)\} serl_venv_auto_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[;,]', body)
    assert names == [f for f, _ in _capi.VenvAutoDesc._fields_], names


def test_the_abi_has_not_moved():
    from serl_amd import _capi
    L = _lib()
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert int(re.search(r'#define SERL_ABI_VERSION (\d+)', hdr).group(1)) == 9


def test_step_auto_refuses_null_arguments_before_any_launch():
    from serl_amd import _capi
    L = _lib()
    d = _capi.VenvDesc(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1)
    au = _capi.VenvAutoDesc()
    nul = (None,) * 7
    assert L.serl_venv_step_auto(None, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert b'NULL' in L.serl_last_error()
    # A context that is never dereferenced: serl_venv_step_auto checks the two descriptors (NULL, pool_rows, pool with desc->ref)
    # before serl_venv_check reads the context, and this test relies on that order.  The cases behind serl_venv_check -- a NULL
    # output, actions_f64 -- need a real context and are covered on the GPU (tests/test_gpu_venv_auto.py::test_bad_arguments).
    ctx = ctypes.c_void_p(8)
    assert L.serl_venv_step_auto(ctx, None, None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert L.serl_venv_step_auto(ctx, ctypes.byref(d), None, 0, *nul, None, None) == _capi.E_INVALID
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    au = _capi.VenvAutoDesc(ref_pool=p, pool_rows=0)
    assert L.serl_venv_step_auto(ctx, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert b'pool_rows' in L.serl_last_error()
    au = _capi.VenvAutoDesc(ref_pool=p, pool_rows=2)
    d.ref = p
    assert L.serl_venv_step_auto(ctx, ctypes.byref(d), None, 0, *nul, ctypes.byref(au), None) == _capi.E_INVALID
    assert b'desc->ref' in L.serl_last_error()


def test_auto_reset_raises_without_a_gpu():
    import serl_amd
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            serl_amd.CitationVecEnv(8, auto_reset=True, ref_pool=0)
        return
    with pytest.raises(RuntimeError, match='needs a ROCm GPU'):
        serl_amd.CitationVecEnv(8, auto_reset=True)
    with pytest.raises(RuntimeError, match='needs a ROCm GPU'):
        serl_amd.CitationVecEnv(8, mode='PHlab_symmetric_incremental', auto_reset=True, ref_pool=2)

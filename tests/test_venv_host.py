"""The step-wise vector env (C ABI v9 serl_venv_*, serl_amd.CitationVecEnv) without a GPU: exports, struct layout, argument checks
that fail before any device work, the refusal to run without a GPU, and the (S, A) of the env configurations."""
import ctypes, os, re
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_venv_symbols_are_exported_and_the_layout_matches():
    from serl_amd import build, _capi
    build.build()
    L = _capi.lib()                       # raises when the ctypes mirror differs from serl_abi_layout
    for f in ('serl_venv_state_bytes', 'serl_venv_reset', 'serl_venv_step'):
        assert f in _capi.EXPORTS and hasattr(L, f)
    want = _capi.expected_layout()
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_abi_layout(got, len(want)) == len(want)
    n = len(_capi.VenvDesc._fields_)
    assert list(got)[-(n + 1):] == [ctypes.sizeof(_capi.VenvDesc)] + [getattr(_capi.VenvDesc, f).offset for f, _ in _capi.VenvDesc._fields_]
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert int(re.search(r'#define SERL_ABI_VERSION (\d+)', hdr).group(1)) == 9 == _capi.ABI_VERSION
    body = re.search(r'typedef struct serl_venv_desc \{(.*?)\} serl_venv_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)\s*[;,]', body)
    assert names == [f for f, _ in _capi.VenvDesc._fields_], names


def test_venv_state_bytes():
    from serl_amd import _capi
    L = _capi.lib()
    per_env = L.serl_venv_state_bytes(64) // 64
    assert per_env > 0 and per_env % 4 == 0
    assert L.serl_venv_state_bytes(0) == 0 and L.serl_venv_state_bytes(-3) == 0
    assert L.serl_venv_state_bytes(1) == L.serl_venv_state_bytes(64) == 64 * per_env     # SoA lines padded to 64 envs
    assert L.serl_venv_state_bytes(65) == 128 * per_env
    assert L.serl_venv_state_bytes(65536) == 65536 * per_env


def test_venv_entry_points_refuse_null_arguments():
    from serl_amd import _capi
    L = _capi.lib()
    d = _capi.VenvDesc(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1)
    assert L.serl_venv_reset(None, ctypes.byref(d), None, None, None) == -1
    assert b'NULL' in L.serl_last_error()
    assert L.serl_venv_step(None, ctypes.byref(d), None, 0, None, None, None, None, None, None, None, None) == -1
    assert L.serl_venv_reset(None, None, None, None, None) == -1


def test_citation_vec_env_raises_without_a_gpu():
    import serl_amd
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError):
        serl_amd.CitationVecEnv(8)
    with pytest.raises(RuntimeError):
        serl_amd.CitationVecEnv(8, mode='PHlab_symmetric_incremental')


@pytest.mark.parametrize('name,cfg,incr,S,A', [
    ('PHlab_attitude_nominal', 0, False, 7, 3), ('nominal', 0, False, 7, 3), ('be', 0, False, 7, 3),
    ('PHlab_symmetric_nominal', 1, False, 2, 1), ('PHlab_full_nominal', 2, False, 13, 3),
    ('PHlab_attitude_incremental', 0, True, 10, 3), ('PHlab_symmetric_incremental', 1, True, 3, 1),
    ('PHlab_full_incremental', 2, True, 16, 3)])
def test_mode_parsing_gives_the_env_widths(name, cfg, incr, S, A):
    from serl_amd import builds, _capi
    assert builds.env_config(name) == (cfg, incr)
    assert builds.env_dims(cfg, incr) == (S, A)
    L = _capi.lib()
    assert (L.serl_env_state_dim(cfg, int(incr)), L.serl_env_action_dim(cfg)) == (S, A)

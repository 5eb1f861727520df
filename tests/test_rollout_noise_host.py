"""serl_rollout_noise and the device-noise arguments of RolloutEngine.rollout / evaluate_pop / evaluate_generation without a GPU: the export, the
descriptor's layout against its ctypes mirror and against the header's text, the argument errors that come before any device work, the build's
units, and the ABI that must not have moved."""
import ctypes, os, re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {'uint64_t': ctypes.c_uint64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double}


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()


def _header():
    return open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()


def test_layout_against_the_mirror_and_the_header():
    from serl_amd import _capi
    L = _lib()
    want = _capi.expected_rollout_noise_layout()
    assert L.serl_rollout_noise_layout(None, 0) == len(want) == 12
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_rollout_noise_layout(got, len(want)) == len(want) and list(got) == want
    body = re.search(r'typedef struct serl_rollout_noise_desc \{(.*?)\} serl_rollout_noise_desc;', _header(), re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = []
    for decl in [x.strip() for x in body.split(';') if x.strip()]:
        m = re.match(r'(const\s+)?(\w+)\s*(\*?)\s*(\w+)(\[(\d+)\])?$', decl)
        assert m, decl
        t = ctypes.c_void_p if m.group(3) else CTYPE[m.group(2)]
        fields.append((m.group(4), t * int(m.group(6)) if m.group(6) else t))
    assert [(n, ctypes.sizeof(t)) for n, t in fields] == [(n, ctypes.sizeof(t)) for n, t in _capi.RolloutNoiseDesc._fields_]
    text = type('FromHeader', (ctypes.Structure,), {'_fields_': fields})
    assert [ctypes.sizeof(text)] + [getattr(text, n).offset for n, _ in fields] == want
    # the generator's parameters sit as in serl_venv_noise_desc: one Python helper fills both
    for n in ('seed', 'sensor', 'sensor_bias', 'sensor_scale', 'action', 'action_sd', 'action_clip'):
        assert dict(_capi.RolloutNoiseDesc._fields_)[n] is dict(_capi.VenvNoiseDesc._fields_)[n] or \
            ctypes.sizeof(dict(_capi.RolloutNoiseDesc._fields_)[n]) == ctypes.sizeof(dict(_capi.VenvNoiseDesc._fields_)[n])


def test_export_and_signature():
    from serl_amd import _capi
    L = _lib()
    hdr = _header()
    for name in ('serl_rollout_noise', 'serl_rollout_noise_layout'):
        assert name in _capi.EXPORTS and hasattr(L, name) and re.search(r'^int %s\(' % name, hdr, re.M), name
    assert L.serl_rollout_noise.argtypes == [ctypes.c_void_p, ctypes.POINTER(_capi.RolloutDesc), ctypes.POINTER(_capi.RolloutNoiseDesc), ctypes.c_void_p]
    sig = re.sub(r'\s+', ' ', re.search(r'^int serl_rollout_noise\((.*?)\);', hdr, re.M | re.S).group(1))
    assert sig == 'serl_ctx *ctx, const serl_rollout_desc *desc, const serl_rollout_noise_desc *nz, void *stream'
    # a NULL context or descriptor is refused before anything is read
    assert L.serl_rollout_noise(None, None, None, None) == _capi.E_INVALID


def test_the_build_has_units_of_their_own_per_code_variant():
    from serl_amd import build
    for fam in ('lanern', 'wavern'):
        assert fam in build.FAMILIES
        for code, v in enumerate(build.VARIANTS):
            assert build.UNITS['rollout_%s_%s' % (fam, v)] == ('family_%s.hip' % fam, ['-DSERL_DYN=%d' % code])
        assert os.path.exists(os.path.join(build.CSRC, 'family_%s.hip' % fam))
    for v in build.VARIANTS:      # the existing units are what they were
        assert build.UNITS['rollout_' + v][0] == 'family_lane.hip' and build.UNITS['rollout_wave_' + v][0] == 'family_wave.hip'


def test_the_abi_has_not_moved():
    from serl_amd import _capi
    L = _lib()
    assert int(re.search(r'#define SERL_ABI_VERSION (\d+)', _header()).group(1)) == 9
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    for name, want in (('serl_venv_auto_layout', _capi.expected_venv_auto_layout()), ('serl_venv_rollout_layout', _capi.expected_venv_rollout_layout()),
                       ('serl_venv_noise_layout', _capi.expected_venv_noise_layout())):
        got = (ctypes.c_int32 * len(want))()
        assert getattr(L, name)(got, len(want)) == len(want) and list(got) == want, name
    assert len(_capi.FAMILIES) == 14 and len(_capi.KERNEL_HINTS) == 8      # no family, no hint added


def _bare_engine():
    """an engine no device stands behind: every call below must raise before it reads one"""
    from serl_amd.evaluator import RolloutEngine
    return RolloutEngine.__new__(RolloutEngine)


ROLLOUT_ERRORS = [
    (dict(sensor_noise='host'), 'sensor_noise'), (dict(action_noise='tables'), 'action_noise'),
    (dict(sensor_noise='device'), 'noise_seed'), (dict(sensor_noise='device', noise_seed=True), 'noise_seed'),
    (dict(sensor_noise='device', noise_seed=2**64), 'noise_seed'), (dict(sensor_noise='device', noise_seed=1.5), 'noise_seed'),
    (dict(action_noise='device', noise_seed=1), 'noise_sd'), (dict(action_noise='device', noise_seed=1, noise_sd=0.1), 'noise_sd'),
    (dict(action_noise='device', noise_seed=1, noise_sd=-0.1, noise_clip=0.5), 'noise_sd'),
    (dict(action_noise='device', noise_seed=1, noise_sd=0.1, noise_clip=float('nan')), 'noise_clip'),
    (dict(noise_sd=0.1, noise_clip=0.5), 'belong'), (dict(sensor_noise='device', noise_seed=1, noise_sd=0.1, noise_clip=0.5), 'belong'),
    (dict(noise_seed=1), 'belong'), (dict(noise_env=[0, 1, 2]), 'belong'), (dict(noise_episode=[0, 0, 0]), 'belong'),
    (dict(sensor_noise='device', noise_seed=1, noise_env=[0, 1]), 'noise_env'),
    (dict(sensor_noise='device', noise_seed=1, noise_env=[0.0, 1.0, 2.0]), 'noise_env'),
    (dict(sensor_noise='device', noise_seed=1, noise_episode=[0, 1, 2**31]), 'noise_episode'),
    (dict(sensor_noise='device', noise_seed=1, sensor_row=[0, -1]), 'sensor_row'),
    (dict(action_noise='device', noise_seed=1, noise_sd=0.1, noise_clip=0.5, noise_row=[0]), 'noise_row'),
    (dict(sensor_noise='device', noise_seed=1, launch=False), 'launch'),
] + [(dict(sensor_noise='device', noise_seed=1, kernel=k), 'kernel') for k in ('team', 'team2', 'team4', 'half', 'laneq')]


@pytest.mark.parametrize('kw,word', ROLLOUT_ERRORS, ids=[str(i) for i in range(len(ROLLOUT_ERRORS))])
def test_rollout_argument_errors_before_any_device_work(kw, word):
    with pytest.raises(ValueError, match=word):
        _bare_engine().rollout(None, None, [0, 1, 0], None, **kw)


def test_rollout_argument_errors_honour_the_engines_kernel_hint():
    eng = _bare_engine()
    eng.kernel_hint = 'team4'
    with pytest.raises(ValueError, match='kernel'):
        eng.rollout(None, None, [0], None, sensor_noise='device', noise_seed=1)


def test_evaluate_pop_argument_errors_before_any_device_work(monkeypatch):
    import torch
    import serl_amd
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # a default engine would raise RuntimeError: the checks come first
    for kw, word in ((dict(sensor_noise='table'), 'sensor_noise'), (dict(seed=3), 'belong'), (dict(noise_episode=1), 'belong'),
                     (dict(sensor_noise='device', sensor_rng=np.random.RandomState(0)), 'sensor_rng'),
                     (dict(sensor_noise='device', seed=-1), 'seed'), (dict(sensor_noise='device', seed=2**64), 'seed'),
                     (dict(sensor_noise='device', seed=1, noise_episode=0.5), 'noise_episode'),
                     (dict(sensor_noise='device', seed=1, kernel='laneq'), 'kernel')):
        with pytest.raises(ValueError, match=word):
            serl_amd.evaluate_pop([None], mode='noise', **kw)


def test_evaluate_generation_argument_errors_before_any_device_work(monkeypatch):
    import torch, types
    from serl_amd import generation
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    args = types.SimpleNamespace(num_evals=1, noise_sd=0.1, noise_clip=0.5)
    for kw, word in ((dict(action_noise='host'), 'action_noise'), (dict(action_noise='device', rl_noise=np.zeros((5, 3))), 'rl_noise'),
                     (dict(noise_seed=1), 'belong'), (dict(noise_episode=2), 'belong')):
        with pytest.raises(ValueError, match=word):
            generation.evaluate_generation([], None, args=args, **kw)


def test_the_defaults_have_not_moved():
    import inspect
    import serl_amd
    from serl_amd import generation
    p = inspect.signature(serl_amd.RolloutEngine.rollout).parameters
    assert [p[n].default for n in ('sensor_noise', 'action_noise', 'noise_seed', 'noise_env', 'noise_episode', 'noise_sd', 'noise_clip')] == [None] * 7
    p = inspect.signature(serl_amd.evaluate_pop).parameters
    assert (p['sensor_noise'].default, p['seed'].default, p['noise_episode'].default, p['sensor_rng'].default) == (None, None, 0, None)
    p = inspect.signature(generation.evaluate_generation).parameters
    assert (p['action_noise'].default, p['noise_seed'].default, p['noise_episode'].default) == (None, None, 0)
    assert 'noise_seed' in serl_amd.evaluator.PopResult.__dataclass_fields__

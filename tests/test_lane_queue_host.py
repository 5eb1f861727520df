"""The boundary of the lane work-queue kernels (kernel_hint SERL_KERNEL_LANEQ, serl_rollout_laneq_kernel_<variant>) that needs no GPU: the hint's number in
the header and in the ctypes mirror, the ABI version it did not move, the `kernel` keyword of evaluate_pop and the development knob's documentation."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'serl_amd.h')


def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_defines_the_hint():
    h = _header()
    m = re.search(r'enum\s+serl_kernel_hint\s*\{([^}]*)\}', h)
    assert m, 'enum serl_kernel_hint not found'
    values = dict((k, int(v)) for k, v in re.findall(r'(SERL_KERNEL_\w+)\s*=\s*(\d+)', m.group(1)))
    assert values['SERL_KERNEL_LANEQ'] == 6
    assert values == {'SERL_KERNEL_AUTO': 0, 'SERL_KERNEL_TEAM': 1, 'SERL_KERNEL_WAVE': 2, 'SERL_KERNEL_HALF': 3, 'SERL_KERNEL_TEAM2': 4,
                      'SERL_KERNEL_TEAM4': 5, 'SERL_KERNEL_LANEQ': 6}      # the earlier hints keep their numbers


def test_ctypes_mirror_names_the_hint():
    from serl_amd import _capi
    assert _capi.KERNEL_HINTS['laneq'] == 6
    assert sorted(v for k, v in _capi.KERNEL_HINTS.items() if k not in (None, 'auto')) == [1, 2, 3, 4, 5, 6]


def test_abi_version_is_unchanged():
    from serl_amd import _capi
    assert _capi.lib().serl_abi_version() == 9 == _capi.ABI_VERSION
    assert re.search(r'#define\s+SERL_ABI_VERSION\s+9\b', _header())
    n = _capi.lib().serl_abi_layout(None, 0)
    assert n == len(_capi.expected_layout())      # no struct grew a member


def test_evaluate_pop_takes_a_kernel():
    from serl_amd import evaluator
    p = inspect.signature(evaluator.evaluate_pop).parameters
    assert 'kernel' in p and p['kernel'].default is None and p['kernel'].kind is inspect.Parameter.KEYWORD_ONLY
    assert 'laneq' in evaluator.evaluate_pop.__doc__


def test_header_documents_the_development_knob():
    h = _header()
    assert 'SERL_LANEQ_WAVES' in h
    assert re.search(r'SERL_KERNEL=[\w|]*\blaneq\b', h), 'SERL_KERNEL=laneq is not listed with the other development overrides'

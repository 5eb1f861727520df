"""The shape contracts of the kernels (serl_amd/csrc/serl_shapes.h) without a GPU: the header as plain C++, serl_shape_query against the
ranges and LDS footprints of every contract written out here as literals (taken from the C sources before the header existed, not computed by
the code under test), the 52 KB bound of serl_ga_novelty's footprint, and the table by which ga.sensitivity / ga.novelty /
ga.sort_groups_by_distance / distill.distil_batch resolve a kernel choice to ONE path -- with the query replaced by every combination of
takes / refused for range / refused for LDS and the library by one that counts its calls.  Planted slips show that each check can fail."""
import itertools, os, shutil, subprocess, types
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
TAKES, RANGE, LDS = 0, 1, 2
KB64, KB160 = 64 * 1024, 160 * 1024
LEARNER_LDS = 4 * (2 * 128 * 132 + 512 + 64 + 128)          # two tiles of 128 rows x 132 floats, red4 [4][128], red [64], one row of 128


def test_the_header_is_plain_cxx(tmp_path):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src = tmp_path / 'shapes.cpp'
    src.write_text('#include "%s"\nint main() { return serl_shape_of(SERL_SHAPE_GA_NOVELTY, 7, 3, 32, 3, 0, 1).why; }\n'
                   % os.path.join(ROOT, 'serl_amd', 'csrc', 'serl_shapes.h'))
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-fsyntax-only', str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_export_header_and_abi():
    import re
    from serl_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert 'serl_shape_query' in _capi.EXPORTS and hasattr(L, 'serl_shape_query') and re.search(r'^int serl_shape_query\(', hdr, re.M)
    assert re.search(r'#define SERL_ABI_VERSION 9\b', hdr) and L.serl_abi_version() == 9 == _capi.ABI_VERSION
    for name, k in _capi.SHAPE_KERNELS.items():
        assert re.search(r'SERL_SHAPE_%s = %d\b' % (name[5:].upper(), k), hdr), name
    assert L.serl_shape_query(None, 99, 7, 3, 32, 3, 0, 1, KB160, None) == INVALID and b'unknown kernel' in L.serl_last_error()


# ---- the contracts as literals ---------------------------------------------------------------------------------------------------------
def model(kernel, S, A, H, L, act, B, lds, slip=None):
    """-> (return code, why) of the entry point `kernel` for the shape; slip: a planted mistake"""
    act_ok = 0 <= act <= 2
    ga_h = 257 if slip == 'ga_hidden_257' else 256
    big = 513 if slip == 'batch_513' else 512
    lds_code = (UNSUPPORTED, RANGE) if slip == 'lds_is_range' else (UNSUPPORTED, LDS)

    def learner(Bmax, B):
        return 4 <= H <= 128 and H % 4 == 0 and 0 <= L <= 4 and 1 <= S <= 16 and 1 <= A <= 4 and 1 <= B <= Bmax
    if kernel in ('serl_ga_sensitivity', 'serl_ga_novelty'):
        if B <= 0:
            return INVALID, RANGE
        if not (1 <= S <= 64 and 1 <= A <= 16 and 2 <= H <= ga_h and 0 <= L <= 16 and act_ok):
            return UNSUPPORTED, RANGE
        need = S + 2 * (L + 1) * H + L * H + L + 2 * A + 16
        if kernel == 'serl_ga_sensitivity':
            need += H * S + L * H * H + A * H + 2 * H
        return lds_code if 4 * need > lds else (0, TAKES)
    if kernel == 'serl_ga_distill':
        if not (H == 32 and L == 3 and 1 <= S <= 16 and 1 <= A <= 4 and act_ok):
            return UNSUPPORTED, RANGE
        P = 32 * S + 32 + 3 * (32 * 32 + 3 * 32) + A * 32 + A
        return lds_code if 4 * (4 * ((P + 3) & ~3) + 6 * 32 * 128) > lds else (0, TAKES)
    if kernel in ('serl_td3_train', 'serl_td3_train_big'):
        if S < 1 or A < 1 or H < 1 or L < 0 or B < 1 or not act_ok:
            return INVALID, RANGE
        if not learner(128 if kernel == 'serl_td3_train' else big, B):
            return UNSUPPORTED, RANGE
        return lds_code if LEARNER_LDS > lds else (0, TAKES)
    if kernel in ('serl_ga_sensitivity_general', 'serl_ga_novelty_general', 'serl_ga_distill_general'):
        if kernel == 'serl_ga_sensitivity_general' and B <= 0:
            return INVALID, RANGE
        if not (learner(big, 1 if kernel == 'serl_ga_distill_general' else B) and act_ok):
            return UNSUPPORTED, RANGE
        return lds_code if LEARNER_LDS > lds else (0, TAKES)
    if kernel == 'serl_venv_rollout':
        if B != 0 or (S, H, A) != (7, 32, 3) or L < 0 or not act_ok:
            return INVALID, RANGE
        return 0, TAKES
    assert kernel == 'serl_venv_rollout_general'
    if not 0 <= B <= 5:
        return INVALID, RANGE
    cfg, inc = B % 3, B // 3
    A_env = 1 if cfg == 1 else 3
    S_env = A_env + (4, 1, 10)[cfg] + (A_env if inc else 0)
    if (S, A) != (S_env, A_env):
        return INVALID, RANGE
    if not (4 <= H <= 128 and H % 4 == 0) or not 0 <= L <= 16:
        return UNSUPPORTED, RANGE
    return (0, TAKES) if act_ok else (INVALID, RANGE)


def library(kernel, S, A, H, L, act, B, lds):
    import ctypes
    from serl_amd import _capi
    why = ctypes.c_int32(-7)
    rc = _capi.lib().serl_shape_query(None, _capi.SHAPE_KERNELS[kernel], S, A, H, L, act, B, lds, ctypes.byref(why))
    return rc, why.value


# the grid around every bound, and per contract a second one around the bounds the first does not reach (S = 7, A = 3, the env codes ...)
GRID = dict(H=(2, 4, 30, 32, 128, 132, 256, 258), L=(0, 3, 4, 5, 16, 17), S=(16, 17, 64, 65), A=(4, 5, 16, 17), B=(0, 1, 128, 129, 512, 513),
            act=(-1, 0, 2, 3))
NEAR = dict(H=(0, 1, 2, 4, 32, 36, 72, 128, 256, 257), L=(-1, 0, 3, 4, 16), S=(0, 1, 2, 7, 10, 13), A=(0, 1, 3), B=(-1, 0, 1, 2, 3, 5, 6), act=(0,))


def mismatches(query, kernels, grids=(GRID, NEAR), slip=None):
    bad = []
    for kernel in kernels:
        for g in grids:
            for S, A, H, L, act, B in itertools.product(g['S'], g['A'], g['H'], g['L'], g['act'], g['B']):
                for lds in (KB64, KB160):
                    if query(kernel, S, A, H, L, act, B, lds) != model(kernel, S, A, H, L, act, B, lds, slip):
                        bad.append((kernel, S, A, H, L, act, B, lds))
    return bad


def test_the_query_is_the_literal_contract_over_the_grid():
    from serl_amd import _capi
    assert mismatches(library, list(_capi.SHAPE_KERNELS)) == []
    # every outcome occurs: the grid can tell them apart
    seen = {library(k, S, A, H, L, 0, B, lds) for k in _capi.SHAPE_KERNELS for S, A, H, L, B, lds in
            ((7, 3, 32, 3, 1, KB160), (7, 3, 128, 3, 1, KB160), (7, 3, 32, 3, 1, KB64), (7, 3, 32, 3, 0, KB160), (7, 3, 130, 3, 1, KB160))}
    assert seen == {(0, TAKES), (UNSUPPORTED, RANGE), (UNSUPPORTED, LDS), (INVALID, RANGE)}


def test_refusals_carry_the_entry_points_own_message():
    from serl_amd import _capi
    spec = types.SimpleNamespace(state_dim=7, action_dim=3, hidden=128, num_layers=3, activation_id=0)
    v = _capi.shape_query('serl_ga_sensitivity', spec, 4, lds_bytes=KB160)          # ~208 KB: the one LDS refusal a 160 KB device can show
    assert (v.rc, v.why, v.message) == (UNSUPPORTED, LDS, 'serl_ga_sensitivity: network too large for the LDS-resident accumulators') and v.lds
    with pytest.raises(RuntimeError, match=r'serl_ga_sensitivity failed \(-3\): serl_ga_sensitivity: network too large'):
        v.check()
    assert _capi.shape_query('serl_ga_sensitivity', spec, 4, lds_bytes=256 * 1024).takes
    spec.hidden = 130
    tail = 'compiled for hidden a multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, state_dim 1 .. 16, action_dim 1 .. 4, '
    for what, rest in (('serl_ga_sensitivity_general', 'the three activations, minibatches of 1 .. 512 rows'),
                       ('serl_ga_novelty_general', 'the three activations, minibatches of 1 .. 512 rows'),
                       ('serl_ga_distill_general', 'the three activations'),
                       ('serl_td3_train', 'minibatches of 1 .. 128 rows; other shapes train in PyTorch'),
                       ('serl_td3_train_big', 'minibatches of 1 .. 512 rows; other shapes train in PyTorch')):
        v = _capi.shape_query(what, spec, 4, lds_bytes=KB160)
        assert (v.rc, v.why, v.message) == (UNSUPPORTED, RANGE, what + ': ' + tail + rest)
    assert _capi.shape_query('serl_ga_novelty', spec, 4, lds_bytes=KB160).takes
    spec.hidden = 258
    assert _capi.shape_query('serl_ga_novelty', spec, 4, lds_bytes=KB160).message == 'serl_ga_novelty: network shape out of range'
    assert _capi.shape_query('serl_ga_distill', spec, 4, lds_bytes=KB160).message.startswith('serl_ga_distill: compiled for the SERL50 actor family')
    assert _capi.shape_query('serl_venv_rollout', spec, 0).message.startswith('serl_venv_rollout: the in-kernel actor is 7 -> 32 .. -> 3 only')
    assert _capi.shape_query('serl_venv_rollout_general', spec, 0).message == 'serl_venv_rollout_general: hidden must be a multiple of 4 in 4 .. 128'


def test_novelty_lds_footprint_stays_under_52_kb_over_the_whole_range():
    """why sort_groups_by_distance(kernel='auto') may ask the context's LDS where it used to test against a fixed 64 KB: serl_ga_novelty's
    footprint is at most 51 712 bytes, so neither rule ever finds a shape refused for LDS.  The footprint grows with each of S, A, H, L:
    S and A at their maxima, every H and L."""
    for H in range(2, 257):
        for L in range(17):
            assert library('serl_ga_novelty', 64, 16, H, L, 0, 1, 52 * 1024) == (0, TAKES), (H, L)
    assert library('serl_ga_novelty', 64, 16, 256, 16, 0, 1, 51712) == (0, TAKES)
    assert library('serl_ga_novelty', 64, 16, 256, 16, 0, 1, 51711) == (UNSUPPORTED, LDS)


@pytest.mark.parametrize('slip', ['ga_hidden_257', 'batch_513', 'lds_is_range'])
def test_planted_slips_in_a_contract_are_caught(slip):
    """a query that has one bound off by one, or that reports an LDS refusal as a range refusal, differs from the literal contract on the grid"""
    from serl_amd import _capi
    bad = mismatches(lambda *a: model(*a, slip=slip), list(_capi.SHAPE_KERNELS))
    assert bad, slip
    hit = {c[0] for c in bad}
    assert hit <= {'ga_hidden_257': {'serl_ga_sensitivity', 'serl_ga_novelty'},
                   'batch_513': {'serl_td3_train_big', 'serl_ga_sensitivity_general', 'serl_ga_novelty_general'},
                   'lds_is_range': set(_capi.SHAPE_KERNELS) - {'serl_venv_rollout', 'serl_venv_rollout_general', 'serl_ga_novelty'}}[slip]


# ---- the resolution table -----------------------------------------------------------------------------------------------------------------
class Library:
    """counts the entry points that are called"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*a):
            self.calls.append(name)
            return 0
        return entry


def verdict(what, how):
    from serl_amd import _capi
    rc, why = {'takes': (0, TAKES), 'range': (UNSUPPORTED, RANGE), 'lds': (UNSUPPORTED, LDS)}[how]
    return _capi.Shape(what, rc, why, '' if rc == 0 else '%s: refused for %s' % (what, how))


HOW = ('takes', 'range', 'lds')


def expected_ga(kernel, lds_how, general_how, fallback):
    """the parent's table -> 'lds' | 'general' | 'torch' | 'error' (the LDS kernel's own refusal)"""
    if kernel == 'general':
        return 'general'
    if lds_how == 'takes':
        return 'lds'
    if lds_how == 'lds':
        if kernel == 'auto' and general_how == 'takes':
            return 'general'
        if fallback:
            return 'torch'
    return 'error'


def ga_table(resolve):
    """every (entry, kernel, fallback) under every answer of the two queries: [(case, got, want)] where they differ"""
    engine = types.SimpleNamespace(ctx=None)
    spec = types.SimpleNamespace(state_dim=7, action_dim=3, hidden=128, num_layers=3, activation_id=0)
    bad = []
    for entry, kernel, fallback, lds_how, general_how in itertools.product(('serl_ga_sensitivity', 'serl_ga_novelty'), ('lds', 'general', 'auto'),
                                                                           (False, True), HOW, HOW):
        answers = {entry: lds_how, entry + '_general': general_how}
        try:
            got = resolve(engine, spec, 4, kernel, entry, fallback, lambda what, *a, **k: verdict(what, answers[what]))
        except RuntimeError as e:
            got = 'error' if str(e) == '%s failed (-3): %s: refused for %s' % (entry, entry, lds_how) else 'another error: %s' % e
        want = expected_ga(kernel, lds_how, general_how, fallback)
        if got != want:
            bad.append(((entry, kernel, fallback, lds_how, general_how), got, want))
    return bad


def _real_ga_resolve(monkeypatch):
    from serl_amd import _capi, ga

    def resolve(engine, spec, B, kernel, entry, fallback, query):
        monkeypatch.setattr(_capi, 'shape_query', query)
        return ga.resolve(engine, spec, B, kernel, entry, fallback)
    return resolve


def test_ga_resolution_table_is_the_parents(monkeypatch):
    assert ga_table(_real_ga_resolve(monkeypatch)) == []


def test_planted_slips_in_the_ga_resolution_are_caught():
    def general_first(engine, spec, B, kernel, entry, fallback, query):          # 'auto' prefers the general kernel
        if kernel == 'general' or (kernel == 'auto' and query(entry + '_general').takes):
            return 'general'
        v = query(entry)
        if v.lds and fallback:
            return 'torch'
        v.check()
        return 'lds'

    def torch_for_range(engine, spec, B, kernel, entry, fallback, query):        # PyTorch for any refusal, where the parent raises for a range
        if kernel == 'general':
            return 'general'
        v = query(entry)
        if not v.takes:
            if kernel == 'auto' and v.lds and query(entry + '_general').takes:
                return 'general'
            if fallback:
                return 'torch'
        v.check()
        return 'lds'
    for slipped in (general_first, torch_for_range):
        assert ga_table(slipped) != [], slipped.__name__


def _ga_setup(monkeypatch, answers):
    import serl_amd
    from serl_amd import _capi, ga
    lib = Library()
    engine = types.SimpleNamespace(ctx=None, lib=lib)
    monkeypatch.setattr(_capi, 'shape_query', lambda what, *a, **k: verdict(what, answers[what]))
    monkeypatch.setattr(ga, '_stream', lambda dev: None)
    monkeypatch.setattr(ga, '_sens_workspace', lambda *a: (None, 0))
    monkeypatch.setattr(ga, 'sensitivity_torch', lambda *a: lib.calls.append('torch') or 'torch')
    spec = serl_amd.NetSpec(7, 3, 8, 1, 'tanh')
    return ga, lib, engine, spec, torch.zeros(2, spec.param_count)


@pytest.mark.parametrize('lds_how,general_how', list(itertools.product(HOW, HOW)))
def test_sensitivity_and_novelty_make_exactly_one_call_per_resolution(monkeypatch, lds_how, general_how):
    """one entry point of the library (or sensitivity_torch) per call, the one the table names, and none before a refusal raises.  (The
    workspace's size function is no entry point that launches: it is replaced here.)"""
    for fn, entry in (('sensitivity', 'serl_ga_sensitivity'), ('novelty', 'serl_ga_novelty')):
        ga, lib, engine, spec, w = _ga_setup(monkeypatch, {entry: lds_how, entry + '_general': general_how})
        for kernel, fallback in itertools.product(('lds', 'general', 'auto'), (False, True)):
            if fn == 'novelty' and fallback:
                continue                      # (novelty has no PyTorch path)
            del lib.calls[:]
            st, ac = torch.zeros(1, 4, 7), torch.zeros(1, 4, 3)
            call = (lambda: ga.sensitivity(engine, w, [0], spec, st, fallback=fallback, kernel=kernel)) if fn == 'sensitivity' else \
                   (lambda: ga.novelty(engine, w, [0], spec, st, ac, kernel=kernel))
            want = expected_ga(kernel, lds_how, general_how, fallback)
            if want == 'error':
                with pytest.raises(RuntimeError, match='refused for ' + lds_how):
                    call()
                assert lib.calls == [], (fn, kernel, fallback)
            else:
                call()
                assert lib.calls == [{'lds': entry, 'general': entry + '_general', 'torch': 'torch'}[want]], (fn, kernel, fallback)


def test_an_empty_batch_is_ones_before_anything_is_asked(monkeypatch):
    ga, lib, engine, spec, w = _ga_setup(monkeypatch, {})                # (any query would be a KeyError)
    out = ga.sensitivity(engine, w, [0, 1], spec, torch.zeros(2, 0, 7), kernel='auto')
    assert out.shape == (2, ga.genome_size(spec)) and bool((out == 1).all()) and lib.calls == []


@pytest.mark.parametrize('lds_how,general_how', list(itertools.product(HOW, HOW)))
def test_sort_groups_auto_is_general_only_where_lds_is_refused_for_lds_and_general_takes_batch_1(monkeypatch, lds_how, general_how):
    from serl_amd import ga
    asked = []

    def query(what, spec, batch=1, ctx=None, lds_bytes=0):
        asked.append((what, batch))
        return verdict(what, {'serl_ga_novelty': lds_how, 'serl_ga_novelty_general': general_how}[what])
    ga_, lib, engine, spec, w = _ga_setup(monkeypatch, {})
    monkeypatch.setattr(ga._capi, 'shape_query', query)
    ring = types.SimpleNamespace(rows=torch.zeros(8, 20), device=torch.device('cpu'), split=lambda r: (r[:, :7], r[:, 7:10], None, None, None))
    plan = dict(pairs=[(1, 0, 4)], members=np.asarray([0, 1], np.int32), rings=[ring, ring], batch=np.asarray([4, 4], np.int32),
                slots=np.zeros((2, 4), np.int32), calls=[1, 0])
    monkeypatch.setattr(ga, 'distance_plan', lambda *a: plan)
    ran = []
    monkeypatch.setattr(ga, '_distance_general', lambda *a: ran.append('general') or np.zeros(2))
    monkeypatch.setattr(ga, 'novelty', lambda *a, **k: ran.append('lds') or torch.zeros(2))
    for kernel in ('lds', 'general', 'auto'):
        del ran[:], asked[:]
        ga.sort_groups_by_distance(engine, w, [0, 1], {}, spec, kernel=kernel)
        want = 'general' if kernel == 'general' or (kernel == 'auto' and lds_how == 'lds' and general_how == 'takes') else 'lds'
        assert ran == [want], kernel
        assert all(b == 1 for _, b in asked) and (asked == [] or kernel == 'auto')


def expected_distil(kernel, dense, cuda, fused_how, general_how):
    general_path = 'fused-general-mfma' if dense == 'mfma' else 'fused-general'
    if kernel == 'general':
        return general_path if cuda and general_how == 'takes' else 'error'
    if cuda and fused_how == 'takes':
        return 'fused'
    if kernel == 'auto' and cuda and general_how == 'takes':
        return general_path
    return 'torch'


def distil_table(resolve):
    spec = types.SimpleNamespace(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation_id=0)
    engine = types.SimpleNamespace(ctx=None)
    bad = []
    for kernel, dense, cuda, fused_how, general_how in itertools.product(('serl50', 'general', 'auto'), ('valu', 'mfma'), (False, True), HOW, HOW):
        if kernel == 'serl50' and dense == 'mfma':
            continue                          # (a ValueError of the validator)
        answers = {'serl_ga_distill': fused_how, 'serl_ga_distill_general': general_how}
        try:
            got = resolve(engine, spec, torch.device('cuda', 0) if cuda else torch.device('cpu'), kernel, dense,
                          lambda what, *a, **k: verdict(what, answers[what]))
        except RuntimeError as e:
            ok = str(e).startswith("distil_batch(kernel='general'): serl_ga_distill_general does not run") and \
                str(e).endswith(': serl_ga_distill_general: refused for %s' % general_how if cuda else ' on cpu')
            got = 'error' if ok else 'another error: %s' % e
        want = expected_distil(kernel, dense, cuda, fused_how, general_how)
        if got != want:
            bad.append(((kernel, dense, cuda, fused_how, general_how), got, want))
    return bad


def test_distil_resolution_table_is_the_parents_and_calls_nothing(monkeypatch):
    from serl_amd import _capi, distill
    lib = Library()
    monkeypatch.setattr(_capi, 'lib', lambda: lib)

    def resolve(engine, spec, dev, kernel, dense, query):
        monkeypatch.setattr(_capi, 'shape_query', query)
        return distill.resolve(engine, spec, dev, kernel, dense)
    assert distil_table(resolve) == [] and lib.calls == []

    def torch_where_general_refuses(engine, spec, dev, kernel, dense, query):          # a planted slip: 'general' falls back where the parent raises
        if kernel == 'general' and not (dev.type == 'cuda' and query('serl_ga_distill_general').takes):
            return 'torch'
        return resolve(engine, spec, dev, kernel, dense, query)

    def general_before_fused(engine, spec, dev, kernel, dense, query):                 # ... and 'auto' that asks the general kernel first
        if kernel == 'auto' and dev.type == 'cuda' and query('serl_ga_distill_general').takes:
            return 'fused-general-mfma' if dense == 'mfma' else 'fused-general'
        return resolve(engine, spec, dev, kernel, dense, query)
    assert distil_table(torch_where_general_refuses) != [] and distil_table(general_before_fused) != []


def test_one_validator_keeps_the_three_messages():
    from serl_amd import ga, distill
    with pytest.raises(ValueError, match=r"^sensitivity: dense='mfma' needs kernel='general' or 'auto' \(serl_ga_sensitivity has no matrix-core phases\)$"):
        ga.check_choice('sensitivity', 'lds', 'mfma', 'serl_ga_sensitivity')
    with pytest.raises(ValueError, match=r"^novelty: kernel must be one of lds, general, auto, not 'x'$"):
        ga.check_choice('novelty', 'x', 'valu', 'serl_ga_novelty')
    with pytest.raises(ValueError, match=r"^distil_batch: kernel must be one of serl50, general, auto, not 'lds'$"):
        ga.check_choice('distil_batch', 'lds', 'valu', 'serl_ga_distill', distill.KERNELS)
    with pytest.raises(ValueError, match=r"^distil_batch: dense='mfma' needs kernel='general' or 'auto' \(serl_ga_distill has no matrix-core phases\)$"):
        ga.check_choice('distil_batch', 'serl50', 'mfma', 'serl_ga_distill', distill.KERNELS)
    with pytest.raises(ValueError, match=r"^SSNE: dense must be one of valu, mfma, not 'f32'$"):
        ga.check_choice('SSNE', 'auto', 'f32', 'serl_ga_novelty')
    for name in ('_kernel_shape_ok', '_general_takes', '_novelty_lds_fits', '_check_sens_choice', '_check_nov_choice'):
        assert not hasattr(ga, name), name
    assert not hasattr(distill, '_probe')

"""serl_ga_sensitivity_general without a GPU: the float64 contract of tests/sens64.py (autograd against the hand-written restatement, the
planted mistakes, the grid's coverage, the float32 reference under the bound and the exclusion cap), the new symbols, the workspace
size and the argument checks in their documented order, and the kernel / dense choices of the Python layer."""
import ctypes, os, re, sys
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sens64 as Z


@pytest.mark.parametrize('key', Z.ALL_KEYS, ids=Z.key_id)
def test_hand_written_contract_equals_autograd(key):
    case, raw = Z.reference(key)
    for k, m in enumerate(case['members']):
        got = Z.explicit64(case, case['weights'][m], case['states'][k])
        np.testing.assert_allclose(got, Z.clamp(raw[k]), rtol=1e-9, atol=1e-13, err_msg='%s member %d' % (Z.key_id(key), m))


@pytest.mark.parametrize('mistake', Z.MISTAKES)
def test_planted_mistakes_exceed_the_bound(mistake):
    """every mistake fails the check of some case: a compared element off by more than TOL (NaN counts: compare() turns it into inf), or
    -- the clamps in the other order, which turn every exact 0 into 0.01, the value a tiny non-zero gradient would legitimately have
    -- more than EXCLUDED_CAP of a member's entries zero in one run and not in the other"""
    worst, share = 0.0, 0.0
    for key in Z.ALL_KEYS:
        case, raw = Z.reference(key)
        for k, m in enumerate(case['members']):
            with np.errstate(all='ignore'):
                got = Z.explicit64(case, case['weights'][m], case['states'][k], mistake)
            e, x = Z.compare(got, raw[k])
            worst, share = max(worst, e), max(share, x)
    print('%s: worst err %.3e (bound %.3e), worst excluded share %.3f' % (mistake, worst, Z.TOL, share))
    if mistake == 'clamp_order':
        assert share > Z.EXCLUDED_CAP, (mistake, worst, share)
    else:
        assert worst > Z.TOL, (mistake, worst)


def test_grid_covers_what_it_claims():
    G = Z.GRID
    assert {c[5] for c in G} >= {1, 3, 64, 65, 128, 129, 256, 512}
    assert {c[2] for c in G} >= {4, 32, 72, 128} and {c[3] for c in G} >= {0, 1, 3, 4}
    assert {(c[0], c[1]) for c in G} >= {(7, 3), (1, 1), (16, 4)}
    for act in ('tanh', 'elu', 'relu'):
        assert sum(c[4] == act for c in G) >= 2, act
    assert any(c[6] > 0 for c in G) and (7, 3, 128, 3) in {c[:4] for c in G}
    assert any(len(set(c[7])) < len(c[7]) and list(c[7]) == sorted(c[7], reverse=True) for c in G)
    L = _lib()
    for c in G:
        assert L.serl_ga_sensitivity_general_work_bytes(len(c[7]), c[0], c[1], c[2], c[3], c[5]) > 0, c
    # the degenerate cases are what they say
    case, raw = Z.reference('sd0')
    H, S = case['H'], case['S']
    g1 = H * S + H * H                                   # hidden layer 1's W in genome order
    assert (raw[1][:g1] == 0).all() and (raw[1][g1:g1 + H * H] > 0.02).any()       # nothing flows below; the layer's own gradient does
    case, raw = Z.reference('wo0')
    G_ = Z.genome_size(case['S'], case['A'], case['H'], case['L'])
    k = case['members'].index(1)
    assert (raw[k][:G_ - case['A'] * case['H']] == 0).all() and (raw[k][G_ - case['A'] * case['H']:] > 0).all()
    case, raw = Z.reference('small')
    assert all(((r > 0) & (r < 0.01)).mean() > Z.SMALL_SHARE for r in raw)


@pytest.mark.parametrize('key', Z.ALL_KEYS, ids=Z.key_id)
def test_float32_reference_meets_bound_and_cap(key):
    """ga.sensitivity_torch in float32 on the CPU (whatever summation order this machine's threads give it): within TOL of the float64
    run and under the exclusion cap in every case"""
    got = Z.torch32(key)
    _, raw = Z.reference(key)
    for k in range(len(got)):
        err, share = Z.compare(got[k], raw[k])
        print('%s member %d: err %.3e excluded %.4f %%' % (Z.key_id(key), k, err, 100 * share))
        assert err <= Z.TOL and share <= Z.EXCLUDED_CAP


def test_tolerance_is_four_times_the_measured_reference():
    """TOL is 4 x the figure written down in sens64.py; measured again here -- torch's f32 sums depend on the machine's thread count, 2.1e-4
    and 2.4e-4 have been seen -- the reference's worst error over GRID x four seeds leaves at least a factor of two below TOL and is no
    less than a sixteenth of it: the bound is neither exhausted by the reference nor inflated"""
    assert Z.TOL == 4 * Z.WORST_REF
    worst, share = Z.measure_reference(verbose=False)
    print('float32 reference: worst err %.3e (TOL %.3e), worst excluded share %.4f %%' % (worst, Z.TOL, 100 * share))
    assert Z.TOL / 16 <= worst <= Z.TOL / 2 and share <= Z.EXCLUDED_CAP


def _lib():
    from serl_amd import _capi
    return _capi.lib()


def test_exports_header_and_work_bytes():
    from serl_amd import _capi
    L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    for f in ('serl_ga_sensitivity_general', 'serl_ga_sensitivity_general_work_bytes'):
        assert f in _capi.EXPORTS and hasattr(L, f) and re.search(r'^int(64_t)? %s\(' % f, hdr, re.M), f
    assert re.search(r'#define SERL_ABI_VERSION 9\b', hdr) and L.serl_abi_version() == 9 == _capi.ABI_VERSION
    wb = L.serl_ga_sensitivity_general_work_bytes
    one = wb(1, 7, 3, 72, 3, 86)
    assert one > 0 and wb(5, 7, 3, 72, 3, 86) == 5 * one
    assert wb(1, 7, 3, 72, 3, 128) == one < wb(1, 7, 3, 72, 3, 129) < wb(1, 7, 3, 72, 3, 257) < wb(1, 7, 3, 72, 3, 512)
    assert wb(1, 7, 3, 128, 3, 86) >= 4 * Z.genome_size(7, 3, 128, 3)
    for inside in ((1, 1, 1, 4, 0, 1), (1, 16, 4, 128, 4, 512)):
        assert wb(*inside) > 0, inside
    for bad in ((0, 7, 3, 72, 3, 86), (1, 7, 3, 70, 3, 86), (1, 7, 3, 132, 3, 86), (1, 7, 3, 0, 3, 86), (1, 17, 3, 72, 3, 86), (1, 0, 3, 72, 3, 86),
                (1, 7, 3, 72, 5, 86), (1, 7, 3, 72, -1, 86), (1, 7, 5, 72, 3, 86), (1, 7, 0, 72, 3, 86), (1, 7, 3, 72, 3, 0), (1, 7, 3, 72, 3, 513)):
        assert wb(*bad) == 0, bad


def test_argument_checks_in_the_documented_order_without_a_gpu():
    """INVALID (pointers, counts) -> INVALID (dense) -> UNSUPPORTED (shape) -> OK (no members) -> INVALID (stride) -> INVALID (work): none
    of them reads the context or launches (a NULL context is itself refused)"""
    from serl_amd import _capi
    L = _lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    ctx = ctypes.c_void_p(p)                            # never dereferenced: every call below returns from the argument checks
    P = 72 * 7 + 72 + 3 * (72 * 72 + 3 * 72) + 3 * 72 + 3
    big = 1 << 40

    def call(ctx=ctx, weights=p, stride=P, S=7, H=72, L_=3, A=3, act=0, members=p, n=2, states=p, batch=86, scaling=p, work=p, work_bytes=big,
             dense=0):
        return L.serl_ga_sensitivity_general(ctx, weights, stride, S, H, L_, A, act, members, n, states, batch, scaling, work, work_bytes, dense, None)
    for kw in (dict(ctx=None), dict(weights=None), dict(members=None), dict(states=None), dict(scaling=None), dict(n=-1), dict(batch=0),
               dict(batch=-3), dict(dense=2), dict(dense=-1)):
        assert call(**kw) == _capi.E_INVALID, kw
        assert L.serl_last_error()
    for kw in (dict(H=132), dict(H=70), dict(H=0), dict(L_=5), dict(L_=-1), dict(S=17), dict(S=0), dict(A=5), dict(A=0), dict(act=3), dict(act=-1),
               dict(batch=513)):
        assert call(**kw) == _capi.E_UNSUPPORTED, kw
        assert b'serl_ga_sensitivity_general' in L.serl_last_error() and b'4 .. 128' in L.serl_last_error()
    # the order: a bad pointer wins over a bad dense, a bad dense over a bad shape, a bad shape over everything behind it
    assert call(scaling=None, dense=7, H=70) == _capi.E_INVALID and b'bad argument' in L.serl_last_error()
    assert call(dense=7, H=70) == _capi.E_INVALID and b'dense' in L.serl_last_error()
    assert call(H=70, n=0) == _capi.E_UNSUPPORTED and call(H=70, stride=1, work=None) == _capi.E_UNSUPPORTED
    # no members: OK without a workspace, whatever the stride
    assert call(n=0, work=None, work_bytes=0, stride=1) == 0
    assert call(stride=P - 1, work=None) == _capi.E_INVALID and b'stride' in L.serl_last_error()
    need = L.serl_ga_sensitivity_general_work_bytes(2, 7, 3, 72, 3, 86)
    for kw in (dict(work=None), dict(work_bytes=need - 1), dict(work_bytes=0), dict(work_bytes=-1)):
        assert call(**kw) == _capi.E_INVALID and b'workspace' in L.serl_last_error(), kw


def test_python_choices_are_checked():
    import serl_amd
    from serl_amd import ga, ssne
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    w, st = torch.zeros(2, spec.param_count), torch.zeros(1, 4, 7)
    with pytest.raises(ValueError, match='kernel must be one of'):
        ga.sensitivity(None, w, [0], spec, st, kernel='bogus')
    with pytest.raises(ValueError, match='dense must be one of'):
        ga.sensitivity(None, w, [0], spec, st, dense='bogus')
    with pytest.raises(ValueError, match='needs kernel'):
        ga.sensitivity(None, w, [0], spec, st, kernel='lds', dense='mfma')
    with pytest.raises(ValueError, match='kernel must be one of'):
        ga.ProximalBatch(None, w, spec, 0.1, 86, kernel='bogus')
    with pytest.raises(ValueError, match='dense must be one of'):
        ga.proximal_mutate(None, w, 0, spec, 0.1, None, 86, dense='bogus')
    import types
    args = types.SimpleNamespace(pop_size=4, elite_fraction=0.25, mut_type='proximal')
    with pytest.raises(ValueError, match='kernel must be one of'):
        ssne.SSNE(args, None, spec, sensitivity_kernel='bogus')
    with pytest.raises(ValueError, match='dense must be one of'):
        ssne.SSNE(args, None, spec, sensitivity_dense='bogus')
    s = ssne.SSNE(args, None, spec, sensitivity_kernel='general', sensitivity_dense='mfma')
    assert (s.sensitivity_kernel, s.sensitivity_dense) == ('general', 'mfma')
    assert (ssne.SSNE(args, None, spec).sensitivity_kernel, ssne.SSNE(args, None, spec).sensitivity_dense) == ('lds', 'valu')

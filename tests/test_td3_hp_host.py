"""CPU tests of the hyper-parameter grid of tests/td3_hp.py: the written-out float64 loop equals the literal one at every point, every
case trains, the clip points do what they are named for in BOTH networks, float32 torch meets the bound each case is held to, and every
planted mistake that only a run away from the default hyper-parameters or from a cold start can show exceeds it on a named case."""
import functools
import numpy as np
import pytest
import torch
import td3_64 as T
import td3_hp as H


@functools.lru_cache(maxsize=None)
def _case(c):
    d = H.make_case(c)
    return d, T.td3_literal(d, **H.state_of(d))


def test_grid_covers_the_points():
    assert 25 <= len(H.CASES) <= 40 and len(set(H.CASES)) == len(H.CASES)
    for name, (over, rew, steps0, shapes) in H.POINTS.items():
        assert len(shapes) >= 2 and set(shapes) <= set(H.SHAPES), name
        assert set(over) <= set(T.DEFAULT_HP), name
        if name != 'ref_defaults':              # one field (the two lambdas count as one) away from td3_64's constants
            assert len(set(over) - {'lambda_s', 'lambda_t'}) <= 1 and all(T.DEFAULT_HP[k] != v for k, v in over.items()), name
    assert {sh for _, sh in H.CASES} == set(H.SHAPES) and {H.SHAPES[sh][4] for sh in H.SHAPES} == {'tanh', 'elu', 'relu'}
    for sh, (S, A, Hd, L, act, B, freq, it0, n) in H.SHAPES.items():
        assert freq == 2 and (it0 + 1) % freq != 0 and n % freq != 0 and 8 <= n <= 12, sh
    hp = lambda name: T.hyper(H.POINTS[name][0])
    assert (hp('tau0')['tau'], hp('tau1')['tau'], hp('gamma0')['gamma'], hp('gamma1')['gamma']) == (0.0, 1.0, 0.0, 1.0)
    assert hp('noise_sd0')['noise_sd'] == 0.0 and hp('noise_clip0')['noise_clip'] == 0.0 and hp('noise_clip5')['noise_clip'] == 5.0
    assert hp('eps_sd0')['eps_sd'] == 0.0 and hp('eps_sd0')['lambda_s'] > 0 and hp('lambdas0')['lambda_s'] == hp('lambdas0')['lambda_t'] == 0.0
    assert (hp('lambdas_apart')['lambda_s'], hp('lambdas_apart')['lambda_t']) == (2.0, 0.01) and hp('lambda_t_negative')['lambda_t'] < 0
    assert H.POINTS['warm700'][2] == (700, 350) and H.POINTS['warm40000'][2] == (40000, 20000)
    r = hp('ref_defaults')
    assert (r['gamma'], r['tau'], r['noise_sd'], r['noise_clip'], r['max_norm']) == (0.98, 0.005, 0.2962183114680794, 0.5, 10.0)
    assert r['lr'] == pytest.approx(H.REF_LR_FACTOR * 0.0004335) and (r['lambda_s'], r['lambda_t'], r['eps_sd']) == (0.5, 0.1, 0.05)
    import serl_amd.td3 as td3
    assert td3.CAPS == dict(lambda_s=0.5, lambda_t=0.1, eps_sd=0.05) and td3.MAX_GRAD_NORM == 10.0
    # |noise_sd z| stays below noise_clip 5 in every draw of the cases of that point: the clamp is never active there
    for c in H.CASES:
        d = H.make_case(c)
        assert d['caps'] and d['uat'] and d['hp'] == hp(c[0])
        if c[0] == 'noise_clip5':
            assert np.abs(d['tn']).max() * d['hp']['noise_sd'] < 5.0
        if c[0] in ('noise_clip0', 'noise_sd0'):
            assert np.abs(d['tn']).min() > 0.0


def test_defaults_are_todays_constants():
    """hp, steps0 and moments left out, given as the defaults, or given as zeros: td3_literal and td3_explicit64 compute what they did"""
    d = T.make_case(T.CASES[3])
    zeros = {k: np.zeros(len(d[k.split('_')[0]]), np.float32) for k in T.MOMENTS}
    a = T.td3_literal(d)
    for kw in (dict(hp=dict(T.DEFAULT_HP)), dict(steps0=(0, 0), moments0=zeros)):
        b, e = T.td3_literal(d, **kw), T.td3_explicit64(d, **kw)
        for k in T.ROWS + T.MOMENTS + ('td', 'pg'):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
            np.testing.assert_allclose(e[k], a[k], rtol=0, atol=1e-11, equal_nan=True, err_msg=k)
    assert T.DEFAULT_HP == dict(lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP, max_norm=T.MAX_NORM, **T.CAPS)
    assert not set(T.HP_MISTAKES) & set(T.MISTAKES)


@pytest.mark.parametrize('c', H.CASES, ids=H.case_id)
def test_float32_loop_meets_the_bound(c):
    """the calibration, asserted on the grid's own seeds: the literal loop in float32 torch is within the case's bound of the float64
    run, every case moves actor and critic by more than MIN_MOVED (inside check), the clip points hold in every step of both networks,
    and the written-out loop equals the literal one to the bound tests/test_td3_host.py uses"""
    d, ref = _case(c)
    assert len(ref['clip_c']) == d['n'] and len(ref['clip_a']) == d['n_actor'] >= 4
    if c[0] == 'clip_active':
        assert all(ref['clip_c']) and all(ref['clip_a']), (ref['clip_c'], ref['clip_a'])
    elif c[0] == 'clip_inactive':
        assert d['rew'] == 'big' and not any(ref['clip_c']) and not any(ref['clip_a']), (ref['clip_c'], ref['clip_a'])
        # ... where td3_64's max_norm of 10 would have been active in every critic step
        assert all(T.td3_literal(d, **dict(H.state_of(d), hp=None))['clip_c'])
    T.check(T.td3_literal(d, torch.float32, **H.state_of(d)), ref, d, H.case_id(c), tol=H.tol_of(c, d['act']))
    ex = T.td3_explicit64(d, **H.state_of(d))
    for k in T.ROWS + T.MOMENTS + ('td',):
        np.testing.assert_allclose(ex[k], ref[k], rtol=0, atol=1e-11, err_msg=k)
    np.testing.assert_allclose(ex['pg'], ref['pg'], rtol=0, atol=1e-11, equal_nan=True)
    assert ex['clip_c'] == ref['clip_c'] and ex['clip_a'] == ref['clip_a']


def test_no_relu_case_sits_on_the_kink(monkeypatch):
    """td3_hp.SEED_OF's criterion on the whole grid: in the float64 run of every leaky-relu case no unit's pre-activation is within one
    float32 ulp of 1 (KINK) of zero -- and the two formula seeds that were replaced are"""
    from torch.nn import functional as F
    seen, orig = [], F.leaky_relu

    def recording(x, *a, **kw):
        seen.append(float(x.detach().abs().min()))
        return orig(x, *a, **kw)
    monkeypatch.setattr(F, 'leaky_relu', recording)
    for c in H.CASES:
        if H.SHAPES[c[1]][4] != 'relu':
            continue
        runs = [(None, True)] + ([(T.make_case(H.tuple_of(c)), False)] if c in H.SEED_OF else [])
        for given, clear in runs:
            d = H.make_case(c) if given is None else dict(given, hp=H.make_case(c)['hp'])
            del seen[:]
            T.td3_literal(d, hp=d['hp'], steps0=H.make_case(c)['steps0'], moments0=H.state_of(H.make_case(c))['moments0'])
            assert len(seen) > 4 * d['n'] and (min(seen) > H.KINK) == clear, (H.case_id(c), min(seen))


@pytest.mark.parametrize('big', [False, True], ids=['B17', 'B129'])
@pytest.mark.parametrize('point', list(H.FLAVOUR_POINTS))
def test_flavour_points_meet_td3_64s_bounds(point, big):
    """the two points the other flavours are flown at (the reference's defaults; tau 1, gamma 0, noise_sd 0, lambdas apart on step counts
    of 40 000 / 20 000), at B = 17 and at B = 129: float32 torch is within td3_64's bounds of the float64 run, and both networks move"""
    d = H.make_flavour_case(point, big)
    kw = H.state_of(d)
    assert d['B'] == (129 if big else 17) and kw['steps0'] == H.FLAVOUR_POINTS[point][1] and kw['moments0'] is None
    ref = T.td3_literal(d, **kw)
    T.check(T.td3_literal(d, torch.float32, **kw), ref, d, 'flavours %s B %d' % (point, d['B']))
    ex = T.td3_explicit64(d, **kw)
    for k in T.ROWS + T.MOMENTS + ('td',):
        np.testing.assert_allclose(ex[k], ref[k], rtol=0, atol=1e-11, err_msg=k)


def test_bounds_are_td3_64s_unless_calibrated():
    """a point without an entry in BOUNDS is held to td3_64's bounds; an entry may only name grid points"""
    assert set(H.BOUNDS) <= set(H.POINTS)
    for c in H.CASES:
        act = H.SHAPES[c[1]][4]
        if c[0] not in H.BOUNDS:
            assert H.tol_of(c, act) == dict(rel=T.TOL_REL[act], mom=T.MOM_REL[act], fwd=T.FWD_TOL)


# the cases a mistake can show in: where the field it fixes, swaps or ignores differs from what the mistake puts in its place
APPLIES = {'gamma_fixed': ('gamma0', 'gamma1'), 'tau_fixed': ('tau0', 'tau1', 'ref_defaults'),
           'noise_fixed': ('noise_sd0', 'noise_clip0', 'noise_clip5', 'ref_defaults'), 'lambdas_swapped': ('lambdas_apart', 'lambda_t_negative'),
           'eps_sd_fixed': ('eps_sd0',), 'actor_clip_fixed': ('clip_active',), 'steps_restart': ('warm700', 'warm40000')}


@pytest.mark.parametrize('mistake', T.HP_MISTAKES)
def test_planted_mistakes_exceed_the_bound(mistake):
    """each planted mistake moves a row or a moment past the case's bound on at least one grid case where it applies; the first such
    case is named in the output.  (tau_fixed at tau 1, noise_fixed at noise_clip 5 and so on: every point is walked, one must catch.)"""
    seen = []
    for c in H.CASES:
        if c[0] not in APPLIES[mistake]:
            continue
        d, ref = _case(c)
        dev, moved = T.deviations(T.td3_explicit64(d, mistake, **H.state_of(d)), ref, d)
        tol = H.tol_of(c, d['act'])
        rows = max(dev[k] / (tol['rel'] + T.TOL_ABS / moved[k.split('_')[0]]) for k in T.ROWS)
        moms = max(dev[k] / tol['mom'] for k in T.MOMENTS)
        seen.append((round(float(rows), 2), round(float(moms), 2), H.case_id(c)))
        if rows > 1.0 or moms > 1.0:
            print('TD3_HP_MISTAKE %s caught on %s: rows %.3g x the bound, moments %.3g x' % (mistake, H.case_id(c), rows, moms))
            return
    pytest.fail('%s stays within the bound in every case: %s' % (mistake, seen))


@pytest.mark.parametrize('mistake', T.HP_MISTAKES)
def test_planted_mistakes_are_the_reference_at_the_defaults(mistake):
    """why these seven are not in td3_64.MISTAKES: on a cold start at td3_64's constants each of them computes the reference (the
    swapped lambdas apart: they differ at the defaults too, and are caught there as well)"""
    d = T.make_case(T.CASES[3])
    ref, ex = T.td3_literal(d), T.td3_explicit64(d, mistake)
    same = all(np.allclose(ex[k], ref[k], rtol=0, atol=1e-11) for k in T.ROWS + T.MOMENTS)
    assert same == (mistake != 'lambdas_swapped')

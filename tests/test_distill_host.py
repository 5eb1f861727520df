"""CPU tests of the float64 contract of serl_ga_distill (tests/distill64.py): what the reference's update step does on a minibatch the
Q-filter drops entirely, the calibration of the tolerance the GPU grid (tests/test_gpu_distill.py) applies, and that the tolerance
catches planted mistakes."""
import functools
import warnings
import numpy as np
import pytest
import torch
import distill64 as D


@functools.lru_cache(maxsize=None)
def _case(c):
    d = D.make_case(c)
    return d, D.distill64(d)


def test_empty_minibatch_takes_an_adam_step_with_zero_gradient():
    """GeneticAgent.update_parameters (genetic_agent.py:22-59, distill.update_parameters) in float32 on the reference's Actor, through a
    minibatch whose Q-filter keeps no state after six ordinary steps: the loss is NaN (torch.mean of nothing), backward leaves every
    .grad exactly 0, and Adam's step still advances its step count and applies the decayed first moment -- the weights move and stay
    finite.  The float64 reference (distill64) takes the same step, and the whole run agrees with it; skipping the step instead does not."""
    import actor_shapes as X
    from serl_amd import distill
    from serl_amd.actor import unpack_into
    S, A, act, B, n = 7, 3, 'tanh', 16, 48
    s = D.net(S, A, act)
    w = X.make_weights(s, 3, 4)
    P = D.param_count(S, A)
    rng = np.random.default_rng(4)
    states = rng.standard_normal((n, S)).astype(np.float32)
    states[:, S - 1] = (np.arange(n) >= B).astype(np.float32)          # rows 0 .. B-1: flag 0
    mods = []
    for k in range(3):
        with torch.random.fork_rng(devices=[]):
            m = X.actor_module(s)
        unpack_into(m, torch.from_numpy(w[k, :P]))
        mods.append(m)
    child, p1, p2 = mods
    for p in list(p1.parameters()) + list(p2.parameters()):
        p.requires_grad_(False)

    def critic(st, a):                 # equal Q for both parents on a flag-0 state (dropped), Q = sum(a) otherwise
        q = a.sum(-1, keepdim=True) * st[:, S - 1:S]
        return q, q
    with torch.no_grad():
        a1, a2 = p1(torch.from_numpy(states)), p2(torch.from_numpy(states))
    targets = torch.where((a1.sum(-1) > a2.sum(-1))[:, None], a1, a2).numpy()
    keep = states[:, S - 1].copy()
    empty_step = 6
    slots = np.zeros((10, 128), np.int32)
    for k in range(10):
        slots[k, :B] = rng.permutation(B) if k == empty_step else rng.choice(n, B, replace=False)
    assert all(0 < keep[slots[k, :B]].sum() < B for k in range(10) if k != empty_step)
    optim = torch.optim.Adam(child.parameters(), lr=D.LR)
    for k in range(10):
        before = [p.detach().clone() for p in child.parameters()]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)
            mse = distill.update_parameters(child, optim, (torch.from_numpy(states[slots[k, :B]]),), p1, p2, critic)
        if k == empty_step:
            assert torch.isnan(mse)
            for p, q in zip(child.parameters(), before):
                assert p.grad is not None and (p.grad == 0).all()
                assert torch.isfinite(p).all()
                st_ = optim.state[p]
                assert int(st_['step']) == empty_step + 1
                # the step of a zero gradient: m = beta1 m, v = beta2 v, w -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
                t = empty_step + 1
                want = q - D.LR / (1 - D.BETA1 ** t) * st_['exp_avg'] / (st_['exp_avg_sq'].sqrt() / np.sqrt(1 - D.BETA2 ** t) + D.EPS)
                torch.testing.assert_close(p.detach(), want, rtol=0, atol=1e-7)
            moved = max((p.detach() - q).abs().max().item() for p, q in zip(child.parameters(), before))
            assert moved > 1e-4, 'an all-dropped step moves the weights by the momentum'
        else:
            assert torch.isfinite(mse)
    got = torch.cat([p.detach().reshape(-1) for p in child.parameters()]).double().numpy()
    d = dict(s=s, row=w[0, :P], states=states, targets=targets, keep=keep, slots=slots, n_steps=10, B=B)
    assert D.n_empty_steps(d) == 1
    w64 = D.distill64(d)
    assert np.isfinite(w64).all()
    d6, d7 = dict(d, n_steps=empty_step), dict(d, n_steps=empty_step + 1)
    assert np.abs(D.distill64(d7) - D.distill64(d6)).max() > 1e-4
    moved = np.abs(w64 - w[0, :P]).max()
    assert moved > D.MIN_MOVED
    assert np.abs(got - w64).max() <= D.tolerance(act, moved)
    assert np.abs(D.distill_explicit64(d, 'skip_empty_step') - w64).max() > 10 * D.tolerance(act, moved)


def test_grid_covers_the_kernels_branches():
    """the grid holds every (S, A) of the env configurations and the ABI's edges, every activation on at least three of them, every
    minibatch size and keep mode; the 'mid' / 'first' cases have exactly one all-dropped step where they say, 'half' drops some rows of
    every step but not all"""
    pairs = {(S, A) for S, A, *_ in D.CASES}
    assert pairs >= {(7, 3), (10, 3), (2, 1), (3, 1), (13, 3), (16, 3), (1, 1), (16, 4)}
    for act in ('tanh', 'elu', 'relu'):
        assert len({(S, A) for S, A, a, *_ in D.CASES if a == act}) >= 3, act
    assert {B for *_, B, _ in D.CASES} >= {128, 127, 64, 3, 1}
    assert {k for *_, k in D.CASES} == {'all', 'half', 'mid', 'first'}
    for c in D.CASES:
        d = D.make_case(c)
        assert 24 <= d['n_steps'] <= 60
        B, keep, sl = d['B'], d['keep'], d['slots']
        assert (sl >= 0).all() and (sl < len(keep)).all()
        kept = np.array([keep[sl[k, :B]].sum() for k in range(d['n_steps'])])
        for k in range(d['n_steps']):
            assert len(set(sl[k, :B])) == B
        if c[4] == 'all':
            assert (kept == B).all(), c
        elif c[4] == 'half' and B > 1:
            assert ((kept > 0) & (kept < B)).all() and kept.mean() < 0.75 * B, c
        elif c[4] in ('mid', 'first'):
            at = 0 if c[4] == 'first' else d['n_steps'] // 2
            assert kept[at] == 0 and D.n_empty_steps(d) == 1 + int((kept[np.arange(len(kept)) != at] == 0).sum()), c
            assert (kept[np.arange(len(kept)) != at] > 0).all(), c


@pytest.mark.parametrize('c', D.CASES, ids=D.case_id)
def test_float32_loop_meets_the_bound(c):
    """the calibration, asserted: the literal loop in float32 torch stays within the bound of the float64 run on every case, every case
    trains (moved > MIN_MOVED), and the written-out float64 loop the planted mistakes go into is the literal one"""
    d, w64 = _case(c)
    moved = np.abs(w64 - d['row']).max()
    assert moved > D.MIN_MOVED, moved
    err = np.abs(D.distill32(d) - w64).max()
    assert err <= D.tolerance(c[2], moved), '%s: |w32 - w64| = %.3g > %.3g (moved %.3g)' % (D.case_id(c), err, D.tolerance(c[2], moved), moved)
    np.testing.assert_allclose(D.distill_explicit64(d), w64, rtol=0, atol=1e-12)


@pytest.mark.parametrize('mistake', D.MISTAKES)
def test_planted_mistakes_exceed_the_bound(mistake):
    """each planted mistake moves the trained parameters past the bound in at least one grid case (cases of the activation the mistake
    lives in only)"""
    only = {'leaky_slope_0.02': 'relu', 'elu_grad_expm1': 'elu'}.get(mistake)
    seen = []
    for c in D.CASES:
        if only and c[2] != only:
            continue
        d, w64 = _case(c)
        moved = np.abs(w64 - d['row']).max()
        ratio = np.abs(D.distill_explicit64(d, mistake) - w64).max() / D.tolerance(c[2], moved)
        seen.append((round(ratio, 2), D.case_id(c)))
        if ratio > 1.0:
            return
    pytest.fail('%s stays within the bound in every case: %s' % (mistake, seen))

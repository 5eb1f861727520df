"""CPU tests of what serl_ga_distill_general is held to (tests/distill64_shapes.py) and of the host side of the choice between the two
distillation kernels: the calibration of the grid's tolerance, that the tolerance catches the planted mistakes at the new shapes, the
shapes serl_ga_distill_general_work_bytes accepts, and that distil_batch's new arguments are checked before any draw and leave the
default path's draws where they were."""
import functools
import random
import numpy as np
import pytest
import torch
import distill64 as D
import distill64_shapes as G


@functools.lru_cache(maxsize=None)
def _case(c):
    d = G.make_case(c)
    return d, D.distill64(d)


def test_grid_covers_every_axis_at_every_shape():
    """every (S, A), minibatch size, keep mode and activation meets every (H, L); 24 .. 60 steps; the 'mid' / 'first' cases have their
    all-dropped step where they say"""
    assert 24 <= len(G.CASES) <= 60
    for H, L in G.SHAPES:
        mine = [c for c in G.CASES if c[:2] == (H, L)]
        assert {c[2:4] for c in mine} == set(G.DIMS), (H, L)
        assert {c[4] for c in mine} == set(G.ACTS), (H, L)
        assert {c[5] for c in mine} == set(G.BATCHES), (H, L)
        assert {c[6] for c in mine} == set(G.KEEPS), (H, L)
    for c in G.CASES:
        d = G.make_case(c)
        assert len(d['row']) == G.param_count(*c[:4])
        assert 24 <= d['n_steps'] <= 60
        B, keep, sl = d['B'], d['keep'], d['slots']
        assert (sl >= 0).all() and (sl < len(keep)).all()
        kept = np.array([keep[sl[k, :B]].sum() for k in range(d['n_steps'])])
        if c[6] == 'all':
            assert (kept == B).all(), c
        elif c[6] in ('mid', 'first'):
            at = 0 if c[6] == 'first' else d['n_steps'] // 2
            assert kept[at] == 0 and (kept[np.arange(len(kept)) != at] > 0).all(), c


@pytest.mark.parametrize('c', G.CASES, ids=G.case_id)
def test_float32_loop_meets_the_bound(c):
    """the calibration, asserted: the float64 run alone moves the parameters of every case by more than MIN_MOVED, and the literal loop
    in float32 torch stays within the bound of it"""
    d, w64 = _case(c)
    moved = np.abs(w64 - d['row']).max()
    assert moved > G.MIN_MOVED, moved
    err = np.abs(D.distill32(d) - w64).max()
    tol = G.tolerance(c[4], moved)
    print('DISTILL_CAL %-34s |w32 - w64| %.3g  moved %.4f  ratio %.3g  bound %.3g' % (G.case_id(c), err, moved, err / moved, tol))
    assert err <= tol, '%s: |w32 - w64| = %.3g > %.3g (moved %.3g)' % (G.case_id(c), err, tol, moved)


@pytest.mark.parametrize('shape', [(72, 3), (128, 4)], ids=lambda s: 'H%dL%d' % s)
@pytest.mark.parametrize('mistake', D.MISTAKES)
def test_planted_mistakes_exceed_the_bound(mistake, shape):
    """each planted mistake of distill64.distill_explicit64 (which reads the shape from the case) moves the trained parameters past the
    bound in at least one of the shape's grid cases (cases of the activation the mistake lives in only); without a mistake the
    written-out loop is the literal one"""
    only = {'leaky_slope_0.02': 'relu', 'elu_grad_expm1': 'elu'}.get(mistake)
    seen = []
    for c in G.CASES:
        if c[:2] != shape or (only and c[4] != only):
            continue
        d, w64 = _case(c)
        np.testing.assert_allclose(D.distill_explicit64(d), w64, rtol=0, atol=1e-12)
        moved = np.abs(w64 - d['row']).max()
        ratio = np.abs(D.distill_explicit64(d, mistake) - w64).max() / G.tolerance(c[4], moved)
        seen.append((round(ratio, 2), G.case_id(c)))
    assert seen and max(seen)[0] > 1.0, '%s stays within the bound in every case of %s: %s' % (mistake, shape, seen)


def test_work_bytes_accepts_the_learners_actor_shapes():
    """serl_ga_distill_general_work_bytes: the size for every shape of the grid and the learner's edges (gradients, two moments, the
    gathered states and the tape per pair), 0 for what the kernel refuses"""
    from serl_amd import _capi
    wb = _capi.lib().serl_ga_distill_general_work_bytes
    for H, L, S, A in sorted({c[:4] for c in G.CASES} | {(4, 0, 1, 1), (128, 4, 16, 4), (32, 3, 7, 3), (8, 0, 16, 1)}):
        P4 = (G.param_count(H, L, S, A) + 3) // 4 * 4
        per = 4 * (3 * P4 + 128 * S + 128 * (2 * (L + 2) * H + (L + 2)))
        assert wb(1, S, A, H, L) == per, (H, L, S, A)
        assert wb(15, S, A, H, L) == 15 * per, (H, L, S, A)
        # the learner takes the same actor (serl_td3_work_bytes is its predicate)
        assert _capi.lib().serl_td3_work_bytes(1, S, A, H, L, 128) > 0
    for H, L, S, A in ((2, 3, 7, 3), (130, 3, 7, 3), (34, 3, 7, 3), (0, 3, 7, 3), (132, 1, 7, 3), (72, 5, 7, 3), (72, -1, 7, 3), (72, 3, 0, 3),
                       (72, 3, 17, 3), (72, 3, 7, 0), (72, 3, 7, 5)):
        assert wb(1, S, A, H, L) <= 0, (H, L, S, A)
        assert _capi.lib().serl_td3_work_bytes(1, S, A, H, L, 128) <= 0
    assert wb(0, 7, 3, 72, 3) <= 0 and wb(-1, 7, 3, 72, 3) <= 0


def test_distil_batch_checks_kernel_and_dense_before_any_draw(golden):
    """an unknown kernel or dense, dense='mfma' with 'serl50' -> ValueError; kernel='general' where the kernel cannot run (no GPU
    here) -> RuntimeError, never PyTorch; python's and torch's generators are where they were"""
    from serl_amd import distill
    from test_ga_host import distill_case
    args, spec, w, bufs, critic, seed, _ = distill_case(golden, 'd_18_0', torch.device('cpu'))
    random.seed(seed); torch.manual_seed(seed)
    st, tst = random.getstate(), torch.get_rng_state()
    for kw, exc in ((dict(kernel='serl'), ValueError), (dict(kernel=None), ValueError), (dict(dense='mma'), ValueError),
                    (dict(kernel='general', dense='f32'), ValueError), (dict(dense='mfma'), ValueError),
                    (dict(kernel='serl50', dense='mfma'), ValueError), (dict(kernel='general'), RuntimeError),
                    (dict(kernel='general', dense='mfma'), RuntimeError)):
        info = {}
        with pytest.raises(exc):
            distill.distil_batch(args, None, spec, w, [(0, 1)], bufs, critic, info=info, **kw)
        assert random.getstate() == st and torch.equal(torch.get_rng_state(), tst), kw
        assert info == {}, kw


def test_serl50_and_auto_on_the_cpu_draw_what_the_pairwise_loop_draws(golden):
    """kernel='serl50' (given or by default) and 'auto' without a GPU train pair by pair in PyTorch: the children's bits and both
    generators' positions are those of distilation_crossover called pair by pair, as before the argument existed"""
    from serl_amd import distill
    from test_ga_host import distill_case
    args, spec, w, bufs, critic, seed, _ = distill_case(golden, 'd_18_0', torch.device('cpu'))
    args.individual_bs = 300           # (two Adam steps per pass: the test is about draws)
    pairs = [(0, 1), (1, 0)]
    random.seed(seed); torch.manual_seed(seed)
    want = [distill.distilation_crossover(args, None, spec, w, f, s, bufs, critic) for f, s in pairs]
    after, tafter = random.getstate(), torch.get_rng_state()
    for kw in (dict(), dict(kernel='serl50'), dict(kernel='serl50', dense='valu'), dict(kernel='auto'), dict(kernel='auto', dense='mfma')):
        info = {}
        random.seed(seed); torch.manual_seed(seed)
        got = distill.distil_batch(args, None, spec, w, pairs, bufs, critic, info=info, **kw)
        assert random.getstate() == after and torch.equal(torch.get_rng_state(), tafter), kw
        assert info == {'path': 'torch'}, kw
        for (row, buf, crit), (row2, buf2, _) in zip(got, want):
            assert torch.equal(row, row2) and len(crit) == 0, kw
            assert torch.equal(buf.rows[:len(buf)], buf2.rows[:len(buf2)]), kw


def test_ssne_passes_the_choice_through():
    """SSNE keeps distil_kernel / distil_dense and hands them to distil_batch with an info dict, whose path it keeps"""
    import types
    from serl_amd import distill, ssne
    args = types.SimpleNamespace(pop_size=4, elite_fraction=0.25)
    assert ssne.SSNE(args, None, None).distil_kernel == 'serl50' and ssne.SSNE(args, None, None).distil_dense == 'valu'
    s = ssne.SSNE(args, None, None, critic='q', distil_kernel='general', distil_dense='mfma')
    assert s.last_distil_path is None
    seen = {}

    def fake(a, engine, spec, weights, pairs, buffers, critic, rng=random, kernel='serl50', dense='valu', info=None):
        seen.update(kernel=kernel, dense=dense, critic=critic, pairs=pairs)
        info['path'] = 'fused-general-mfma'
        return ['child']
    old, distill.distil_batch = distill.distil_batch, fake
    try:
        assert s.distilation_crossovers('w', [(1, 2)], 'b') == ['child']
    finally:
        distill.distil_batch = old
    assert seen == dict(kernel='general', dense='mfma', critic='q', pairs=[(1, 2)])
    assert s.last_distil_path == 'fused-general-mfma'

"""CPU tests of what tests/test_gpu_distill_general_edges.py holds serl_ga_distill_general to (tests/distill_general_edges.py): the grids
cover what they say, every case trains (MIN_MOVED) and the literal loop in float32 torch meets its bound, inputs the contract calls
equivalent give identical float64 runs, an all-dropped table leaves the row bit for bit as it was, and each planted mistake of the
contract on raw inputs is noticed by the case named for it."""
import numpy as np
import pytest
import distill64 as D
import distill64_shapes as G
import distill_general_edges as E


def _moved_and_f32(d, lr=D.LR):
    w64 = D.distill64(d, lr)
    moved = np.abs(w64 - d['row']).max()
    return w64, moved, np.abs(D.distill32(d, lr) - w64).max()


def test_no_hidden_layer_grid_covers_every_axis():
    """nine cases: every L = 0 shape with every minibatch size, and every (S, A), activation and keep mode at least once (each
    activation at every shape); actor_shapes builds and runs such actors (make_weights, forward64: the row has the L = 0 count)"""
    assert len(E.L0_CASES) == 9 and {c[:2] for c in E.L0_CASES} == set(E.L0_SHAPES) == {(4, 0), (72, 0), (128, 0)}
    for H, L in E.L0_SHAPES:
        mine = [c for c in E.L0_CASES if c[:2] == (H, L)]
        assert {c[5] for c in mine} == {1, 127, 128} and {c[4] for c in mine} == set(G.ACTS) and {c[2:4] for c in mine} == set(G.DIMS)
    assert {c[6] for c in E.L0_CASES} == set(G.KEEPS)


@pytest.mark.parametrize('c', E.L0_CASES, ids=G.case_id)
def test_no_hidden_layer_float32_loop_meets_the_bound(c):
    """A: the float64 run moves every L = 0 case by more than MIN_MOVED, the float32 loop stays within the grid's bound of it, and the
    written-out loop of distill64 is the literal one without LayerNorm layers too"""
    d = G.make_case(c)
    assert len(d['row']) == G.param_count(*c[:4]) == c[0] * c[2] + c[0] + c[3] * c[0] + c[3]
    w64, moved, err = _moved_and_f32(d)
    assert moved > G.MIN_MOVED
    print('EDGE_CAL %-34s |w32 - w64| %.3g  moved %.4f  ratio %.3g' % (G.case_id(c), err, moved, err / moved))
    assert err <= G.tolerance(c[4], moved)
    np.testing.assert_allclose(D.distill_explicit64(d), w64, rtol=0, atol=1e-12)


@pytest.mark.parametrize('c', E.E_CASES, ids=E.e_id)
def test_learning_rate_and_step_cases_float32_loop_meets_half_the_bound(c):
    """E: every case moves by more than MIN_MOVED (lr 1e-4 x 60 steps: 6e-3) and the float32 loop stays under HALF of the grid's bound,
    which is why the bound is used as it is"""
    d = E.e_case(c)
    assert d['n_steps'] == c[2] and d['B'] == 64 and len(d['keep']) == 300
    w64, moved, err = _moved_and_f32(d, c[1])
    assert moved > G.MIN_MOVED, moved
    print('EDGE_CAL %-34s |w32 - w64| %.3g  moved %.4f  ratio %.3g' % (E.e_id(c), err, moved, err / moved))
    assert err / moved < 0.5 * G.TOL_REL[c[0]]
    assert E.e_tolerance(c, moved) == G.tolerance(c[0], moved)


def test_the_other_cases_train_and_their_float32_loop_meets_the_bound():
    """B6, C, C4 and D: the pairs that are checked against float64 only or launched alone: MIN_MOVED and the float32 loop"""
    pairs = [('B6', E.contract_case(E.repeats_case('tanh'))), ('C4', E.contract_case(E.one_row_case('elu')))]
    pairs += [('C H36 %d' % k, d) for k, d in enumerate(E.layout_cases(E.SHAPE_B))] + [('D %d' % k, d) for k, d in enumerate(E.many_cases())]
    for what, d in pairs:
        _, moved, err = _moved_and_f32(d)
        assert moved > G.MIN_MOVED, what
        assert err <= G.tolerance(d['s']['activation'], moved), what
    six = E.many_cases()
    assert len({d['row'].tobytes() + d['slots'].tobytes() for d in six}) == 6 and all(d['n_steps'] == 8 and d['B'] == 3 for d in six)


def test_equivalent_inputs_give_identical_float64_runs():
    """B, restated on the CPU: the contract's pair of a raw pair is the pair clamped / mapped on the host, and the literal float64 loop --
    which reads keep as it is -- gives the same parameters for the raw mask and for its flags; batch above 128 is 128, n_steps past
    the table is the table, below zero is no step"""
    d = E.slots_case('tanh')
    np.testing.assert_array_equal(E.contract_case(d)['slots'], E.clamped(d)['slots'])
    used = d['slots'][:, :d['B']]
    assert {int(v) for v in E.OUT_OF_RANGE(300)} <= set(used.ravel().tolist())
    assert (d['keep'][[0, 299]] == 1).all() and not np.array_equal(d['states'][0], d['states'][299])
    k = E.keep_case('elu')
    np.testing.assert_array_equal(E.contract_case(k)['keep'], E.keep_as_flags(k)['keep'])
    tiny = k['keep'] == np.float32(1e-45)
    assert tiny.any() and (k['keep'][tiny] > 0).all() and (k['keep'][tiny] < np.finfo(np.float32).tiny).all()
    assert E.keep_as_flags(k)['keep'][tiny].all() and not E.keep_as_flags(k)['keep'][np.signbit(k['keep']) & (k['keep'] == 0)].any()
    np.testing.assert_array_equal(D.distill64(k), D.distill64(E.keep_as_flags(k)))
    b = E.batch_case('elu')
    for raw in E.BATCH_TOO_LARGE:
        c = E.contract_case(b, batch=raw)
        assert c['B'] == 128 and c['n_steps'] == 24
    for raw in E.BATCH_NONE:
        assert E.contract_case(b, batch=raw)['B'] == 0
    s = E.steps_case('tanh')
    assert [E.contract_case(s, n_steps=n)['n_steps'] for n in (25, E.I32_MAX, -1, E.I32_MIN, 0)] == [24, 24, 0, 0, 0]
    np.testing.assert_array_equal(E.contract64(s, n_steps=-1), s['row'].astype(np.float64))


@pytest.mark.parametrize('act', E.ACTS)
def test_all_dropped_table_leaves_the_row_as_it_was(act):
    """B3: Adam steps with zero gradients from zero moments are updates of 0 / (0 + eps): the float64 loop returns the f32 row bit for
    bit, in the literal loop (whose loss is NaN there) and in the written-out one with batch = 0"""
    d = E.batch_case(act)
    np.testing.assert_array_equal(D.distill64(dict(d, keep=np.zeros_like(d['keep']))), d['row'].astype(np.float64))
    for raw in E.BATCH_NONE:
        np.testing.assert_array_equal(E.contract64(d, batch=raw), d['row'].astype(np.float64))


@pytest.mark.parametrize('mistake', E.MISTAKES)
def test_planted_mistakes_are_noticed_by_their_named_case(mistake):
    """G: the case of B or C named for the mistake is an equality between two launches, so the mistaken contract must differ from the
    contract at all -- it does at every activation -- and the one of the two that is checked against float64 catches it as well: the
    difference exceeds the bound at tanh and ELU (at LeakyReLU, whose bound is 84 x wider, for five of the seven)"""
    what, build, batch, n_steps = E.NAMED[mistake]
    seen = {}
    for act in E.ACTS:
        d = build(act)
        ref = E.contract64(d, batch, n_steps)
        if batch is None and n_steps is None:
            np.testing.assert_allclose(ref, D.distill64(E.contract_case(d)), rtol=0, atol=1e-12)
        bad = E.contract64(d, batch, n_steps, mistake)
        diff = np.abs(bad - ref).max()
        moved = np.abs(ref - d['row']).max()
        assert moved > G.MIN_MOVED
        seen[act] = diff / G.tolerance(act, moved)
        assert diff > 0, (mistake, what, act)
    print('EDGE_MISTAKE %-22s %s  difference / bound %s' % (mistake, what, {a: round(float(r), 2) for a, r in seen.items()}))
    assert seen['tanh'] > 1 and seen['elu'] > 1, seen
    if mistake not in ('batch_unclamped_high', 'steps_unclamped'):
        assert seen['relu'] > 1, seen

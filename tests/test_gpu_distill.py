"""serl_ga_distill -- all Adam steps of an epoch's distillation crossovers in one launch -- against the float64 contract of
tests/distill64.py across the shapes the kernel accepts (S 1 .. 16, A 1 .. 4, tanh / ELU / LeakyReLU, minibatches of 1 .. 128 rows,
partial and empty Q-filter masks, several pairs of different lengths in one launch), its refusals, and distil_batch with the non-tanh
actors the device replay ring reaches."""
import ctypes
import random
import numpy as np
import pytest
import torch
import distill64 as D

pytestmark = pytest.mark.gpu


def _call(engine, child_ptr, stride, n_pairs, S, A, act_id, states, targets, keep, slots, n_steps, batch, H=32, L=3):
    """serl_ga_distill on device tensors (as distill.distil_batch calls it) -> status code; synchronised"""
    from serl_amd import _capi
    stream = torch.cuda.current_stream(engine.device).cuda_stream
    rc = _capi.lib().serl_ga_distill(engine.ctx, child_ptr, stride, n_pairs, S, H, L, A, act_id, states.data_ptr(), targets.data_ptr(),
                                     keep.data_ptr(), states.shape[1], slots.data_ptr(), slots.shape[1], n_steps.data_ptr(),
                                     batch.data_ptr(), ctypes.c_float(D.LR), ctypes.c_void_p(stream))
    torch.cuda.synchronize()
    return rc


def _launch(engine, cases, n_steps=None, extra_rows=1, extra_steps=0, extra_cols=0, batch=None, n_steps_arg=None, unused_slot=None):
    """one launch for the pairs `cases` (make_case dicts of one shape) -> (child [K + 2, stride] after the launch, the same before).
    The launch covers rows 1 .. K of the child tensor; stride = the row's floats rounded up to 4 plus extra_cols.  Buffers are padded to
    the longest pair plus extra_rows rows of NaN, minibatch tables to the most steps plus extra_steps; every unused slot (columns from B
    on, steps beyond a pair's n_steps) names a NaN row: a kernel that read one would return NaN.
    For tests/test_gpu_distill_general_edges.py (the defaults are the above): batch, n_steps_arg -- what the kernel is handed per pair
    in place of the pairs' B and of n_steps (the tables are still filled by those); unused_slot -- the value of every unused table
    entry, and then neither it nor what the pairs' own tables hold needs to name a row."""
    from serl_amd.actor import ACTIVATION_IDS
    s = cases[0]['s']
    S, A, P = s['state_dim'], s['action_dim'], len(cases[0]['row'])
    K = len(cases)
    n_steps = [d['n_steps'] for d in cases] if n_steps is None else n_steps
    rows = max(len(d['keep']) for d in cases) + extra_rows
    steps = max(max(n_steps), 1) + extra_steps
    stride = (P + 3) // 4 * 4 + extra_cols
    st = np.full((K, rows, S), np.nan, np.float32)
    tg = np.full((K, rows, A), np.nan, np.float32)
    kp = np.ones((K, rows), np.float32)
    sl = np.full((K, steps, 128), rows - 1 if unused_slot is None else unused_slot, np.int32)
    child = np.full((K + 2, stride), 7.25, np.float32)
    for k, d in enumerate(cases):
        n = len(d['keep'])
        st[k, :n], tg[k, :n], kp[k, :n] = d['states'], d['targets'], d['keep']
        sl[k, :n_steps[k], :d['B']] = d['slots'][:n_steps[k], :d['B']]
        child[1 + k, :P] = d['row']
    assert unused_slot is not None or ((sl >= 0).all() and (sl < rows).all())
    dev = engine.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ch = t(child)
    rc = _call(engine, ch[1].data_ptr(), stride, K, S, A, ACTIVATION_IDS[s['activation']], t(st), t(tg), t(kp), t(sl),
               t(np.array(n_steps if n_steps_arg is None else n_steps_arg, np.int32)),
               t(np.array([d['B'] for d in cases] if batch is None else batch, np.int32)))
    assert rc == 0, rc
    return ch.cpu().numpy(), child


def _check(got, d, what):
    """one pair: the kernel's child against its float64 run; -> max |w - w64| / moved"""
    w64 = D.distill64(d)
    moved = np.abs(w64 - d['row']).max()
    assert moved > D.MIN_MOVED, what
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - w64).max()
    tol = D.tolerance(d['s']['activation'], moved)
    print('DISTILL_DEV %-26s act %-4s |w - w64| %.3g  moved %.4f  ratio %.3g  bound %.3g' % (what, d['s']['activation'], err, moved, err / moved, tol))
    assert err <= tol, '%s: |w - w64| = %.3g > %.3g (moved %.3g), worst at parameter %d' % (
        what, err, tol, moved, int(np.argmax(np.abs(got - w64))))
    return err / moved


@pytest.mark.parametrize('c', D.CASES, ids=D.case_id)
def test_distill_kernel_vs_float64(engine, c):
    """one pair per case of the grid, every step of its minibatch table"""
    d = D.make_case(c)
    P = len(d['row'])
    out, before = _launch(engine, [d])
    _check(out[1, :P], d, D.case_id(c))
    np.testing.assert_array_equal(out[1, P:], before[1, P:])
    np.testing.assert_array_equal(out[[0, 2]], before[[0, 2]])


@pytest.mark.parametrize('S,A,act', [(10, 3, 'elu'), (16, 4, 'relu'), (2, 1, 'tanh')])
def test_distill_kernel_several_pairs_in_one_launch(engine, S, A, act):
    """five pairs of one shape in one launch: different minibatch sizes and keep masks, a pair of n_steps = 0 between longer ones
    (bit for bit unchanged), buffers padded to the longest, a row stride larger than the row; columns past the row and rows outside
    the launch untouched"""
    kinds = [(128, 'half'), (3, 'mid'), (64, 'all'), (1, 'first'), (127, 'half')]
    cases = [D.make_case((S, A, act, B, keep), seed=11 * S + 5 * A + k) for k, (B, keep) in enumerate(kinds)]
    n_steps = [d['n_steps'] for d in cases]
    n_steps[2] = 0
    P = len(cases[0]['row'])
    out, before = _launch(engine, cases, n_steps=n_steps, extra_rows=5, extra_steps=3, extra_cols=12)
    for k, d in enumerate(cases):
        what = 'S%dA%d_%s pair %d (B %d, %d steps)' % (S, A, act, k, d['B'], n_steps[k])
        if n_steps[k] == 0:
            np.testing.assert_array_equal(out[1 + k], before[1 + k], err_msg=what)
        else:
            _check(out[1 + k, :P], d, what)
    np.testing.assert_array_equal(out[:, P:], before[:, P:])
    np.testing.assert_array_equal(out[[0, len(cases) + 1]], before[[0, len(cases) + 1]])


def test_distill_kernel_refusals_and_probe(engine):
    """shapes outside the kernel's (H != 32, L != 3, S outside 1 .. 16, A outside 1 .. 4, an unknown activation) are refused with
    SERL_E_UNSUPPORTED and the weights stay untouched; every (S, A) of the grid passes distil_batch's n_pairs = 0 probe, the largest
    (S 16, A 4: 162 880 B of training state) included"""
    from serl_amd import _capi
    dev = engine.device
    big = 64 * 17 + 64 + 3 * (64 * 64 + 3 * 64) + 5 * 64 + 5          # buffers sized for the largest shape asked for below
    child = torch.full((1, big + 3), 0.5, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    st = torch.from_numpy(rng.standard_normal((1, 8, 17)).astype(np.float32)).to(dev)
    tg = torch.zeros(1, 8, 5, device=dev)
    kp = torch.ones(1, 8, device=dev)
    sl = torch.zeros(1, 1, 128, dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    for H, L, S, A, act in ((64, 3, 7, 3, 0), (16, 3, 7, 3, 0), (32, 2, 7, 3, 0), (32, 4, 7, 3, 1), (32, 3, 0, 3, 0), (32, 3, 17, 3, 0),
                            (32, 3, 7, 0, 0), (32, 3, 7, 5, 2), (32, 3, 7, 3, 3), (32, 3, 7, 3, -1)):
        rc = _call(engine, child.data_ptr(), child.shape[1], 1, S, A, act, st, tg, kp, sl, one, one, H=H, L=L)
        assert rc == _capi.E_UNSUPPORTED, (H, L, S, A, act, rc)
        assert (child == 0.5).all(), (H, L, S, A, act)
    for S, A in sorted({(c[0], c[1]) for c in D.CASES}):
        for act in (0, 1, 2):
            rc = _call(engine, child.data_ptr(), child.shape[1], 0, S, A, act, st, tg, kp, sl, one, one)
            assert rc == 0, (S, A, act, rc)
    assert (child == 0.5).all()


@pytest.mark.parametrize('act', ['elu', 'relu'])
def test_distil_batch_with_non_tanh_actors(engine, golden, monkeypatch, act):
    """distill.distil_batch with ELU / LeakyReLU SERL50-shaped actors (S 7, A 3: the layout the device replay ring stores) on
    reference-filled rings: the fused path is taken (the PyTorch path raises), and four pairs -- one of them with a child buffer of
    100 rows (a minibatch of 100, one step per epoch pass) -- agree with the same pairs trained one by one in PyTorch from the same
    seeds, python's generator left at the same place.  Both are f32 runs within the bound of the float64 one: 2 x the bound apart."""
    import actor_shapes as X
    import serl_amd
    from serl_amd import distill, replay
    from test_ga_host import distill_case
    args, _, _, _, critic, _, _ = distill_case(golden, 'd_18_0', engine.device, engine)
    spec = serl_amd.NetSpec(7, 3, 32, 3, act)
    w = torch.from_numpy(X.make_weights(D.net(7, 3, act), 4, 31)).to(engine.device)
    P = spec.param_count
    Pg = golden('proximal')
    bufs = []
    for i, n in zip((18, 0, 7, 33), (1002, 852, 60, 40)):
        r = replay.DeviceReplay(10_000, engine.device, engine)
        r.append_rows(torch.from_numpy(Pg['buf_serl50_%d' % i][:n]))
        bufs.append(r)
    args.individual_bs = 600
    pairs = [(0, 1), (2, 3), (1, 2), (3, 0)]

    def unfused(*a, **k):
        raise AssertionError('distil_batch left the fused path')
    with monkeypatch.context() as mp:
        mp.setattr(distill, 'distilation_crossover', unfused)
        random.seed(13); torch.manual_seed(13)
        kids = distill.distil_batch(args, engine, spec, w, pairs, bufs, critic)
        torch.cuda.synchronize()
        after = random.random()
    random.seed(13); torch.manual_seed(13)
    ref = [distill.distilation_crossover(args, engine, spec, w, f, s, bufs, critic) for f, s in pairs]
    assert random.random() == after
    sizes = []
    for (row, buf, _), (row2, buf2, _), (f, s) in zip(kids, ref, pairs):
        sizes.append(len(buf))
        assert len(buf) == len(buf2) == min(300, len(bufs[f])) + min(300, len(bufs[s]))
        np.testing.assert_array_equal(buf.rows[:len(buf)].cpu().numpy(), buf2.rows[:len(buf2)].cpu().numpy())
        a, b = row.cpu().numpy()[:P].astype(np.float64), row2.cpu().numpy()[:P].astype(np.float64)
        moved = np.abs(b - w[s].cpu().numpy()[:P]).max()
        assert moved > D.MIN_MOVED
        err = np.abs(a - b).max()
        print('DISTILL_BATCH %s pair %s buffer %d |fused - torch| %.3g moved %.4f ratio %.3g' % (act, (f, s), len(buf), err, moved, err / moved))
        assert err <= 2 * D.tolerance(act, moved), (act, f, s, err, moved)
    assert min(sizes) < 128

"""serl_ga_distill_general -- the distillation crossover's Adam steps for every actor shape the TD3 learner takes, one launch per epoch
-- against the float64 contract of tests/distill64.py on the grid of tests/distill64_shapes.py: one pair per case with the padding
invariants of tests/test_gpu_distill.py, several pairs of different lengths in one launch, the matrix-core flavour bit for bit against
the VALU one, refusals and the probe, the overlap with serl_ga_distill at hidden 32 x 3, and the host paths that choose the kernel
(distill.distil_batch(kernel='general'), SSNE(distil_kernel='general'))."""
import ctypes
import random
import types
import numpy as np
import pytest
import torch
import distill64 as D
import distill64_shapes as G

pytestmark = pytest.mark.gpu


def _call(engine, child_ptr, stride, n_pairs, H, L, S, A, act_id, states, targets, keep, slots, n_steps, batch, dense=0, work='sized', lr=D.LR):
    """serl_ga_distill_general on device tensors (as distill.distil_batch calls it) -> status code; synchronised.  work='sized': a
    workspace of serl_ga_distill_general_work_bytes, or none where that is 0 (a refused shape, the probe); work = a float32 device
    tensor: the caller's workspace, all of it and no more (tests/test_gpu_distill_general_edges.py)."""
    from serl_amd import _capi
    stream = torch.cuda.current_stream(engine.device).cuda_stream
    if isinstance(work, torch.Tensor):
        assert work.dtype == torch.float32 and work.is_contiguous()
        wk, nbytes = work, 4 * work.numel()
    else:
        nbytes = int(_capi.lib().serl_ga_distill_general_work_bytes(n_pairs, S, A, H, L))
        wk = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=engine.device) if nbytes > 0 else None
    rc = _capi.lib().serl_ga_distill_general(engine.ctx, child_ptr, stride, n_pairs, S, H, L, A, act_id, states.data_ptr(), targets.data_ptr(),
                                             keep.data_ptr(), states.shape[1], slots.data_ptr(), slots.shape[1], n_steps.data_ptr(),
                                             batch.data_ptr(), ctypes.c_float(lr), wk.data_ptr() if wk is not None else None,
                                             max(nbytes, 0), dense, ctypes.c_void_p(stream))
    torch.cuda.synchronize()
    return rc


def _launch(engine, cases, dense=0, n_steps=None, extra_rows=1, extra_steps=0, extra_cols=0, batch=None, n_steps_arg=None, lr=D.LR,
            stride=None, work='sized', child_offset=0, unused_slot=None):
    """tests/test_gpu_distill.py::_launch for the general kernel: one launch for the pairs `cases` (make_case dicts of one shape) ->
    (child [K + 2, stride] after the launch, the same before).  The launch covers rows 1 .. K; buffers are padded with rows of NaN,
    and every unused slot (columns from B on, steps beyond a pair's n_steps) names a NaN row: a kernel that read one would return NaN.
    For tests/test_gpu_distill_general_edges.py (the defaults are the above): batch, n_steps_arg -- what the kernel is handed per pair
    in place of the pairs' B and of n_steps (the tables are still filled by those); lr; stride -- the row stride in floats, whatever
    its remainder by 4; work -- _call's; child_offset -- the child tensor starts that many floats into its allocation (they are checked
    to stay as they were); unused_slot -- the value of every unused table entry, and then neither it nor what the pairs' own tables
    hold needs to name a row (with extra_rows = 0 there is no NaN row either)."""
    from serl_amd.actor import ACTIVATION_IDS
    s = cases[0]['s']
    S, A, H, L, P = s['state_dim'], s['action_dim'], s['hidden'], s['num_layers'], len(cases[0]['row'])
    K = len(cases)
    n_steps = [d['n_steps'] for d in cases] if n_steps is None else n_steps
    rows = max(len(d['keep']) for d in cases) + extra_rows
    steps = max(max(n_steps), 1) + extra_steps
    stride = (P + 3) // 4 * 4 + extra_cols if stride is None else stride
    st = np.full((K, rows, S), np.nan, np.float32)
    tg = np.full((K, rows, A), np.nan, np.float32)
    kp = np.ones((K, rows), np.float32)
    sl = np.full((K, steps, 128), rows - 1 if unused_slot is None else unused_slot, np.int32)
    flat = np.full(child_offset + (K + 2) * stride, 7.25, np.float32)
    child = flat[child_offset:].reshape(K + 2, stride)
    for k, d in enumerate(cases):
        n = len(d['keep'])
        st[k, :n], tg[k, :n], kp[k, :n] = d['states'], d['targets'], d['keep']
        sl[k, :n_steps[k], :d['B']] = d['slots'][:n_steps[k], :d['B']]
        child[1 + k, :P] = d['row']
    assert unused_slot is not None or ((sl >= 0).all() and (sl < rows).all())
    dev = engine.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fl = t(flat)
    ch = fl[child_offset:].view(K + 2, stride)
    rc = _call(engine, ch[1].data_ptr(), stride, K, H, L, S, A, ACTIVATION_IDS[s['activation']], t(st), t(tg), t(kp), t(sl),
               t(np.array(n_steps if n_steps_arg is None else n_steps_arg, np.int32)),
               t(np.array([d['B'] for d in cases] if batch is None else batch, np.int32)), dense, work, lr)
    assert rc == 0, rc
    assert (fl[:child_offset] == 7.25).all()
    return ch.cpu().numpy(), child.copy()


_REF, _RUN = {}, {}


def _ref(c, seed=None):
    """the case and its float64 run, computed once"""
    if (c, seed) not in _REF:
        d = G.make_case(c, seed)
        _REF[c, seed] = d, D.distill64(d)
    return _REF[c, seed]


def _run(engine, c, dense):
    """one pair, the grid case c, launched once per flavour"""
    if (c, dense) not in _RUN:
        _RUN[c, dense] = _launch(engine, [_ref(c)[0]], dense)
    return _RUN[c, dense]


def _check(got, d, w64, what):
    """one pair: the kernel's child against its float64 run; -> max |w - w64| / moved"""
    moved = np.abs(w64 - d['row']).max()
    assert moved > G.MIN_MOVED, what
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - w64).max()
    act = d['s']['activation']
    tol = G.tolerance(act, moved)
    print('DISTILL_GEN %-40s act %-4s |w - w64| %.3g  moved %.4f  ratio %.3g  bound %.3g' % (what, act, err, moved, err / moved, tol))
    assert err <= tol, '%s: |w - w64| = %.3g > %.3g (moved %.3g), worst at parameter %d' % (
        what, err, tol, moved, int(np.argmax(np.abs(got - w64))))
    return err / moved


@pytest.mark.parametrize('c', G.CASES, ids=G.case_id)
def test_general_kernel_vs_float64(engine, c):
    """one pair per case of the grid, every step of its minibatch table; NaN rows behind every unused slot, columns past the row and
    the neighbouring rows unchanged"""
    d, w64 = _ref(c)
    P = len(d['row'])
    out, before = _run(engine, c, 0)
    _check(out[1, :P], d, w64, G.case_id(c))
    np.testing.assert_array_equal(out[1, P:], before[1, P:])
    np.testing.assert_array_equal(out[[0, 2]], before[[0, 2]])


@pytest.mark.parametrize('c', G.CASES, ids=G.case_id)
def test_matrix_core_flavour_is_bit_for_bit_the_valu_one(engine, c):
    """dense = 1 against dense = 0 on the whole grid: the same bits in the trained row, nothing else written"""
    d, _ = _ref(c)
    out0, before = _run(engine, c, 0)
    out1, _ = _run(engine, c, 1)
    assert np.abs(out0[1, :len(d['row'])] - before[1, :len(d['row'])]).max() > G.MIN_MOVED
    np.testing.assert_array_equal(out1.view(np.uint32), out0.view(np.uint32))


@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('H,L,S,A,act', [(72, 3, 7, 3, 'elu'), (128, 4, 16, 4, 'relu'), (72, 3, 1, 1, 'tanh')])
def test_general_kernel_several_pairs_in_one_launch(engine, H, L, S, A, act, dense):
    """five pairs of one shape in one launch: different minibatch sizes, keep masks and lengths, a pair of n_steps = 0 between longer
    ones (bit for bit unchanged), buffers padded to the longest, a row stride larger than the row; columns past the row and rows
    outside the launch untouched"""
    kinds = [(128, 'half'), (3, 'mid'), (64, 'all'), (1, 'first'), (127, 'half')]
    cs = [((H, L, S, A, act, B, keep), 11 * S + 5 * A + k) for k, (B, keep) in enumerate(kinds)]
    cases = [_ref(c, seed)[0] for c, seed in cs]
    n_steps = [d['n_steps'] for d in cases]
    n_steps[2] = 0
    assert len(set(n_steps)) >= 3
    P = len(cases[0]['row'])
    out, before = _launch(engine, cases, dense, n_steps=n_steps, extra_rows=5, extra_steps=3, extra_cols=12)
    for k, ((c, seed), d) in enumerate(zip(cs, cases)):
        what = 'H%dL%d_S%dA%d_%s pair %d (B %d, %d steps)' % (H, L, S, A, act, k, d['B'], n_steps[k])
        if n_steps[k] == 0:
            np.testing.assert_array_equal(out[1 + k], before[1 + k], err_msg=what)
        else:
            _check(out[1 + k, :P], d, _ref(c, seed)[1], what)
    np.testing.assert_array_equal(out[:, P:], before[:, P:])
    np.testing.assert_array_equal(out[[0, len(cases) + 1]], before[[0, len(cases) + 1]])


def test_general_kernel_refusals_and_probe(engine):
    """shapes outside the learner's actor range are refused with SERL_E_UNSUPPORTED in both flavours and the weights stay
    untouched; every shape of the grid, every activation and both flavours pass the n_pairs = 0 probe, which needs no workspace"""
    from serl_amd import _capi
    dev = engine.device
    big = 130 * 17 + 130 + 5 * (130 * 130 + 3 * 130) + 5 * 130 + 5      # buffers sized for the largest shape asked for below
    child = torch.full((1, big + 3), 0.5, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    st = torch.from_numpy(rng.standard_normal((1, 8, 17)).astype(np.float32)).to(dev)
    tg = torch.zeros(1, 8, 5, device=dev)
    kp = torch.ones(1, 8, device=dev)
    sl = torch.zeros(1, 1, 128, dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    for H, L, S, A, act in ((2, 3, 7, 3, 0), (130, 3, 7, 3, 0), (34, 3, 7, 3, 0), (72, 5, 7, 3, 0), (72, 3, 0, 3, 0), (72, 3, 17, 3, 1),
                            (72, 3, 7, 0, 0), (72, 3, 7, 5, 2), (72, 3, 7, 3, -1), (72, 3, 7, 3, 3)):
        for dense in (0, 1):
            rc = _call(engine, child.data_ptr(), child.shape[1], 1, H, L, S, A, act, st, tg, kp, sl, one, one, dense)
            assert rc == _capi.E_UNSUPPORTED, (H, L, S, A, act, dense, rc)
            assert (child == 0.5).all(), (H, L, S, A, act, dense)
    for H, L, S, A in sorted({c[:4] for c in G.CASES}):
        for act in (0, 1, 2):
            for dense in (0, 1):
                rc = _call(engine, child.data_ptr(), child.shape[1], 0, H, L, S, A, act, st, tg, kp, sl, one, one, dense)
                assert rc == 0, (H, L, S, A, act, dense, rc)
    assert (child == 0.5).all()


@pytest.mark.parametrize('c', [c for c in G.CASES if c[:2] == (32, 3)], ids=G.case_id)
def test_both_kernels_at_hidden_32(engine, c):
    """at hidden 32 x 3 serl_ga_distill and the general kernel on the same case both stay within the float64 bound (the grid's and
    distill64's own), so they are within 2 x the bound of each other"""
    from test_gpu_distill import _launch as launch50
    d, w64 = _ref(c)
    P = len(d['row'])
    new, _ = _run(engine, c, 0)
    old, _ = launch50(engine, [d])
    moved = np.abs(w64 - d['row']).max()
    act = c[4]
    _check(new[1, :P], d, w64, 'general ' + G.case_id(c))
    err = np.abs(old[1, :P].astype(np.float64) - w64).max()
    print('DISTILL_GEN serl_ga_distill %-26s |w - w64| %.3g ratio %.3g' % (G.case_id(c), err, err / moved))
    assert err <= G.tolerance(act, moved)
    assert np.abs(new[1, :P].astype(np.float64) - old[1, :P]).max() <= 2 * G.tolerance(act, moved)


@pytest.mark.parametrize('H,act,dense', [(72, 'tanh', 'valu'), (96, 'relu', 'mfma')])
def test_distil_batch_general(engine, golden, monkeypatch, H, act, dense):
    """distill.distil_batch(kernel='general') with hidden-72 and non-tanh hidden-96 actors on reference-filled rings (the fixtures of
    test_gpu_distill.py::test_distil_batch_with_non_tanh_actors): the fused path is taken (the PyTorch path raises), info['path'] says
    which, and four pairs -- one with a child buffer of 100 rows -- agree with the same pairs trained one by one in PyTorch from the
    same seeds, python's generator left at the same place.  Both are f32 runs within the bound of the float64 one: 2 x the bound apart."""
    import actor_shapes as X
    import serl_amd
    from serl_amd import distill, replay
    from test_ga_host import distill_case
    args, _, _, _, critic, _, _ = distill_case(golden, 'd_18_0', engine.device, engine)
    spec = serl_amd.NetSpec(7, 3, H, 3, act)
    w = torch.from_numpy(X.make_weights(G.net(H, 3, 7, 3, act), 4, 31)).to(engine.device)
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
    info = {}
    with monkeypatch.context() as mp:
        mp.setattr(distill, 'distilation_crossover', unfused)
        random.seed(13); torch.manual_seed(13)
        kids = distill.distil_batch(args, engine, spec, w, pairs, bufs, critic, kernel='general', dense=dense, info=info)
        torch.cuda.synchronize()
        after, tafter = random.random(), torch.get_rng_state()
    assert info == {'path': 'fused-general-mfma' if dense == 'mfma' else 'fused-general'}
    random.seed(13); torch.manual_seed(13)
    ref = [distill.distilation_crossover(args, engine, spec, w, f, s, bufs, critic) for f, s in pairs]
    assert random.random() == after and torch.equal(torch.get_rng_state(), tafter)
    sizes = []
    for (row, buf, crit), (row2, buf2, _), (f, s) in zip(kids, ref, pairs):
        sizes.append(len(buf))
        assert len(crit) == 0
        assert len(buf) == len(buf2) == min(300, len(bufs[f])) + min(300, len(bufs[s]))
        np.testing.assert_array_equal(buf.rows[:len(buf)].cpu().numpy(), buf2.rows[:len(buf2)].cpu().numpy())
        a, b = row.cpu().numpy()[:P].astype(np.float64), row2.cpu().numpy()[:P].astype(np.float64)
        moved = np.abs(b - w[s].cpu().numpy()[:P]).max()
        assert moved > G.MIN_MOVED
        err = np.abs(a - b).max()
        print('DISTILL_GEN_BATCH H%d %s %s pair %s buffer %d |fused - torch| %.3g moved %.4f ratio %.3g' % (
            H, act, dense, (f, s), len(buf), err, moved, err / moved))
        assert err <= 2 * G.tolerance(act, moved), (act, f, s, err, moved)
    assert min(sizes) < 128


def test_distil_batch_auto_and_refused_general(engine, golden):
    """kernel='auto' takes serl_ga_distill at hidden 32 x 3 and the general kernel at 72 x 3; kernel='general' for a shape the kernel
    refuses (hidden 34) is a RuntimeError before any draw"""
    import actor_shapes as X
    import serl_amd
    from serl_amd import distill, replay
    from test_ga_host import distill_case
    args, _, _, _, critic, _, _ = distill_case(golden, 'd_18_0', engine.device, engine)
    args.individual_bs = 300
    Pg = golden('proximal')
    bufs = []
    for i in (18, 0):
        r = replay.DeviceReplay(10_000, engine.device, engine)
        r.append_rows(torch.from_numpy(Pg['buf_serl50_%d' % i][:400]))
        bufs.append(r)
    for H, want in ((32, 'fused'), (72, 'fused-general')):
        spec = serl_amd.NetSpec(7, 3, H, 3, 'tanh')
        w = torch.from_numpy(X.make_weights(G.net(H, 3, 7, 3, 'tanh'), 2, 3)).to(engine.device)
        info = {}
        random.seed(2); torch.manual_seed(2)
        (row, buf, _), = distill.distil_batch(args, engine, spec, w, [(0, 1)], bufs, critic, kernel='auto', info=info)
        torch.cuda.synchronize()
        assert info['path'] == want
        assert torch.isfinite(row).all() and (row[:spec.param_count] - w[1, :spec.param_count]).abs().max() > G.MIN_MOVED
    w = torch.zeros(2, 4096, device=engine.device)
    random.seed(2)
    st = random.getstate()
    with pytest.raises(RuntimeError, match='serl_ga_distill_general'):
        distill.distil_batch(args, engine, types.SimpleNamespace(state_dim=7, action_dim=3, hidden=34, num_layers=3, activation='tanh',
                                                                 activation_id=0, param_count=4000), w, [(0, 1)], bufs, critic, kernel='general')
    assert random.getstate() == st


def test_ssne_epoch_with_the_general_kernel(engine, golden):
    """SSNE(.., distil_kernel='general').epoch at hidden 72 x 3 records the operator calls of distil_kernel='serl50' (which trains such
    actors pair by pair in PyTorch) from the same seeds, leaves python's generator at the same place, trains the same children to
    within 2 x the bound (at least one of them far from its parent), and says what ran in last_distil_path"""
    import actor_shapes as X
    import serl_amd
    from serl_amd import replay, ssne
    from test_ga_host import distill_case
    _, _, _, _, critic, _, _ = distill_case(golden, 'd_18_0', engine.device, engine)
    n = 8
    spec = serl_amd.NetSpec(7, 3, 72, 3, 'tanh')
    P = spec.param_count
    w0 = X.make_weights(G.net(72, 3, 7, 3, 'tanh'), n, 5)
    Pg = golden('proximal')
    args = types.SimpleNamespace(pop_size=n, elite_fraction=0.25, mutation_prob=0.0, mutation_mag=0.05, mut_type='normal',
                                 distil_crossover=True, distil_type='fitness', crossover_prob=0.0, mutation_batch_size=86, individual_bs=300)
    fit = np.random.default_rng(2).normal(-150, 50, n)
    runs = {}
    for kernel in ('serl50', 'general'):
        bufs, crits = [], []
        for k in range(n):
            r = replay.DeviceReplay(10_000, engine.device, engine)
            r.append_rows(torch.from_numpy(Pg['buf_serl50_%d' % (18, 0, 7, 33)[k % 4]][:900 - 100 * k]))
            bufs.append(r)
            crits.append(replay.DeviceReplay(10_000, engine.device, engine))
        w = torch.from_numpy(w0.copy()).to(engine.device)
        rec = []
        random.seed(3); np.random.seed(3); torch.manual_seed(3)
        ep = ssne.SSNE(args, engine, spec, critic=critic, record=rec, distil_kernel=kernel)
        assert ep.last_distil_path is None
        slot = ep.epoch(w, fit, buffers=bufs, critical=crits)
        torch.cuda.synchronize()
        runs[kernel] = (rec, slot, random.random(), w.cpu().numpy()[:, :P], ep.last_distil_path)
    (rec_a, slot_a, rnd_a, w_a, path_a), (rec_b, slot_b, rnd_b, w_b, path_b) = runs['serl50'], runs['general']
    assert (path_a, path_b) == ('torch', 'fused-general')
    assert rec_a == rec_b and slot_a == slot_b and rnd_a == rnd_b
    pairs = [(r[1], r[2], rec_a[k + 1][2]) for k, r in enumerate(rec_a) if r[0] == 3]      # (first, second, the child's slot)
    print('DISTILL_GEN_EPOCH operator calls %s' % (rec_a,))
    children, moved_most = [slot for _, _, slot in pairs], 0.0
    for first, second, slot in pairs:
        # (the parents are not written after the clones; a pair of a member with its own clone keeps no state -- equal Q -- and its
        # child takes zero-gradient steps from zero moments: it does not move, on either path)
        moved = np.abs(w_a[slot].astype(np.float64) - w_a[second]).max()
        moved_most = max(moved_most, moved)
        err = np.abs(w_a[slot].astype(np.float64) - w_b[slot]).max()
        print('DISTILL_GEN_EPOCH pair (%d, %d) -> slot %d |general - torch| %.3g moved %.4f' % (first, second, slot, err, moved))
        assert err <= 2 * G.tolerance('tanh', moved), (first, second, slot, err, moved)
    assert moved_most > G.MIN_MOVED
    others = [k for k in range(n) if k not in children]
    np.testing.assert_array_equal(w_a[others], w_b[others])

"""serl_ga_distill_general at the edges of its contract (tests/distill_general_edges.py): no hidden layer against float64; every clamp
and the keep rule as bit-for-bit equalities between two launches that the contract calls equivalent, one of them checked against
float64 -- on serl_ga_distill at hidden 32 x 3 as well, whose semantics the general kernel states as its own; row strides, child and
workspace pointers that are only 4 B aligned, whatever the workspace holds, a workspace of the exact size; 600 pairs in one launch;
other learning rates and 276 and 1000 steps against float64; and the SERL_E_INVALID refusals, which must launch nothing."""
import ctypes
import functools
import numpy as np
import pytest
import torch
import distill64 as D
import distill64_shapes as G
import distill_general_edges as E
import test_gpu_distill as T50
import test_gpu_distill_general as T

pytestmark = pytest.mark.gpu

KERNELS = ['valu', 'mfma', 'serl50']        # the general kernel's two dense flavours at SHAPE_B, serl_ga_distill at SHAPE_50
KERNEL_ACTS = [(k, a) for k in KERNELS[:2] for a in E.ACTS] + [('serl50', 'elu')]     # B1, B5: every activation on the general kernel
DENSE = [0, 1]
DENSE_IDS = ['valu', 'mfma']


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what=''):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=str(what))


def _shape(kernel):
    return E.SHAPE_50 if kernel == 'serl50' else E.SHAPE_B


def _go(engine, kernel, cases, **kw):
    """one launch of `kernel` -> (child after, before)"""
    if kernel == 'serl50':
        return T50._launch(engine, cases, **kw)
    return T._launch(engine, cases, KERNELS.index(kernel), **kw)


@functools.lru_cache(maxsize=None)
def _pair(build, act, shape, *a):
    """a raw pair, the pair the contract makes of it and that pair's float64 run, computed once"""
    d = build(act, *a, shape=shape)
    c = E.contract_case(d)
    return d, c, D.distill64(c)


def _check64(kernel, got, c, w64, what):
    """a trained row against the float64 run of its contract pair, within the bound of the kernel that trained it"""
    if kernel == 'serl50':
        return T50._check(got, c, what)
    return T._check(got, c, w64, what)


# ---- A ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', E.L0_CASES, ids=G.case_id)
def test_no_hidden_layer_vs_float64(engine, c):
    """L = 0: Linear, activation, Linear, tanh -- no LayerNorm layer, a tape of two layers.  Both dense flavours against float64 and bit
    for bit against each other; columns past the row and the neighbouring rows unchanged"""
    d, w64 = T._ref(c)
    P = len(d['row'])
    assert P == G.param_count(*c[:4]) and d['s']['num_layers'] == 0
    out0, before = T._launch(engine, [d], 0)
    out1, _ = T._launch(engine, [d], 1)
    T._check(out0[1, :P], d, w64, G.case_id(c))
    _same(out1, out0, c)
    _same(out0[1, P:], before[1, P:])
    _same(out0[[0, 2]], before[[0, 2]])


def test_no_hidden_layer_passes_the_probe(engine):
    """the n_pairs = 0 probe of test_general_kernel_refusals_and_probe at the L = 0 shapes: every activation, both flavours, no workspace"""
    dev = engine.device
    child = torch.full((1, 4096), 0.5, dtype=torch.float32, device=dev)
    st, tg, kp = torch.zeros(1, 8, 16, device=dev), torch.zeros(1, 8, 4, device=dev), torch.ones(1, 8, device=dev)
    sl = torch.zeros(1, 1, 128, dtype=torch.int32, device=dev)
    one = torch.ones(1, dtype=torch.int32, device=dev)
    for H, L, S, A in sorted({c[:4] for c in E.L0_CASES}):
        for act in (0, 1, 2):
            for dense in DENSE:
                assert T._call(engine, child.data_ptr(), child.shape[1], 0, H, L, S, A, act, st, tg, kp, sl, one, one, dense) == 0, (H, L, S, A, act, dense)
    assert (child == 0.5).all()


# ---- B ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel,act', KERNEL_ACTS)
def test_slots_outside_the_table_are_clamped(engine, act, kernel):
    """B1: a table a quarter of whose used entries are -1, -rows, INT32_MIN, rows, rows + 7 or INT32_MAX gives the bits of the same table
    clamped on the host.  Rows 0 and rows - 1 are real, kept rows (no padding row); unused columns and steps hold INT32_MAX."""
    d, c, w64 = _pair(E.slots_case, act, _shape(kernel))
    rows, P = len(d['keep']), len(d['row'])
    used = d['slots'][:, :d['B']]
    assert 0.15 < ((used < 0) | (used >= rows)).mean() < 0.35 and {int(v) for v in E.OUT_OF_RANGE(rows)} <= set(used.ravel().tolist())
    kw = dict(extra_rows=0, extra_steps=2, unused_slot=E.I32_MAX)
    raw, before = _go(engine, kernel, [d], **kw)
    ref, _ = _go(engine, kernel, [E.clamped(d)], **kw)
    _check64(kernel, ref[1, :P], c, w64, 'B1 %s %s' % (kernel, act))
    _same(raw, ref)
    _same(raw[1, P:], before[1, P:])
    _same(raw[[0, 2]], before[[0, 2]])


@pytest.mark.parametrize('kernel', KERNELS)
def test_batch_above_128_is_128(engine, kernel):
    """B2: batch[p] = 129, 1000, INT32_MAX on a table of 128 valid columns: the bits of batch[p] = 128"""
    d, c, w64 = _pair(E.batch_case, 'elu', _shape(kernel))
    P = len(d['row'])
    ref, before = _go(engine, kernel, [d])
    _check64(kernel, ref[1, :P], c, w64, 'B2 %s' % kernel)
    for b in E.BATCH_TOO_LARGE:
        out, _ = _go(engine, kernel, [d], batch=[b])
        _same(out, ref, b)


@pytest.mark.parametrize('kernel', KERNELS)
def test_batch_of_no_rows_takes_zero_gradient_steps(engine, kernel):
    """B3: batch[p] = 0, -1, INT32_MIN: every step is a minibatch with no kept row, an Adam step with zero gradients from zero moments --
    an update of 0 / (0 + eps).  The float64 loop on a table whose every row is dropped leaves the row as it was, bit for bit
    (tests/test_distill_general_edges_host.py), and so must the kernel -- having run: the table and n_steps are those of B2."""
    d, _, _ = _pair(E.batch_case, 'elu', _shape(kernel))
    P = len(d['row'])
    w64 = D.distill64(dict(d, keep=np.zeros_like(d['keep'])))
    for b in E.BATCH_NONE:
        out, before = _go(engine, kernel, [d], batch=[b])
        np.testing.assert_array_equal(out[1, :P].astype(np.float64), w64, err_msg=str(b))
        _same(out, before, b)


@pytest.mark.parametrize('kernel', KERNELS)
def test_n_steps_past_the_table_is_the_table(engine, kernel):
    """B4: n_steps[p] = steps + 1, INT32_MAX: the bits of n_steps[p] = steps"""
    d, c, w64 = _pair(E.steps_case, 'tanh', _shape(kernel))
    P, steps = len(d['row']), d['n_steps']
    ref, _ = _go(engine, kernel, [d])
    _check64(kernel, ref[1, :P], c, w64, 'B4 %s' % kernel)
    for n in (steps + 1, E.I32_MAX):
        out, _ = _go(engine, kernel, [d], n_steps_arg=[n])
        _same(out, ref, n)


@pytest.mark.parametrize('kernel', KERNELS)
def test_negative_n_steps_is_zero(engine, kernel):
    """B4: n_steps[p] = -1, INT32_MIN for the pair between two that train (its table is filled: steps taken would show): its row and
    the columns behind it unchanged bit for bit, the neighbours' rows those of the launch with n_steps[p] = 0, the guard rows untouched"""
    shape = _shape(kernel)
    trio = [_pair(E.steps_case, 'tanh', shape, k) for k in range(3)]
    cases = [t[0] for t in trio]
    P = len(cases[0]['row'])
    ref, before = _go(engine, kernel, cases, n_steps_arg=[24, 0, 24], extra_cols=4)
    for k in (0, 2):
        _check64(kernel, ref[1 + k, :P], trio[k][1], trio[k][2], 'B4 %s pair %d' % (kernel, k))
    _same(ref[2], before[2])
    for n in (-1, E.I32_MIN):
        out, _ = _go(engine, kernel, cases, n_steps_arg=[24, n, 24], extra_cols=4)
        _same(out[2], before[2], n)
        _same(out, ref, n)
        _same(out[[0, 4]], before[[0, 4]], n)
        _same(out[:, P:], before[:, P:], n)


@pytest.mark.parametrize('kernel,act', KERNEL_ACTS)
def test_keep_is_a_flag(engine, act, kernel):
    """B5: a mask of 2, -1, 0.5, the smallest positive subnormal and 1 (kept), -0.0 and 0.0 (dropped) gives the bits of the mask mapped
    to 1 / 0 by keep != 0"""
    d, c, w64 = _pair(E.keep_case, act, _shape(kernel))
    P = len(d['row'])
    assert set(np.unique(d['keep'])) >= {np.float32(v) for v in E.KEEP_VALUES_KEPT} and np.signbit(d['keep']).sum() > 20
    flags = E.keep_as_flags(d)
    assert flags['keep'][d['keep'] == np.float32(1e-45)].all() and not flags['keep'][np.signbit(d['keep']) & (d['keep'] == 0)].any()
    ref, _ = _go(engine, kernel, [flags])
    _check64(kernel, ref[1, :P], c, w64, 'B5 %s %s' % (kernel, act))
    raw, _ = _go(engine, kernel, [d])
    _same(raw, ref)


@pytest.mark.parametrize('dense', DENSE, ids=DENSE_IDS)
def test_minibatches_that_repeat_rows(engine, dense):
    """B6: minibatches drawn with replacement, one of them 64 times the same row, against float64"""
    d, c, w64 = _pair(E.repeats_case, 'tanh', E.SHAPE_B)
    out, _ = T._launch(engine, [d], dense)
    T._check(out[1, :len(d['row'])], c, w64, 'B6 %s' % DENSE_IDS[dense])


# ---- C ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout(shape):
    cases = E.layout_cases(shape)
    return cases, [D.distill64(d) for d in cases]


_ALIGNED = {}


def _aligned(engine, shape, dense):
    """the three pairs of `shape` with a row stride that is a multiple of 4, a fresh allocation and a workspace of the kernel's size,
    checked against float64: what every layout below must reproduce"""
    if (shape, dense) not in _ALIGNED:
        cases, w64 = _layout(shape)
        out, before = T._launch(engine, cases, dense)
        P = len(cases[0]['row'])
        for k, d in enumerate(cases):
            T._check(out[1 + k, :P], d, w64[k], 'C %s pair %d %s' % (shape, k, DENSE_IDS[dense]))
        _ALIGNED[shape, dense] = out, before
    return _ALIGNED[shape, dense]


@pytest.mark.parametrize('dense', DENSE, ids=DENSE_IDS)
@pytest.mark.parametrize('shape', [E.SHAPE_B, E.SHAPE_C], ids=['H36L2', 'H72L3'])
def test_row_stride_and_alignment_do_not_matter(engine, shape, dense):
    """C1: row strides P + 1, P + 2, P + 3 and P + 5 (three rows: every remainder of 16 B) and a child tensor that starts one, two and
    three floats into its allocation train the bits of the aligned launch; columns between the rows and the guard rows untouched"""
    cases, _ = _layout(shape)
    P = len(cases[0]['row'])
    ref, _ = _aligned(engine, shape, dense)
    assert {((1 + k) * (P + extra)) % 4 for extra in (1, 2, 3) for k in range(3)} == {0, 1, 2, 3}       # (in floats, from a 16 B aligned allocation)
    for extra in (1, 2, 3, 5):
        out, before = T._launch(engine, cases, dense, stride=P + extra)
        assert out.shape[1] == P + extra
        _same(out[1:4, :P], ref[1:4, :P], extra)
        _same(out[:, P:], before[:, P:], extra)
        _same(out[[0, 4]], before[[0, 4]], extra)
    for off in (1, 2, 3):
        out, before = T._launch(engine, cases, dense, child_offset=off)
        _same(out, ref, off)


@pytest.mark.parametrize('dense', DENSE, ids=DENSE_IDS)
@pytest.mark.parametrize('shape', [E.SHAPE_B, E.SHAPE_C], ids=['H36L2', 'H72L3'])
def test_workspace_contents_do_not_matter(engine, shape, dense):
    """C2: a workspace of zeros, of NaN, of 3e38, and one that a launch of the OTHER shape has just used (sized for the larger of the
    two) give the bits of a fresh one"""
    from serl_amd import _capi
    cases, _ = _layout(shape)
    other = E.SHAPE_C if shape == E.SHAPE_B else E.SHAPE_B
    ref, _ = _aligned(engine, shape, dense)
    n, n_other = (int(_capi.lib().serl_ga_distill_general_work_bytes(3, s[2], s[3], s[0], s[1])) // 4 for s in (shape, other))
    for fill in (0.0, float('nan'), 3e38):
        out, _ = T._launch(engine, cases, dense, work=torch.full((n,), fill, dtype=torch.float32, device=engine.device))
        _same(out, ref, fill)
    wk = torch.full((max(n, n_other),), 1.0, dtype=torch.float32, device=engine.device)
    T._launch(engine, _layout(other)[0], dense, work=wk[:n_other])
    assert (wk[:n_other] != 1.0).any()
    out, _ = T._launch(engine, cases, dense, work=wk[:n])
    _same(out, ref, 'after the other shape')


@pytest.mark.parametrize('dense', DENSE, ids=DENSE_IDS)
@pytest.mark.parametrize('shape', [E.SHAPE_B, E.SHAPE_C], ids=['H36L2', 'H72L3'])
def test_workspace_of_the_exact_size_at_float_alignment(engine, shape, dense):
    """C3: serl_ga_distill_general_work_bytes bytes and not one more, one float into a NaN-filled allocation (4 B alignment is what
    include/serl_amd.h asks of `work`): the bits of the aligned launch, and every float on both sides still the NaN it was"""
    from serl_amd import _capi
    cases, _ = _layout(shape)
    ref, _ = _aligned(engine, shape, dense)
    nbytes = int(_capi.lib().serl_ga_distill_general_work_bytes(3, shape[2], shape[3], shape[0], shape[1]))
    assert nbytes % 4 == 0
    n = nbytes // 4
    big = torch.full((1 + n + 1024,), float('nan'), dtype=torch.float32, device=engine.device)
    assert big.data_ptr() % 16 == 0
    was = big.view(torch.int32).clone()
    out, _ = T._launch(engine, cases, dense, work=big[1:1 + n])
    _same(out, ref)
    now = big.view(torch.int32)
    assert torch.equal(now[:1], was[:1]) and torch.equal(now[1 + n:], was[1 + n:])
    assert not torch.equal(now[1:1 + n], was[1:1 + n])


@pytest.mark.parametrize('dense', DENSE, ids=DENSE_IDS)
def test_table_of_one_row(engine, dense):
    """C4: rows = 1: whatever the slots say, every sample is row 0; against float64"""
    d, c, w64 = _pair(E.one_row_case, 'elu', E.SHAPE_B)
    assert len(d['keep']) == 1 and (c['slots'] == 0).all()
    out, before = T._launch(engine, [d], dense, extra_rows=0, unused_slot=E.I32_MAX)
    T._check(out[1, :len(d['row'])], c, w64, 'C4 %s' % DENSE_IDS[dense])
    _same(out[[0, 2]], before[[0, 2]])


# ---- D ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', DENSE, ids=DENSE_IDS)
def test_six_hundred_pairs_in_one_launch(engine, dense):
    """D: more workgroups than the device has CUs, each on its own slice of the workspace: 600 pairs cycling through six cases, every
    row the bits of its case launched alone (those against float64), one pair in each hundred with n_steps = 0 and unchanged"""
    six = E.many_cases()
    P = len(six[0]['row'])
    assert E.N_MANY > torch.cuda.get_device_properties(engine.device).multi_processor_count
    alone = []
    for k, d in enumerate(six):
        out, _ = T._launch(engine, [d], dense)
        T._check(out[1, :P], d, D.distill64(d), 'D case %d %s' % (k, DENSE_IDS[dense]))
        alone.append(out[1])
    cases = [six[k % 6] for k in range(E.N_MANY)]
    n_steps = [0 if k % 100 == E.MANY_IDLE else 8 for k in range(E.N_MANY)]
    assert n_steps.count(0) == 6
    out, before = T._launch(engine, cases, dense, n_steps_arg=n_steps)
    want = np.stack([before[1 + k] if n_steps[k] == 0 else alone[k % 6] for k in range(E.N_MANY)])
    _same(out[1:-1], want)
    _same(out[[0, -1]], before[[0, -1]])


# ---- E ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', E.E_CASES, ids=E.e_id)
def test_learning_rates_and_step_counts_vs_float64(engine, c):
    """E: lr 1e-4 and 3e-3 at 60 steps, lr 1e-3 at 276 (a production pair) and 1000 steps: both flavours against float64 within the
    grid's bound, bit for bit each other"""
    d = E.e_case(c)
    P = len(d['row'])
    w64 = D.distill64(d, c[1])
    out0, _ = T._launch(engine, [d], 0, lr=c[1])
    out1, _ = T._launch(engine, [d], 1, lr=c[1])
    moved = np.abs(w64 - d['row']).max()
    assert E.e_tolerance(c, moved) == G.tolerance(c[0], moved)
    T._check(out0[1, :P], d, w64, 'E ' + E.e_id(c))
    _same(out1, out0)


# ---- F ------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_nothing_is_launched(engine):
    """F: lr 0, negative or NaN, a row stride below the parameter count, no workspace or one a byte short, each pointer NULL in turn,
    rows = 0, steps = -1, n_pairs = -1, dense -1 or 2: SERL_E_INVALID, and the child -- a constant before -- unchanged.  steps = 0 is
    SERL_OK and writes nothing.  The arguments are otherwise those of a launch that trains (asserted last)."""
    from serl_amd import _capi
    from serl_amd.actor import ACTIVATION_IDS
    lib, dev = _capi.lib(), engine.device
    H, L, S, A = E.SHAPE_B
    d = E.steps_case('tanh')
    P, rows, steps = len(d['row']), len(d['keep']), d['n_steps']
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    child = torch.full((3, P + 4), 0.25, dtype=torch.float32, device=dev)
    nbytes = int(lib.serl_ga_distill_general_work_bytes(1, S, A, H, L))
    wk = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
    keepalive = [t(d['states'][None]), t(d['targets'][None]), t(d['keep'][None]), t(d['slots'][None]), t(np.array([steps], np.int32)),
                 t(np.array([d['B']], np.int32))]
    st, tg, kp, sl, ns, bt = (x.data_ptr() for x in keepalive)
    good = dict(ctx=engine.ctx, child=child[1].data_ptr(), stride=P + 4, n_pairs=1, S=S, H=H, L=L, A=A, act=ACTIVATION_IDS['tanh'], states=st,
                targets=tg, keep=kp, rows=rows, slots=sl, steps=steps, n_steps=ns, batch=bt, lr=D.LR, work=wk.data_ptr(), work_bytes=nbytes, dense=0)

    def call(**over):
        a = dict(good, **over)
        rc = lib.serl_ga_distill_general(a['ctx'], a['child'], a['stride'], a['n_pairs'], a['S'], a['H'], a['L'], a['A'], a['act'], a['states'],
                                         a['targets'], a['keep'], a['rows'], a['slots'], a['steps'], a['n_steps'], a['batch'], ctypes.c_float(a['lr']),
                                         a['work'], a['work_bytes'], a['dense'], ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        return rc
    bad = [dict(lr=0.0), dict(lr=-1e-3), dict(lr=float('nan')), dict(stride=P - 1), dict(work=None), dict(work_bytes=nbytes - 1),
           dict(rows=0), dict(steps=-1), dict(n_pairs=-1), dict(dense=-1), dict(dense=2)]
    bad += [{k: None} for k in ('ctx', 'child', 'states', 'targets', 'keep', 'slots', 'n_steps', 'batch')]
    assert len(bad) == 19
    for over in bad:
        assert call(**over) == _capi.E_INVALID, over
        assert (child == 0.25).all(), over
    assert call(steps=0) == 0
    assert (child == 0.25).all()
    assert call() == 0
    assert (child[[0, 2]] == 0.25).all() and (child[1, P:] == 0.25).all() and (child[1, :P] != 0.25).any()

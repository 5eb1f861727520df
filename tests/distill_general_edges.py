"""Shared by tests/test_distill_general_edges_host.py (CPU) and tests/test_gpu_distill_general_edges.py (GPU): serl_ga_distill_general at
the edges of its contract -- no hidden layer, every clamp the kernel applies to what its tables hold (slots, batch, n_steps), the keep
rule, repeated rows, row strides and pointers that are only 4 B aligned, what the workspace holds, many pairs, other learning rates and
three- and four-digit step counts.  The cases, their construction, the contract on raw inputs written out with planted mistakes, and the
calibration notes.  The float64 loops are distill64's.  A plain module (not a conftest): nothing here is a fixture.

A pair here is distill64_shapes.make_case's dict.  What is raw about it: `slots` may name rows outside the table, `keep` may hold any
float, and the batch and n_steps handed to the kernel are given beside the dict."""
import numpy as np
import distill64 as D
import distill64_shapes as G

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
ACTS = G.ACTS
SHAPE_B = (36, 2, 7, 3)                     # (H, L, S, A) of sections B and E; C adds SHAPE_C, the overlap with serl_ga_distill is SHAPE_50
SHAPE_C = (72, 3, 16, 4)
SHAPE_50 = (32, 3, 7, 3)
SHAPE_D = (4, 1, 7, 3)


def make_pair(act, B, rows, n_steps, seed, keep_mode='half', replace=False, shape=SHAPE_B):
    """distill64_shapes.make_case's construction with the buffer length and the step count given: minibatches of B of `rows` rows, drawn
    without replacement, or with"""
    import actor_shapes as X
    H, L, S, A = shape
    assert replace or rows >= B
    rng = np.random.default_rng(seed)
    s = G.net(H, L, S, A, act)
    w = X.make_weights(s, 2, seed)
    P = G.param_count(H, L, S, A)
    states = (rng.standard_normal((rows, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)
    targets = X.forward64(s, w[1, :P], states).astype(np.float32)
    keep = np.ones(rows, np.float32)
    if keep_mode == 'half':
        keep[rng.permutation(rows)[:rows // 2]] = 0.0
    slots = np.zeros((n_steps, 128), np.int32)
    for k in range(n_steps):
        slots[k, :B] = rng.choice(rows, B, replace=replace)
    return dict(s=s, row=w[0, :P].copy(), states=states, targets=targets, keep=keep, slots=slots, n_steps=n_steps, B=B)


# ---- A: no hidden layer -------------------------------------------------------------------------------------------------------------
L0_SHAPES = [(4, 0), (72, 0), (128, 0)]
L0_BATCHES = [1, 127, 128]


def _l0_grid():
    """distill64_shapes._grid for the L = 0 shapes: three minibatch sizes per shape, (S, A), activation and keep mode walked round"""
    out = []
    for i, (H, L) in enumerate(L0_SHAPES):
        for k, B in enumerate(L0_BATCHES):
            S, A = G.DIMS[(i + k) % 3]
            out.append((H, L, S, A, ACTS[(2 * i + k) % 3], B, G.KEEPS[(i + 3 * k) % 4]))
    return out


L0_CASES = _l0_grid()


# ---- B: the clamps and the keep rule ------------------------------------------------------------------------------------------------
OUT_OF_RANGE = lambda rows: [-1, -rows, I32_MIN, rows, rows + 7, I32_MAX]
KEEP_VALUES_KEPT = [2.0, -1.0, 0.5, float(np.float32(1e-45)), 1.0]          # (1e-45 rounds to the smallest positive f32 subnormal, 2^-149)
KEEP_VALUES_DROPPED = [-0.0, 0.0]


def slots_case(act, shape=SHAPE_B):
    """B1: 24 steps of 100 of 300 rows in which about a quarter of the used entries name a row outside the table, all six kinds in turn.
    Rows 0 and rows - 1, where they must land, are kept rows."""
    d = make_pair(act, 100, 300, 24, 9000 + len(act), shape=shape)
    rng = np.random.default_rng(77)
    bad = rng.random((24, 100)) < 0.25
    vals = np.array(OUT_OF_RANGE(300), np.int64)
    sl = d['slots'].astype(np.int64)
    sl[:, :100][bad] = vals[np.arange(int(bad.sum())) % 6]
    d['slots'] = sl.astype(np.int32)
    d['keep'][[0, 299]] = 1.0
    return d


def clamped(d):
    """the same pair with its table clamped on the host"""
    return dict(d, slots=np.clip(d['slots'], 0, len(d['keep']) - 1))


def batch_case(act, shape=SHAPE_B):
    """B2, B3: 24 steps of 128 of 300 rows, every column of the table valid"""
    return make_pair(act, 128, 300, 24, 9100 + len(act), shape=shape)


BATCH_TOO_LARGE = [129, 1000, I32_MAX]
BATCH_NONE = [0, -1, I32_MIN]


def steps_case(act, k=0, shape=SHAPE_B):
    """B4: 24 steps of 37 of 90 rows (k: one of the three pairs of the launch)"""
    return make_pair(act, 37, 90, 24, 9200 + len(act) + 10 * k, shape=shape)


def keep_case(act, shape=SHAPE_B):
    """B5: 24 steps of 64 of 200 rows; the kept half of the mask holds 2, -1, 0.5, the smallest subnormal and 1 in turn, the dropped half
    -0.0 and 0.0"""
    d = make_pair(act, 64, 200, 24, 9300 + len(act), shape=shape)
    kp = d['keep'].copy()
    on, off = np.flatnonzero(kp != 0), np.flatnonzero(kp == 0)
    kp[on] = np.array(KEEP_VALUES_KEPT, np.float32)[np.arange(len(on)) % len(KEEP_VALUES_KEPT)]
    kp[off] = np.array(KEEP_VALUES_DROPPED, np.float32)[np.arange(len(off)) % 2]
    d['keep'] = kp
    return d


def keep_as_flags(d):
    """the same pair with its mask mapped to 1.0 / 0.0 by keep != 0, as numpy evaluates it in float32"""
    assert d['keep'].dtype == np.float32
    return dict(d, keep=(d['keep'] != 0).astype(np.float32))


def repeats_case(act, shape=SHAPE_B):
    """B6: 24 steps of 64 rows drawn WITH replacement from 40 (every minibatch repeats rows), step 5 naming one row 64 times"""
    d = make_pair(act, 64, 40, 24, 9400 + len(act), keep_mode='all', replace=True, shape=shape)
    d['slots'][5, :64] = 17
    assert all(len(set(r[:64])) < 64 for r in d['slots'])
    return d


def one_row_case(act, shape=SHAPE_B):
    """C4: a table of one row; the slots name everything but it"""
    d = make_pair(act, 5, 1, 24, 9500 + len(act), keep_mode='all', replace=True, shape=shape)
    d['slots'][:, :5] = np.array([1, -1, I32_MAX, I32_MIN, 3], np.int32)
    return d


# ---- C: layouts -------------------------------------------------------------------------------------------------------------------
def layout_cases(shape):
    """three pairs of one shape: different minibatch sizes, buffer lengths and keep masks, 24 steps"""
    act = {SHAPE_B: 'elu', SHAPE_C: 'relu'}.get(shape, 'tanh')
    return [make_pair(act, B, rows, 24, 9600 + k, keep_mode=km, shape=shape) for k, (B, rows, km) in
            enumerate([(128, 300, 'half'), (37, 90, 'all'), (3, 3, 'all')])]


# ---- D: many pairs ------------------------------------------------------------------------------------------------------------------
N_MANY = 600
MANY_IDLE = 57                              # pairs k with k % 100 == MANY_IDLE have n_steps = 0


def many_cases():
    """the six distinct pairs that the 600 cycle through: (4, 1, 7, 3) with ELU (a launch has one activation), minibatches of 3 of 10
    rows, 8 steps"""
    return [make_pair('elu', 3, 10, 8, 9700 + k, keep_mode='all' if k < 3 else 'half', shape=SHAPE_D) for k in range(6)]


# ---- E: learning rates and step counts ----------------------------------------------------------------------------------------------
#   (lr, steps)
LR_STEPS = [(1e-4, 60), (3e-3, 60), (1e-3, 276), (1e-3, 1000)]
E_CASES = [(act, lr, steps) for lr, steps in LR_STEPS for act in ACTS]


def e_id(c):
    return '%s_lr%g_%dsteps' % c


def e_case(c, seed=None):
    """minibatches of 64 of 300 rows, about half of them kept"""
    act, lr, steps = c
    return make_pair(act, 64, 300, steps, (9800 + steps + len(act)) if seed is None else seed)


# The tolerance of every case here is distill64_shapes.tolerance(act, moved), unchanged.  For E it was calibrated as that module's was, on
# the CPU and never on the kernel: distill64.distill32 (the literal loop in float32 torch) against distill64.distill64 over E_CASES and
# five more seeds of each (seeds 1000 .. 1004 of e_case), 72 runs; max |w32 - w64| / moved:
#   * lr 1e-4, 60 steps: 0.8e-4 .. 1.5e-4 in all 18 runs, whatever the activation (worst: tanh 1.25e-4, ELU 1.46e-4, LeakyReLU 1.27e-4).
#     The parameters move by 6e-3 only (5.8e-3 .. 6.9e-3: above MIN_MOVED in every run), in steps of 1e-4 on weights of the order of 1,
#     each step rounded to an f32 ulp of 6e-8: the rounding of w itself, which does not shrink with lr, is what is seen.
#   * lr 3e-3, 60 steps: 5e-6 .. 1.1e-5.   * lr 1e-3, 276 steps: 0.8e-5 .. 2.2e-5.
#   * lr 1e-3, 1000 steps: tanh, ELU 0.9e-5 .. 3.0e-5; LeakyReLU 1.1e-5 .. 1.5e-5 in three runs and 1.1e-3, 2.3e-3 (the grid case), 2.9e-3
#     in three: the kinks of distill64.py, which a thousand steps meet more often than sixty.
# Worst per activation: tanh 1.25e-4, ELU 1.46e-4, LeakyReLU 2.9e-3 -- 0.05, 0.06 and 0.014 of distill64_shapes.TOL_REL, under half of it
# in every case, so the bound is that module's, unchanged.  The cases of A, B, C and D (24 or 8 steps, lr 1e-3) stay below 6.1e-5.
# The kernel on the MI355X (tests/test_gpu_distill_general_edges.py, both dense flavours -- the same bits), max |w - w64| / moved.  E: tanh
# 1.11e-4 and ELU 9.4e-5 (both lr 1e-4, 60 steps: the float32 loop's figures of those two runs to three digits), LeakyReLU 2.26e-3
# (1000 steps: the float32 loop's figure again -- the kernel takes that run's kinks where torch's f32 does), 0.8e-5 .. 2.4e-5 elsewhere.
# A, B, C, D: tanh 2.4e-5 (B1), ELU 3.6e-5 (D, case 0), LeakyReLU 3.1e-5 (C, 72 x 3, the pair of three rows); serl_ga_distill at hidden
# 32 x 3 on B1 - B5: 2.6e-5 at the worst.  None of these figures enters a bound.
def e_tolerance(c, moved):
    return G.tolerance(c[0], moved)


# ---- G: the contract on raw inputs, written out, with planted mistakes ----------------------------------------------------------------
MISTAKES = ('slot_wraps', 'slot_unclamped_low', 'batch_unclamped_high', 'keep_positive_only', 'keep_as_weight', 'moments_carried',
            'steps_unclamped')


def contract_case(d, batch=None, n_steps=None, mistake=None):
    """what the kernel makes of a raw pair and the raw batch / n_steps beside it (default: the pair's own) -> the pair distill64 takes:
    n_steps into [0, the table's steps], batch into [0, 128], every slot into [0, rows), keep to a flag by keep != 0.  With a mistake:
      slot_wraps            a slot is taken modulo rows
      slot_unclamped_low    only the upper bound is applied; a negative slot counts back from the end of the table (the rows in front of
                            the pair's belong to the pair before it)
      batch_unclamped_high  batch up to 256: columns from 128 on are the next step's
      keep_positive_only    keep > 0
      keep_as_weight        the raw mask is handed on (contract64 weights the loss by it)
      steps_unclamped       steps past the table's run on through the memory behind it: the table again"""
    assert mistake is None or mistake in MISTAKES, mistake
    rows = len(d['keep'])
    table = d['slots'].astype(np.int64)
    steps = table.shape[0]
    B = max(int(d['B'] if batch is None else batch), 0)
    n = max(int(d['n_steps'] if n_steps is None else n_steps), 0)
    if mistake == 'steps_unclamped':
        table, n = np.concatenate([table, table]), min(n, 2 * steps)
    else:
        n = min(n, steps)
    if mistake == 'batch_unclamped_high':
        table, B = np.concatenate([table, np.roll(table, -1, axis=0)], axis=1), min(B, 256)
    else:
        B = min(B, 128)
    if mistake == 'slot_wraps':
        table = table % rows
    elif mistake == 'slot_unclamped_low':
        table = np.where(table < 0, rows - 1 - (-table - 1) % rows, np.minimum(table, rows - 1))
    else:
        table = np.clip(table, 0, rows - 1)
    keep = d['keep']
    if mistake == 'keep_positive_only':
        keep = (keep > 0).astype(np.float32)
    elif mistake != 'keep_as_weight':
        keep = (keep != 0).astype(np.float32)
    return dict(d, slots=table, keep=keep, n_steps=n, B=B)


def contract64(d, batch=None, n_steps=None, mistake=None, lr=D.LR):
    """the float64 run of a raw pair under the contract, or under one planted mistake (moments_carried: Adam's moments start from what the
    same pair's run left behind, as a workspace that is not zeroed would hand them on)"""
    c = contract_case(d, batch, n_steps, mistake)
    if mistake == 'keep_as_weight':
        return D.distill_explicit64(c, lr=lr, weight_by_keep=True)
    if mistake == 'moments_carried':
        _, m, v = D.distill_explicit64(c, lr=lr, return_moments=True)
        return D.distill_explicit64(c, lr=lr, moments=(m, v))
    return D.distill_explicit64(c, lr=lr)


# the case of B or C that notices each mistake: (how the raw pair is built, batch, n_steps: None = the pair's own; n_steps +1 = one past
# the table)
NAMED = {'slot_wraps': ('B1', slots_case, None, None), 'slot_unclamped_low': ('B1', slots_case, None, None),
         'batch_unclamped_high': ('B2', batch_case, 129, None), 'keep_positive_only': ('B5', keep_case, None, None),
         'keep_as_weight': ('B5', keep_case, None, None), 'moments_carried': ('C2', batch_case, None, None),
         'steps_unclamped': ('B4', steps_case, None, 25)}

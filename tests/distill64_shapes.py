"""Shared by tests/test_distill_general_host.py (CPU) and tests/test_gpu_distill_general.py (GPU): the contract of
serl_ga_distill_general -- serl_ga_distill's (tests/distill64.py), for every actor shape the TD3 learner takes -- as a grid of cases
over (hidden, layers) and the tolerance an f32 implementation must meet on it against the float64 run.  The float64 and float32
literal loops and the written-out loop with planted mistakes are distill64's own: they read the shape from the case.  A plain module
(not a conftest): nothing here is a fixture."""
import numpy as np
import distill64 as D


def net(H, L, S, A, act):
    """the actor_shapes dict of an (H, L) actor at any (S, A)"""
    return dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=0, incremental=False)


def param_count(H, L, S, A):
    return H * S + H + L * (H * H + 3 * H) + A * H + A


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# (H, L): the smallest everything; not a multiple of 8 or 16 (edges of the matrix-core blocks and of the 4 x 4 gradient tiles); the
# SERL10 / TD3 default; a multiple of 4 only, at the deepest; the widest and deepest (full tile rows, the largest workspace); the overlap
# with serl_ga_distill.
SHAPES = [(4, 1), (36, 2), (72, 3), (100, 4), (128, 4), (32, 3)]
DIMS = [(1, 1), (7, 3), (16, 4)]
BATCHES = [128, 127, 64, 3, 1]
KEEPS = ['all', 'half', 'mid', 'first']
ACTS = ['tanh', 'elu', 'relu']


def _grid():
    """five cases per (H, L): every minibatch size once, and (S, A), the keep mode and the activation walked round from a start that
    moves with the shape, so that every value of every axis meets every (H, L) and the pairings differ from shape to shape"""
    out = []
    for i, (H, L) in enumerate(SHAPES):
        for k, B in enumerate(BATCHES):
            S, A = DIMS[(i + k) % 3]
            out.append((H, L, S, A, ACTS[(2 * i + k) % 3], B, KEEPS[(i + 3 * k) % 4]))
    return out


#   (H, L, S, A, activation, B, keep)
CASES = _grid()


def case_id(c):
    H, L, S, A, act, B, keep = c
    return 'H%dL%d_S%dA%d_%s_B%d_%s' % (H, L, S, A, act, B, keep)


def make_case(c, seed=None):
    """distill64.make_case for an (H, L) actor: the same construction of buffer, targets, keep mask and minibatch table"""
    import actor_shapes as X
    H, L, S, A, act, B, keep_mode = c
    seed = (H * 257 + L * 61 + S * 131 + A * 17 + B * 7 + len(act) + len(keep_mode) * 3) if seed is None else seed
    rng = np.random.default_rng(seed)
    s = net(H, L, S, A, act)
    n_steps = int(rng.integers(24, 61))
    w = X.make_weights(s, 2, seed)
    P = param_count(H, L, S, A)
    empty = keep_mode in ('mid', 'first')
    pool = 300 if B == 128 else B                     # the rows the ordinary steps draw from
    rows = pool + (B if empty else 0)
    states = (rng.standard_normal((rows, S)) * rng.uniform(0.3, 2.0, S)).astype(np.float32)
    targets = X.forward64(s, w[1, :P], states).astype(np.float32)
    keep = np.ones(rows, np.float32)
    if keep_mode == 'half':
        keep[rng.permutation(rows)[:rows // 2]] = 0.0
    base = B if empty else 0
    if empty:
        keep[:B] = 0.0
    slots = np.zeros((n_steps, 128), np.int32)
    for k in range(n_steps):
        pick = rng.choice(pool, B, replace=False) if pool > B else rng.permutation(B)
        slots[k, :B] = base + pick
    if empty:
        slots[0 if keep_mode == 'first' else n_steps // 2, :B] = rng.permutation(B)
    return dict(s=s, row=w[0, :P].copy(), states=states, targets=targets, keep=keep, slots=slots, n_steps=n_steps, B=B)


# ---- the tolerance ------------------------------------------------------------------------------------------------------------------
# The form is distill64.tolerance: TOL_REL[activation] x (how far the float64 run moved the parameters) + TOL_ABS.  Calibrated as there,
# on the CPU and never on the kernel: distill64.distill32 (the literal loop in float32 torch) against distill64.distill64 over CASES and
# five more seeds of each (seeds 1000 .. 1004 of make_case), 180 runs (tests/test_distill_general_host.py asserts the grid itself):
#   * tanh: max |w32 - w64| / moved is 1e-5 .. 4e-5 in most runs (median 2.2e-5), worst 1.5e-4 (H100 L4, S1 A1, B 3) and 1.3e-4
#     (H128 L4, S16 A4, B 1): the saturated tanh output units distill64.py describes.  distill64's TOL_REL 2.5e-3 is 16 x the worst case:
#     it holds with more than its margin and is used as it is.
#   * ELU: median 2.1e-5, worst 1.0e-4 (H36 L2, S1 A1, B 64).  2.5e-3 is 24 x the worst case: used as it is.
#   * LeakyReLU: median 2.3e-5, and 4.9e-2 in one run (the grid case H100 L4, S16 A4, B 64) and 6.5e-3 in another (the grid case H128 L4,
#     S7 A3, B 3); the next is 7e-4.  The kinks of distill64.py again -- a hidden pre-activation within f32 rounding of zero takes the
#     other slope in one of the two runs -- and four LayerNorm layers of 100 units offer more of them than three of 32, with more layers
#     below to carry the difference on.  distill64's 6e-2 would leave a margin of 1.2 x, not its 4.3 x; the bound here is the same margin
#     over the new worst case: 4.3 x 4.9e-2 = 0.21.
# The planted mistakes of distill64.distill_explicit64 at (72, 3) and (128, 4): tests/test_distill_general_host.py.
# The kernel on the MI355X (tests/test_gpu_distill_general.py, CASES and the several-pairs launches, both dense flavours -- they give the
# same bits): worst 1.05e-4 x moved for tanh (H128 L4, S16 A4, B 1), 3.6e-5 for ELU (H100 L4, S7 A3, B 1), and for LeakyReLU 0.18 in the
# grid case H100 L4, S16 A4, B 64 -- the case where the float32 torch loop has its 4.9e-2: the kernel meets that run's kinks at places
# of its own and ends 86 % of the way to the bound -- and 6.9e-4 in the next (H128 L4, S7 A3, B 3).
TOL_REL = {'tanh': D.TOL_REL['tanh'], 'elu': D.TOL_REL['elu'], 'relu': 0.21}
TOL_ABS = D.TOL_ABS
MIN_MOVED = D.MIN_MOVED


def tolerance(act, moved):
    """bound on max |w_f32 - w_f64| over a pair's parameters after its Adam steps, given how far the float64 run moved them"""
    return TOL_REL[act] * moved + TOL_ABS

"""Shared by tests/test_distill_host.py (CPU) and tests/test_gpu_distill.py (GPU): the contract of serl_ga_distill -- Adam steps of
GeneticAgent.update_parameters (base/core/genetic_agent.py:22-59) on minibatches drawn beforehand, the critic's Q-filter replaced by a
given keep mask -- restated in float64, a grid of cases over the shapes the kernel accepts, and the tolerance an f32 implementation must
meet against the float64 run.  A plain module (not a conftest): nothing here is a fixture."""
import warnings
import numpy as np
import torch

LR = 1e-3
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8            # torch.optim.Adam's defaults (genetic_agent.py:16)


def net(S, A, act):
    """the actor_shapes dict of the SERL50 family (hidden 32, three hidden layers) at any (S, A)"""
    return dict(state_dim=S, action_dim=A, hidden=32, num_layers=3, activation=act, env_config=0, incremental=False)


def param_count(S, A):
    return 32 * S + 32 + 3 * (32 * 32 + 3 * 32) + A * 32 + A


# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# (S, A) of every env configuration -- att (7, 3), att_inc (10, 3), sym (2, 1), sym_inc (3, 1), full (13, 3), full_inc (16, 3) -- and
# the ABI's edges (1, 1) and (16, 4) (the largest training state: 162 880 B of LDS); every activation on six of them; minibatches of 128,
# 127, 64, 3 and 1 rows; keep masks: all kept, about half dropped, one step in the middle whose minibatch is all dropped (after Adam's
# moments exist), the first step all dropped.
#   (S, A, activation, B, keep)
CASES = [(7, 3, 'tanh', 128, 'all'), (7, 3, 'elu', 127, 'half'), (7, 3, 'relu', 64, 'mid'), (10, 3, 'elu', 128, 'half'),
         (10, 3, 'tanh', 3, 'first'), (2, 1, 'relu', 128, 'half'), (2, 1, 'tanh', 1, 'mid'), (3, 1, 'elu', 64, 'all'),
         (3, 1, 'relu', 3, 'half'), (13, 3, 'tanh', 127, 'mid'), (13, 3, 'relu', 1, 'all'), (13, 3, 'elu', 64, 'half'),
         (16, 3, 'elu', 128, 'first'), (16, 3, 'tanh', 64, 'half'), (1, 1, 'elu', 127, 'half'), (1, 1, 'relu', 128, 'all'),
         (1, 1, 'tanh', 3, 'all'), (16, 4, 'tanh', 128, 'half'), (16, 4, 'elu', 1, 'first'), (16, 4, 'relu', 127, 'mid'),
         (7, 3, 'relu', 1, 'mid'), (2, 1, 'elu', 3, 'mid')]


def case_id(c):
    S, A, act, B, keep = c
    return 'S%dA%d_%s_B%d_%s' % (S, A, act, B, keep)


def make_case(c, seed=None):
    """inputs of one pair: dict(s, row f32 [P] (the second parent), states f32 [rows, S], targets f32 [rows, A] (the other parent's
    actions), keep f32 [rows], slots int32 [n_steps, 128] (columns from B on unused), n_steps, B).
    Buffers of 128 rows and more are sampled without replacement from 300 rows, as random.sample does; a smaller buffer is taken whole in
    a new order every step, as distil_batch does when the child's buffer holds fewer than 128 rows.  'mid' / 'first': rows 0 .. B-1 are
    all dropped and form the minibatch of step n_steps // 2 / step 0; the other steps draw from the rows after them.  'half': half
    the rows, at random, are dropped."""
    import actor_shapes as X
    S, A, act, B, keep_mode = c
    seed = (S * 131 + A * 17 + B * 7 + len(act) + len(keep_mode) * 3) if seed is None else seed
    rng = np.random.default_rng(seed)
    s = net(S, A, act)
    n_steps = int(rng.integers(24, 61))
    w = X.make_weights(s, 2, seed)
    P = param_count(S, A)
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


def n_empty_steps(d):
    return sum(int(not d['keep'][d['slots'][k, :d['B']]].any()) for k in range(d['n_steps']))


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------
def distill_literal(s, row, states, targets, keep, slots, n_steps, B, lr=LR, dtype=torch.float64):
    """GeneticAgent.update_parameters, step by step, on the reference's Actor with torch.optim.Adam in `dtype`: the rows slots[step, :B]
    the keep mask keeps, loss = sum((out - target)^2) + mean(out^2), zero_grad, backward, step.  An all-dropped minibatch goes through
    the same lines: the loss is NaN (mean of nothing), every gradient zero, and Adam still steps (tests/test_distill_host.py).
    -> the trained parameters, float64 [P]"""
    import actor_shapes as X
    from serl_amd.actor import unpack_into
    with torch.random.fork_rng(devices=[]):
        m = X.actor_module(s, dtype)
    unpack_into(m, torch.from_numpy(np.asarray(row, np.float64)))
    opt = torch.optim.Adam(m.parameters(), lr)
    st, tg, kp = torch.from_numpy(states).to(dtype), torch.from_numpy(targets).to(dtype), torch.from_numpy(keep)
    for step in range(n_steps):
        idx = torch.from_numpy(slots[step, :B].astype(np.int64))
        idx = idx[kp[idx] != 0]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', UserWarning)          # std() and mean() of an empty minibatch
            out = m(st[idx])
            loss = torch.sum((out - tg[idx]) ** 2) + torch.mean(out ** 2)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).to(torch.float64).numpy()


def distill64(d, lr=LR):
    return distill_literal(d['s'], d['row'], d['states'], d['targets'], d['keep'], d['slots'], d['n_steps'], d['B'], lr)


def distill32(d, lr=LR):
    """the same literal loop in float32 torch: what an f32 implementation of the contract is calibrated on"""
    return distill_literal(d['s'], d['row'], d['states'], d['targets'], d['keep'], d['slots'], d['n_steps'], d['B'], lr, torch.float32)


# ---- the same loop written out, with switches for planted mistakes ------------------------------------------------------------------
MISTAKES = ('biased_std', 'leaky_slope_0.02', 'elu_grad_expm1', 'no_mean_term', 'mean_over_B', 'no_bias_correction', 'skip_empty_step')


class _EluGradExpm1(torch.autograd.Function):
    """ELU whose derivative is taken as exp(v) - 1 instead of exp(v) on the negative side"""

    @staticmethod
    def forward(ctx, v):
        ctx.save_for_backward(v)
        return torch.nn.functional.elu(v)

    @staticmethod
    def backward(ctx, g):
        v, = ctx.saved_tensors
        return g * torch.where(v > 0, torch.ones_like(v), torch.expm1(v))


def distill_explicit64(d, mistake=None, lr=LR, weight_by_keep=False, moments=None, return_moments=False):
    """distill64 with the forward pass, the loss and Adam written out in float64 (like distill._batched_forward), and at most one of
    MISTAKES planted.  With mistake=None it is the reference (tests/test_distill_host.py checks that).
    Two more mistakes, for tests/distill_general_edges.py, as arguments (the defaults are the contract): weight_by_keep -- a kept row's
    terms of the loss are multiplied by its keep value instead of counted once; moments = (m, v) -- Adam's moments start from these
    instead of zero.  return_moments: -> (parameters, m, v)."""
    assert mistake is None or mistake in MISTAKES, mistake
    s, B, n_steps = d['s'], d['B'], d['n_steps']
    S, A, H, L, actn = s['state_dim'], s['action_dim'], s['hidden'], s['num_layers'], s['activation']
    if actn == 'tanh':
        act = torch.tanh
    elif actn == 'elu':
        act = _EluGradExpm1.apply if mistake == 'elu_grad_expm1' else torch.nn.functional.elu
    else:
        slope = 0.02 if mistake == 'leaky_slope_0.02' else 0.01
        act = lambda v: torch.nn.functional.leaky_relu(v, slope)
    w = torch.from_numpy(np.asarray(d['row'], np.float64)).clone().requires_grad_(True)
    st, tg, kp = (torch.from_numpy(np.asarray(d[k], np.float64)) for k in ('states', 'targets', 'keep'))

    def forward(x):
        off = 0

        def take(*shape):
            nonlocal off
            n = int(np.prod(shape))
            v = w[off:off + n].view(shape)
            off += n
            return v
        W, b = take(H, S), take(H)
        h = act(x @ W.T + b)
        for _ in range(L):
            W, b, g, be = take(H, H), take(H), take(H), take(H)
            y = h @ W.T + b
            mean = y.mean(-1, keepdim=True)
            std = y.std(-1, keepdim=True, correction=0 if mistake == 'biased_std' else 1)
            h = act(g * (y - mean) / (std + 1e-6) + be)
        W, b = take(A, H), take(A)
        return torch.tanh(h @ W.T + b)

    m1, v1 = torch.zeros_like(w), torch.zeros_like(w)
    if moments is not None:
        m1, v1 = (torch.from_numpy(np.asarray(x, np.float64)).clone() for x in moments)
    t = 0
    for step in range(n_steps):
        idx = torch.from_numpy(d['slots'][step, :B].astype(np.int64))
        idx = idx[kp[idx] != 0]
        n = len(idx)
        if n == 0 and mistake == 'skip_empty_step':
            continue
        g = torch.zeros_like(w)                   # an all-dropped minibatch: no term reaches a weight
        if n:
            out = forward(st[idx])
            kw = kp[idx][:, None] if weight_by_keep else 1.0
            loss = torch.sum(kw * (out - tg[idx]) ** 2)
            if mistake != 'no_mean_term':
                loss = loss + torch.sum(kw * out ** 2) / ((B if mistake == 'mean_over_B' else n) * A)
            g, = torch.autograd.grad(loss, w)
        t += 1
        with torch.no_grad():
            m1 = BETA1 * m1 + (1 - BETA1) * g
            v1 = BETA2 * v1 + (1 - BETA2) * g * g
            if mistake == 'no_bias_correction':
                w -= lr * m1 / (v1.sqrt() + EPS)
            else:
                w -= lr / (1 - BETA1 ** t) * m1 / (v1.sqrt() / np.sqrt(1 - BETA2 ** t) + EPS)
    if return_moments:
        return w.detach().numpy(), m1.numpy(), v1.numpy()
    return w.detach().numpy()


# ---- the tolerance ------------------------------------------------------------------------------------------------------------------
# Adam divides every gradient by its own running magnitude, so an f32 implementation's deviation from the float64 run is best measured
# against how far the run moved the parameters (max |w - w0| over the pair).  Calibrated with distill32 -- the literal loop in float32
# torch -- against distill64 over CASES and five more seeds of each (tests/test_distill_host.py asserts the grid itself):
#   * tanh, ELU: max |w32 - w64| / moved is 1e-5 .. 5e-5 in all cases but one, 5.7e-4 (S2 A1 tanh, B 1): a tanh output unit saturated
#     to 1 - a^2 ~ 3e-7, whose f32 derivative carries a relative error of ~u / (1 - a^2), and Adam turns the ratio of such gradients
#     into steps of the order of lr whatever their size.  TOL_REL 2.5e-3 = 4.4 x that worst case.
#   * LeakyReLU: the same in 40 of 42 runs (worst 2e-4), and 6.2e-3 and 1.4e-2 in two (both S16 A4, B 127): a pre-activation of a hidden
#     unit within f32 rounding of zero took the other slope (1 against 0.01) in one of the two runs, and that sample's share of the unit's
#     gradient changed by 99 %.  Any f32 implementation meets such kinks at its own places.  TOL_REL 6e-2 = 4.3 x the worst case.
# The planted mistakes of tests/test_distill_host.py -- LayerNorm's biased std, a LeakyReLU slope of 0.02, the ELU derivative exp(v) - 1,
# no mean(out^2) term, that mean over B instead of the kept rows, Adam without bias correction, an all-dropped minibatch skipped -- reach
# deviations from 0.09 x moved (the mean over B) to 5 x moved (no bias correction): each exceeds its activation's bound by 18 x or more
# in some case.
# The kernel on the MI355X (tests/test_gpu_distill.py, CASES and the several-pairs launches): worst 1.4e-4 x moved for tanh (S2 A1, B 1),
# 2.9e-5 for ELU, 1.4e-2 for LeakyReLU -- the S16 A4 grid case, where it takes the other slope at the same kink as the float32 torch loop.
TOL_REL = {'tanh': 2.5e-3, 'elu': 2.5e-3, 'relu': 6e-2}
TOL_ABS = 1e-6
MIN_MOVED = 5e-3        # every case moves its parameters by more than this (no bound is met by a case that did not train)


def tolerance(act, moved):
    """bound on max |w_f32 - w_f64| over a pair's parameters after its Adam steps, given how far the float64 run moved them (max |w - w0|)"""
    return TOL_REL[act] * moved + TOL_ABS

"""Shared by tests/test_ga_sens_host.py (CPU) and tests/test_gpu_ga_sens.py (GPU): the contract of serl_ga_sensitivity_general (and of
serl_ga_sensitivity) -- the clamped output sensitivity of proximal_mutate / safe_mutate (base/core/mod_neuro_evo.py:188-217) -- restated in
float64 through autograd on ga._actor_forward_torch, the same contract written out by hand with switches for planted mistakes, a grid of
cases, three degenerate cases and the tolerance an f32 implementation must meet against the float64 run.  A plain module (not a
conftest): nothing here is a fixture."""
import functools
import numpy as np
import torch

EPS = 1e-6
CHUNK = 128             # samples per chunk of the general kernel: minibatches above it accumulate over chunks before anything is squared
POP = 3                 # rows of a case's population

# ---- the grid ---------------------------------------------------------------------------------------------------------------------
# A covering set: minibatches of 1, 3, 64, 65, 128, 129, 256, 512 rows (one and two wavefronts of samples and their edges, one chunk and
# its edge, two and four chunks); hidden 4, 32, 72, 128; 0, 1, 3, 4 hidden layers; (S, A) of the attitude task and the ABI's edges (1, 1),
# (16, 4); every activation at least three times; rows with a stride beyond their length (the columns behind the row hold NaN); members
# repeated and in descending order.  Hidden 128 x 3 (case 1) is the shape serl_ga_sensitivity refuses for LDS, 128 x 4 (case 4) likewise.
#   (S, A, H, L, activation, B, extra columns of the stride, members)
GRID = [(7, 3, 72, 3, 'tanh', 129, 0, (2, 1, 1, 0)), (7, 3, 128, 3, 'relu', 256, 5, (2, 0)),
        (1, 1, 4, 0, 'tanh', 1, 3, (0, 2, 0)), (16, 4, 32, 1, 'elu', 3, 0, (2, 1, 0)),
        (16, 4, 128, 4, 'elu', 512, 1, (1, 1)), (7, 3, 32, 3, 'relu', 64, 0, (0, 1, 2)),
        (1, 1, 72, 1, 'tanh', 65, 7, (2, 2, 0)), (7, 3, 4, 4, 'relu', 128, 0, (1, 0)),
        (16, 4, 72, 0, 'elu', 256, 2, (2, 1)), (7, 3, 128, 1, 'tanh', 3, 0, (1,))]
# Three degenerate cases, (name, grid-style tuple):
#   sd0        hidden layer 1 of member 1 has W = 0 and equal biases: its pre-LayerNorm values are all equal, sd == 0, the mask matters
#   wo0        Wo = 0 in member 1: every gradient but Wo's own is exactly 0, scaling == 1 there
#   small      the states scaled so that a visible share of the entries falls below the 0.01 clamp
DEGENERATE = [('sd0', (7, 3, 32, 3, 'tanh', 86, 0, (0, 1))), ('wo0', (7, 3, 72, 1, 'elu', 130, 0, (1, 0))),
              ('small', (7, 3, 32, 3, 'relu', 86, 0, (0, 1, 2)))]
SMALL_SHARE = 0.05      # 'small': at least this share of the float64 entries below 0.01 (and not 0)
MORE_SEEDS = (101, 202, 303)     # the tolerance is measured over the grid's own seeds and these

# ---- the tolerance ----------------------------------------------------------------------------------------------------------------
# err = |got - ref| / max(ref, 0.01) per element, ref the clamped float64 value.  TOL = 4 x the worst err of ga.sensitivity_torch in
# float32 on the CPU (the same sums in torch's order) over GRID with its own seeds and MORE_SEEDS: the project's usual
# margin for a different f32 summation order.  Left out of the comparison: elements whose float64 value before clamping lies within TOL
# (relative) of 0.01, and elements that are exactly 0 in one run and not in the other; at most EXCLUDED_CAP of a member's entries.
# measure_reference() prints what the constants below were taken from (python tests/sens64.py):
#   worst err of the float32 reference over GRID x (own seed, MORE_SEEDS): 2.055e-04 (S16A4_H128L4_elu_B512, seed 101) -> WORST_REF
#   (8 threads; torch's f32 sums depend on the thread count: 2.42e-04 was measured on a machine with more)
#   per case, the worst of the four seeds: 72x3 B129 1.2e-04, 128x3 B256 5.3e-05, 4x0 B1 4.9e-07, 32x1 B3 3.5e-05, 128x4 B512 2.1e-04,
#   32x3 B64 3.2e-05, 72x1 B65 3.8e-05, 4x4 B128 2.5e-05, 72x0 B256 1.5e-04, 128x1 B3 2.5e-05
#   the degenerate cases, which the bound is not taken from: sd0 6.5e-05, wo0 4.6e-04 (own seed; <= 4.9e-05 on the others), small 2.1e-05
#   worst excluded share of the float32 reference: 0.07 % in the grid (72x0 B256), 0.09 % in 'small'
WORST_REF = 2.055e-4
TOL = 4 * WORST_REF
EXCLUDED_CAP = 0.01


def case_id(c):
    if isinstance(c[0], str):
        return c[0]
    S, A, H, L, act, B, pad, members = c
    return 'S%dA%d_H%dL%d_%s_B%d' % (S, A, H, L, act, B)


def spec_of(c):
    import serl_amd
    S, A, H, L, act = c[:5]
    return serl_amd.NetSpec(S, A, H, L, act)


def make_case(c, seed=None):
    """inputs of one case: weights f32 [POP, P + pad] (the pad columns NaN), members, states f32 [n, B, S]; `c` a GRID tuple or a
    DEGENERATE (name, tuple) pair"""
    import actor_shapes as X
    name, c = (c if isinstance(c[0], str) else (None, c))
    S, A, H, L, act, B, pad, members = c
    seed = (S * 131 + A * 17 + H * 5 + L * 3 + B * 7 + len(act)) if seed is None else seed
    s = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=0, incremental=False)
    P = H * S + H + L * (H * H + 3 * H) + A * H + A
    w = np.full((POP, P + pad), np.nan, np.float32)
    w[:, :P] = X.make_weights(s, POP, seed)[:, :P]
    rng = np.random.default_rng(seed)
    st = (rng.standard_normal((len(members), B, S)) * rng.uniform(0.2, 2.0, S)).astype(np.float32)
    if name == 'sd0':
        off = H * S + H + 1 * (H * H + 3 * H)
        w[1, off:off + H * H] = 0.0
        w[1, off + H * H:off + H * H + H] = 0.375
    elif name == 'wo0':
        off = H * S + H + L * (H * H + 3 * H)
        w[1, off:off + A * H] = 0.0
    elif name == 'small':
        st *= np.float32(2e-3)
    return dict(name=name, S=S, A=A, H=H, L=L, act=act, B=B, P=P, members=list(members), weights=w, states=st)


def genome_size(S, A, H, L):
    return H * S + L * H * H + A * H


def clamp(raw):
    """mod_neuro_evo.py:215-217"""
    sc = np.array(raw, copy=True)
    sc[sc == 0] = 1.0
    sc[sc < 0.01] = 0.01
    return sc


# ---- the contract in float64: autograd on the project's own forward -----------------------------------------------------------------
def autograd64(spec, row, states):
    """-> the unclamped float64 sensitivity [G] of one member: the forward of ga._actor_forward_torch and, per output, autograd.grad of
    y[:, i].sum(); the squares summed, the root taken"""
    from serl_amd import ga
    row = torch.from_numpy(np.asarray(row[:spec.param_count], np.float64))
    x = torch.from_numpy(np.asarray(states, np.float64))
    shapes = [(spec.hidden, spec.state_dim)] + [(spec.hidden, spec.hidden)] * spec.num_layers + [(spec.action_dim, spec.hidden)]
    genome = [row[o:o + n].clone().view(shp).requires_grad_() for (o, n), shp in zip(spec.genome_segments(), shapes)]
    y = ga._actor_forward_torch(spec, row, genome, x)
    sq = torch.zeros(sum(n for _, n in spec.genome_segments()), dtype=torch.float64)
    for i in range(spec.action_dim):
        g = torch.autograd.grad(y[:, i].sum(), genome, retain_graph=i + 1 < spec.action_dim)
        sq += torch.cat([t.reshape(-1) for t in g]) ** 2
    return torch.sqrt(sq).numpy()


# ---- the contract written out by hand, with planted mistakes --------------------------------------------------------------------------
MISTAKES = ('biased_std', 'eps_inside', 'no_mask', 'square_of_sum', 'batch_mean', 'clamp_order', 'no_tanh_deriv', 'chunk_square')


def _act(v, act):
    if act == 'tanh':
        return np.tanh(v)
    if act == 'elu':
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    return np.where(v > 0, v, 0.01 * v)


def _dact(v, act):
    if act == 'tanh':
        return 1.0 - np.tanh(v) ** 2
    if act == 'elu':
        return np.where(v > 0, 1.0, np.exp(np.minimum(v, 0)))
    return np.where(v > 0, 1.0, 0.01)


def _unpack(c, row):
    S, A, H, L = c['S'], c['A'], c['H'], c['L']
    row = np.asarray(row[:c['P']], np.float64)
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        v = row[o:o + n].reshape(shape)
        o += n
        return v
    p = dict(W0=take(H, S), b0=take(H), layers=[])
    for _ in range(L):
        p['layers'].append((take(H, H), take(H), take(H), take(H)))
    p['Wo'], p['bo'] = take(A, H), take(A)
    return p


def _jacobians(c, p, x, mistake):
    """d sum_b out[b, i] / d genome for every output i over the rows x: [A, G]"""
    H, A, act = c['H'], c['A'], c['act'].lower()
    z0 = x @ p['W0'].T + p['b0']
    hs, tape = [_act(z0, act)], []
    for W, b, g, be in p['layers']:
        z = hs[-1] @ W.T + b
        cz = z - z.mean(-1, keepdims=True)
        var = (cz ** 2).sum(-1, keepdims=True) / (H if mistake == 'biased_std' else H - 1)
        sd = np.sqrt(var)
        D = np.sqrt(var + EPS) if mistake == 'eps_inside' else sd + EPS
        y = g * cz / D + be
        tape.append((cz, sd, D, y))
        hs.append(_act(y, act))
    out = np.tanh(hs[-1] @ p['Wo'].T + p['bo'])
    J = []
    for i in range(A):
        do = np.zeros_like(out)
        do[:, i] = 1.0 if mistake == 'no_tanh_deriv' else 1.0 - out[:, i] ** 2
        grads = [do.T @ hs[-1]]
        dh = do @ p['Wo']
        for l in range(len(p['layers']) - 1, -1, -1):
            W, b, g, be = p['layers'][l]
            cz, sd, D, y = tape[l]
            dn = dh * _dact(y, act) * g
            s2 = (dn * cz).sum(-1, keepdims=True)
            n1 = H if mistake == 'biased_std' else H - 1
            with np.errstate(divide='ignore', invalid='ignore'):
                if mistake == 'eps_inside':
                    k = s2 / (D * D * n1 * D)
                elif mistake == 'no_mask':
                    k = s2 / (D * D * n1 * sd)
                else:                       # torch's std_backward masks the term to 0 where sd == 0
                    k = np.where(sd > 0, s2 / (D * D * n1 * np.where(sd > 0, sd, 1.0)), 0.0)
            dz = (dn - dn.mean(-1, keepdims=True)) / D - cz * k
            grads.append(dz.T @ hs[l])
            dh = dz @ W
        dz0 = dh * _dact(z0, act)
        grads.append(dz0.T @ x)
        J.append(np.concatenate([gr.reshape(-1) for gr in grads[::-1]]))
    return np.stack(J)


def explicit64(c, row, states, mistake=None):
    """-> the CLAMPED float64 sensitivity [G] of one member, written out by hand; `mistake`: one of MISTAKES, or None"""
    assert mistake is None or mistake in MISTAKES
    p = _unpack(c, row)
    x = np.asarray(states, np.float64)
    B = x.shape[0]
    parts = [_jacobians(c, p, x[b0:b0 + CHUNK], mistake) for b0 in range(0, B, CHUNK)]
    J = sum(parts)                                           # [A, G], accumulated over the chunks
    if mistake == 'batch_mean':
        J = J / B
    if mistake == 'chunk_square':
        raw = np.sqrt(sum(Jc ** 2 for Jc in parts).sum(0))   # chunks squared before they are accumulated
    elif mistake == 'square_of_sum':
        raw = np.sqrt(J.sum(0) ** 2)                         # the square of the sum over the outputs
    else:
        raw = np.sqrt((J ** 2).sum(0))
    if mistake == 'clamp_order':
        sc = np.array(raw, copy=True)
        sc[sc < 0.01] = 0.01
        sc[sc == 0] = 1.0
        return sc
    return clamp(raw)


# ---- references, computed once and shared -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(key, seed=None):
    """(case, raw float64 [n, G]) of GRID[key] (an int) or the degenerate case `key` (a name); cached: callers must not write to it"""
    c = GRID[key] if isinstance(key, int) else next(d for d in DEGENERATE if d[0] == key)
    case = make_case(c, seed)
    spec = spec_of(c if isinstance(key, int) else c[1])
    raw = np.stack([autograd64(spec, case['weights'][m], case['states'][k]) for k, m in enumerate(case['members'])])
    raw.setflags(write=False)
    return case, raw


ALL_KEYS = list(range(len(GRID))) + [d[0] for d in DEGENERATE]


def key_id(key):
    return case_id(GRID[key]) if isinstance(key, int) else key


def compare(got, raw, tol=TOL):
    """one member: got f32 / f64 [G] clamped, raw float64 [G] unclamped -> (worst err over the compared elements, excluded share)"""
    got = np.asarray(got, np.float64)
    ref = clamp(raw)
    excluded = (np.abs(raw - 0.01) <= tol * 0.01) | ((raw == 0) != (got == 1.0))
    err = np.abs(got - ref) / np.maximum(ref, 0.01)
    err = np.where(np.isfinite(err), err, np.inf)
    return (float(err[~excluded].max()) if (~excluded).any() else 0.0), float(excluded.mean())


def torch32(key, seed=None):
    """ga.sensitivity_torch in float32 on the CPU for the case: f32 [n, G]"""
    from serl_amd import ga
    case, _ = reference(key, seed)
    c = GRID[key] if isinstance(key, int) else next(d for d in DEGENERATE if d[0] == key)[1]
    return ga.sensitivity_torch(torch.from_numpy(case['weights']), case['members'], spec_of(c), torch.from_numpy(case['states'])).numpy()


def measure_reference(verbose=True):
    """what TOL was taken from: -> (worst err of the float32 torch reference over GRID x (own seed, MORE_SEEDS), worst excluded share
    over ALL_KEYS x the same seeds); the degenerate cases are printed beside, the bound is the grid's"""
    worst, worst_at, share = 0.0, None, 0.0
    for key in ALL_KEYS:
        for seed in (None,) + MORE_SEEDS:
            got = torch32(key, seed)
            _, raw = reference(key, seed)
            res = [compare(got[k], raw[k]) for k in range(len(got))]
            e, x = max(r[0] for r in res), max(r[1] for r in res)
            share = max(share, x)
            if verbose:
                print('%-28s seed %-5s err %.3e excluded %.4f %%' % (key_id(key), seed, e, 100 * x))
            if isinstance(key, int) and e > worst:
                worst, worst_at = e, (key_id(key), seed)
    if verbose:
        print('grid: worst err %.3e at %s; 4 x = %.3e; worst excluded share (all cases) %.4f %%' % (worst, worst_at, 4 * worst, 100 * share))
    return worst, share


if __name__ == '__main__':
    measure_reference()

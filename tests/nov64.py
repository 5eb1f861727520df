"""Shared by tests/test_ga_nov_host.py (CPU) and tests/test_gpu_ga_nov.py (GPU): the contract of serl_ga_novelty_general (and of
serl_ga_novelty) -- Actor.get_novelty (base/core/genetic_agent.py:111-115), the mean over a batch of sum_a (action - actor(state))^2 --
in float64 through the project's own Actor module, a grid of cases, and the tolerance an f32 implementation must meet against the
float64 run.  A plain module (not a conftest): nothing here is a fixture."""
import functools
import numpy as np
import torch

POP = 3                       # rows of a case's population
MEMBERS = (2, 0, 2, 1)        # every case: four evaluations; member 2 is listed twice
CHUNK = 128                   # samples per chunk of the general kernel

# ---- the grid ---------------------------------------------------------------------------------------------------------------------
#   (S, A, H, L, activation, B): batches of 1, 2, 86, 127, 128, 129, 256, 512 rows (one sample, below / at / above one chunk, two and
#   four chunks), hidden 4 .. 128, 0 .. 4 hidden layers, the attitude task's (7, 3) and the ABI's edges (1, 1), (16, 4), every activation
GRID = [(7, 3, 4, 0, 'tanh', 1), (7, 3, 32, 3, 'tanh', 86), (7, 3, 72, 3, 'elu', 256), (7, 3, 96, 3, 'relu', 128),
        (7, 3, 128, 4, 'tanh', 129), (16, 4, 128, 3, 'elu', 512), (1, 1, 8, 1, 'relu', 127), (13, 3, 100, 2, 'tanh', 2)]
MORE_SEEDS = (101, 202, 303)  # the tolerance is measured over the grid's own seeds and these

# ---- the tolerance ----------------------------------------------------------------------------------------------------------------
# err = |got - ref| / ref per evaluation, ref the float64 value.  The actions are drawn uniform in (-1, 1) independently of the actor, so
# the differences are O(1), ref is O(1) and no case rests on cancellation.  TOL = 4 x the worst err of the f32 CPU path
# (ga._actor_forward_torch in float32, torch's sums) over GRID with its own seeds and MORE_SEEDS: the project's usual margin for a
# different f32 summation order (the rule of tests/sens64.py).  measure_reference() prints what the constant was taken from
# (python tests/nov64.py):
#   worst err of the float32 reference over GRID x (own seed, MORE_SEEDS): 1.864e-07 (S13A3_H100L2_tanh_B2, own seed) -> WORST_REF
#   (the same with 1 and with 8 threads); per case, the worst of the four seeds: 4x0 B1 1.8e-07, 32x3 B86 1.1e-07, 72x3 B256 7.5e-08,
#   96x3 B128 1.4e-07, 128x4 B129 1.2e-07, 128x3 B512 1.1e-07, 8x1 B127 1.2e-07, 100x2 B2 1.9e-07
# That is three f32 roundings (2^-24 = 6e-8 each): the bound holds an implementation to ~12 roundings of a value of order 1, whatever its
# summation order, and lies three orders of magnitude below what a wrong divisor, a dropped chunk or a shifted column move the value by.
WORST_REF = 1.864e-7
TOL = 4 * WORST_REF


def case_id(c):
    S, A, H, L, act, B = c
    return 'S%dA%d_H%dL%d_%s_B%d' % (S, A, H, L, act, B)


def shape_of(c):
    S, A, H, L, act = c[:5]
    return dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=0, incremental=False)


def spec_of(c):
    import serl_amd
    return serl_amd.NetSpec(*c[:5])


def make_case(c, seed=None):
    """inputs of one case: weights f32 [POP, stride], members, states f32 [n, B, S] (per-feature scales 0.2 .. 2), actions f32 [n, B, A]
    uniform in (-1, 1), drawn independently of the actor; evaluations 0 and 2 (the member listed twice) share one batch"""
    import actor_shapes as X
    S, A, H, L, act, B = c
    seed = (S * 131 + A * 17 + H * 5 + L * 3 + B * 7 + len(act)) if seed is None else seed
    w = X.make_weights(shape_of(c), POP, seed)
    rng = np.random.default_rng(seed)
    n = len(MEMBERS)
    st = (rng.standard_normal((n, B, S)) * rng.uniform(0.2, 2.0, S)).astype(np.float32)
    ac = rng.uniform(-1.0, 1.0, (n, B, A)).astype(np.float32)
    st[2], ac[2] = st[0], ac[0]             # the member listed twice is judged twice on the same batch
    return dict(c=c, S=S, A=A, H=H, L=L, act=act, B=B, P=H * S + H + L * (H * H + 3 * H) + A * H + A, members=list(MEMBERS), weights=w,
                states=st, actions=ac)


def novelty64(c, row, states, actions):
    """Actor.get_novelty of the project's Actor module in float64 on f32 inputs (cast exactly) -> python float"""
    import actor_shapes as X
    from serl_amd.actor import unpack_into
    m = X.actor_module(shape_of(c), torch.float64)
    unpack_into(m, torch.from_numpy(np.asarray(row, dtype=np.float64)))
    with torch.no_grad():
        return m.get_novelty((torch.from_numpy(np.asarray(states, np.float64)), torch.from_numpy(np.asarray(actions, np.float64)), None, None, None))


def novelty32_torch(c, row, states, actions):
    """the f32 CPU path: ga._actor_forward_torch in float32, torch's mean and sum"""
    from serl_amd import ga
    spec = spec_of(c)
    row = torch.from_numpy(np.asarray(row[:spec.param_count], np.float32))
    S, H, L, A = spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim
    shapes = [(H, S)] + [(H, H)] * L + [(A, H)]
    genome = [row[o:o + n].view(shp) for (o, n), shp in zip(spec.genome_segments(), shapes)]
    with torch.no_grad():
        y = ga._actor_forward_torch(spec, row, genome, torch.from_numpy(np.asarray(states, np.float32)))
        return float(torch.mean(torch.sum((torch.from_numpy(np.asarray(actions, np.float32)) - y) ** 2, dim=-1)).item())


def reference_of(case):
    """float64 novelty of every evaluation of a case -> f64 [n]"""
    return np.array([novelty64(case['c'], case['weights'][m], case['states'][k], case['actions'][k]) for k, m in enumerate(case['members'])])


@functools.lru_cache(maxsize=None)
def reference(key):
    """(case, float64 novelty [n]) of GRID[key], computed once per process and shared: treat both as read-only"""
    case = make_case(GRID[key])
    return case, reference_of(case)


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / ref


# ---- the ring layout, and the contract written out by hand with planted slips ---------------------------------------------------------
def ring_layout(case, extra=37, seed=9):
    """the case's batches stored in replay rings: per evaluation a ring f32 [B + extra, 2 S + A + 3] full of other transitions and a slot
    row int32 [B] (distinct slots in random order) such that ring[e][slots[e][b]] starts with (states[e][b], actions[e][b])"""
    S, A, B = case['S'], case['A'], case['B']
    n = len(case['members'])
    rng = np.random.default_rng(seed)
    rings = rng.uniform(-1.0, 1.0, (n, B + extra, 2 * S + A + 3)).astype(np.float32)
    slots = np.stack([rng.permutation(B + extra)[:B] for _ in range(n)]).astype(np.int32)
    for e in range(n):
        rings[e, slots[e], :S] = case['states'][e]
        rings[e, slots[e], S:S + A] = case['actions'][e]
    return rings, slots


SLIPS = ('mean_128', 'padded_counted', 'action_offset', 'neighbour_slots', 'square_of_sum', 'first_chunk_only')


def by_hand64(case, rings, slots, slip=None):
    """the kernel's steps in float64 over the ring layout: gather by slot, forward, per sample the sum over a of the squared difference,
    the sum over the samples, the division by the batch; `slip` plants one of SLIPS -> f64 [n]"""
    import actor_shapes as X
    assert slip is None or slip in SLIPS
    S, A, B = case['S'], case['A'], case['B']
    n = len(case['members'])
    out = np.zeros(n)
    for e, m in enumerate(case['members']):
        sl = slots[(e + 1) % n] if slip == 'neighbour_slots' else slots[e]
        rows = rings[e][sl].astype(np.float64)
        st, ac = rows[:, :S], rows[:, S + 1:S + 1 + A] if slip == 'action_offset' else rows[:, S:S + A]
        if slip == 'padded_counted':
            pad = -B % CHUNK
            st, ac = np.concatenate([st, np.zeros((pad, S))]), np.concatenate([ac, np.zeros((pad, A))])
        if slip == 'first_chunk_only':
            st, ac = st[:CHUNK], ac[:CHUNK]
        d = ac - X.forward64(shape_of(case['c']), case['weights'][m], st)
        per = d.sum(1) ** 2 if slip == 'square_of_sum' else (d ** 2).sum(1)
        out[e] = per.sum() / (CHUNK if slip == 'mean_128' else B)
    return out


def measure_reference():
    worst = (0.0, None)
    for key, c in enumerate(GRID):
        per = 0.0
        for seed in (None,) + MORE_SEEDS:
            case = make_case(c, seed)
            ref = reference_of(case)
            got = [novelty32_torch(c, case['weights'][m], case['states'][k], case['actions'][k]) for k, m in enumerate(case['members'])]
            e = float(rel_err(got, ref).max())
            per = max(per, e)
            if e > worst[0]:
                worst = (e, '%s, seed %s' % (case_id(c), 'own' if seed is None else seed))
        print('%-28s worst of four seeds %.3e   (float64 values %.3f .. %.3f)' % (case_id(c), per, ref.min(), ref.max()))
    print('worst err of the float32 reference over GRID x (own seed, MORE_SEEDS): %.3e (%s), %d threads' % (worst + (torch.get_num_threads(),)))


if __name__ == '__main__':
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    measure_reference()

"""SSNE weight-tensor edits (base/core/mod_neuro_evo.py) on a device-resident population tensor.

The population lives as one f32 tensor `weights[pop, P]` (packed rows, actor.NetSpec.param_layout).
Selection and every random draw stay on the host and consume the *same* RNG streams in the *same*
order as the reference (python `random`, `numpy.random`), so index decisions are identical; only the
tensor edits run as HIP kernels (C ABI `serl_ga_*`).

Reference quirks kept: `random.randint(0, n)` is inclusive, so the reference can index
one past the end (`:76,89,357-358`) and raise IndexError mid-operator; here such a draw is consumed
(RNG parity) and the edit skipped.
"""
import ctypes, math, random
import numpy as np
import torch
from . import _capi
from .actor import NetSpec


def _i32(dev, a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)


def _f32(dev, a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def clone(engine, weights, src, dst, spec: NetSpec):
    """weights[dst[i]] <- weights[src[i]]  (SSNE.clone, mod_neuro_evo.py:371-382; parameter part)."""
    src, dst = np.atleast_1d(src), np.atleast_1d(dst)
    s, d = _i32(weights.device, src), _i32(weights.device, dst)
    _capi.check(engine.lib.serl_ga_clone(engine.ctx, weights.data_ptr(), weights.stride(0), spec.param_count,
                                         s.data_ptr(), d.data_ptr(), len(src), _stream(weights.device)), 'serl_ga_clone')


def plan_crossover(spec: NetSpec, rng=random):
    """Draw the op list of crossover_inplace (mod_neuro_evo.py:61-93) -> int32 [n, 3] (offset, length, dir)
    dir 0: gene1 <- gene2, dir 1: gene2 <- gene1."""
    ops = []
    for name, off, shape in spec.param_layout():
        rows = shape[0]
        if len(shape) == 2:
            n = rng.randint(0, rows * 2)
            width = shape[1]
        else:
            n = rng.randint(0, rows)
            width = 1
        for _ in range(n):
            receiver = rng.random()
            ind = rng.randint(0, rows)
            if ind >= rows:
                continue          # the reference raises IndexError here
            ops.append((off + ind * width, width, 0 if receiver < 0.5 else 1))
    return np.asarray(ops, dtype=np.int32).reshape(-1, 3)


def crossover_inplace(engine, weights, member_a, member_b, spec: NetSpec, rng=random, ops=None):
    ops = plan_crossover(spec, rng) if ops is None else ops
    if len(ops):
        o = _i32(weights.device, ops)
        _capi.check(engine.lib.serl_ga_crossover(engine.ctx, weights.data_ptr(), weights.stride(0), int(member_a),
                                                 int(member_b), o.data_ptr(), len(ops), _stream(weights.device)),
                    'serl_ga_crossover')
    return ops


def plan_mutation(spec: NetSpec, mag, rng=random, nprng=np.random):
    """Draw the edit list of mutate_inplace (mod_neuro_evo.py:329-369) -> (idx, kind, z, strength)."""
    num_mutation_frac, super_mut_strength, super_mut_prob = 0.1, 10 * mag, 0.05
    reset_prob = super_mut_prob + 0.05
    layout = spec.param_layout()
    probs = nprng.uniform(0, 1, len(layout)) * 2
    idx, kind, z, strength = [], [], [], []
    for i, (name, off, shape) in enumerate(layout):
        if len(shape) != 2:
            continue
        num_weights = shape[0] * shape[1]
        if rng.random() < probs[i]:
            for _ in range(rng.randint(0, int(math.ceil(num_mutation_frac * num_weights)))):
                d1 = rng.randint(0, shape[0])
                d2 = rng.randint(0, shape[-1])
                r = rng.random()
                g = rng.gauss(0, 1.0)           # random.gauss(0, sigma) == sigma * this draw
                if d1 >= shape[0] or d2 >= shape[1]:
                    continue                    # the reference raises IndexError here
                idx.append(off + d1 * shape[1] + d2)
                if r < super_mut_prob:
                    kind.append(0); strength.append(super_mut_strength)
                elif r < reset_prob:
                    kind.append(1); strength.append(0.0)
                else:
                    kind.append(0); strength.append(mag)
                z.append(g)
    return (np.asarray(idx, np.int32), np.asarray(kind, np.int32), np.asarray(z, np.float32),
            np.asarray(strength, np.float32))


def mutate_inplace(engine, weights, member, spec: NetSpec, mag, rng=random, nprng=np.random, plan=None):
    idx, kind, z, strength = plan_mutation(spec, mag, rng, nprng) if plan is None else plan
    if len(idx):
        dev = weights.device
        a, b, c, d = _i32(dev, idx), _i32(dev, kind), _f32(dev, z), _f32(dev, strength)
        _capi.check(engine.lib.serl_ga_mutate(engine.ctx, weights.data_ptr(), weights.stride(0), int(member),
                                              a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), len(idx),
                                              _stream(dev)), 'serl_ga_mutate')
    return idx, kind, z, strength


def scaled_perturb(engine, weights, member, spec: NetSpec, delta, scaling):
    """theta <- theta + delta / scaling over the 2-D-weights genome (proximal_mutate / safe_mutate update,
    mod_neuro_evo.py:183-223, 254-298; the Jacobian-based `scaling` comes from torch.autograd)."""
    segs = spec.genome_segments()
    dev = weights.device
    so, sl = _i32(dev, [s[0] for s in segs]), _i32(dev, [s[1] for s in segs])
    dl = torch.as_tensor(delta, dtype=torch.float32).to(dev).contiguous()
    sc = torch.as_tensor(scaling, dtype=torch.float32).to(dev).contiguous()
    assert dl.numel() == sc.numel() == sum(s[1] for s in segs)
    _capi.check(engine.lib.serl_ga_scaled_perturb(engine.ctx, weights.data_ptr(), weights.stride(0), int(member),
                                                  so.data_ptr(), sl.data_ptr(), len(segs), dl.data_ptr(), sc.data_ptr(),
                                                  _stream(dev)), 'serl_ga_scaled_perturb')


# ---- operators that need the actor itself (kernels in csrc/serl_ga.hip) ----------------------------------------------------
def _net_args(spec: NetSpec):
    return (spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim, spec.activation_id)


def genome_size(spec: NetSpec):
    return sum(n for _, n in spec.genome_segments())


KERNELS = ('lds', 'general', 'auto')
DENSE = ('valu', 'mfma')


def check_choice(who, kernel, dense, entry, kernels=KERNELS):
    """a (kernel, dense) pair of sensitivity / novelty / distil_batch: `kernels` = (the kernel behind `entry`, which has no matrix-core phases,
    'general', 'auto')"""
    if kernel not in kernels:
        raise ValueError('%s: kernel must be one of %s, not %r' % (who, ', '.join(kernels), kernel))
    if dense not in DENSE:
        raise ValueError('%s: dense must be one of %s, not %r' % (who, ', '.join(DENSE), dense))
    if kernel == kernels[0] and dense != 'valu':
        raise ValueError('%s: dense=%r needs kernel=\'general\' or \'auto\' (%s has no matrix-core phases)' % (who, dense, entry))


def resolve(engine, spec: NetSpec, B, kernel, entry, fallback=False):
    """The one path a checked choice runs `spec` on at minibatches of B rows, asked of the library (serl_shape_query) before anything is
    launched -> 'lds' (`entry`) | 'general' (`entry`_general) | 'torch'; where none of them is to run, the library's own error.
    'general': that kernel.  'lds': `entry` where it takes the shape; refused for LDS (not for range), 'torch' with `fallback`.  'auto': as
    'lds', but a shape refused for LDS goes to the general kernel where that takes it, before `fallback` is considered."""
    if kernel == 'general':
        return 'general'
    v = _capi.shape_query(entry, spec, B, engine.ctx)
    if v.lds:
        if kernel == 'auto' and _capi.shape_query(entry + '_general', spec, B, engine.ctx).takes:
            return 'general'
        if fallback:
            return 'torch'
    v.check()
    return 'lds'


def _sens_workspace(engine, dev, spec: NetSpec, n, B):
    """the workspace of serl_ga_sensitivity_general, cached on the engine per (shape, n, batch) -- and per stream: two launches on two
    streams must not share one.  -> (tensor or None, bytes); 0 bytes: the library refuses the shape (the launch call says why)."""
    nbytes = int(engine.lib.serl_ga_sensitivity_general_work_bytes(n, spec.state_dim, spec.action_dim, spec.hidden, spec.num_layers, B))
    if nbytes <= 0:
        return None, 0
    cache = engine.__dict__.setdefault('_sens_work', {})
    key = (str(dev), torch.cuda.current_stream(dev).cuda_stream, spec.state_dim, spec.action_dim, spec.hidden, spec.num_layers, n, B)
    work = cache.get(key)
    if work is None:
        work = cache[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    return work, nbytes


def sensitivity(engine, weights, members, spec: NetSpec, states, fallback=True, kernel='lds', dense='valu'):
    """The clamped output sensitivity of proximal_mutate / safe_mutate (mod_neuro_evo.py:188-217) for several members at
    once: states f32 [n, B, state_dim] (device) -> scaling f32 [n, G] (device).

    kernel  'lds' (default): serl_ga_sensitivity, which keeps one output's gradient of the whole genome in LDS; an actor whose genome
            does not fit there (H = 128 with three hidden layers: ~208 KB) is refused with SERL_E_UNSUPPORTED and, with `fallback`,
            computed by sensitivity_torch instead (the policy of serl_ga_distill).
            'general': serl_ga_sensitivity_general, batch-parallel, for every shape the TD3 learner takes (hidden a multiple of 4 in
            4 .. 128, 0 .. 4 hidden layers, S <= 16, A <= 4, B <= 512); it is that kernel or a RuntimeError with the library's message,
            never PyTorch: `fallback` does not apply to it.
            'auto': 'lds' where it runs, 'general' where 'lds' is refused for LDS (the rule of distil_kernel='auto').
    dense   the dense phases of the general kernel: 'valu' or 'mfma' (the f32 matrix cores; the same bits).  'mfma' with 'lds' is a
            ValueError: that kernel has no such phases."""
    check_choice('sensitivity', kernel, dense, 'serl_ga_sensitivity')
    dev = weights.device
    members = np.atleast_1d(np.asarray(members, dtype=np.int32))
    states = torch.as_tensor(states, dtype=torch.float32).to(dev).contiguous()
    n, B = states.shape[0], states.shape[1]
    assert n == len(members) and states.shape[2] == spec.state_dim
    G = genome_size(spec)
    if B == 0 or n == 0:  # empty buffer: every gradient is zero -> scaling[scaling == 0] = 1; no members: nothing to ask or to launch
        return torch.ones(n, G, dtype=torch.float32, device=dev)
    path = resolve(engine, spec, B, kernel, 'serl_ga_sensitivity', fallback)
    if path == 'torch':
        return sensitivity_torch(weights, members, spec, states)
    out = torch.empty(n, G, dtype=torch.float32, device=dev)
    m = _i32(dev, members)
    if path == 'lds':
        _capi.check(engine.lib.serl_ga_sensitivity(engine.ctx, weights.data_ptr(), weights.stride(0), *_net_args(spec), m.data_ptr(), n,
                                                   states.data_ptr(), B, out.data_ptr(), _stream(dev)), 'serl_ga_sensitivity')
        return out
    work, nbytes = _sens_workspace(engine, dev, spec, n, B)
    _capi.check(engine.lib.serl_ga_sensitivity_general(engine.ctx, weights.data_ptr(), weights.stride(0), *_net_args(spec), m.data_ptr(), n,
                                                       states.data_ptr(), B, out.data_ptr(), work.data_ptr() if work is not None else None,
                                                       nbytes, int(dense == 'mfma'), _stream(dev)), 'serl_ga_sensitivity_general')
    return out


def _actor_forward_torch(spec: NetSpec, row, genome, x):
    """Actor.forward (genetic_agent.py:104; LayerNorm mod_utils.py:47-50: unbiased std, eps on the std) over a packed row whose 2-D
    weights are the tensors `genome` (W0, W1 .. WL, Wo)"""
    S, H, L, A = spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim
    act = {'tanh': torch.tanh, 'elu': torch.nn.functional.elu,
           'relu': lambda v: torch.nn.functional.leaky_relu(v, 0.01)}[spec.activation.lower()]
    off = H * S
    h = act(x @ genome[0].t() + row[off:off + H])
    off += H
    for l in range(L):
        off += H * H
        b, g, be = row[off:off + H], row[off + H:off + 2 * H], row[off + 2 * H:off + 3 * H]
        z = h @ genome[1 + l].t() + b
        h = act(g * (z - z.mean(-1, keepdim=True)) / (z.std(-1, keepdim=True) + 1e-6) + be)
        off += 3 * H
    off += A * H
    return torch.tanh(h @ genome[-1].t() + row[off:off + A])


def sensitivity_torch(weights, members, spec: NetSpec, states):
    """sensitivity() in PyTorch autograd (f32, on the weights' device), for the shapes the kernel has no room for: per member and action
    the gradient of sum_b out[b, i] with respect to the 2-D weights, scaling = sqrt(sum_i grad_i^2) with the clamps of
    mod_neuro_evo.py:213-217.  torch's std backward masks the term of a LayerNorm whose inputs are all equal, as the reference's does."""
    states = torch.as_tensor(states, dtype=torch.float32).to(weights.device)
    out = []
    for k, member in enumerate(np.atleast_1d(members)):
        row = weights[int(member)].detach()
        shapes = [(spec.hidden, spec.state_dim)] + [(spec.hidden, spec.hidden)] * spec.num_layers + [(spec.action_dim, spec.hidden)]
        genome = [row[o:o + n].clone().view(shp).requires_grad_() for (o, n), shp in zip(spec.genome_segments(), shapes)]
        y = _actor_forward_torch(spec, row, genome, states[k])
        sq = torch.zeros(sum(n for _, n in spec.genome_segments()), dtype=torch.float32, device=weights.device)
        for i in range(spec.action_dim):
            g = torch.autograd.grad(y[:, i].sum(), genome, retain_graph=i + 1 < spec.action_dim)
            sq += torch.cat([t.reshape(-1) for t in g]) ** 2
        sc = torch.sqrt(sq)
        sc[sc == 0] = 1.0
        sc[sc < 0.01] = 0.01
        out.append(sc)
    return torch.stack(out)


def draw_delta(spec: NetSpec, mag):
    """the initial perturbation of mod_neuro_evo.py:195-197, drawn from torch's global CPU generator like the reference
    (whose `params` live on the CPU): Normal(zeros(G), ones(G) * mag).sample()"""
    import torch.distributions as dist
    G = genome_size(spec)
    return dist.Normal(torch.zeros(G), torch.ones(G) * mag).sample()


def proximal_mutate(engine, weights, member, spec: NetSpec, mag, buffer, batch_size, rng=random, delta=None, kernel='lds', dense='valu'):
    """SSNE.proximal_mutate (mod_neuro_evo.py:183-223) on the device-resident population: the batch is what the
    reference's `gene.buffer.sample(min(mutation_batch_size, len(buffer)))` picks (same python `random` draws), the
    sensitivity comes from serl_ga_sensitivity, delta from torch's generator, the update is serl_ga_scaled_perturb.
    `buffer` is a replay.DeviceReplay.  safe_mutate (:254-298) is the same operator fed from the critical buffer.  kernel / dense:
    sensitivity()'s, checked before any draw."""
    check_choice('proximal_mutate', kernel, dense, 'serl_ga_sensitivity')
    states = buffer.sample(min(int(batch_size), len(buffer)), rng)[0]
    scaling = sensitivity(engine, weights, [int(member)], spec, states[None], kernel=kernel, dense=dense)[0]
    delta = draw_delta(spec, mag) if delta is None else delta
    scaled_perturb(engine, weights, int(member), spec, delta, scaling)
    return scaling


class ProximalBatch:
    """Several proximal / safe mutations of one epoch applied together: `add` makes a member's host draws right away, in the
    reference's order (its minibatch from python `random`, its delta from torch's generator); `apply` computes all
    sensitivities in ONE serl_ga_sensitivity launch per batch size (one workgroup per member, side by side instead of one
    after the other) and perturbs the rows.  A mutation only reads and writes its own member.  kernel / dense: sensitivity()'s
    (one launch per batch size whichever kernel runs)."""

    def __init__(self, engine, weights, spec: NetSpec, mag, batch_size, rng=random, kernel='lds', dense='valu'):
        check_choice('ProximalBatch', kernel, dense, 'serl_ga_sensitivity')
        self.engine, self.weights, self.spec, self.mag, self.batch_size, self.rng = engine, weights, spec, mag, int(batch_size), rng
        self.kernel, self.dense = kernel, dense
        self.items = []

    def add(self, member, buffer, critical_buffer=None):
        src = buffer
        if critical_buffer is not None and len(critical_buffer) > 1:           # safe_mutate, mod_neuro_evo.py:258-261
            src = critical_buffer
        states = src.sample(min(self.batch_size, len(src)), self.rng)[0]
        self.items.append((int(member), states, draw_delta(self.spec, self.mag)))

    def apply(self):
        if not self.items:
            return
        dev = self.weights.device
        by_size = {}
        for k, (_, st, _) in enumerate(self.items):
            by_size.setdefault(st.shape[0], []).append(k)
        scal = [None] * len(self.items)
        for B, ks in by_size.items():
            sc = sensitivity(self.engine, self.weights, [self.items[k][0] for k in ks], self.spec, torch.stack([self.items[k][1] for k in ks]),
                             kernel=self.kernel, dense=self.dense)
            for j, k in enumerate(ks):
                scal[k] = sc[j]
        deltas = torch.stack([d for _, _, d in self.items]).to(dev)
        segs = self.spec.genome_segments()
        so, sl = _i32(dev, [s_[0] for s_ in segs]), _i32(dev, [s_[1] for s_ in segs])
        for k, (member, _, _) in enumerate(self.items):
            _capi.check(self.engine.lib.serl_ga_scaled_perturb(self.engine.ctx, self.weights.data_ptr(), self.weights.stride(0), member,
                                                               so.data_ptr(), sl.data_ptr(), len(segs), deltas[k].data_ptr(),
                                                               scal[k].contiguous().data_ptr(), _stream(dev)), 'serl_ga_scaled_perturb')
        self.items = []


def safe_mutate(engine, weights, member, spec: NetSpec, mag, buffer, critical_buffer, batch_size, rng=random, delta=None, kernel='lds',
                dense='valu'):
    src = critical_buffer if len(critical_buffer) > 1 else buffer          # mod_neuro_evo.py:258-261
    return proximal_mutate(engine, weights, member, spec, mag, src, batch_size, rng, delta, kernel, dense)


def _check_members(who, weights, members):
    members = np.atleast_1d(np.asarray(members, dtype=np.int32))
    if members.size and (members.min() < 0 or members.max() >= weights.shape[0]):
        raise ValueError('%s: a member outside the population of %d rows' % (who, weights.shape[0]))
    return members


def _novelty_general(engine, weights, members, spec: NetSpec, state_ptr, state_stride, action_ptr, action_stride, slots, n_rows, batch,
                     max_batch, dense):
    """one launch of serl_ga_novelty_general: every table (host arrays; slots int32 [n, max_batch] or None) goes up in ONE int64 upload
    -- pointers | members, n_rows, batch and the slot rows packed two int32 to a word -- and nothing comes back.  -> f32 [n] (device)"""
    dev = weights.device
    n = len(members)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    i32s = [np.asarray(members, np.int32), np.asarray(n_rows, np.int32), np.asarray(batch, np.int32)]
    if slots is not None:
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        assert slots.shape == (n, max_batch)
        i32s.append(slots.reshape(-1))
    ints = np.concatenate(i32s)
    if ints.size % 2:
        ints = np.concatenate([ints, np.zeros(1, np.int32)])
    host = np.concatenate([np.asarray(state_ptr, np.int64), np.asarray(action_ptr, np.int64), ints.view(np.int64)])
    tab = torch.from_numpy(host).to(dev)
    base = tab.data_ptr()
    p_state, p_action, p_int = base, base + 8 * n, base + 16 * n
    _capi.check(engine.lib.serl_ga_novelty_general(engine.ctx, weights.data_ptr(), weights.stride(0), *_net_args(spec), p_int, n,
                                                   p_state, int(state_stride), p_action, int(action_stride),
                                                   p_int + 12 * n if slots is not None else None, p_int + 4 * n, p_int + 8 * n,
                                                   int(max_batch), out.data_ptr(), int(dense == 'mfma'), _stream(dev)),
                'serl_ga_novelty_general')
    return out          # (tab is freed to torch's allocator, which hands it out again only behind this launch on its stream)


def novelty(engine, weights, members, spec: NetSpec, states, actions, kernel='lds', dense='valu'):
    """Actor.get_novelty (genetic_agent.py:111-115) for n (actor, batch) pairs: states [n, B, S], actions [n, B, A]
    -> f32 [n] (device)

    kernel  'lds' (default): serl_ga_novelty, one sample at a time, the shapes of its contract (csrc/serl_shapes.h) that fit the LDS.
            'general': serl_ga_novelty_general, batch-parallel, for every shape the TD3 learner takes (hidden a multiple of 4 in 4 .. 128,
            0 .. 4 hidden layers, S <= 16, A <= 4, B <= 512); it is that kernel or a RuntimeError with the library's message, never
            another path.
            'auto': 'lds' where it runs, 'general' where 'lds' is refused for LDS and the general kernel takes the shape.
    dense   the dense phase of the general kernel: 'valu' or 'mfma' (the f32 matrix cores; the same bits).  'mfma' with 'lds' is a
            ValueError: that kernel has no such phase."""
    check_choice('novelty', kernel, dense, 'serl_ga_novelty')
    dev = weights.device
    members = np.atleast_1d(np.asarray(members, dtype=np.int32))
    states = torch.as_tensor(states, dtype=torch.float32).to(dev).contiguous()
    actions = torch.as_tensor(actions, dtype=torch.float32).to(dev).contiguous()
    n, B = states.shape[0], states.shape[1]
    if n == 0 and B > 0:          # no evaluations: what every kernel returns for them, whatever the shape
        return torch.empty(0, dtype=torch.float32, device=dev)
    if resolve(engine, spec, B, kernel, 'serl_ga_novelty') == 'lds':
        out = torch.empty(n, dtype=torch.float32, device=dev)
        m = _i32(dev, members)
        _capi.check(engine.lib.serl_ga_novelty(engine.ctx, weights.data_ptr(), weights.stride(0), *_net_args(spec), m.data_ptr(), n,
                                               states.data_ptr(), actions.data_ptr(), B, out.data_ptr(), _stream(dev)), 'serl_ga_novelty')
        return out
    members = _check_members('novelty', weights, members)
    assert n == len(members) and states.shape[2] == spec.state_dim and actions.shape == (n, B, spec.action_dim)
    S, A = spec.state_dim, spec.action_dim
    sp = states.data_ptr() + 4 * B * S * np.arange(n, dtype=np.int64)
    ap = actions.data_ptr() + 4 * B * A * np.arange(n, dtype=np.int64)
    return _novelty_general(engine, weights, members, spec, sp, S, ap, A, None, np.full(n, B), np.full(n, B), B, dense)


def distance_plan(genomes, buffers, rng=random):
    """The host side of sort_groups_by_distance (mod_neuro_evo.py:426-445), pure: no GPU, no engine.  Every pair (i < j in list order)
    of `genomes` is two evaluations -- gene1 judged on a batch of gene2's buffer, gene2 on one of gene1's -- with batches of
    min(256, len(buffer1), len(buffer2)) picked from the latest 1000 tuples of a buffer: `ring.sample_from_latest(bs, 1000, rng)` of
    gene1's buffer, then of gene2's, pair after pair -- the same python `random` draws in the reference's order (latest_slots(1000)
    once per ring, runs of calls with the same (len(latest), batch) replayed in bulk by replay.sample_many).
    -> dict: pairs   [(second, first, bs)]
             members int32 [2 pairs]: evaluation 2 k is `first` on the batch of second's buffer, 2 k + 1 `second` on first's
             rings   the ring every evaluation reads (2 k: buffers[second], 2 k + 1: buffers[first])
             batch   int32 [2 pairs]
             slots   int32 [2 pairs, max batch]: PHYSICAL ring slots of the batch rows, in draw order; 0 from batch[e] on
             calls   [2 pairs]: the evaluation that gets the k-th sample_from_latest call of the reference's order"""
    from . import replay
    pairs, members, rings, calls = [], [], [], []
    for i, first in enumerate(genomes):
        for second in genomes[i + 1:]:
            b1, b2 = buffers[first], buffers[second]
            bs = min(256, min(len(b1), len(b2)))
            e = len(members)
            calls += [e + 1, e]                            # sample_from_latest(bs, 1000) of gene1's, then of gene2's buffer
            pairs.append((second, first, bs))
            members += [first, second]                     # gene1 judged on gene2's batch, gene2 on gene1's
            rings += [b2, b1]
    n = len(members)
    batch = np.asarray([pairs[e // 2][2] for e in range(n)], dtype=np.int32)
    slots = np.zeros((n, int(batch.max()) if n else 0), dtype=np.int32)
    # the draws, in the reference's order; runs of calls with the same (len(latest), batch) are replayed in bulk
    latest = {}
    for e in calls:
        if id(rings[e]) not in latest:
            latest[id(rings[e])] = rings[e].latest_slots(1000)
    k0 = 0
    while k0 < n:
        key = lambda k: (len(latest[id(rings[calls[k]])]), int(batch[calls[k]]))
        n0, bs0 = key(k0)
        k1 = k0
        while k1 < n and key(k1) == (n0, bs0):
            k1 += 1
        got = replay.sample_many(n0, bs0, k1 - k0, rng)
        for k in range(k0, k1):
            e = calls[k]
            slots[e, :bs0] = latest[id(rings[e])][got[k - k0].astype(np.int64)]
        k0 = k1
    return dict(pairs=pairs, members=np.asarray(members, dtype=np.int32), rings=rings, batch=batch, slots=slots, calls=calls)


def sort_groups_by_distance(engine, weights, genomes, buffers, spec: NetSpec, rng=random, kernel='lds', dense='valu'):
    """SSNE.sort_groups_by_distance (mod_neuro_evo.py:426-445): every pair (i < j in list order) of `genomes` keyed by
    get_distance = gene1.get_novelty(batch of gene2) + gene2.get_novelty(batch of gene1), batches of
    min(256, len(buffer1), len(buffer2)) from the latest 1000 tuples of each buffer (same python `random` draws, in the
    reference's order: distance_plan).  -> [(second, first, distance)] sorted descending.

    kernel  'lds' (default): the batches are gathered from the rings by torch, evaluation by evaluation, and go through serl_ga_novelty,
            one launch per distinct batch size.
            'general': the plan's tables go up in one transfer and serl_ga_novelty_general reads the rings itself -- ONE launch for all
            2 * pairs evaluations whatever their batch sizes, one read-back; a RuntimeError with the library's message where it refuses.
            'auto': 'lds' where serl_ga_novelty takes the actor, 'general' where that is refused for LDS.
    dense   novelty()'s.  A pair with an empty buffer is a ValueError before the launch with 'general' (and with 'auto' where it
            resolves to it)."""
    check_choice('sort_groups_by_distance', kernel, dense, 'serl_ga_novelty')
    plan = distance_plan(genomes, buffers, rng)
    pairs, members = plan['pairs'], plan['members']
    if not pairs:
        return []
    if kernel == 'auto':          # (at batch 1: the general kernel where serl_ga_novelty is refused for LDS and it takes the actor, else 'lds' and its errors)
        kernel = 'general' if (_capi.shape_query('serl_ga_novelty', spec, 1, engine.ctx).lds and
                               _capi.shape_query('serl_ga_novelty_general', spec, 1, engine.ctx).takes) else 'lds'
    if kernel == 'general':
        nov = _distance_general(engine, weights, plan, spec, dense)
    else:
        st, ac = [], []
        for ring, bs, sl in zip(plan['rings'], plan['batch'], plan['slots']):
            s, a, _, _, _ = ring.split(ring.rows[torch.from_numpy(sl[:bs].astype(np.int64)).to(ring.device)])
            st.append(s); ac.append(a)
        members = [int(m) for m in members]
        sizes = {p[2] for p in pairs}
        if len(sizes) == 1:
            nov = novelty(engine, weights, members, spec, torch.stack(st), torch.stack(ac)).cpu().numpy().astype(np.float64)
        else:               # buffers of different fill: one launch per batch size
            nov = np.zeros(len(members), dtype=np.float64)
            for bs in sizes:
                idx = [k for k in range(len(members)) if pairs[k // 2][2] == bs]
                nov[idx] = novelty(engine, weights, [members[k] for k in idx], spec, torch.stack([st[k] for k in idx]),
                                   torch.stack([ac[k] for k in idx])).cpu().numpy()
    groups = [(p[0], p[1], float(nov[2 * k]) + float(nov[2 * k + 1])) for k, p in enumerate(pairs)]   # two .item() floats added in f64
    return sorted(groups, key=lambda g: g[2], reverse=True)


def _distance_general(engine, weights, plan, spec: NetSpec, dense):
    """the 2 * pairs evaluations of a distance_plan in ONE serl_ga_novelty_general launch that reads the rings in place -> f64 [2 pairs]"""
    rings, batch = plan['rings'], plan['batch']
    S, A = spec.state_dim, spec.action_dim
    if int(batch.min()) < 1:
        k = int(np.argmin(batch)) // 2
        raise ValueError('sort_groups_by_distance: the pair (%d, %d) has an empty buffer: no batch to judge a distance on'
                         % (plan['pairs'][k][1], plan['pairs'][k][0]))
    members = _check_members('sort_groups_by_distance', weights, plan['members'])
    for ring in rings:
        if (ring.state_dim, ring.action_dim) != (S, A) or ring.rows.device != weights.device or not ring.rows.is_contiguous():
            raise ValueError('sort_groups_by_distance: a ring of state_dim %d, action_dim %d on %s does not hold transitions of this actor '
                             '(state_dim %d, action_dim %d on %s)' % (ring.state_dim, ring.action_dim, ring.rows.device, S, A, weights.device))
    W = 2 * S + A + 3
    sp = np.asarray([r.rows.data_ptr() for r in rings], dtype=np.int64)
    out = _novelty_general(engine, weights, members, spec, sp, W, sp + 4 * S, W, plan['slots'], [r.capacity for r in rings], batch,
                           int(batch.max()), dense)
    return out.cpu().numpy().astype(np.float64)

"""GPU tests of the SSNE operators that need the actor itself and of the device replay rings, against golden vectors from the
REFERENCE'S OWN mod_neuro_evo.py / genetic_agent.py / replay_memory.py (tests/golden/make_proximal_golden.py)."""
import random, types
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MAG, MBS = 0.0247682869654, 86


def _spec(tag):
    import serl_amd
    return serl_amd.NetSpec(7, 3, 32, 3, 'tanh') if tag == 'serl50' else serl_amd.NetSpec(7, 3, 96, 3, 'relu')


def _rings(engine, g, key):
    """buffer / critical buffer of a golden agent as device rings, filled in the reference's order"""
    from serl_amd.replay import DeviceReplay
    rows = torch.from_numpy(g['buf_' + key])
    buf, crit = DeviceReplay(10_000, engine.device, engine), DeviceReplay(10_000, engine.device, engine)
    buf.append_rows(rows)
    crit.append_rows(rows[torch.from_numpy(g['crit_' + key].astype(np.int64))])
    return buf, crit


def _genome(row, spec):
    return np.concatenate([row[o:o + n] for o, n in spec.genome_segments()])


@pytest.mark.parametrize('tag,idx,ops', [('serl50', 18, ('prox', 'safe')), ('serl50', 0, ('prox', 'safe')), ('td3', 0, ('prox',))])
def test_proximal_and_safe_mutation_vs_reference(engine, golden, tag, idx, ops):
    """SSNE.proximal_mutate / safe_mutate (mod_neuro_evo.py:183-223, 254-298): seeded python `random` (batch) and torch
    (perturbation) -> the genome the reference's own operator left.  Tolerance: the sensitivity is an f32 sum over 86 x 3
    backward passes in another order than autograd's (rtol 2e-5 on scaling); the update divides a N(0, 0.025) draw by a
    scaling >= 0.01, so the new weights agree to 2e-5 absolute / 2e-5 relative."""
    from serl_amd import ga
    g = golden('proximal')
    key = '%s_%d' % (tag, idx)
    spec = _spec(tag)
    w0 = golden('actors')[tag][[idx]]
    buf, crit = _rings(engine, g, key)
    for op in ops:
        seed = int(g['%s_seed_%s' % (op, key)])
        w = torch.from_numpy(np.ascontiguousarray(w0)).to(engine.device)
        if w.shape[1] % 4:
            w = torch.nn.functional.pad(w, (0, (-w.shape[1]) % 4)).contiguous()
        random.seed(seed); torch.manual_seed(seed)
        if op == 'prox':
            sc = ga.proximal_mutate(engine, w, 0, spec, MAG, buf, MBS)
        else:
            sc = ga.safe_mutate(engine, w, 0, spec, MAG, buf, crit, MBS)
        torch.cuda.synchronize()
        # the batch is the one the reference sampled
        random.seed(seed)
        src = buf if op == 'prox' else crit
        np.testing.assert_array_equal(np.asarray(src.sample_slots(MBS)), g['%s_pick_%s' % (op, key)])
        if '%s_scaling_%s' % (op, key) in g.files:
            np.testing.assert_allclose(sc.cpu().numpy(), g['%s_scaling_%s' % (op, key)], rtol=2e-5, atol=1e-7)
        got = _genome(w[0].cpu().numpy(), spec)
        want = g['%s_%s' % (op, key)]
        assert np.abs(want - _genome(w0[0], spec)).max() > 1e-3, 'the golden must have moved the weights'
        # (H = 96, LeakyReLU: 28 608 entries, longer sums and a kinked activation -- a handful of entries reach 4e-5)
        tol = 2e-5 if tag == 'serl50' else 1e-4
        np.testing.assert_allclose(got, want, rtol=tol, atol=tol)
        assert np.mean(np.abs(got - want) > 2e-5 * (1 + np.abs(want))) < 1e-3
        # biases / norms are not part of the genome and stay untouched
        mask = np.ones(spec.param_count, bool)
        for o, n in spec.genome_segments():
            mask[o:o + n] = False
        np.testing.assert_array_equal(w[0].cpu().numpy()[:spec.param_count][mask], w0[0][mask])


def test_sort_groups_by_distance_vs_reference(engine, golden):
    """SSNE.sort_groups_by_distance (mod_neuro_evo.py:411-445) over four shipped actors with reference-filled buffers:
    pairs, order and distances of the reference's own call under the same `random` seed."""
    from serl_amd import ga
    g = golden('proximal')
    spec = _spec('serl50')
    w = torch.from_numpy(golden('actors')['serl50'][[18, 0, 7, 33]]).to(engine.device)
    w = torch.nn.functional.pad(w, (0, (-w.shape[1]) % 4)).contiguous()
    bufs = [_rings(engine, g, 'serl50_%d' % i)[0] for i in (18, 0, 7, 33)]
    random.seed(int(g['dist_seed']))
    groups = ga.sort_groups_by_distance(engine, w, [0, 1, 2, 3], bufs, spec)
    want = g['dist_groups']
    assert [(a, b) for a, b, _ in groups] == [(int(a), int(b)) for a, b, _ in want]
    np.testing.assert_allclose([d for _, _, d in groups], want[:, 2], rtol=1e-5)


def test_replay_scatter_kernel(engine):
    """serl_replay_scatter: whole episodes appended to rings in step order, wrap-around, cost-flagged rows compacted, an
    episode longer than the ring leaves its tail -- against n sequential add() calls emulated in numpy."""
    from serl_amd.replay import DeviceReplay, scatter_episodes
    rs = np.random.RandomState(0)
    E, T = 5, 700
    staged = rs.randn(E, T, 20).astype(np.float32)
    staged[..., 19] = (rs.rand(E, T) < 0.3)
    lens = [700, 333, 1, 512, 64]
    dev = engine.device
    st = torch.from_numpy(staged).to(dev)
    shared, small = DeviceReplay(1500, dev, engine), DeviceReplay(300, dev, engine)
    own = [DeviceReplay(1000, dev, engine) for _ in range(E)]
    crit = [DeviceReplay(100, dev, engine) for _ in range(E)]

    def emulate(cap, rows_list, pos=0, size=0, mem=None):
        mem = np.zeros((cap, 20), np.float32) if mem is None else mem
        for rows in rows_list:
            for r in rows:
                mem[pos] = r; pos = (pos + 1) % cap; size = min(cap, size + 1)
        return mem, pos, size
    for rnd in range(2):          # second round: rings already partly filled / wrapped
        jobs = []
        for e in range(E):
            n = lens[e]
            nc = int(staged[e, :n, 19].sum())
            jobs += [(shared, e, n, False, n), (small, e, n, False, n), (own[e], e, n, False, n), (crit[e], e, n, True, nc)]
        scatter_episodes(engine, st, jobs)
        torch.cuda.synchronize()
    eps = [staged[e, :lens[e]] for e in range(E)]
    for ring, lists in [(shared, eps * 2), (small, eps * 2)] + [(own[e], [eps[e]] * 2) for e in range(E)] + \
                       [(crit[e], [eps[e][eps[e][:, 19] != 0]] * 2) for e in range(E)]:
        mem, pos, size = emulate(ring.capacity, lists)
        assert (ring.position, len(ring)) == (pos, size)
        np.testing.assert_array_equal(ring.rows.cpu().numpy()[:size], mem[:size])


class _Critic(torch.nn.Module):
    """stand-in for TD3's twin critic (base/core/td3.py:17-85): two small MLPs over (state, action)"""

    def __init__(self):
        super().__init__()
        self.q1 = torch.nn.Sequential(torch.nn.Linear(10, 32), torch.nn.ELU(), torch.nn.Linear(32, 1))
        self.q2 = torch.nn.Sequential(torch.nn.Linear(10, 32), torch.nn.ELU(), torch.nn.Linear(32, 1))

    def forward(self, s, a):
        x = torch.cat([s, a], -1)
        return self.q1(x), self.q2(x)


def test_default_config_epoch_runs_on_device(engine, golden):
    """The reference's default SSNE configuration (base/parameters.py:110-115: proximal mutation, distillation crossover,
    distance-sorted parent groups) on a device-resident population of 8 with reference-filled rings: the operator sequence
    is consistent, elites are copied bit for bit together with their rings, distilled children differ from both parents,
    everything stays finite."""
    from serl_amd import ssne
    g = golden('proximal')
    spec = _spec('serl50')
    n = 8
    w0 = golden('actors')['serl50'][:n].copy()
    w = torch.nn.functional.pad(torch.from_numpy(w0), (0, 1)).contiguous().to(engine.device)
    keys = ['serl50_18', 'serl50_0', 'serl50_7', 'serl50_33']
    rings = [_rings(engine, g, keys[i % 4]) for i in range(n)]
    bufs, crits = [r[0] for r in rings], [r[1] for r in rings]
    args = types.SimpleNamespace(pop_size=n, elite_fraction=0.25, mutation_prob=0.9, mutation_mag=MAG, mut_type='proximal',
                                 distil_crossover=True, distil_type='distance', crossover_prob=0.0, mutation_batch_size=MBS,
                                 individual_bs=2_000)
    torch.manual_seed(0)
    critic = _Critic().to(engine.device)
    fit = np.random.default_rng(2).normal(-150, 50, n)
    rec = []
    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    s = ssne.SSNE(args, engine, spec, critic=critic, record=rec)
    elite_slot = s.epoch(w, fit, buffers=bufs, critical=crits)
    torch.cuda.synchronize()
    out = w.cpu().numpy()[:, :spec.param_count]
    assert np.isfinite(out).all()
    kinds = [r[0] for r in rec]
    assert kinds.count(3) >= 1 and kinds.count(2) >= 1 and kinds[0] == 0
    best = int(np.argmax(fit))
    assert rec[0] == (0, best, elite_slot)
    mutated = {r[1] for r in rec if r[0] == 2}
    if elite_slot not in mutated:
        np.testing.assert_array_equal(out[elite_slot], w0[best])
    assert len(bufs[elite_slot]) == len(bufs[best])
    np.testing.assert_array_equal(bufs[elite_slot].rows[:50].cpu().numpy(), bufs[best].rows[:50].cpu().numpy())
    # a distilled child: cloned into an unselected slot right after its distillation
    k = kinds.index(3)
    first, second, slot = rec[k][1], rec[k][2], rec[k + 1][2]
    assert rec[k + 1][0] == 0 and rec[k + 1][1] == -1
    if slot not in mutated:
        assert np.abs(out[slot] - w0[second]).max() > 1e-4 and np.abs(out[slot] - w0[first]).max() > 1e-4
    assert len(bufs[slot]) == min(2000, 2 * min(1000, len(bufs[first])))
    assert len(crits[slot]) == 0


def test_smoothness_of_episodes_of_different_lengths(engine):
    """serl_smoothness (direct DFT, one launch for any set of lengths) against the FFT formulation of calc_smoothness
    (base/core/utils.py:82-120; metrics.calc_smoothness per distinct length) and against numpy's FFT on the host."""
    import numpy as np, torch
    from serl_amd import metrics
    rng = np.random.default_rng(3)
    lengths = np.array([1, 3, 4, 5, 6, 7, 64, 199, 200, 1001, 2001, 2001, 1503, 8001, 8000, 12], dtype=np.int64)
    T = 8001
    t = np.arange(T) * 0.01
    y = np.zeros((len(lengths), T, 3))
    for e in range(len(lengths)):
        for c in range(3):
            y[e, :, c] = 0.1 * np.sin(2 * np.pi * rng.uniform(0.1, 3.0) * t + rng.uniform(0, 6)) + 0.01 * rng.standard_normal(T)
    a = torch.from_numpy(y).to(engine.device)
    got = metrics.calc_smoothness(a, lengths).cpu().numpy()            # > 2 distinct lengths on the GPU: the DFT kernel
    want = np.zeros(len(lengths))
    for e, N in enumerate(lengths):
        if N < 4:
            continue
        Y = np.fft.fft(y[e, :N], axis=0)[1:N // 2]
        S = np.abs(Y * np.conj(Y)) * 0.01
        f = np.linspace(0.01, 50.0, N // 2 - 1)
        want[e] = -np.sqrt((S * f[:, None]).sum() * 2 / N) * 100 * (80 / (N * 0.01))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)
    fft = torch.stack([metrics.calc_smoothness(a[e:e + 1, :int(lengths[e])], None)[0] for e in range(len(lengths))]).cpu().numpy()   # full-length batches: the FFT path
    np.testing.assert_allclose(got, fft, rtol=1e-9, atol=1e-12)
    assert got[0] == 0.0 and got[1] == 0.0                         # fewer than four steps: no spectrum (metrics.calc_smoothness)


@pytest.mark.parametrize('name', ['d_18_0', 'd_7_33', 'd_0_18'])
def test_fused_distillation_vs_reference(engine, golden, name):
    """distill.distil_batch -- targets and Q-filter once per pair, all Adam steps in the serl_ga_distill kernel -- against the
    child the REFERENCE'S OWN SSNE.distilation_crossover produced (tests/golden/make_distill_golden.py): same buffer, same
    minibatches (the generator ends where the reference's ends), parameters to f32 rounding of 36 - 84 Adam steps."""
    import random
    from serl_amd import distill
    from test_ga_host import distill_case
    args, spec, w, bufs, critic, seed, g = distill_case(golden, name, engine.device, engine)
    random.seed(seed); torch.manual_seed(seed)
    (row, buf, crit), = distill.distil_batch(args, engine, spec, w, [(0, 1)], bufs, critic)
    after = random.random()
    np.testing.assert_array_equal(buf.rows[:len(buf), :7].cpu().numpy(), g[name + '_states'])
    child = row.cpu().numpy()[:spec.param_count]
    moved = np.abs(g[name + '_child'] - w[1].cpu().numpy()[:spec.param_count]).max()
    assert moved > 5e-3
    np.testing.assert_allclose(child, g[name + '_child'], rtol=0, atol=2e-4 * moved / 0.04 + 2e-5)
    # the sequential PyTorch path from the same seed leaves python's generator at the same place
    random.seed(seed); torch.manual_seed(seed)
    row2, _, _ = distill.distilation_crossover(args, engine, spec, w, 0, 1, bufs, critic)
    assert random.random() == after
    np.testing.assert_allclose(child, row2.cpu().numpy()[:spec.param_count], rtol=0, atol=2e-4)


def test_fused_distillation_of_several_pairs(engine, golden):
    """four pairs with buffers of different fill in one launch == the same pairs trained one by one in PyTorch"""
    import random
    from serl_amd import distill, replay
    from test_ga_host import distill_case
    args, spec, w2, bufs2, critic, seed, g = distill_case(golden, 'd_18_0', engine.device, engine)
    P, W = golden('proximal'), golden('actors')['serl50']
    ids = [18, 0, 7, 33]
    w = torch.from_numpy(W[ids]).to(engine.device)
    bufs = []
    for j, i in enumerate(ids):
        r = replay.DeviceReplay(10_000, engine.device, engine)
        r.append_rows(torch.from_numpy(P['buf_serl50_%d' % i][:1002 - 150 * j]))
        bufs.append(r)
    args.individual_bs = 1500
    pairs = [(0, 1), (2, 3), (1, 2), (3, 0)]
    random.seed(9); torch.manual_seed(9)
    kids = distill.distil_batch(args, engine, spec, w, pairs, bufs, critic)
    after = random.random()
    random.seed(9); torch.manual_seed(9)
    ref = [distill.distilation_crossover(args, engine, spec, w, f, s, bufs, critic) for f, s in pairs]
    assert random.random() == after
    for (row, buf, _), (row2, buf2, _), (f, s) in zip(kids, ref, pairs):
        assert len(buf) == len(buf2) == min(750, len(bufs[f])) + min(750, len(bufs[s]))
        np.testing.assert_array_equal(buf.rows[:len(buf)].cpu().numpy(), buf2.rows[:len(buf2)].cpu().numpy())
        a, b = row.cpu().numpy()[:spec.param_count], row2.cpu().numpy()[:spec.param_count]
        assert np.abs(a - w[s].cpu().numpy()[:spec.param_count]).max() > 5e-3
        np.testing.assert_allclose(a, b, rtol=0, atol=3e-4)


# ---- serl_ga_sensitivity / serl_ga_novelty against float64 autograd, across the shapes the kernels accept ----------------------------
def _net(S, A, H, L, act):
    return dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=0, incremental=False)


def _raw_sensitivity64(s, row, states):
    """the reference's own computation (mod_neuro_evo.py:198-214) in float64 on the reference's Actor: for every action i the gradient of
    sum_b out[b, i] w.r.t. the 2-D weights in genome order (extract_grad), then sqrt(sum_i g_i^2) -- before the clamps"""
    import actor_shapes as X
    from serl_amd.actor import unpack_into
    m = X.actor_module(s, torch.float64)
    unpack_into(m, torch.from_numpy(np.asarray(row, dtype=np.float64)))
    out = m(torch.from_numpy(np.asarray(states, dtype=np.float64)))
    sq = 0.0
    for i in range(s['action_dim']):
        m.zero_grad()
        go = torch.zeros_like(out)
        go[:, i] = 1.0
        out.backward(go, retain_graph=True)
        sq = sq + m.extract_grad() ** 2
    return torch.sqrt(sq).numpy()


def _clamped(raw):
    """mod_neuro_evo.py:215-217"""
    sc = raw.copy()
    sc[sc == 0] = 1.0
    sc[sc < 0.01] = 0.01
    return sc


def _novelty64(s, row, states, actions):
    import actor_shapes as X
    from serl_amd.actor import unpack_into
    m = X.actor_module(s, torch.float64)
    unpack_into(m, torch.from_numpy(np.asarray(row, dtype=np.float64)))
    with torch.no_grad():
        out = m(torch.from_numpy(np.asarray(states, dtype=np.float64))).numpy()
    return float(np.mean(np.sum((np.asarray(actions, np.float64) - out) ** 2, -1)))


# Tolerance of the sensitivity: every entry is an f32 sum over the batch of products of an f32 forward and backward pass, accumulated
# in another order than autograd's; entries whose terms cancel carry an absolute error of the order of the larger entries' rounding.
# |got - want| <= SENS_RTOL want + SENS_ATOL max(want of the same weight matrix): the f32 autograd path of serl_amd.ga (the same
# sums in torch's order) stays below 2e-5 relative / 3e-7 of the maximum on these shapes.  Entries whose unclamped value lies within
# 5 % of the 0.01 clamp are only checked to be clamped to no less than 0.01.  A wrong term in the LayerNorm backward moves entries by tens of percent.
SENS_RTOL, SENS_ATOL = 2e-4, 1e-5
NOV_RTOL = 1e-5          # novelty: a mean of B f32 sums of A squares, each difference to f32 rounding of the forward pass


def _check_sensitivity(got, raw, what, spec):
    want = _clamped(raw)
    near = np.abs(raw - 0.01) < 5e-4
    err = np.abs(got - want)
    scale = np.concatenate([np.full(n, want[o:o + n].max()) for o, n in _genome_offsets(spec)])      # per weight matrix
    bad = (err > SENS_RTOL * want + SENS_ATOL * scale) & ~near
    assert not bad.any(), '%s: %d entries off, worst at %d: got %r want %r (raw %r)' % (
        what, bad.sum(), np.argmax(np.where(bad, err, 0)), got[bad][:4], want[bad][:4], raw[bad][:4])
    np.testing.assert_array_equal(got[raw == 0], 1.0, err_msg=what + ': scaling == 0 -> 1')
    np.testing.assert_array_equal(got[(raw > 0) & (raw < 0.0095)], np.float32(0.01), err_msg=what + ': scaling < 0.01 -> 0.01')
    assert (got[near] >= np.float32(0.01)).all(), what


def _genome_offsets(spec):
    """(offset, length) of every 2-D weight inside the genome vector"""
    out, o = [], 0
    for _, n in spec.genome_segments():
        out.append((o, n)); o += n
    return out


# (S, A) of the attitude task, the symmetric / full configurations and full + incremental; hidden sizes below a wavefront, odd, one and
# more than one wavefront's worth of rows, the 256 the kernels' range ends at; batch sizes 1, 2, SSNE's 86 and 256.  (H = 2 only without
# hidden layers: a LayerNorm over two values is a sign function whose gradient is eps / sd^2, the difference of two ~1 / sd terms --
# pure f32 rounding in any implementation.)
SENS_CASES = [(7, 3, 2, 0, 'tanh', 86), (7, 3, 3, 3, 'elu', 2), (2, 1, 33, 3, 'relu', 86), (13, 3, 64, 1, 'tanh', 256),
              (16, 3, 65, 3, 'elu', 86), (7, 3, 100, 1, 'relu', 1), (7, 3, 128, 1, 'tanh', 86), (16, 3, 256, 0, 'relu', 86),
              (2, 1, 256, 0, 'elu', 256), (7, 3, 33, 0, 'tanh', 2), (13, 3, 100, 3, 'tanh', 86), (2, 1, 2, 0, 'relu', 1),
              (7, 3, 64, 3, 'elu', 256), (16, 3, 3, 1, 'tanh', 86)]


@pytest.mark.parametrize('S,A,H,L,act,B', SENS_CASES)
def test_sensitivity_and_novelty_vs_float64_autograd(engine, S, A, H, L, act, B):
    """serl_ga_sensitivity (the analytic backward pass through LayerNorm with the unbiased std) and serl_ga_novelty (Actor.get_novelty)
    for several members in one launch, repeats among them, against float64 autograd on the reference's Actor"""
    import actor_shapes as X
    from serl_amd import ga
    import serl_amd
    s = _net(S, A, H, L, act)
    spec = serl_amd.NetSpec(S, A, H, L, act)
    w = torch.from_numpy(X.make_weights(s, 3, 7 * H + L)).to(engine.device)
    members = [2, 0, 2, 1]
    rng = np.random.default_rng(H + 100 * L + B)
    st = (rng.standard_normal((len(members), B, S)) * rng.uniform(0.2, 2.0, S)).astype(np.float32)
    acts = rng.uniform(-1, 1, (len(members), B, A)).astype(np.float32)
    sc = ga.sensitivity(engine, w, members, spec, torch.from_numpy(st), fallback=False).cpu().numpy()
    nov = ga.novelty(engine, w, members, spec, torch.from_numpy(st), torch.from_numpy(acts)).cpu().numpy()
    wc = w.cpu().numpy()
    for k, m in enumerate(members):
        what = 'S%d A%d H%d L%d %s B%d member %d' % (S, A, H, L, act, B, m)
        _check_sensitivity(sc[k], _raw_sensitivity64(s, wc[m], st[k]), what, spec)
        np.testing.assert_allclose(nov[k], _novelty64(s, wc[m], st[k], acts[k]), rtol=NOV_RTOL, err_msg=what)


def test_sensitivity_edge_cases_vs_float64_autograd(engine):
    """a hidden layer whose pre-LayerNorm values are all equal (sd = 0: torch's std backward masks the term, the kernel's `sd > 0`
    branch), a state column that is zero in every batch row (its W0 entries have no gradient: exactly 1.0 by the `scaling == 0`
    rule), a column scaled so small that its W0 entries fall under the 0.01 clamp"""
    import actor_shapes as X
    from serl_amd import ga
    import serl_amd
    for H, L, layer, act in ((32, 3, 1, 'tanh'), (65, 1, 0, 'elu'), (100, 3, 2, 'relu'), (7, 3, 0, 'tanh')):
        S, A, B = 7, 3, 86
        s = _net(S, A, H, L, act)
        spec = serl_amd.NetSpec(S, A, H, L, act)
        w = X.make_weights(s, 2, 3 + H)
        off = H * S + H + layer * (H * H + 3 * H)         # hidden layer `layer`: W = 0, one bias for every row -> z constant, sd = 0
        w[1, off:off + H * H] = 0.0
        w[1, off + H * H:off + H * H + H] = 0.375
        rng = np.random.default_rng(H)
        st = rng.standard_normal((2, B, S)).astype(np.float32)
        st[:, :, 2] = 0.0                                 # a state column that is zero in every row
        st[:, :, 5] *= 1e-4                               # a column whose W0 entries fall under the clamp
        wt = torch.from_numpy(w).to(engine.device)
        sc = ga.sensitivity(engine, wt, [0, 1], spec, torch.from_numpy(st), fallback=False).cpu().numpy()
        assert np.isfinite(sc).all()
        for k in (0, 1):
            what = 'H%d L%d %s member %d' % (H, L, act, k)
            raw = _raw_sensitivity64(s, w[k], st[k])
            assert np.isfinite(raw).all()
            _check_sensitivity(sc[k], raw, what, spec)
            w0 = sc[k][:H * S].reshape(H, S)
            np.testing.assert_array_equal(w0[:, 2], 1.0, err_msg=what)
            if k == 0:
                assert (w0[:, 5] == np.float32(0.01)).mean() > 0.5, what
            else:                                         # nothing flows below a layer whose weights are zero
                np.testing.assert_array_equal(sc[k][:H * S + layer * H * H], 1.0, err_msg=what)
        g_off = H * S + layer * H * H                      # the degenerate layer's W in genome order: gradient through the masked std term
        assert (np.abs(_raw_sensitivity64(s, w[1], st[1])[g_off:g_off + H * H]) > 0.02).any()


def _prox_epoch_args(n):
    return types.SimpleNamespace(pop_size=n, elite_fraction=0.25, mutation_prob=0.9, mutation_mag=MAG, mut_type='proximal',
                                 distil_crossover=True, distil_type='distance', crossover_prob=0.0, mutation_batch_size=MBS,
                                 individual_bs=2_000)


def test_sensitivity_beyond_the_kernels_lds_vs_float64_autograd(engine, golden):
    """H = 128 with three hidden layers: the rollout accepts the actor, but one output's gradient of its genome (50 432 floats) and
    the forward buffers need ~208 KB of LDS -- serl_ga_sensitivity refuses the shape (SERL_E_UNSUPPORTED) and ga.sensitivity
    computes it in PyTorch.  Both paths against float64 autograd: the PyTorch path on that shape (mixed batch sizes through
    ProximalBatch, as an SSNE epoch applies them), the kernel's refusal itself."""
    import actor_shapes as X
    from serl_amd import ga, _capi
    import serl_amd
    for H, L, act in ((128, 3, 'tanh'), (124, 4, 'relu')):
        s = _net(7, 3, H, L, act)
        spec = serl_amd.NetSpec(7, 3, H, L, act)
        w = torch.from_numpy(X.make_weights(s, 3, 11)).to(engine.device)
        st = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 86, 7)).astype(np.float32))
        with pytest.raises(RuntimeError, match=r'serl_ga_sensitivity failed \(%d\)' % _capi.E_UNSUPPORTED):
            ga.sensitivity(engine, w, [0, 2], spec, st, fallback=False)
        sc = ga.sensitivity(engine, w, [0, 2], spec, st).cpu().numpy()
        for k, m in enumerate((0, 2)):
            _check_sensitivity(sc[k], _raw_sensitivity64(s, w[m].cpu().numpy(), st[k].numpy()), 'H%d L%d member %d' % (H, L, m), spec)
    # ProximalBatch with buffers of different fill (one sensitivity call per batch size): every row moved by delta / scaling
    from serl_amd.replay import DeviceReplay
    g = golden('proximal')
    spec = serl_amd.NetSpec(7, 3, 128, 3, 'tanh')
    w = torch.from_numpy(X.make_weights(_net(7, 3, 128, 3, 'tanh'), 3, 12)).to(engine.device)
    w0 = w.cpu().numpy().copy()
    rings = []
    for n_rows in (40, 200, 30):
        r = DeviceReplay(10_000, engine.device, engine)
        r.append_rows(torch.from_numpy(g['buf_serl50_18'][:n_rows]))
        rings.append(r)
    random.seed(4); torch.manual_seed(4)
    batch = ga.ProximalBatch(engine, w, spec, MAG, MBS)
    for m in (0, 1, 2):
        batch.add(m, rings[m])
    items = [(m, st.clone(), d.clone()) for m, st, d in batch.items]
    batch.apply()
    torch.cuda.synchronize()
    s = _net(7, 3, 128, 3, 'tanh')
    for m, st, delta in items:
        assert st.shape[0] == min(MBS, len(rings[m]))
        want = _clamped(_raw_sensitivity64(s, w0[m], st.cpu().numpy()))
        got = _genome(w[m].cpu().numpy(), spec) - _genome(w0[m], spec)
        np.testing.assert_allclose(got, delta.numpy() / want, rtol=1e-3, atol=2e-6, err_msg='member %d' % m)


def test_proximal_epoch_at_hidden_128_three_layers(engine, golden):
    """the default SSNE configuration (proximal mutation) on a population of H = 128, L = 3 actors -- a shape the rollout accepts and
    whose sensitivity does not fit the kernel's LDS: one epoch completes, mutates members, and leaves every weight finite"""
    import actor_shapes as X
    from serl_amd import ssne
    import serl_amd
    spec = serl_amd.NetSpec(7, 3, 128, 3, 'tanh')
    g = golden('proximal')
    n = 6
    w0 = X.make_weights(_net(7, 3, 128, 3, 'tanh'), n, 21)
    w = torch.from_numpy(w0.copy()).to(engine.device)
    keys = ['serl50_18', 'serl50_0', 'serl50_7']
    rings = [_rings(engine, g, keys[i % 3]) for i in range(n)]
    torch.manual_seed(0)
    critic = _Critic().to(engine.device)
    fit = np.random.default_rng(5).normal(-150, 50, n)
    rec = []
    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    s = ssne.SSNE(_prox_epoch_args(n), engine, spec, critic=critic, record=rec)
    s.epoch(w, fit, buffers=[r[0] for r in rings], critical=[r[1] for r in rings])
    torch.cuda.synchronize()
    out = w.cpu().numpy()
    assert np.isfinite(out).all()
    mutated = sorted({r[1] for r in rec if r[0] == 2})
    assert mutated, 'the epoch should mutate some member'
    for m in mutated:
        assert np.abs(out[m] - w0[m]).max() > 0, m

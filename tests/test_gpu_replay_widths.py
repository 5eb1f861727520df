"""GPU tests of the device replay rings at every row width: serl_replay_scatter_rows against n sequential add() calls emulated in numpy
(tests/replay_widths.py), against serl_replay_scatter at width 20, its refusals, a generation per env configuration with list-backed
buffers and with DeviceReplay rings of the configuration's dims, and one device SSNE epoch on the full-state configuration.  Everything
the scatter path produces is a copy: every comparison but the distilled child's is exact."""
import random, types
import numpy as np
import pytest
import torch
import actor_shapes as X
import distill64 as D
import replay_widths as RW

pytestmark = pytest.mark.gpu

LENS = [700, 333, 1, 512, 64, 0]          # a whole episode, a non-multiple of 256, one row, two tiles, a short one, none
T = 700


def _staged(S, A, device, src_offset, seed):
    """staged rows on the device, their first float `src_offset` floats behind a 16 B aligned address"""
    st = RW.make_staged(len(LENS), T, S, A, seed)
    store = torch.zeros(st.size + 4, dtype=torch.float32, device=device)
    assert store.data_ptr() % 16 == 0
    dev = store[src_offset:src_offset + st.size].view(st.shape)
    dev.copy_(torch.from_numpy(st))
    return st, dev, store


def _check(rings, what):
    for k, ring in enumerate(rings):
        assert ring.guards_intact(), '%s: ring %d written outside its rows' % (what, k)
        np.testing.assert_array_equal(ring.rows().view(np.uint32), ring.mem.view(np.uint32), err_msg='%s: ring %d' % (what, k))


# (ring offset, staged offset) in floats from a 16 B aligned address: with W % 4 == 0 the destination span of a job starts at residue
# `ring offset` mod 4 floats whatever the position is, so offsets 0 .. 3 visit every residue; with other W the positions the two rounds
# reach (position * W mod 4) visit them as well
OFFSETS = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 2), (2, 2), (0, 1)]


@pytest.mark.parametrize('offsets', OFFSETS, ids=lambda o: 'ring%d_src%d' % o)
@pytest.mark.parametrize('dims', RW.DIMS, ids=RW.dims_id)
def test_scatter_rows_equals_sequential_adds(engine, dims, offsets):
    """the job mix of test_gpu_ga.py::test_replay_scatter_kernel at every width: a shared ring, a ring shorter than one episode, own
    rings, cost_only rings; two rounds, the second on wrapped, partly filled rings.  The access width each case must take follows from
    W and the two base offsets (include/serl_amd.h) and is asserted here from the parametrisation, not observed."""
    S, A = dims
    W = RW.width(S, A)
    ring_off, src_off = offsets
    bytes_per_access = RW.access_width(W, ring_off, src_off)
    if W % 4 == 0 and ring_off % 4 == 0 and src_off % 4 == 0:
        assert bytes_per_access == 16
    elif W % 2 == 0 and ring_off % 2 == 0 and src_off % 2 == 0:
        assert bytes_per_access == 8
    else:
        assert bytes_per_access == 4
    st, dev, _keep = _staged(S, A, engine.device, src_off, seed=W)
    rings, items = RW.job_mix(st, LENS, engine.device, W, ring_off)
    starts = set()
    for rnd in range(2):
        jobs = RW.plan_launch(items)
        starts |= {(ring_off + j[2] * W + j[6] * W) % 4 for j in jobs if not j[5] and j[4] > j[6]}
        assert RW.launch(engine, dev, S, A, jobs) == 0
        _check(rings, '%s %s round %d' % (RW.dims_id(dims), offsets, rnd))
    assert any(r.pos != 0 and r.size == r.cap for r in rings) and any(0 < r.size < r.cap for r in rings)
    # destination spans started at these residues mod 4 floats: all four for odd W, both even / odd ones for W % 4 == 2
    want = {ring_off % 4} if W % 4 == 0 else ({ring_off % 2, ring_off % 2 + 2} if W % 2 == 0 else {0, 1, 2, 3})
    assert starts == want, (starts, want)
    np.testing.assert_array_equal(dev.cpu().numpy(), st)                      # the staged rows are read only


@pytest.mark.parametrize('dims', [(7, 3), (13, 3), RW.ODD_DIMS], ids=RW.dims_id)
def test_scatter_rows_edge_jobs(engine, dims):
    """n_jobs == 0, length == 0, skip == rows taken (plain and cost_only) are no-ops; a one-row ring keeps the last row; a cost_only job
    on an episode without a flagged row writes nothing; positions at every slot of a small ring"""
    S, A = dims
    W = RW.width(S, A)
    st, dev, _keep = _staged(S, A, engine.device, 0, seed=50 + W)
    st[4, :, W - 1] = 0.0
    dev.copy_(torch.from_numpy(st))
    ring = RW.Ring(9, W, engine.device)
    nc = int((st[0, :40, W - 1] != 0).sum())
    assert nc > 2
    noop = [(ring.ptr, 9, 3, 0, 0, 0, 0), (ring.ptr, 9, 3, 0, 40, 0, 40), (ring.ptr, 9, 3, 0, 40, 1, nc), (ring.ptr, 9, 3, 4, 64, 1, 0)]
    assert RW.launch(engine, dev, S, A, []) == 0
    assert RW.launch(engine, dev, S, A, noop) == 0
    _check([ring], 'no-op jobs')
    one = RW.Ring(1, W, engine.device)
    for p in range(9):                                   # one episode per launch, the ring at every position in turn
        ring.pos = p
        jobs = RW.plan_launch([(ring, 1, st[1, :5 + p], False), (one, 1, st[1, :5 + p], False)])
        assert RW.launch(engine, dev, S, A, jobs) == 0
        _check([ring, one], 'position %d' % p)
    np.testing.assert_array_equal(one.rows()[0], st[1, 12])


def test_width_20_through_both_entry_points(engine):
    """serl_replay_scatter_rows at S = 7, A = 3 leaves what serl_replay_scatter leaves on the same jobs"""
    S, A, W = 7, 3, 20
    st, dev, _keep = _staged(S, A, engine.device, 0, seed=7)
    rings_a, items_a = RW.job_mix(st, LENS, engine.device, W)
    rings_b, items_b = RW.job_mix(st, LENS, engine.device, W)
    for rnd in range(2):
        ja, jb = RW.plan_launch(items_a), RW.plan_launch(items_b)
        assert [j[1:] for j in ja] == [j[1:] for j in jb]
        assert RW.launch(engine, dev, S, A, ja, 'rows') == 0
        assert RW.launch(engine, dev, S, A, jb, 'attitude') == 0
        for a, b in zip(rings_a, rings_b):
            np.testing.assert_array_equal(a.rows().view(np.uint32), b.rows().view(np.uint32))
            assert a.guards_intact() and b.guards_intact()
    _check(rings_a, 'serl_replay_scatter_rows')
    _check(rings_b, 'serl_replay_scatter')


@pytest.mark.parametrize('S,A', [(0, 3), (65, 3), (7, 0), (7, 17)])
def test_scatter_rows_refuses_dims_outside_the_network_range(engine, S, A):
    from serl_amd import _capi
    st, dev, _keep = _staged(7, 3, engine.device, 0, seed=3)
    ring = RW.Ring(50, 20, engine.device)
    jobs = [(ring.ptr, 50, 0, 0, 30, 0, 0)]
    assert RW.launch(engine, dev, S, A, jobs) == _capi.E_UNSUPPORTED
    assert b'serl_replay_scatter_rows' in engine.lib.serl_last_error()
    assert ring.guards_intact() and (ring.rows() == RW.SENTINEL).all()
    assert RW.launch(engine, dev, 7, 3, jobs) == 0                          # the same jobs with dims in range are served
    np.testing.assert_array_equal(ring.rows()[:30], st[0, :30])


# ---- a generation per env configuration ---------------------------------------------------------------------------------------------
class _Buf(list):
    def add(self, *t):
        self.append(t)


def _shape_of(name):
    from serl_amd import builds
    cfg, incr = builds.env_config(name)
    S, A = builds.env_dims(cfg, incr)
    return dict(state_dim=S, action_dim=A, hidden=32, num_layers=3, activation='tanh', env_config=cfg, incremental=incr)


def _weights(s, n, seed):
    """seeded hidden-32 actors (actor_shapes.make_weights); the output biases of every third member moved by -2 / +2 (a steady surface
    deflection on top of the policy) so that some episodes leave the envelope early and collect cost-flagged steps in every
    configuration -- the symmetric task has none otherwise"""
    w = X.make_weights(s, n, seed)
    P, A = X.spec_of(s).param_count, s['action_dim']
    w[:, P - A:P] += 2.0 * (np.arange(n) % 3 - 1)[:, None]
    return w


def _agents(s, w, make_ring):
    from serl_amd.actor import unpack_into
    P = X.spec_of(s).param_count
    out = []
    for row in w:
        m = X.actor_module(s)
        unpack_into(m, torch.from_numpy(row[:P].copy()))
        out.append(types.SimpleNamespace(actor=m, buffer=make_ring(), critical_buffer=make_ring()))
    return out


def _generation(engine, name, s, w, make_ring, shared, n_evals=2, t_max=20, seed=1):
    import serl_amd
    from serl_amd import refsignals
    agents = _agents(s, w, make_ring)
    pop, rl = agents[:-1], agents[-1]
    args = types.SimpleNamespace(num_evals=n_evals, smooth_fitness=False, noise_sd=0.2, noise_clip=0.5)
    E = len(pop) * n_evals + 1
    refs = refsignals.synthetic_reference_tables(E, n_evals, 20, seed=seed)[:, :refsignals.n_steps_for(t_max)]
    noise = np.clip(0.2 * np.random.default_rng(seed).standard_normal((refs.shape[1], 3)), -0.5, 0.5)
    counters = {}
    g = serl_amd.evaluate_generation(pop, rl, args=args, mode=name, t_max=t_max, refs=refs, rl_noise=noise, engine=engine,
                                     replay_buffer=shared, counters=counters, env_config=s['env_config'], incremental=s['incremental'])
    return g, agents, counters, refs, noise


@pytest.mark.parametrize('name', ['PHlab_symmetric_nominal', 'PHlab_full_nominal', 'PHlab_attitude_incremental', 'PHlab_symmetric_incremental',
                                  'PHlab_full_incremental'])
def test_generation_fills_device_rings_like_list_buffers(engine, oracle_engine, name):
    """evaluate_generation on a non-attitude configuration, once with list-backed buffers (a host copy and one add() per step) and once
    with DeviceReplay rings of the configuration's dims (one scatter launch): equal counters, and the rings hold slot for slot what the
    lists hold; the rows of one member equal the CPU oracle's bit for bit"""
    from serl_amd.replay import DeviceReplay
    s = _shape_of(name)
    S, A = s['state_dim'], s['action_dim']
    W = RW.width(S, A)
    n_evals, t_max = 2, 20
    w = _weights(s, 5, seed=1)
    shared = _Buf()
    g, agents, counters, refs, noise = _generation(engine, name, s, w, _Buf, shared, n_evals, t_max)
    dshared = DeviceReplay(20_000, engine.device, engine, S, A)
    ring = lambda: DeviceReplay(150, engine.device, engine, S, A)             # shorter than some stored episodes: those leave their tails
    dg, dagents, dcounters, _, _ = _generation(engine, name, s, w, ring, dshared, n_evals, t_max)
    np.testing.assert_array_equal(dg.pop.fitness, g.pop.fitness)
    assert dcounters == counters and counters['num_episodes'] == 5
    stored = [len(a.buffer) for a in agents]
    T_ = refs.shape[1]
    print('GENERATION %s W %d stored %s critical %s' % (name, W, stored, [len(a.critical_buffer) for a in agents]))
    assert min(stored) < T_, 'no stored episode ended early'
    assert max(stored) > 150, 'no stored episode is longer than its ring'
    assert any(len(a.critical_buffer) for a in agents), 'no cost-flagged step: the compaction path did not run'
    as_rows = lambda buf: np.stack([np.concatenate([np.ravel(np.asarray(x, np.float32)) for x in t]) for t in buf])
    assert tuple(dshared.rows.shape) == (20_000, W) and len(dshared) == len(shared) == sum(stored)
    np.testing.assert_array_equal(dshared.rows[:len(dshared), :W - 1].cpu().numpy(), as_rows(shared))
    for a, d in zip(agents, dagents):
        for lst, rg in ((a.buffer, d.buffer), (a.critical_buffer, d.critical_buffer)):
            assert len(rg) == min(len(lst), rg.capacity) and rg.position == len(lst) % rg.capacity
            if len(lst):
                # a list that outgrew the ring's capacity: the ring holds its last `capacity` tuples, the oldest at `position`
                want = as_rows(lst)
                if len(lst) > rg.capacity:
                    want = np.roll(want[-rg.capacity:], len(lst) % rg.capacity, axis=0)
                np.testing.assert_array_equal(rg.rows[:len(rg), :W - 1].cpu().numpy(), want)
        assert (d.critical_buffer.rows[:len(d.critical_buffer), W - 1] == 1).all()
    # member 0's stored episode (its last evaluation) on the CPU oracle
    e = n_evals - 1
    o = oracle_engine.rollout(torch.from_numpy(w[:1]), X.spec_of(s), [0], refs[e].numpy() if torch.is_tensor(refs) else np.asarray(refs[e]),
                              t_max=t_max, traces=True, transitions=True, env_config=s['env_config'], incremental=s['incremental'])
    n = int(o['length_steps'][0])
    assert n == stored[0]
    got = dagents[0].buffer
    want = o['transitions'][0, :n].numpy()
    if n > got.capacity:
        want = np.roll(want[-got.capacity:], n % got.capacity, axis=0)
    np.testing.assert_array_equal(got.rows[:len(got)].cpu().numpy().view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32))


def test_mismatched_rings_are_refused_before_anything_is_stored(engine):
    """attitude rings (the defaults) under a full-state generation: ValueError naming both, rings and counters untouched"""
    from serl_amd.replay import DeviceReplay
    name = 'PHlab_full_nominal'
    s = _shape_of(name)
    w = _weights(s, 2, seed=2)
    shared = DeviceReplay(5000, engine.device, engine)
    with pytest.raises(ValueError, match='state_dim 7, action_dim 3.*state_dim 13, action_dim 3'):
        _generation(engine, name, s, w, lambda: DeviceReplay(100, engine.device, engine, 13, 3), shared, 1, 3)
    assert len(shared) == 0


# ---- one SSNE epoch on the full-state configuration ---------------------------------------------------------------------------------
class _Critic(torch.nn.Module):
    """stand-in for TD3's twin critic (base/core/td3.py:17-85): two small MLPs over (state, action)"""

    def __init__(self, n_in):
        super().__init__()
        self.q1 = torch.nn.Sequential(torch.nn.Linear(n_in, 32), torch.nn.ELU(), torch.nn.Linear(32, 1))
        self.q2 = torch.nn.Sequential(torch.nn.Linear(n_in, 32), torch.nn.ELU(), torch.nn.Linear(32, 1))

    def forward(self, s, a):
        x = torch.cat([s, a], -1)
        return self.q1(x), self.q2(x)


def _full_population(engine, n=8):
    """8 random hidden-32 actors of the full-state task and their rings, filled by a generation (test 7's path)"""
    from serl_amd.replay import DeviceReplay
    name = 'PHlab_full_nominal'
    s = _shape_of(name)
    w = _weights(s, n + 1, seed=4)
    ring = lambda: DeviceReplay(10_000, engine.device, engine, 13, 3)
    _, agents, _, _, _ = _generation(engine, name, s, w, ring, ring(), 1, 20, seed=4)
    return s, w[:n], [a.buffer for a in agents[:n]], [a.critical_buffer for a in agents[:n]]


def test_default_config_epoch_on_full_state_rings(engine):
    """what test_gpu_ga.py::test_default_config_epoch_runs_on_device asserts, on S = 13 actors with rings of 32-float rows"""
    from serl_amd import ssne
    n = 8
    s, w0, bufs, crits = _full_population(engine, n)
    spec = X.spec_of(s)
    P = spec.param_count
    w = torch.from_numpy(w0.copy()).to(engine.device)
    fills = [len(b) for b in bufs]
    print('EPOCH full-state fills %s critical %s' % (fills, [len(c) for c in crits]))
    assert min(fills) >= 100 and all(tuple(b.rows.shape) == (10_000, 32) for b in bufs + crits)
    args = types.SimpleNamespace(pop_size=n, elite_fraction=0.25, mutation_prob=0.9, mutation_mag=0.0247682869654, mut_type='proximal',
                                 distil_crossover=True, distil_type='distance', crossover_prob=0.0, mutation_batch_size=86,
                                 individual_bs=2_000)
    torch.manual_seed(0)
    critic = _Critic(16).to(engine.device)
    fit = np.random.default_rng(2).normal(-150, 50, n)
    rec = []
    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    ep = ssne.SSNE(args, engine, spec, critic=critic, record=rec)
    elite_slot = ep.epoch(w, fit, buffers=bufs, critical=crits)
    torch.cuda.synchronize()
    out = w.cpu().numpy()[:, :P]
    assert np.isfinite(out).all()
    kinds = [r[0] for r in rec]
    assert kinds.count(3) >= 1 and kinds.count(2) >= 1 and kinds[0] == 0
    best = int(np.argmax(fit))
    assert rec[0] == (0, best, elite_slot)
    mutated = {r[1] for r in rec if r[0] == 2}
    if elite_slot not in mutated:
        np.testing.assert_array_equal(out[elite_slot], w0[best, :P])
    assert len(bufs[elite_slot]) == fills[best]
    np.testing.assert_array_equal(bufs[elite_slot].rows[:fills[best]].cpu().numpy(), bufs[best].rows[:fills[best]].cpu().numpy())
    k = kinds.index(3)
    first, second, slot = rec[k][1], rec[k][2], rec[k + 1][2]
    assert rec[k + 1][0] == 0 and rec[k + 1][1] == -1
    if slot not in mutated:
        assert np.abs(out[slot] - w0[second, :P]).max() > 1e-4 and np.abs(out[slot] - w0[first, :P]).max() > 1e-4
    cur = list(fills)                  # the parents' fills when the child was distilled: after the elite copies that precede it
    for r in rec[:k]:
        if r[0] == 0 and r[1] >= 0:
            cur[r[2]] = cur[r[1]]
    assert len(bufs[slot]) == min(2000, min(1000, cur[first]) + min(1000, cur[second])) > 0
    assert len(crits[slot]) == 0
    for b in bufs + crits:
        assert (b.state_dim, b.action_dim, b.row) == (13, 3, 32) and tuple(b.rows.shape) == (10_000, 32)
        assert torch.isfinite(b.rows[:len(b)]).all()


def test_distil_batch_on_full_state_rings_vs_float64_adam(engine, monkeypatch):
    """distill.distil_batch on rings of 32-float rows (S = 13): the fused path is taken, the child's buffer and empty critical buffer
    have the parents' dims, and the child's parameters agree with the float64 Adam restatement of tests/distill64.py -- fed the child's
    own buffer, the parents' actions and the critic's Q-filter as distil_batch evaluates them, and the minibatches the same seed draws
    -- within distill64.tolerance."""
    from serl_amd import distill
    from serl_amd.replay import DeviceReplay
    s, w0, bufs, _ = _full_population(engine, 8)
    spec = X.spec_of(s)
    P, S, A = spec.param_count, 13, 3
    w = torch.from_numpy(w0.copy()).to(engine.device)
    order = np.argsort([len(b) for b in bufs])
    first, second = int(order[-1]), int(order[-2])                       # the two fullest rings
    args = types.SimpleNamespace(individual_bs=600)
    torch.manual_seed(0)
    critic = _Critic(S + A).to(engine.device)

    def unfused(*a, **k):
        raise AssertionError('distil_batch left the fused path')
    with monkeypatch.context() as mp:
        mp.setattr(distill, 'distilation_crossover', unfused)
        random.seed(13); torch.manual_seed(13)
        (row, buf, crit), = distill.distil_batch(args, engine, spec, w, [(first, second)], bufs, critic)
        torch.cuda.synchronize()
        after = random.random()
    assert (buf.state_dim, buf.action_dim, crit.state_dim, crit.action_dim) == (13, 3, 13, 3) and len(crit) == 0
    n = len(buf)
    assert n == min(300, len(bufs[first])) + min(300, len(bufs[second])) and n >= 128
    # the host draws again, in distil_batch's order: the buffer shuffle, then 12 x (n // B) minibatches
    random.seed(13)
    again = DeviceReplay(600, engine.device, engine, S, A)
    again.add_latest_from(bufs[first], 300); again.add_latest_from(bufs[second], 300)
    again.shuffle(random)
    np.testing.assert_array_equal(again.rows[:n].cpu().numpy(), buf.rows[:n].cpu().numpy())
    B = min(128, n)
    n_steps = 12 * (n // B)
    slots = distill.sample_minibatches(n, B, n_steps, random)
    assert random.random() == after
    states = buf.rows[:n, :S].contiguous()
    with torch.no_grad():
        a1 = distill._batched_forward(spec, w[[first]], states[None])[0]
        a2 = distill._batched_forward(spec, w[[second]], states[None])[0]
        q1, q2 = torch.min(*critic(states, a1)).flatten(), torch.min(*critic(states, a2)).flatten()
        take1 = (q1 - q2) > 1e-5                                            # genetic_agent.py:44-46
        keep = (take1 | ((q2 - q1) >= 1e-5)).to(torch.float32)
        targets = torch.where(take1[:, None], a1, a2)
    w64 = D.distill_literal(s, w0[second, :P], states.cpu().numpy(), targets.cpu().numpy(), keep.cpu().numpy(), slots, n_steps, B)
    moved = np.abs(w64 - w0[second, :P]).max()
    err = np.abs(row.cpu().numpy()[:P].astype(np.float64) - w64).max()
    print('DISTILL_FULL pair %s buffer %d steps %d kept %d |fused - f64| %.3g moved %.4f ratio %.3g' %
          ((first, second), n, n_steps, int(keep.sum()), err, moved, err / moved))
    assert moved > D.MIN_MOVED
    assert err <= D.tolerance('tanh', moved), (err, moved)

"""serl_ga_novelty_general on the GPU against the float64 contract of tests/nov64.py: every grid case in both dense flavours (the same
bits) and both gather layouts (the same bits), mixed batch sizes in one launch against single launches, the member listed twice, clamped
slots, an empty batch, serl_ga_novelty held against it where both run, every refusal with the output untouched, and
sort_groups_by_distance / SSNE with the choice passed through.

Planted slips: each of these, planted in the kernel's steps as restated by nov64.by_hand64, moves a grid value by more than 1000 x the
bound (tests/test_ga_nov_host.py::test_planted_slips_exceed_the_bound), i.e. fails test_grid_vs_float64 below on the cases named:
  mean_128          a mean over 128 instead of batch[e]                  every case but B = 128 (0.8 % at B 127 / 129, 33 % and more elsewhere)
  padded_counted    the zero columns behind batch[e] counted             every case whose B is no multiple of 128
  action_offset     the ring's action offset off by one                  every case, in the ring layout (and ring != dense bit for bit)
  neighbour_slots   the slot row of the neighbouring evaluation          every case, in the ring layout
  square_of_sum     (sum_a d_a)^2 instead of sum_a d_a^2                 every case with A > 1
  first_chunk_only  chunks beyond the first dropped                      B = 129, 256, 512
"""
import ctypes, os, random, sys, types
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nov64 as Z

pytestmark = pytest.mark.gpu
GUARD = 16
SENTINEL = 12345.678
KEYS = list(range(len(Z.GRID)))


def _id(key):
    return Z.case_id(Z.GRID[key])


def _call(engine, spec, w, members, sp, ss, ap, as_, slots, n_rows, batch, max_batch, dense, expect=0):
    """a direct call of serl_ga_novelty_general, `novelty` between guard words and pre-filled with the sentinel -> f32 [n] (host).  sp /
    ap: per-evaluation device addresses; slots: int32 [n, max_batch] or None"""
    dev = engine.device
    n = len(members)
    out = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float32, device=dev)
    i32 = lambda a: torch.tensor(np.asarray(a, np.int32), device=dev) if a is not None else None
    i64 = lambda a: torch.tensor(np.asarray(a, np.int64), device=dev) if a is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    m, spt, apt, sl, nr, bt = i32(members), i64(sp), i64(ap), i32(slots), i32(n_rows), i32(batch)
    if sl is not None:
        assert sl.shape == (n, max_batch)
    rc = engine.lib.serl_ga_novelty_general(engine.ctx, w.data_ptr(), w.stride(0), spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim,
                                            spec.activation_id, ptr(m), n, ptr(spt), ss, ptr(apt), as_, ptr(sl), ptr(nr), ptr(bt), max_batch,
                                            out[GUARD:].data_ptr(), dense, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect, (rc, engine.lib.serl_last_error())
    o = out.cpu().numpy()
    assert (o[:GUARD] == np.float32(SENTINEL)).all() and (o[GUARD + n:] == np.float32(SENTINEL)).all(), 'guard words around novelty changed'
    return o[GUARD:GUARD + n].copy()


class _Case:
    """a grid case on the device in both layouts"""

    def __init__(self, engine, key):
        self.case, self.ref = Z.reference(key)
        c = self.case
        self.spec = Z.spec_of(c['c'])
        dev = engine.device
        self.engine = engine
        self.w = torch.from_numpy(c['weights']).to(dev)
        self.st = torch.from_numpy(c['states']).to(dev).contiguous()
        self.ac = torch.from_numpy(c['actions']).to(dev).contiguous()
        rings, self.slots = Z.ring_layout(c)
        self.rings = torch.from_numpy(rings).to(dev).contiguous()
        self.n, self.B, self.S, self.A = len(c['members']), c['B'], c['S'], c['A']
        self.W = 2 * self.S + self.A + 3

    def dense(self, dense=0, evals=None, batch=None, max_batch=None):
        ev = list(range(self.n)) if evals is None else evals
        batch = [self.B] * len(ev) if batch is None else batch
        sp = [self.st.data_ptr() + 4 * e * self.B * self.S for e in ev]
        ap = [self.ac.data_ptr() + 4 * e * self.B * self.A for e in ev]
        return _call(self.engine, self.spec, self.w, [self.case['members'][e] for e in ev], sp, self.S, ap, self.A, None, [self.B] * len(ev),
                     batch, self.B if max_batch is None else max_batch, dense)

    def ring(self, dense=0, slots=None):
        rows = self.rings.shape[1]
        sp = [self.rings.data_ptr() + 4 * e * rows * self.W for e in range(self.n)]
        ap = [p + 4 * self.S for p in sp]
        return _call(self.engine, self.spec, self.w, self.case['members'], sp, self.W, ap, self.W, self.slots if slots is None else slots,
                     [rows] * self.n, [self.B] * self.n, self.B, dense)


@pytest.mark.parametrize('key', KEYS, ids=_id)
def test_grid_vs_float64(engine, key):
    """every case: four evaluations, members [2, 0, 2, 1], within TOL of float64; dense 0 and 1 the same bits; the ring layout with a slot
    table the same bits as the rows passed densely; the member listed twice (on the same batch) twice the same value"""
    k = _Case(engine, key)
    valu, mfma = k.dense(0), k.dense(1)
    err = Z.rel_err(valu, k.ref)
    print('%s general: err %s (bound %.3e)' % (_id(key), err, Z.TOL))
    assert np.isfinite(valu).all() and err.max() <= Z.TOL
    np.testing.assert_array_equal(mfma, valu)
    np.testing.assert_array_equal(k.ring(0), valu)
    np.testing.assert_array_equal(k.ring(1), valu)
    assert valu[0] == valu[2] and len(set(valu.tolist())) == 3


def test_mixed_batch_sizes_in_one_launch_equal_single_launches(engine):
    """batch sizes [1, 127, 128, 129, 256] side by side (max_batch 256) against each evaluation launched alone with max_batch = its own
    batch, both flavours: the same bits; and each within TOL of float64 on the rows it takes"""
    k = _Case(engine, 2)
    assert k.B == 256
    evals, batch = [0, 1, 3, 1, 3], [1, 127, 128, 129, 256]
    for dense in (0, 1):
        together = k.dense(dense, evals, batch)
        alone = np.array([k.dense(dense, [e], [b], max_batch=b)[0] for e, b in zip(evals, batch)])
        np.testing.assert_array_equal(together, alone)
    c = k.case
    ref = [Z.novelty64(c['c'], c['weights'][c['members'][e]], c['states'][e][:b], c['actions'][e][:b]) for e, b in zip(evals, batch)]
    assert Z.rel_err(together, ref).max() <= Z.TOL
    # a batch above max_batch is clamped to it
    np.testing.assert_array_equal(k.dense(0, [1], [300], max_batch=129), k.dense(0, [1], [129], max_batch=129))


def test_empty_batch_is_nan_and_leaves_its_neighbours(engine):
    k = _Case(engine, 4)
    full = k.dense(0)
    for batch in ([k.B, 0, k.B, k.B], [k.B, k.B, k.B, -7]):
        got = k.dense(0, None, batch)
        e = batch.index(min(batch))
        assert np.isnan(got[e])
        keep = [i for i in range(4) if i != e]
        np.testing.assert_array_equal(got[keep], full[keep])
    # no rows behind the bases: the same
    sp = [k.st.data_ptr()] * 2
    got = _call(engine, k.spec, k.w, [0, 1], sp, k.S, [k.ac.data_ptr()] * 2, k.A, None, [0, k.B], [k.B, k.B], k.B, 1)
    assert np.isnan(got[0]) and np.isfinite(got[1])


def test_slots_are_clamped_to_the_rows(engine):
    """slots -5 and n_rows + 3 read rows 0 and n_rows - 1: the same bits as the clamped table, and not those of the original"""
    k = _Case(engine, 1)
    rows = k.rings.shape[1]
    wild, clamped = k.slots.copy(), k.slots.copy()
    wild[:, 3], wild[:, 40] = -5, rows + 3
    clamped[:, 3], clamped[:, 40] = 0, rows - 1
    got = k.ring(0, wild)
    np.testing.assert_array_equal(got, k.ring(0, clamped))
    assert (got != k.ring(0)).all()


@pytest.mark.parametrize('key', KEYS, ids=_id)
def test_general_and_lds_within_the_bound_of_each_other(engine, key):
    """serl_ga_novelty takes every shape of the grid (its LDS holds one sample): the two kernels sum in different orders, so they are
    within TOL of each other, not equal; ga.novelty(kernel='general') is the direct call"""
    from serl_amd import ga
    k = _Case(engine, key)
    c = k.case
    lds = ga.novelty(engine, k.w, c['members'], k.spec, k.st, k.ac).cpu().numpy()
    gen = ga.novelty(engine, k.w, c['members'], k.spec, k.st, k.ac, kernel='general').cpu().numpy()
    mf = ga.novelty(engine, k.w, c['members'], k.spec, k.st, k.ac, kernel='general', dense='mfma').cpu().numpy()
    np.testing.assert_array_equal(gen, k.dense(0))
    np.testing.assert_array_equal(mf, gen)
    d = np.abs(gen.astype(np.float64) - lds) / gen
    print('%s general vs lds: %s; lds vs float64 %s (bound %.3e)' % (_id(key), d, Z.rel_err(lds, k.ref), Z.TOL))
    assert d.max() <= Z.TOL


def test_auto_is_lds_at_hidden_128_x_3(engine):
    """hidden 128 x 3, which serl_ga_novelty still takes (its LDS holds one sample): 'auto' equals 'lds' bit for bit, 'general' is within
    the bound of it; a shape the general kernel refuses is the library's message, never another path"""
    import serl_amd
    from serl_amd import ga
    c = Z.make_case((7, 3, 128, 3, 'tanh', 86))
    spec = Z.spec_of(c['c'])
    w = torch.from_numpy(c['weights']).to(engine.device)
    lds = ga.novelty(engine, w, c['members'], spec, c['states'], c['actions'])
    assert torch.equal(ga.novelty(engine, w, c['members'], spec, c['states'], c['actions'], kernel='auto'), lds)
    assert torch.equal(ga.novelty(engine, w, c['members'], spec, c['states'], c['actions'], kernel='auto', dense='mfma'), lds)
    gen = ga.novelty(engine, w, c['members'], spec, c['states'], c['actions'], kernel='general').cpu().numpy()
    ref = Z.reference_of(c)
    assert Z.rel_err(gen, ref).max() <= Z.TOL
    assert (np.abs(gen.astype(np.float64) - lds.cpu().numpy()) / gen).max() <= Z.TOL
    spec = serl_amd.NetSpec(7, 3, 34, 3, 'tanh')
    with pytest.raises(RuntimeError, match=r'serl_ga_novelty_general failed \(-3\).*4 \.\. 128'):
        ga.novelty(engine, torch.zeros(2, spec.param_count, device=engine.device), [0], spec, torch.zeros(1, 5, 7), torch.zeros(1, 5, 3),
                   kernel='general')
    with pytest.raises(ValueError, match='outside the population'):
        ga.novelty(engine, w, [3], Z.spec_of(c['c']), c['states'][:1], c['actions'][:1], kernel='general')


def test_every_refusal_leaves_the_output_untouched(engine):
    """with a live context: every refusal of the contract returns its code before any launch; `novelty` keeps the sentinel"""
    from serl_amd import _capi
    k = _Case(engine, 1)
    spec, n = k.spec, k.n
    sp = [k.st.data_ptr() + 4 * e * k.B * k.S for e in range(n)]
    ap = [k.ac.data_ptr() + 4 * e * k.B * k.A for e in range(n)]
    ok = dict(spec=spec, w=k.w, members=k.case['members'], sp=sp, ss=k.S, ap=ap, as_=k.A, slots=None, n_rows=[k.B] * n, batch=[k.B] * n,
              max_batch=k.B, dense=0)

    def refused(code, **kw):
        a = dict(ok, **kw)
        got = _call(engine, a['spec'], a['w'], a['members'], a['sp'], a['ss'], a['ap'], a['as_'], a['slots'], a['n_rows'], a['batch'],
                    a['max_batch'], a['dense'], expect=code)
        assert (got == np.float32(SENTINEL)).all(), kw
    for kw in (dict(sp=None), dict(ap=None), dict(n_rows=None), dict(batch=None), dict(dense=2), dict(dense=-1), dict(ss=k.S - 1),
               dict(as_=k.A - 1), dict(w=torch.zeros(3, spec.param_count - 1, device=engine.device))):
        refused(_capi.E_INVALID, **kw)
    import serl_amd
    for shp in ((7, 3, 34, 3), (7, 3, 132, 3), (7, 3, 32, 5), (17, 3, 32, 3), (7, 5, 32, 3)):
        refused(_capi.E_UNSUPPORTED, spec=serl_amd.NetSpec(*shp, 'tanh'))
    for mb in (0, 513, -1):
        refused(_capi.E_UNSUPPORTED, max_batch=mb)
    bad_act = types.SimpleNamespace(state_dim=7, hidden=32, num_layers=3, action_dim=3, activation_id=3)
    refused(_capi.E_UNSUPPORTED, spec=bad_act)
    assert np.isfinite(_call(engine, **ok)).all()       # and the unrefused call runs


# ---- sort_groups_by_distance and SSNE ---------------------------------------------------------------------------------------------------
def _device_rings(engine, seed=3):
    """five rings of different fill: 300, 700 (wrapped twice), 40, 2600 (wrapped), 120 rows -> batches of 40, 120 and 256"""
    from serl_amd.replay import DeviceReplay
    g = torch.Generator().manual_seed(seed)
    out = []
    for cap, n in ((5000, 300), (700, 1900), (5000, 40), (2600, 4000), (1500, 120)):
        r = DeviceReplay(cap, engine.device, engine)
        for lo in range(0, n, 900):
            r.append_rows(2 * torch.rand(min(900, n - lo), r.row, generator=g) - 1)
        out.append(r)
    return out


def _same_groups(got, want, what):
    """the same pairs; distances within TOL of each other; the same order wherever neighbouring distances differ by more than TOL"""
    assert sorted((a, b) for a, b, _ in got) == sorted((a, b) for a, b, _ in want), what
    dw = {(a, b): d for a, b, d in want}
    for a, b, d in got:
        assert abs(d - dw[a, b]) / dw[a, b] <= Z.TOL, (what, a, b, d, dw[a, b])
    ds = [d for _, _, d in want]
    clear = all((ds[i] - ds[i + 1]) / ds[i] > 2 * Z.TOL for i in range(len(ds) - 1))
    if clear:
        assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want], what
    assert [d for _, _, d in got] == sorted((d for _, _, d in got), reverse=True)
    return clear


def test_sort_groups_by_distance_one_launch_for_all_batch_sizes(engine):
    """five rings of different fill (batches of 40, 120 and 256 rows in ONE launch): the pairs of 'lds', python's generator left in the
    same state, the distances within TOL of 'lds' and of float64, the same order"""
    from serl_amd import ga
    c = Z.make_case((7, 3, 32, 3, 'tanh', 1))
    spec = Z.spec_of(c['c'])
    w = torch.from_numpy(np.concatenate([c['weights'], Z.make_case((7, 3, 32, 3, 'tanh', 1), 77)['weights'][:2]])).to(engine.device)
    rings = _device_rings(engine)
    genomes = [3, 0, 4, 1, 2]
    buffers = {i: rings[i] for i in range(5)}
    random.seed(21)
    lds = ga.sort_groups_by_distance(engine, w, genomes, buffers, spec)
    state = random.getstate()
    plan = ga.distance_plan(genomes, buffers, random.Random(0))
    assert sorted(set(plan['batch'].tolist())) == [40, 120, 256]
    calls = []
    for dense in ('valu', 'mfma'):
        random.seed(21)
        got = ga.sort_groups_by_distance(engine, w, genomes, buffers, spec, kernel='general', dense=dense)
        assert random.getstate() == state
        clear = _same_groups(got, lds, dense)
        calls.append((got, clear))
    assert calls[0][0] == calls[1][0] and calls[0][1]
    # against float64, evaluation by evaluation, through the plan of the same seed
    random.seed(21)
    plan = ga.distance_plan(genomes, buffers, random)
    ref = {}
    for k, (second, first, bs) in enumerate(plan['pairs']):
        d = 0.0
        for e in (2 * k, 2 * k + 1):
            rows = plan['rings'][e].rows[torch.from_numpy(plan['slots'][e, :bs].astype(np.int64)).to(engine.device)].cpu().numpy()
            d += Z.novelty64(c['c'], w[int(plan['members'][e])].cpu().numpy(), rows[:, :7], rows[:, 7:10])
        ref[second, first] = d
    for a, b, d in calls[0][0]:
        assert abs(d - ref[a, b]) / ref[a, b] <= Z.TOL
    # 'auto': serl_ga_novelty takes this actor, so it is 'lds', bit for bit
    random.seed(21)
    assert ga.sort_groups_by_distance(engine, w, genomes, buffers, spec, kernel='auto') == lds
    # an empty buffer: refused before the launch
    from serl_amd.replay import DeviceReplay
    with pytest.raises(ValueError, match='empty buffer'):
        ga.sort_groups_by_distance(engine, w, [0, 1], {0: rings[0], 1: DeviceReplay(100, engine.device, engine)}, spec, kernel='general')


def test_one_launch_for_every_batch_size(engine, monkeypatch):
    """kernel='general' calls serl_ga_novelty_general once for the 20 evaluations and never serl_ga_novelty; 'lds' calls serl_ga_novelty
    once per batch size"""
    from serl_amd import ga
    c = Z.make_case((7, 3, 32, 3, 'tanh', 1))
    spec = Z.spec_of(c['c'])
    w = torch.from_numpy(np.concatenate([c['weights'], Z.make_case((7, 3, 32, 3, 'tanh', 1), 77)['weights'][:2]])).to(engine.device)
    rings = _device_rings(engine)
    seen = []
    real = ga._novelty_general
    monkeypatch.setattr(ga, '_novelty_general', lambda *a, **k: (seen.append(('general', len(a[2]))), real(*a, **k))[1])
    real_nov = ga.novelty
    monkeypatch.setattr(ga, 'novelty', lambda *a, **k: (seen.append(('lds', len(a[2]))), real_nov(*a, **k))[1])
    random.seed(2)
    ga.sort_groups_by_distance(engine, w, [0, 1, 2, 3, 4], {i: rings[i] for i in range(5)}, spec, kernel='general')
    assert seen == [('general', 20)]
    del seen[:]
    random.seed(2)
    ga.sort_groups_by_distance(engine, w, [0, 1, 2, 3, 4], {i: rings[i] for i in range(5)}, spec)
    assert sorted(seen) == [('lds', 6), ('lds', 6), ('lds', 8)]          # batches of 256, 120 and 40 rows


class _Critic(torch.nn.Module):
    """stand-in for TD3's twin critic: two small MLPs over (state, action)"""

    def __init__(self):
        super().__init__()
        self.q1 = torch.nn.Sequential(torch.nn.Linear(10, 32), torch.nn.ELU(), torch.nn.Linear(32, 1))
        self.q2 = torch.nn.Sequential(torch.nn.Linear(10, 32), torch.nn.ELU(), torch.nn.Linear(32, 1))

    def forward(self, s, a):
        x = torch.cat([s, a], -1)
        return self.q1(x), self.q2(x)


def test_ssne_epoch_with_the_general_novelty_kernel(engine, golden, monkeypatch):
    """SSNE(novelty_kernel='general') with distance-sorted distillation: one epoch runs; its groups are those of an epoch with 'lds'
    (pairs, distances within TOL, order), and so are the recorded operator calls and python's generator afterwards"""
    import serl_amd
    from serl_amd import ga, ssne
    from serl_amd.replay import DeviceReplay
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    n = 6
    w0 = golden('actors')['serl50'][:n].copy()
    rows = torch.from_numpy(golden('proximal')['buf_serl50_18'])
    args = types.SimpleNamespace(pop_size=n, elite_fraction=0.34, mutation_prob=0.9, mutation_mag=0.05, mut_type='normal',
                                 distil_crossover=True, distil_type='distance', crossover_prob=0.0, mutation_batch_size=86, individual_bs=600)
    fit = np.random.default_rng(2).normal(-150, 50, n)
    groups, runs = {}, {}
    real = ga.sort_groups_by_distance
    for kernel, dense in (('lds', 'valu'), ('general', 'valu'), ('general', 'mfma')):
        monkeypatch.setattr(ga, 'sort_groups_by_distance',
                            lambda *a, **k: (groups.__setitem__((k['kernel'], k['dense']), real(*a, **k)), groups[k['kernel'], k['dense']])[1])
        bufs, crits = [], []
        for k in range(n):
            r = DeviceReplay(5_000, engine.device, engine)
            r.append_rows(rows[:150 + 40 * k])
            bufs.append(r)
            crits.append(DeviceReplay(1_000, engine.device, engine))
        w = torch.nn.functional.pad(torch.from_numpy(w0.copy()), (0, 1)).contiguous().to(engine.device)
        torch.manual_seed(0)
        critic = _Critic().to(engine.device)
        rec = []
        random.seed(3); np.random.seed(3); torch.manual_seed(3)
        ep = ssne.SSNE(args, engine, spec, critic=critic, record=rec, novelty_kernel=kernel, novelty_dense=dense)
        ret = ep.epoch(w, fit, buffers=bufs, critical=crits)
        torch.cuda.synchronize()
        assert np.isfinite(w.cpu().numpy()[:, :spec.param_count]).all()
        runs[kernel, dense] = (rec, ret, random.random())
    assert len(groups) == 3 and len(groups['lds', 'valu']) >= 3 and any(r[0] == 3 for r in runs['lds', 'valu'][0])
    assert len({g[2] for g in groups['lds', 'valu']}) > 1
    for key in (('general', 'valu'), ('general', 'mfma')):
        if _same_groups(groups[key], groups['lds', 'valu'], key):
            assert runs[key] == runs['lds', 'valu'], key
    assert groups['general', 'valu'] == groups['general', 'mfma']

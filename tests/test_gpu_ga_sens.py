"""serl_ga_sensitivity_general on the GPU against the float64 contract of tests/sens64.py: every grid and degenerate case in both dense
flavours (the same bits), serl_ga_sensitivity held to the same yardstick where it runs, hidden 128 x 3 -- the shape that kernel refuses --
through ga.sensitivity(kernel='general'), the default path bit for bit what it was, guard words, two streams, ProximalBatch and an SSNE
epoch with the choice passed through."""
import ctypes, os, random, re, sys, types
import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sens64 as Z

pytestmark = pytest.mark.gpu
GUARD = 64                      # guard words on either side of `scaling` and `work`
SENTINEL = 12345.678


def _lds_kernel_fits(case, lds_bytes=160 * 1024):
    """whether serl_ga_sensitivity takes the shape: one output's gradient of the genome, the forward buffers and two vectors in LDS"""
    S, A, H, L = case['S'], case['A'], case['H'], case['L']
    fwd = S + 2 * (L + 1) * H + L * H + L + 2 * A + 16
    return 4 * (Z.genome_size(S, A, H, L) + fwd + 2 * H) <= lds_bytes


def _general(engine, case, spec, dense, stream=None):
    """a direct call of serl_ga_sensitivity_general between guard words, the workspace full of NaN on entry -> scaling f32 [n, G] (device)"""
    from serl_amd import _capi
    dev = engine.device
    L = engine.lib
    w = torch.from_numpy(case['weights']).to(dev)
    st = torch.from_numpy(case['states']).to(dev).contiguous()
    m = torch.tensor(case['members'], dtype=torch.int32, device=dev)
    n, B = st.shape[0], st.shape[1]
    G = Z.genome_size(case['S'], case['A'], case['H'], case['L'])
    nbytes = int(L.serl_ga_sensitivity_general_work_bytes(n, case['S'], case['A'], case['H'], case['L'], B))
    assert nbytes > 0 and nbytes % 4 == 0
    out = torch.full((2 * GUARD + n * G,), SENTINEL, dtype=torch.float32, device=dev)
    work = torch.full((2 * GUARD + nbytes // 4,), float('nan'), dtype=torch.float32, device=dev)
    work[:GUARD] = SENTINEL
    work[-GUARD:] = SENTINEL
    s = torch.cuda.current_stream(dev) if stream is None else stream
    s.wait_stream(torch.cuda.current_stream(dev))
    rc = L.serl_ga_sensitivity_general(engine.ctx, w.data_ptr(), w.stride(0), spec.state_dim, spec.hidden, spec.num_layers, spec.action_dim,
                                       spec.activation_id, m.data_ptr(), n, st.data_ptr(), B, out[GUARD:].data_ptr(),
                                       work[GUARD:].data_ptr(), nbytes, dense, ctypes.c_void_p(s.cuda_stream))
    _capi.check(rc, 'serl_ga_sensitivity_general')
    s.synchronize()
    for name, t in (('scaling', out), ('work', work)):
        assert (t[:GUARD] == SENTINEL).all() and (t[-GUARD:] == SENTINEL).all(), 'guard words around %s changed' % name
    assert w.stride(0) == case['P'] + (case['weights'].shape[1] - case['P'])
    return out[GUARD:GUARD + n * G].reshape(n, G).clone()


def _held_to_the_yardstick(got, raw, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), what
    for k in range(len(got)):
        err, share = Z.compare(got[k], raw[k])
        print('%s member %d: err %.3e (bound %.3e) excluded %.4f %%' % (what, k, err, Z.TOL, 100 * share))
        assert err <= Z.TOL, (what, k, err)
        assert share <= Z.EXCLUDED_CAP, (what, k, share)


@pytest.mark.parametrize('key', Z.ALL_KEYS, ids=Z.key_id)
def test_both_flavours_and_the_lds_kernel_vs_float64(engine, key):
    """every case: dense 0 and 1 within TOL of the float64 run and equal to each other bit for bit, guard words intact; where
    serl_ga_sensitivity takes the shape it meets the same bound in the same run (both kernels are held to the yardstick, not to each
    other), and it is refused exactly where its LDS accumulators do not fit"""
    from serl_amd import ga, _capi
    case, raw = Z.reference(key)
    spec = Z.spec_of(Z.GRID[key] if isinstance(key, int) else next(d for d in Z.DEGENERATE if d[0] == key)[1])
    valu = _general(engine, case, spec, 0)
    mfma = _general(engine, case, spec, 1)
    _held_to_the_yardstick(valu, raw, Z.key_id(key) + ' general valu')
    _held_to_the_yardstick(mfma, raw, Z.key_id(key) + ' general mfma')
    assert torch.equal(valu, mfma)
    w = torch.from_numpy(case['weights']).to(engine.device)
    st = torch.from_numpy(case['states'])
    if _lds_kernel_fits(case):
        lds = ga.sensitivity(engine, w, case['members'], spec, st, fallback=False)
        _held_to_the_yardstick(lds, raw, Z.key_id(key) + ' lds')
    else:
        with pytest.raises(RuntimeError, match=r'serl_ga_sensitivity failed \(%d\)' % _capi.E_UNSUPPORTED):
            ga.sensitivity(engine, w, case['members'], spec, st, fallback=False)
    if case['name'] == 'wo0':                       # every gradient but Wo's own is exactly 0 -> scaling == 1
        k = case['members'].index(1)
        assert (valu[k, :-case['A'] * case['H']] == 1.0).all() and (valu[k, -case['A'] * case['H']:] != 1.0).all()
    if case['name'] == 'sd0':                       # nothing flows below the degenerate layer; its own W has a gradient
        H, S = case['H'], case['S']
        assert (valu[1, :H * S + H * H] == 1.0).all() and (valu[1, H * S + H * H:H * S + 2 * H * H] > 0.02).any()
    if case['name'] == 'small':
        assert ((valu == np.float32(0.01)).float().mean(1) > Z.SMALL_SHARE).all()


def test_hidden_128_three_layers_with_the_general_kernel(engine):
    """the shape the TD3 learner and serl_ga_distill_general take and serl_ga_sensitivity refuses: ga.sensitivity(kernel='general')
    returns it within TOL of float64, in both flavours; kernel='auto' takes the same kernel there and the LDS kernel at 32 x 3"""
    from serl_amd import ga
    key = 1
    assert Z.GRID[key][:4] == (7, 3, 128, 3)
    case, raw = Z.reference(key)
    spec = Z.spec_of(Z.GRID[key])
    w = torch.from_numpy(case['weights']).to(engine.device)
    st = torch.from_numpy(case['states'])
    with pytest.raises(RuntimeError, match='serl_ga_sensitivity failed'):
        ga.sensitivity(engine, w, case['members'], spec, st, fallback=False)
    got = {}
    for dense in ('valu', 'mfma'):
        got[dense] = ga.sensitivity(engine, w, case['members'], spec, st, kernel='general', dense=dense, fallback=False)
        _held_to_the_yardstick(got[dense], raw, '128x3 general ' + dense)
    assert torch.equal(got['valu'], got['mfma'])
    assert torch.equal(ga.sensitivity(engine, w, case['members'], spec, st, kernel='auto'), got['valu'])
    assert torch.equal(ga.sensitivity(engine, w, case['members'], spec, st, kernel='auto', dense='mfma', fallback=False), got['valu'])
    case, _ = Z.reference(5)                         # 32 x 3: 'auto' is the LDS kernel
    spec = Z.spec_of(Z.GRID[5])
    w = torch.from_numpy(case['weights']).to(engine.device)
    st = torch.from_numpy(case['states'])
    assert torch.equal(ga.sensitivity(engine, w, case['members'], spec, st, kernel='auto'), ga.sensitivity(engine, w, case['members'], spec, st))
    # a shape the general kernel does not take: the library's message, never PyTorch
    import serl_amd
    spec = serl_amd.NetSpec(7, 3, 34, 3, 'tanh')
    with pytest.raises(RuntimeError, match=r'serl_ga_sensitivity_general failed \(-3\).*4 \.\. 128'):
        ga.sensitivity(engine, torch.zeros(2, spec.param_count, device=engine.device), [0], spec, torch.zeros(1, 5, 7), kernel='general')


def test_the_default_is_bit_for_bit_what_it_was(engine):
    """kernel='lds' (the default) returns what a direct call of serl_ga_sensitivity returns; at 128 x 3 what sensitivity_torch returns"""
    from serl_amd import ga, _capi
    case, _ = Z.reference(0)
    spec = Z.spec_of(Z.GRID[0])
    dev = engine.device
    w = torch.from_numpy(case['weights']).to(dev)
    st = torch.from_numpy(case['states']).to(dev).contiguous()
    m = torch.tensor(case['members'], dtype=torch.int32, device=dev)
    n, B = st.shape[0], st.shape[1]
    direct = torch.empty(n, Z.genome_size(7, 3, 72, 3), dtype=torch.float32, device=dev)
    _capi.check(engine.lib.serl_ga_sensitivity(engine.ctx, w.data_ptr(), w.stride(0), 7, 72, 3, 3, spec.activation_id, m.data_ptr(), n,
                                               st.data_ptr(), B, direct.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                'serl_ga_sensitivity')
    assert torch.equal(ga.sensitivity(engine, w, case['members'], spec, st), direct)
    assert torch.equal(ga.sensitivity(engine, w, case['members'], spec, st, kernel='lds', dense='valu'), direct)
    case, _ = Z.reference(1)
    spec = Z.spec_of(Z.GRID[1])
    w = torch.from_numpy(case['weights']).to(dev)
    st = torch.from_numpy(case['states']).to(dev)
    assert torch.equal(ga.sensitivity(engine, w, case['members'], spec, st), ga.sensitivity_torch(w, case['members'], spec, st))


def test_two_streams_give_equal_results(engine):
    """two launches on two streams over the same members (workspaces of their own): equal results"""
    case, _ = Z.reference(0)
    spec = Z.spec_of(Z.GRID[0])
    s1, s2 = torch.cuda.Stream(engine.device), torch.cuda.Stream(engine.device)
    a = _general(engine, case, spec, 1, s1)
    b = _general(engine, case, spec, 1, s2)
    assert torch.equal(a, b) and torch.equal(a, _general(engine, case, spec, 1))
    # through ga.sensitivity: the cached workspace is per stream
    from serl_amd import ga
    w = torch.from_numpy(case['weights']).to(engine.device)
    st = torch.from_numpy(case['states']).to(engine.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c = ga.sensitivity(engine, w, case['members'], spec, st, kernel='general')
    with torch.cuda.stream(s2):
        d = ga.sensitivity(engine, w, case['members'], spec, st, kernel='general')
    torch.cuda.synchronize()
    assert torch.equal(c, a) and torch.equal(d, a)
    assert len(engine._sens_work) >= 2


def test_proximal_batch_equals_single_mutations(engine, golden):
    """ProximalBatch.apply with kernel='general' over three members with two different batch sizes (one launch per batch size) equals
    three single proximal_mutate calls fed the same draws"""
    import actor_shapes as X
    import serl_amd
    from serl_amd import ga
    from serl_amd.replay import DeviceReplay
    g = golden('proximal')
    spec = serl_amd.NetSpec(7, 3, 128, 3, 'tanh')
    w0 = X.make_weights(dict(state_dim=7, action_dim=3, hidden=128, num_layers=3, activation='tanh', env_config=0, incremental=False), 3, 12)
    rings = []
    for n_rows in (40, 200, 150):               # batches of 40, 86, 86 rows
        r = DeviceReplay(10_000, engine.device, engine)
        r.append_rows(torch.from_numpy(g['buf_serl50_18'][:n_rows]))
        rings.append(r)
    for dense in ('valu', 'mfma'):
        wb = torch.from_numpy(w0.copy()).to(engine.device)
        random.seed(4); torch.manual_seed(4)
        batch = ga.ProximalBatch(engine, wb, spec, 0.05, 86, kernel='general', dense=dense)
        for m in (0, 1, 2):
            batch.add(m, rings[m])
        assert sorted(it[1].shape[0] for it in batch.items) == [40, 86, 86]
        calls = []
        real = ga.sensitivity
        ga.sensitivity = lambda *a, **k: (calls.append((a[4].shape[1], k.get('kernel'), k.get('dense'))), real(*a, **k))[1]
        try:
            batch.apply()
        finally:
            ga.sensitivity = real
        assert sorted(calls) == [(40, 'general', dense), (86, 'general', dense)]
        ws = torch.from_numpy(w0.copy()).to(engine.device)
        random.seed(4); torch.manual_seed(4)
        for m in (0, 1, 2):
            ga.proximal_mutate(engine, ws, m, spec, 0.05, rings[m], 86, kernel='general', dense=dense)
        torch.cuda.synchronize()
        assert torch.equal(wb, ws)
        assert (wb.cpu().numpy()[:, :spec.param_count] != w0[:, :spec.param_count]).any(1).all()


def test_ssne_epoch_makes_the_same_index_decisions(engine, golden):
    """an SSNE.epoch (proximal mutation) with sensitivity_kernel='general' on the inputs of ssne_epoch.npz (fitness, seed) records the
    operator calls of one with 'lds', returns the same elite slot and leaves python's generator at the same place: selection, cloning and
    mutation choices are host draws and do not depend on the scaling"""
    from serl_amd import ssne
    from serl_amd.replay import DeviceReplay
    import serl_amd
    g = golden('ssne_epoch')
    key = sorted(k[:-4] for k in g.files if k.endswith('_ops'))[0]
    m = re.match(r'p(\d+)_e(\d+)_s(\d+)', key)
    pop, elit, seed = int(m.group(1)), int(m.group(2)), int(m.group(3))
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    w0 = np.resize(golden('actors')['serl50'], (pop, golden('actors')['serl50'].shape[1])).copy()
    rows = torch.from_numpy(golden('proximal')['buf_serl50_18'])
    args = types.SimpleNamespace(pop_size=pop, elite_fraction=elit / pop, mutation_prob=0.9, mutation_mag=0.05, mut_type='proximal',
                                 distil_crossover=False, crossover_prob=0.0, mutation_batch_size=86, individual_bs=10_000)
    runs = {}
    for kernel, dense in (('lds', 'valu'), ('general', 'valu'), ('general', 'mfma')):
        bufs, crits = [], []
        for k in range(pop):
            r = DeviceReplay(10_000, engine.device, engine)
            r.append_rows(rows[:300 + 10 * k])
            bufs.append(r)
            crits.append(DeviceReplay(10_000, engine.device, engine))
        w = torch.from_numpy(w0.copy()).to(engine.device)
        rec = []
        random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
        ep = ssne.SSNE(args, engine, spec, record=rec, sensitivity_kernel=kernel, sensitivity_dense=dense)
        assert ep.num_elitists == elit
        ret = ep.epoch(w, g[key + '_fit'], buffers=bufs, critical=crits)
        torch.cuda.synchronize()
        runs[kernel, dense] = (rec, ret, random.random(), w.cpu().numpy())
        assert np.isfinite(runs[kernel, dense][3]).all()
    rec, ret, rnd, _ = runs['lds', 'valu']
    # (the file's own operator list was recorded with the mutations replaced by recorders, which draw nothing: from the first proximal
    # mutation on, whose minibatch comes from python's generator, the decisions of a real epoch are its own -- but the same in every run)
    ops = g[key + '_ops']
    first = next(k for k, r in enumerate(rec) if r[0] == 2)
    np.testing.assert_array_equal(np.array(rec[:first + 1], dtype=np.int64).reshape(-1, 3), ops[:first + 1])
    assert sum(r[0] == 2 for r in rec) >= 2
    for k in (('general', 'valu'), ('general', 'mfma')):
        assert runs[k][:3] == (rec, ret, rnd), k
    np.testing.assert_array_equal(runs['general', 'valu'][3], runs['general', 'mfma'][3])

"""serl_td3_train_group_big / serl_td3_train_group_wide -- groups of independent TD3 learners on minibatches of up to 512 rows, the chunks of
128 samples walked by the learner's one workgroup or spread over workgroups of their own -- against single-learner serl_td3_train_big /
serl_td3_train_wide calls with the generator (the code before these kernels), bit for bit in every array a learner writes: unlike learners
with unlike update counts in both dense flavours with CAPS on and off, serial against parallel, one chunk against serl_td3_train_group,
the learner's place in the grid, split calls, rows a workgroup refuses, launches the host refuses, and serl_amd.TD3Group(chunks=...)
against TD3.train(draws='device', chunks=...).  There is no test of the time-out path: it would mean making workgroups wait on purpose."""
import copy
import ctypes
import time
import numpy as np
import pytest
import torch
import td3_64 as T
import test_gpu_td3 as G
import test_gpu_td3_rng as R
import test_gpu_td3_group as GG

pytestmark = pytest.mark.gpu
OUT, FILL, bits, specs = GG.OUT, GG.FILL, GG.bits, GG.specs
ENTRIES = ('big', 'wide')
# (S, A, hidden, layers, B): two chunks, the last of one sample, on the smallest network; three chunks, the last of one sample; the default
# learner at three chunks; the largest of everything, four full chunks (GG.specs gives it 3 updates at most)
SHAPES = [(2, 1, 4, 0, 129), (7, 3, 20, 2, 257), (7, 3, 72, 3, 300), (16, 4, 128, 4, 512)]
ONE_CHUNK = [(7, 3, 20, 2, B) for B in (1, 86, 128)]
shape_id = lambda s: 'S%dA%d_H%dL%d_B%d' % s


class Group(GG.Group):
    """test_gpu_td3_group.Group for any minibatch up to 512 rows: the workspace of serl_td3_big_work_bytes / serl_td3_wide_work_bytes
    (NaN-filled, the synchronisation blocks included, eight floats of guard behind), the two new group entries, and the single-learner
    serl_td3_train_big / serl_td3_train_wide call the contract names"""

    def __init__(self, engine, shape, sp, nmax=None, entry='big'):
        super().__init__(engine, shape[:4] + (min(shape[4], 128),), sp, nmax)       # (B sizes nothing there but the old entry's workspace)
        self.shape, self.entry = shape, entry
        self.size = self.L.serl_td3_wide_work_bytes if entry == 'wide' else self.L.serl_td3_big_work_bytes
        self.wb = int(self.size(self.K, *shape))
        assert self.wb > 0
        self.work = torch.full((self.wb // 4 + 8,), float('nan'), dtype=torch.float32, device=self.dev)
        self.one_status = torch.full((3,), -7, dtype=torch.int32, device=self.dev)

    def run_group(self, dense, caps, n=None, it0=None, plant=None, nmax=None, loss=None, d=None):
        tb = self.table(n, it0, plant)
        g = self.C.Td3GroupDesc(rows=tb.data_ptr(), status=self.t['status'][1:].data_ptr(), dense=dense, caps=caps)
        d = self.desc(self.nmax if nmax is None else nmax, loss=loss) if d is None else d
        rc = getattr(self.L, 'serl_td3_train_group_' + self.entry)(self.engine.ctx, ctypes.byref(d), ctypes.byref(g), self.stream())
        torch.cuda.synchronize()
        return rc

    def run_single(self, i, dense, caps, n=None, it0=None):
        """learner i alone as the contract words it: the row's values in the descriptor, rng = {seed, n_rows, key}"""
        s = self.sp[i]
        d = self.desc(0, first=i, K=1, single=(s, self.rings[i], s.n if n is None else n, s.it0 if it0 is None else it0))
        d.work_bytes = int(self.size(1, *self.shape))
        rg = self.C.Td3RngDesc(seed=s.seed, n_rows=s.n_rows, learner0=s.key, dense=dense, caps=caps)
        if self.entry == 'wide':
            x = self.C.Td3WideDesc(rng=ctypes.pointer(rg), status=self.one_status[1:].data_ptr(), dense=dense)
            rc = self.L.serl_td3_train_wide(self.engine.ctx, ctypes.byref(d), ctypes.byref(x), self.stream())
        else:
            x = self.C.Td3BigDesc(rng=ctypes.pointer(rg), dense=dense)
            rc = self.L.serl_td3_train_big(self.engine.ctx, ctypes.byref(d), ctypes.byref(x), self.stream())
        torch.cuda.synchronize()
        assert rc == 0, self.L.serl_last_error()
        if self.entry == 'wide':
            assert self.one_status.cpu().tolist() == [-7, 0 if d.n_updates else -7, -7]


_refs = {}


def reference(engine, shape, spec, entry, dense, caps, n=None, it0=None):
    """what learner `spec` writes in a single-learner serl_td3_train_big (entry 'wide': serl_td3_train_wide) call with the generator:
    {array: its row}; computed once per argument set and left unchanged"""
    key = (shape, spec._replace(hp=tuple(sorted(spec.hp.items()))), entry, dense, caps, n, it0)
    if key not in _refs:
        g = Group(engine, shape, [spec], nmax=max(spec.n, n or 0), entry=entry)
        g.run_single(0, dense, caps, n, it0)
        o = g.out()
        for k in OUT:
            np.testing.assert_array_equal(o[k][[0, 2]], g.host[k][[0, 2]], err_msg=k)
        assert torch.isnan(g.work[-8:]).all()
        _refs[key] = {k: o[k][1].copy() for k in OUT}
        for v in _refs[key].values():
            v.setflags(write=False)
    return _refs[key]


def expect(g, refs, status=None):
    o = GG.expect(g, refs, status=[int(s != 0) for s in status] if status is not None else None)
    if status is not None:
        np.testing.assert_array_equal(o['status'], [-9] + list(status) + [-9])
    return o


def same(a, b, what=''):
    for k in OUT + ('status',):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg='%s %s' % (what, k))


# ---- 1. unlike learners with unlike update counts ------------------------------------------------------------------------------------
@pytest.mark.parametrize('caps', [0, 1])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_group_equals_single_learner_calls(engine, shape, entry, dense, caps):
    """0 / 3 / 5 updates (0 / 3 / 3 at hidden 128): in the wide entry the learners' workgroups leave behind different hand-overs.  Every
    written array, the losses past a learner's own count, the guard rows 0 and K + 1, the rings and the guard behind the workspace"""
    sp = specs(shape)[:3]
    assert [s.n for s in sp][:2] == [0, 3] and sp[0].n_rows == shape[4] and sp[2].seed == 2**64 - 1
    g = Group(engine, shape, sp, entry=entry)
    assert g.run_group(dense, caps) == 0, g.L.serl_last_error()
    o = expect(g, [reference(engine, shape, s, entry, dense, caps) for s in sp])
    for k in OUT:                                       # the learner with no updates is as it was, adam_steps included
        np.testing.assert_array_equal(bits(o[k][1]), bits(g.host[k][1]), err_msg=k)
    for i, s in enumerate(sp[1:], 2):
        actor_updates = [u for u in range(s.n) if (s.it0 + u + 1) % s.freq == 0]
        assert np.isfinite(o['td'][i, :s.n]).all() and (o['td'][i, s.n:] == FILL).all()
        for u in range(g.nmax + 2):
            assert (o['pg'][i, u] != FILL) == (u in actor_updates), (i, u)
        np.testing.assert_array_equal(o['steps'][i], [s.n, len(actor_updates)])
        assert actor_updates and np.isfinite(o['actor'][i, :g.Pa]).all() and np.isfinite(o['critic'][i, :g.Pc]).all()
        assert (o['critic'][i, :g.Pc] != g.host['critic'][i, :g.Pc]).any() and (o['actor'][i, :g.Pa] != g.host['actor'][i, :g.Pa]).any()
        assert (o['actor_target'][i, :g.Pa] != g.host['actor_target'][i, :g.Pa]).any() == bool(s.uat), i


# ---- 2. serial chunks equal parallel chunks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_serial_equals_parallel(engine, shape, dense):
    outs = []
    for entry in ENTRIES:
        g = Group(engine, shape, specs(shape)[:3], entry=entry)
        assert g.run_group(dense, 1) == 0, g.L.serl_last_error()
        outs.append(g.out())
    same(outs[0], outs[1], shape_id(shape))
    assert (outs[0]['status'] == [-9, 0, 0, 0, -9]).all()


# ---- 3. one chunk: both entries are serl_td3_train_group --------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('shape', ONE_CHUNK, ids=shape_id)
def test_one_chunk_equals_the_group_kernel(engine, shape, dense):
    sp = specs(shape)[:3]
    old = GG.Group(engine, shape, sp)
    assert old.run_group(dense, 1) == 0, old.L.serl_last_error()
    want = old.out()
    assert (want['status'] == [-9, 0, 0, 0, -9]).all() and (want['steps'][2:4] > 0).all()
    for entry in ENTRIES:
        g = Group(engine, shape, sp, entry=entry)
        assert g.run_group(dense, 1) == 0, g.L.serl_last_error()
        same(want, g.out(), entry)
        assert torch.isnan(g.work[-8:]).all()


# ---- 4. the learner's place in the grid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('entry', ENTRIES)
def test_place_in_the_grid(engine, entry, dense):
    """the same three learners in reversed order, and as learners 0 .. 2 of a launch of five (`first` 0, K 5); then learners 1 .. 3 of
    those five alone, through a descriptor that starts at the second row of every array"""
    shape = SHAPES[1]
    sp = specs(shape)
    for order in (sp[2::-1], sp):
        g = Group(engine, shape, order, entry=entry)
        assert g.run_group(dense, 1) == 0, g.L.serl_last_error()
        expect(g, [reference(engine, shape, s, entry, dense, 1) for s in order])
    pad = Group(engine, shape, sp, entry=entry)
    pad.sp, pad.K, pad.rings = pad.sp[1:4], 3, pad.rings[1:4]
    d = pad.desc(pad.nmax, first=1, K=3)
    tb = pad.table()
    gd = pad.C.Td3GroupDesc(rows=tb.data_ptr(), status=pad.t['status'][2:].data_ptr(), dense=dense, caps=1)
    assert getattr(pad.L, 'serl_td3_train_group_' + entry)(engine.ctx, ctypes.byref(d), ctypes.byref(gd), pad.stream()) == 0
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in pad.t.items()}
    for i, s in enumerate(sp[1:4]):
        r = reference(engine, shape, s, entry, dense, 1)
        for k in OUT:
            np.testing.assert_array_equal(bits(o[k][2 + i, :len(r[k])]), bits(r[k]), err_msg='%s learner %d' % (k, i))
    for k in OUT:                                       # rows 0 and 1 in front of the three and rows 5 and 6 behind them are as they were
        np.testing.assert_array_equal(bits(o[k][[0, 1, 5, 6]]), bits(pad.host[k][[0, 1, 5, 6]]), err_msg=k)
    np.testing.assert_array_equal(o['status'], [-9, -9, 0, 0, 0, -9, -9])


# ---- 5. split calls -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('entry', ENTRIES)
def test_split_calls(engine, entry, dense):
    """group calls of (2, 1, 3) then (3, 2, 0) updates, iteration0 advanced per learner, against single calls of (5, 3, 3)"""
    shape = SHAPES[1]
    sp = [s._replace(n=n) for s, n in zip(specs(shape)[:3], (5, 3, 3))]
    first, second = (2, 1, 3), (3, 2, 0)
    g = Group(engine, shape, sp, entry=entry)
    assert g.run_group(dense, 1, n=first, nmax=3) == 0
    expect(g, [reference(engine, shape, s, entry, dense, 1, n=n) for s, n in zip(sp, first)])
    loss2 = tuple(torch.full_like(g.t[k], FILL) for k in ('td', 'pg'))
    assert g.run_group(dense, 1, n=second, it0=[s.it0 + n for s, n in zip(sp, first)], nmax=3, loss=loss2) == 0
    o = g.out()
    for i, s in enumerate(sp):
        w = reference(engine, shape, s, entry, dense, 1)
        for k in T.ROWS + T.MOMENTS + ('steps',):
            np.testing.assert_array_equal(bits(o[k][1 + i, :len(w[k])]), bits(w[k]), err_msg='%s learner %d' % (k, i))
        for k, second_k in zip(('td', 'pg'), loss2):
            got = np.concatenate([o[k][1 + i, :first[i]], second_k[1 + i, :second[i]].cpu().numpy()])
            np.testing.assert_array_equal(bits(got), bits(w[k][:s.n]), err_msg='%s learner %d' % (k, i))
            assert (second_k[1 + i, second[i]:] == FILL).all()
    np.testing.assert_array_equal(o['status'], [-9, 0, 0, 0, -9])


# ---- 6. rows a workgroup refuses ----------------------------------------------------------------------------------------------------------
CODE = {'ring': 1, 'n_updates': 2, 'iteration0': 3, 'n_rows': 4, 'policy_update_freq': 5, 'lr': 6, 'tau': 6, 'gamma': 6, 'eps_sd': 6}


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('plant', list(enumerate(GG.PLANTS)), ids=lambda p: '%s=%s' % p[1])
def test_refused_rows(engine, plant, entry):
    """the twelve bad rows of the group test, one in a launch of three: its status is the check's code and nothing else of it is written,
    the neighbours end where they end alone.  In the wide entry none of the refused learner's three workgroups is waited for: the launch
    is back long before the 4 s a wait would spin"""
    idx, (field, v) = plant
    shape = SHAPES[1]
    sp = [s._replace(n=max(s.n, 2)) for s in specs(shape)[:3]]
    j, dense = idx % 3, idx % 2
    g = Group(engine, shape, sp, entry=entry)
    v = {'B-1': shape[4] - 1, 'cap+1': sp[j].cap + 1, 'nmax+1': g.nmax + 1}.get(v, v)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert g.run_group(dense, 1, plant=(j, field, v)) == 0
    elapsed = time.perf_counter() - t0
    refs = [None if i == j else reference(engine, shape, s, entry, dense, 1) for i, s in enumerate(sp)]
    expect(g, refs, status=[CODE[field] if i == j else 0 for i in range(3)])
    assert elapsed < 2.0, elapsed
    if entry == 'wide':                                 # the refused learner's synchronisation words are as the launch zeroed them
        words = g.work[:4 * g.K].view(torch.int32).cpu().numpy().reshape(g.K, 4)
        assert (words[j] == 0).all() and (words[:, 2] == 0).all(), words


# ---- 7. launches the host refuses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', ENTRIES)
def test_host_refusals_launch_nothing(engine, entry):
    shape = SHAPES[1]
    g = Group(engine, shape, specs(shape)[:3], entry=entry)
    C, L = g.C, g.L
    fn = getattr(L, 'serl_td3_train_group_' + entry)
    tb = g.table()
    group = lambda **kw: C.Td3GroupDesc(**dict(dict(rows=tb.data_ptr(), status=g.t['status'][1:].data_ptr(), dense=0, caps=1), **kw))
    call = lambda d, gd: fn(engine.ctx, ctypes.byref(d), ctypes.byref(gd) if gd is not None else None, g.stream())
    assert call(g.desc(g.nmax), None) == C.E_INVALID and ('serl_td3_train_group_%s:' % entry).encode() in L.serl_last_error()
    for kw in (dict(rows=None), dict(status=None), dict(dense=2), dict(dense=-1), dict(caps=2)):
        assert call(g.desc(g.nmax), group(**kw)) == C.E_INVALID, kw
    for field, v, rc in (('work_bytes', g.wb - 4, C.E_INVALID), ('batch', 513, C.E_UNSUPPORTED), ('batch', 0, C.E_INVALID), ('hidden', 6, C.E_UNSUPPORTED),
                         ('actor', None, C.E_INVALID), ('n_updates', -1, C.E_INVALID), ('n_learners', 0, C.E_INVALID), ('max_grad_norm', 0.0, C.E_INVALID),
                         ('loss_stride', g.nmax - 1, C.E_INVALID)):
        d = g.desc(g.nmax)
        setattr(d, field, v)
        assert call(d, group()) == rc, field
        assert ('serl_td3_train_group_%s:' % entry).encode() in L.serl_last_error()
    if entry == 'wide':
        # more workgroups than CUs: n_learners x 3 chunks (nothing of the other learners is looked at before the refusal); the chunked
        # entry's workspace is too small
        cus = torch.cuda.get_device_properties(engine.device).multi_processor_count
        d = g.desc(g.nmax); d.n_learners = cus // 3 + 1; d.work_bytes = 1 << 40
        assert call(d, group()) == C.E_UNSUPPORTED and b'CU' in L.serl_last_error()
        d = g.desc(g.nmax); d.work_bytes = int(L.serl_td3_big_work_bytes(3, *shape))
        assert call(d, group()) == C.E_INVALID
    torch.cuda.synchronize()
    o = g.out()
    for k, v in g.host.items():
        np.testing.assert_array_equal(bits(o[k]), bits(v), err_msg=k)
    assert torch.isnan(g.work).all()


# ---- 8. through serl_amd.TD3Group ----------------------------------------------------------------------------------------------------------
def _learners(engine, B, H, Ly):
    import serl_amd
    S, A = 7, 3
    fills = [(B, B), (B + 40, B + 64), (B + 9, B + 9)]
    out = []
    for i in range(3):
        torch.manual_seed(5 + i)
        a = G._args(S, A, H, Ly, 'tanh', B, 'cpu')
        a.lr, a.gamma, a.tau, a.policy_update_freq = (T.LR, 5e-4, 3e-3)[i], (T.GAMMA, 0.9, 0.99)[i], (T.TAU, 0.2, 0.01)[i], (2, 2, 3)[i]
        a.noise_sd, a.noise_clip = (T.NOISE_SD, 0.4, 0.1)[i], (T.NOISE_CLIP, 0.3, 1.0)[i]
        t = serl_amd.TD3(a, engine)
        if i == 1:
            t.caps_dict = dict(lambda_s=0.25, lambda_t=0.3, eps_sd=0.1)
        ring = serl_amd.DeviceReplay(fills[i][1], engine.device, engine, S, A)
        ring.append_rows(torch.from_numpy(R._ring(S, A, fills[i][0], fills[i][0])))
        out.append((t, ring))
    return out


def _same_learner(a, b, what):
    sa, sb = R._state(a), R._state(b)
    for k in sa:
        np.testing.assert_array_equal(bits(sa[k]), bits(sb[k]), err_msg='%s %s' % (k, what))
    for x, y in ((a.actor_optim, b.actor_optim), (a.critic_optim, b.critic_optim)):
        sx, sy = x.state_dict()['state'], y.state_dict()['state']
        assert sx.keys() == sy.keys(), what
        for j in sx:
            assert float(sx[j]['step']) == float(sy[j]['step'])
            assert torch.equal(sx[j]['exp_avg'], sy[j]['exp_avg']) and torch.equal(sx[j]['exp_avg_sq'], sy[j]['exp_avg_sq'])
    for m in ('actor', 'actor_target', 'critic', 'critic_target'):
        da, db = getattr(a, m).state_dict(), getattr(b, m).state_dict()
        assert da.keys() == db.keys() and all(torch.equal(da[k], db[k]) for k in da), (m, what)


@pytest.mark.parametrize('dense', ['valu', 'mfma'])
@pytest.mark.parametrize('chunks', ['serial', 'parallel'])
@pytest.mark.parametrize('B,H,Ly', [(129, 20, 2), (300, 72, 3)], ids=['B129', 'B300'])
def test_td3_group_train_chunks(engine, B, H, Ly, chunks, dense):
    """three TD3 objects through TD3Group.train(chunks=...) against deep copies trained one by one with
    TD3.train(draws='device', seed, learner=key, dense, chunks): modules, Adam state, the returned losses, last_path"""
    import serl_amd
    grouped = _learners(engine, B, H, Ly)
    alone = [(copy.deepcopy(t, {id(engine): engine}), ring) for t, ring in grouped]            # (the engine is shared, not copied)
    assert all(u.engine is engine and u is not t for (t, _), (u, _) in zip(grouped, alone))
    seeds, keys = [77, 77, 2**64 - 1], [3, 4, 3]
    n, it0, champ = [4, 0, 3], [0, 6, 3], [False, True, False]
    got = serl_amd.TD3Group([t for t, _ in grouped]).train([r for _, r in grouped], n, iteration0=it0, seed=seeds, key=keys, champion_target=champ,
                                                           dense=dense, chunks=chunks)
    path = 'fused%s-%s-group-rng' % ('-mfma' if dense == 'mfma' else '', 'wide' if chunks == 'parallel' else 'big')
    for i, (u, ring) in enumerate(alone):
        want = u.train(ring, n[i], iteration0=it0[i], champion_target=champ[i], draws='device', seed=seeds[i], learner=keys[i], dense=dense, chunks=chunks)
        assert set(got[i]) == {'PG_obj', 'TD_loss'}
        for k in want:
            np.testing.assert_array_equal(np.float64(got[i][k]).view(np.uint64), np.float64(want[k]).view(np.uint64), err_msg='%s learner %d' % (k, i))
        assert grouped[i][0].last_path == path
        assert n[i] == 0 or u.last_path == path.replace('-group', '')
        _same_learner(grouped[i][0], u, 'learner %d' % i)
    assert [R._state(t)['steps'].tolist() for t, _ in grouped] == [[4, 2], [0, 0], [3, 1]]


def test_td3_group_train_default_is_todays_call(engine):
    """batch_size 86 with the default `chunks`: serl_td3_train_group and its last_path; chunks='parallel' names the wide entry"""
    import serl_amd
    for chunks, path in ((None, 'fused-group-rng'), ('parallel', 'fused-wide-group-rng')):
        pairs = _learners(engine, 86, 20, 2)
        kw = {} if chunks is None else dict(chunks=chunks)
        out = serl_amd.TD3Group([t for t, _ in pairs]).train([r for _, r in pairs], 2, iteration0=0, seed=5, **kw)
        assert [t.last_path for t, _ in pairs] == [path] * 3 and all(np.isfinite(o['TD_loss']) for o in out)

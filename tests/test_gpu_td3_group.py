"""serl_td3_train_group -- K independent TD3 learners in one launch, each with its own ring, fill, update count, iteration, seed, key and
hyper-parameters, read from a device row -- against K single-learner serl_td3_train_rng calls (the code before the group kernels), bit
for bit in every array a learner writes: a heterogeneous launch in both dense flavours with CAPS on and off, the learner's place in the
grid, split calls, rows a workgroup refuses, launches the host refuses, and serl_amd.TD3Group against TD3.train(draws='device')."""
import collections
import ctypes
import numpy as np
import pytest
import torch
import td3_64 as T
import test_gpu_td3 as G
import test_gpu_td3_rng as R

pytestmark = pytest.mark.gpu
OUT = T.ROWS + T.MOMENTS + ('td', 'pg', 'steps')
FILL = -3.5             # td / pg before a launch
# (S, A, hidden, layers, B): a small odd one (two hidden layers, a minibatch of one wavefront's quarter plus one); the smallest of
# everything (no hidden layer, one sample); the largest of everything; the default learner
SHAPES = [(7, 3, 20, 2, 17), (2, 1, 4, 0, 1), (16, 3, 128, 4, 128), (7, 3, 72, 3, 86)]
Spec = collections.namedtuple('Spec', 'wseed n_rows cap n it0 freq uat hp seed key')
HP = [dict(lr=2e-3, gamma=0.98, tau=0.05, noise_sd=0.2, noise_clip=0.5, lambda_s=0.5, lambda_t=0.1, eps_sd=0.05),
      dict(lr=5e-4, gamma=0.9, tau=0.2, noise_sd=0.4, noise_clip=0.3, lambda_s=0.25, lambda_t=0.3, eps_sd=0.1),
      dict(lr=4e-3, gamma=0.995, tau=1.0, noise_sd=0.1, noise_clip=1.0, lambda_s=1.0, lambda_t=0.05, eps_sd=0.02)]


def specs(shape):
    """three learners that differ in everything a row holds -- a ring filled to exactly one minibatch with 0 updates, a full ring, a part-filled
    one; iteration0 0, 1, 7 with the actor every 2nd, 2nd, 3rd iteration; actor target updated, frozen, updated -- and two more to pad a grid"""
    B = shape[4]
    n = (0, 3, 3) if shape[2] == 128 else (0, 3, 5)
    return [Spec(11, B, B + 3, n[0], 0, 2, 1, HP[0], 0x9E3779B97F4A7C15, 4),
            Spec(12, B + 9, B + 9, n[1], 1, 2, 0, HP[1], 77, 0),
            Spec(13, B + 20, 2 * B + 40, n[2], 7, 3, 1, HP[2], 2**64 - 1, 2**31 - 2),
            Spec(14, B + 5, B + 6, 2, 3, 1, 1, HP[1], 77, 1),
            Spec(15, B + 1, B + 30, 1, 0, 2, 1, HP[0], 5, 0)]


_cases = {}


def _case(shape, wseed):
    if (shape, wseed) not in _cases:
        S, A, H, L, B = shape
        d = T.make_case((S, A, H, L, 'tanh', 8, 2, 0, 6, 1, 1, 'small'), seed=wseed)
        _cases[(shape, wseed)] = {k: d[k] for k in T.ROWS}
    return _cases[(shape, wseed)]


class Group:
    """device buffers of the learners `sp` of one shape: rows 1 .. K of every per-learner array (row 0 and row K + 1 are guards), one ring
    each (NaN behind the filled part), and calls of the group entry and of the single-learner generator entry on them"""

    def __init__(self, engine, shape, sp, nmax=None):
        from serl_amd import _capi
        self.C, self.L, self.engine, self.dev = _capi, _capi.lib(), engine, engine.device
        self.shape, self.sp, self.K = shape, list(sp), len(sp)
        S, A, H, Ly, B = shape
        K = self.K
        self.nmax = max(s.n for s in sp) if nmax is None else nmax
        host = {}
        for i, s in enumerate(sp):
            d = _case(shape, s.wseed)
            for k in T.ROWS + T.MOMENTS:
                P = len(d[k.split('_')[0]])
                host.setdefault(k, np.full((K + 2, P + 5), 7.25, np.float32))[1 + i, :P] = d[k] if k in d else 0.0
        self.Pa, self.Pc = len(d['actor']), len(d['critic'])
        host['steps'] = np.zeros((K + 2, 2), np.int32)
        host['td'] = np.full((K + 2, self.nmax + 2), FILL, np.float32)
        host['pg'] = np.full((K + 2, self.nmax + 2), FILL, np.float32)
        host['status'] = np.full(K + 2, -9, np.int32)
        self.host = host
        self.t = {k: torch.from_numpy(v).to(self.dev) for k, v in host.items()}
        self.rings = [torch.from_numpy(R._ring(S, A, s.n_rows, s.cap)).to(self.dev) for s in sp]
        self.wb = int(self.L.serl_td3_work_bytes(K, S, A, H, Ly, B))
        assert self.wb > 0
        self.work = torch.full((self.wb // 4 + 8,), float('nan'), dtype=torch.float32, device=self.dev)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def desc(self, n, first=0, K=None, single=None, loss=None):
        """the group form: everything a row holds left zero / NULL.  single = (spec, ring, n, it0): the single-learner form of that spec"""
        S, A, H, Ly, B = self.shape
        t = self.t
        td, pg = loss if loss is not None else (t['td'], t['pg'])
        p = lambda x, *idx: x[idx].data_ptr()
        d = self.C.Td3Desc(
            state_dim=S, action_dim=A, hidden=H, num_layers=Ly, activation=0, n_learners=self.K if K is None else K, batch=B, n_updates=n,
            max_grad_norm=T.MAX_NORM, actor=p(t['actor'], 1 + first), actor_target=p(t['actor_target'], 1 + first), actor_m=p(t['actor_m'], 1 + first),
            actor_v=p(t['actor_v'], 1 + first), actor_stride=t['actor'].stride(0), critic=p(t['critic'], 1 + first),
            critic_target=p(t['critic_target'], 1 + first), critic_m=p(t['critic_m'], 1 + first), critic_v=p(t['critic_v'], 1 + first),
            critic_stride=t['critic'].stride(0), adam_steps=p(t['steps'], 1 + first), td_loss=p(td, 1 + first), pg_loss=p(pg, 1 + first),
            loss_stride=td.stride(0), work=self.work.data_ptr(), work_bytes=self.wb)
        if single is not None:
            s, ring, n1, it0 = single
            d.n_updates, d.capacity, d.policy_update_freq, d.iteration0, d.update_actor_target = n1, s.cap, s.freq, it0, s.uat
            d.ring = ring.data_ptr()
            for k, v in s.hp.items():
                setattr(d, k, v)
        return d

    def table(self, n=None, it0=None, plant=None):
        """the rows on the device.  n / it0: per-learner overrides; plant = (learner, field, value)"""
        rows = (self.C.Td3LearnerRow * self.K)()
        for i, s in enumerate(self.sp):
            rows[i] = self.C.Td3LearnerRow(ring=self.rings[i].data_ptr(), seed=s.seed, capacity=s.cap, n_rows=s.n_rows,
                                           n_updates=s.n if n is None else n[i], iteration0=s.it0 if it0 is None else it0[i], key=s.key,
                                           policy_update_freq=s.freq, update_actor_target=s.uat, **s.hp)
        if plant is not None:
            setattr(rows[plant[0]], plant[1], plant[2])
        return torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(self.dev)

    def run_group(self, dense, caps, n=None, it0=None, plant=None, nmax=None, loss=None):
        tb = self.table(n, it0, plant)
        g = self.C.Td3GroupDesc(rows=tb.data_ptr(), status=self.t['status'][1:].data_ptr(), dense=dense, caps=caps)
        rc = self.L.serl_td3_train_group(self.engine.ctx, ctypes.byref(self.desc(self.nmax if nmax is None else nmax, loss=loss)), ctypes.byref(g),
                                         self.stream())
        torch.cuda.synchronize()
        return rc

    def run_single(self, i, dense, caps, n=None, it0=None):
        """learner i alone through serl_td3_train_rng, as the contract words it: the row's values in the descriptor, rng = {seed, n_rows, key}"""
        s = self.sp[i]
        d = self.desc(0, first=i, K=1, single=(s, self.rings[i], s.n if n is None else n, s.it0 if it0 is None else it0))
        d.work_bytes = int(self.L.serl_td3_work_bytes(1, *self.shape))
        rg = self.C.Td3RngDesc(seed=s.seed, n_rows=s.n_rows, learner0=s.key, dense=dense, caps=caps)
        rc = self.L.serl_td3_train_rng(self.engine.ctx, ctypes.byref(d), ctypes.byref(rg), self.stream())
        torch.cuda.synchronize()
        assert rc == 0, self.L.serl_last_error()

    def out(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}


_refs = {}


def reference(engine, shape, spec, dense, caps, n=None, it0=None):
    """what learner `spec` writes in a single-learner serl_td3_train_rng call: {array: its row}; computed once per argument set"""
    key = (shape, spec._replace(hp=tuple(sorted(spec.hp.items()))), dense, caps, n, it0)
    if key not in _refs:
        g = Group(engine, shape, [spec], nmax=max(spec.n, n or 0))
        g.run_single(0, dense, caps, n, it0)
        o = g.out()
        for k in OUT:
            np.testing.assert_array_equal(o[k][[0, 2]], g.host[k][[0, 2]], err_msg=k)
        _refs[key] = {k: o[k][1].copy() for k in OUT}
    return _refs[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def expect(g, refs, status=None):
    """the group's buffers must be, bit for bit, their initial contents with learner i's rows replaced by refs[i] (None: left as they were)"""
    o = g.out()
    for k in OUT:
        want = g.host[k].copy()
        for i, r in enumerate(refs):
            if r is not None:
                want[1 + i, :len(r[k])] = r[k]
        np.testing.assert_array_equal(bits(o[k]), bits(want), err_msg=k)
    want = np.array([-9] + list(status if status is not None else [0] * g.K) + [-9])
    if status is None:
        np.testing.assert_array_equal(o['status'], want)
    else:
        assert ((o['status'] != 0) == (want != 0)).all() and (o['status'][[0, -1]] == -9).all(), o['status']
    for i, ring in enumerate(g.rings):
        np.testing.assert_array_equal(bits(ring.cpu().numpy()), bits(R._ring(g.shape[0], g.shape[1], g.sp[i].n_rows, g.sp[i].cap)))
    assert torch.isnan(g.work[-8:]).all()
    return o


@pytest.mark.parametrize('caps', [0, 1])
@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'S%dA%d_H%dL%d_B%d' % s)
def test_heterogeneous_launch_equals_single_learner_calls(engine, shape, dense, caps):
    sp = specs(shape)[:3]
    g = Group(engine, shape, sp)
    assert g.run_group(dense, caps) == 0, g.L.serl_last_error()
    refs = [reference(engine, shape, s, dense, caps) for s in sp]
    o = expect(g, refs)
    # the learner with no updates is as it was; the others moved, stayed finite, and their losses sit where their own schedule puts them
    for k in OUT:
        np.testing.assert_array_equal(bits(o[k][1]), bits(g.host[k][1]), err_msg=k)
    for i, s in enumerate(sp[1:], 2):
        actor_updates = [u for u in range(s.n) if (s.it0 + u + 1) % s.freq == 0]
        assert np.isfinite(o['td'][i, :s.n]).all() and (o['td'][i, s.n:] == FILL).all()
        for u in range(g.nmax + 2):
            assert (o['pg'][i, u] != FILL) == (u in actor_updates), (i, u)
        np.testing.assert_array_equal(o['steps'][i], [s.n, len(actor_updates)])
        assert actor_updates and np.isfinite(o['actor'][i, :g.Pa]).all() and np.isfinite(o['critic'][i, :g.Pc]).all()
        assert (o['critic'][i, :g.Pc] != g.host['critic'][i, :g.Pc]).any() and (o['actor'][i, :g.Pa] != g.host['actor'][i, :g.Pa]).any()
        moved = (o['actor_target'][i, :g.Pa] != g.host['actor_target'][i, :g.Pa]).any()
        assert moved == bool(s.uat), i


@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
def test_place_in_the_grid(engine, dense):
    """the same three learners in reversed order, and as learners 0 .. 2 of a launch of five"""
    shape = SHAPES[0]
    sp = specs(shape)
    for order in (sp[2::-1], sp):
        g = Group(engine, shape, order)
        assert g.run_group(dense, 1) == 0
        expect(g, [reference(engine, shape, s, dense, 1) for s in order])


@pytest.mark.parametrize('dense', [0, 1], ids=['valu', 'mfma'])
def test_split_calls(engine, dense):
    """group calls of (2, 1, 3) then (3, 2, 0) updates, iteration0 advanced per learner, against single calls of (5, 3, 3): rows, moments and
    Adam counts carried over; the losses of the second call are those of the single call from the first call's count on"""
    shape = SHAPES[0]
    sp = [s._replace(n=n) for s, n in zip(specs(shape)[:3], (5, 3, 3))]
    first, second = (2, 1, 3), (3, 2, 0)
    g = Group(engine, shape, sp)
    assert g.run_group(dense, 1, n=first, nmax=3) == 0
    part = [reference(engine, shape, s, dense, 1, n=n) for s, n in zip(sp, first)]
    expect(g, part)
    loss2 = tuple(torch.full_like(g.t[k], FILL) for k in ('td', 'pg'))
    assert g.run_group(dense, 1, n=second, it0=[s.it0 + n for s, n in zip(sp, first)], nmax=3, loss=loss2) == 0
    o = g.out()
    whole = [reference(engine, shape, s, dense, 1) for s in sp]
    for i, (s, w) in enumerate(zip(sp, whole)):
        for k in T.ROWS + T.MOMENTS + ('steps',):
            np.testing.assert_array_equal(bits(o[k][1 + i, :len(w[k])]), bits(w[k]), err_msg='%s learner %d' % (k, i))
        for k, second_k in zip(('td', 'pg'), loss2):
            got = np.concatenate([o[k][1 + i, :first[i]], second_k[1 + i, :second[i]].cpu().numpy()])
            np.testing.assert_array_equal(bits(got), bits(w[k][:s.n]), err_msg='%s learner %d' % (k, i))
            assert (second_k[1 + i, second[i]:] == FILL).all()
    np.testing.assert_array_equal(o['status'], [-9, 0, 0, 0, -9])


PLANTS = [('n_rows', 'B-1'), ('n_rows', 'cap+1'), ('n_updates', -1), ('n_updates', 'nmax+1'), ('ring', None), ('policy_update_freq', 0),
          ('lr', 0.0), ('tau', 1.5), ('iteration0', -1), ('iteration0', 2**31 - 3), ('gamma', float('nan')), ('eps_sd', -0.5)]


@pytest.mark.parametrize('plant', list(enumerate(PLANTS)), ids=lambda p: '%s=%s' % p[1])
def test_refused_rows(engine, plant):
    """one bad row in a launch of three: its status is non-zero and nothing else of it is written, the neighbours run as if alone.  (The
    issue's eight cases, then four more of the same checks: a negative and an overflowing iteration, a NaN, a negative eps_sd.)"""
    idx, (field, v) = plant
    shape = SHAPES[0]
    sp = [s._replace(n=max(s.n, 2)) for s in specs(shape)[:3]]
    j, dense = idx % 3, idx % 2
    g = Group(engine, shape, sp)
    v = {'B-1': shape[4] - 1, 'cap+1': sp[j].cap + 1, 'nmax+1': g.nmax + 1}.get(v, v)
    assert g.run_group(dense, 1, plant=(j, field, v)) == 0
    refs = [None if i == j else reference(engine, shape, s, dense, 1) for i, s in enumerate(sp)]
    expect(g, refs, status=[int(i == j) for i in range(3)])


def test_launch_wide_refusals_launch_nothing(engine):
    shape = SHAPES[0]
    g = Group(engine, shape, specs(shape)[:3])
    C, L = g.C, g.L
    tb = g.table()
    group = lambda **kw: C.Td3GroupDesc(**dict(dict(rows=tb.data_ptr(), status=g.t['status'][1:].data_ptr(), dense=0, caps=1), **kw))
    call = lambda d, gd: L.serl_td3_train_group(engine.ctx, ctypes.byref(d), ctypes.byref(gd) if gd is not None else None, g.stream())
    assert call(g.desc(g.nmax), None) == C.E_INVALID
    for kw in (dict(rows=None), dict(status=None), dict(dense=2), dict(dense=-1), dict(caps=2)):
        assert call(g.desc(g.nmax), group(**kw)) == C.E_INVALID, kw
    for field, v, rc in (('hidden', 6, C.E_UNSUPPORTED), ('batch', 129, C.E_UNSUPPORTED), ('work_bytes', g.wb - 1, C.E_INVALID),
                         ('actor', None, C.E_INVALID), ('n_updates', -1, C.E_INVALID), ('n_learners', 0, C.E_INVALID), ('max_grad_norm', 0.0, C.E_INVALID),
                         ('loss_stride', g.nmax - 1, C.E_INVALID)):
        d = g.desc(g.nmax)
        setattr(d, field, v)
        assert call(d, group()) == rc, field
        rg = C.Td3RngDesc(seed=1, n_rows=shape[4], learner0=0, dense=0, caps=1)          # the code of serl_td3_train_rng for the same descriptor
        s = g.sp[1]
        d1 = g.desc(g.nmax, single=(s, g.rings[1], g.nmax, 0))
        setattr(d1, field, v)
        assert L.serl_td3_train_rng(engine.ctx, ctypes.byref(d1), ctypes.byref(rg), g.stream()) == rc, field
    torch.cuda.synchronize()
    o = g.out()
    for k, v in g.host.items():
        np.testing.assert_array_equal(bits(o[k]), bits(v), err_msg=k)
    assert torch.isnan(g.work).all()


@pytest.mark.parametrize('dense', ['valu', 'mfma'])
def test_td3_group_train(engine, dense):
    """three TD3 objects through TD3Group.train, twice, against twins trained one by one with TD3.train(draws='device', seed, learner=key)"""
    import serl_amd
    dev = engine.device
    S, A, H, Ly, B = 7, 3, 20, 2, 17
    fills = [(17, 17), (40, 64), (26, 26)]
    seeds, keys = [77, 77, 2**63 + 5], [3, 4, 3]
    calls = [dict(n=[4, 0, 5], it0=[0, 6, 3], champ=[False, True, False]), dict(n=[2, 3, 1], it0=[4, 6, 8], champ=False)]

    def learners():
        out = []
        for i in range(3):
            torch.manual_seed(5 + i)
            a = G._args(S, A, H, Ly, 'tanh', B, 'cpu')
            a.lr, a.gamma, a.tau, a.policy_update_freq = (T.LR, 5e-4, 3e-3)[i], (T.GAMMA, 0.9, 0.99)[i], (T.TAU, 0.2, 0.01)[i], (2, 2, 3)[i]
            a.noise_sd, a.noise_clip = (T.NOISE_SD, 0.4, 0.1)[i], (T.NOISE_CLIP, 0.3, 1.0)[i]
            t = serl_amd.TD3(a, engine)
            if i == 1:
                t.caps_dict = dict(lambda_s=0.25, lambda_t=0.3, eps_sd=0.1)
            ring = serl_amd.DeviceReplay(fills[i][1], dev, engine, S, A)
            ring.append_rows(torch.from_numpy(R._ring(S, A, fills[i][0], fills[i][0])))
            out.append((t, ring))
        return out

    grouped, alone = learners(), learners()
    group = serl_amd.TD3Group([t for t, _ in grouped])
    for c in calls:
        got = group.train([r for _, r in grouped], c['n'], iteration0=c['it0'], seed=seeds, key=keys, champion_target=c['champ'], dense=dense)
        assert len(got) == 3
        for i, (t, ring) in enumerate(alone):
            champ = c['champ'][i] if isinstance(c['champ'], list) else c['champ']
            want = t.train(ring, c['n'][i], iteration0=c['it0'][i], champion_target=champ, draws='device', seed=seeds[i], learner=keys[i], dense=dense)
            assert set(got[i]) == {'PG_obj', 'TD_loss'}
            for k in want:
                np.testing.assert_array_equal(np.float64(got[i][k]).view(np.uint64), np.float64(want[k]).view(np.uint64), err_msg='%s learner %d' % (k, i))
            assert grouped[i][0].last_path == ('fused-mfma-group-rng' if dense == 'mfma' else 'fused-group-rng')
            a, b = R._state(grouped[i][0]), R._state(t)
            for k in a:
                np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg='%s learner %d' % (k, i))
            for x, y in ((grouped[i][0].actor_optim, t.actor_optim), (grouped[i][0].critic_optim, t.critic_optim)):
                sx, sy = x.state_dict()['state'], y.state_dict()['state']
                assert sx.keys() == sy.keys()
                for j in sx:
                    assert float(sx[j]['step']) == float(sy[j]['step'])
                    assert torch.equal(sx[j]['exp_avg'], sy[j]['exp_avg']) and torch.equal(sx[j]['exp_avg_sq'], sy[j]['exp_avg_sq'])
            for m in ('actor', 'actor_target', 'critic', 'critic_target'):
                sa, sb = getattr(grouped[i][0], m).state_dict(), getattr(t, m).state_dict()
                assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa), (m, i)
    steps = [R._state(t)['steps'].tolist() for t, _ in grouped]
    assert steps == [[6, 3], [3, 1], [6, 2]], steps

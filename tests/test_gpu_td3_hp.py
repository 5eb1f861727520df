"""The fused TD3 learner across the hyper-parameters and the warm optimiser state it accepts (tests/td3_hp.py): serl_td3_train against
the float64 contract at every grid point; what the edge values imply exactly (tau 0, gamma 0, noise_sd 0, noise_clip 0, eps_sd 0), as
pairs of launches compared bit for bit; slots outside [0, capacity) against their clamped values on a ring with NaN on either side; every
other flavour -- mfma, rng, big, wide, the three group entries -- at the reference's defaults and at a combined edge on a warm
optimiser; TD3.train and TD3Group.train away from the default arguments; learners that share ring, slots and both noise tables."""
import ctypes
import functools
import random
import numpy as np
import pytest
import torch
import td3_64 as T
import td3_hp as H
import test_gpu_td3 as G
import test_gpu_td3_rng as R
import test_gpu_td3_big as GB
import test_gpu_td3_wide as GW
import test_gpu_td3_group as GG
import test_gpu_td3_group_big as GGB

pytestmark = pytest.mark.gpu
OUT = T.ROWS + T.MOMENTS + ('td', 'pg', 'steps')
HP_FIELDS = ('lr', 'gamma', 'tau', 'noise_sd', 'noise_clip', 'lambda_s', 'lambda_t', 'eps_sd')
I32_MIN, I32_MAX = -2**31, 2**31 - 1


@functools.lru_cache(maxsize=None)
def _case(c):
    d = H.make_case(c)
    return d, T.td3_literal(d, **H.state_of(d))


@functools.lru_cache(maxsize=None)
def _flavour(point, big=False):
    d = H.make_flavour_case(point, big)
    return d, T.td3_literal(d, **H.state_of(d))


class _WithState:
    """over a Launch of the older test files: the hyper-parameters of the first case's 'hp' instead of td3_64's constants in every
    descriptor, each case's 'steps0' in adam_steps (its moment rows, where it has some, are taken by the base class), and `over`:
    descriptor fields set last (a ring placed by the test, strides of 0)"""

    def __init__(self, engine, cases, **kw):
        super().__init__(engine, cases, **kw)
        self.over = {}
        for i, d in enumerate(cases):
            self.host['steps'][1 + i] = d.get('steps0', (0, 0))
        self.host['steps'][[0, -1]] = 0
        self.t['steps'] = torch.from_numpy(self.host['steps']).to(self.engine.device)

    def desc(self, *a, **kw):
        d = super().desc(*a, **kw)
        hp = self.cases[0].get('hp', T.DEFAULT_HP)
        for k in HP_FIELDS:
            setattr(d, k, hp[k])
        d.max_grad_norm = hp['max_norm']
        for k, v in self.over.items():
            setattr(d, k, v)
        return d

    def place_ring(self, pad=3):
        """the learners' rings with exactly `capacity` = their own rows each, inside a NaN-filled buffer with `pad` rows of NaN in front
        of and behind every one: a read outside [0, capacity) shows as NaN in every output instead of faulting"""
        rows = np.stack([d['ring'] for d in self.cases])
        K, cap, W = rows.shape
        buf = np.full((K, cap + 2 * pad, W), np.nan, np.float32)
        buf[:, pad:pad + cap] = rows
        self.ring_host, self.ring_buf = buf, torch.from_numpy(buf).to(self.engine.device)
        self.over.update(ring=self.ring_buf[0, pad].data_ptr(), ring_stride=self.ring_buf.stride(0), capacity=cap)
        return cap

    def steps_of(self, o, i=0):
        return o['steps'][1 + i].tolist()


class Launch(_WithState, G.Launch):
    def run(self, fn='serl_td3_train', **kw):
        d0 = self.cases[0]
        kw.setdefault('n', self.n)
        kw.setdefault('it0', d0['it0'])
        rc = getattr(self.L, fn)(self.engine.ctx, ctypes.byref(self.desc(**kw)), ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        torch.cuda.synchronize()
        return rc


class BigLaunch(_WithState, GB.Launch):
    pass


class WideLaunch(_WithState, GW.Launch):
    pass


def _same(a, b, what='', keys=OUT):
    for k in keys:
        np.testing.assert_array_equal(GG.bits(a[k]), GG.bits(b[k]), err_msg='%s %s' % (what, k))


def _finite(la, o):
    for i in range(la.K):
        r = la.result(o, i)
        for k in T.ROWS + T.MOMENTS + ('td',):
            assert np.isfinite(r[k]).all(), (i, k)


# ---- a. serl_td3_train against float64 at every grid point ----------------------------------------------------------------------------
_worst = {}


@pytest.mark.parametrize('c', H.CASES, ids=H.case_id)
def test_td3_kernel_vs_float64_across_hyper_parameters(engine, c):
    """rows, targets, moments, td_loss[0] and the first pg_loss within the case's bound of the float64 run with the same hyper-parameters,
    step counts and (f32) moments; guards, inputs and spare columns untouched; adam_steps = steps0 + the steps taken"""
    d, ref = _case(c)
    la = Launch(engine, [d])
    assert la.run() == 0, la.L.serl_last_error()
    o = la.out()
    got = la.result(o, 0)
    dev = T.check(got, ref, d, H.case_id(c), tol=H.tol_of(c, d['act']))
    la.assert_guards(o)
    assert la.steps_of(o) == H.steps_taken(d)
    np.testing.assert_allclose(got['td'], ref['td'], rtol=2e-3, atol=1e-5)
    w = max(dev[k] for k in T.ROWS)
    if w > _worst.get(d['act'], (0, ''))[0]:
        _worst[d['act']] = (w, H.case_id(c))
    print('TD3_HP_WORST so far: %s' % ' '.join('%s %.2g (%s)' % (a, v, n) for a, (v, n) in sorted(_worst.items())))


# ---- b. what the edge values imply, bit for bit --------------------------------------------------------------------------------------
def _run(engine, d):
    la = Launch(engine, [d])
    assert la.run() == 0, la.L.serl_last_error()
    o = la.out()
    _finite(la, o)
    return la, o


def _other_draws(d, seed=99):
    rng = np.random.default_rng(seed)
    return dict(tn=(3.0 * rng.standard_normal(d['tn'].shape)).astype(np.float32), cn=rng.random(d['cn'].shape).astype(np.float32))


@pytest.mark.parametrize('c', [c for c in H.CASES if c[0] == 'tau0'], ids=H.case_id)
def test_tau_0_leaves_both_targets_as_given(engine, c):
    d, _ = _case(c)
    la, o = _run(engine, d)
    for k, P in (('critic_target', la.Pc), ('actor_target', la.Pa)):
        np.testing.assert_array_equal(GG.bits(o[k][1, :P]), GG.bits(la.host[k][1, :P]), err_msg=k)
    assert (o['critic'][1, :la.Pc] != la.host['critic'][1, :la.Pc]).any() and (o['actor'][1, :la.Pa] != la.host['actor'][1, :la.Pa]).any()


@pytest.mark.parametrize('c', [c for c in H.CASES if c[0] == 'tau1'], ids=H.case_id)
def test_tau_1_targets_against_their_networks(engine, c):
    """held by the float64 bound (section a); whether target == network bit for bit depends on how the soft update is written
    (t * (1 - tau) + p * tau gives p + 0 * t): the finding is printed, not asserted.  One update fewer than the case has, so that the
    call ends on an actor update: the last thing done to every row is the soft update"""
    d, _ = _case(c)
    la = Launch(engine, [d], n=d['n'] - 1)
    assert (d['it0'] + d['n'] - 1) % d['freq'] == 0 and la.run() == 0, la.L.serl_last_error()
    o = la.out()
    _finite(la, o)
    for k, P in (('critic', la.Pc), ('actor', la.Pa)):
        same = np.array_equal(GG.bits(o[k][1, :P]), GG.bits(o[k + '_target'][1, :P]))
        print('TD3_HP_TAU1 %s: %s_target %s its network bit for bit (max |difference| %.3g)'
              % (H.case_id(c), k, 'equals' if same else 'differs from', np.abs(o[k][1, :P] - o[k + '_target'][1, :P]).max()))
        np.testing.assert_allclose(o[k + '_target'][1, :P], o[k][1, :P], rtol=0, atol=1e-6)


@pytest.mark.parametrize('c', [c for c in H.CASES if c[0] == 'gamma0'], ids=H.case_id)
def test_gamma_0_ignores_the_targets_and_their_noise(engine, c):
    """other (finite) critic_target, actor_target and target_noise: critic, its moments and td_loss do not change"""
    d, _ = _case(c)
    e = H.make_case(c, 1)
    d2 = dict(d, critic_target=e['critic_target'], actor_target=e['actor_target'], tn=_other_draws(d)['tn'])
    assert (d2['critic_target'] != d['critic_target']).any() and (d2['actor_target'] != d['actor_target']).any()
    (_, a), (_, b) = _run(engine, d), _run(engine, d2)
    _same(a, b, H.case_id(c), ('critic', 'critic_m', 'critic_v', 'td'))
    assert (a['critic_target'] != b['critic_target']).any()


@pytest.mark.parametrize('c', [c for c in H.CASES if c[0] in ('noise_sd0', 'noise_clip0', 'eps_sd0')], ids=H.case_id)
def test_a_zero_scale_ignores_its_noise_table(engine, c):
    """noise_sd 0 and noise_clip 0: another target_noise table; eps_sd 0: another caps_noise table -- every output is the same"""
    d, _ = _case(c)
    k = 'cn' if c[0] == 'eps_sd0' else 'tn'
    d2 = dict(d, **{k: _other_draws(d)[k]})
    assert (d2[k] != d[k]).all()
    (_, a), (_, b) = _run(engine, d), _run(engine, d2)
    _same(a, b, H.case_id(c))
    # ... while at td3_64's constants the table matters (the pair of launches can tell a read table from an ignored one)
    plain = dict(d, hp=T.hyper())
    (_, a), (_, b) = _run(engine, plain), _run(engine, dict(plain, **{k: d2[k]}))
    assert (a['critic' if k == 'tn' else 'actor'] != b['critic' if k == 'tn' else 'actor']).any()


# ---- c. slots outside [0, capacity) --------------------------------------------------------------------------------------------------
LOW, HIGH = (-1, I32_MIN), ('cap', 'cap+7', I32_MAX)


def _plant_slots(d, cap, positions):
    """-> (slots with out-of-range entries at `positions` of updates 0, 1, 3 and the last, the same entries clamped): the five values of
    the issue walk over the planted places"""
    bad, good = d['slots'].copy(), d['slots'].copy()
    values = [-1, I32_MIN, cap, cap + 7, I32_MAX]
    i = 0
    for u in sorted({0, 1, 3, d['n'] - 1}):
        for b in positions:
            v = values[i % 5]
            i += 3
            bad[u, b], good[u, b] = v, (0 if v < 0 else cap - 1)
    assert i // 3 >= 10 and {int(v) for v in bad[bad != good]} == set(values) and (bad[:, list(positions)] != good[:, list(positions)]).any(0).all()
    return bad, good


def _clamp_pair(engine, cls, cases, positions, run):
    outs = []
    for which in (0, 1):
        planted = [dict(d, slots=_plant_slots(d, d['ring'].shape[0], positions)[which]) for d in cases]
        la = cls(engine, planted)
        cap = la.place_ring()
        assert cap == cases[0]['ring'].shape[0] and (which == 1 or min(int(p['slots'].min()) for p in planted) == I32_MIN)
        assert run(la) == 0, la.L.serl_last_error()
        o = la.out()
        _finite(la, o)
        la.assert_guards(o)
        np.testing.assert_array_equal(GG.bits(la.ring_buf.cpu().numpy()), GG.bits(la.ring_host))
        outs.append(o)
    _same(outs[0], outs[1], 'planted against clamped')
    return outs[0]


def test_slot_clamp_train(engine):
    """B = 65: sample 0, the last sample of the first wavefront (63), the lone sample of the second (64) and one in between"""
    d, _ = _case(('tau0', 'l'))
    assert d['B'] == 65
    _clamp_pair(engine, Launch, [d], (0, 30, 63, 64), lambda la: la.run())


def test_slot_clamp_train_big(engine):
    """B = 129: the same places in the first chunk, its last sample (127) and the one sample of the second chunk (128), in both dense flavours"""
    d, _ = _flavour('ref_defaults', big=True)
    assert d['B'] == 129
    a = _clamp_pair(engine, BigLaunch, [d], (0, 63, 64, 127, 128), lambda la: la.run('big', 0))
    b = _clamp_pair(engine, BigLaunch, [d], (0, 63, 64, 127, 128), lambda la: la.run('big', 1))
    _same(a, b, 'valu against mfma')


def test_slot_clamp_three_learners_in_one_launch(engine):
    """three learners of one serl_td3_train launch, each with its own ring, table and planted places.  (The serl_td3_train_group entries
    take no slot table: they draw their slots in the kernel, inside [0, n_rows) by construction.)"""
    c = ('tau0', 'l')
    cases = [H.make_case(c)] + [H.make_case(c, seed) for seed in (21, 22)]
    _clamp_pair(engine, Launch, cases, (0, 63, 64), lambda la: la.run())


# ---- d. every other flavour at two points away from td3_64's constants -----------------------------------------------------------------
POINTS2 = list(H.FLAVOUR_POINTS)


def _rng_fill(la, d):
    """serl_td3_rng_fill's tables of the call la.run('old', gen=True) makes"""
    S, A, B, n, it0, freq = d['S'], d['A'], d['B'], d['n'], d['it0'], d['freq']
    k = (it0 + n) // freq - it0 // freq
    sl = torch.full((n, B), -9, dtype=torch.int32, device=la.dev)
    tn = torch.full((n, B, A), float('nan'), device=la.dev)
    cn = torch.full((max(k, 1), B, S), float('nan'), device=la.dev)
    rc = la.L.serl_td3_rng_fill(la.engine.ctx, ctypes.byref(la.rng_desc(0, 2)), 0, S, A, B, it0, n, freq, sl.data_ptr(), tn.data_ptr(), cn.data_ptr(),
                                la.stream())
    torch.cuda.synchronize()
    assert rc == 0, la.L.serl_last_error()
    return sl, tn, cn[:k]


@pytest.mark.parametrize('point', POINTS2)
def test_mfma_and_rng_equal_train(engine, point):
    """serl_td3_train_mfma on the same descriptor, and serl_td3_train_rng against serl_td3_train (and _mfma) on serl_td3_rng_fill's tables"""
    d, ref = _flavour(point)
    res = {}
    for dense in (0, 1):
        la = BigLaunch(engine, [d])
        assert la.run('old', dense) == 0, la.L.serl_last_error()
        res[dense] = la.out()
        la.assert_guards(res[dense])
        assert la.steps_of(res[dense]) == H.steps_taken(d)
    T.check(la.result(res[0], 0), ref, d, 'flavours %s B %d' % (point, d['B']))
    _same(res[0], res[1], 'valu against mfma')
    for dense in (0, 1):
        g = BigLaunch(engine, [d])
        assert g.run('old', dense, gen=True, learner0=2) == 0, g.L.serl_last_error()
        tb = BigLaunch(engine, [d])
        assert tb.run('old', dense, tables=_rng_fill(tb, d)) == 0, tb.L.serl_last_error()
        o = g.out()
        _finite(g, o)
        assert g.steps_of(o) == H.steps_taken(d)
        _same(o, tb.out(), 'generator against its tables, dense %d' % dense)


@pytest.mark.parametrize('point', POINTS2)
def test_big_vs_float64_and_wide_and_mfma_equal_big(engine, point):
    """B = 129: serl_td3_train_big against the float64 run within td3_64's bounds (tests/test_td3_hp_host.py holds float32 torch to
    them at these two points); serl_td3_train_wide and the mfma variants of both bit for bit"""
    d, ref = _flavour(point, big=True)
    big = BigLaunch(engine, [d])
    assert big.run('big', 0) == 0, big.L.serl_last_error()
    a = big.out()
    T.check(big.result(a, 0), ref, d, 'big %s B %d' % (point, d['B']))
    big.assert_guards(a)
    assert big.steps_of(a) == H.steps_taken(d)
    for entry, dense, cls in (('big', 1, BigLaunch), ('wide', 0, WideLaunch), ('wide', 1, WideLaunch)):
        la = cls(engine, [d])
        assert la.run(entry, dense) == 0, la.L.serl_last_error()
        assert entry != 'wide' or la.ran()
        b = la.out()
        la.assert_guards(b)
        _same(a, b, '%s dense %d against serl_td3_train_big' % (entry, dense))


def _group_specs(B, n):
    """three learners: the reference's defaults, the combined edge (on a warm optimiser: group_steps), td3_64's constants"""
    row = lambda hp: {k: T.hyper(hp)[k] for k in HP_FIELDS}
    return [GG.Spec(11, B + 9, B + 9, n, 0, 2, 1, row(H.REF_DEFAULTS), 77, 0), GG.Spec(12, B + 20, 2 * B + 40, n, 1, 2, 0, row(H.COMBINED_EDGE), 2**64 - 1, 5),
            GG.Spec(13, B + 5, B + 6, n - 1, 7, 3, 1, row(None), 0x9E3779B97F4A7C15, 2**31 - 2)]


def _warm(g):
    """learner 1 of a group starts from the combined edge's step counts"""
    g.host['steps'][2] = H.FLAVOUR_POINTS['combined_edge'][1]
    g.t['steps'] = torch.from_numpy(g.host['steps']).to(g.dev)
    return g


@pytest.mark.parametrize('entry,shape', [('group', (7, 3, 20, 2, 17)), ('big', (2, 1, 4, 0, 129)), ('wide', (2, 1, 4, 0, 129))], ids=['group', 'group_big', 'group_wide'])
def test_group_rows_carry_the_points(engine, entry, shape):
    """a heterogeneous launch whose rows carry the two points and td3_64's constants: each learner bit for bit its single-learner
    generator call (serl_td3_train_rng, resp. serl_td3_train_big / _wide) with the row's values in the descriptor"""
    sp = _group_specs(shape[4], 5)
    make = (lambda: GG.Group(engine, shape, sp)) if entry == 'group' else (lambda: GGB.Group(engine, shape, sp, entry=entry))
    g = _warm(make())
    assert g.run_group(0, 1) == 0, g.L.serl_last_error()
    o = g.out()
    assert o['status'].tolist() == [-9, 0, 0, 0, -9]
    for i, s in enumerate(sp):
        solo = _warm(make())
        solo.run_single(i, 0, 1)
        so = solo.out()
        for k in OUT:
            np.testing.assert_array_equal(GG.bits(so[k][1 + i]), GG.bits(o[k][1 + i]), err_msg='%s learner %d' % (k, i))
            others = [j for j in range(5) if j != 1 + i]
            np.testing.assert_array_equal(GG.bits(so[k][others]), GG.bits(solo.host[k][others]), err_msg=k)
        k_act = (s.it0 + s.n) // s.freq - s.it0 // s.freq
        assert o['steps'][1 + i].tolist() == [g.host['steps'][1 + i][0] + s.n, g.host['steps'][1 + i][1] + k_act]
        assert np.isfinite(o['critic'][1 + i, :g.Pc]).all() and (o['critic'][1 + i, :g.Pc] != g.host['critic'][1 + i, :g.Pc]).any()
    # tau 1 on a held actor target (uat 0): the critic target follows its network, the actor target stays
    np.testing.assert_array_equal(GG.bits(o['actor_target'][2]), GG.bits(g.host['actor_target'][2]))
    np.testing.assert_allclose(o['critic_target'][2, :g.Pc], o['critic'][2, :g.Pc], rtol=0, atol=1e-6)


# ---- e. the Python layer ----------------------------------------------------------------------------------------------------------------
def _py_args(dev, B=86, **over):
    a = G._args(7, 3, 72, 3, 'tanh', B, dev)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_td3_train_fused_equals_eager_away_from_the_defaults(engine):
    """as test_gpu_td3.test_td3_train_fused_path_and_fallback, with gamma, tau, noise_sd, noise_clip and the CAPS dict away from what
    that test runs: the fused path agrees with the eager loop on the same draws (both f32: twice the bound apart)"""
    import serl_amd
    from serl_amd.actor import pack_actor, pack_critic
    dev = engine.device
    d = T.make_case(T.CASES[0])
    res = {}
    for fused in (True, False):
        torch.manual_seed(5)
        t = serl_amd.TD3(_py_args('cpu', gamma=0.9, tau=0.2, noise_sd=0.4, noise_clip=0.25), engine)
        t.caps_dict = dict(lambda_s=1.5, lambda_t=0.02, eps_sd=0.2)
        ring = serl_amd.DeviceReplay(400, dev, engine, 7, 3)
        ring.append_rows(torch.from_numpy(d['ring']))
        w0 = pack_actor(t.actor).numpy().astype(np.float64), pack_critic(t.critic).numpy().astype(np.float64)
        out = t.train(ring, 14, iteration0=3, rng=random.Random(3), generator=torch.Generator().manual_seed(9), fused=fused)
        assert t.last_path == ('fused' if fused else 'eager')
        res[fused] = (pack_actor(t.actor).numpy().astype(np.float64), pack_critic(t.critic).numpy().astype(np.float64), out, w0,
                      pack_actor(t.actor_target).numpy().astype(np.float64), pack_critic(t.critic_target).numpy().astype(np.float64))
    for k, name in ((0, 'actor'), (1, 'critic')):
        moved = np.abs(res[False][k] - res[False][3][k]).max()
        assert moved > T.MIN_MOVED
        for j, what in ((k, name), (4 + k, name + '_target')):
            err = np.abs(res[True][j] - res[False][j]).max()
            print('TD3_HP_TRAIN %s |fused - eager| %.3g moved %.4f' % (what, err, moved))
            assert err <= 2 * T.TOL_REL['tanh'] * moved + T.TOL_ABS
    assert abs(res[True][2]['TD_loss'] - res[False][2]['TD_loss']) <= 1e-3 * abs(res[False][2]['TD_loss']) + 1e-6
    assert abs(res[True][2]['PG_obj'] - res[False][2]['PG_obj']) <= 1e-3 * abs(res[False][2]['PG_obj']) + 1e-6


def test_td3_group_train_two_hyper_parameter_sets(engine):
    """TD3Group.train with two members -- the reference's defaults and the combined edge -- against two TD3.train(draws='device') calls"""
    import serl_amd
    dev = engine.device
    S, A = 7, 3
    points = [H.REF_DEFAULTS, T.hyper(H.COMBINED_EDGE)]

    def learners():
        out = []
        for i, hp in enumerate(points):
            torch.manual_seed(5 + i)
            t = serl_amd.TD3(_py_args('cpu', B=17, hidden_size=20, num_layers=2, **{k: hp[k] for k in ('lr', 'gamma', 'tau', 'noise_sd', 'noise_clip')}), engine)
            t.caps_dict = {k: hp[k] for k in ('lambda_s', 'lambda_t', 'eps_sd')}
            ring = serl_amd.DeviceReplay(64, dev, engine, S, A)
            ring.append_rows(torch.from_numpy(R._ring(S, A, 40, 40)))
            out.append((t, ring))
        return out

    grouped, alone = learners(), learners()
    group = serl_amd.TD3Group([t for t, _ in grouped])
    for n, it0 in ((5, 0), (5, 5)):                 # the second call runs on the warm optimisers of the first; it ends on an actor update
        got = group.train([r for _, r in grouped], n, iteration0=it0, seed=[77, 78], key=[3, 4])
        for i, (t, ring) in enumerate(alone):
            want = t.train(ring, n, iteration0=it0, draws='device', seed=77 + i, learner=3 + i)
            assert got[i] == want and grouped[i][0].last_path == 'fused-group-rng'
            a, b = R._state(grouped[i][0]), R._state(t)
            for k in a:
                np.testing.assert_array_equal(GG.bits(a[k]), GG.bits(b[k]), err_msg='%s learner %d' % (k, i))
    a, b = R._state(grouped[0][0]), R._state(grouped[1][0])
    assert a['steps'].tolist() == b['steps'].tolist() == [10, 5]
    np.testing.assert_allclose(b['critic_target'], b['critic'], rtol=0, atol=1e-6)            # tau 1
    assert np.abs(a['critic_target'] - a['critic']).max() > 1e-4                                 # tau 0.005


# ---- f. learners that share every input array ----------------------------------------------------------------------------------------
def test_shared_input_arrays(engine):
    """two learners (different weights) of one serl_td3_train launch with ring_stride = slots_stride = noise_stride = caps_stride = 0
    against the same launch with a copy of every input per learner.  (No older test does: test_gpu_td3_rng shares the ring among several
    learners, but on the generator path, which ignores the three tables; the table path shares them with one learner only.)"""
    c = ('ref_defaults', 'm')
    d0, d1 = H.make_case(c), H.make_case(c, 31)
    shared = {k: d0[k] for k in ('ring', 'slots', 'tn', 'cn')}
    cases = [d0, dict(d1, **shared)]
    assert (cases[1]['actor'] != d0['actor']).any()
    copies = BigLaunch(engine, cases)
    assert copies.run('old', 0) == 0, copies.L.serl_last_error()
    a = copies.out()
    one = BigLaunch(engine, cases)
    t = one.t
    one.over.update(ring_stride=0)
    assert one.run('old', 0, tables=(t['slots'][0, :, :d0['B']].contiguous(), t['tn'][0].contiguous(), t['cn'][0].contiguous())) == 0, one.L.serl_last_error()
    b = one.out()
    d = one.desc(tables=(t['slots'][0], t['tn'][0], t['cn'][0]))
    assert (d.ring_stride, d.slots_stride, d.noise_stride, d.caps_stride, d.n_learners) == (0, 0, 0, 0, 2)
    _finite(one, b)
    one.assert_guards(b)
    _same(a, b, 'shared against copied inputs')
    assert (a['critic'][1] != a['critic'][2]).any()
    T.check(one.result(b, 0), _case(c)[1], d0, 'shared inputs, learner 0', tol=H.tol_of(c, d0['act']))

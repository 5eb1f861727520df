"""CPU tests of the TD3 learner: the float64 contract of serl_td3_train (tests/td3_64.py) against the chains the reference's own TD3
ran (tests/golden/td3_update.npz), the calibration of the tolerance the GPU grid applies and that it catches planted mistakes, the
packed critic row, the C exports and their argument checks, and serl_amd.TD3 without a GPU."""
import ctypes
import functools
import os
import random
import re
import types
import numpy as np
import pytest
import torch
import td3_64 as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _case(c):
    d = T.make_case(c)
    return d, T.td3_literal(d)


def test_grid_covers_the_kernels_paths():
    C = T.CASES
    assert {c[5] for c in C} >= {1, 3, 64, 65, 86, 127, 128}
    assert {c[2] for c in C} >= {4, 32, 72, 96, 128} and {c[3] for c in C} >= {0, 1, 3}
    assert {(c[0], c[1]) for c in C} >= {(7, 3), (2, 1), (16, 3), (1, 1), (16, 4)}
    for act in ('tanh', 'elu', 'relu'):
        assert sum(1 for c in C if c[4] == act) >= 3
    assert {c[6] for c in C} == {1, 2, 3} and {c[9] for c in C} == {0, 1} and {c[10] for c in C} == {0, 1} and {c[11] for c in C} == {'small', 'big'}
    first = {(c[7] + 1) % c[6] == 0 for c in C if c[6] > 1}
    assert first == {True, False}
    assert all(c[8] % c[6] != 0 for c in C if c[6] > 1) and all(12 <= c[8] <= 30 for c in C)
    for c in C:
        d = T.make_case(c)
        S, A = d['S'], d['A']
        assert d['ring'][d['slots'].reshape(-1), 2 * S + A + 1].any() or d['B'] < 4, 'no done row in ' + T.case_id(c)
        assert all(len(set(r)) == d['B'] for r in d['slots'])
        assert len(d['critic']) == T.critic_param_count(S, A) and len(d['actor']) == T.actor_param_count(S, A, d['H'], d['L'])


@pytest.mark.parametrize('c', T.CASES, ids=T.case_id)
def test_float32_loop_meets_the_bound(c):
    """the calibration, asserted: the literal loop in float32 torch is within the bound of the float64 run, every case trains, the clip
    is active in every critic step of a 'big' case and in none of a 'small' one, and the written-out loop equals the literal one"""
    d, ref = _case(c)
    assert all(ref['clip_c']) if d['rew'] == 'big' else not any(ref['clip_c']), ref['clip_c']
    T.check(T.td3_literal(d, torch.float32), ref, d, T.case_id(c))
    ex = T.td3_explicit64(d)
    for k in T.ROWS + T.MOMENTS + ('td',):
        np.testing.assert_allclose(ex[k], ref[k], rtol=0, atol=1e-11, err_msg=k)
    np.testing.assert_allclose(ex['pg'], ref['pg'], rtol=0, atol=1e-11, equal_nan=True)
    assert ex['clip_c'] == ref['clip_c']


@pytest.mark.parametrize('mistake', T.MISTAKES)
def test_planted_mistakes_exceed_the_bound(mistake):
    """each planted mistake moves a row past the bound in at least one grid case (cases the mistake can show in only)"""
    seen = []
    for c in T.CASES:
        S, A, H, L, act, B, freq, it0, n, caps, uat, rew = c
        if (mistake in ('clip_per_critic',) and rew != 'big') or (mistake == 'clip_always' and rew != 'small') or \
           (mistake == 'no_caps' and not caps) or (mistake == 'champion_target_updated' and uat) or (mistake == 'actor_every_step' and freq == 1):
            continue
        d, ref = _case(c)
        dev, moved = T.deviations(T.td3_explicit64(d, mistake), ref, d)
        ratio = max(dev[k] / (T.TOL_REL[act] + T.TOL_ABS / moved[k.split('_')[0]]) for k in T.ROWS)
        seen.append((round(float(ratio), 2), T.case_id(c)))
        if ratio > 1.0:
            return
    pytest.fail('%s stays within the bound in every case: %s' % (mistake, seen))


def _golden_case(g, tag):
    from test_gpu_td3 import golden_case
    return golden_case(g, tag)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_float64_restatement_reproduces_the_reference(golden, tag):
    """the chains of the reference's own TD3 (float32 torch, CPU): the float64 restatement on the recorded rows, slots and draws ends
    within the f32 bound of the reference's rows, with its loss sequences"""
    d, ref = _golden_case(golden('td3_update'), tag)
    r64 = T.td3_literal(d)
    dev, moved = T.deviations({k: ref[k] for k in T.ROWS} | {k: r64[k] for k in T.MOMENTS}, r64, d)
    assert moved['actor'] > T.MIN_MOVED and moved['critic'] > T.MIN_MOVED
    for k in T.ROWS:
        assert dev[k] <= T.TOL_REL[d['act']] + T.TOL_ABS / moved[k.split('_')[0]], (k, dev[k])
    np.testing.assert_allclose(ref['td'], r64['td'], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(ref['pg'], r64['pg'], rtol=2e-3, atol=1e-5, equal_nan=True)
    if not d['uat']:
        np.testing.assert_array_equal(ref['actor_target'], d['actor_target'].astype(np.float64))


@pytest.mark.needs_reference
def test_golden_maker_reproduces_the_committed_file(golden, tmp_path):
    import subprocess, sys
    g = golden('td3_update')
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_td3_golden as M
    out = M.run('b', M.CHAINS['b'])
    for k, v in out.items():
        np.testing.assert_allclose(v, g[k], rtol=1e-5, atol=1e-6, equal_nan=True, err_msg=k)


def _args(S=7, A=3, H=72, L=3, act='tanh', B=86, caps=True, freq=2):
    return types.SimpleNamespace(state_dim=S, action_dim=A, hidden_size=H, num_layers=L, activation_actor=act, device='cpu', individual_bs=300,
                                 lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP, policy_update_freq=freq,
                                 use_caps=caps, batch_size=B)


def test_pack_critic_round_trip_and_row_length():
    import serl_amd
    from serl_amd import _capi
    for S, A in ((7, 3), (2, 1), (16, 4)):
        c = serl_amd.Critic(_args(S, A))
        row = serl_amd.pack_critic(c)
        assert row.numel() == _capi.lib().serl_td3_param_count(S, A) == T.critic_param_count(S, A) == serl_amd.td3.critic_param_count(S, A)
        c2 = serl_amd.Critic(_args(S, A))
        assert serl_amd.unpack_critic(c2, row) == row.numel()
        assert torch.equal(serl_amd.pack_critic(c2), row)
        x, a = torch.randn(5, S), torch.rand(5, A)
        q1, q2 = c(x, a)
        assert q1.shape == (5, 1) and torch.equal(q1, c2(x, a)[0]) and not torch.equal(q1, q2)
        # the row's order: W1 of critic 1 first, bo of critic 2 last
        assert torch.equal(row[:64 * (S + A)], c.q1.l1.weight.detach().reshape(-1)) and row[-1] == c.q2.out.bias.detach()[0]
    assert _capi.lib().serl_td3_param_count(7, 3) == 10370


def test_exports_header_and_layout():
    from serl_amd import _capi
    L = _capi.lib()
    for f in ('serl_td3_train', 'serl_td3_work_bytes', 'serl_td3_param_count', 'serl_td3_layout'):
        assert f in _capi.EXPORTS and hasattr(L, f)
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert re.search(r'#define SERL_ABI_VERSION 9\b', hdr) and L.serl_abi_version() == 9 == _capi.ABI_VERSION
    for f in ('serl_td3_train', 'serl_td3_work_bytes', 'serl_td3_param_count', 'serl_td3_layout', 'serl_td3_desc'):
        assert f in hdr
    assert L.serl_abi_layout(None, 0) == len(_capi.expected_layout()) == 62
    want = _capi.expected_td3_layout()
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_td3_layout(got, len(want)) == len(want) and list(got) == want
    assert L.serl_td3_work_bytes(1, 7, 3, 72, 3, 86) > 0
    assert L.serl_td3_work_bytes(3, 7, 3, 72, 3, 86) == 3 * L.serl_td3_work_bytes(1, 7, 3, 72, 3, 86)
    for bad in ((0, 7, 3, 72, 3, 86), (1, 7, 3, 70, 3, 86), (1, 17, 3, 72, 3, 86), (1, 7, 3, 72, 5, 86), (1, 7, 3, 72, 3, 0), (1, 7, 5, 72, 3, 86)):
        assert L.serl_td3_work_bytes(*bad) == 0, bad


def test_bad_arguments_are_refused_without_a_gpu():
    """NULL and out-of-range arguments return SERL_E_INVALID before any device work (no context is needed to get that far: a NULL
    context is itself refused)"""
    from serl_amd import _capi
    L = _capi.lib()
    assert L.serl_td3_train(None, None, None) == _capi.E_INVALID
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def desc(**kw):
        d = _capi.Td3Desc(state_dim=7, action_dim=3, hidden=72, num_layers=3, activation=0, n_learners=1, batch=86, n_updates=2, capacity=100,
                          slot_cols=86, policy_update_freq=2, iteration0=0, update_actor_target=1, lr=1e-3, gamma=0.99, tau=0.005, noise_sd=0.2,
                          noise_clip=0.5, lambda_s=0.5, lambda_t=0.1, eps_sd=0.05, max_grad_norm=10.0, actor=p, actor_target=p, actor_m=p, actor_v=p,
                          actor_stride=20000, critic=p, critic_target=p, critic_m=p, critic_v=p, critic_stride=11000, adam_steps=p, ring=p,
                          slots=p, target_noise=p, caps_noise=p, td_loss=p, pg_loss=p, loss_stride=2, work=p, work_bytes=1 << 30)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    ctx = ctypes.c_void_p(buf.ctypes.data)          # never dereferenced: every call below is refused by the argument checks
    assert L.serl_td3_train(None, ctypes.byref(desc()), None) == _capi.E_INVALID
    for kw in (dict(actor=None), dict(critic_v=None), dict(adam_steps=None), dict(ring=None), dict(slots=None), dict(target_noise=None),
               dict(td_loss=None), dict(pg_loss=None), dict(work=None), dict(state_dim=0), dict(action_dim=0), dict(hidden=0), dict(num_layers=-1),
               dict(batch=0), dict(activation=3), dict(activation=-1), dict(n_learners=0), dict(n_updates=-1), dict(capacity=0), dict(slot_cols=85),
               dict(policy_update_freq=0), dict(iteration0=-1), dict(lr=0.0), dict(gamma=-0.1), dict(tau=1.5), dict(noise_sd=-1.0),
               dict(max_grad_norm=0.0), dict(actor_stride=100), dict(critic_stride=100), dict(loss_stride=1), dict(work_bytes=8),
               dict(ring_stride=-1), dict(lr=float('nan'))):
        assert L.serl_td3_train(ctx, ctypes.byref(desc(**kw)), None) == _capi.E_INVALID, kw
        assert L.serl_last_error()
    for kw in (dict(hidden=132), dict(hidden=70), dict(num_layers=5), dict(state_dim=17), dict(action_dim=5), dict(batch=129, slot_cols=129)):
        assert L.serl_td3_train(ctx, ctypes.byref(desc(**kw)), None) == _capi.E_UNSUPPORTED, kw


@pytest.mark.parametrize('caps,champion', [(True, False), (False, True)])
def test_train_without_a_gpu_equals_the_literal_float32_loop(caps, champion):
    """TD3.train on a CPU ring loops update_parameters over the draws it made: the same slots (python's random stream), the same noise
    (the torch generator, in the reference's order) fed to the literal float32 loop give the same rows"""
    import serl_amd
    from serl_amd import replay
    from serl_amd.actor import pack_actor, pack_critic
    c = (7, 3, 32, 2, 'elu', 24, 2, 3, 13, int(caps), int(not champion), 'small')
    d = T.make_case(c)
    torch.manual_seed(3)
    t = serl_amd.TD3(_args(7, 3, 32, 2, 'elu', 24, caps), None)
    from serl_amd.actor import unpack_into, unpack_critic
    unpack_into(t.actor, torch.from_numpy(d['actor'])); unpack_into(t.actor_target, torch.from_numpy(d['actor_target']))
    unpack_critic(t.critic, torch.from_numpy(d['critic'])); unpack_critic(t.critic_target, torch.from_numpy(d['critic_target']))
    ring = serl_amd.DeviceReplay(300, 'cpu', None, 7, 3)
    ring.append_rows(torch.from_numpy(d['ring']))
    out = t.train(ring, 13, iteration0=3, champion_target=champion, rng=random.Random(11), generator=torch.Generator().manual_seed(12))
    assert t.last_path == 'eager'
    d['slots'] = replay.sample_many(len(ring), 24, 13, random.Random(11))
    tn, cn = serl_amd.td3.draw_noise(13, 24, 7, 3, 3, 2, caps, torch.Generator().manual_seed(12))
    d['tn'], d['cn'] = tn.numpy(), (cn.numpy() if caps else None)
    ref = T.td3_literal(d, torch.float32)
    for k, m in (('actor', t.actor), ('actor_target', t.actor_target)):
        np.testing.assert_array_equal(pack_actor(m).numpy(), ref[k].astype(np.float32), err_msg=k)
    for k, m in (('critic', t.critic), ('critic_target', t.critic_target)):
        np.testing.assert_array_equal(pack_critic(m).numpy(), ref[k].astype(np.float32), err_msg=k)
    assert out['TD_loss'] == pytest.approx(np.median(ref['td']), rel=1e-6)
    assert out['PG_obj'] == pytest.approx(np.mean(-ref['pg'][~np.isnan(ref['pg'])]), rel=1e-6)
    if champion:
        np.testing.assert_array_equal(pack_actor(t.actor_target).numpy(), d['actor_target'])


def test_td3_fits_the_host_adaptors():
    """TD3 carries what generation.evaluate_generation(rl_agent=...) and Agent.rl_to_evo read (.actor with a spec, .buffer and
    .critical_buffer of the env's dims), and its critic is the callable distillation's Q-filter calls"""
    import serl_amd
    from serl_amd import distill, generation
    from serl_amd.actor import spec_of
    a = _args(7, 3, 32, 3, 'tanh', 16)
    t = serl_amd.TD3(a, None)
    assert generation._actor_of(t) is t.actor and spec_of(t) == serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    assert serl_amd.pack_actor(t).numel() == spec_of(t).param_count
    for b in (t.buffer, t.critical_buffer):
        assert isinstance(b, serl_amd.DeviceReplay) and (b.state_dim, b.action_dim, b.capacity) == (7, 3, 300)
    assert torch.equal(serl_amd.pack_actor(t.actor), serl_amd.pack_actor(t.actor_target))
    assert torch.equal(serl_amd.pack_critic(t.critic), serl_amd.pack_critic(t.critic_target))
    p1, p2, child = serl_amd.Actor(a), serl_amd.Actor(a), serl_amd.Actor(a)
    opt = torch.optim.Adam(child.parameters(), lr=1e-3)
    before = serl_amd.pack_actor(child)
    mse = distill.update_parameters(child, opt, (torch.randn(32, 7),), p1, p2, t.critic)
    assert torch.isfinite(mse) and not torch.equal(serl_amd.pack_actor(child), before)
    pgl, td = t.update_parameters((torch.randn(16, 7), torch.rand(16, 3), torch.randn(16, 7), torch.randn(16, 1), torch.zeros(16, 1)), 2)
    assert pgl is not None and np.isfinite(td)


@pytest.mark.parametrize('shape', [(2, 1, 4, 0, 1), (7, 3, 72, 3, 86)], ids=['S2A1_H4L0', 'S7A3_H72L3'])
def test_one_packer_and_descriptor_for_td3_and_group(shape):
    """What TD3.train and TD3Group.train share, on CPU tensors: a TD3Group of one learner packs the rows and the steps and describes the
    launch as that learner's own TD3 path does -- every scalar field of the Td3Desc, a learner's own values in the descriptor on one side
    and in its Td3LearnerRow on the other -- and packing followed by unpacking leaves parameters, targets and both Adam states as they were"""
    import serl_amd
    from serl_amd import _capi, td3
    S, A, H, L, B = shape
    torch.manual_seed(S + H)
    fresh, stepped = serl_amd.TD3(_args(S, A, H, L, 'elu', B), None), serl_amd.TD3(_args(S, A, H, L, 'elu', B), None)
    for it in (1, 2, 3):                # the critic has stepped three times, the actor (every second iteration) once
        stepped.update_parameters((torch.randn(B, S), torch.rand(B, A), torch.randn(B, S), torch.randn(B, 1), torch.zeros(B, 1)), it)
    with torch.no_grad():               # (a target that differs from its network)
        for p in stepped.actor_target.parameters():
            p.add_(0.25)
    for t, want_steps in ((fresh, [0, 0]), (stepped, [3, 1])):
        ring = serl_amd.DeviceReplay(300, 'cpu', None, S, A)
        n, lib = 13, _capi.lib()
        launches = []
        for learners in ([t], serl_amd.TD3Group([t]).learners):
            rows, steps = td3._pack(learners, 'cpu')
            td, pg, work = td3._outputs(lib, learners[0].args, 1, n, False, 'cpu')
            launches.append((rows, steps, td, pg, work))
        own = td3._learner_fields(t, ring, 4, True)
        d_one = td3._describe(t.args, n, *launches[0], ring=ring.rows.data_ptr(), slot_cols=B, **own)
        d_grp = td3._describe(t.args, n, *launches[1])
        row = _capi.Td3LearnerRow(ring=ring.rows.data_ptr(), seed=5, n_rows=len(ring), n_updates=n, key=0, **own)
        # the rows and the steps
        (rows, steps), (rows_g, steps_g) = launches[0][:2], launches[1][:2]
        assert set(rows) == set(rows_g) == set(td3.ROWS) and steps.tolist() == steps_g.tolist() == [want_steps]
        Pa, Pc = T.actor_param_count(S, A, H, L), T.critic_param_count(S, A)
        for k in td3.ROWS:
            assert rows[k].shape == (1, Pa if k.startswith('actor') else Pc) and rows[k].dtype == torch.float32 and torch.equal(rows[k], rows_g[k]), k
        assert torch.equal(rows['actor'][0], serl_amd.pack_actor(t.actor)) and torch.equal(rows['critic_target'][0], serl_amd.pack_critic(t.critic_target))
        assert bool(rows['critic_m'].any()) == bool(want_steps[0]) and bool(rows['actor_v'].any()) == bool(want_steps[1])
        # every scalar of the descriptor
        scalars = [f for f, ty in _capi.Td3Desc._fields_ if ty in (ctypes.c_int32, ctypes.c_float, ctypes.c_int64) and not f.startswith('pad')]
        assert {'state_dim', 'batch', 'n_updates', 'n_learners', 'actor_stride', 'critic_stride', 'loss_stride', 'work_bytes', 'max_grad_norm', 'lr',
                'capacity', 'policy_update_freq'} <= set(scalars)
        for f in scalars:
            if f in own:
                assert getattr(d_one, f) == getattr(row, f) and getattr(d_grp, f) == 0, f
            elif f != 'slot_cols':
                assert getattr(d_one, f) == getattr(d_grp, f), f
        assert (d_one.state_dim, d_one.action_dim, d_one.hidden, d_one.num_layers, d_one.activation, d_one.n_learners, d_one.batch, d_one.n_updates) \
            == (S, A, H, L, 1, 1, B, n)
        assert (d_one.actor_stride, d_one.critic_stride, d_one.loss_stride, d_one.max_grad_norm) == (Pa, Pc, n, 10.0)
        assert d_one.work_bytes == lib.serl_td3_work_bytes(1, S, A, H, L, B) > 0
        assert (d_one.capacity, d_one.iteration0, d_one.policy_update_freq, d_one.update_actor_target) == (300, 4, 2, 1)
        assert d_one.lr == pytest.approx(T.LR) and d_one.lambda_s == pytest.approx(0.5) and d_one.eps_sd == pytest.approx(0.05)
        # pack, then unpack: nothing moves
        nets = lambda: [p.detach().clone() for m in (t.actor, t.actor_target, t.critic, t.critic_target) for p in m.parameters()]
        adam = lambda o, m: [{k: v.clone() for k, v in o.state.get(p, {}).items()} for p in m.parameters()]
        before = nets(), adam(t.critic_optim, t.critic), adam(t.actor_optim, t.actor)
        td3._unpack(t, rows, steps.tolist(), 0)
        after = nets(), adam(t.critic_optim, t.critic), adam(t.actor_optim, t.actor)
        assert all(torch.equal(x, y) for x, y in zip(before[0], after[0]))
        for was, now, step in zip(before[1:], after[1:], want_steps):
            for x, y in zip(was, now):
                if x:
                    assert set(x) == set(y) == {'step', 'exp_avg', 'exp_avg_sq'} and float(x['step']) == float(y['step']) == step
                    assert torch.equal(x['exp_avg'], y['exp_avg']) and torch.equal(x['exp_avg_sq'], y['exp_avg_sq'])
                else:                   # no state yet: what Adam would start from, or nothing
                    assert step == 0 and (not y or (float(y['step']) == 0 and not y['exp_avg'].any() and not y['exp_avg_sq'].any()))
        assert bool(t.actor_optim.state) == bool(want_steps[1])         # the actor's optimiser is only written once it has stepped

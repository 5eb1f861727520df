"""The GA entry points against serl_shape_query on the device, at the shapes on either side of each bound of their contracts
(serl_amd/csrc/serl_shapes.h): SERL_OK exactly where the query says "takes", the same return code and the same serl_last_error where it
refuses, and a refused call leaves its outputs alone.  One member or pair, batch 2, guard values around the outputs; no timing, no workload
shapes.  (serl_td3_train* and serl_venv_rollout* refuse through the same predicates; their own GPU suites drive those refusals.)"""
import ctypes
import pytest
import torch

pytestmark = pytest.mark.gpu
SENT = 777.0
B = 2


def _spec(S, A, H, L, act=0):
    import types
    return types.SimpleNamespace(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation_id=act)


def _params(S, A, H, L):
    return H * S + H + L * (H * H + 3 * H) + A * H + A


def _genome(S, A, H, L):
    return H * S + L * H * H + A * H


# (S, A, H, L, act): the corners of the range and one step outside each bound
GA_LDS = [(1, 1, 2, 0, 0), (64, 16, 2, 0, 1), (7, 3, 256, 0, 2), (7, 3, 2, 16, 0), (7, 3, 128, 3, 0),
          (0, 3, 32, 3, 0), (65, 3, 32, 3, 0), (7, 0, 32, 3, 0), (7, 17, 32, 3, 0), (7, 3, 1, 3, 0), (7, 3, 257, 3, 0), (7, 3, 32, -1, 0), (7, 3, 32, 17, 0),
          (7, 3, 32, 3, -1), (7, 3, 32, 3, 3)]
LEARNER = [(1, 1, 4, 0, 0), (16, 4, 4, 0, 1), (7, 3, 128, 0, 2), (7, 3, 4, 4, 0),
           (0, 3, 8, 1, 0), (17, 3, 8, 1, 0), (7, 0, 8, 1, 0), (7, 5, 8, 1, 0), (7, 3, 0, 1, 0), (7, 3, 2, 1, 0), (7, 3, 6, 1, 0), (7, 3, 132, 1, 0),
           (7, 3, 8, -1, 0), (7, 3, 8, 5, 0), (7, 3, 8, 1, -1), (7, 3, 8, 1, 3)]
DISTILL = [(1, 1, 32, 3, 0), (16, 4, 32, 3, 2), (0, 3, 32, 3, 0), (17, 3, 32, 3, 0), (7, 0, 32, 3, 0), (7, 5, 32, 3, 0), (7, 3, 28, 3, 0), (7, 3, 36, 3, 0),
           (7, 3, 32, 2, 0), (7, 3, 32, 4, 0), (7, 3, 32, 3, -1), (7, 3, 32, 3, 3)]


def _agree(engine, what, spec, batch, rc):
    """the call's return code and message against the query's -> whether the shape is taken"""
    from serl_amd import _capi
    message = _capi.lib().serl_last_error().decode() if rc else ''
    torch.cuda.synchronize(engine.device)
    v = _capi.shape_query(what, spec, batch, engine.ctx)
    assert (rc, message) == (v.rc, v.message), (what, vars(spec), batch)
    assert (rc == 0) == v.takes
    return v


def _buffers(engine, S, A, H, L, out_floats):
    """weights of one member, states and actions of B rows and a guarded output, sized for the shape where it is a shape at all"""
    dev = engine.device
    ok = S >= 1 and A >= 1 and H >= 1 and L >= 0
    P = _params(S, A, H, L) if ok else 4
    g = torch.Generator().manual_seed(S * 1000 + H)
    w = (0.3 * torch.randn(1, P + 4, generator=g)).to(dev)
    st = torch.randn(1, B, max(S, 1), generator=g).to(dev)
    ac = torch.zeros(1, B, max(A, 1), device=dev)
    out = torch.full((out_floats + 8,), SENT, dtype=torch.float32, device=dev)
    return w, st, ac, out, torch.zeros(1, dtype=torch.int32, device=dev), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _guards_ok(out, n, written):
    assert bool((out[:4] == SENT).all()) and bool((out[4 + n:] == SENT).all())
    assert bool((out[4:4 + n] != SENT).all()) if written else bool((out[4:4 + n] == SENT).all())


@pytest.mark.parametrize('S,A,H,L,act', GA_LDS)
def test_sensitivity_and_novelty_agree_with_the_query(engine, S, A, H, L, act):
    """(7, 3, 128, 3): serl_ga_sensitivity's genome footprint of ~208 KB, the one LDS refusal this device can show; serl_ga_novelty takes it"""
    from serl_amd import _capi
    lib = _capi.lib()
    G = _genome(S, A, H, L) if min(S, A, H) >= 1 and L >= 0 else 4
    w, st, ac, out, m, stream = _buffers(engine, S, A, H, L, G)
    rc = lib.serl_ga_sensitivity(engine.ctx, w.data_ptr(), w.shape[1], S, H, L, A, act, m.data_ptr(), 1, st.data_ptr(), B, out.data_ptr() + 16, stream)
    v = _agree(engine, 'serl_ga_sensitivity', _spec(S, A, H, L, act), B, rc)
    _guards_ok(out, G, v.takes)
    if (S, A, H, L) == (7, 3, 128, 3):
        assert v.lds and v.message == 'serl_ga_sensitivity: network too large for the LDS-resident accumulators'
    out.fill_(SENT)
    rc = lib.serl_ga_novelty(engine.ctx, w.data_ptr(), w.shape[1], S, H, L, A, act, m.data_ptr(), 1, st.data_ptr(), ac.data_ptr(), B, out.data_ptr() + 16, stream)
    v = _agree(engine, 'serl_ga_novelty', _spec(S, A, H, L, act), B, rc)
    _guards_ok(out, 1, v.takes)


@pytest.mark.parametrize('S,A,H,L,act', LEARNER)
def test_the_general_kernels_agree_with_the_query(engine, S, A, H, L, act):
    from serl_amd import _capi
    lib = _capi.lib()
    dev = engine.device
    ok = min(S, A, H) >= 1 and L >= 0
    G = _genome(S, A, H, L) if ok else 4
    w, st, ac, out, m, stream = _buffers(engine, S, A, H, L, G)
    for batch in (B, 513):                                       # (513: one past the largest minibatch; refused before the states are looked at)
        nbytes = int(lib.serl_ga_sensitivity_general_work_bytes(1, S, A, H, L, batch))
        work = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
        out.fill_(SENT)
        rc = lib.serl_ga_sensitivity_general(engine.ctx, w.data_ptr(), w.shape[1], S, H, L, A, act, m.data_ptr(), 1, st.data_ptr(), batch,
                                             out.data_ptr() + 16, work.data_ptr(), nbytes, 0, stream)
        v = _agree(engine, 'serl_ga_sensitivity_general', _spec(S, A, H, L, act), batch, rc)
        assert not (batch == 513 and v.takes)
        _guards_ok(out, G, v.takes)
    ptrs = torch.tensor([st.data_ptr(), ac.data_ptr()], dtype=torch.int64, device=dev)
    rows = torch.full((2,), B, dtype=torch.int32, device=dev)
    for max_batch in (B, 0, 513):
        out.fill_(SENT)
        rc = lib.serl_ga_novelty_general(engine.ctx, w.data_ptr(), w.shape[1], S, H, L, A, act, m.data_ptr(), 1, ptrs.data_ptr(), max(S, 1),
                                         ptrs.data_ptr() + 8, max(A, 1), None, rows.data_ptr(), rows.data_ptr() + 4, max_batch, out.data_ptr() + 16, 0, stream)
        v = _agree(engine, 'serl_ga_novelty_general', _spec(S, A, H, L, act), max_batch, rc)
        assert not (max_batch != B and v.takes)
        _guards_ok(out, 1, v.takes)


def _distill_call(engine, general, S, A, H, L, act):
    """one pair, one Adam step on a minibatch of B of 8 rows -> (rc, child, its copy before the call)"""
    from serl_amd import _capi
    lib = _capi.lib()
    dev = engine.device
    ok = min(S, A, H) >= 1 and L >= 0
    P = _params(S, A, H, L) if ok else 4
    g = torch.Generator().manual_seed(S * 1000 + A)
    child = (0.3 * torch.randn(1, ((P + 3) & ~3) + 8, generator=g)).to(dev)          # (a row stride that is a multiple of 4 floats)
    before = child.clone()
    st = torch.randn(1, 8, max(S, 1), generator=g).to(dev)
    tg = torch.zeros(1, 8, max(A, 1), device=dev)
    kp = torch.ones(1, 8, device=dev)
    sl = torch.zeros(1, 1, 128, dtype=torch.int32, device=dev)
    ns, bt = torch.ones(1, dtype=torch.int32, device=dev), torch.full((1,), B, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    a = (engine.ctx, child.data_ptr(), child.shape[1], 1, S, H, L, A, act, st.data_ptr(), tg.data_ptr(), kp.data_ptr(), 8, sl.data_ptr(), 1,
         ns.data_ptr(), bt.data_ptr(), ctypes.c_float(1e-3))
    if general:
        nbytes = int(lib.serl_ga_distill_general_work_bytes(1, S, A, H, L))
        work = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
        rc = lib.serl_ga_distill_general(*a, work.data_ptr(), nbytes, 0, stream)
    else:
        rc = lib.serl_ga_distill(*a, stream)
    return rc, child, before, P


@pytest.mark.parametrize('general,S,A,H,L,act', [(False,) + c for c in DISTILL] + [(True,) + c for c in LEARNER])
def test_the_distillation_kernels_agree_with_the_query(engine, general, S, A, H, L, act):
    what = 'serl_ga_distill_general' if general else 'serl_ga_distill'
    rc, child, before, P = _distill_call(engine, general, S, A, H, L, act)
    v = _agree(engine, what, _spec(S, A, H, L, act), 1, rc)
    assert torch.equal(child[:, P:], before[:, P:])               # behind the row: never written
    if v.takes:
        assert not torch.equal(child[:, :P], before[:, :P])         # an Adam step moves every parameter it has a gradient for
    else:
        assert torch.equal(child, before)


# ---- serl_td3_train / serl_td3_train_big: one learner at the corners of the learner shape, and one step outside each bound ----------------
#   (S, A, H, L, activation, B, freq, iteration0, n_updates, caps, update_actor_target, rewards) of tests/td3_64.py; {B}: the entry's largest minibatch
TD3_LO = (1, 1, 4, 0, 'tanh', 1, 1, 0, 2, 0, 1, 'small')
TD3_HI = (16, 4, 128, 4, 'relu', '{B}', 1, 0, 2, 1, 1, 'small')
TD3_OUT_LO = [('hidden', 0), ('hidden', 2), ('hidden', 6), ('num_layers', -1), ('state_dim', 0), ('action_dim', 0), ('batch', 0), ('activation', -1),
              ('activation', 3)]
TD3_OUT_HI = [('hidden', 132), ('num_layers', 5), ('state_dim', 17), ('action_dim', 5), ('batch', '{B}+1')]


@pytest.mark.parametrize('what,bmax', [('serl_td3_train', 128), ('serl_td3_train_big', 512)])
def test_the_learner_agrees_with_the_query(engine, what, bmax):
    """the descriptor of tests/test_gpu_td3_big.py (guard rows and columns around every array, a NaN workspace).  In range: SERL_OK, the query
    takes, the rows move and the guards stand.  One field one step outside: the call's code and message are the query's -- the
    SERL_E_INVALID of a shape that is none, the SERL_E_UNSUPPORTED of one outside the compiled range -- and nothing at all is written.
    (The LDS refusal does not occur on this device: the tiles take ~135 KB.)"""
    import numpy as np
    import td3_64 as T
    import td3_big as TB
    import test_gpu_td3_big as GB
    from serl_amd import _capi
    big = what == 'serl_td3_train_big'
    for corner, outside in ((TD3_LO, TD3_OUT_LO), (TD3_HI, TD3_OUT_HI)):
        c = tuple(bmax if f == '{B}' else f for f in corner)
        d = (TB.make_case(c) if big and c[5] > 128 else T.make_case(c))
        la = GB.Launch(engine, [d])
        for field, value in outside:
            desc = la.desc()
            setattr(desc, field, bmax + 1 if value == '{B}+1' else value)
            desc.slot_cols = 600                                  # (not what refuses a batch of 129 or 513)
            if big:
                bd = _capi.Td3BigDesc(rng=None, dense=0)
                rc = la.L.serl_td3_train_big(engine.ctx, ctypes.byref(desc), ctypes.byref(bd), la.stream())
            else:
                rc = la.L.serl_td3_train(engine.ctx, ctypes.byref(desc), la.stream())
            spec = _spec(desc.state_dim, desc.action_dim, desc.hidden, desc.num_layers, desc.activation)
            v = _agree(engine, what, spec, desc.batch, rc)
            assert not v.takes and v.rc == (_capi.E_INVALID if value in (0, -1) or field == 'activation' else _capi.E_UNSUPPORTED), (field, value)
            la.assert_untouched()
        assert la.run(entry='big' if big else 'old') == 0
        assert _agree(engine, what, _spec(c[0], c[1], c[2], c[3], GB.G.ACT[c[4]]), c[5], 0).takes
        o = la.out()
        la.assert_guards(o)
        assert not np.array_equal(o['actor'][1, :la.Pa], la.host['actor'][1, :la.Pa]) and not np.array_equal(o['critic'][1, :la.Pc], la.host['critic'][1, :la.Pc])


# ---- serl_venv_rollout / _general / _wave: one env kind each side of every bound -------------------------------------------------------------
VENV_LANE32 = [(7, 3, 32, 0, 2), (7, 3, 32, 3, 0), (7, 3, 28, 1, 0), (7, 3, 36, 1, 0), (6, 3, 32, 1, 0), (8, 3, 32, 1, 0), (7, 2, 32, 1, 0), (7, 4, 32, 1, 0),
               (7, 3, 32, -1, 0), (7, 3, 32, 1, -1), (7, 3, 32, 1, 3)]
VENV_GENERAL = [(7, 3, 4, 0, 0), (7, 3, 128, 0, 1), (7, 3, 4, 16, 2), (7, 3, 0, 1, 0), (7, 3, 2, 1, 0), (7, 3, 6, 1, 0), (7, 3, 132, 1, 0), (7, 3, 4, -1, 0),
                (7, 3, 4, 17, 0), (6, 3, 4, 1, 0), (8, 3, 4, 1, 0), (7, 2, 4, 1, 0), (7, 4, 4, 1, 0), (7, 3, 4, 1, -1), (7, 3, 4, 1, 3)]
VENV_SYMMETRIC = [(2, 1, 4, 0, 0), (2, 1, 32, 1, 0), (7, 3, 4, 0, 0), (7, 3, 32, 1, 0), (3, 1, 4, 0, 0)]


def _venv_calls(engine, env, entry, cases):
    """K = 3 steps of every env through the C entry with one member of zero weights: the call against the query (whose message carries the
    name of the contract's first entry point), the outputs' sentinels and the env state"""
    from serl_amd import _capi
    K = 3
    env.reset()
    wd = torch.zeros(1, 4096, dtype=torch.float32, device=env.device)          # room for every shape that is taken: at most 1 411 parameters
    contract = 'serl_venv_rollout' if entry == 'serl_venv_rollout' else 'serl_venv_rollout_general'
    took = 0
    for S, A, H, L, act in cases:
        assert not (S == env.state_dim and A == env.action_dim and 4 <= H <= 128 and 0 <= L <= 16) or \
            H * S + H + L * (H * H + 3 * H) + A * H + A <= wd.shape[1]
        out = env._rollout_buffers(K, False, True)
        for k in ('obs', 'actions', 'reward', 'final_obs', 'x', 'ref', 't'):
            out[k].fill_(SENT)
        torch.cuda.synchronize(env.device)
        state0 = env._state.clone()
        rd = _capi.VenvRolloutDesc(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, n_members=1, weights=wd.data_ptr(),
                                   weight_stride=wd.shape[1], n_steps=K, **{k: out[k].data_ptr() for k in out})
        rc = getattr(engine.lib, entry)(engine.ctx, ctypes.byref(env.desc), ctypes.byref(env.auto_desc), ctypes.byref(rd), env._stream())
        message = engine.lib.serl_last_error().decode() if rc else ''
        torch.cuda.synchronize(env.device)
        v = _capi.shape_query(contract, _spec(S, A, H, L, act), int(env.env_config) + 3 * bool(env.incremental))
        assert rc == v.rc and (rc == 0) == v.takes, (entry, S, A, H, L, act, rc, message)
        assert message == (entry + v.message[len(contract):] if rc else ''), (entry, S, A, H, L, act)
        if v.takes:
            took += 1
            assert not bool((out['obs'] == SENT).any()) and not bool((out['reward'] == SENT).any()) and not torch.equal(env._state, state0)
        else:
            assert all(bool((out[k] == SENT).all()) for k in ('obs', 'actions', 'reward', 'final_obs', 'x', 'ref', 't')) and torch.equal(env._state, state0)
    return took


def test_the_env_rollouts_agree_with_the_query(engine):
    import test_gpu_venv_rollout_general as G
    import test_gpu_venv_rollout_wave as RW
    from actor_shapes import _shape, SYMMETRIC
    N = 4
    lane = G._venv(N, 'nominal', engine, **G._env_kw('nominal', N))
    assert _venv_calls(engine, lane, 'serl_venv_rollout', VENV_LANE32) == 2
    assert _venv_calls(engine, lane, 'serl_venv_rollout_general', VENV_GENERAL) == 3
    wave = RW._venv(N, 'nominal', RW.T_SHORT, engine, **G._env_kw('nominal', N))
    assert _venv_calls(engine, wave, 'serl_venv_rollout_wave', VENV_GENERAL) == 3
    mode = G._mode_of(_shape(12, 2, 'tanh', SYMMETRIC))
    sym = G._venv(N, mode, engine, **G._env_kw(mode, N))
    assert _venv_calls(engine, sym, 'serl_venv_rollout_general', VENV_SYMMETRIC) == 2
    assert _venv_calls(engine, sym, 'serl_venv_rollout', [(7, 3, 32, 1, 0), (2, 1, 32, 1, 0)]) == 0          # not the attitude task


# ---- distil_batch: one entry point per resolution, counted on real rings --------------------------------------------------------------------
@pytest.mark.parametrize('kernel,fused_how,general_how,want', [
    ('serl50', 'takes', 'range', ['serl_ga_distill']), ('auto', 'takes', 'takes', ['serl_ga_distill']),
    ('auto', 'lds', 'takes', ['serl_ga_distill_general']), ('general', 'takes', 'takes', ['serl_ga_distill_general']),
    ('general', 'takes', 'range', 'error'), ('serl50', 'range', 'takes', []), ('auto', 'range', 'lds', [])])
def test_distil_batch_makes_exactly_one_call_per_resolution(engine, golden, monkeypatch, kernel, fused_how, general_how, want):
    """distil_batch with one pair on device rings, the query answering as told and the two training entry points replaced by counters
    (the rest of the library is the real one): the entry point the table names is called once, PyTorch trains where the table says so with
    neither called, and a refused 'general' raises before any call and any draw.  (The workspace's size function launches nothing.)"""
    import random
    from serl_amd import _capi, distill
    from test_ga_host import distill_case
    from test_shapes_host import verdict
    args, spec, w, bufs, critic, seed, _ = distill_case(golden, 'd_18_0', engine.device, engine)
    args.individual_bs = 300
    real, calls = _capi.lib(), []

    class Counting:
        def __getattr__(self, name):
            if name in ('serl_ga_distill', 'serl_ga_distill_general'):
                return lambda *a: calls.append(name) or 0
            return getattr(real, name)
    monkeypatch.setattr(_capi, 'lib', lambda: Counting())
    answers = {'serl_ga_distill': fused_how, 'serl_ga_distill_general': general_how}
    monkeypatch.setattr(_capi, 'shape_query', lambda what, *a, **k: verdict(what, answers[what]))
    random.seed(seed); torch.manual_seed(seed)
    st, tst = random.getstate(), torch.get_rng_state()
    info = {}
    if want == 'error':
        with pytest.raises(RuntimeError, match='refused for ' + general_how):
            distill.distil_batch(args, engine, spec, w, [(0, 1)], bufs, critic, kernel=kernel, info=info)
        assert calls == [] and info == {} and random.getstate() == st and torch.equal(torch.get_rng_state(), tst)
        return
    got = distill.distil_batch(args, engine, spec, w, [(0, 1)], bufs, critic, kernel=kernel, info=info)
    assert calls == want and len(got) == 1
    assert info['path'] == {(): 'torch', ('serl_ga_distill',): 'fused', ('serl_ga_distill_general',): 'fused-general'}[tuple(want)]

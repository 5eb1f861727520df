"""Every rollout kernel family at every actor shape of the grid in tests/actor_shapes.py (hidden 4 .. 128, 0 .. 16 layers, the three
activations, the general env configurations) against the CPU oracle bit for bit -- the product's stated contract -- and the actions
against the reference's Actor in float64 (the tolerance tests/test_oracle_actor_shapes.py establishes for the oracle).  Behind the
C ABI's shape checks the forward pass is about ten shape-specialised implementations (rollout_device.h): small<32> / <64>,
chunked<72> / <96>, the generic wave pass, its general-env form, the LDS actor, cu<72 / 96 / 128>, the split actor, half32 /
quarter32, lane32 / lane32_t; which one runs depends on the shape and on the family, so every family that accepts a shape runs it,
and every launch asserts the family that ran.  Shapes the ABI refuses must be refused, not run."""
import contextlib, os, types
import numpy as np
import pytest
import torch
import actor_shapes as X
from test_gpu_rollout import kernel, ran, _oracle

pytestmark = pytest.mark.gpu
N_MEMBERS = 5                                    # not a multiple of 64: serl_regroup_weights_kernel pads the last group
MOE = np.array([0, 1, 2, 3, 4, 2, 1])            # episodes of different members, one member twice


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope='module')
def engines(engine):
    """contexts created under the development overrides that select the other families (read once, at context creation)"""
    import serl_amd
    with _env(SERL_REMOTE_ACTOR=0):
        same_cu = serl_amd.RolloutEngine(0)                  # H = 72 / 96 / 128: the seven-wavefront team with a streamed actor (teams)
    with _env(SERL_REMOTE_ACTOR=0, SERL_SPLIT_ACTOR=1):
        split = serl_amd.RolloutEngine(0)                    # 64 < H <= 128: two actor wavefronts share one forward pass (teams2)
    with _env(SERL_LANE_WEIGHTS='rows'):
        rows = serl_amd.RolloutEngine(0)                     # H = 32 lanes walk the member rows (lane32) instead of regrouped weights (lane32_t)
    yield types.SimpleNamespace(default=engine, same_cu=same_cu, split=split, rows=rows)
    for e in (same_cu, split, rows):
        e.close()


def _launches(s, eng):
    """(label, engine, kernel-block mode, lanes_per_wave, families the launch must report) of every family that accepts shape s"""
    H, L = s['hidden'], s['num_layers']
    general = s['env_config'] != X.ATTITUDE or s['incremental']
    if general:
        return [('teamx', eng.default, 'team', 0, ('teamx',)), ('wavex', eng.default, 'wave', 0, ('wavex',))]
    team = 'teamr' if H in (72, 96, 128) else ('team' if H == 32 and L <= 3 else 'teams')
    out = [('wave', eng.default, 'wave', 0, ('wave',)), (team, eng.default, 'team', 0, (team,)),
           ('team2', eng.default, 'team2', 0, ('team2' if H == 32 else 'team2s',)),
           ('lane1', eng.default, 1, 1, ('lane',)), ('lane8', eng.default, 8, 8, ('lane',))]
    if H in (72, 96, 128):
        out.append(('teams', eng.same_cu, 'team', 0, ('teams',)))
    if 64 < H <= 128:
        out.append(('teams2', eng.split, 'team', 0, ('teams2',)))
    if H == 32:
        out += [('team4', eng.default, 'team4', 0, ('team4',)), ('half', eng.default, 'half', 0, ('half',)),
                ('lane8_rows', eng.rows, 8, 8, ('lane',))]
    return out


@pytest.mark.parametrize('s', X.GRID, ids=X.shape_id)
def test_every_family_at_every_shape_vs_oracle_and_float64(engines, s):
    i = X.GRID.index(s)
    w = X.make_weights(s, N_MEMBERS, 100 + i)
    ref = X.references(len(MOE), seed=3 + i)
    kw = dict(t_max=X.T_MAX, transitions=True, env_config=s['env_config'], incremental=s['incremental'])
    o = _oracle(w, X.net_of(s), MOE, ref, traces=True, threads=7, **kw)
    X.check_actions_f64(s, w, MOE, o['transitions'], o['length_steps'], X.shape_id(s) + ' oracle')
    spec = X.spec_of(s)
    A = s['action_dim']
    for label, eng, mode, lanes, families in _launches(s, engines):
        what = '%s %s' % (X.shape_id(s), label)
        with kernel(mode, eng):
            out = eng.rollout(torch.from_numpy(w), spec, MOE, ref, traces='actions', lanes_per_wave=lanes, **kw)
            ran(eng, *families)
        got = {k: v.cpu().numpy() for k, v in out.items() if torch.is_tensor(v)}
        for key in ('fitness', 'length_steps', 'length_t', 'cost_steps'):
            np.testing.assert_array_equal(got[key], o[key], err_msg='%s: %s' % (what, key))
        for e, n in enumerate(o['length_steps']):
            np.testing.assert_array_equal(got['actions'][e, :n], o['actions'][e, :n], err_msg='%s: actions of episode %d' % (what, e))
            np.testing.assert_array_equal(got['transitions'][e, :n], o['transitions'][e, :n], err_msg='%s: transitions of episode %d' % (what, e))
        assert not got['actions'][:, :, A:].any()
        X.check_actions_f64(s, w, MOE, got['transitions'], got['length_steps'], what)


def _refused(eng, spec, moe, ref, rc, **kw):
    """the call must fail with status rc and launch nothing (the record of the last launch stays what it was)"""
    before = eng.last_rollout_info()
    with pytest.raises(RuntimeError, match=r'serl_rollout failed \(%d\)' % rc):
        eng.rollout(torch.zeros(len(set(moe)), (spec.param_count + 3) // 4 * 4), spec, moe, ref, t_max=1, **kw)
    assert eng.last_rollout_info() == before


def test_shapes_the_abi_refuses(engine):
    """serl_check_desc: hidden outside 4 .. 128 or not a multiple of 4 (dwordx4 row loads), more than 16 layers, an unknown activation,
    four-per-team / two-per-wavefront at H != 32, lane-per-episode kernels with a general env configuration"""
    import serl_amd
    E_INVALID, E_UNSUPPORTED = -1, -3
    ref = X.references(2, t_max=1)
    s32 = X.GRID[X.GRID.index(X._shape(32, 3))]
    w = X.make_weights(s32, 2, 0)
    engine.rollout(torch.from_numpy(w), X.spec_of(s32), [0, 1], ref, t_max=1)           # a launch on record
    for H, L in ((2, 3), (130, 3), (132, 1), (6, 3), (34, 1), (126, 0), (32, 17), (4, 17)):
        _refused(engine, serl_amd.NetSpec(7, 3, H, L, 'tanh'), [0, 1], ref, E_UNSUPPORTED)
    bad_act = types.SimpleNamespace(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation='?', activation_id=3,
                                    param_count=serl_amd.NetSpec(7, 3, 32, 3, 'tanh').param_count)
    _refused(engine, bad_act, [0, 1], ref, E_INVALID)
    for mode in ('team4', 'half'):
        for H in (64, 72, 96, 128, 4):
            _refused(engine, serl_amd.NetSpec(7, 3, H, 3, 'tanh'), [0, 1], ref, E_UNSUPPORTED, kernel=mode)
    for cfg, incr, S, A in ((X.SYMMETRIC, False, 2, 1), (X.FULL, True, 16, 3), (X.ATTITUDE, True, 10, 3)):
        for lanes in (1, 8):
            _refused(engine, serl_amd.NetSpec(S, A, 32, 3, 'tanh'), [0, 1], ref, E_UNSUPPORTED, env_config=cfg, incremental=incr, lanes_per_wave=lanes)

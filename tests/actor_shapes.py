"""Shared by tests/test_oracle_actor_shapes.py (CPU) and tests/test_gpu_actor_shapes.py (GPU): the grid of actor shapes the C ABI
accepts, seeded weights built by the reference's Actor module, the float64 forward pass and the tolerance the f32 actors must meet
against it.  A plain module (not a conftest): nothing here is a fixture."""
import types
import numpy as np
import torch

ATTITUDE, SYMMETRIC, FULL = 0, 1, 2          # serl_env_config


def _env_dims(cfg, incr):
    A = 1 if cfg == SYMMETRIC else 3
    return A + {ATTITUDE: 4, SYMMETRIC: 1, FULL: 10}[cfg] + (A if incr else 0), A


def _shape(H, L, act='tanh', cfg=ATTITUDE, incr=False):
    S, A = _env_dims(cfg, incr)
    return dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=act, env_config=cfg, incremental=bool(incr))


# A covering set, not a product: every hidden size the ABI range holds in the classes the forward implementations split on (below 16,
# not a multiple of 16 / 32, the specialised 32 / 64 / 72 / 96 / 128 and their neighbours), every layer count class (0, 1, 2, 3, 4, 16 --
# 16 only at small H: the runtime), every activation at 32 / 64 / 96 / 128 and at a few odd sizes, and the general env configurations.
GRID = ([_shape(H, 3) for H in (4, 8, 12, 20, 32, 36, 48, 60, 64, 68, 72, 76, 96, 100, 124, 128)]
        + [_shape(32, L) for L in (0, 1, 2, 4, 16)]
        + [_shape(64, L) for L in (0, 1, 2, 4)]
        + [_shape(72, L) for L in (0, 1, 4)]
        + [_shape(96, L) for L in (0, 2)]
        + [_shape(128, L) for L in (0, 1, 2)]
        + [_shape(4, 16), _shape(8, 16), _shape(12, 0), _shape(20, 1), _shape(100, 1), _shape(124, 0)]
        + [_shape(H, L, act) for act in ('elu', 'relu') for H, L in ((32, 3), (32, 1), (64, 3), (96, 3), (128, 3), (72, 2), (20, 4), (8, 16))]
        + [_shape(H, 1, 'elu') for H in (100,)] + [_shape(H, 0, 'relu') for H in (64,)]
        + [_shape(H, L, act, SYMMETRIC) for H, L, act in ((4, 0, 'tanh'), (32, 3, 'elu'), (64, 1, 'relu'), (12, 2, 'tanh'))]
        + [_shape(H, L, act, FULL) for H, L, act in ((32, 1, 'tanh'), (72, 3, 'relu'), (96, 0, 'elu'), (20, 3, 'tanh'))]
        + [_shape(H, L, act, SYMMETRIC, True) for H, L, act in ((8, 1, 'tanh'), (64, 3, 'relu'))]
        + [_shape(H, L, act, ATTITUDE, True) for H, L, act in ((32, 2, 'elu'), (100, 1, 'tanh'))]
        + [_shape(H, L, act, FULL, True) for H, L, act in ((48, 3, 'tanh'), (128, 1, 'relu'))])


def shape_id(s):
    env = {ATTITUDE: 'att', SYMMETRIC: 'sym', FULL: 'full'}[s['env_config']] + ('_inc' if s['incremental'] else '')
    return '%s_S%dA%d_H%d_L%d_%s' % (env, s['state_dim'], s['action_dim'], s['hidden'], s['num_layers'], s['activation'])


def net_of(s):
    """the oracle's net dict"""
    return {k: s[k] for k in ('state_dim', 'action_dim', 'hidden', 'num_layers', 'activation')}


def spec_of(s):
    import serl_amd
    return serl_amd.NetSpec(s['state_dim'], s['action_dim'], s['hidden'], s['num_layers'], s['activation'])


def actor_module(s, dtype=torch.float32):
    from serl_amd.actor import Actor
    args = types.SimpleNamespace(state_dim=s['state_dim'], action_dim=s['action_dim'], hidden_size=s['hidden'], num_layers=s['num_layers'],
                                 activation_actor=s['activation'], device='cpu')
    return Actor(args).to(dtype)


OUT_SCALE = 0.6         # output layer of the default init scaled down: actions mostly out of tanh saturation (a saturated tanh hides the hidden layers)


def make_weights(s, n_members, seed):
    """f32 [n_members, row_stride] packed rows of reference Actors, seeded: torch's default init of every Linear, LayerNorm gamma in
    [0.5, 2] and beta ~ N(0, 0.3) (away from 1 and 0: the affine parameters matter), the output layer scaled by OUT_SCALE; in the full
    configuration the layer-0 columns of airspeed and altitude scaled to their magnitude"""
    from serl_amd.actor import pack_actor, pad_rows
    gen = torch.Generator().manual_seed(seed)
    rows = []
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        for _ in range(n_members):
            m = actor_module(s)
            with torch.no_grad():
                for name, p in m.named_parameters():
                    if name.endswith('gamma'):
                        p.copy_(0.5 + 1.5 * torch.rand(p.shape, generator=gen))
                    elif name.endswith('beta'):
                        p.copy_(0.3 * torch.randn(p.shape, generator=gen))
                if s['env_config'] == FULL:         # airspeed (~90 m/s) and altitude (~2 000 m) are observed unscaled: keep layer 0 out of saturation
                    m.net[0].weight[:, s['action_dim'] + 3].mul_(1e-2)
                    m.net[0].weight[:, s['action_dim'] + 9].mul_(5e-4)
                out = m.net[-2]
                out.weight.mul_(OUT_SCALE)
                out.bias.mul_(OUT_SCALE)
            rows.append(pack_actor(m))
    return pad_rows(torch.stack(rows)).numpy()


def forward64(s, row, obs):
    """the reference's Actor in float64 on f32 observations [n, S] (cast exactly) -> f64 actions [n, A]"""
    from serl_amd.actor import unpack_into
    m = actor_module(s, torch.float64)
    unpack_into(m, torch.from_numpy(np.asarray(row, dtype=np.float64)))
    with torch.no_grad():
        return m(torch.from_numpy(np.asarray(obs, dtype=np.float64))).numpy()


TOL_SCALE = 4.0


def action_tolerance(s):
    """Bound on |a_f32 - a_f64| of one forward pass.  Every f32 dot product of length n carries a relative rounding error of the
    order sqrt(n) u (u = 2^-24, random-walk growth of n roundings) of the magnitude of its terms, and each LayerNorm divides by a
    standard deviation that can be small against the values it centres -- the relative error it passes on grows by the ratio;
    layers add their errors.  Calibrated on the oracle over this grid (tests/test_oracle_actor_shapes.py: 5 members, 6 episodes of
    3 s per shape, every step): |a_f32 - a_f64| / (sqrt(H) (L + 1) u) peaks at 0.55 (H = 32, L = 16, tanh; other seeds up to 0.9) and
    stays below 0.3 elsewhere; the largest absolute difference is 3e-6.  TOL_SCALE = 4 leaves a margin of 4x over the worst case seen
    and still sits two to four orders of magnitude below what a wrong LayerNorm divisor (H instead of H - 1: ~1e-3 in an action), a
    dropped block of a sum or a shifted weight offset move an action by."""
    H, L = s['hidden'], s['num_layers']
    return TOL_SCALE * np.sqrt(H) * (L + 1) * 2.0 ** -24


MIN_STEPS = 100         # every episode of a case flies at least 1 s of model time: no case passes on an episode that ended at once
T_MAX = 3.0
MIN_UNSATURATED = 0.9   # fraction of the actions with |a| < 0.9 (make_weights keeps the output layer out of saturation)


def check_actions_f64(s, w, moe, tr, length_steps, what=''):
    """open loop, per step: every stored action against the float64 forward pass of its member on the stored f32 observation"""
    S, A = s['state_dim'], s['action_dim']
    tol = action_tolerance(s)
    worst, n_all, n_unsat = 0.0, 0, 0
    for e, n in enumerate(np.asarray(length_steps)):
        assert n >= MIN_STEPS, '%s: episode %d flew %d steps only' % (what, e, n)
        obs, act = tr[e, :n, :S], tr[e, :n, S:S + A].astype(np.float64)
        ref = forward64(s, w[moe[e]], obs)
        err = np.abs(act - ref).max()
        worst = max(worst, err)
        assert err <= tol, '%s: episode %d (member %d): |a - a_f64| = %.3g > %.3g' % (what, e, moe[e], err, tol)
        n_all += act.size; n_unsat += int((np.abs(act) < 0.9).sum())
    assert n_unsat >= MIN_UNSATURATED * n_all, '%s: only %d of %d actions below 0.9 in magnitude' % (what, n_unsat, n_all)
    return worst


def references(n_episodes, t_max=T_MAX, seed=5):
    """per-episode reference tables of t_max seconds: the base reference and seeded step sequences"""
    from serl_amd import refsignals
    return refsignals.synthetic_reference_tables(n_episodes, 3, 20, seed=seed)[:, :refsignals.n_steps_for(t_max)]

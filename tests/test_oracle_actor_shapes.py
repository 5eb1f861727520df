"""The oracle's actor (oracle/rollout_ref.c actor_forward) against the reference's Actor evaluated in float64, at every shape of the
grid in tests/actor_shapes.py -- hidden sizes 4 .. 128, 0 .. 16 layers, the three activations, the general env configurations.
The golden vectors pin the oracle at three shapes only (H = 32 / 72 / 96, three layers); this establishes it everywhere the C ABI
accepts an actor, which is what makes the GPU suite's bit-for-bit comparison with the oracle meaningful at those shapes
(tests/test_gpu_actor_shapes.py).  Open loop, per step: the f32 observation the actor was fed and the f32 action it returned, from
every stored transition of short closed-loop episodes (free of the closed loop's amplification of rounding)."""
import numpy as np
import pytest
import actor_shapes as X


@pytest.mark.parametrize('s', X.GRID, ids=X.shape_id)
def test_oracle_actor_vs_float64_reference(s):
    from oracle import rollout as R
    i = X.GRID.index(s)
    w = X.make_weights(s, 5, 100 + i)
    moe = np.array([0, 1, 2, 3, 4, 2])
    ref = X.references(len(moe), seed=3 + i)
    o = R.rollout(w, X.net_of(s), moe, ref, t_max=X.T_MAX, traces=True, transitions=True, env_config=s['env_config'], incremental=s['incremental'],
                  threads=6)
    worst = X.check_actions_f64(s, w, moe, o['transitions'], o['length_steps'], X.shape_id(s))
    assert worst > 0.0, 'an f32 forward pass that equals the f64 one at every step: the comparison is not looking at the actor'
    # the stored action is the one the episode flew: its scaled deflection is the command trace (phlabenv.py:72-73, f32 part)
    if not s['incremental']:
        A, S = s['action_dim'], s['state_dim']
        bound = 10.0 * np.pi / 180.0
        for e, n in enumerate(o['length_steps']):
            a = o['transitions'][e, :n, S:S + A]
            u = -bound + (0.5 * (a + np.float32(1.0))).astype(np.float32).astype(np.float64) * (2 * bound)
            np.testing.assert_array_equal(o['actions'][e, :n, :A], u)


def test_grid_covers_the_shapes_the_abi_accepts():
    """the covering set holds what the forward implementations split on"""
    att = [s for s in X.GRID if s['env_config'] == X.ATTITUDE and not s['incremental']]
    assert {s['hidden'] for s in att} >= {4, 8, 12, 20, 32, 36, 48, 60, 64, 68, 72, 76, 96, 100, 124, 128}
    assert {s['num_layers'] for s in att} >= {0, 1, 2, 3, 4, 16}
    assert all(s['hidden'] <= 32 for s in X.GRID if s['num_layers'] == 16)
    for act in ('tanh', 'elu', 'relu'):
        assert {32, 64, 96, 128} <= {s['hidden'] for s in att if s['activation'] == act}, act
    envs = {(s['env_config'], s['incremental'], s['state_dim'], s['action_dim']) for s in X.GRID}
    assert envs >= {(X.SYMMETRIC, False, 2, 1), (X.FULL, False, 13, 3), (X.SYMMETRIC, True, 3, 1), (X.ATTITUDE, True, 10, 3), (X.FULL, True, 16, 3)}
    assert all(4 <= s['hidden'] <= 128 and s['hidden'] % 4 == 0 for s in X.GRID)

"""What a call launches is what the host planner says it launches: serl_last_rollout_info after a real call equals RolloutEngine.plan_rollout() for the
engine's CU count, for every family a handful of episodes can reach (kernel hints, lanes_per_wave, a general env configuration, the noise entry, the
open-loop entry).  At most 9 episodes of 3 env steps under a zero actor; what the kernels return is checked elsewhere (test_gpu_rollout.py ...)."""
import numpy as np
import pytest
import torch
import serl_amd
from serl_amd import builds

pytestmark = pytest.mark.gpu
REF = np.zeros((3, 3))      # three rows: max_steps = 3
INFO = ('family', 'workgroups', 'episodes_per_team', 'work_queue', 'actor_wavefronts', 'actor_streamed', 'launches', 'code')


def _spec(H=32, L=3, env=(0, False)):
    return serl_amd.NetSpec(*builds.env_dims(*env), H, L, 'tanh')


def _fly(engine, spec, n, env=(0, False), **kw):
    out = engine.rollout(torch.zeros(1, spec.row_stride), spec, np.zeros(n, np.int32), REF, t_max=0.025, env_config=env[0], incremental=env[1], sync=False, **kw)
    torch.cuda.synchronize()
    assert (out['length_steps'].cpu().numpy() != 0).all()      # (every episode ran)
    return engine.last_rollout_info()


CALLS = [('team', 32, {}), ('team2', 32, {}), ('team4', 32, {}), ('half', 32, {}), ('wave', 32, {}), ('laneq', 32, {}),
         ('team', 72, {}), ('team2', 72, {}), (None, 32, dict(lanes_per_wave=4)), (None, 32, dict(concurrent_episodes=5))]


@pytest.mark.parametrize('kernel,H,kw', CALLS)
def test_rollout_launches_its_plan(engine, kernel, H, kw):
    spec = _spec(H, 3 if H == 32 else 1)
    got = _fly(engine, spec, 9, kernel=kernel, **kw)
    plan = engine.plan_rollout(spec, 9, kernel=kernel, **kw)
    assert got == {k: plan[k] for k in INFO}, (got, plan)
    assert plan['family'] == {'laneq': 'lane', None: 'lane' if 'lanes_per_wave' in kw else 'team'}.get(kernel, kernel if H == 32 else {'team': 'teamr', 'team2': 'team2s'}[kernel])


@pytest.mark.parametrize('kernel', ['team', 'wave'])
def test_general_env_launches_its_plan(engine, kernel):
    env = (1, False)
    spec = _spec(32, 1, env)
    got = _fly(engine, spec, 9, env=env, kernel=kernel)
    plan = engine.plan_rollout(spec, 9, kernel=kernel, env_config=env[0], incremental=env[1])
    assert got == {k: plan[k] for k in INFO} and plan['family'] == {'team': 'teamx', 'wave': 'wavex'}[kernel], (got, plan)


@pytest.mark.parametrize('kw', [dict(kernel='wave'), dict(lanes_per_wave=4)])
def test_noise_entry_launches_its_plan(engine, kw):
    spec = _spec()
    got = _fly(engine, spec, 9, sensor_noise='device', noise_seed=7, **kw)
    plan = engine.plan_rollout(spec, 9, noise=True, **kw)
    assert got == {k: plan[k] for k in INFO} and plan['family'] == ('wave' if 'kernel' in kw else 'lane'), (got, plan)


@pytest.mark.parametrize('kw', [dict(kernel='team'), dict(kernel='wave'), dict(lanes_per_wave=4)])
def test_open_loop_launches_its_plan(engine, kw):
    engine.dynamics_open_loop(np.zeros((9, 3, 10)), **kw)
    got = engine.last_rollout_info()
    plan = engine.plan_rollout(None, 9, open_loop=True, **kw)
    assert got == {k: plan[k] for k in INFO} and not plan['actor_streamed'], (got, plan)


def test_kernel_time_after_a_timed_call_only(engine):
    spec = _spec()
    _fly(engine, spec, 9)
    assert engine.kernel_ms() > 0.0
    _fly(engine, spec, 9, concurrent_episodes=5)
    with pytest.raises(RuntimeError, match='no rollout recorded'):
        engine.kernel_ms()
    _fly(engine, spec, 9, kernel='team4')
    assert engine.kernel_ms() > 0.0

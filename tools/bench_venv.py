#!/usr/bin/env python3
"""Throughput of the step-wise vector env (serl_amd.CitationVecEnv, C ABI v9 serl_venv_step) on the GPU box:
    python tools/bench_venv.py [--sizes 1024,8192,65536] [--steps 2001] [--warmup 50]
One JSON line: env-steps/s and microseconds per `step` call at each N, in three configurations --
    env        a fixed action tensor (the env alone)
    mlp        a torch SERL50-shaped actor (7 -> 32 tanh, 3 x [32 LayerNorm tanh], -> 3 tanh; the shipped actor 18) on the same stream,
               closed loop, no host synchronisation inside the loop
    fused      for reference: the fused lane rollout (lanes_per_wave = 64: actor + env + dynamics in one kernel) at the same N
-- timed with device events after a warm-up, every env flying the base reference (one shared table) from a fresh reset; only live env
steps count (a done env is frozen and costs little).  Also the resource usage of the new kernels (tools/kernel_regs.sh on the build's objects)."""
import argparse, json, os, subprocess, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import serl_amd
from serl_amd import refsignals as rs


def serl50_policy(device):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'actors.npz'))['serl50'][18]
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    layers = {}
    for name, o, shape in spec.param_layout():
        layers[name] = torch.from_numpy(g[o:o + int(np.prod(shape))].reshape(shape).copy())
    a = serl_amd.Actor(argparse.Namespace(hidden_size=32, num_layers=3, activation_actor='tanh', state_dim=7, action_dim=3, device=torch.device('cpu')))
    a.load_state_dict(layers)
    return a.to(device).eval()


def live_steps(t_final, dt=0.01):
    """env steps taken: a done env's t is frozen at its last step"""
    return int(np.rint(t_final.cpu().numpy() / dt).sum())


def bench_env(eng, N, steps, warmup, ref, policy=None):
    env = serl_amd.CitationVecEnv(N, mode='nominal', t_max=20, refs=ref, engine=eng)
    dev = env.device
    fixed = torch.zeros(N, 3, dtype=torch.float32, device=dev)
    with torch.no_grad():
        obs = env.reset()
        for _ in range(warmup):
            obs, _, _, _ = env.step(policy(obs.float()) if policy is not None else fixed)
        obs = env.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            obs, rew, done, info = env.step(policy(obs.float()) if policy is not None else fixed)
        e1.record()
        e1.synchronize()
    ms = e0.elapsed_time(e1)
    n = live_steps(info['t'])
    return dict(N=N, config='mlp' if policy is not None else 'env', calls=steps, ms=round(ms, 3), us_per_call=round(1e3 * ms / steps, 2),
                live_env_steps=n, env_steps_per_s=round(n / (ms * 1e-3), 1), done_at_end=int(done.sum()))


def bench_fused(eng, N, ref, warmup):
    w = torch.from_numpy(np.load(os.path.join(ROOT, 'tests', 'golden', 'actors.npz'))['serl50'][[18]])
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    moe = np.zeros(N, np.int32)
    if warmup:
        eng.rollout(w, spec, moe, ref, t_max=20, lanes_per_wave=64)
    out = eng.rollout(w, spec, moe, ref, t_max=20, lanes_per_wave=64)
    ms = eng.last_kernel_ms
    n = int(out['length_steps'].abs().sum())
    return dict(N=N, config='fused', calls=1, ms=round(ms, 3), us_per_call=None, live_env_steps=n, env_steps_per_s=round(n / (ms * 1e-3), 1))


def kernel_report():
    rep = {}
    for v in ('nominal', 'ice', 'cg_timed', 'gust', 'test'):
        obj = os.path.join(ROOT, 'serl_amd', 'csrc', 'build', 'rollout_%s.o' % v)
        try:
            r = subprocess.run(['bash', os.path.join(ROOT, 'tools', 'kernel_regs.sh'), obj, 'venv'], capture_output=True, text=True, timeout=120)
        except Exception as ex:
            return {'error': str(ex)[:200]}
        for line in r.stdout.splitlines():
            if '.name:' not in line:
                continue
            f = dict(p.strip().split(': ', 1) for p in line.split('\t') if ': ' in p)
            name = f['.name'].strip()
            kind = 'step' if 'step' in name else 'reset'
            rep['%s_%s' % (kind, v)] = dict(vgpr=int(f['.vgpr_count']), vgpr_spill=int(f['.vgpr_spill_count']), sgpr_spill=int(f['.sgpr_spill_count']),
                                            lds_bytes=int(f['.group_segment_fixed_size']), scratch_bytes=int(f['.private_segment_fixed_size']))
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='1024,8192,65536')
    ap.add_argument('--steps', type=int, default=2001)
    ap.add_argument('--warmup', type=int, default=50)
    ap.add_argument('--no-fused', action='store_true')
    args = ap.parse_args()
    eng = serl_amd.RolloutEngine(0)
    ref = rs.tabulate(*rs.base_reference(20), 20)
    policy = serl50_policy(eng.device)
    res = []
    for N in (int(s) for s in args.sizes.split(',')):
        res.append(bench_env(eng, N, args.steps, args.warmup, ref))
        res.append(bench_env(eng, N, args.steps, args.warmup, ref, policy))
        if not args.no_fused:
            res.append(bench_fused(eng, N, ref, args.warmup))
    print(json.dumps(dict(tool='bench_venv', device=torch.cuda.get_device_name(0), steps=args.steps, results=res, kernels=kernel_report())))


if __name__ == '__main__':
    main()

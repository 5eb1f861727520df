#!/usr/bin/env python
"""One epoch's distillation crossovers: PyTorch pair by pair, serl_ga_distill (hidden 32 x 3 only) and serl_ga_distill_general with its
dense phases on the VALU and on the f32 matrix cores, on the same GPU, the same rings and the same seeds.

Per shape (hidden 32 / 72 / 96, 3 hidden layers, S 7, A 3, tanh): a population of --pairs + 1 actors with rings of random transitions,
--pairs distillations (member i with member i + 1), child buffers of --rows rows (individual_bs), so 12 x (rows // 128) Adam steps of
128 rows per pair.  Two figures per path:
  kernel ms   device events around the one launch distil_batch makes
  wall ms     distill.distil_batch end to end, synchronised: host draws, the parents' actions and the Q-filter, uploads, the launch
both from the same --reps runs after a warm-up run of each path, the paths alternating; median [min .. max].
The PyTorch path (distill.distilation_crossover, what kernel='serl50' falls back to off hidden 32 x 3) is timed on --torch-pairs of
the pairs, once after a one-pair warm-up, and reported per pair and scaled to --pairs (it is a serial loop over pairs: the scaling is
exact up to the pairs' equal lengths).  The children of all paths are checked against the PyTorch ones of the pairs it trained.
Results, with the source hash, go to profiles/distill_general_timing.json.

  python tools/bench_distill.py
  python tools/bench_distill.py --hidden 72 --pairs 15 --rows 3000 --reps 5 --torch-pairs 3
"""
import argparse, json, os, random, statistics, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

S, A, L, ACT = 7, 3, 3, 'tanh'


class TwinQ(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q1 = torch.nn.Sequential(torch.nn.Linear(S + A, 64), torch.nn.ELU(), torch.nn.Linear(64, 1))
        self.q2 = torch.nn.Sequential(torch.nn.Linear(S + A, 64), torch.nn.ELU(), torch.nn.Linear(64, 1))

    def forward(self, s, a):
        x = torch.cat([s, a], -1)
        return self.q1(x), self.q2(x)


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': len(v)}


def population(engine, H, n, rows, seed):
    import actor_shapes as X
    import serl_amd
    from serl_amd import replay
    s = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=ACT, env_config=0, incremental=False)
    w = torch.from_numpy(X.make_weights(s, n, seed)).to(engine.device)
    rng = np.random.default_rng(seed)
    bufs = []
    for _ in range(n):
        r = replay.DeviceReplay(10_000, engine.device, engine)
        t = rng.standard_normal((rows, 2 * S + A + 3)).astype(np.float32)
        t[:, S:S + A] = np.tanh(t[:, S:S + A])
        r.append_rows(torch.from_numpy(t))
        bufs.append(r)
    return serl_amd.NetSpec(S, A, H, L, ACT), w, bufs


class Timed:
    """wraps the library so that the launch distil_batch makes is bracketed by device events on the launch's stream"""

    def __init__(self, lib):
        self.lib, self.events = lib, []

    def __getattr__(self, name):
        f = getattr(self.lib, name)
        if name not in ('serl_ga_distill', 'serl_ga_distill_general'):
            return f

        def g(*a):
            if a[3] == 0:                  # (the probe)
                return f(*a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = f(*a)
            e1.record()
            self.events.append((e0, e1))
            return rc
        return g


def run_batch(engine, args, spec, w, pairs, bufs, critic, kernel, dense):
    """-> (children, wall ms, kernel ms, info) of one synchronised distil_batch from fixed seeds"""
    from serl_amd import distill, _capi
    info = {}
    random.seed(7); torch.manual_seed(7)
    real = _capi.lib()
    timed = _capi._lib = Timed(real)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kids = distill.distil_batch(args, engine, spec, w, pairs, bufs, critic, kernel=kernel, dense=dense, info=info)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        _capi._lib = real
    assert len(timed.events) == 1, len(timed.events)
    return kids, wall, timed.events[0][0].elapsed_time(timed.events[0][1]), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hidden', default='32,72,96')
    ap.add_argument('--pairs', type=int, default=15)
    ap.add_argument('--rows', type=int, default=3000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--torch-pairs', type=int, default=2)
    ap.add_argument('--kernel-regs', default=None, help='output of tools/kernel_regs.sh for the record')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'distill_general_timing.json'))
    o = ap.parse_args()
    import serl_amd
    from serl_amd import build, distill, _capi
    engine = serl_amd.RolloutEngine(0)
    res = {'tool': 'tools/bench_distill.py', 'argv': sys.argv[1:], 'source_hash': build.source_hash(), 'device': torch.cuda.get_device_name(0),
           'pairs': o.pairs, 'rows': o.rows, 'steps_per_pair': 12 * (o.rows // 128), 'S': S, 'A': A, 'layers': L, 'activation': ACT,
           'kernel_regs': open(o.kernel_regs).read().splitlines() if o.kernel_regs else None, 'shapes': []}
    torch.manual_seed(0)
    critic = TwinQ().to(engine.device)
    args = types.SimpleNamespace(individual_bs=o.rows)
    pairs = [(i, i + 1) for i in range(o.pairs)]
    for H in (int(h) for h in o.hidden.split(',')):
        spec, w, bufs = population(engine, H, o.pairs + 1, o.rows, seed=H)
        P = spec.param_count
        row = {'hidden': H, 'params': P, 'paths': {}}
        paths = ([('fused', 'serl50', 'valu')] if H == 32 else []) + [('fused-general', 'general', 'valu'), ('fused-general-mfma', 'general', 'mfma')]
        # PyTorch pair by pair: a one-pair warm-up, then --torch-pairs pairs, timed once
        random.seed(7); torch.manual_seed(7)
        distill.distilation_crossover(args, engine, spec, w, 0, 1, bufs, critic)
        random.seed(7); torch.manual_seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = [distill.distilation_crossover(args, engine, spec, w, f, s, bufs, critic) for f, s in pairs[:o.torch_pairs]]
        torch.cuda.synchronize()
        tw = (time.perf_counter() - t0) * 1e3
        row['paths']['torch'] = {'pairs_timed': o.torch_pairs, 'wall_ms_per_pair': tw / o.torch_pairs, 'wall_ms_scaled_to_pairs': tw / o.torch_pairs * o.pairs}
        print('H %3d torch            %9.1f ms per pair -> %10.1f ms for %d pairs' % (H, tw / o.torch_pairs, tw / o.torch_pairs * o.pairs, o.pairs), flush=True)
        kids_of = {}
        for path, kernel, dense in paths:             # warm-up of each path
            kids, _, _, info = run_batch(engine, args, spec, w, pairs, bufs, critic, kernel, dense)
            assert info['path'] == path, info
            kids_of[path] = torch.stack([k[0] for k in kids])
            moved = max(float((k[0] - w[s, :P]).abs().max()) for k, (_, s) in zip(kids, pairs))
            dev = max(float((k[0] - r[0]).abs().max()) for k, r in zip(kids, ref))
            row['paths'][path] = {'max_abs_dev_from_torch': dev, 'max_moved': moved}
            assert dev < 0.05 * moved, (path, dev, moved)
        assert torch.equal(kids_of['fused-general'], kids_of['fused-general-mfma']), 'the two dense flavours differ'
        walls, kms = {p: [] for p, _, _ in paths}, {p: [] for p, _, _ in paths}
        for _ in range(o.reps):                       # alternating
            for path, kernel, dense in paths:
                _, wall, km, _ = run_batch(engine, args, spec, w, pairs, bufs, critic, kernel, dense)
                walls[path].append(wall); kms[path].append(km)
        for path, _, _ in paths:
            row['paths'][path].update(kernel_ms=stats(kms[path]), wall_ms=stats(walls[path]))
            print('H %3d %-18s kernel %8.2f ms [%.2f .. %.2f]   distil_batch wall %8.1f ms [%.1f .. %.1f]' % (
                H, path, statistics.median(kms[path]), min(kms[path]), max(kms[path]), statistics.median(walls[path]), min(walls[path]),
                max(walls[path])), flush=True)
        res['shapes'].append(row)
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
        with open(o.out, 'w') as f:
            json.dump(res, f, indent=1)
    print('wrote', o.out)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The parent distances of one epoch's distillation crossover: ga.sort_groups_by_distance on serl_ga_novelty (kernel='lds': a torch
gather per evaluation, one launch per batch size, one sample at a time in the kernel) and on serl_ga_novelty_general (the plan's tables
in one upload, one launch that reads the rings, batch-parallel) with its dense phase on the VALU and on the f32 matrix cores, on the same
GPU, the same parents, the same rings and the same draws.

Per shape (hidden 32 / 72 / 96 / 128, 3 hidden layers, S 7, A 3, tanh): --parents actors (10: 45 pairs, 90 evaluations of 256 rows) with
rings of --rows transitions.  Two figures per flavour:
  kernel ms   device events around the launches sort_groups_by_distance makes (summed when there are several)
  wall ms     sort_groups_by_distance end to end, synchronised: the draws, the gathers or the upload, the launch, the read-back, the sort
both from the same --reps runs after a warm-up run of each flavour, the flavours alternating; median [min .. max].  The general kernel's
distances are checked against the 'lds' flavour's (to 1e-5 relative, the figure recorded) and its two flavours for equal values.

Then the share of one SSNE.epoch the distance sort takes at hidden 72 x 3: the reference's default configuration (proximal mutation,
distillation crossover by distance) on a population of --pop actors, distillation and sensitivity on their general kernels, the epoch
timed end to end and the time inside ga.sort_groups_by_distance (synchronised on both sides) beside it, per flavour (--reps epochs each,
alternating).  Results, with the source hash, go to profiles/ga_novelty_timing.json.

  python tools/bench_novelty.py
  python tools/bench_novelty.py --hidden 72 --parents 10 --reps 7
"""
import argparse, json, os, random, statistics, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ.setdefault('OMP_NUM_THREADS', '16')
import numpy as np
import torch

S, A, L, ACT = 7, 3, 3, 'tanh'
FLAVOURS = [('lds', 'lds', 'valu'), ('general-valu', 'general', 'valu'), ('general-mfma', 'general', 'mfma')]
ENTRIES = ('serl_ga_novelty', 'serl_ga_novelty_general')


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': len(v)} if v else None


class Timed:
    """wraps the library so that every launch of ENTRIES is bracketed by device events on the launch's stream"""

    def __init__(self, lib):
        self.lib, self.events = lib, {e: [] for e in ENTRIES}

    def __getattr__(self, name):
        f = getattr(self.lib, name)
        if name not in ENTRIES:
            return f

        def g(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = f(*a)
            e1.record()
            if rc == 0:
                self.events[name].append((e0, e1))
            return rc
        return g

    def ms(self):
        return [a.elapsed_time(b) for e in ENTRIES for a, b in self.events[e]]


def weights_of(H, n, seed):
    import actor_shapes as X
    import serl_amd
    s = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=ACT, env_config=0, incremental=False)
    return serl_amd.NetSpec(S, A, H, L, ACT), X.make_weights(s, n, seed)


def rings_of(engine, rows):
    from serl_amd import replay
    out = []
    for t in rows:
        r = replay.DeviceReplay(10_000, engine.device, engine)
        r.append_rows(t)
        out.append(r)
    return out


def transitions(rng, n, rows):
    out = []
    for _ in range(n):
        t = rng.standard_normal((rows, 2 * S + A + 3)).astype(np.float32)
        t[:, S:S + A] = np.tanh(t[:, S:S + A])
        out.append(torch.from_numpy(t))
    return out


def run_sort(engine, w, parents, bufs, spec, kernel, dense, seed=7):
    """-> (groups, wall ms, kernel ms summed, launches) of one synchronised ga.sort_groups_by_distance"""
    from serl_amd import ga
    real = engine.lib
    timed = engine.lib = Timed(real)
    random.seed(seed)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        groups = ga.sort_groups_by_distance(engine, w, parents, bufs, spec, kernel=kernel, dense=dense)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        engine.lib = real
    km = timed.ms()
    return groups, wall, sum(km), len(km)


def run_epoch(engine, spec, w0, rows, fit, critic, o, kernel, dense):
    """-> (epoch wall ms, ms inside ga.sort_groups_by_distance, novelty kernel ms, launches)"""
    from serl_amd import ga, ssne, replay
    n = len(w0)
    bufs = rings_of(engine, rows)
    crits = [replay.DeviceReplay(10_000, engine.device, engine) for _ in range(n)]
    w = torch.from_numpy(w0.copy()).to(engine.device)
    args = types.SimpleNamespace(pop_size=n, elite_fraction=0.2, mutation_prob=0.9, mutation_mag=0.05, mut_type='proximal', distil_crossover=True,
                                 distil_type='distance', crossover_prob=0.0, mutation_batch_size=86, individual_bs=o.rows)
    inside = []
    real_sort, real_lib = ga.sort_groups_by_distance, engine.lib

    def timed_sort(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real_sort(*a, **k)
        torch.cuda.synchronize()
        inside.append((time.perf_counter() - t0) * 1e3)
        return out
    random.seed(11); np.random.seed(11); torch.manual_seed(11)
    ep = ssne.SSNE(args, engine, spec, critic=critic, distil_kernel='general', sensitivity_kernel='general', novelty_kernel=kernel,
                   novelty_dense=dense)
    ga.sort_groups_by_distance = timed_sort
    timed = engine.lib = Timed(real_lib)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep.epoch(w, fit, buffers=bufs, critical=crits)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        ga.sort_groups_by_distance, engine.lib = real_sort, real_lib
    assert torch.isfinite(w).all() and len(inside) == 1
    return wall, inside[0], sum(timed.ms()), len(timed.ms())


class TwinQ(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.q1 = torch.nn.Sequential(torch.nn.Linear(S + A, 64), torch.nn.ELU(), torch.nn.Linear(64, 1))
        self.q2 = torch.nn.Sequential(torch.nn.Linear(S + A, 64), torch.nn.ELU(), torch.nn.Linear(64, 1))

    def forward(self, s, a):
        x = torch.cat([s, a], -1)
        return self.q1(x), self.q2(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hidden', default='32,72,96,128')
    ap.add_argument('--parents', type=int, default=10)
    ap.add_argument('--rows', type=int, default=3000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--epoch-hidden', type=int, default=72, help='0: no epoch')
    ap.add_argument('--pop', type=int, default=20)
    ap.add_argument('--kernel-regs', default=None, help='output of tools/kernel_regs.sh for the record')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ga_novelty_timing.json'))
    o = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    import serl_amd
    from serl_amd import build
    engine = serl_amd.RolloutEngine(0)
    res = {'tool': 'tools/bench_novelty.py', 'argv': sys.argv[1:], 'csrc_sha256': build.source_hash(), 'device': torch.cuda.get_device_name(0),
           'parents': o.parents, 'pairs': o.parents * (o.parents - 1) // 2, 'evaluations': o.parents * (o.parents - 1), 'rows': o.rows, 'S': S, 'A': A,
           'layers': L, 'activation': ACT, 'reps': o.reps, 'kernel_regs': open(o.kernel_regs).read().splitlines() if o.kernel_regs else None,
           'shapes': [], 'epoch': None}

    def save():
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
        with open(o.out, 'w') as f:
            json.dump(res, f, indent=1)
    for H in (int(h) for h in o.hidden.split(',')):
        spec, w0 = weights_of(H, o.parents, seed=H)
        w = torch.from_numpy(w0).to(engine.device)
        parents = list(range(o.parents))
        bufs = rings_of(engine, transitions(np.random.default_rng(H), o.parents, o.rows))
        row = {'hidden': H, 'flavours': {}}
        got = {}
        for name, kernel, dense in FLAVOURS:            # warm-up of each flavour
            got[name], _, _, launches = run_sort(engine, w, parents, bufs, spec, kernel, dense)
            row['flavours'][name] = {'launches': launches}
        assert got['general-valu'] == got['general-mfma'], 'the two dense flavours differ'
        row['same_order_as_lds'] = [g[:2] for g in got['lds']] == [g[:2] for g in got['general-valu']]
        by_pair = {g[:2]: g[2] for g in got['general-valu']}
        dev = max(abs(g[2] - by_pair[g[:2]]) / g[2] for g in got['lds'])
        row['max_rel_dev_general_from_lds'] = dev
        assert dev < 1e-5, dev
        walls, kms = {n: [] for n, _, _ in FLAVOURS}, {n: [] for n, _, _ in FLAVOURS}
        for _ in range(o.reps):                         # alternating
            for name, kernel, dense in FLAVOURS:
                _, wall, km, _ = run_sort(engine, w, parents, bufs, spec, kernel, dense)
                walls[name].append(wall)
                kms[name].append(km)
        for name, _, _ in FLAVOURS:
            row['flavours'][name].update(kernel_ms=stats(kms[name]), wall_ms=stats(walls[name]))
            print('H %3d %-13s %d launch(es), kernel %8.3f ms [%.3f .. %.3f]   sort_groups_by_distance wall %8.2f ms [%.2f .. %.2f]' % (
                H, name, row['flavours'][name]['launches'], statistics.median(kms[name]), min(kms[name]), max(kms[name]),
                statistics.median(walls[name]), min(walls[name]), max(walls[name])), flush=True)
        res['shapes'].append(row)
        save()
    if o.epoch_hidden:
        H = o.epoch_hidden
        spec, w0 = weights_of(H, o.pop, seed=H + 1)
        rng = np.random.default_rng(5)
        rows = transitions(rng, o.pop, o.rows)
        fit = rng.normal(-150, 50, o.pop)
        torch.manual_seed(0)
        critic = TwinQ().to(engine.device)
        ep = {'hidden': H, 'pop': o.pop, 'rows': o.rows, 'runs': {},
              'config': 'mut_type proximal, distil_crossover, distil_type distance, mutation_prob 0.9, distil_kernel general, sensitivity_kernel general'}
        for name, kernel, dense in FLAVOURS:            # warm-up
            run_epoch(engine, spec, w0, rows, fit, critic, o, kernel, dense)
        acc = {n: [] for n, _, _ in FLAVOURS}
        for _ in range(o.reps):
            for name, kernel, dense in FLAVOURS:
                acc[name].append(run_epoch(engine, spec, w0, rows, fit, critic, o, kernel, dense))
        for name, runs in acc.items():
            wall, inside = [r[0] for r in runs], [r[1] for r in runs]
            share = [i / w_ for i, w_ in zip(inside, wall)]
            ep['runs'][name] = {'launches': runs[0][3], 'epoch_wall_ms': stats(wall), 'distance_sort_wall_ms': stats(inside),
                                'distance_sort_share_of_epoch': stats(share), 'novelty_kernel_ms': stats([r[2] for r in runs])}
            print('epoch H %d novelty %-13s epoch %9.1f ms, in sort_groups_by_distance %7.2f ms = %5.2f %%, novelty kernels %.3f ms (%d launch(es))' % (
                H, name, statistics.median(wall), statistics.median(inside), 100 * statistics.median(share),
                statistics.median([r[2] for r in runs]), runs[0][3]), flush=True)
        res['epoch'] = ep
        save()
    print('wrote', o.out)


if __name__ == '__main__':
    main()

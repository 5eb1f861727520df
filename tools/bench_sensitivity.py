#!/usr/bin/env python
"""The sensitivities of one epoch's proximal mutations: serl_ga_sensitivity (kernel='lds'; at hidden 128 x 3 its PyTorch fallback) and
serl_ga_sensitivity_general with its dense phases on the VALU and on the f32 matrix cores, on the same GPU, the same members and the same
minibatches.

Per shape (hidden 32 / 72 / 96 / 128, 3 hidden layers, S 7, A 3, tanh): --members actors, one minibatch of --batch states each (the
reference's mutation_batch_size: 86), all in ONE ga.sensitivity call as ProximalBatch.apply makes it.  Two figures per flavour:
  kernel ms   device events around the one launch ga.sensitivity makes (none for the PyTorch fallback)
  wall ms     ga.sensitivity end to end, synchronised: uploads, the launch (or the fallback's autograd passes), the result on the device
both from the same --reps runs after a warm-up run of each flavour, the flavours alternating; median [min .. max].  The general kernel's
result is checked against the 'lds' flavour's (to 5e-3 relative, but where one of them is clamped) and its two flavours for equal bits.

Then the share of one SSNE.epoch the sensitivity calls take at hidden 72 x 3: the reference's default configuration (proximal mutation,
distillation crossover by distance) on a population of --pop actors with rings of --rows transitions, the epoch timed end to end and the
time inside ga.sensitivity (synchronised on both sides) beside it, per sensitivity flavour, with the distillation on
serl_ga_distill_general (--reps epochs each, alternating) and once on the default distil_kernel='serl50', which trains such actors pair
by pair in PyTorch.  serl_ga_novelty's launches of the same epochs are timed the same way for the record.
Results, with the source hash, go to profiles/ga_sensitivity_timing.json.

  python tools/bench_sensitivity.py
  python tools/bench_sensitivity.py --hidden 72 --members 15 --batch 86 --reps 7
"""
import argparse, json, os, random, statistics, sys, time, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

S, A, L, ACT = 7, 3, 3, 'tanh'
FLAVOURS = [('lds', 'lds', 'valu'), ('general-valu', 'general', 'valu'), ('general-mfma', 'general', 'mfma')]
ENTRIES = ('serl_ga_sensitivity', 'serl_ga_sensitivity_general', 'serl_ga_novelty')


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

    def ms(self, name):
        return [a.elapsed_time(b) for a, b in self.events[name]]


def weights_of(H, n, seed):
    import actor_shapes as X
    import serl_amd
    s = dict(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=ACT, env_config=0, incremental=False)
    return serl_amd.NetSpec(S, A, H, L, ACT), X.make_weights(s, n, seed)


def run_sens(engine, w, members, spec, st, kernel, dense):
    """-> (scaling, wall ms, kernel ms or None) of one synchronised ga.sensitivity"""
    from serl_amd import ga
    real = engine.lib
    timed = engine.lib = Timed(real)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc = ga.sensitivity(engine, w, members, spec, st, kernel=kernel, dense=dense)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        engine.lib = real
    km = timed.ms('serl_ga_sensitivity') + timed.ms('serl_ga_sensitivity_general')
    assert len(km) <= 1
    return sc, wall, (km[0] if km else None)


def run_epoch(engine, spec, w0, rows, fit, critic, o, kernel, dense, distil_kernel):
    """-> (epoch wall ms, ms inside ga.sensitivity, sensitivity calls, members mutated, novelty kernel ms, distillation path)"""
    from serl_amd import ga, ssne, replay
    n = len(w0)
    bufs, crits = [], []
    for k in range(n):
        r = replay.DeviceReplay(10_000, engine.device, engine)
        r.append_rows(rows[k])
        bufs.append(r)
        crits.append(replay.DeviceReplay(10_000, engine.device, engine))
    w = torch.from_numpy(w0.copy()).to(engine.device)
    args = types.SimpleNamespace(pop_size=n, elite_fraction=0.2, mutation_prob=0.9, mutation_mag=0.05, mut_type='proximal', distil_crossover=True,
                                 distil_type='distance', crossover_prob=0.0, mutation_batch_size=o.batch, individual_bs=o.rows)
    rec, inside = [], []
    real_sens, real_lib = ga.sensitivity, engine.lib

    def timed_sens(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = real_sens(*a, **k)
        torch.cuda.synchronize()
        inside.append((time.perf_counter() - t0) * 1e3)
        return out
    random.seed(11); np.random.seed(11); torch.manual_seed(11)
    ep = ssne.SSNE(args, engine, spec, critic=critic, record=rec, distil_kernel=distil_kernel, sensitivity_kernel=kernel, sensitivity_dense=dense)
    ga.sensitivity = timed_sens
    timed = engine.lib = Timed(real_lib)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ep.epoch(w, fit, buffers=bufs, critical=crits)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
    finally:
        ga.sensitivity, engine.lib = real_sens, real_lib
    assert torch.isfinite(w).all()
    return wall, sum(inside), len(inside), sum(r[0] == 2 for r in rec), sum(timed.ms('serl_ga_novelty')), ep.last_distil_path


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
    ap.add_argument('--members', type=int, default=15)
    ap.add_argument('--batch', type=int, default=86)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--epoch-hidden', type=int, default=72, help='0: no epoch')
    ap.add_argument('--pop', type=int, default=20)
    ap.add_argument('--rows', type=int, default=3000)
    ap.add_argument('--kernel-regs', default=None, help='output of tools/kernel_regs.sh for the record')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ga_sensitivity_timing.json'))
    o = ap.parse_args()
    import serl_amd
    from serl_amd import build
    engine = serl_amd.RolloutEngine(0)
    res = {'tool': 'tools/bench_sensitivity.py', 'argv': sys.argv[1:], 'source_hash': build.source_hash(), 'device': torch.cuda.get_device_name(0),
           'members': o.members, 'batch': o.batch, 'S': S, 'A': A, 'layers': L, 'activation': ACT, 'reps': o.reps,
           'kernel_regs': open(o.kernel_regs).read().splitlines() if o.kernel_regs else None, 'shapes': [], 'epoch': None}

    def save():
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
        with open(o.out, 'w') as f:
            json.dump(res, f, indent=1)
    for H in (int(h) for h in o.hidden.split(',')):
        spec, w0 = weights_of(H, o.members, seed=H)
        w = torch.from_numpy(w0).to(engine.device)
        members = list(range(o.members))
        rng = np.random.default_rng(H)
        st = torch.from_numpy((rng.standard_normal((o.members, o.batch, S)) * rng.uniform(0.2, 2.0, S)).astype(np.float32)).to(engine.device)
        row = {'hidden': H, 'genome': sum(n for _, n in spec.genome_segments()), 'flavours': {}}
        got = {}
        for name, kernel, dense in FLAVOURS:            # warm-up of each flavour
            got[name], _, km = run_sens(engine, w, members, spec, st, kernel, dense)
            row['flavours'][name] = {'path': 'kernel' if km is not None else 'torch fallback (serl_ga_sensitivity refuses the shape for LDS)'}
        assert torch.equal(got['general-valu'], got['general-mfma']), 'the two dense flavours differ'
        a, b = got['lds'].double(), got['general-valu'].double()
        free = (a != 0.01) & (b != 0.01) & (a != 1.0) & (b != 1.0)
        dev = float(((a - b).abs() / torch.maximum(a, b))[free].max())
        row['max_rel_dev_general_from_lds'] = dev
        assert dev < 5e-3, dev
        walls, kms = {n: [] for n, _, _ in FLAVOURS}, {n: [] for n, _, _ in FLAVOURS}
        for _ in range(o.reps):                         # alternating
            for name, kernel, dense in FLAVOURS:
                _, wall, km = run_sens(engine, w, members, spec, st, kernel, dense)
                walls[name].append(wall)
                if km is not None:
                    kms[name].append(km)
        for name, _, _ in FLAVOURS:
            row['flavours'][name].update(kernel_ms=stats(kms[name]), wall_ms=stats(walls[name]))
            print('H %3d %-13s kernel %s   ga.sensitivity wall %8.2f ms [%.2f .. %.2f]' % (
                H, name, ('%8.3f ms [%.3f .. %.3f]' % (statistics.median(kms[name]), min(kms[name]), max(kms[name]))) if kms[name] else '   (PyTorch fallback)',
                statistics.median(walls[name]), min(walls[name]), max(walls[name])), flush=True)
        res['shapes'].append(row)
        save()
    if o.epoch_hidden:
        H = o.epoch_hidden
        spec, w0 = weights_of(H, o.pop, seed=H + 1)
        rng = np.random.default_rng(5)
        rows = []
        for _ in range(o.pop):
            t = rng.standard_normal((o.rows, 2 * S + A + 3)).astype(np.float32)
            t[:, S:S + A] = np.tanh(t[:, S:S + A])
            rows.append(torch.from_numpy(t))
        fit = rng.normal(-150, 50, o.pop)
        torch.manual_seed(0)
        critic = TwinQ().to(engine.device)
        ep = {'hidden': H, 'pop': o.pop, 'rows': o.rows, 'config': 'mut_type proximal, distil_crossover, distil_type distance, mutation_prob 0.9', 'runs': {}}
        for distil_kernel, reps in (('general', o.reps), ('serl50', 1)):
            for name, kernel, dense in FLAVOURS:        # warm-up
                run_epoch(engine, spec, w0, rows, fit, critic, o, kernel, dense, 'general')
            acc = {n: [] for n, _, _ in FLAVOURS}
            for _ in range(reps):
                for name, kernel, dense in (FLAVOURS if distil_kernel == 'general' else FLAVOURS[:1]):
                    acc[name].append(run_epoch(engine, spec, w0, rows, fit, critic, o, kernel, dense, distil_kernel))
            for name, runs in acc.items():
                if not runs:
                    continue
                wall, inside = [r[0] for r in runs], [r[1] for r in runs]
                share = [i / w_ for i, w_ in zip(inside, wall)]
                ep['runs']['distil_%s/%s' % (distil_kernel, name)] = {
                    'distil_path': runs[0][5], 'sensitivity_calls': runs[0][2], 'members_mutated': int(runs[0][3]), 'epoch_wall_ms': stats(wall),
                    'sensitivity_wall_ms': stats(inside), 'sensitivity_share_of_epoch': stats(share), 'novelty_kernel_ms': stats([r[4] for r in runs])}
                print('epoch H %d distil %-7s (%s) sens %-13s epoch %9.1f ms, in ga.sensitivity %7.2f ms (%d call(s), %d members) = %5.2f %%, novelty kernels %.2f ms' % (
                    H, distil_kernel, runs[0][5], name, statistics.median(wall), statistics.median(inside), runs[0][2], runs[0][3],
                    100 * statistics.median(share), statistics.median([r[4] for r in runs])), flush=True)
        res['epoch'] = ep
        save()
    print('wrote', o.out)


if __name__ == '__main__':
    main()

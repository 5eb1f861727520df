#!/usr/bin/env python3
"""What lane_weights='regrouped' (C ABI serl_rollout_regrouped: kernel='laneg' over a copy of the population regrouped to [P / 4][members][4]) buys the
lane population kernel of every actor shape, against the rows and against what else runs.  tools/bench_laneg.py's protocol and populations.

    python tools/bench_lanegt.py [--shapes 72x3,96x3,32x3] [--episodes 4096,16384,65536] [--populations pop50,own] [--t-max 20] [--reps 5]
                                 [--out profiles/rollout_lanegt_timing.json]

Nominal build, base reference shared by all episodes, t_max seconds (2 001 env steps at 20 s).  `pop50` = 50 members x episodes / 50 evaluations in
evaluate_pop's order, `own` = every episode a member of its own.  Flavours, alternating within every repetition and rotated from one repetition to the
next, after one small warm-up launch each:
    lanegt64   kernel='laneg', lane_weights='regrouped'   the regrouped copy, 64 lanes per wavefront
    laneg64    kernel='laneg'                             the rows
    lane64     lanes_per_wave=64                          the lane kernel without the hint (at 32 x 3: the regrouped hidden-32 lane kernel)
    wave       kernel='wave'                              one wavefront per episode
Kernel times are HIP events around the launch (serl_last_rollout_ms: the regroup kernel runs in front of the first event); `call_ms` are events
around the whole rollout() call, and regroup_ms = median(call_ms - kernel_ms) of lanegt64 minus the same of laneg64 -- the regroup kernel's own time per
launch, allocation of the slot excluded (the warm-up launch of the full member count grows it).  env-steps/s = sum of |length_steps| over the median
kernel time.  The results of all flavours are compared with torch.equal in the same run.  The JSON document (with the source hash) is rewritten after
every point; points already in --out are kept and not measured again."""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import serl_amd
from serl_amd import refsignals, build as hip_build

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='72x3,96x3,32x3')
ap.add_argument('--episodes', default='4096,16384,65536')
ap.add_argument('--populations', default='pop50,own')
ap.add_argument('--t-max', type=float, default=20.0)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_lanegt_timing.json'))
a = ap.parse_args()
eng = serl_amd.RolloutEngine(0)
KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps')
FLAVOURS = (('lanegt64', dict(kernel='laneg', lanes_per_wave=64, lane_weights='regrouped')), ('laneg64', dict(kernel='laneg', lanes_per_wave=64)),
            ('lane64', dict(lanes_per_wave=64)), ('wave', dict(kernel='wave')))


def members(spec, n, seed=7):
    """f32 [n, row_stride] on the device: 50 seeded actors, tiled, N(0, 0.01^2) on the 2-D weights of every member beyond them (tools/bench_laneg.py's)"""
    from serl_amd.actor import Actor, pack_actor, pad_rows
    args = types.SimpleNamespace(state_dim=7, action_dim=3, hidden_size=spec.hidden, num_layers=spec.num_layers, activation_actor='tanh', device='cpu')
    rows = []
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        for _ in range(50):
            m = Actor(args)
            with torch.no_grad():
                m.net[-2].weight.mul_(0.1); m.net[-2].bias.mul_(0.1)
            rows.append(pack_actor(m))
    base = pad_rows(torch.stack(rows)).to(eng.device)
    w = base[torch.arange(n, device=eng.device) % 50].contiguous()
    if n > 50:
        g = torch.Generator(device=eng.device).manual_seed(seed)
        for off, cnt in spec.genome_segments():
            w[50:, off:off + cnt] += 0.01 * torch.randn(n - 50, cnt, generator=g, device=eng.device)
    return w


def point(spec, E, population, ref):
    n = 50 if population == 'pop50' else E
    w = members(spec, n)
    moe = (np.arange(E) // max(E // n, 1) % n).astype(np.int32)
    for _, kw in FLAVOURS:      # warm-up: every flavour's code object loaded (and the slot of the copy grown to n members), not recorded
        eng.rollout(w, spec, moe[:256], ref, t_max=a.t_max, **kw)
    ms, call, outs, infos, copy = {name: [] for name, _ in FLAVOURS}, {name: [] for name, _ in FLAVOURS}, {}, {}, None
    for i in range(a.reps):
        for j in range(len(FLAVOURS)):
            name, kw = FLAVOURS[(j + i) % len(FLAVOURS)]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = eng.rollout(w, spec, moe, ref, t_max=a.t_max, **kw)
            e1.record()
            e1.synchronize()
            ms[name].append(eng.last_kernel_ms)
            call[name].append(e0.elapsed_time(e1))
            if name == 'lanegt64':
                copy = eng.last_rollout_weights()
                assert copy['regrouped'] == 1
            if name not in outs:
                outs[name], infos[name] = {k: out[k] for k in KEYS}, eng.last_rollout_info()
            else:
                assert all(torch.equal(out[k], outs[name][k]) for k in KEYS), name + ': a repetition changed the results'
    first = FLAVOURS[0][0]
    ls = outs[first]['length_steps']
    steps = int(ls.abs().sum())
    equal = bool(all(torch.equal(outs[nm][k], outs[first][k]) for nm, _ in FLAVOURS for k in KEYS))
    around = {nm: float(np.median(np.array(call[nm]) - np.array(ms[nm]))) for nm in ('lanegt64', 'laneg64')}
    case = dict(shape='%dx%d' % (spec.hidden, spec.num_layers), params_per_member=spec.param_count, episodes=E, population=population, members=n,
                weight_bytes=int(w.numel() * 4), copy=copy, regroup_ms=round(around['lanegt64'] - around['laneg64'], 3), env_steps=steps,
                full_flights=int((ls == ref.shape[0]).sum()), results_equal=equal, kernels={})
    for name, _ in FLAVOURS:
        v = sorted(ms[name])
        med = float(np.median(v))
        case['kernels'][name] = dict(family=infos[name]['family'], workgroups=infos[name]['workgroups'], per_wave_or_team=infos[name]['episodes_per_team'],
                                     kernel_ms=[round(x, 2) for x in ms[name]], call_ms=[round(x, 2) for x in call[name]], median_ms=round(med, 2),
                                     min_ms=round(v[0], 2), max_ms=round(v[-1], 2), env_steps_per_s=steps / (med * 1e-3))
    print(json.dumps(case), flush=True)
    assert equal, 'the flavours disagree'
    return case


ref = refsignals.tabulate(*refsignals.base_reference(a.t_max), a.t_max)
doc = json.load(open(a.out)) if os.path.exists(a.out) else None
if not doc or doc.get('source_hash') != hip_build.source_hash():
    doc = dict(what="kernel='laneg' with lane_weights='regrouped' (lanegt64) against kernel='laneg' on the rows (laneg64), lanes_per_wave=64 without the hint "
                    "(lane64; at 32x3 the regrouped hidden-32 lane kernel) and kernel='wave'; nominal build, base reference, t_max %g s; pop50 = 50 members in "
                    "evaluate_pop's order, own = every episode a member of its own; regroup_ms = the regroup kernel's own time per launch" % a.t_max,
               source_hash=hip_build.source_hash(), device=torch.cuda.get_device_name(0), cus=eng.num_cus, t_max=a.t_max, steps_per_full_episode=int(ref.shape[0]),
               reps=a.reps, order='the flavours alternate within a repetition, rotated from one repetition to the next; one warm-up launch of 256 episodes each',
               cases=[])


def save():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


done = {(c['shape'], c['episodes'], c['population']) for c in doc['cases']}
for sh in [x for x in a.shapes.split(',') if x]:
    for E in [int(x) for x in a.episodes.split(',') if x]:
        for p in a.populations.split(','):
            if (sh, E, p) in done:
                continue
            H, L = (int(x) for x in sh.split('x'))
            doc['cases'].append(point(serl_amd.NetSpec(7, 3, H, L, 'tanh'), E, p, ref))
            save()

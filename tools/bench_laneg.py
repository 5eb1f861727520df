#!/usr/bin/env python3
"""What kernel='laneg' (kernel_hint SERL_KERNEL_LANEG: one episode per lane, every lane its own actor of any shape over its member's row) buys
large populations of the shapes that are not hidden 32, against what runs today.

    python tools/bench_laneg.py [--shapes 72x3,96x3] [--episodes 4096,16384,65536] [--t-max 20] [--reps 5] [--ceiling] [--out profiles/rollout_laneg_timing.json]

Nominal build, base reference shared by all episodes, t_max seconds (2 001 env steps at 20 s).  Per shape and episode count two populations: `pop50`
= 50 members x episodes / 50 evaluations in evaluate_pop's order (member = episode // evals: the weights stay cache-resident), and `own` = every
episode a member of its own (episodes x P x 4 bytes of weights streamed per env step).  Members: 50 seeded actors of torch's default init (output
layer x 0.1: benign flights), tiled with N(0, 0.01^2) noise on every member beyond them.  Flavours, alternating within every repetition and rotated from
one repetition to the next, after one small warm-up launch each (256 episodes: the code objects are loaded):
    auto     kernel=None               what runs today
    wave     kernel='wave'             one wavefront per episode
    lane64   lanes_per_wave=64         the lane kernel without the hint: up to 64 wavefront-wide forward passes per env step
    laneg64 / laneg32 / laneg16        kernel='laneg' at 64 / 32 / 16 lanes per wavefront
--ceiling adds hidden 32 x 3 once (65 536 episodes, pop50): the hint against the regrouped lane kernel (lanes_per_wave=64).
Kernel times are HIP events around the launch (serl_last_rollout_ms); median, minimum and maximum of the repetitions, env-steps/s = sum of
|length_steps| over the median.  The results of all flavours are compared with torch.equal in the same run.  The JSON document (with the source hash)
is rewritten after every point, so an interrupted run keeps what it measured; points already in --out are kept and not measured again."""
import argparse, json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import serl_amd
from serl_amd import refsignals, build as hip_build

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', default='72x3,96x3')
ap.add_argument('--episodes', default='4096,16384,65536')
ap.add_argument('--populations', default='pop50,own')
ap.add_argument('--t-max', type=float, default=20.0)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--ceiling', action='store_true')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_laneg_timing.json'))
a = ap.parse_args()
eng = serl_amd.RolloutEngine(0)
KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps')
FLAVOURS = (('auto', dict()), ('wave', dict(kernel='wave')), ('lane64', dict(lanes_per_wave=64)), ('laneg64', dict(kernel='laneg', lanes_per_wave=64)),
            ('laneg32', dict(kernel='laneg', lanes_per_wave=32)), ('laneg16', dict(kernel='laneg', lanes_per_wave=16)))


def members(spec, n, seed=7):
    """f32 [n, row_stride] on the device: 50 seeded actors, tiled, N(0, 0.01^2) on the 2-D weights of every member beyond them"""
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


def point(spec, E, population, flavours, ref):
    n = 50 if population == 'pop50' else E
    w = members(spec, n)
    moe = (np.arange(E) // max(E // n, 1) % n).astype(np.int32)
    for _, kw in flavours:      # warm-up: every flavour's code object loaded, not recorded
        eng.rollout(w, spec, moe[:256], ref, t_max=a.t_max, **kw)
    ms, outs, infos = {name: [] for name, _ in flavours}, {}, {}
    for i in range(a.reps):
        for j in range(len(flavours)):
            name, kw = flavours[(j + i) % len(flavours)]
            out = eng.rollout(w, spec, moe, ref, t_max=a.t_max, **kw)
            ms[name].append(eng.last_kernel_ms)
            if name not in outs:
                outs[name], infos[name] = {k: out[k] for k in KEYS}, eng.last_rollout_info()
            else:
                assert all(torch.equal(out[k], outs[name][k]) for k in KEYS), name + ': a repetition changed the results'
    first = flavours[0][0]
    ls = outs[first]['length_steps']
    steps = int(ls.abs().sum())
    equal = bool(all(torch.equal(outs[nm][k], outs[first][k]) for nm, _ in flavours for k in KEYS))
    case = dict(shape='%dx%d' % (spec.hidden, spec.num_layers), params_per_member=spec.param_count, episodes=E, population=population, members=n,
                weight_bytes=int(w.numel() * 4), env_steps=steps, full_flights=int((ls == ref.shape[0]).sum()), results_equal=equal, kernels={})
    for name, _ in flavours:
        v = sorted(ms[name])
        med = float(np.median(v))
        case['kernels'][name] = dict(family=infos[name]['family'], workgroups=infos[name]['workgroups'], per_wave_or_team=infos[name]['episodes_per_team'],
                                     kernel_ms=[round(x, 2) for x in ms[name]], median_ms=round(med, 2), min_ms=round(v[0], 2), max_ms=round(v[-1], 2),
                                     env_steps_per_s=steps / (med * 1e-3))
    print(json.dumps(case), flush=True)
    assert equal, 'the flavours disagree'
    return case


ref = refsignals.tabulate(*refsignals.base_reference(a.t_max), a.t_max)
doc = json.load(open(a.out)) if os.path.exists(a.out) else None
if not doc or doc.get('source_hash') != hip_build.source_hash():
    doc = dict(what="kernel='laneg' (one episode per lane, every lane its own actor over its member's row) against kernel=None, kernel='wave' and "
                    "lanes_per_wave=64 without the hint; nominal build, base reference, t_max %g s; pop50 = 50 members in evaluate_pop's order, own = every "
                    "episode a member of its own" % a.t_max,
               source_hash=hip_build.source_hash(), device=torch.cuda.get_device_name(0), cus=eng.num_cus, t_max=a.t_max, steps_per_full_episode=int(ref.shape[0]),
               reps=a.reps, order='the flavours alternate within a repetition, rotated from one repetition to the next; one warm-up launch of 256 episodes each',
               cases=[])


def save():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


done = {(c['shape'], c['episodes'], c['population']) for c in doc['cases']}
todo = [(sh, E, p, FLAVOURS) for sh in a.shapes.split(',') if sh for E in [int(x) for x in a.episodes.split(',') if x] for p in a.populations.split(',')]
if a.ceiling:
    todo.append(('32x3', 65536, 'pop50', (FLAVOURS[2], FLAVOURS[3])))
for sh, E, p, flavours in todo:
    if (sh, E, p) in done:
        continue
    H, L = (int(x) for x in sh.split('x'))
    doc['cases'].append(point(serl_amd.NetSpec(7, 3, H, L, 'tanh'), E, p, flavours, ref))
    save()

#!/usr/bin/env python3
"""SURVEY 8d's SATURATING configuration: many more episodes than the GPU has lane groups, where throughput -- not the latency of one env step --
is the regime and the fp64 fraction means something.

    python tools/bench_saturate.py [--episodes 16384,65536] [--t-max 20] [--members 2048] [--modes lane64,auto] [--reps 2]

For every episode count and mode one JSON line: env-steps/s of the rollout kernel (HIP events around the launch), the kernel family the library
launched (serl_last_rollout_info), the fraction of the MEASURED fp64 peak (profiles/valu_latency_current.json) by SURVEY 8d's F_alg = 24 059 f64
operations per env step, and -- for the first 64 episodes -- whether the results equal the one-episode-per-team kernel's bit for bit.
Modes: laneN = the lane-per-episode DAG kernels with N episodes per wavefront (lanes_per_wave = N, rollout_variant.inc); auto = what serl_rollout
chooses (four episodes per team + work queue beyond 4 x CUs episodes); half = two episodes per wavefront.
Workload: the shipped SERL50 actors tiled with seeded noise to `members`, member = episode mod members, the base reference of
/root/reference/base/evaluate.py:173-180 shared by all episodes, nominal build, t_max seconds (2 001 env steps at 20 s).

    python tools/bench_saturate.py --mixed-lengths [--slots-x 1,2,4] [--reps 5] [--out profiles/lane_queue_timing.json]

The lane work queue (kernel_hint LANEQ) against today's lane family (lanes_per_wave = 64) and the queue launch of four-episode teams on episodes of UNEQUAL
length: the population of tools/bench_refill.py (512 members, half shipped SERL50 actors, half untrained ones that leave the envelope within seconds), at
1 x, 2 x and 4 x the resident lane slots (64 x 4 x CUs episodes), and one equal-length control (shipped actors only) at the largest size.  The three kernels
alternate within every repetition; median, minimum and maximum of the kernel times (HIP events) are reported, env-steps/s = sum of length_steps over the
median, and the three results are compared with torch.equal in the same run.  One JSON document, with the source hash, to --out.

    python tools/bench_saturate.py --sensor-noise table|device [--episodes 65536] [--sn-kernel auto|wave] [--reps 5] [--out-json FILE]

Mode 'noise' (the nominal build under the reference's sensor model, every episode noisy) on the same workload.  table: the host draws one
builds.sensor_noise_table per episode from np.random ([episodes][steps + 1][7] f64), copies it to the device, and serl_rollout reads it; reported:
host draw time, H2D time (once each) and the kernel times.  device: serl_rollout_noise draws inside the kernel; reported: the kernel times.  One JSON
line per episode count with median / min / max of the kernel times; --out-json appends the line to a JSON list in FILE."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench, serl_amd
from serl_amd import refsignals

ap = argparse.ArgumentParser()
ap.add_argument('--episodes', default='16384,65536')
ap.add_argument('--t-max', type=float, default=20.0)
ap.add_argument('--members', type=int, default=2048)
ap.add_argument('--modes', default='lane64,auto')
ap.add_argument('--reps', type=int, default=2)
ap.add_argument('--activation', default='tanh', help="tanh (the shipped SERL50 actors) | relu | elu: what the per-lane actor's 96 hidden activations cost (the weights stay the tanh actors': the flights differ)")
ap.add_argument('--order', choices=['interleaved', 'member-major'], default='interleaved',
                help='interleaved: member = episode mod members (64 different members per wavefront: the worst case for the per-lane actor); member-major: member = episode // (episodes / members), the order evaluate_pop produces (agent.py:234-256: all episodes of a member one after the other)')
ap.add_argument('--profile', action='store_true', help='with SERL_PROFILE=1 in the environment: cycles per env step wavefront 0 of workgroup 0 spent in the actor / dynamics / env bookkeeping (lane-per-episode kernels)')
ap.add_argument('--mixed-lengths', action='store_true', help='the lane work queue against the lane family and the team4 queue launch on episodes of unequal length (see above)')
ap.add_argument('--slots-x', default='1,2,4', help='--mixed-lengths: episode counts as multiples of the resident lane slots, 64 x 4 x CUs')
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lane_queue_timing.json'), help='--mixed-lengths: where the JSON document goes')
ap.add_argument('--sensor-noise', choices=['table', 'device'], default=None, help="mode 'noise': sensor noise from host-drawn tables or drawn inside the kernels (see above)")
ap.add_argument('--sn-kernel', choices=['auto', 'wave'], default='auto', help='--sensor-noise: the kernel family (auto: what the library chooses)')
ap.add_argument('--out-json', default=None, help='--sensor-noise: append the result lines to the JSON list in this file')
a = ap.parse_args()
eng = serl_amd.RolloutEngine(0)
spec = serl_amd.NetSpec(7, 3, 32, 3, a.activation)


def mixed_lengths():
    from serl_amd import build as hip_build
    KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps')
    MODES = (('laneq', dict(kernel='laneq')), ('lane64', dict(lanes_per_wave=64)), ('team4_queue', dict(kernel='team4')))
    rng = np.random.default_rng(11)      # (tools/bench_refill.py's population)
    shipped = np.load(os.path.join(ROOT, 'tests', 'golden', 'actors.npz'))['serl50']
    pop = 512
    good = shipped[rng.integers(0, 50, pop)].copy()
    bad = rng.random(pop) < 0.5
    r = rng.normal(0, 0.3, good.shape).astype(np.float32)
    for name, off, shape in spec.param_layout():
        if name.endswith('gamma'):
            r[:, off:off + shape[0]] = 1.0
    mixed = good.copy()
    mixed[bad] = r[bad]
    ref = refsignals.tabulate(*refsignals.base_reference(a.t_max), a.t_max)
    slots = 64 * 4 * eng.num_cus
    mult = [int(x) for x in a.slots_x.split(',')]
    cases = [('mixed', m, mixed) for m in mult] + [('equal', max(mult), good)]
    doc = dict(what='lane work queue (LANEQ) against the lane family (lanes_per_wave=64) and the team4 queue launch; nominal build, base reference, t_max %g s; '
                    'mixed = 512 members, half shipped SERL50 actors, half untrained; equal = shipped actors only' % a.t_max,
               source_hash=hip_build.source_hash(), device=torch.cuda.get_device_name(0), cus=eng.num_cus, resident_lane_slots=slots, t_max=a.t_max,
               steps_per_full_episode=int(ref.shape[0]), reps=a.reps, order='the three kernels alternate within a repetition, rotated from one repetition to the next; one warm-up launch each', cases=[])
    for label, m, wts in cases:
        E = m * slots
        moe = ((np.arange(E) % pop) if a.order == 'interleaved' else (np.arange(E) // (E // pop)) % pop).astype(np.int32)
        wd = torch.from_numpy(wts).to(eng.device)
        ms = {name: [] for name, _ in MODES}
        outs, infos = {}, {}
        for i in range(-1, a.reps):      # (-1: warm-up, not recorded)
            for j in range(len(MODES)):
                name, kw = MODES[(j + max(i, 0)) % len(MODES)]
                out = eng.rollout(wd, spec, moe, ref, t_max=a.t_max, **kw)
                if i >= 0:
                    ms[name].append(eng.last_kernel_ms)
                if name not in outs:
                    outs[name] = {k: out[k] for k in KEYS}
                    infos[name] = eng.last_rollout_info()
                else:
                    assert all(torch.equal(out[k], outs[name][k]) for k in KEYS), name + ': a repetition changed the results'
        ls = outs['laneq']['length_steps']
        steps = int(ls.abs().sum())
        equal = bool(all(torch.equal(outs[n][k], outs['laneq'][k]) for n, _ in MODES for k in KEYS))
        case = dict(case=label, slots_x=m, episodes=E, order=a.order, env_steps=steps, full_flights=int((ls == ref.shape[0]).sum()), median_length=int(ls.median()),
                    results_equal=equal, kernels={})
        for name, _ in MODES:
            v = sorted(ms[name])
            med = float(np.median(v))
            case['kernels'][name] = dict(family=infos[name]['family'], workgroups=infos[name]['workgroups'], per_wave_or_team=infos[name]['episodes_per_team'],
                                         work_queue=infos[name]['work_queue'], kernel_ms=[round(x, 2) for x in ms[name]], median_ms=round(med, 2), min_ms=round(v[0], 2),
                                         max_ms=round(v[-1], 2), env_steps_per_s=steps / (med * 1e-3))
        case['laneq_over_lane64'] = case['kernels']['lane64']['median_ms'] / case['kernels']['laneq']['median_ms']
        case['laneq_over_team4_queue'] = case['kernels']['team4_queue']['median_ms'] / case['kernels']['laneq']['median_ms']
        doc['cases'].append(case)
        print(json.dumps(case), flush=True)
        assert equal, 'the three kernels disagree'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


def sensor_noise():
    from serl_amd import build as hip_build, builds
    w = bench.make_population(a.members, 0, tag='serl50').to(eng.device)
    ref = refsignals.tabulate(*refsignals.base_reference(a.t_max), a.t_max)
    T = ref.shape[0]
    kernel = None if a.sn_kernel == 'auto' else a.sn_kernel
    for E in [int(x) for x in a.episodes.split(',')]:
        moe = ((np.arange(E) % a.members) if a.order == 'interleaved' else (np.arange(E) // max(E // a.members, 1)) % a.members).astype(np.int32)
        line = dict(what="mode 'noise', sensor noise %s" % ('from host tables' if a.sensor_noise == 'table' else 'drawn in the kernel'), sensor_noise=a.sensor_noise,
                    kernel=a.sn_kernel, episodes=E, steps_per_episode=T, members=a.members, order=a.order, reps=a.reps, source_hash=hip_build.source_hash(),
                    device=torch.cuda.get_device_name(0))
        if a.sensor_noise == 'table':
            t0 = time.perf_counter()
            host = np.empty((E, T + 1, 7))
            for e in range(E):
                host[e] = builds.sensor_noise_table(T, np.random)
            t1 = time.perf_counter()
            sn = torch.from_numpy(host).to(eng.device)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            line.update(table_bytes=int(host.nbytes), host_draw_s=t1 - t0, h2d_s=t2 - t1)
            del host
            kw = dict(sensor_noise=sn)
        else:
            kw = dict(sensor_noise='device', noise_seed=0x5EED)
        ms = []
        for i in range(-1, a.reps):      # (-1: warm-up, not recorded)
            out = eng.rollout(w, spec, moe, ref, t_max=a.t_max, kernel=kernel, **kw)
            if i >= 0:
                ms.append(eng.last_kernel_ms)
        info = eng.last_rollout_info()
        steps = int(out['length_steps'].abs().sum())
        med = float(np.median(ms))
        line.update(family=info['family'], workgroups=info['workgroups'], episodes_per_team_or_wave=info['episodes_per_team'], work_queue=info['work_queue'],
                    kernel_ms=[round(v, 2) for v in ms], median_ms=round(med, 2), min_ms=round(min(ms), 2), max_ms=round(max(ms), 2),
                    spread_ms=round(max(ms) - min(ms), 2), env_steps=steps, env_steps_per_s=steps / (med * 1e-3))
        if a.sensor_noise == 'table':
            line['end_to_end_s'] = line['host_draw_s'] + line['h2d_s'] + med * 1e-3
        print(json.dumps(line), flush=True)
        if a.out_json:
            doc = json.load(open(a.out_json)) if os.path.exists(a.out_json) else []
            doc.append(line)
            os.makedirs(os.path.dirname(os.path.abspath(a.out_json)), exist_ok=True)
            with open(a.out_json, 'w') as f:
                json.dump(doc, f, indent=1)
                f.write('\n')
        kw.clear()


if a.mixed_lengths:
    mixed_lengths()
    sys.exit(0)
if a.sensor_noise:
    sensor_noise()
    sys.exit(0)
w = bench.make_population(a.members, 0, tag='serl50').to(eng.device)
ref = refsignals.tabulate(*refsignals.base_reference(a.t_max), a.t_max)
T = ref.shape[0]
try:
    peak = float(json.load(open(os.path.join(ROOT, 'profiles', 'valu_latency_current.json')))['fp64_fma_peak_tflops_measured'])
except Exception:
    peak = None
base = None
for E in [int(x) for x in a.episodes.split(',')]:
    moe = ((np.arange(E) % a.members) if a.order == 'interleaved' else (np.arange(E) // max(E // a.members, 1)) % a.members).astype(np.int32)
    for mode in a.modes.split(','):
        kw = dict(lanes_per_wave=int(mode[4:])) if mode.startswith('lane') else dict(kernel=None if mode == 'auto' else mode)
        ms = []
        try:
            for _ in range(a.reps):
                out = eng.rollout(w, spec, moe, ref, t_max=a.t_max, **kw)
                ms.append(eng.last_kernel_ms)
        except Exception as ex:
            print(json.dumps(dict(episodes=E, mode=mode, error=repr(ex)[:300])), flush=True)
            continue
        steps = int(out['length_steps'].abs().sum())
        info = eng.last_rollout_info()
        k_ms = min(ms)
        rate = steps / (k_ms * 1e-3)
        extra = {}
        if a.profile and os.environ.get('SERL_PROFILE'):
            import ctypes
            buf = (ctypes.c_ulonglong * 32)()
            eng.lib.serl_debug_profile(eng.ctx, buf)
            st = max(int(buf[3]), 1)
            extra['cycles_per_env_step_wave0'] = dict(actor=int(buf[0] / st), dynamics=int(buf[1] / st), env=int(buf[2] / st), steps=int(buf[3]))
        chk = eng.rollout(w, spec, moe[:64], ref, t_max=a.t_max, kernel='team')
        same = bool(torch.equal(chk['fitness'], out['fitness'][:64]) and torch.equal(chk['length_steps'], out['length_steps'][:64]))
        print(json.dumps(dict(extra, what='saturating configuration (SURVEY 8d)', order=a.order, episodes=E, steps_per_episode=T, members=a.members, mode=mode, family=info['family'],
                              workgroups=info['workgroups'], episodes_per_team_or_wave=info['episodes_per_team'], work_queue=info['work_queue'],
                              kernel_ms=[round(v, 2) for v in ms], env_steps=steps, env_steps_per_s=rate,
                              us_per_env_step_and_wavefront_or_team=k_ms * 1e3 / T,
                              fp64_tflops_by_F_alg=rate * bench.F_ALG / 1e12, fp64_frac_of_measured_peak=(rate * bench.F_ALG / 1e12 / peak) if peak else None,
                              fp64_peak_measured_tflops=peak, first_64_episodes_equal_one_per_team=same)), flush=True)

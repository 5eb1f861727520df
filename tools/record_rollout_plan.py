"""Record WHAT the library launches for a table of rollout calls: tests/golden/rollout_plan.npz.

    python tools/record_rollout_plan.py [--out tests/golden/rollout_plan.npz]

Uses only RolloutEngine.rollout (plain and with device noise), rollout_multi, dynamics_open_loop and last_rollout_info, so it runs on
any commit that has them.  Every episode is ONE env step long (a one-row reference table, one zero actor shared by all episodes, no
traces): even the 80 x CUs cases are one short launch.  The development overrides (SERL_KERNEL ...) are read once per context, so each
override's cases run in a child process of their own started with that variable set -- one child at a time, each under a time limit;
the first child that fails ends the recording.

The file holds, per case: the inputs (columns COLS), the override in force (index into `overrides` / `caps`), the returned status and
the 8 words of serl_last_rollout_info (zeros where the call was refused).  tests/test_rollout_plan_host.py replays it on the host planner."""
import argparse, os, re, subprocess, sys, tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = ('entry', 'override', 'state_dim', 'action_dim', 'hidden', 'num_layers', 'n_members', 'n_episodes', 'lanes_per_wave',
        'concurrent_episodes', 'kernel_hint', 'env_config', 'incremental')
ENTRY_ROLLOUT, ENTRY_NOISE, ENTRY_DYN = 0, 1, 2
HINTS = (None, 'team', 'wave', 'half', 'team2', 'team4', 'laneq')      # _capi.KERNEL_HINTS order
# name, environment, and what serl_ctx_create makes of it: (env_kernel, env_waves_per_block, env_laneq_waves, env_split_actor, env_remote_actor, env_lane_regroup)
OVERRIDES = (('none', {}, (0, -1, -1, 0, 1, 1)),
             ('waves_per_block_2', {'SERL_WAVES_PER_BLOCK': '2'}, (0, 2, -1, 0, 1, 1)),
             ('laneq_waves_2', {'SERL_LANEQ_WAVES': '2'}, (0, -1, 2, 0, 1, 1)),
             ('remote_actor_0', {'SERL_REMOTE_ACTOR': '0'}, (0, -1, -1, 0, 0, 1)),
             ('split_actor_1', {'SERL_SPLIT_ACTOR': '1'}, (0, -1, -1, 1, 1, 1)),
             ('kernel_half', {'SERL_KERNEL': 'half'}, (3, -1, -1, 0, 1, 1)))
MULTI_PARTS = ((341, 341, 342), (600, 600), (2000, 40), (1, 1, 600, 600))
SHAPES = ((7, 3, 32, 0), (7, 3, 32, 3), (7, 3, 72, 1), (7, 3, 96, 1))      # state_dim, action_dim, hidden, num_layers
ENVS = ((0, 1), (1, 0), (2, 0))      # (env_config, incremental) other than the plain attitude task


def counts_for(cus, hidden):
    n = [1, cus, cus + 1, 2 * cus, 2 * cus + 1, 4 * cus, 4 * cus + 1, 80 * cus - 1, 80 * cus]
    if hidden != 32:      # the remote-actor residency edge: 16 * ceil(n / 8) <= CUs
        n += [8 * (cus // 16), 8 * (cus // 16) + 1]
    return sorted(set(n))


def cases_for(override, cus):
    """[(entry, shape, n_episodes, lanes_per_wave, concurrent_episodes, hint, (env_config, incremental))]"""
    from serl_amd import builds
    att = (0, 0)
    out = []
    add = lambda entry, shape, n, lanes=0, conc=0, hint=None, env=att: out.append((entry, shape, n, lanes, conc, hint, env))
    env_shape = lambda env: builds.env_dims(*env) + (32, 1)
    if override == 'none':
        for shape in SHAPES:
            for n in counts_for(cus, shape[2]):
                for hint in HINTS:
                    add(ENTRY_ROLLOUT, shape, n, hint=hint)
        for shape in (SHAPES[1], SHAPES[2]):
            for n in counts_for(cus, shape[2]):
                for conc in (100, 5000):
                    for hint in (None, 'team', 'wave', 'team4', 'laneq'):
                        add(ENTRY_ROLLOUT, shape, n, conc=conc, hint=hint)
            for lanes in (4, 64, 100):
                for n in (1, cus + 1, 80 * cus):
                    for hint in (None, 'team', 'laneq'):
                        add(ENTRY_ROLLOUT, shape, n, lanes=lanes, hint=hint)
                add(ENTRY_ROLLOUT, shape, 4 * cus + 1, lanes=lanes, conc=100, hint='laneq')
        for env in ENVS:
            for n in (cus, cus + 1, 2 * cus, 2 * cus + 1):
                for hint in HINTS:
                    add(ENTRY_ROLLOUT, env_shape(env), n, hint=hint, env=env)
                for conc in (100, 5000):
                    add(ENTRY_ROLLOUT, env_shape(env), n, conc=conc, env=env)
                add(ENTRY_NOISE, env_shape(env), n, env=env)
            add(ENTRY_ROLLOUT, env_shape(env), cus, lanes=4, env=env)
        for shape in (SHAPES[1], SHAPES[2]):
            for n in counts_for(cus, shape[2]):
                for hint in (None, 'wave'):
                    add(ENTRY_NOISE, shape, n, hint=hint)
                add(ENTRY_NOISE, shape, n, lanes=4)
                add(ENTRY_NOISE, shape, n, conc=100)
        for n in (1, cus, cus + 1, 4 * cus + 1):
            for hint in (None, 'team', 'wave'):
                add(ENTRY_DYN, (0, 0, 0, 0), n, hint=hint)
            add(ENTRY_DYN, (0, 0, 0, 0), n, lanes=4)
        add(ENTRY_DYN, (0, 0, 0, 0), cus, hint='half')
    elif override == 'waves_per_block_2':
        for shape in (SHAPES[1], SHAPES[2]):
            for n in (1, cus + 1, 4 * cus + 1, 80 * cus):
                for hint in (None, 'wave', 'half', 'laneq'):
                    add(ENTRY_ROLLOUT, shape, n, hint=hint)
                add(ENTRY_ROLLOUT, shape, n, lanes=4)
                add(ENTRY_NOISE, shape, n)
                add(ENTRY_NOISE, shape, n, lanes=4)
        for n in (1, cus + 1):
            add(ENTRY_ROLLOUT, env_shape(ENVS[1]), 2 * cus + n, env=ENVS[1])
            add(ENTRY_DYN, (0, 0, 0, 0), n, hint='wave')
            add(ENTRY_DYN, (0, 0, 0, 0), n, lanes=4)
    elif override == 'laneq_waves_2':
        for lanes in (0, 4):
            for conc in (0, 100):
                for n in (1, 200, 80 * cus):
                    add(ENTRY_ROLLOUT, SHAPES[1], n, lanes=lanes, conc=conc, hint='laneq')
        add(ENTRY_ROLLOUT, SHAPES[2], 200, hint='laneq')
        add(ENTRY_ROLLOUT, SHAPES[1], 200)
    elif override in ('remote_actor_0', 'split_actor_1'):
        for shape in SHAPES[1:]:
            for n in (1, 8 * (cus // 16), 8 * (cus // 16) + 1, cus, cus + 1):
                for hint in (None, 'team'):
                    add(ENTRY_ROLLOUT, shape, n, hint=hint)
            add(ENTRY_ROLLOUT, shape, 8, conc=8 * (cus // 16))
    elif override == 'kernel_half':
        for shape in SHAPES:
            for n in (1, cus + 1, 4 * cus + 1):
                add(ENTRY_ROLLOUT, shape, n)
                add(ENTRY_ROLLOUT, shape, n, hint='wave')
                add(ENTRY_ROLLOUT, shape, n, lanes=4)
        for n in (1, cus + 1):      # (the override reaches the noise and open-loop entries as a hint they refuse)
            add(ENTRY_NOISE, SHAPES[1], n)
            add(ENTRY_NOISE, SHAPES[1], n, hint='wave')
            add(ENTRY_NOISE, SHAPES[1], n, lanes=4)
            add(ENTRY_DYN, (0, 0, 0, 0), n)
        add(ENTRY_ROLLOUT, env_shape(ENVS[0]), cus, env=ENVS[0])
    return out


def _status(ex):
    m = re.search(r'failed \((-?\d+)\)', str(ex))
    if not m:
        raise ex
    return int(m.group(1))


def child(override, path):
    import torch
    import serl_amd
    from serl_amd import _capi
    k = [o[0] for o in OVERRIDES].index(override)
    eng = serl_amd.RolloutEngine(0)
    cus = eng.num_cus
    ref = np.zeros((1, 3))      # one row: max_steps = 1, every episode is one env step
    rows, status, info = [], [], []
    for entry, shape, n, lanes, conc, hint, env in cases_for(override, cus):
        S, A, H, L = shape
        try:
            if entry == ENTRY_DYN:
                eng.dynamics_open_loop(np.zeros((n, 1, 10)), lanes_per_wave=lanes, kernel=hint)
            else:
                spec = serl_amd.NetSpec(S, A, H, L, 'tanh')
                P = H * S + H + L * (H * H + 3 * H) + A * H + A
                kw = dict(sensor_noise='device', noise_seed=1) if entry == ENTRY_NOISE else {}
                eng.rollout(torch.zeros(1, (P + 3) // 4 * 4), spec, np.zeros(n, np.int32), ref, t_max=0.005, lanes_per_wave=lanes,
                            concurrent_episodes=conc, kernel=hint, env_config=env[0], incremental=bool(env[1]), sync=False, **kw)
            torch.cuda.synchronize()
            st, words = 0, eng.last_rollout_info()
            fam = {v: i for i, v in _capi.FAMILIES.items()}[words['family']]
            words = [fam, words['workgroups'], words['episodes_per_team'], int(words['work_queue']), words['actor_wavefronts'],
                     int(words['actor_streamed']), words['launches'], words['code']]
        except RuntimeError as ex:
            st, words = _status(ex), [0] * 8
        rows.append([entry, k, S, A, H, L, 0 if entry == ENTRY_DYN else 1, n, lanes, conc, _capi.KERNEL_HINTS[hint], env[0], env[1]])
        status.append(st)
        info.append(words)
    extra = {}
    if override == 'none':
        spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
        parts, mst, minfo = np.zeros((len(MULTI_PARTS), 4), np.int32), [], []
        for i, p in enumerate(MULTI_PARTS):
            parts[i, :len(p)] = p
            prepared = [eng.rollout(torch.zeros(1, spec.row_stride), spec, np.zeros(n, np.int32), ref, t_max=0.005, sync=False, launch=False) for n in p]
            ok = eng.rollout_multi(prepared)
            torch.cuda.synchronize()
            w = eng.last_rollout_info() if ok else None
            mst.append(0 if ok else _capi.E_UNSUPPORTED)
            minfo.append([0] * 8 if not ok else [{v: i for i, v in _capi.FAMILIES.items()}[w['family']], w['workgroups'], w['episodes_per_team'],
                                                  int(w['work_queue']), w['actor_wavefronts'], int(w['actor_streamed']), w['launches'], w['code']])
        extra = dict(multi_parts=parts, multi_status=np.asarray(mst, np.int32), multi_info=np.asarray(minfo, np.int32))
    np.savez(path, cases=np.asarray(rows, np.int32), status=np.asarray(status, np.int32), info=np.asarray(info, np.int32),
             num_cus=np.int32(cus), **extra)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'rollout_plan.npz'))
    ap.add_argument('--child')
    ap.add_argument('--timeout', type=float, default=240.0)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.out)
        return 0
    parts = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, env, _ in OVERRIDES:
            path = os.path.join(tmp, name + '.npz')
            clean = {k: v for k, v in os.environ.items() if not k.startswith('SERL_') or k == 'SERL_LIB'}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', name, '--out', path], env=dict(clean, **env), timeout=a.timeout)
            if r.returncode != 0:
                print('record_rollout_plan: child %s ended with %d: stopping' % (name, r.returncode), file=sys.stderr)
                return 1
            with np.load(path) as z:
                parts.append({k: z[k] for k in z.files})
            print('%s: %d cases' % (name, len(parts[-1]['cases'])), flush=True)
    cus = int(parts[0]['num_cus'])
    assert all(int(p['num_cus']) == cus for p in parts)
    np.savez_compressed(a.out, cols=np.asarray(COLS), cases=np.concatenate([p['cases'] for p in parts]), status=np.concatenate([p['status'] for p in parts]),
                        info=np.concatenate([p['info'] for p in parts]), num_cus=np.int32(cus), overrides=np.asarray([o[0] for o in OVERRIDES]),
                        caps=np.asarray([(cus,) + o[2] for o in OVERRIDES], np.int32), multi_parts=parts[0]['multi_parts'],
                        multi_status=parts[0]['multi_status'], multi_info=parts[0]['multi_info'])
    print('wrote %s: %d cases, num_cus %d' % (a.out, sum(len(p['cases']) for p in parts), cus))
    return 0


if __name__ == '__main__':
    sys.exit(main())

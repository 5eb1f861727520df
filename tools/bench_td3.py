#!/usr/bin/env python
"""ms per TD3 update: the fused launch (serl_td3_train) against the eager float32 PyTorch loop on the same GPU.

The eager loop is the tests' literal restatement of the reference's update (tests/td3_64.py: td3_literal with dtype=float32,
device='cuda') -- what a SERL user runs today.  Both get the same rows, ring, slots and draws.  Per shape: one warm-up run of each, then
`--reps` timed repetitions (host wall clock around a synchronised run; the fused launch also by device events), reported as median and
range.  Results go to profiles/td3_fused_timing.json.

With --dense the two flavours of the fused kernel are compared instead -- serl_td3_train ('valu') and serl_td3_train_mfma ('mfma', the
dense phases on the f32 matrix cores) -- in one process on the same inputs, alternating, device events only; the final rows of the
flavours are checked to be equal.  Results, with the source hash, go to profiles/td3_mfma_timing.json.

  python tools/bench_td3.py                      # hidden 72 / 32 / 96, 3 layers, minibatch 86, CAPS on, 2 000 updates
  python tools/bench_td3.py --hidden 72 --updates 200 --eager-updates 50 --reps 3
  python tools/bench_td3.py --dense valu,mfma    # the same shapes, both kernels

With --draws the two ways of drawing the minibatches and the noise are compared -- 'host' (python's random and a torch CPU generator,
uploaded as tables: serl_td3_train / _mfma, the path of the commit before the generator) and 'device' (serl_td3_train_rng, drawn inside
the kernel) -- in one process, alternating: (a) device ms per update of the four kernels, the table kernels fed serl_td3_rng_fill's
tables so that all four compute the same rows (checked); (b) wall time of TD3.train end to end, host draws and upload included; (c) the
bytes of tables each mode put on the device.  Hidden 72 unless --hidden says otherwise.  Results go to profiles/td3_rng_timing.json.

  python tools/bench_td3.py --draws host,device  # 2 000 updates per launch; TD3.train at 2 000 and 20 000 updates
"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch


ENTRY = {'valu': 'serl_td3_train', 'mfma': 'serl_td3_train_mfma'}


def fused_run(engine, d, n, dense='valu', rows_out=None, rng_seed=None):
    """-> (device ms, wall ms) of one launch of n updates of serl_td3_train (dense='mfma': serl_td3_train_mfma) on fresh copies of the
    case's rows; with rows_out (a dict) the four rows after the launch are left in it.  With rng_seed the launch is serl_td3_train_rng
    with that seed, slots from all rows of the case's ring, and no table is uploaded."""
    import td3_64 as T
    from serl_amd import _capi
    L = _capi.lib()
    dev = engine.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rows = {k: t(d[k]) for k in T.ROWS}
    for k in T.MOMENTS:
        rows[k] = torch.zeros_like(rows[k.split('_')[0]])
    steps = torch.zeros(2, dtype=torch.int32, device=dev)
    ring = t(d['ring'])
    slots = tn = cn = None
    if rng_seed is None:
        slots, tn = t(d['slots'][:n]), t(d['tn'][:n])
        cn = t(d['cn']) if d['caps'] else None
    td, pg = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    wb = int(L.serl_td3_work_bytes(1, d['S'], d['A'], d['H'], d['L'], d['B']))
    work = torch.empty(wb // 4, dtype=torch.float32, device=dev)
    desc = _capi.Td3Desc(state_dim=d['S'], action_dim=d['A'], hidden=d['H'], num_layers=d['L'], activation={'tanh': 0, 'elu': 1, 'relu': 2}[d['act']],
                         n_learners=1, batch=d['B'], n_updates=n, capacity=ring.shape[0], slot_cols=d['B'], policy_update_freq=d['freq'],
                         iteration0=d['it0'], update_actor_target=int(d['uat']), lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD,
                         noise_clip=T.NOISE_CLIP, lambda_s=T.CAPS['lambda_s'], lambda_t=T.CAPS['lambda_t'], eps_sd=T.CAPS['eps_sd'],
                         max_grad_norm=T.MAX_NORM, actor=rows['actor'].data_ptr(), actor_target=rows['actor_target'].data_ptr(),
                         actor_m=rows['actor_m'].data_ptr(), actor_v=rows['actor_v'].data_ptr(), actor_stride=rows['actor'].numel(),
                         critic=rows['critic'].data_ptr(), critic_target=rows['critic_target'].data_ptr(), critic_m=rows['critic_m'].data_ptr(),
                         critic_v=rows['critic_v'].data_ptr(), critic_stride=rows['critic'].numel(), adam_steps=steps.data_ptr(),
                         ring=ring.data_ptr(), slots=slots.data_ptr() if slots is not None else None,
                         target_noise=tn.data_ptr() if tn is not None else None,
                         caps_noise=cn.data_ptr() if cn is not None else None, td_loss=td.data_ptr(), pg_loss=pg.data_ptr(), loss_stride=n,
                         work=work.data_ptr(), work_bytes=wb)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    e0.record()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if rng_seed is None:
        _capi.check(getattr(L, ENTRY[dense])(engine.ctx, ctypes.byref(desc), stream), ENTRY[dense])
    else:
        rd = _capi.Td3RngDesc(seed=rng_seed, n_rows=ring.shape[0], learner0=0, dense=int(dense == 'mfma'), caps=int(bool(d['caps'])))
        _capi.check(L.serl_td3_train_rng(engine.ctx, ctypes.byref(desc), ctypes.byref(rd), stream), 'serl_td3_train_rng')
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - w0) * 1e3
    assert torch.isfinite(td).all()
    if rows_out is not None:
        rows_out.update({k: rows[k].cpu().numpy() for k in T.ROWS}, td=td.cpu().numpy())
    return e0.elapsed_time(e1), wall


def eager_run(d, n):
    import td3_64 as T
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    r = T.td3_literal(d, torch.float32, 'cuda', n)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - w0) * 1e3
    assert np.isfinite(r['td']).all()
    return wall


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hidden', type=int, nargs='*', default=None, help='default: 72 32 96; with --draws 72')
    ap.add_argument('--layers', type=int, default=3)
    ap.add_argument('--batch', type=int, default=86)
    ap.add_argument('--updates', type=int, default=2000)
    ap.add_argument('--eager-updates', type=int, default=300, help='updates of one eager repetition (the loop is slow; ms per update is what is compared)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only-fused', action='store_true', help='one fused launch per shape and nothing else (for a kernel trace)')
    ap.add_argument('--dense', default=None, help="'valu,mfma': time the flavours of the fused kernel against each other (no eager loop)")
    ap.add_argument('--draws', default=None, help="'host,device': time the table path against the in-kernel generator (kernels and TD3.train)")
    ap.add_argument('--train-updates', type=int, nargs='*', default=[2000, 20000], help='with --draws: updates of one TD3.train call')
    ap.add_argument('--out', default=None, help='default: profiles/td3_fused_timing.json, with --dense profiles/td3_mfma_timing.json, '
                                                'with --draws profiles/td3_rng_timing.json')
    a = ap.parse_args()
    if a.hidden is None:
        a.hidden = [72] if a.draws else [72, 32, 96]
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'td3_rng_timing.json' if a.draws else 'td3_mfma_timing.json' if a.dense else 'td3_fused_timing.json')
    import serl_amd
    import td3_64 as T
    engine = serl_amd.RolloutEngine(0)
    if a.draws:
        return draws_main(a, engine)
    if a.dense:
        return dense_main(a, engine)
    res = {'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'layers': a.layers, 'updates': a.updates, 'eager_updates': a.eager_updates,
           'caps': True, 'policy_update_freq': 2, 'shapes': {}}
    for H in a.hidden:
        d = T.make_case((7, 3, H, a.layers, 'tanh', a.batch, 2, 0, a.updates, 1, 1, 'small'), seed=H)
        fused_run(engine, d, min(a.updates, 50))                        # warm-up
        if a.only_fused:
            print('H %d fused %.3f ms per update' % (H, fused_run(engine, d, a.updates)[0] / a.updates))
            continue
        eager_run(d, 20)
        f = [fused_run(engine, d, a.updates) for _ in range(a.reps)]
        e = [eager_run(d, a.eager_updates) / a.eager_updates for _ in range(a.reps)]
        r = {'fused_ms_per_update_device': spread([x[0] / a.updates for x in f]), 'fused_ms_per_update_wall': spread([x[1] / a.updates for x in f]),
             'eager_f32_ms_per_update_wall': spread(e)}
        r['speedup_median'] = r['eager_f32_ms_per_update_wall']['median'] / r['fused_ms_per_update_wall']['median']
        res['shapes']['H%d_L%d_B%d' % (H, a.layers, a.batch)] = r
        print('H %d  fused %.4f ms/update (device; wall %.4f)  eager f32 %.3f ms/update  x%.1f' % (
            H, r['fused_ms_per_update_device']['median'], r['fused_ms_per_update_wall']['median'], r['eager_f32_ms_per_update_wall']['median'],
            r['speedup_median']), flush=True)
    if not a.only_fused:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps(res))


def dense_main(a, engine):
    import td3_64 as T
    from serl_amd import build as hip_build
    flavours = a.dense.split(',')
    assert flavours and all(f in ENTRY for f in flavours), a.dense
    res = {'tool': 'bench_td3 --dense ' + a.dense, 'device': torch.cuda.get_device_name(0), 'source_hash': hip_build.source_hash(), 'batch': a.batch,
           'layers': a.layers, 'updates': a.updates, 'reps': a.reps, 'caps': True, 'policy_update_freq': 2, 'activation': 'tanh', 'shapes': {}}
    for H in a.hidden:
        d = T.make_case((7, 3, H, a.layers, 'tanh', a.batch, 2, 0, a.updates, 1, 1, 'small'), seed=H)
        rows = {f: {} for f in flavours}
        for f in flavours:
            fused_run(engine, d, min(a.updates, 50), f)                 # warm-up
        ms = {f: [] for f in flavours}
        for _ in range(a.reps):                                         # alternating: a drift of the clock hits both alike
            for f in flavours:
                ms[f].append(fused_run(engine, d, a.updates, f, rows[f])[0] / a.updates)
        r = {f + '_ms_per_update_device': spread(ms[f]) for f in flavours}
        same = all(np.array_equal(rows[f][k], rows[flavours[0]][k]) for f in flavours for k in rows[f])
        r['rows_equal'] = bool(same)
        if 'valu' in ms and 'mfma' in ms:
            r['valu_over_mfma_median'] = r['valu_ms_per_update_device']['median'] / r['mfma_ms_per_update_device']['median']
        res['shapes']['H%d_L%d_B%d' % (H, a.layers, a.batch)] = r
        print('H %d  %s  rows equal: %s' % (H, '  '.join('%s %.4f [%.4f .. %.4f] ms/update' % (f, r[f + '_ms_per_update_device']['median'],
              r[f + '_ms_per_update_device']['min'], r[f + '_ms_per_update_device']['max']) for f in flavours), same), flush=True)
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


def draws_main(a, engine):
    import random
    import types
    import serl_amd
    import td3_64 as T
    from serl_amd import build as hip_build
    modes = a.draws.split(',')
    assert modes and all(m in ('host', 'device') for m in modes), a.draws
    seed = 20261019
    dev = engine.device
    res = {'tool': 'bench_td3 --draws ' + a.draws, 'device': torch.cuda.get_device_name(0), 'source_hash': hip_build.source_hash(), 'batch': a.batch,
           'layers': a.layers, 'updates': a.updates, 'reps': a.reps, 'caps': True, 'policy_update_freq': 2, 'activation': 'tanh', 'seed': seed,
           'shapes': {}}
    for H in a.hidden:
        d = T.make_case((7, 3, H, a.layers, 'tanh', a.batch, 2, 0, 4, 1, 1, 'small'), seed=H)
        # (a) the four kernels on the same draws: the generator's, replayed as tables for the two table kernels
        sl, tn, cn = serl_amd.td3_draws(engine, seed=seed, learner=0, iteration0=0, n_updates=a.updates, batch=a.batch, n_rows=d['ring'].shape[0],
                                        state_dim=7, action_dim=3, policy_update_freq=2, caps=True)
        dt = dict(d, slots=sl.cpu().numpy(), tn=tn.cpu().numpy(), cn=cn.cpu().numpy())
        kernels = [(m, f) for m in modes for f in ('valu', 'mfma')]
        name = lambda m, f: ENTRY[f] if m == 'host' else 'serl_td3_train_rng(dense=%d)' % (f == 'mfma')
        run = lambda m, f, n, out=None: fused_run(engine, dt, n, f, out, seed if m == 'device' else None)
        for m, f in kernels:
            run(m, f, min(a.updates, 50))                               # warm-up
        ms, rows = {k: [] for k in kernels}, {k: {} for k in kernels}
        for _ in range(a.reps):                                         # alternating: a drift of the clock hits all alike
            for k in kernels:
                ms[k].append(run(k[0], k[1], a.updates, rows[k])[0] / a.updates)
        r = {'kernel_ms_per_update_device': {name(*k): spread(ms[k]) for k in kernels}}
        r['rows_equal'] = bool(all(np.array_equal(rows[k][x], rows[kernels[0]][x]) for k in kernels for x in rows[k]))
        for k in kernels:
            print('H %d  %-32s %.4f [%.4f .. %.4f] ms/update' % (H, name(*k), r['kernel_ms_per_update_device'][name(*k)]['median'], min(ms[k]), max(ms[k])), flush=True)
        print('H %d  rows equal: %s' % (H, r['rows_equal']), flush=True)
        # (b), (c) TD3.train end to end on a ring of 20 000 rows: host draws, upload, launch, write-back
        args = types.SimpleNamespace(state_dim=7, action_dim=3, hidden_size=H, num_layers=a.layers, activation_actor='tanh', device='cpu',
                                     individual_bs=64, lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP,
                                     policy_update_freq=2, use_caps=True, batch_size=a.batch)
        ring = serl_amd.DeviceReplay(20000, dev, engine, 7, 3)
        ring.append_rows(torch.from_numpy(np.tile(d['ring'], (20000 // d['ring'].shape[0], 1))))

        def train(mode, n):
            torch.manual_seed(H)
            t = serl_amd.TD3(args, engine)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            out = t.train(ring, n, iteration0=0, rng=random.Random(1), generator=torch.Generator().manual_seed(1), draws=mode, seed=seed)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - w0) * 1e3
            assert np.isfinite(out['TD_loss']) and t.last_path == ('fused-rng' if mode == 'device' else 'fused')
            return wall, t.last_table_bytes
        r['train_wall_ms'], r['table_bytes'] = {}, {}
        for n in a.train_updates:
            for m in modes:
                train(m, min(n, 50))                                    # warm-up
            wall, tb = {m: [] for m in modes}, {}
            for _ in range(a.reps):
                for m in modes:
                    w, tb[m] = train(m, n)
                    wall[m].append(w)
            r['train_wall_ms'][str(n)] = {m: spread(wall[m]) for m in modes}
            r['table_bytes'][str(n)] = tb
            print('H %d  TD3.train %6d updates  %s' % (H, n, '  '.join('%s %.1f [%.1f .. %.1f] ms, tables %d B' % (
                m, statistics.median(wall[m]), min(wall[m]), max(wall[m]), tb[m]) for m in modes)), flush=True)
        res['shapes']['H%d_L%d_B%d' % (H, a.layers, a.batch)] = r
    with open(a.out, 'w') as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

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

With --group K learners of the benchmark shape (hidden 72 unless --hidden says otherwise), each with its own rows, ring, seed and key, run
their --updates updates as ONE serl_td3_train_group launch, against K back-to-back single-learner serl_td3_train_rng launches on the same
buffers -- what the library offered before the group entry.  Both dense flavours, the two versions alternating in one process, device
events, median [min .. max] of --reps repetitions after a warm-up; the rows of the two versions are checked to be equal.  The
back-to-back version costs K launches per repetition: --serial-max bounds the K up to which it is run (beyond it only the group launch
is timed, and the result says so).  --kernel-regs takes the output of tools/kernel_regs.sh for the record.  Results go to
profiles/td3_group_timing.json, rewritten after every K.

  python tools/bench_td3.py --group 1,2,4,8,16,32,64,128,256

With --batch B1,B2,... (a list) the chunked kernel serl_td3_train_big is timed at each minibatch size in both dense flavours, against the
eager float32 loop at the same size (what a user with such a minibatch gets by default) and, up to 128 rows, against the unchanged
serl_td3_train / _mfma on the same inputs -- the cost of the chunk loop at one chunk.  Rings of 640 rows (tests/td3_big.py), hidden 72
unless --hidden says otherwise, the protocol of --dense: one process, alternating, device events, median [min .. max] of --reps
repetitions after a warm-up.  Results, with ms per sample, go to profiles/td3_batch_timing.json.

  python tools/bench_td3.py --batch 86,128,256,512

With --group K1,K2,... AND a --batch list (or one size above 128) the group launches of large minibatches are timed: ONE
serl_td3_train_group_big launch (chunks 'serial') or serl_td3_train_group_wide launch ('parallel') of K learners against K back-to-back
single-learner generator launches of the entry points the library had before them, on the same buffers -- serl_td3_train_big for serial,
serl_td3_train_wide for parallel.  --chunks picks the versions (default serial,parallel); all of them alternate in one process, both
dense flavours, device events, --reps repetitions after a warm-up; the final rows of every version of a (K, B) must be equal, and the
tool stops if they are not.  A parallel launch whose K x chunks workgroups outnumber the CUs is not run (the library refuses it), and the
result says so; --serial-max bounds the back-to-back legs.  The K = 1 rows are also the generator flavours' time at these sizes.
Results go to profiles/td3_group_big_timing.json, rewritten after every (K, B).

  python tools/bench_td3.py --group 1,8,32 --batch 256,512 --updates 100
"""
import argparse, ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch


ENTRY = {'valu': 'serl_td3_train', 'mfma': 'serl_td3_train_mfma'}


def fused_run(engine, d, n, dense='valu', rows_out=None, rng_seed=None, big=False, wide=False):
    """-> (device ms, wall ms) of one launch of n updates of serl_td3_train (dense='mfma': serl_td3_train_mfma) on fresh copies of the
    case's rows; with rows_out (a dict) the four rows after the launch are left in it.  With rng_seed the launch is serl_td3_train_rng
    with that seed, slots from all rows of the case's ring, and no table is uploaded.  big: serl_td3_train_big (tables) instead; wide: serl_td3_train_wide
    (tables), its status checked."""
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
    wb = int((L.serl_td3_wide_work_bytes if wide else L.serl_td3_big_work_bytes if big else L.serl_td3_work_bytes)(1, d['S'], d['A'], d['H'], d['L'], d['B']))
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
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
    if wide:
        wd = _capi.Td3WideDesc(rng=None, status=status.data_ptr(), dense=int(dense == 'mfma'))
        _capi.check(L.serl_td3_train_wide(engine.ctx, ctypes.byref(desc), ctypes.byref(wd), stream), 'serl_td3_train_wide')
    elif big:
        bd = _capi.Td3BigDesc(rng=None, dense=int(dense == 'mfma'))
        _capi.check(L.serl_td3_train_big(engine.ctx, ctypes.byref(desc), ctypes.byref(bd), stream), 'serl_td3_train_big')
    elif rng_seed is None:
        _capi.check(getattr(L, ENTRY[dense])(engine.ctx, ctypes.byref(desc), stream), ENTRY[dense])
    else:
        rd = _capi.Td3RngDesc(seed=rng_seed, n_rows=ring.shape[0], learner0=0, dense=int(dense == 'mfma'), caps=int(bool(d['caps'])))
        _capi.check(L.serl_td3_train_rng(engine.ctx, ctypes.byref(desc), ctypes.byref(rd), stream), 'serl_td3_train_rng')
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - w0) * 1e3
    assert torch.isfinite(td).all() and (not wide or int(status[0]) == 0), status
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
    ap.add_argument('--batch', default='86', help="a minibatch size; a list 'B1,B2,...' times serl_td3_train_big at each (see above)")
    ap.add_argument('--chunks', default=None, help="'serial,parallel' with a --batch list: serl_td3_train_big against serl_td3_train_wide at each size "
                                                   '(-> profiles/td3_wide_timing.json)')
    ap.add_argument('--updates', type=int, default=2000)
    ap.add_argument('--eager-updates', type=int, default=300, help='updates of one eager repetition (the loop is slow; ms per update is what is compared)')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only-fused', action='store_true', help='one fused launch per shape and nothing else (for a kernel trace)')
    ap.add_argument('--dense', default=None, help="'valu,mfma': time the flavours of the fused kernel against each other (no eager loop)")
    ap.add_argument('--draws', default=None, help="'host,device': time the table path against the in-kernel generator (kernels and TD3.train)")
    ap.add_argument('--train-updates', type=int, nargs='*', default=[2000, 20000], help='with --draws: updates of one TD3.train call')
    ap.add_argument('--group', default=None, help="'1,2,4,...': K learners in one serl_td3_train_group launch against K serl_td3_train_rng launches")
    ap.add_argument('--serial-max', type=int, default=None, help='with --group: the largest K whose K back-to-back launches are run (default: all)')
    ap.add_argument('--kernel-regs', default=None, help='with --group: a file holding the output of tools/kernel_regs.sh <serl_td3 object> td3_kernel')
    ap.add_argument('--out', default=None, help='default: profiles/td3_fused_timing.json, with --dense profiles/td3_mfma_timing.json, '
                                                'with --draws profiles/td3_rng_timing.json')
    a = ap.parse_args()
    batches = [int(b) for b in a.batch.split(',')] if ',' in a.batch else None
    a.batch = int(a.batch) if batches is None else batches[0]
    if a.hidden is None:
        a.hidden = [72] if a.draws or a.group or batches else [72, 32, 96]
    group_big = bool(a.group) and (batches is not None or a.batch > 128 or a.chunks is not None)
    if a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'td3_group_big_timing.json' if group_big else 'td3_wide_timing.json' if a.chunks else 'td3_batch_timing.json' if batches else 'td3_group_timing.json' if a.group else 'td3_rng_timing.json' if a.draws else 'td3_mfma_timing.json' if a.dense else 'td3_fused_timing.json')
    import serl_amd
    import td3_64 as T
    engine = serl_amd.RolloutEngine(0)
    if group_big:
        return group_big_main(a, engine, batches or [a.batch])
    if a.chunks:
        assert batches and sorted(a.chunks.split(',')) == ['parallel', 'serial'], '--chunks serial,parallel needs a --batch list'
        return chunks_main(a, engine, batches)
    if batches:
        return batch_main(a, engine, batches)
    if a.group:
        return group_main(a, engine)
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


def batch_main(a, engine, batches):
    import td3_big as TB
    from serl_amd import _capi, build as hip_build
    H = a.hidden[0]
    res = {'tool': 'bench_td3 --batch ' + ','.join(str(b) for b in batches), 'device': torch.cuda.get_device_name(0),
           'source_hash': hip_build.source_hash(), 'hidden': H, 'layers': a.layers, 'updates': a.updates, 'eager_updates': a.eager_updates,
           'reps': a.reps, 'caps': True, 'policy_update_freq': 2, 'activation': 'tanh', 'ring_rows': TB.RING_ROWS, 'batches': {}}
    for B in batches:
        d = TB.make_case((7, 3, H, a.layers, 'tanh', B, 2, 0, a.updates, 1, 1, 'small'), seed=H)
        runs = [('big_' + f, dict(dense=f, big=True)) for f in ENTRY] + ([(f, dict(dense=f)) for f in ENTRY] if B <= 128 else [])
        rows = {k: {} for k, _ in runs}
        for _, kw in runs:
            fused_run(engine, d, min(a.updates, 50), **kw)              # warm-up
        eager_run(d, 20)
        ms = {k: [] for k, _ in runs}
        eager = []
        for _ in range(a.reps):                                         # alternating: a drift of the clock hits all alike
            for k, kw in runs:
                ms[k].append(fused_run(engine, d, a.updates, rows_out=rows[k], **kw)[0] / a.updates)
            eager.append(eager_run(d, a.eager_updates) / a.eager_updates)
        r = {k + '_ms_per_update_device': spread(ms[k]) for k in ms}
        r['eager_f32_ms_per_update_wall'] = spread(eager)
        r['rows_equal'] = bool(all(np.array_equal(rows[k][x], rows['big_valu'][x]) for k in rows for x in rows[k]))
        for f in ENTRY:
            m = r['big_%s_ms_per_update_device' % f]['median']
            r['big_%s_us_per_sample' % f] = 1e3 * m / B
            r['eager_over_big_%s_median' % f] = r['eager_f32_ms_per_update_wall']['median'] / m
            if B <= 128:
                r['big_over_old_%s_median' % f] = m / r[f + '_ms_per_update_device']['median']
        r['work_bytes'] = int(_capi.lib().serl_td3_big_work_bytes(1, 7, 3, H, a.layers, B))
        res['batches']['B%d' % B] = r
        print('B %d  %s  eager %.3f ms/update  rows equal: %s' % (B, '  '.join('%s %.4f [%.4f .. %.4f]' % (
            k, r[k + '_ms_per_update_device']['median'], r[k + '_ms_per_update_device']['min'], r[k + '_ms_per_update_device']['max']) for k in ms),
            r['eager_f32_ms_per_update_wall']['median'], r['rows_equal']), flush=True)
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1)
    print(json.dumps(res))


def chunks_main(a, engine, batches):
    """the protocol of batch_main without the eager loop: at each size serl_td3_train_big (serial) and serl_td3_train_wide (parallel) in
    both dense flavours, and serl_td3_train / _mfma where they run, alternating in one process, final rows compared"""
    import td3_big as TB
    from serl_amd import _capi, build as hip_build
    H = a.hidden[0]
    res = {'tool': 'bench_td3 --batch %s --chunks serial,parallel' % ','.join(str(b) for b in batches), 'device': torch.cuda.get_device_name(0),
           'source_hash': hip_build.source_hash(), 'hidden': H, 'layers': a.layers, 'updates': a.updates, 'reps': a.reps, 'caps': True,
           'policy_update_freq': 2, 'activation': 'tanh', 'ring_rows': TB.RING_ROWS, 'batches': {}}
    for B in batches:
        d = TB.make_case((7, 3, H, a.layers, 'tanh', B, 2, 0, a.updates, 1, 1, 'small'), seed=H)
        runs = ([('serial_' + f, dict(dense=f, big=True)) for f in ENTRY] + [('parallel_' + f, dict(dense=f, wide=True)) for f in ENTRY] +
                ([(f, dict(dense=f)) for f in ENTRY] if B <= 128 else []))
        rows = {k: {} for k, _ in runs}
        for _, kw in runs:
            fused_run(engine, d, min(a.updates, 50), **kw)              # warm-up
        ms = {k: [] for k, _ in runs}
        for _ in range(a.reps):                                         # alternating: a drift of the clock hits all alike
            for k, kw in runs:
                ms[k].append(fused_run(engine, d, a.updates, rows_out=rows[k], **kw)[0] / a.updates)
        r = {k + '_ms_per_update_device': spread(ms[k]) for k in ms}
        r['rows_equal'] = bool(all(np.array_equal(rows[k][x], rows['serial_valu'][x]) for k in rows for x in rows[k]))
        for f in ENTRY:
            s_, p_ = r['serial_%s_ms_per_update_device' % f], r['parallel_%s_ms_per_update_device' % f]
            r['serial_%s_us_per_sample' % f], r['parallel_%s_us_per_sample' % f] = 1e3 * s_['median'] / B, 1e3 * p_['median'] / B
            r['serial_over_parallel_%s_median' % f] = s_['median'] / p_['median']
            r['parallel_%s_median_below_serial_min' % f] = bool(p_['median'] < s_['min'])
            if B <= 128:
                o = r[f + '_ms_per_update_device']
                r['parallel_%s_median_inside_old_spread' % f] = bool(o['min'] <= p_['median'] <= o['max'])
        r['work_bytes'] = int(_capi.lib().serl_td3_wide_work_bytes(1, 7, 3, H, a.layers, B))
        res['batches']['B%d' % B] = r
        print('B %d  %s  rows equal: %s' % (B, '  '.join('%s %.4f [%.4f .. %.4f]' % (
            k, r[k + '_ms_per_update_device']['median'], r[k + '_ms_per_update_device']['min'], r[k + '_ms_per_update_device']['max']) for k in ms),
            r['rows_equal']), flush=True)
    # the hand-over cost per update, as a DIFFERENCE of two timings of this run (no counter): wide at the largest size minus the 128-row time
    if 'B128' in res['batches'] and len(batches) > 1:
        big_b = 'B%d' % max(batches)
        for f in ENTRY:
            res['handover_ms_per_update_%s_%s_minus_B128' % (f, big_b)] = (
                res['batches'][big_b]['parallel_%s_ms_per_update_device' % f]['median'] - res['batches']['B128']['parallel_%s_ms_per_update_device' % f]['median'])
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


def group_main(a, engine):
    import td3_64 as T
    from serl_amd import _capi
    from serl_amd import build as hip_build
    L = _capi.lib()
    dev = engine.device
    Ks = [int(k) for k in a.group.split(',')]
    assert Ks and min(Ks) >= 1, a.group
    seed, n, B, Ly = 20261020, a.updates, a.batch, a.layers
    regs = [ln.strip() for ln in open(a.kernel_regs)] if a.kernel_regs else None
    res = {'tool': 'bench_td3 --group ' + a.group, 'device': torch.cuda.get_device_name(0), 'source_hash': hip_build.source_hash(), 'batch': B,
           'layers': Ly, 'updates_per_learner': n, 'reps': a.reps, 'caps': True, 'policy_update_freq': 2, 'activation': 'tanh', 'seed': seed,
           'serial_max': a.serial_max, 'kernel_resources': regs,
           'what': 'ms of ONE launch of K learners (group) and of K back-to-back single-learner launches (serial), device events; per_update = '
                   'ms / updates_per_learner: the time one more update of EVERY learner costs', 'shapes': {}}
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for H in a.hidden:
        d = T.make_case((7, 3, H, Ly, 'tanh', B, 2, 0, 4, 1, 1, 'small'), seed=H)
        cap = d['ring'].shape[0]
        shape = res['shapes'].setdefault('H%d_L%d_B%d' % (H, Ly, B), {})
        for K in Ks:
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            init = {k: t(np.tile(d[k], (K, 1))) for k in T.ROWS}
            rings = t(np.tile(d['ring'], (K, 1, 1)))
            wb = int(L.serl_td3_work_bytes(K, 7, 3, H, Ly, B))
            work = torch.empty(wb // 4, dtype=torch.float32, device=dev)
            table = (_capi.Td3LearnerRow * K)()
            for i in range(K):
                table[i] = _capi.Td3LearnerRow(ring=rings[i].data_ptr(), seed=seed, capacity=cap, n_rows=cap, n_updates=n, iteration0=0, key=i,
                                               policy_update_freq=2, update_actor_target=1, lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD,
                                               noise_clip=T.NOISE_CLIP, **T.CAPS)
            table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)

            def run(version, dense, n_, rows_out=None):
                rows = {k: v.clone() for k, v in init.items()}
                for k in T.MOMENTS:
                    rows[k] = torch.zeros_like(rows[k.split('_')[0]])
                steps = torch.zeros(K, 2, dtype=torch.int32, device=dev)
                td, pg = torch.zeros(K, n_, device=dev), torch.zeros(K, n_, device=dev)
                status = torch.full((K,), -1, dtype=torch.int32, device=dev)

                def desc(first, k):
                    return _capi.Td3Desc(
                        state_dim=7, action_dim=3, hidden=H, num_layers=Ly, activation=0, n_learners=k, batch=B, n_updates=n_, capacity=cap,
                        policy_update_freq=2, iteration0=0, update_actor_target=1, lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD,
                        noise_clip=T.NOISE_CLIP, lambda_s=T.CAPS['lambda_s'], lambda_t=T.CAPS['lambda_t'], eps_sd=T.CAPS['eps_sd'], max_grad_norm=T.MAX_NORM,
                        actor=rows['actor'][first].data_ptr(), actor_target=rows['actor_target'][first].data_ptr(),
                        actor_m=rows['actor_m'][first].data_ptr(), actor_v=rows['actor_v'][first].data_ptr(), actor_stride=rows['actor'].stride(0),
                        critic=rows['critic'][first].data_ptr(), critic_target=rows['critic_target'][first].data_ptr(),
                        critic_m=rows['critic_m'][first].data_ptr(), critic_v=rows['critic_v'][first].data_ptr(),
                        critic_stride=rows['critic'].stride(0), adam_steps=steps[first].data_ptr(), ring=rings[first].data_ptr(),
                        td_loss=td[first].data_ptr(), pg_loss=pg[first].data_ptr(), loss_stride=n_, work=work.data_ptr(), work_bytes=wb)
                if n_ != n:                                              # (the warm-up: fewer updates in every row)
                    short = (_capi.Td3LearnerRow * K).from_buffer_copy(bytes(table))
                    for i in range(K):
                        short[i].n_updates = n_
                    tb = torch.frombuffer(bytearray(bytes(short)), dtype=torch.uint8).to(dev)
                else:
                    tb = table_d
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                if version == 'group':
                    gd = _capi.Td3GroupDesc(rows=tb.data_ptr(), status=status.data_ptr(), dense=int(dense == 'mfma'), caps=1)
                    _capi.check(L.serl_td3_train_group(engine.ctx, ctypes.byref(desc(0, K)), ctypes.byref(gd), stream()), 'serl_td3_train_group')
                else:
                    for i in range(K):
                        rd = _capi.Td3RngDesc(seed=seed, n_rows=cap, learner0=i, dense=int(dense == 'mfma'), caps=1)
                        _capi.check(L.serl_td3_train_rng(engine.ctx, ctypes.byref(desc(i, 1)), ctypes.byref(rd), stream()), 'serl_td3_train_rng')
                e1.record()
                torch.cuda.synchronize()
                assert torch.isfinite(td).all() and (version != 'group' or int(status.abs().max()) == 0)
                if rows_out is not None:
                    rows_out.update({k: rows[k].cpu().numpy() for k in T.ROWS}, td=td.cpu().numpy())
                return e0.elapsed_time(e1)

            serial = a.serial_max is None or K <= a.serial_max
            runs = [(v, f) for v in (('group', 'serial') if serial else ('group',)) for f in ('valu', 'mfma')]
            for v, f in runs:
                run(v, f, min(n, 50))                                    # warm-up
            ms, rows = {k: [] for k in runs}, {k: {} for k in runs}
            for _ in range(a.reps):                                      # alternating: a drift of the clock hits all alike
                for k in runs:
                    ms[k].append(run(k[0], k[1], n, rows[k]))
            r = {'%s_%s_ms' % k: spread(ms[k]) for k in runs}
            r.update({'%s_%s_ms_per_update' % k: spread([x / n for x in ms[k]]) for k in runs})
            r['serial_measured'] = serial
            r['rows_equal'] = bool(all(np.array_equal(rows[k][x], rows[runs[0]][x]) for k in runs for x in rows[k]))
            for f in ('valu', 'mfma'):
                r['%s_learner_updates_per_s' % f] = K * n / (r['group_%s_ms' % f]['median'] * 1e-3)
                if serial:
                    r['%s_serial_over_group_median' % f] = r['serial_%s_ms' % f]['median'] / r['group_%s_ms' % f]['median']
            shape['K%d' % K] = r
            print('H %d K %3d  %s  rows equal: %s' % (H, K, '  '.join('%s/%s %.1f [%.1f .. %.1f] ms' % (k[0], k[1], statistics.median(ms[k]), min(ms[k]),
                  max(ms[k])) for k in runs), r['rows_equal']), flush=True)
            with open(a.out, 'w') as fh:
                json.dump(res, fh, indent=1)
    print(json.dumps(res))


def group_big_main(a, engine, batches):
    import td3_64 as T
    import td3_big as TB
    from serl_amd import _capi, build as hip_build
    L = _capi.lib()
    dev = engine.device
    Ks = [int(k) for k in a.group.split(',')]
    modes = (a.chunks or 'serial,parallel').split(',')
    assert Ks and min(Ks) >= 1 and modes and all(m in ('serial', 'parallel') for m in modes) and all(1 <= B <= 512 for B in batches), (a.group, a.chunks)
    seed, n, Ly = 20261020, a.updates, a.layers
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    regs = [ln.strip() for ln in open(a.kernel_regs)] if a.kernel_regs else None
    GROUP = {'serial': 'serl_td3_train_group_big', 'parallel': 'serl_td3_train_group_wide'}
    SINGLE = {'serial': 'serl_td3_train_big', 'parallel': 'serl_td3_train_wide'}
    SIZE = {'serial': L.serl_td3_big_work_bytes, 'parallel': L.serl_td3_wide_work_bytes}
    res = {'tool': 'bench_td3 --group %s --batch %s --chunks %s' % (a.group, ','.join(str(B) for B in batches), ','.join(modes)),
           'device': torch.cuda.get_device_name(0), 'compute_units': cus, 'source_hash': hip_build.source_hash(), 'layers': Ly, 'updates_per_learner': n,
           'reps': a.reps, 'caps': True, 'policy_update_freq': 2, 'activation': 'tanh', 'seed': seed, 'serial_max': a.serial_max, 'kernel_resources': regs,
           'what': 'ms of ONE launch of K learners (group_<chunks>: %s / %s) and of K back-to-back single-learner generator launches of the '
                   'entries the library had before (single_<chunks>: %s / %s), device events; per_update = ms / updates_per_learner: the time one '
                   'more update of EVERY learner costs.  The K1 single rows are the generator flavours of serl_td3_train_big / _wide at this '
                   'minibatch size.' % (GROUP['serial'], GROUP['parallel'], SINGLE['serial'], SINGLE['parallel']), 'shapes': {}}
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for H in a.hidden:
        for B in batches:
            d = TB.make_case((7, 3, H, Ly, 'tanh', B, 2, 0, 4, 1, 1, 'small'), seed=H)
            cap, G = d['ring'].shape[0], (B + 127) // 128
            shape = res['shapes'].setdefault('H%d_L%d_B%d' % (H, Ly, B), {})
            for K in Ks:
                t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                init = {k: t(np.tile(d[k], (K, 1))) for k in T.ROWS}
                rings = t(np.tile(d['ring'], (K, 1, 1)))
                wb = {m: int(SIZE[m](K, 7, 3, H, Ly, B)) for m in modes}
                wb1 = {m: int(SIZE[m](1, 7, 3, H, Ly, B)) for m in modes}
                work = torch.empty(max(wb.values()) // 4, dtype=torch.float32, device=dev)

                def table(n_):
                    rows = (_capi.Td3LearnerRow * K)()
                    for i in range(K):
                        rows[i] = _capi.Td3LearnerRow(ring=rings[i].data_ptr(), seed=seed, capacity=cap, n_rows=cap, n_updates=n_, iteration0=0, key=i,
                                                      policy_update_freq=2, update_actor_target=1, lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD,
                                                      noise_clip=T.NOISE_CLIP, **T.CAPS)
                    return torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
                tables = {n: table(n), min(n, 20): table(min(n, 20))}

                def run(version, mode, dense, n_, rows_out=None):
                    rows = {k: v.clone() for k, v in init.items()}
                    for k in T.MOMENTS:
                        rows[k] = torch.zeros_like(rows[k.split('_')[0]])
                    steps = torch.zeros(K, 2, dtype=torch.int32, device=dev)
                    td, pg = torch.zeros(K, n_, device=dev), torch.zeros(K, n_, device=dev)
                    status = torch.full((K,), -1, dtype=torch.int32, device=dev)
                    mf = int(dense == 'mfma')

                    def desc(first, k, work_bytes):
                        return _capi.Td3Desc(
                            state_dim=7, action_dim=3, hidden=H, num_layers=Ly, activation=0, n_learners=k, batch=B, n_updates=n_, capacity=cap,
                            policy_update_freq=2, iteration0=0, update_actor_target=1, lr=T.LR, gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD,
                            noise_clip=T.NOISE_CLIP, lambda_s=T.CAPS['lambda_s'], lambda_t=T.CAPS['lambda_t'], eps_sd=T.CAPS['eps_sd'], max_grad_norm=T.MAX_NORM,
                            actor=rows['actor'][first].data_ptr(), actor_target=rows['actor_target'][first].data_ptr(),
                            actor_m=rows['actor_m'][first].data_ptr(), actor_v=rows['actor_v'][first].data_ptr(), actor_stride=rows['actor'].stride(0),
                            critic=rows['critic'][first].data_ptr(), critic_target=rows['critic_target'][first].data_ptr(),
                            critic_m=rows['critic_m'][first].data_ptr(), critic_v=rows['critic_v'][first].data_ptr(),
                            critic_stride=rows['critic'].stride(0), adam_steps=steps[first].data_ptr(), ring=rings[first].data_ptr(),
                            td_loss=td[first].data_ptr(), pg_loss=pg[first].data_ptr(), loss_stride=n_, work=work.data_ptr(), work_bytes=work_bytes)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    if version == 'group':
                        gd = _capi.Td3GroupDesc(rows=tables[n_].data_ptr(), status=status.data_ptr(), dense=mf, caps=1)
                        _capi.check(getattr(L, GROUP[mode])(engine.ctx, ctypes.byref(desc(0, K, wb[mode])), ctypes.byref(gd), stream()), GROUP[mode])
                    else:
                        for i in range(K):
                            rd = _capi.Td3RngDesc(seed=seed, n_rows=cap, learner0=i, dense=mf, caps=1)
                            x = (_capi.Td3WideDesc(rng=ctypes.pointer(rd), status=status[i].data_ptr(), dense=mf) if mode == 'parallel' else
                                 _capi.Td3BigDesc(rng=ctypes.pointer(rd), dense=mf))
                            _capi.check(getattr(L, SINGLE[mode])(engine.ctx, ctypes.byref(desc(i, 1, wb1[mode])), ctypes.byref(x), stream()), SINGLE[mode])
                    e1.record()
                    torch.cuda.synchronize()
                    assert torch.isfinite(td).all() and ((version, mode) == ('single', 'serial') or int(status.abs().max()) == 0), status
                    if rows_out is not None:
                        rows_out.update({k: rows[k].cpu().numpy() for k in T.ROWS}, td=td.cpu().numpy(), pg=pg.cpu().numpy(), steps=steps.cpu().numpy())
                    return e0.elapsed_time(e1)

                single = a.serial_max is None or K <= a.serial_max
                fits = {m: m == 'serial' or K * G <= cus for m in modes}
                runs = [(v, m, f) for m in modes if fits[m] for v in (('group', 'single') if single else ('group',)) for f in ('valu', 'mfma')]
                for k in runs:
                    run(*k, min(n, 20))                                  # warm-up
                ms, rows = {k: [] for k in runs}, {k: {} for k in runs}
                for _ in range(a.reps):                                  # alternating: a drift of the clock hits all alike
                    for k in runs:
                        ms[k].append(run(*k, n, rows[k]))
                r = {'%s_%s_%s_ms' % k: spread(ms[k]) for k in runs}
                r.update({'%s_%s_%s_ms_per_update' % k: spread([x / n for x in ms[k]]) for k in runs})
                r['single_measured'] = single
                r['parallel_measured'] = fits.get('parallel', False)
                r['workgroups'] = {m: K * (G if m == 'parallel' else 1) for m in modes}
                r['rows_equal'] = bool(all(np.array_equal(rows[k][x], rows[runs[0]][x]) for k in runs for x in rows[k]))
                for m, f in ((m, f) for m in modes if fits[m] for f in ('valu', 'mfma')):
                    r['%s_%s_learner_updates_per_s' % (m, f)] = K * n / (r['group_%s_%s_ms' % (m, f)]['median'] * 1e-3)
                    if single:
                        r['%s_%s_single_over_group_median' % (m, f)] = r['single_%s_%s_ms' % (m, f)]['median'] / r['group_%s_%s_ms' % (m, f)]['median']
                if all(fits[m] for m in ('serial', 'parallel') if m in modes) and len(modes) == 2:
                    for f in ('valu', 'mfma'):
                        r['%s_group_serial_over_group_parallel_median' % f] = r['group_serial_%s_ms' % f]['median'] / r['group_parallel_%s_ms' % f]['median']
                shape['K%d' % K] = r
                print('H %d B %d K %3d  %s  rows equal: %s' % (H, B, K, '  '.join('%s/%s/%s %.1f [%.1f .. %.1f] ms' % (k + (statistics.median(ms[k]), min(ms[k]),
                      max(ms[k]))) for k in runs), r['rows_equal']), flush=True)
                with open(a.out, 'w') as fh:
                    json.dump(res, fh, indent=1)
                assert r['rows_equal'], 'the versions of K %d, B %d differ in their final rows' % (K, B)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The bits of the fused TD3 learner, for comparing two builds of the library: every entry point of serl_td3.hip run once on the tests'
cases (tests/td3_64.py, tests/td3_big.py), SHA-256 of every array the call may write.

    python tools/td3_bits.py --out new.json                          # this tree's library
    python tools/td3_bits.py --tree <other checkout> --out old.json  # another checkout's (built there), same cases
    python tools/td3_bits.py --out new.json --against old.json       # ... and compare: exit status 1 if a hash differs

Entries: serl_td3_train, _mfma, _rng (dense 0 / 1), _group (dense 0 / 1, three unlike learners), _big (tables / generator x dense 0 / 1),
serl_td3_rng_fill, _rng_fill_big.  Shapes: 7-72x3-3 at B 86 with CAPS and an actor update every second step, 2-4x0-1 at B 1, 16-128x4-4
at B 128; for _big each of them at B 129 and 300; 13 updates each.  Hashed: the eight rows with one guard learner before and after
and five spare columns behind every row, both loss arrays with two entries past the last update, the Adam steps, and the fill tables
with a guard update before and after.  Only the library's public entry points and the tests' case makers are used, so the same file
runs against any checkout that has them.  A record (profiles/td3_one_body.json), not a test: a deliberate change of a summation order
changes these hashes, and may."""
import argparse, ctypes, hashlib, json, os, sys

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the checkout whose serl_amd and tests are used')
ap.add_argument('--out', required=True)
ap.add_argument('--against', default=None, help='a file an earlier run wrote: compare, exit 1 on a difference')
args = ap.parse_args()
sys.path[:0] = [args.tree, os.path.join(args.tree, 'tests')]

import numpy as np
import torch
import serl_amd
from serl_amd import _capi
import td3_64 as T
import td3_big as TB

N = 13
ACT = {'tanh': 0, 'elu': 1, 'relu': 2}
ROWS = T.ROWS + T.MOMENTS
EXTRA = 5               # spare columns behind every row
SEED = 0x5EED0123456789
#         (S, A, H, L, activation, B, freq, iteration0, n_updates, caps, update_actor_target, rewards)
SMALL = [(7, 3, 72, 3, 'tanh', 86, 2, 0, N, 1, 1, 'small'), (2, 1, 4, 0, 'elu', 1, 1, 3, N, 1, 0, 'small'),
         (16, 4, 128, 4, 'relu', 128, 3, 1, N, 0, 1, 'big')]
BIG = [c[:5] + (B,) + c[6:] for c in SMALL for B in (129, 300)]

L = _capi.lib()
engine = serl_amd.RolloutEngine(0)
dev = engine.device
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes()).hexdigest()


class Buffers:
    """the arrays of K learners of one shape on the device: learner i in row 1 + i of the eight rows, the steps and the losses"""

    def __init__(self, cases, big):
        d0 = self.d0 = cases[0]
        K = self.K = len(cases)
        S, A, B = d0['S'], d0['A'], d0['B']
        self.Pa, self.Pc = len(d0['actor']), len(d0['critic'])
        h = {}
        for k in ROWS:
            P = self.Pa if k.startswith('actor') else self.Pc
            h[k] = np.full((K + 2, P + EXTRA), 7.25, np.float32)
            for i, d in enumerate(cases):
                h[k][1 + i, :P] = d[k] if k in d else 0.0
        h['ring'] = np.stack([d['ring'] for d in cases])
        h['slots'] = np.stack([d['slots'] for d in cases])
        h['tn'] = np.stack([d['tn'] for d in cases])
        h['cn'] = np.stack([d['cn'] if d['caps'] else np.zeros((max(d['n_actor'], 1), B, S), np.float32) for d in cases])
        h['steps'] = np.zeros((K + 2, 2), np.int32)
        h['td'] = np.full((K + 2, N + 2), -3.5, np.float32)
        h['pg'] = np.full((K + 2, N + 2), -3.5, np.float32)
        self.t = {k: torch.from_numpy(v).to(dev) for k, v in h.items()}
        self.wb = int((L.serl_td3_big_work_bytes if big else L.serl_td3_work_bytes)(K, S, A, d0['H'], d0['L'], B))
        assert self.wb > 0
        self.work = torch.full((self.wb // 4,), float('nan'), dtype=torch.float32, device=dev)

    def desc(self, tables=True, per_launch=True):
        d0, t = self.d0, self.t
        p = lambda x, *idx: x[idx].data_ptr()
        kw = dict(state_dim=d0['S'], action_dim=d0['A'], hidden=d0['H'], num_layers=d0['L'], activation=ACT[d0['act']], n_learners=self.K,
                  batch=d0['B'], n_updates=N, max_grad_norm=T.MAX_NORM, adam_steps=p(t['steps'], 1), td_loss=p(t['td'], 1), pg_loss=p(t['pg'], 1),
                  loss_stride=t['td'].stride(0), work=self.work.data_ptr(), work_bytes=self.wb, actor_stride=self.Pa + EXTRA,
                  critic_stride=self.Pc + EXTRA, **{k: p(t[k], 1) for k in ROWS})
        if per_launch:
            kw.update(capacity=t['ring'].shape[1], policy_update_freq=d0['freq'], iteration0=d0['it0'], update_actor_target=int(d0['uat']), lr=T.LR,
                      gamma=T.GAMMA, tau=T.TAU, noise_sd=T.NOISE_SD, noise_clip=T.NOISE_CLIP, ring=p(t['ring']), ring_stride=t['ring'].stride(0), **T.CAPS)
        if tables:
            kw.update(slot_cols=t['slots'].shape[2], slots=p(t['slots']), slots_stride=t['slots'].stride(0), target_noise=p(t['tn']),
                      noise_stride=t['tn'].stride(0), caps_noise=p(t['cn']) if d0['caps'] else None, caps_stride=t['cn'].stride(0))
        return _capi.Td3Desc(**kw)

    def hashes(self):
        torch.cuda.synchronize()
        return {k: sha(self.t[k]) for k in ROWS + ('steps', 'td', 'pg')}


def rng_desc(d, dense, n_rows):
    return _capi.Td3RngDesc(seed=SEED, n_rows=n_rows, learner0=3, dense=dense, caps=int(d['caps']))


def run(name, rc, buf, out):
    assert rc == 0, (name, rc, _capi.last_error() if hasattr(_capi, 'last_error') else '')
    out[name] = buf.hashes()
    print(name, 'ok', flush=True)


def main():
    out = {}
    for c in SMALL:
        d, cid = T.make_case(c), T.case_id(c)
        for entry in ('serl_td3_train', 'serl_td3_train_mfma'):
            b = Buffers([d], False)
            run('%s %s' % (entry, cid), getattr(L, entry)(engine.ctx, ctypes.byref(b.desc()), stream()), b, out)
        for dense in (0, 1):
            b = Buffers([d], False)
            rd = rng_desc(d, dense, T.RING_ROWS - 7)
            run('serl_td3_train_rng dense=%d %s' % (dense, cid),
                L.serl_td3_train_rng(engine.ctx, ctypes.byref(b.desc(tables=False)), ctypes.byref(rd), stream()), b, out)
        # three unlike learners: their own rings, weights, fills, update counts, iterations, seeds, keys and hyper-parameters
        ds = [T.make_case(c, seed=900 + i) for i in range(3)]
        for dense in (0, 1):
            b = Buffers(ds, False)
            table = (_capi.Td3LearnerRow * 3)()
            for i in range(3):
                table[i] = _capi.Td3LearnerRow(ring=b.t['ring'][i].data_ptr(), seed=SEED + 11 * i, capacity=T.RING_ROWS, n_rows=T.RING_ROWS - 9 * i,
                                               n_updates=N - 2 * i, iteration0=c[7] + i, key=5 - i, policy_update_freq=1 + (c[6] + i) % 3,
                                               update_actor_target=int(i != 1), lr=T.LR * (1 + i), gamma=T.GAMMA - 0.01 * i, tau=T.TAU * (1 + i),
                                               noise_sd=T.NOISE_SD + 0.05 * i, noise_clip=T.NOISE_CLIP + 0.1 * i,
                                               lambda_s=T.CAPS['lambda_s'] + 0.1 * i, lambda_t=T.CAPS['lambda_t'] + 0.1 * i,
                                               eps_sd=T.CAPS['eps_sd'] * (1 + i))
            table_d = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
            status = torch.full((3,), -1, dtype=torch.int32, device=dev)
            gd = _capi.Td3GroupDesc(rows=table_d.data_ptr(), status=status.data_ptr(), dense=dense, caps=int(ds[0]['caps']))
            rc = L.serl_td3_train_group(engine.ctx, ctypes.byref(b.desc(tables=False, per_launch=False)), ctypes.byref(gd), stream())
            run('serl_td3_train_group dense=%d %s' % (dense, cid), rc, b, out)
            assert status.cpu().tolist() == [0, 0, 0], status
            out['serl_td3_train_group dense=%d %s' % (dense, cid)]['status'] = sha(status)
    for c in BIG:
        d, cid = TB.make_case(c), T.case_id(c)
        for gen in (False, True):
            for dense in (0, 1):
                b = Buffers([d], True)
                rd = rng_desc(d, dense, TB.RING_ROWS - 7)
                bd = _capi.Td3BigDesc(rng=ctypes.pointer(rd) if gen else None, dense=dense)
                run('serl_td3_train_big %s dense=%d %s' % ('generator' if gen else 'tables', dense, cid),
                    L.serl_td3_train_big(engine.ctx, ctypes.byref(b.desc(tables=not gen)), ctypes.byref(bd), stream()), b, out)
    # the fill tables, one guard update before and after
    for c, entry, rows in [(c, 'serl_td3_rng_fill', T.RING_ROWS) for c in SMALL] + [(c, 'serl_td3_rng_fill_big', TB.RING_ROWS) for c in BIG]:
        S, A, B, freq, it0 = c[0], c[1], c[5], c[6], c[7]
        k = (it0 + N) // freq - it0 // freq
        sl = torch.full((N + 2, B), -9, dtype=torch.int32, device=dev)
        tn = torch.full((N + 2, B, A), 7.25, device=dev)
        cn = torch.full((k + 2, B, S), 7.25, device=dev)
        rd = _capi.Td3RngDesc(seed=SEED, n_rows=rows - 7, learner0=3, dense=0, caps=1)
        rc = getattr(L, entry)(engine.ctx, ctypes.byref(rd), 2, S, A, B, it0, N, freq, sl[1].data_ptr(), tn[1].data_ptr(), cn[1].data_ptr(), stream())
        assert rc == 0, (entry, rc)
        torch.cuda.synchronize()
        out['%s %s' % (entry, T.case_id(c))] = {'slots': sha(sl), 'target_noise': sha(tn), 'caps_noise': sha(cn)}
        print(entry, T.case_id(c), 'ok', flush=True)
    json.dump(out, open(args.out, 'w'), indent=1, sort_keys=True)
    print('%d calls, %d arrays hashed -> %s' % (len(out), sum(len(v) for v in out.values()), args.out))
    if args.against:
        old = json.load(open(args.against))
        diff = sorted(k for k in set(old) | set(out) if old.get(k) != out.get(k))
        print('against %s: %s' % (args.against, 'every hash equal' if not diff else 'DIFFERENT: ' + '; '.join(diff)))
        sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()

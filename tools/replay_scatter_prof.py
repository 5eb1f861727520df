"""Launches of one replay-scatter entry point on the job mix of a default generation (pop 50: 51 stored episodes of 2 001 steps to one
shared ring, 51 own rings and 51 critical rings), for a kernel trace -- one variant per process, 1 warm-up + 5 launches:
    rocprofv3 --kernel-trace --stats -d OUT -o TAG --output-format csv -- python tools/replay_scatter_prof.py <attitude|rows> <S> <A>
`attitude` = serl_replay_scatter (S A must be 7 3), `rows` = serl_replay_scatter_rows.  profiles/replay_scatter_widths.md holds the numbers."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, ROOT)
import numpy as np, torch
import serl_amd
import replay_widths as RW
entry, S, A = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
W = RW.width(S, A)
eng = serl_amd.RolloutEngine(0)
E, T = 51, 2001
rs = np.random.RandomState(0)
st = rs.randn(E, T, W).astype(np.float32)
st[..., W - 1] = rs.rand(E, T) < 0.3
dev = torch.from_numpy(st).to(eng.device)
shared = RW.Ring(1_000_000, W, eng.device)
own = [RW.Ring(8000, W, eng.device) for _ in range(E)]
crit = [RW.Ring(8000, W, eng.device) for _ in range(E)]
items = []
for e in range(E):
    items += [(shared, e, st[e], False), (own[e], e, st[e], False), (crit[e], e, st[e], True)]
jobs = RW.plan_launch(items)
assert len(jobs) == 153
for k in range(6):
    assert RW.launch(eng, dev, S, A, jobs, entry) == 0
for r in [shared] + own[:2] + crit[:2]:
    assert r.guards_intact() and (r.rows().view(np.uint32) == r.mem.view(np.uint32)).all()
print('ok', entry, W)

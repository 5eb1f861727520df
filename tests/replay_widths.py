"""Shared by tests/test_replay_widths_host.py (CPU) and tests/test_gpu_replay_widths.py (GPU): the row widths of the replay rings, the
sequential-add() emulation of tests/support_refs.py generalised to W columns, and the job list of one scatter launch written out from
that emulation's own book-keeping (not from replay.scatter_episodes).  A plain module (not a conftest): nothing here is a fixture."""
import ctypes
import numpy as np
import torch

# (state_dim, action_dim) of the six env configurations (builds.env_dims) and one width no configuration has: 13 floats, odd
CONFIG_DIMS = [(7, 3), (10, 3), (2, 1), (3, 1), (13, 3), (16, 3)]
ODD_DIMS = (4, 2)
DIMS = CONFIG_DIMS + [ODD_DIMS]


def width(S, A):
    return 2 * S + A + 3


def dims_id(d):
    return 'S%dA%d_W%d' % (d[0], d[1], width(*d))


def emulate(cap, W, rows_list, pos=0, size=0, mem=None):
    """n sequential add() calls (base/core/replay_memory.py:21-31) on rows of W floats -> (memory [cap, W], position, size)"""
    mem = np.zeros((cap, W), np.float32) if mem is None else mem
    for rows in rows_list:
        for r in np.asarray(rows, np.float32).reshape(-1, W):
            mem[pos] = r
            pos = (pos + 1) % cap
            size = min(cap, size + 1)
    return mem, pos, size


def make_staged(E, T, S, A, seed, p_cost=0.3):
    """f32 [E, T, W] of random rows, the cost column 0 / 1"""
    rs = np.random.RandomState(seed)
    W = width(S, A)
    st = rs.randn(E, T, W).astype(np.float32)
    st[..., W - 1] = rs.rand(E, T) < p_cost
    return st


def access_width(W, *offsets_in_floats):
    """bytes per access serl_replay_scatter_rows may use (include/serl_amd.h): 16 when W % 4 == 0 and every base is 16 B aligned, 8 when
    W is even and every base 8 B aligned, 4 otherwise; offsets are those of the bases from a 16 B aligned address"""
    if W % 4 == 0 and all(o % 4 == 0 for o in offsets_in_floats):
        return 16
    if W % 2 == 0 and all(o % 2 == 0 for o in offsets_in_floats):
        return 8
    return 4


SENTINEL = np.float32(-12345.5)


class Ring:
    """a device ring of `cap` rows of W floats whose first float sits `offset` floats behind a 16 B aligned address, between two guard
    zones of sentinels; beside it the emulation's memory, position and size"""

    def __init__(self, cap, W, device, offset=0, guard=64):
        self.cap, self.W, self.offset, self.guard = cap, W, offset, guard
        self.store = torch.full((guard + 4 + cap * W + guard,), float(SENTINEL), dtype=torch.float32, device=device)
        assert self.store.data_ptr() % 16 == 0
        self.lo = guard + offset
        self.mem = np.full((cap, W), SENTINEL, np.float32)
        self.pos, self.size = 0, 0
        self.pending = []

    @property
    def ptr(self):
        return self.store.data_ptr() + 4 * self.lo

    def rows(self):
        return self.store[self.lo:self.lo + self.cap * self.W].cpu().numpy().reshape(self.cap, self.W)

    def guards_intact(self):
        s = self.store.cpu().numpy()
        return bool((s[:self.lo] == SENTINEL).all() and (s[self.lo + self.cap * self.W:] == SENTINEL).all())


def taken(rows, cost_only):
    rows = np.asarray(rows)
    return rows[rows[:, -1] != 0] if cost_only else rows


def plan_launch(items):
    """items: [(Ring, episode index, episode rows f32 [n, W], cost_only)] in add() order -> the serl_replay_job fields of one launch,
    [(ring, capacity, position, episode, length, cost_only, skip)]; advances every ring's emulation by sequential add() calls.  skip = the
    ranks of a job that later rows of the same launch overwrite (a row survives iff fewer than `capacity` rows follow it on its ring)."""
    total = {}
    for ring, e, rows, cost_only in items:
        total[id(ring)] = total.get(id(ring), 0) + len(taken(rows, cost_only))
    seen, jobs = {}, []
    for ring, e, rows, cost_only in items:
        tk = taken(rows, cost_only)
        start = seen.get(id(ring), 0)
        seen[id(ring)] = start + len(tk)
        dead = total[id(ring)] - ring.cap - start
        jobs.append((ring.ptr, ring.cap, ring.pos, e, len(rows), int(cost_only), min(max(dead, 0), len(tk))))
        ring.mem, ring.pos, ring.size = emulate(ring.cap, ring.W, [tk], ring.pos, ring.size, ring.mem)
    return jobs


def launch(engine, staged, S, A, jobs, entry='rows'):
    """one launch of serl_replay_scatter_rows (entry='rows') or serl_replay_scatter (entry='attitude') -> its status"""
    from serl_amd import _capi
    arr = (_capi.ReplayJob * max(len(jobs), 1))()
    for k, j in enumerate(jobs):
        arr[k] = _capi.ReplayJob(*[int(v) for v in j])
    buf = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(staged.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(staged.device).cuda_stream)
    T = int(staged.shape[1])
    if entry == 'rows':
        rc = engine.lib.serl_replay_scatter_rows(engine.ctx, staged.data_ptr(), T, int(S), int(A), buf.data_ptr(), len(jobs), stream)
    else:
        rc = engine.lib.serl_replay_scatter(engine.ctx, staged.data_ptr(), T, buf.data_ptr(), len(jobs), stream)
    torch.cuda.synchronize()
    return rc


def job_mix(staged, lens, device, W, offset=0):
    """the rings and items of tests/test_gpu_ga.py::test_replay_scatter_kernel: one shared ring, a ring shorter than one episode, a ring
    and a critical ring per episode -> (rings, items of one round)"""
    E = staged.shape[0]
    shared, small = Ring(1500, W, device, offset), Ring(300, W, device, offset)
    own = [Ring(1000, W, device, offset) for _ in range(E)]
    crit = [Ring(100, W, device, offset) for _ in range(E)]
    items = []
    for e in range(E):
        rows = staged[e, :lens[e]]
        items += [(shared, e, rows, False), (small, e, rows, False), (own[e], e, rows, False), (crit[e], e, rows, True)]
    return [shared, small] + own + crit, items

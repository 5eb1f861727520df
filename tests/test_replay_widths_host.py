"""CPU tests of the replay rings at every row width: DeviceReplay(..., state_dim, action_dim) on the host against the sequential-add()
emulation of tests/replay_widths.py, the defaults that keep the attitude task's 20-float ring what it was, and the additive C export
serl_replay_scatter_rows (header, binding, library) under an unchanged ABI number."""
import os, random, re
import numpy as np
import pytest
import torch
import replay_widths as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ring(cap, S, A):
    from serl_amd.replay import DeviceReplay
    return DeviceReplay(cap, 'cpu', state_dim=S, action_dim=A)


@pytest.mark.parametrize('dims', RW.DIMS, ids=RW.dims_id)
def test_appends_wrap_like_sequential_adds(dims):
    """append_rows (and add, one tuple) with wrap-around and with more rows than the ring holds"""
    S, A = dims
    W = RW.width(S, A)
    rs = np.random.RandomState(W)
    for cap in (1, 7, 64, 257):
        ring = _ring(cap, S, A)
        assert (ring.state_dim, ring.action_dim, ring.row) == (S, A, W) and tuple(ring.rows.shape) == (cap, W)
        mem, pos, size = None, 0, 0
        for n in (0, 1, 5, cap - 1, cap, cap + 3, 2 * cap + 1, 33):
            rows = rs.randn(n, W).astype(np.float32)
            ring.append_rows(torch.from_numpy(rows))
            mem, pos, size = RW.emulate(cap, W, [rows], pos, size, mem)
            assert (ring.position, len(ring)) == (pos, size)
            np.testing.assert_array_equal(ring.rows.numpy()[:size], mem[:size])
        r = rs.randn(W).astype(np.float32)
        ring.add(r[:S], r[S:S + A], r[S + A:2 * S + A], r[2 * S + A], r[2 * S + A + 1], r[2 * S + A + 2])
        mem, pos, size = RW.emulate(cap, W, [r[None]], pos, size, mem)
        assert (ring.position, len(ring)) == (pos, size)
        np.testing.assert_array_equal(ring.rows.numpy()[:size], mem[:size])


def _list_latest(mem, pos, cap, latest):
    """ReplayMemory.get_latest (base/core/replay_memory.py:42-56) on a python list"""
    if cap < latest:
        return mem[pos:] + mem[:pos], 'capacity < latest'
    if len(mem) < cap:
        return mem[-latest:], 'not full'
    if pos >= latest:
        return mem[:pos][-latest:], 'full, position >= latest'
    return mem[-latest + pos:] + mem[:pos], 'full, position < latest'


@pytest.mark.parametrize('dims', RW.DIMS, ids=RW.dims_id)
def test_latest_views_and_ring_to_ring_copies(dims):
    """get_latest in the four branches of latest_slots, add_content_of, add_latest_from: against a python list filled like the
    reference's ReplayMemory.add fills it"""
    S, A = dims
    W = RW.width(S, A)
    rs = np.random.RandomState(100 + W)
    branches = set()
    for cap, n, latest in ((50, 30, 10), (50, 80, 20), (50, 60, 20), (50, 80, 60), (50, 50, 50), (50, 3, 10)):
        ring, mem, pos = _ring(cap, S, A), [], 0
        rows = rs.randn(n, W).astype(np.float32)
        ring.append_rows(torch.from_numpy(rows))
        for r in rows:
            if len(mem) < cap:
                mem.append(None)
            mem[pos] = r
            pos = (pos + 1) % cap
        want, branch = _list_latest(mem, pos, cap, latest)
        branches.add(branch)
        np.testing.assert_array_equal(ring.get_latest(latest).numpy(), np.stack(want))
        for dcap in (20, 200):
            d1, d2 = _ring(dcap, S, A), _ring(dcap, S, A)
            pre = rs.randn(7, W).astype(np.float32)
            d1.append_rows(torch.from_numpy(pre)); d2.append_rows(torch.from_numpy(pre))
            d1.add_content_of(ring)
            m1, p1, s1 = RW.emulate(dcap, W, [pre, np.stack(_list_latest(mem, pos, cap, dcap)[0])])
            assert (d1.position, len(d1)) == (p1, s1)
            np.testing.assert_array_equal(d1.rows.numpy()[:s1], m1[:s1])
            d2.add_latest_from(ring, latest)
            m2, p2, s2 = RW.emulate(dcap, W, [pre, np.stack(want)])
            assert (d2.position, len(d2)) == (p2, s2)
            np.testing.assert_array_equal(d2.rows.numpy()[:s2], m2[:s2])
    assert branches == {'capacity < latest', 'not full', 'full, position >= latest', 'full, position < latest'}


@pytest.mark.parametrize('dims', RW.DIMS, ids=RW.dims_id)
def test_shuffle_and_samples_consume_the_generator_like_a_width_20_ring(dims):
    """shuffle with a seeded `random` permutes the rows like random.shuffle permutes the list; sample / sample_from_latest return
    [B, S], [B, A], [B, S], [B, 1], [B, 1] of the rows the same draws pick, and leave python's generator where the same calls on a
    width-20 ring of the same fill leave it"""
    from serl_amd.replay import DeviceReplay
    S, A = dims
    W = RW.width(S, A)
    rs = np.random.RandomState(200 + W)
    cap, n, B = 90, 130, 16
    rows = rs.randn(n, W).astype(np.float32)
    ring, ring20 = _ring(cap, S, A), DeviceReplay(cap, 'cpu')
    ring.append_rows(torch.from_numpy(rows))
    ring20.append_rows(torch.from_numpy(rs.randn(n, 20).astype(np.float32)))
    mem, pos, size = RW.emulate(cap, W, [rows])

    def calls(r):
        r.shuffle(random)
        return r.sample(B, random), r.sample_from_latest(B, 40, random)
    random.seed(5)
    got, got_latest = calls(ring)
    after = random.random()
    random.seed(5)
    calls(ring20)
    assert random.random() == after
    random.seed(5)
    lst = [mem[k] for k in range(size)]
    random.shuffle(lst)
    np.testing.assert_array_equal(ring.rows.numpy()[:size], np.stack(lst))
    pick = np.stack(random.sample(lst, B))
    latest = np.stack(_list_latest(lst, pos, cap, 40)[0])
    pick_latest = latest[random.sample(range(len(latest)), B)]
    for out, want in ((got, pick), (got_latest, pick_latest)):
        assert [tuple(t.shape) for t in out] == [(B, S), (B, A), (B, S), (B, 1), (B, 1)]
        np.testing.assert_array_equal(torch.cat(out, 1).numpy(), want[:, :W - 1])


def test_defaults_are_the_attitude_ring():
    from serl_amd import replay
    from serl_amd.replay import DeviceReplay
    ring = DeviceReplay(11, 'cpu')
    assert tuple(ring.rows.shape) == (11, 20) and replay.ROW == 20 and (ring.state_dim, ring.action_dim, ring.row) == (7, 3, 20)
    rows = torch.arange(60, dtype=torch.float32).reshape(3, 20)
    for out in (DeviceReplay.split(rows), ring.split(rows)):            # the static call of ga.py and the tests, and the bound one
        want = (rows[:, 0:7], rows[:, 7:10], rows[:, 10:17], rows[:, 17:18], rows[:, 18:19])
        assert len(out) == 5
        for a, b in zip(out, want):
            assert torch.equal(a, b)
    full = DeviceReplay(4, 'cpu', state_dim=13, action_dim=3)
    rows32 = torch.arange(64, dtype=torch.float32).reshape(2, 32)
    s, a, s2, r, d = full.split(rows32)
    assert torch.equal(s, rows32[:, :13]) and torch.equal(a, rows32[:, 13:16]) and torch.equal(s2, rows32[:, 16:29])
    assert torch.equal(r, rows32[:, 29:30]) and torch.equal(d, rows32[:, 30:31])


def test_mismatched_widths_are_refused():
    from serl_amd import replay, generation
    from serl_amd.replay import DeviceReplay
    att, full, sym = DeviceReplay(8, 'cpu'), DeviceReplay(8, 'cpu', state_dim=13, action_dim=3), DeviceReplay(8, 'cpu', state_dim=2, action_dim=1)
    # 2 S + A + 3 = 20 as well, but not the attitude task's cut
    other20 = DeviceReplay(8, 'cpu', state_dim=8, action_dim=1)
    att.append_rows(torch.zeros(3, 20)); full.append_rows(torch.zeros(3, 32))
    with pytest.raises(ValueError):
        full.append_rows(torch.zeros(2, 20))
    with pytest.raises(ValueError):
        att.append_rows(torch.zeros(2, 32))
    with pytest.raises(ValueError):
        sym.add(np.zeros(7), np.zeros(3), np.zeros(7), 0.0, 0.0)
    with pytest.raises(ValueError):
        full.add_content_of(att)
    with pytest.raises(ValueError):
        att.add_latest_from(full, 2)
    with pytest.raises(ValueError):
        other20.add_content_of(att)
    with pytest.raises(ValueError):
        DeviceReplay.split(torch.zeros(2, 32))
    with pytest.raises(ValueError):
        full.split(torch.zeros(2, 20))
    assert (len(att), len(full), len(sym), len(other20)) == (3, 3, 0, 0)
    # the buffer side of a generation: rings of other dims than the call's are named, nothing is stored
    import types
    agent = types.SimpleNamespace(buffer=att, critical_buffer=DeviceReplay(8, 'cpu'))
    counters = {}
    with pytest.raises(ValueError, match=r'state_dim 7, action_dim 3 .* state_dim 13, action_dim 3'):
        replay.store_episodes(None, torch.zeros(1, 4, 32), [(agent, 0, 4, 0)], None, counters, state_dim=13, action_dim=3)
    with pytest.raises(ValueError):
        replay.scatter_episodes(None, torch.zeros(1, 4, 32), [(att, 0, 4, False, 4)])
    with pytest.raises(ValueError):
        replay.scatter_episodes(None, torch.zeros(1, 4, 32), [(full, 0, 4, False, 4), (att, 0, 4, False, 4)])
    with pytest.raises(ValueError):
        generation.store_transitions(torch.zeros(4, 32), agent)
    assert len(att) == 3 and att.position == 3 and full.position == 3


def test_store_transitions_feeds_list_buffers_of_any_width():
    """generation.store_transitions with host rows: the cost column is the last one of the row whatever its width"""
    import types
    from serl_amd import generation

    class Buf(list):
        def add(self, *t):
            self.append(t)
    S, A = 13, 3
    rows = RW.make_staged(1, 9, S, A, seed=1, p_cost=0.5)[0]
    agent = types.SimpleNamespace(buffer=Buf(), critical_buffer=Buf())
    shared, counters = Buf(), {}
    generation.store_transitions(rows, agent, shared, counters, state_dim=S, action_dim=A)
    nc = int(rows[:, -1].sum())
    assert 0 < nc < 9 and (len(shared), len(agent.buffer), len(agent.critical_buffer)) == (9, 9, nc)
    assert counters == {'num_frames': 9, 'gen_frames': 9, 'num_episodes': 1}
    as_rows = lambda buf: np.stack([np.concatenate([np.ravel(np.asarray(x, np.float32)) for x in t]) for t in buf])
    np.testing.assert_array_equal(as_rows(shared), rows[:, :-1])
    np.testing.assert_array_equal(as_rows(agent.critical_buffer), rows[rows[:, -1] != 0][:, :-1])
    assert shared[0][0].shape == (S,) and shared[0][1].shape == (A,)


def test_scatter_rows_is_an_additive_export():
    """declared in the header, listed in the binding, exported by the built library -- and the ABI number is still 9"""
    from serl_amd import _capi
    header = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    decl = re.search(r'int\s+serl_replay_scatter_rows\s*\(([^)]*)\)\s*;', header)
    assert decl, 'include/serl_amd.h does not declare serl_replay_scatter_rows'
    args = re.sub(r'/\*.*?\*/', '', decl.group(1))
    assert [re.sub(r'\s+', ' ', a).strip() for a in args.split(',')] == [
        'serl_ctx *ctx', 'const float *staged', 'int64_t rows_per_episode', 'int32_t state_dim', 'int32_t action_dim',
        'const serl_replay_job *jobs', 'int32_t n_jobs', 'void *stream']
    assert re.search(r'#define\s+SERL_ABI_VERSION\s+9\b', header) and _capi.ABI_VERSION == 9
    assert 'serl_replay_scatter_rows' in _capi.EXPORTS and 'serl_replay_scatter' in _capi.EXPORTS
    L = _capi.lib()
    assert L.serl_abi_version() == 9
    assert hasattr(L, 'serl_replay_scatter_rows') and len(L.serl_replay_scatter_rows.argtypes) == 8

"""CPU tests of tests/support_refs.py: every reference the GPU tests of the SSNE-edit, replay-scatter and smoothness kernels compare with
is itself compared with an independent counterpart and with the goldens the reference project produced."""
import random, re
import numpy as np
import torch

import support_refs as R


# ---- smoothness ---------------------------------------------------------------------------------------------------------------------
def test_longdouble_dft_against_fft_and_oracle():
    """the direct longdouble DFT against numpy's FFT (the formulation of tests/test_gpu_ga.py) and against oracle/smoothness.py, over the
    length classes of the kernel and three values of dt; they agree to a few ulp of float64"""
    from oracle.smoothness import calc_smoothness
    y = R.traces(2, 2001, seed=3)
    for N in (4, 5, 6, 7, 8, 64, 513, 514, 517, 1029, 2001):
        for dt in (0.01, 0.02, 0.005):
            P = R.dft_power(y[N % 2, :N])
            a = R.smoothness_from_power(P, N, dt)
            np.testing.assert_allclose(a, R.smoothness_fft(y[N % 2, :N], dt), rtol=1e-13, err_msg='N %d dt %g' % (N, dt))
            np.testing.assert_allclose(a, calc_smoothness(y[N % 2, :N], dt), rtol=1e-13, err_msg='N %d dt %g' % (N, dt))
    for N in (0, 1, 2, 3):
        assert R.smoothness_dft(y[0, :N]) == 0.0 and R.smoothness_fft(y[0, :N]) == 0.0


def test_smoothness_references_against_the_reference_goldens(golden):
    """the smoothness the reference itself computed for shipped actors (pop_*.npz, td3.npz) from the action traces it recorded (traj.npz)"""
    tr = golden('traj')
    for key, gold, i, ref in (('serl50_18', 'pop_serl50', 18, R.smoothness_dft), ('serl10_0', 'pop_serl10', 0, R.smoothness_fft),
                              ('td3_0', 'td3', 0, R.smoothness_fft)):
        want = np.atleast_1d(golden(gold)['smoothness'])[i]
        np.testing.assert_allclose(ref(tr[key + '_actions']), want, rtol=1e-11, err_msg=key)


def test_closed_forms_of_the_known_signals():
    """tone, impulse and exact-zero signals: the closed forms the GPU test asserts hold for the longdouble DFT"""
    N = 2001
    for k in (1, 256, 257, N // 2 - 1):
        for dt in (0.01, 0.02):
            np.testing.assert_allclose(R.smoothness_dft(R.tone(N, k), dt), R.tone_value(N, k, dt), rtol=1e-12)
    for N, at in ((2001, 0), (2001, 2000), (516, 515)):
        y = np.zeros((N, 3)); y[at, 1] = 0.25
        np.testing.assert_allclose(R.smoothness_dft(y), R.impulse_value(N, 0.01, 0.25), rtol=1e-12)
    assert abs(R.smoothness_dft(np.full((2001, 3), 0.7))) < 1e-14
    assert abs(R.smoothness_dft(np.tile((0.7 * (-1.0) ** np.arange(2000))[:, None], (1, 3)))) < 1e-14


# ---- replay -------------------------------------------------------------------------------------------------------------------------
def test_replay_emulation_against_device_replay_on_cpu():
    """the sequential add() emulation against DeviceReplay('cpu').append_rows, which test_ga_host.py pins to the reference's ReplayMemory"""
    from serl_amd.replay import DeviceReplay
    rs = np.random.RandomState(4)
    for cap in (1, 7, 63, 64, 257, 1000):
        ring = DeviceReplay(cap, 'cpu')
        mem, pos, size = np.zeros((cap, R.ROW), np.uint32), 0, 0
        for n in (0, 1, 5, cap - 1, cap, cap + 3, 2 * cap + 1, 33):
            rows = rs.randn(n, R.ROW).astype(np.float32)
            ring.append_rows(torch.from_numpy(rows))
            mem, pos, size = R.replay_emulate(cap, [rows.view(np.uint32)], pos, size, mem)
            assert (ring.position, len(ring)) == (pos, size)
            np.testing.assert_array_equal(ring.rows.numpy().view(np.uint32)[:size], mem[:size])


def test_scatter_job_reference_equals_sequential_adds():
    """with skip = the ranks a ring cannot hold, the header's slot rule leaves what sequential add() calls leave; flags: -0.0 is not taken, NaN is"""
    st = R.fuzz_staged(4, 300, seed=2)
    flags = st[2, :, 19].view(np.float32)
    assert np.isnan(flags).any() and (st[2, :, 19] == 0x80000000).any()
    with np.errstate(invalid='ignore'):
        assert len(R.taken_rows(st[2], True)) == int(np.sum(~(flags == 0.0)))
    assert not (R.taken_rows(st[2], True)[:, 19] == 0x80000000).any()
    for cap in (1, 7, 100, 1000):
        for e, cost in ((1, False), (2, True), (3, True), (0, True)):
            tk = R.taken_rows(st[e], cost)
            ring = R.sentinel_u32(cap * R.ROW).reshape(cap, R.ROW)
            want, _, _ = R.replay_emulate(cap, [tk], 3 % cap, 0, ring.copy())
            assert R.scatter_job_ref(ring, cap, 3 % cap, st[e], cost, max(0, len(tk) - cap)) == len(tk)
            np.testing.assert_array_equal(ring, want)


def test_fuzz_plan_covers_every_class():
    staged, caps, launches = R.fuzz_plan()
    assert len(launches) <= 5 and sum(len(ids) for ids, _ in launches) >= 200 and sum(len(j) for j in launches[0][1]) >= 500
    seen, pos = set(), [0] * len(caps)
    for ids, lists in launches:
        for r, jobs in zip(ids, lists):
            seen |= R.fuzz_classes(staged, caps[r], pos[r], jobs)
            pos[r] = (pos[r] + sum(len(R.taken_rows(staged[e, :n], c)) for e, n, c in jobs)) % caps[r]
    assert not [c for c in R.FUZZ_REQUIRED + ['len_%d' % R.FUZZ_T] if c not in seen]


# ---- SSNE edits -----------------------------------------------------------------------------------------------------------------------
def _spec():
    import serl_amd
    return serl_amd.NetSpec(7, 3, 32, 3, 'tanh')


def test_mutate_reference_against_the_reference_golden(golden):
    """mutate_ref on the plans of serl_amd.ga.plan_mutation == what the reference's own mutate_inplace left (ga_ops.npz), bit for bit"""
    from serl_amd import ga
    g = golden('ga_ops')
    keys = [k for k in g.files if k.startswith('mut_seed')]
    assert keys
    for key in keys:
        seed = int(re.match(r'mut_seed(\d+)', key).group(1))
        random.seed(seed); np.random.seed(seed)
        got = R.mutate_ref(g['base'][2], *ga.plan_mutation(_spec(), 0.05))
        assert len(R.same_f32(got, g[key])) == 0, key


def test_clamp_reference_is_torch_clamp():
    vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, 999999.9, 1e6, 1000000.06, -1e6, -1000000.06, 3e38, -3e38, np.inf, -np.inf, np.nan],
                    np.float32)
    want = torch.clamp(torch.from_numpy(vals), -1000000, 1000000).numpy()
    got = np.array([R.clamp_ref(v) for v in vals], np.float32)
    assert len(R.same_f32(got, want)) == 0
    assert np.isnan(got[-1]) and got[-3] == 1e6 and got[-2] == -1e6
    np.testing.assert_array_equal(got[:2].view(np.uint32), vals[:2].view(np.uint32))          # the sign of a zero survives


def test_crossover_reference_against_the_reference_golden(golden):
    from serl_amd import ga
    import serl_amd
    gx = golden('ga_cross_tiny')
    S_, A_, H_, L_ = (int(v) for v in gx['net'])
    tiny = serl_amd.NetSpec(S_, A_, H_, L_, 'tanh')
    for seed in gx['seeds']:
        random.seed(int(seed))
        ops = ga.plan_crossover(tiny)
        w = np.stack([gx['parents'][0], gx['parents'][1], gx['parents'][0]])
        out = R.crossover_ref(w, 0, 1, ops)
        np.testing.assert_array_equal(out[0], gx['seed%d_a' % seed])
        np.testing.assert_array_equal(out[1], gx['seed%d_b' % seed])
        np.testing.assert_array_equal(out[2], gx['parents'][0])
    # later ops see earlier ones, in both directions
    w = np.arange(20, dtype=np.float32).reshape(2, 10)
    out = R.crossover_ref(w, 0, 1, [(0, 4, 1), (2, 4, 0)])          # a -> b on [0, 4), then b -> a on [2, 6): columns 2, 3 of a come back unchanged
    np.testing.assert_array_equal(out[0], [0, 1, 2, 3, 14, 15, 6, 7, 8, 9])
    np.testing.assert_array_equal(out[1], [0, 1, 2, 3, 14, 15, 16, 17, 18, 19])


def test_clone_and_scaled_perturb_references():
    w = R.sentinel_f32((6, 9))
    out = R.clone_ref(w, 7, [0, 0, 2], [3, 4, 2])
    np.testing.assert_array_equal(out[3, :7], w[0, :7]); np.testing.assert_array_equal(out[4, :7], w[0, :7])
    np.testing.assert_array_equal(out[:, 7:], w[:, 7:]); np.testing.assert_array_equal(out[[0, 1, 2, 5]], w[[0, 1, 2, 5]])
    row = np.array([1, 2, 3, 4, 5, 6], np.float32)
    out = R.scaled_perturb_ref(row, [(1, 2), (5, 1)], [0.3, 0.0, -0.5], [0.01, 2.0, 3.0])
    want = row.copy()
    want[1] = np.float32(2) + np.float32(0.3) / np.float32(0.01); want[5] = np.float32(6) + np.float32(-0.5) / np.float32(3)
    np.testing.assert_array_equal(out, want)
    assert out.dtype == np.float32

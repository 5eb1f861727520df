"""GPU tests of the device kernels a training generation calls besides the rollout -- serl_ga_clone / crossover / mutate /
scaled_perturb, serl_replay_scatter, serl_smoothness -- at their edges, through the C ABI (engine.lib, engine.ctx, ctypes), against the
plain references of tests/support_refs.py (which tests/test_support_refs.py pins on the CPU).

Copied or edited f32 data is compared BIT FOR BIT (uint32 views; a NaN the operation itself produces may carry either sign).  Every
output or in/out buffer starts as a pattern in which each cell differs, and the whole buffer is compared afterwards: other members'
rows, the columns between param_count and stride, ring slots not written, work / out beyond the batch.

serl_ga_clone: the pairs of one call run in parallel, so a destination that is another pair's source has no defined result
(serl_amd.ssne passes one pair per call); that is documented in include/serl_amd.h and not tested.  Arguments whose wrong handling
would be a memory fault (|length| > max_len, a misaligned ring, a NULL device pointer that is not refused on the host) are not tested.

Measured on an MI355X (worst over every smoothness case of this file):
  against the longdouble DFT / numpy FFT:  |got - want| / |want| = 9.2e-15 (a pure tone), 1.4e-15 on the actor-like traces; 1e-9 allowed
  exact-zero signals:                      |got| / |numpy-FFT value of the same trace| = 3.95 (Nyquist alternation, N = 8 000; constants
                                           up to 3.1); the factor allowed is 16
Batch limits: 65 536 and 65 537 episodes / clone pairs in one call are computed in full (include/serl_amd.h)."""
import ctypes
import numpy as np
import pytest
import torch

import support_refs as R

pytestmark = pytest.mark.gpu
VP = ctypes.c_void_p


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _u32(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _ptr(t):
    return VP(t.data_ptr()) if t is not None else None


def _sync_stream():
    torch.cuda.synchronize()
    return VP(torch.cuda.current_stream().cuda_stream)


def _assert_bits(got, want, what):
    bad = R.same_f32(got, want)
    assert len(bad) == 0, '%s: %d cells differ, first at %s: got %r want %r' % (
        what, len(bad), bad[:4], np.asarray(got).reshape(-1)[bad[:4]], np.asarray(want).reshape(-1)[bad[:4]])


# =====================================================================================================================================
# SSNE edits
# =====================================================================================================================================
def _param_counts():
    import actor_shapes as X
    return [X.spec_of(X._shape(H, 3)).param_count for H in (4, 32, 128)]


def test_clone_shapes_strides_and_pair_counts(engine):
    """serl_ga_clone over param_count 1 / 255 / 256 / 257 and three actor shapes, stride P and P + 5, 1 / 7 / 50 pairs with several
    destinations per source and a src == dst pair; n = 0 writes nothing"""
    lib, M = engine.lib, 64
    for P in [1, 255, 256, 257] + _param_counts():
        for stride in (P, P + 5):
            w0 = R.sentinel_f32((M, stride))
            for n in (1, 7, 50):
                src = [i % 6 for i in range(n)]                   # sources 0 .. 5, each to several destinations
                dst = [10 + i for i in range(n)]
                if n > 1:
                    src[3], dst[3] = 5, 5                         # src == dst (row 5 is also a source of other pairs: a copy onto itself changes nothing)
                w = _dev(engine, w0)
                s, d = _dev(engine, np.asarray(src, np.int32)), _dev(engine, np.asarray(dst, np.int32))
                rc = lib.serl_ga_clone(engine.ctx, _ptr(w), stride, P, _ptr(s), _ptr(d), n, _sync_stream())
                torch.cuda.synchronize()
                assert rc == 0
                np.testing.assert_array_equal(_u32(w), R.clone_ref(w0, P, src, dst).view(np.uint32), err_msg='P %d stride %d n %d' % (P, stride, n))
            w = _dev(engine, w0)
            assert lib.serl_ga_clone(engine.ctx, _ptr(w), stride, P, _ptr(s), _ptr(d), 0, _sync_stream()) == 0
            torch.cuda.synchronize()
            np.testing.assert_array_equal(_u32(w), w0.view(np.uint32))


def _crossover(engine, w0, stride, ma, mb, ops, what):
    w = _dev(engine, w0)
    o = _dev(engine, np.asarray(ops, np.int32).reshape(-1, 3))
    rc = engine.lib.serl_ga_crossover(engine.ctx, _ptr(w), stride, ma, mb, _ptr(o), len(ops), _sync_stream())
    torch.cuda.synchronize()
    assert rc == 0
    np.testing.assert_array_equal(_u32(w), R.crossover_ref(w0, ma, mb, ops).view(np.uint32), err_msg=what)


def test_crossover_ops_apply_in_order(engine):
    """serl_ga_crossover: overlapping ranges in both directions (a -> b then b -> a and the reverse, same and shifted ranges), lengths
    1 / 255 / 256 / 257 / 1000, members 0 and 63 of 64, ma == mb, 0 / 1 / 600 ops"""
    P = 3000
    stride = P + 3
    w0 = R.sentinel_f32((64, stride))
    ops = [(10, 257, 1), (10, 257, 0),                  # a -> b, then b -> a over the same range: a unchanged, b = a
           (300, 256, 0), (300, 256, 1),                # the reverse: b unchanged, a = b
           (600, 1000, 1), (728, 1000, 0),              # shifted: [728, 1600) of a comes back from b, where another wavefront put it
           (1700, 1000, 0), (1828, 1000, 1),
           (0, 1, 0), (5, 255, 1), (2744, 256, 0), (2999, 1, 1)]
    for ma, mb in ((0, 63), (63, 0), (7, 8)):
        _crossover(engine, w0, stride, ma, mb, ops, 'members %d %d' % (ma, mb))
    for ln in (1, 255, 256, 257, 1000):
        _crossover(engine, w0, stride, 0, 63, [(3, ln, 1)], 'one op of length %d' % ln)
        _crossover(engine, w0, stride, 0, 63, [(3, ln, 0)], 'one op of length %d' % ln)
    _crossover(engine, w0, stride, 5, 5, ops, 'ma == mb')          # copies of a row onto itself
    w = _dev(engine, w0)
    assert engine.lib.serl_ga_crossover(engine.ctx, _ptr(w), stride, 0, 1, None, 0, _sync_stream()) == 0          # n_ops = 0: ops may be NULL
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(w), w0.view(np.uint32))


def test_crossover_600_ops_each_reading_what_the_one_before_wrote(engine):
    """300 pairs of ops: the first copies 1024 columns one way, the second copies a range back that starts in the LAST 128 columns of
    the first -- written there by wavefronts 2 and 3 in their last pass, read here by wavefronts 0 and 1 in their first.  If the second
    op did not wait for the first, those columns would come back with the other member's old values."""
    n_pairs, pitch = 300, 1500
    P = n_pairs * pitch
    stride = P + 3
    w0 = R.sentinel_f32((3, stride))
    ops = []
    for j in range(n_pairs):
        d = j % 2
        ops += [(j * pitch, 1024, 1 - d), (j * pitch + 896, 512, d)]
    assert len(ops) == 600
    _crossover(engine, w0, stride, 0, 2, ops, '600 ops')


def _mutate(engine, w0, stride, member, idx, kind, z, strength):
    w = _dev(engine, w0)
    a, b = _dev(engine, np.asarray(idx, np.int32)), _dev(engine, np.asarray(kind, np.int32))
    c, d = _dev(engine, np.asarray(z, np.float32)), _dev(engine, np.asarray(strength, np.float32))
    rc = engine.lib.serl_ga_mutate(engine.ctx, _ptr(w), stride, member, _ptr(a), _ptr(b), _ptr(c), _ptr(d), len(idx), _sync_stream())
    torch.cuda.synchronize()
    assert rc == 0
    return w.cpu().numpy()


def test_mutate_special_values_keep_torch_clamp_semantics(engine):
    """serl_ga_mutate on hand-built edits: one index edited three times (kinds 0, 1, 0), values driven past +-1e6, weights that are
    +-0, denormal, +-inf or NaN, z = +-inf or NaN.  Expected: f32 arithmetic in order, then torch.clamp -- a NaN stays a NaN (a diverged
    actor must not come back as a finite one)."""
    P, stride, member = 3715, 3720, 3
    inf, nan = np.inf, np.nan
    w0 = R.sentinel_f32((8, stride))
    special = {20: 0.0, 21: -0.0, 22: 1e-45, 23: -1e-40, 24: inf, 25: -inf, 26: inf, 27: -inf, 28: nan, 29: 0.5, 30: 0.5, 31: 0.0,
               32: 9e5, 33: -9e5, 34: 0.25, 35: 0.25, 36: 0.75, 37: 0.75, 38: nan, 39: 999999.0, 40: -999999.0, 41: 1e-45}
    for i, v in special.items():
        w0[member, i] = v
    edits = [(10, 0, 0.7, 0.05), (10, 1, -0.3, 0.0), (10, 0, 1.5, 0.5),              # the same weight three times
             (20, 0, 1.0, 0.05), (21, 0, 1.0, 0.05), (22, 0, 1.0, 0.5), (23, 0, -2.0, 0.5),
             (24, 0, 1.0, 0.05), (25, 0, 1.0, 0.05),                                  # inf + inf -> clamped to +-1e6
             (26, 0, -1.0, 0.05), (27, 0, -1.0, 0.05),                                # inf - inf -> NaN, stays NaN
             (28, 0, 1.0, 0.05),                                                      # a NaN weight stays NaN ...
             (29, 0, nan, 0.05), (30, 1, nan, 0.0),                                   # ... and so does a NaN draw
             (31, 0, inf, 0.05),                                                      # inf * 0 -> NaN
             (32, 0, 1.0, 10.0), (33, 0, 1.0, 10.0),                                  # 9e5 + 9e6 -> +1e6, -9e5 - 9e6 -> -1e6
             (34, 1, 2e6, 0.0), (35, 1, -3e6, 0.0), (36, 1, inf, 0.0), (37, 1, -inf, 0.0),
             (38, 1, 0.125, 0.0),                                                     # a reset heals a NaN weight
             (39, 0, 1.0, 0.05), (40, 0, 1.0, 0.05),                                  # just past the clamp
             (41, 1, -0.0, 0.0), (P - 1, 0, 0.5, 0.05), (0, 0, -0.5, 0.05)]
    idx, kind, z, st = zip(*edits)
    got = _mutate(engine, w0, stride, member, idx, kind, z, st)
    want = w0.copy()
    want[member] = R.mutate_ref(w0[member], idx, kind, z, st)
    for i in (26, 27, 28, 29, 30, 31):
        assert np.isnan(want[member, i]), i
    assert want[member, 24] == 1e6 and want[member, 25] == -1e6 and want[member, 36] == 1e6 and want[member, 37] == -1e6
    assert want[member, 32] == 1e6 and want[member, 33] == -1e6 and want[member, 38] == 0.125
    _assert_bits(got, want, 'special values')
    # n = 1
    got = _mutate(engine, w0, stride, 0, [7], [0], [0.3], [0.05])
    want = w0.copy(); want[0] = R.mutate_ref(w0[0], [7], [0], [0.3], [0.05])
    _assert_bits(got, want, 'n = 1')


def test_mutate_5000_edits_in_order(engine):
    """5 000 random edits of 3 715 weights (most weights hit more than once, kinds mixed): bit-equal to the sequential f32 loop"""
    P, stride, member, n = 3715, 3715, 1, 5000
    rs = np.random.RandomState(8)
    w0 = R.sentinel_f32((3, stride))
    w0[member] = (rs.randn(P) * 0.3).astype(np.float32)
    idx = rs.randint(0, P, n)
    kind = (rs.rand(n) < 0.1).astype(np.int32)
    z = rs.randn(n).astype(np.float32)
    st = np.where(rs.rand(n) < 0.1, 0.5, 0.05).astype(np.float32)
    assert len(np.unique(idx)) < n - 1000
    got = _mutate(engine, w0, stride, member, idx, kind, z, st)
    want = w0.copy(); want[member] = R.mutate_ref(w0[member], idx, kind, z, st)
    assert (want[member] != w0[member]).sum() > 2000
    _assert_bits(got, want, '5000 edits')


def _perturb(engine, w0, stride, member, segs, delta, scaling, what):
    w = _dev(engine, w0)
    so, sl = _dev(engine, np.asarray([s[0] for s in segs], np.int32)), _dev(engine, np.asarray([s[1] for s in segs], np.int32))
    dl, sc = _dev(engine, delta), _dev(engine, scaling)
    rc = engine.lib.serl_ga_scaled_perturb(engine.ctx, _ptr(w), stride, member, _ptr(so), _ptr(sl), len(segs), _ptr(dl), _ptr(sc), _sync_stream())
    torch.cuda.synchronize()
    assert rc == 0
    want = w0.copy()
    want[member] = R.scaled_perturb_ref(w0[member], segs, delta, scaling)
    assert (want[member] != w0[member]).sum() > 0.85 * len(delta) - 2
    _assert_bits(w.cpu().numpy(), want, what)


def _delta_scaling(n, seed):
    rs = np.random.RandomState(seed)
    delta = (rs.randn(n) * 0.01).astype(np.float32)
    scaling = rs.uniform(0.01, 2.0, n).astype(np.float32)
    scaling[::7] = np.float32(0.01)                 # the floor serl_ga_sensitivity applies
    delta[::11] = 0.0
    delta[5::211] = -0.0
    return delta, scaling


def test_scaled_perturb_is_the_f32_quotient_and_sum(engine):
    """serl_ga_scaled_perturb: p + d / s in f32 (no contraction, correctly rounded division), bit for bit, over the genomes of H 4 / 32 /
    128 x L 0 / 3 and over hand-built segments of 1, 8 191, 8 192, 8 193 and 20 000 weights (the launch has 8 192 threads)"""
    import serl_amd
    for H in (4, 32, 128):
        for L in (0, 3):
            spec = serl_amd.NetSpec(7, 3, H, L, 'tanh')
            segs = spec.genome_segments()
            stride = spec.param_count + 5
            w0 = R.sentinel_f32((4, stride))
            delta, scaling = _delta_scaling(sum(s[1] for s in segs), H + L)
            _perturb(engine, w0, stride, 2, segs, delta, scaling, 'H %d L %d' % (H, L))
    segs = [(3, 1), (10, 8191), (8300, 8192), (16600, 8193), (24900, 20000)]
    stride = 45000 + 5
    w0 = R.sentinel_f32((3, stride))
    delta, scaling = _delta_scaling(sum(s[1] for s in segs), 99)
    _perturb(engine, w0, stride, 1, segs, delta, scaling, 'hand-built segments')
    _perturb(engine, w0, stride, 0, [(44999, 1)], np.array([0.5], np.float32), np.array([0.01], np.float32), 'one weight')


def test_ssne_edit_refusals_on_the_host(engine):
    """arguments serl_capi.hip rejects before any launch: SERL_E_INVALID, the tensor untouched"""
    lib, ctx = engine.lib, engine.ctx
    w0 = R.sentinel_f32((4, 40))
    w = _dev(engine, w0)
    i4, f4 = _dev(engine, np.zeros(4, np.int32)), _dev(engine, np.ones(4, np.float32))
    s = _sync_stream()
    W, I, F = _ptr(w), _ptr(i4), _ptr(f4)
    calls = [lambda: lib.serl_ga_clone(None, W, 40, 40, I, I, 1, s), lambda: lib.serl_ga_clone(ctx, None, 40, 40, I, I, 1, s),
             lambda: lib.serl_ga_clone(ctx, W, 40, 40, None, I, 1, s), lambda: lib.serl_ga_clone(ctx, W, 40, 40, I, None, 1, s),
             lambda: lib.serl_ga_clone(ctx, W, 40, 40, I, I, -1, s), lambda: lib.serl_ga_clone(ctx, W, 40, 0, I, I, 1, s),
             lambda: lib.serl_ga_crossover(None, W, 40, 0, 1, I, 1, s), lambda: lib.serl_ga_crossover(ctx, None, 40, 0, 1, I, 1, s),
             lambda: lib.serl_ga_crossover(ctx, W, 40, 0, 1, None, 1, s), lambda: lib.serl_ga_crossover(ctx, W, 40, 0, 1, I, -1, s),
             lambda: lib.serl_ga_mutate(None, W, 40, 0, I, I, F, F, 1, s), lambda: lib.serl_ga_mutate(ctx, None, 40, 0, I, I, F, F, 1, s),
             lambda: lib.serl_ga_mutate(ctx, W, 40, 0, I, I, F, F, -1, s),
             lambda: lib.serl_ga_mutate(ctx, W, 40, 0, None, I, F, F, 1, s), lambda: lib.serl_ga_mutate(ctx, W, 40, 0, I, None, F, F, 1, s),
             lambda: lib.serl_ga_mutate(ctx, W, 40, 0, I, I, None, F, 1, s), lambda: lib.serl_ga_mutate(ctx, W, 40, 0, I, I, F, None, 1, s),
             lambda: lib.serl_ga_scaled_perturb(None, W, 40, 0, I, I, 1, F, F, s), lambda: lib.serl_ga_scaled_perturb(ctx, None, 40, 0, I, I, 1, F, F, s),
             lambda: lib.serl_ga_scaled_perturb(ctx, W, 40, 0, None, I, 1, F, F, s), lambda: lib.serl_ga_scaled_perturb(ctx, W, 40, 0, I, None, 1, F, F, s),
             lambda: lib.serl_ga_scaled_perturb(ctx, W, 40, 0, I, I, 1, None, F, s), lambda: lib.serl_ga_scaled_perturb(ctx, W, 40, 0, I, I, 1, F, None, s),
             lambda: lib.serl_ga_scaled_perturb(ctx, W, 40, 0, I, I, 0, F, F, s)]
    for k, call in enumerate(calls):
        assert call() == R.E_INVALID, 'call %d' % k
    assert lib.serl_ga_mutate(ctx, W, 40, 0, None, None, None, None, 0, s) == 0          # n = 0: the lists may be NULL
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(w), w0.view(np.uint32))


def test_clone_pair_count_at_and_past_65536(engine):
    """serl_ga_clone with 65 536 and 65 537 pairs (the pairs are a grid dimension of their own): each call either copies every pair or
    is refused with a negative status and leaves the tensor untouched -- never half of it.  65 536 must be served."""
    P, stride = 3, 4
    for n in (65536, 65537):
        w0 = R.sentinel_f32((2 * n, stride))
        w = _dev(engine, w0)
        src, dst = np.arange(n, dtype=np.int32), (np.arange(n, dtype=np.int32) + n)
        s, d = _dev(engine, src), _dev(engine, dst)
        rc = engine.lib.serl_ga_clone(engine.ctx, _ptr(w), stride, P, _ptr(s), _ptr(d), n, _sync_stream())
        torch.cuda.synchronize()
        print('serl_ga_clone n = %d -> status %d' % (n, rc))
        if rc == 0:
            np.testing.assert_array_equal(_u32(w), R.clone_ref(w0, P, src, dst).view(np.uint32), err_msg='n %d' % n)
        else:
            assert rc < 0
            np.testing.assert_array_equal(_u32(w), w0.view(np.uint32), err_msg='n %d refused' % n)
        assert rc == 0, 'n = %d refused' % n          # both are served: include/serl_amd.h states the limit that remains


# =====================================================================================================================================
# replay scatter
# =====================================================================================================================================
class _Job(ctypes.Structure):
    _fields_ = [('ring', VP), ('capacity', ctypes.c_int32), ('position', ctypes.c_int32), ('episode', ctypes.c_int32),
                ('length', ctypes.c_int32), ('cost_only', ctypes.c_int32), ('skip', ctypes.c_int32)]


def _flags(T, on_rows=None, density=None, seed=0, mixed=False):
    """cost column of T rows as f32"""
    rs = np.random.RandomState(seed)
    f = np.zeros(T, np.float32)
    if on_rows is not None:
        f[list(on_rows)] = 1.0
    if density is not None:
        f[rs.rand(T) < density] = 1.0
    if mixed:          # 1.0, 2.0 and NaN are taken; 0.0 and -0.0 are not
        f = np.array([1.0, 2.0, -0.0, np.nan, 0.0], np.float32)[rs.randint(0, 5, T)]
    return f


def test_replay_scatter_hand_built_jobs(engine):
    """serl_replay_scatter, one property per job, all jobs in one launch: lengths around the wavefront and block edges with NaN rows
    past the length, cost-flag patterns (none, all, first, last, across the wavefront and block edges, two densities, the flag values
    1.0 / 2.0 / NaN taken and -0.0 not), skips, capacities from 1 up with the position at 0, at capacity - 1 and wrapping inside the
    first wavefront.  Rows are random bit patterns; every ring lies in one sentinel-filled buffer that is compared as a whole."""
    T = 600
    rs = np.random.RandomState(21)
    specs = []          # (length, flags or None, cost_only, skip, capacity, position)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, T):
        specs.append((n, None, 0, 0, 1000, 0))
    pats = [_flags(T), _flags(T, range(T)), _flags(T, [0]), _flags(T, [T - 1]), _flags(T, [255, 256]), _flags(T, [63, 64]),
            _flags(T, density=0.5, seed=1), _flags(T, density=0.02, seed=2), _flags(T, mixed=True, seed=3)]
    for f in pats:
        specs.append((T, f, 1, 0, 1000, 5))
    specs.append((300, _flags(T, [255, 256, 299, 300, 301]), 1, 0, 1000, 5))          # flagged rows past the length are not taken
    half = _flags(T, density=0.5, seed=4)
    for f, cost in ((None, 0), (half, 1)):
        taken = T if f is None else int((half != 0).sum())
        for skip in (0, 1, 37, 256, taken - 1, taken, taken + 5):
            specs.append((T, f, cost, skip, 1000, 990))
    for cap in (1, 7, 63, 255, 256, 257, 1000):
        for pos in sorted({0, cap - 1, max(cap - 10, 0), cap // 2}):
            n = min(T, cap + 70)
            specs.append((n, None, 0, max(0, n - cap), cap, pos))          # taken - skip <= capacity: what scatter_episodes guarantees
            specs.append((n, half, 1, max(0, int((half[:n] != 0).sum()) - cap), cap, pos))
    E = len(specs) + 1
    staged = rs.randint(0, 2 ** 32, size=(E, T, R.ROW), dtype=np.uint64).astype(np.uint32)
    offs, rows_total = [], 3
    for e, (n, f, cost, skip, cap, pos) in enumerate(specs, start=1):          # job j reads episode j + 1: episode 0 is never read
        staged[e, :, 19] = (_flags(T, mixed=True, seed=100 + e) if f is None else f).view(np.uint32)
        staged[e, n:] = (np.uint32(0x7FC00000) + np.arange((T - n) * R.ROW, dtype=np.uint32)).reshape(T - n, R.ROW)      # NaN rows past the length
        offs.append(rows_total)
        rows_total += cap + 3                                                   # three guard rows between rings
    rings0 = R.sentinel_u32(rows_total * R.ROW).reshape(rows_total, R.ROW)
    want = rings0.copy()
    rings = _dev(engine, rings0.view(np.float32))
    arr = (_Job * len(specs))()
    wrote_nothing = 0
    for j, ((n, f, cost, skip, cap, pos), off) in enumerate(zip(specs, offs)):
        arr[j] = _Job(rings.data_ptr() + off * R.ROW * 4, cap, pos, j + 1, n, cost, skip)
        before = want[off:off + cap].copy()
        taken = R.scatter_job_ref(want[off:off + cap], cap, pos, staged[j + 1, :n], cost, skip)
        assert taken - skip <= cap
        wrote_nothing += int((want[off:off + cap] == before).all())
    assert wrote_nothing >= 6          # length 0, no flagged row, skip = taken and taken + 5 (twice)
    st = _dev(engine, staged.view(np.float32))
    jb = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(engine.device)
    rc = engine.lib.serl_replay_scatter(engine.ctx, _ptr(st), T, _ptr(jb), len(specs), _sync_stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = _u32(rings)
    bad = np.nonzero((got != want).any(1))[0]
    owner = {r: j for j, off in enumerate(offs) for r in range(off - 3, off + specs[j][4])}
    assert len(bad) == 0, 'ring rows differ; jobs (length, cost_only, skip, capacity, position): %s' % sorted(
        {(j,) + tuple(specs[j][i] for i in (0, 2, 3, 4, 5)) for j in {owner.get(int(b), -1) for b in bad[:50]} if j >= 0})[:8]
    # n_jobs = 0 and the host-side refusals: nothing is launched
    lib, ctx, s = engine.lib, engine.ctx, _sync_stream()
    assert lib.serl_replay_scatter(ctx, _ptr(st), T, _ptr(jb), 0, s) == 0
    for call in (lambda: lib.serl_replay_scatter(None, _ptr(st), T, _ptr(jb), 1, s), lambda: lib.serl_replay_scatter(ctx, None, T, _ptr(jb), 1, s),
                 lambda: lib.serl_replay_scatter(ctx, _ptr(st), T, None, 1, s), lambda: lib.serl_replay_scatter(ctx, _ptr(st), T, _ptr(jb), -1, s),
                 lambda: lib.serl_replay_scatter(ctx, _ptr(st), 0, _ptr(jb), 1, s)):
        assert call() == R.E_INVALID
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_u32(rings), want)


def test_replay_scatter_fuzz_through_scatter_episodes(engine):
    """replay.scatter_episodes on 620 random job lists in four launches (644 jobs in the first; several jobs per ring; rings from one
    slot to 3 000; a second round on partly filled rings) against sequential add() calls: position, len and every slot of every ring,
    bit for bit -- the slots never written keep their sentinel.  The classes the draw must contain are asserted."""
    from serl_amd.replay import DeviceReplay, scatter_episodes
    staged, caps, launches = R.fuzz_plan()
    st = _dev(engine, staged.view(np.float32))
    rings, mems, state = [], [], []
    for r, cap in enumerate(caps):
        ring = DeviceReplay(cap, engine.device, engine)
        mem = R.sentinel_u32(cap * R.ROW, base=0x3F000000 + 64 * r).reshape(cap, R.ROW)
        ring.rows.copy_(_dev(engine, mem.view(np.float32)))
        rings.append(ring); mems.append(mem); state.append((0, 0))
    seen = set()
    assert sum(len(ids) for ids, _ in launches) >= 200 and sum(len(j) for j in launches[0][1]) >= 500
    for ids, lists in launches:
        jobs, keys = [], []
        for r, jl in zip(ids, lists):
            seen |= R.fuzz_classes(staged, caps[r], state[r][0], jl)
            for i, (e, n, cost) in enumerate(jl):
                keys.append((i, r))
                tk = R.taken_rows(staged[e, :n], cost)
                jobs.append((rings[r], e, n, cost, len(tk)))
                mems[r], pos, size = R.replay_emulate(caps[r], [tk], state[r][0], state[r][1], mems[r])
                state[r] = (pos, size)
        order = sorted(range(len(jobs)), key=lambda k: keys[k])          # rings interleaved, the order within a ring kept
        scatter_episodes(engine, st, [jobs[k] for k in order])
        torch.cuda.synchronize()
        for r in ids:
            assert (rings[r].position, len(rings[r])) == state[r], 'ring %d' % r
            np.testing.assert_array_equal(_u32(rings[r].rows), mems[r], err_msg='ring %d (capacity %d)' % (r, caps[r]))
    missing = [c for c in R.FUZZ_REQUIRED + ['len_%d' % R.FUZZ_T] if c not in seen]
    assert not missing, missing


# =====================================================================================================================================
# smoothness
# =====================================================================================================================================
WORST = {'rel': 0.0, 'zero': 0.0}


def _smooth(engine, y, lengths, max_len, dt=0.01, pad=0, expect=0):
    """serl_smoothness through the ABI.  y: list of traces [>= |length|, 3]; the device buffer holds NaN wherever the kernel must not
    read (rows past an episode's length, the `pad` doubles between episodes), work and out are NaN before the call and longer than
    the call needs: what lies beyond must still be NaN."""
    E = len(lengths)
    T = max(max_len, 1)
    stride = 3 * T + pad
    a = np.full((E, stride), np.nan)
    for e, n in enumerate(np.abs(lengths)):
        a[e, :3 * n] = np.asarray(y[e], np.float64)[:n].reshape(-1)
    ws = int(engine.lib.serl_smoothness_work_size(E, max_len))
    work = torch.full((ws + 64,), float('nan'), dtype=torch.float64, device=engine.device)
    out = torch.full((E + 8,), float('nan'), dtype=torch.float64, device=engine.device)
    ad, ln = _dev(engine, a), _dev(engine, np.asarray(lengths, np.int32))
    rc = engine.lib.serl_smoothness(engine.ctx, _ptr(ad), stride, _ptr(ln), E, max_len, float(dt), _ptr(work), _ptr(out), _sync_stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, engine.lib.serl_last_error())
    o, w = out.cpu().numpy(), work.cpu().numpy()
    assert np.isnan(o[E:]).all() and np.isnan(w[ws:]).all()
    if rc != 0:
        assert np.isnan(o).all()
        return None
    assert not np.isnan(o[:E]).any()
    return o[:E]


def _check(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    nz = want != 0
    if nz.any():
        rel = float((np.abs(got - want)[nz] / np.abs(want[nz])).max())
        WORST['rel'] = max(WORST['rel'], rel)
        print('smoothness %s: worst relative error %.3g (allowed %g)' % (what, rel, R.SMOOTH_RTOL))
    np.testing.assert_allclose(got, want, rtol=R.SMOOTH_RTOL, atol=R.SMOOTH_ATOL, err_msg=what)


def _same(a, b, what):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64), err_msg=what)


@pytest.fixture(scope='module')
def edge_batch():
    """every edge length once as +N and once as -N on the same trace -> (traces, lengths, longdouble DFT power per distinct N)"""
    L = R.SMOOTH_EDGE_LENGTHS
    base = R.traces(len(L), 8192, seed=5)
    y = [base[i] for i in range(len(L))] * 2
    lengths = np.array(L + [-n for n in L], np.int32)
    perm = np.random.RandomState(1).permutation(len(lengths))          # signs and lengths mixed through the batch
    power = {n: R.dft_power(base[i][:n]) for i, n in enumerate(L)}
    return [y[p] for p in perm], lengths[perm], power


def _edge_want(lengths, power, dt):
    return np.array([R.smoothness_from_power(power[abs(n)], abs(n), dt) for n in lengths])


def test_smoothness_edge_lengths_against_longdouble_dft(engine, edge_batch):
    """lengths 0 .. 8, the chunk edges (N/2 - 1 = 255 .. 257, 512, 513), 2 001, 8 001, 8 191, 8 192, each also negative, against the
    longdouble DFT; a negative length gives the bits of the positive one; no spectrum below four steps"""
    y, lengths, power = edge_batch
    got = _smooth(engine, y, lengths, 8192)
    _check(got, _edge_want(lengths, power, 0.01), 'edge lengths')
    for n in R.SMOOTH_EDGE_LENGTHS:
        i, j = np.nonzero(lengths == n)[0][0], np.nonzero(lengths == -n)[0][0]
        assert got[i].tobytes() == got[j].tobytes(), n
        assert (got[i] == 0.0) == (n < 4), n


def test_smoothness_does_not_depend_on_the_grid(engine, edge_batch):
    """max_len = the longest episode or 8 192, episode_stride 3 T or 3 T + 9, dt 0.01 / 0.02 / 0.005, an episode alone, in the middle
    of the batch or in a permuted batch: bit-identical results (fixed summation order), and right for every dt"""
    y, lengths, power = edge_batch
    keep = [e for e in range(len(lengths)) if abs(lengths[e]) <= 2001]
    ys, ls = [y[e] for e in keep], lengths[keep]
    assert len(ls) == 2 * (len(R.SMOOTH_EDGE_LENGTHS) - 3)
    ref = _smooth(engine, ys, ls, 2001)
    _check(ref, _edge_want(ls, power, 0.01), 'max_len 2001')
    _same(_smooth(engine, ys, ls, 8192), ref, 'max_len 8192 against 2001')
    _same(_smooth(engine, ys, ls, 2001, pad=9), ref, 'episode_stride 3 T + 9')
    _same(_smooth(engine, ys, ls, 8192, pad=9), ref, 'episode_stride 3 T + 9, max_len 8192')
    _same(_smooth(engine, y, lengths, 8192)[keep], ref, 'inside the full batch')
    perm = np.random.RandomState(2).permutation(len(ls))
    _same(_smooth(engine, [ys[p] for p in perm], ls[perm], 2001), ref[perm], 'permuted')
    for e in (int(np.nonzero(ls == 1029)[0][0]), int(np.nonzero(ls == -517)[0][0]), int(np.nonzero(ls == 2001)[0][0])):
        _same(_smooth(engine, [ys[e]], ls[[e]], abs(int(ls[e]))), ref[[e]], 'episode %d alone' % e)
    for dt in (0.02, 0.005):
        got = _smooth(engine, ys, ls, 2001, dt=dt)
        _check(got, _edge_want(ls, power, dt), 'dt %g' % dt)
        _same(_smooth(engine, ys, ls, 8192, dt=dt, pad=9), got, 'dt %g, other grid' % dt)


def test_smoothness_signals_with_a_known_answer(engine):
    """pure tones on bin 1, N//2 - 1 and the chunk-edge bins 256 / 257 of N = 2 001 (a dropped first, last or chunk-edge bin zeroes
    them), impulses at sample 0 and N - 1 (flat spectrum), one channel non-zero at a time, and exact homogeneity under 2^-20 / 2^20"""
    N, dt = 2001, 0.01
    ks = (1, 256, 257, N // 2 - 1)
    y = [R.tone(N, k) for k in ks]
    want = [R.tone_value(N, k, dt) for k in ks]
    for N2, at in ((2001, 0), (2001, 2000), (516, 0), (516, 515), (8, 0), (8, 7)):
        t = np.zeros((N2, 3)); t[at, 2] = 0.25
        y.append(t); want.append(R.impulse_value(N2, dt, 0.25))
    base = R.traces(1, N, seed=9)[0]
    for c in range(3):
        t = np.zeros((N, 3)); t[:, c] = base[:, 0]
        y.append(t); want.append(R.smoothness_dft(t, dt) if c == 0 else want[-1])
    h = R.smoothness_dft(base, dt)
    for s in (1.0, 2.0 ** -20, 2.0 ** 20):
        y.append(base * s); want.append(h * s)
    lengths = np.array([len(t) for t in y], np.int32)
    got = _smooth(engine, y, lengths, 2001)
    assert (np.abs(got[:4]) > 1.0).all()
    _check(got, want, 'known answers')
    n = len(y)
    assert got[n - 6].tobytes() == got[n - 5].tobytes() == got[n - 4].tobytes()          # the channel does not matter
    assert got[n - 2] == got[n - 3] * 2.0 ** -20 and got[n - 1] == got[n - 3] * 2.0 ** 20          # exact: powers of two
    for dt2 in (0.02, 0.005):
        _check(_smooth(engine, y[:10], lengths[:10], 2001, dt=dt2),
               [R.tone_value(N, k, dt2) for k in ks] + [R.impulse_value(len(t), dt2, 0.25) for t in y[4:10]], 'known answers, dt %g' % dt2)


def test_smoothness_of_exact_zero_signals(engine):
    """constant traces (saturated actuator, jammed rudder) and the Nyquist alternation (+c, -c, ...) at even N: bin 0 and bin N/2 are
    not part of the metric, so the exact value is 0 (an `i <= N/2` off-by-one gives ~1e3).  What is left is rounding noise:
    |got| <= max(16 x the numpy-FFT value of the same trace, 1e-12)."""
    y, kind = [], []
    for N in R.ZERO_CONST_LENGTHS:
        y.append(np.full((N, 3), 0.7)); kind.append('constant 0.7, N %d' % N)
        y.append(np.tile(np.array([0.7, -0.25, 1.0]), (N, 1))); kind.append('constant per channel, N %d' % N)
    for N in R.ZERO_NYQUIST_LENGTHS:
        y.append(np.tile((0.7 * (-1.0) ** np.arange(N))[:, None], (1, 3))); kind.append('alternation 0.7, N %d' % N)
    lengths = np.array([len(t) for t in y], np.int32)
    got = _smooth(engine, y, lengths, 8001)
    fft = np.array([R.smoothness_fft(t) for t in y])
    ratio = np.abs(got) / np.maximum(np.abs(fft), R.SMOOTH_ATOL / R.ZERO_FACTOR)
    for k, g, f, r in zip(kind, got, fft, ratio):
        print('smoothness zero signal %s: got %.3g, numpy FFT %.3g, ratio %.3g (allowed %g)' % (k, g, f, r, R.ZERO_FACTOR))
    WORST['zero'] = max(WORST['zero'], float(ratio.max()))
    bad = [(k, g, f) for k, g, f in zip(kind, got, fft) if abs(g) > max(R.ZERO_FACTOR * abs(f), R.SMOOTH_ATOL)]
    assert not bad, bad


def test_smoothness_of_a_training_generation(engine):
    """300 episodes of ~150 distinct lengths in 200 .. 2 001, some recorded as negative, against numpy's FFT"""
    rs = np.random.RandomState(6)
    pool = rs.randint(200, 2002, 150)
    lengths = pool[rs.randint(0, 150, 300)]
    lengths[:3] = (200, 2001, 2001)
    assert len(np.unique(lengths)) >= 120
    base = R.traces(300, 2001, seed=7)
    want = np.array([R.smoothness_fft(base[e, :n]) for e, n in enumerate(lengths)])
    sign = np.where(rs.rand(300) < 0.3, -1, 1)
    got = _smooth(engine, list(base), (lengths * sign).astype(np.int32), 2001)
    _check(got, want, 'training generation')


def test_smoothness_batch_at_and_past_65536_episodes(engine):
    """65 536 episodes in one call (what the product evaluates at its saturating configuration; the batch is a grid dimension of its
    own) and 65 537: every episode computed, or a negative status and `out` untouched.  65 536 must be served."""
    N = 8
    rs = np.random.RandomState(12)
    y = rs.randn(65537, N, 3) * 0.1
    Y = np.fft.fft(y, axis=1)[:, 1:N // 2]
    f = np.linspace(0.01, 50.0, N // 2 - 1)
    want = -np.sqrt(((np.abs(Y) ** 2 * 0.01) * f[None, :, None]).sum((1, 2)) * 2 / N) * 100 * (80 / (N * 0.01))
    for E in (65536, 65537):
        ws = int(engine.lib.serl_smoothness_work_size(E, N))
        work = torch.full((ws + 64,), float('nan'), dtype=torch.float64, device=engine.device)
        out = torch.full((E + 8,), float('nan'), dtype=torch.float64, device=engine.device)
        ad, ln = _dev(engine, y[:E]), _dev(engine, np.full(E, N, np.int32))
        rc = engine.lib.serl_smoothness(engine.ctx, _ptr(ad), 3 * N, _ptr(ln), E, N, 0.01, _ptr(work), _ptr(out), _sync_stream())
        torch.cuda.synchronize()
        print('serl_smoothness n_episodes = %d -> status %d' % (E, rc))
        o = out.cpu().numpy()
        assert np.isnan(o[E:]).all() and np.isnan(work.cpu().numpy()[ws:]).all()
        if rc == 0:
            _check(o[:E], want[:E], '%d episodes' % E)
        else:
            assert rc < 0 and np.isnan(o).all(), 'refused, but out was written'
        assert rc == 0, 'n_episodes = %d refused' % E          # both are served: include/serl_amd.h states the limit that remains


def test_smoothness_refusals_on_the_host(engine):
    """max_len = 8 193 -> SERL_E_UNSUPPORTED; dt = 0, n_episodes = 0, NULL buffers -> SERL_E_INVALID; nothing launched, out untouched"""
    lib, ctx = engine.lib, engine.ctx
    y = R.traces(2, 16, seed=1)
    a, ln = _dev(engine, y), _dev(engine, np.array([16, 12], np.int32))
    work = torch.full((64,), float('nan'), dtype=torch.float64, device=engine.device)
    out = torch.full((8,), float('nan'), dtype=torch.float64, device=engine.device)
    s = _sync_stream()
    A, L, W, O = _ptr(a), _ptr(ln), _ptr(work), _ptr(out)
    assert lib.serl_smoothness(ctx, A, 48, L, 2, 8193, 0.01, W, O, s) == R.E_UNSUPPORTED
    for call in (lambda: lib.serl_smoothness(ctx, A, 48, L, 2, 16, 0.0, W, O, s), lambda: lib.serl_smoothness(ctx, A, 48, L, 2, 16, -0.01, W, O, s),
                 lambda: lib.serl_smoothness(ctx, A, 48, L, 2, 16, float('nan'), W, O, s),
                 lambda: lib.serl_smoothness(ctx, A, 48, L, 0, 16, 0.01, W, O, s), lambda: lib.serl_smoothness(ctx, A, 48, L, 2, 0, 0.01, W, O, s),
                 lambda: lib.serl_smoothness(None, A, 48, L, 2, 16, 0.01, W, O, s), lambda: lib.serl_smoothness(ctx, None, 48, L, 2, 16, 0.01, W, O, s),
                 lambda: lib.serl_smoothness(ctx, A, 48, None, 2, 16, 0.01, W, O, s), lambda: lib.serl_smoothness(ctx, A, 48, L, 2, 16, 0.01, None, O, s),
                 lambda: lib.serl_smoothness(ctx, A, 48, L, 2, 16, 0.01, W, None, s)):
        assert call() == R.E_INVALID
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all() and np.isnan(work.cpu().numpy()).all()
    assert lib.serl_smoothness(ctx, A, 48, L, 2, 16, 0.01, W, O, s) == 0          # the same buffers are fine
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy()[:2], [R.smoothness_dft(y[0]), R.smoothness_dft(y[1, :12])], rtol=R.SMOOTH_RTOL)


def test_zz_report_worst_smoothness_ratios(engine):
    """prints the worst ratios the smoothness tests of this run saw (the figures quoted in the module docstring)"""
    print('smoothness worst: relative error %.3g of %g allowed; zero-signal ratio %.3g of %g allowed' % (
        WORST['rel'], R.SMOOTH_RTOL, WORST['zero'], R.ZERO_FACTOR))
    assert WORST['rel'] <= R.SMOOTH_RTOL

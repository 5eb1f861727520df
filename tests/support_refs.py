"""Shared by tests/test_support_refs.py (CPU) and tests/test_gpu_support_kernels.py (GPU): plain references of the device kernels a
training generation calls besides the rollout -- the SSNE weight-tensor edits (serl_ga_clone / crossover / mutate / scaled_perturb),
serl_replay_scatter and serl_smoothness -- as include/serl_amd.h words them, plus the case lists of the GPU tests.  Every reference is
sequential and does nothing clever; the CPU test pins each to an independent counterpart and to the goldens the reference project
itself produced.  A plain module (not a conftest): nothing here is a fixture."""
import numpy as np

ROW = 20                      # floats of a replay row: obs7 | action3 | next_obs7 | reward | done | cost
E_INVALID, E_HIP, E_UNSUPPORTED = -1, -2, -3            # enum serl_status


# ---- bit patterns -----------------------------------------------------------------------------------------------------------------
def sentinel_u32(n, base=0x3F000000):
    """n different f32 bit patterns, every one a finite non-zero number (base 0x3F000000: 0.5 upwards, one ulp apart): what an output
    buffer holds before a call, so that a cell the call must not touch is recognised and no two cells can be confused"""
    assert 0 < base and base + n < 0x7F800000
    return (np.uint32(base) + np.arange(n, dtype=np.uint32)).astype(np.uint32)


def sentinel_f32(shape, base=0x3F000000):
    return sentinel_u32(int(np.prod(shape)), base).view(np.float32).reshape(shape)


def same_f32(got, want):
    """bit for bit, except that any NaN equals any NaN: the payload and sign of a NaN an operation PRODUCES (inf - inf, 0 * inf) are the
    processor's choice (x86 returns the negative quiet NaN, the GPU the positive one).  -> indices that differ"""
    g, w = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    gn, wn = np.isnan(g), np.isnan(w)
    return np.nonzero((gn != wn) | (~gn & (g.view(np.uint32) != w.view(np.uint32))))[0]


# ---- SSNE edits (include/serl_amd.h "SSNE weight-tensor edits"), sequential numpy f32 ------------------------------------------------
def clone_ref(w, P, src, dst):
    """weights[dst[i]][0 .. P) = weights[src[i]][0 .. P).  The pairs of one call are independent (no destination is another pair's
    source), so reading every source from the tensor as it was is the same as any order."""
    out = w.copy()
    for s, d in zip(src, dst):
        out[d, :P] = w[s, :P]
    return out


def crossover_ref(w, ma, mb, ops):
    """ops in order, later ones see earlier ones: dir 0 copies member b -> a, dir 1 copies a -> b, at columns [offset, offset + length)"""
    out = w.copy()
    for off, ln, d in np.asarray(ops, np.int64).reshape(-1, 3):
        if d == 0:
            out[ma, off:off + ln] = out[mb, off:off + ln].copy()
        else:
            out[mb, off:off + ln] = out[ma, off:off + ln].copy()
    return out


CLAMP = np.float32(1000000.0)


def clamp_ref(v):
    """torch.clamp(v, -1e6, 1e6) (mod_neuro_evo.py:57-59): a NaN stays a NaN"""
    v = np.float32(v)
    if v > CLAMP:
        return CLAMP
    if v < -CLAMP:
        return -CLAMP
    return v


def mutate_ref(row, idx, kind, z, strength):
    """n sparse edits of one member IN ORDER: kind 0: w += z * (strength * w), kind 1: w = z; each followed by the clamp"""
    m = np.array(row, dtype=np.float32)
    with np.errstate(all='ignore'):
        for i, k, zz, s in zip(idx, kind, np.asarray(z, np.float32), np.asarray(strength, np.float32)):
            v = m[i]
            v = np.float32(v + np.float32(zz * np.float32(s * v))) if k == 0 else np.float32(zz)
            m[i] = clamp_ref(v)
    return m


def scaled_perturb_ref(row, segs, delta, scaling):
    """theta[i] += delta[i] / scaling[i] over the (offset, length) segments of the packed row, delta / scaling packed segment after segment"""
    out = np.array(row, dtype=np.float32)
    delta, scaling = np.asarray(delta, np.float32), np.asarray(scaling, np.float32)
    p = 0
    with np.errstate(all='ignore'):
        for off, ln in segs:
            out[off:off + ln] = out[off:off + ln] + delta[p:p + ln] / scaling[p:p + ln]
            p += ln
    return out


# ---- replay rings --------------------------------------------------------------------------------------------------------------------
def taken_rows(rows_u32, cost_only):
    """the rows a job takes: all, or the cost-flagged ones -- row[19] != 0.0 as a float: -0.0 is not flagged, a NaN is"""
    rows_u32 = np.asarray(rows_u32, np.uint32).reshape(-1, ROW)
    if not cost_only:
        return rows_u32
    with np.errstate(invalid='ignore'):
        return rows_u32[rows_u32[:, 19].view(np.float32) != 0.0]


def replay_emulate(cap, rows_list, pos=0, size=0, mem=None):
    """n sequential add() calls (base/core/replay_memory.py:21-31) on uint32 views of the rows -> (memory, position, size)"""
    mem = np.zeros((cap, ROW), np.uint32) if mem is None else mem
    for rows in rows_list:
        for r in np.asarray(rows).reshape(-1, ROW):
            mem[pos] = r
            pos = (pos + 1) % cap
            size = min(cap, size + 1)
    return mem, pos, size


def scatter_job_ref(ring_u32, cap, position, rows_u32, cost_only, skip):
    """one serl_replay_job as the header words it: the taken row of rank k goes to slot (position + k) % capacity, ranks below `skip`
    are not written.  In place on ring_u32 [cap, 20]; -> number of rows taken"""
    tk = taken_rows(rows_u32, cost_only)
    for k in range(int(skip), len(tk)):
        ring_u32[(position + k) % cap] = tk[k]
    return len(tk)


# ---- smoothness ---------------------------------------------------------------------------------------------------------------------
def dft_power(y):
    """P_i = sum_c |Y_i,c|^2 for the bins i = 1 .. N//2 - 1 of y [N, C], as a direct DFT in numpy.longdouble with twiddles
    cos / sin(2 pi ((i k) mod N) / N) -- no FFT library, no incremental index.  -> longdouble [N//2 - 1]"""
    y = np.asarray(y, dtype=np.longdouble)
    N = y.shape[0]
    nf = N // 2 - 1
    if N < 4:
        return np.zeros(0, np.longdouble)
    two_pi = np.longdouble(8) * np.arctan(np.longdouble(1))
    k = np.arange(N, dtype=np.int64)
    ang = two_pi * k.astype(np.longdouble) / np.longdouble(N)
    c, s = np.cos(ang), np.sin(ang)
    P = np.zeros(nf, np.longdouble)
    for i0 in range(1, nf + 1, 128):
        i = np.arange(i0, min(i0 + 128, nf + 1), dtype=np.int64)
        m = (i[:, None] * k[None, :]) % N
        re, im = c[m] @ y, -(s[m] @ y)
        P[i0 - 1:i0 - 1 + len(i)] = (re * re + im * im).sum(1)
    return P


def smoothness_from_power(P, N, dt):
    """-sqrt(S 2 / N) 100 (80 / (N dt)), S = sum_i P_i dt f_i, f = linspace(dt, 1 / (2 dt), N//2 - 1); 0 for N < 4"""
    if N < 4:
        return 0.0
    f = np.linspace(dt, 1 / (2 * dt), N // 2 - 1).astype(np.longdouble)
    S = (np.asarray(P, np.longdouble) * np.longdouble(dt) * f).sum()
    return float(-(np.sqrt(S * 2 / N) * 100 * (np.longdouble(80) / (N * np.longdouble(dt)))))


def smoothness_dft(y, dt=0.01):
    y = np.asarray(y)
    return smoothness_from_power(dft_power(y), y.shape[0], dt)


def smoothness_fft(y, dt=0.01):
    """the same metric through numpy's FFT (float64): the bulk reference, and the yardstick of the exact-zero signals"""
    y = np.asarray(y, np.float64)
    N = y.shape[0]
    if N < 4:
        return 0.0
    Y = np.fft.fft(y, axis=0)[1:N // 2]
    S = np.abs(Y * np.conj(Y)) * dt
    f = np.linspace(dt, 1 / (2 * dt), N // 2 - 1)
    return float(-np.sqrt((S * f[:, None]).sum() * 2 / N) * 100 * (80 / (N * dt)))


def traces(n, T, seed, dt=0.01):
    """n action traces [n, T, 3] of the kind an actor produces: a sinusoid of 0.1 .. 3 Hz per channel plus white noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(T) * dt
    y = np.zeros((n, T, 3))
    for e in range(n):
        for c in range(3):
            y[e, :, c] = 0.1 * np.sin(2 * np.pi * rng.uniform(0.1, 3.0) * t + rng.uniform(0, 6)) + 0.01 * rng.standard_normal(T)
    return y


# The lengths where the kernel's cases split: no spectrum (N < 4), the first bins (4 .. 8), the edges of the 256-frequency chunks
# (N/2 - 1 = 255 .. 257 and 512 .. 513), the training episode (2 001), the full episode (8 001) and the largest twiddle table (8 192).
SMOOTH_EDGE_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 512, 513, 514, 515, 516, 517, 1026, 1027, 1028, 1029, 2001, 8001, 8191, 8192]
SMOOTH_RTOL, SMOOTH_ATOL = 1e-9, 1e-12          # the project's tolerance of the metric (tests/test_gpu_ga.py)
ZERO_FACTOR = 16.0                              # exact-zero signals: |got| <= max(ZERO_FACTOR |numpy-FFT value of the same trace|, SMOOTH_ATOL)
# Exact-zero signals.  Lengths: the two at which the numpy-FFT yardstick's own rounding noise is on record (2 001: 1.2e-12, 4 001: 3.9e-12
# at c = 0.7) and the full episode of 8 001 steps; the Nyquist alternation needs an even length: their even neighbours.  Shorter traces are
# left out on purpose: the metric multiplies the spectrum's norm by 8000 / (N^2 dt), so the absolute floor of 1e-12 asks for more than
# float64 holds once N falls below a few hundred steps.
ZERO_CONST_LENGTHS = [2001, 4001, 8001]
ZERO_NYQUIST_LENGTHS = [2000, 4000, 8000]


def tone(N, k, amp=0.3, phase=0.4):
    """amp cos(2 pi k n / N + phase) on channel 0: all its power in bin k -> (trace [N, 3], closed-form smoothness at dt)"""
    y = np.zeros((N, 3))
    y[:, 0] = amp * np.cos(2 * np.pi * k * np.arange(N) / N + phase)
    return y


def tone_value(N, k, dt, amp=0.3):
    f = np.linspace(dt, 1 / (2 * dt), N // 2 - 1)[k - 1]
    return -np.sqrt((amp * N / 2) ** 2 * dt * f * 2 / N) * 100 * (80 / (N * dt))


def impulse_value(N, dt, amp):
    """one sample of height amp anywhere: |Y_i|^2 = amp^2 in every bin"""
    f = np.linspace(dt, 1 / (2 * dt), N // 2 - 1)
    return -np.sqrt(amp ** 2 * dt * f.sum() * 2 / N) * 100 * (80 / (N * dt))


# ---- replay fuzz: random job lists for replay.scatter_episodes -------------------------------------------------------------------------
FUZZ_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513]          # + T, the whole staged episode
FUZZ_CAPS = [1, 7, 63, 255, 256, 257, 1000]


def fuzz_staged(E, T, seed):
    """staged episodes [E, T, 20] as uint32: random bit patterns (NaN payloads, denormals, -0.0 ...), the cost column of episode e flagged
    with density (0, 0.02, 0.5, 1)[e % 4] -- flagged cells hold 1.0, 2.0 or a NaN, the others 0.0 or -0.0"""
    rs = np.random.RandomState(seed)
    st = rs.randint(0, 2 ** 32, size=(E, T, ROW), dtype=np.uint64).astype(np.uint32)
    on = np.array([1.0, 2.0, np.nan], np.float32).view(np.uint32)
    off = np.array([0.0, -0.0], np.float32).view(np.uint32)
    for e in range(E):
        flag = rs.rand(T) < (0.0, 0.02, 0.5, 1.0)[e % 4]
        st[e, :, 19] = np.where(flag, on[rs.randint(0, 3, T)], off[rs.randint(0, 2, T)])
    return st


def fuzz_round(rs, n_rings, caps, E, T):
    """one launch: for every ring a list of 1 .. 5 jobs (episode, length, cost_only), lengths half from FUZZ_LENGTHS + [T], half uniform"""
    out = []
    for r in range(n_rings):
        jobs = []
        for _ in range(rs.randint(1, 6)):
            n = int((FUZZ_LENGTHS + [T])[rs.randint(0, len(FUZZ_LENGTHS) + 1)]) if rs.rand() < 0.5 else int(rs.randint(0, T + 1))
            jobs.append((int(rs.randint(0, E)), n, bool(rs.rand() < 0.4)))
        out.append(jobs)
    return out


def fuzz_caps(rs, n_rings):
    """ring capacities: the edge list in turn, then 2 .. 3000 at random"""
    return [FUZZ_CAPS[r] if r < len(FUZZ_CAPS) else int(rs.randint(2, 3001)) for r in range(n_rings)]


def fuzz_classes(staged, cap, position, jobs):
    """what a ring's job list of one launch exercises -> set of class names; mirrors the skip rule of replay.scatter_episodes
    (a rank survives iff fewer than `capacity` rows follow it on its ring in this launch)"""
    cls = set()
    counts = [len(taken_rows(staged[e, :n], c)) for e, n, c in jobs]
    total, start = sum(counts), 0
    cls.add('ring_smaller_than_total' if cap < total else 'ring_holds_total')
    if cap < 64:
        cls.add('ring_below_wavefront')
    if len(jobs) > 1:
        cls.add('several_jobs')
    for (e, n, c), k in zip(jobs, counts):
        skip = min(max(total - cap - start, 0), k)
        cls.add('len_%d' % n if n in FUZZ_LENGTHS or n == staged.shape[1] else 'len_other')
        if c:
            cls.add('cost_none' if k == 0 and n > 0 else 'cost_all' if k == n and n > 0 else 'cost_some')
        if skip and skip < k:
            cls.add('skip_mid_wave' if skip % 64 else 'skip_on_wave_edge')
        if k and skip >= k:
            cls.add('skip_everything')
        if k - skip > 0 and (position + start + skip) % cap + (k - skip) > cap:
            cls.add('wraps')
        if n > 256 and c and 0 < k:
            cls.add('cost_across_blocks')
        start += k
        if e > 0:
            cls.add('episode_gt0')
    return cls


FUZZ_REQUIRED = (['len_%d' % n for n in FUZZ_LENGTHS] + ['len_other', 'cost_none', 'cost_all', 'cost_some', 'skip_mid_wave', 'skip_everything',
                 'wraps', 'cost_across_blocks', 'episode_gt0', 'ring_smaller_than_total', 'ring_holds_total', 'ring_below_wavefront',
                 'several_jobs'])


FUZZ_SEED, FUZZ_E, FUZZ_T, FUZZ_RINGS = 11, 24, 700, 220


def fuzz_plan():
    """-> (staged u32 [E, T, 20], capacities [R], launches): four launches of (ring ids, job list per ring) -- every ring, every ring again
    (partly filled or wrapped by then), and two subsets; 620 job lists in all, more than 500 jobs in the first launch"""
    rs = np.random.RandomState(FUZZ_SEED)
    staged = fuzz_staged(FUZZ_E, FUZZ_T, FUZZ_SEED + 1)
    caps = fuzz_caps(rs, FUZZ_RINGS)
    launches = []
    for ids in (range(FUZZ_RINGS), range(FUZZ_RINGS), range(0, 60), range(100, FUZZ_RINGS)):
        ids = list(ids)
        launches.append((ids, fuzz_round(rs, len(ids), [caps[r] for r in ids], FUZZ_E, FUZZ_T)))
    return staged, caps, launches

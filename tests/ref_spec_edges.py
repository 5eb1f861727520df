"""The in-kernel reference generator (include/serl_amd.h serl_ref_spec; det_cospi / serl_ref_channel / serl_ref_generate in
serl_amd/csrc/rollout_device.h) at its edges: the grid of specs, a high-precision reference, the tolerance.  No GPU.

The generator is compiled into nine kernels (the five fused rollout families, the plain step, the auto step and both rollout kernels of
the vector env) and is the default source of training references, yet every other test feeds it one kind of spec: 4 .. 6 sorted steps,
width 2 .. 3 s, first step at 0.  EDGES is what it has not seen: 0, 1, 7 and 8 steps (SERL_REF_MAX_STEPS = 8, the unrolled loop's
length), one channel full beside an empty one, tied step times, a step time equal to an ACCUMULATED env time t_k = fl(sum of k x 0.01)
(which is not k * 0.01 for k = 6, 10 .. 14, ...) and one ulp to either side, a blend argument s on the branch points 1/4, 1/2, 3/4, 1 of
det_cospi, widths shorter than a step and longer than the gap to the next one, steps before 0 and after the end, amplitudes +-1e3, 0 and
-0.0, several trims in one batch -- and NaN in the entries past n, which the generator must not read.

Episodes are short: T_MAX = 0.6 s (61 steps; the last sample is the accumulated 0.6000000000000003, three ulp beyond t_max) and
T_MAX_GATED = 0.605 s (62 steps: the last sample t = 0.61 lies well beyond t_max); the trim gate `t <= t_max` is off at the last sample
of both and on at the one before.  Step times and widths are chosen inside that window; they are not tied to t_max.

`reference` is the literal formula of signals.SmoothedStepSequence plus the trim gate and deg -> rad in np.longdouble (64-bit mantissa):
pi to 36 digits, np.cos on longdouble.  It shares no code with det_cospi or refsignals.tabulate_specs."""
import collections
import numpy as np
from serl_amd import refsignals as rs

T_MAX = 0.6
T_MAX_GATED = 0.605
N_ENVS = 70                      # one full wavefront and a partial one: the cases are cycled over them
LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, 'np.longdouble is no wider than float64 here: the high-precision reference needs the x87 format'
PI = LD('3.14159265358979323846264338327950288')
EPS = float(np.finfo(np.float64).eps)
_T = rs.env_times(rs.n_steps_for(T_MAX_GATED))
assert rs.n_steps_for(T_MAX) == 61 and rs.n_steps_for(T_MAX_GATED) == 62 and _T[60] <= T_MAX_GATED < _T[61]
K_OFF = 6                        # an accumulated time that is not k * 0.01
assert _T[K_OFF] != K_OFF * 0.01 and _T[10] != 10 * 0.01 and _T[12] != 12 * 0.01

Case = collections.namedtuple('Case', 'name theta phi trim')


def _seq(times, amps, w):
    return rs.SmoothedStepSequence(times, amps, w)


def _alt(n, a, first=1.0):
    return [first * a * (-1.0) ** i for i in range(n)]


def _k_where(ratio, of):
    """a step index k at which fl(t_k / of(t_k)) == ratio exactly"""
    for k in range(3, 40):
        if _T[k] / of(_T[k]) == ratio:
            return k
    raise AssertionError('no sample lands on s = %r' % ratio)


_K34 = _k_where(0.75, lambda t: 4.0 * t / 3.0)
_NONE = _seq([], [], 1.0)
_TK = float(_T[K_OFF])
EDGES = [
    # ---- step counts
    Case('none', _NONE, _NONE, 0.22),
    Case('one_at_0', _seq([0.0], [5.0], 0.2), _seq([0.0], [-3.0], 0.1), 0.2106),
    Case('seven', _seq(np.arange(7) * 0.08, _alt(7, 2.0), 0.05), _seq(np.arange(7) * 0.08 + 0.01, _alt(7, 1.5, -1.0), 0.06), 0.2106),
    Case('eight', _seq(np.arange(8) * 0.07, _alt(8, 2.0), 0.04), _seq(np.arange(8) * 0.07 + 0.02, _alt(8, 3.0, -1.0), 0.05), 0.22),
    Case('eight_none', _seq(np.arange(8) * 0.07, _alt(8, 1.0, -1.0), 0.03), _NONE, 0.0),
    Case('none_eight', _NONE, _seq(np.arange(8) * 0.07 + 0.03, _alt(8, 2.5), 0.05), -0.3),
    # ---- boundaries and ordering: theta one step, phi the same time as the second step of a cut-off blend (there `>` for `>=` shows)
    Case('at_tk', _seq([_TK], [4.0], 0.1), _seq([0.0, _TK], [3.0, -2.0], 0.3), 0.2106),
    Case('below_tk', _seq([np.nextafter(_TK, -1.0)], [4.0], 0.1), _seq([0.0, np.nextafter(_TK, -1.0)], [3.0, -2.0], 0.3), 0.2106),
    Case('above_tk', _seq([np.nextafter(_TK, 1.0)], [4.0], 0.1), _seq([0.0, np.nextafter(_TK, 1.0)], [3.0, -2.0], 0.3), 0.2106),
    Case('at_k_dt', _seq([12 * 0.01], [-4.0], 0.05), _seq([0.0, 10 * 0.01], [2.0, 5.0], 0.4), 0.22),
    Case('tie2', _seq([0.1, 0.1, 0.3], [3.0, -2.0, 1.0], 0.1), _seq([0.0, 0.25, 0.25], [1.0, 6.0, -1.0], 0.15), 0.22),
    Case('tie3', _seq([0.2, 0.2, 0.2], [3.0, -5.0, 2.0], 0.1), _seq([0.0, 0.0, 0.0, 0.3], [9.0, -9.0, 1.0, 2.0], 0.2), 0.0),
    Case('first_late', _seq([0.25, 0.4], [3.0, -1.0], 0.1), _seq([0.31], [2.0], 0.5), 0.2106),
    Case('before_0', _seq([-0.05, 0.3], [4.0, 1.0], 0.2), _seq([-1.0, -0.03], [2.0, -3.0], 0.1), -0.3),
    Case('after_end', _seq([0.1, 5.0], [2.0, 50.0], 0.1), _seq([0.7], [7.0], 0.1), 0.22),
    # ---- widths
    Case('w_1e-6', _seq([0.0, 0.2, 0.4], [3.0, -3.0, 2.0], 1e-6), _seq([0.0, _TK, 0.33], [1.0, 2.0, -2.0], 1e-6), 0.2106),
    Case('w_short', _seq([0.0, 0.2, 0.4], [3.0, -3.0, 2.0], 0.004), _seq([0.105, 0.3], [2.0, -2.0], 0.0099), 0.22),
    Case('s_14_12', _seq([0.0], [7.0], 4.0 * _T[7]), _seq([0.0], [-7.0], 2.0 * _T[9]), 0.2106),
    Case('s_34_1', _seq([0.0], [7.0], 4.0 * _T[_K34] / 3.0), _seq([0.0], [-7.0], float(_T[11])), 0.0),
    Case('cut_off', _seq([0.0, float(_T[10]), float(_T[20])], [4.0, -4.0, 3.0], 0.3), _seq([0.05, 0.12, 0.2, 0.25], [2.0, -1.0, 3.0, 0.5], 0.2), 0.22),
    Case('w_1e300', _seq([0.1], [6.0], 1e300), _seq([0.0, 0.3], [2.0, -2.0], 1e300), 0.2106),
    # ---- amplitudes and trim
    Case('big', _seq(np.arange(4) * 0.15, _alt(4, 1e3), 0.1), _seq(np.arange(4) * 0.15 + 0.05, _alt(4, 1e3, -1.0), 0.12), 0.22),
    Case('zeros', _seq([0.0, 0.2, 0.4], [0.0, -0.0, 0.0], 0.1), _seq([0.1, 0.3], [-0.0, -0.0], 0.1), 0.0),
    Case('neg_trim', _seq([0.0, 0.3], [1.0, -1.0], 0.15), _seq([0.0, 0.3], [-0.0, 2.0], 0.15), -0.5),
]
NAMES = [c.name for c in EDGES]
assert len(set(NAMES)) == len(NAMES)
CHANNELS = (('n_theta', 'w_theta', 't_theta', 'a_theta'), ('n_phi', 'w_phi', 't_phi', 'a_phi'))


def specs(cases=EDGES, tail=np.nan):
    """serl_ref_spec rows of `cases`; the entries past n of every t_* / a_* array are set to `tail` AFTER ref_specs made (and checked)
    the rows: NaN by default -- a generator that read them would show"""
    rows = rs.ref_specs([c.theta for c in cases], [c.phi for c in cases], [c.trim for c in cases])
    for e in range(len(rows)):
        for nk, _, tk, ak in CHANNELS:
            n = int(rows[nk][e])
            rows[tk][e, n:] = tail
            rows[ak][e, n:] = tail
    return rs.check_specs(rows)


def cycled(n=N_ENVS, cases=EDGES, shift=0):
    """the indices into `cases` of n envs / episodes: the cases cycled, starting at `shift`"""
    return (np.arange(n) + shift) % len(cases)


def _channel_ld(seq, t):
    v, prev = np.zeros(len(t), dtype=LD), LD(0)
    for ti, a in zip(seq.times, seq.amps):
        ti, a = LD(ti), LD(a)
        s = np.minimum((t - ti) / LD(seq.w), LD(1))
        v = np.where(t >= ti, prev + (a - prev) * (1 - np.cos(PI * s)) / 2, v)
        prev = a
    return v


def reference(case, t, t_max=T_MAX):
    """The reference samples of `case` at the times t (f64, taken exactly) in np.longdouble, radians [len(t), 3]: the literal
    SmoothedStepSequence formula, the theta trim on [0, t_max], beta = 0, times pi / 180."""
    t = np.asarray(t, dtype=np.float64).astype(LD)
    th = _channel_ld(case.theta, t) + np.where((t >= 0) & (t <= LD(t_max)), LD(case.trim), LD(0))
    ph = _channel_ld(case.phi, t)
    return np.stack([th, ph, np.zeros_like(th)], axis=1) * (PI / 180)


def units(case):
    """the error unit of each column of `case` (radians): eps64 x (max |a| + |trim|) x pi / 180 per channel (phi has no trim, beta is
    exactly 0).  A channel without amplitude and trim has unit 0: it must be exact."""
    amp = lambda seq: float(np.abs(seq.amps).max()) if len(seq.amps) else 0.0
    return np.array([amp(case.theta) + abs(case.trim), amp(case.phi), 0.0]) * EPS * (np.pi / 180.0)


def error_in_units(got, case, t, t_max=T_MAX):
    """max over the samples of |got - reference| per column, in units(case); a column of unit 0 counts 0 if exact, inf if not"""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - reference(case, t, t_max)).max(axis=0).astype(np.float64)
    if not np.isfinite(np.asarray(got)).all():
        return np.inf
    u = units(case)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(u > 0, err / u, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


# ---- the tolerance ----------------------------------------------------------------------------------------------------------------------
# Absolute error against `reference`, in units(case).  Calibrated on the CPU with refsignals.tabulate_specs (the float64 host restatement
# of the kernels' arithmetic, to which every kernel is held bit for bit) over EDGES at both t_max; tests/test_ref_spec_host.py asserts it.
# TOL = 4 x the worst case, the margin of tests/td3_64.py and tests/distill64.py: it covers the last place of another evaluation order of
# the polynomials, no more.
TOL = 5.9
# Measured (units; identical at t_max = 0.6 and 0.605): worst 1.462 ('eight'), then 1.456 ('none_eight'), 1.373 ('before_0'), 1.325
# ('cut_off'), 1.291 ('above_tk'), 1.221 ('seven'), 1.166 ('at_tk'), 1.069 ('big': +-1e3 deg); at most 0.82 for the single steps whose
# blend argument lands on 1/4, 1/2, 3/4, 1; 0.4 at width 1e-6; 0.04 for the trim alone (one rounding of the deg -> rad product); 'zeros'
# exact.  4 x 1.462 = 5.85.  The planted mistakes of tests/test_ref_spec_host.py are wrong by whole levels: `>` for `>=` 4.1e15 .. 6.4e15
# units ('at_tk', 'tie3', 'cut_off': a step time on a sample), prev not updated 1.8e15 .. 4.5e15 (every case with two steps), the blend
# not clamped 3.2e15 and up (every case whose blend completes inside the episode).


def check(got, case, t, t_max=T_MAX, what=''):
    e = error_in_units(got, case, t, t_max)
    assert e <= TOL, '%s %s: %.3g units from the longdouble reference > %.3g' % (what, case.name, e, TOL)
    return e


# ---- planted mistakes -------------------------------------------------------------------------------------------------------------------
BUGS = ('gt', 'prev', 'clamp')


def generator(row, t, t_max, bug=None):
    """The kernels' generator, scalar and literal (serl_ref_channel / serl_ref_generate), on one serl_ref_spec row at the times t -> f64
    [len(t), 3].  bug=None is refsignals.tabulate_specs bit for bit (the host test asserts it, and it may read rows that check_specs
    refuses); 'gt': `t > tt[i]` for `>=`; 'prev': prev not updated (it stays 0); 'clamp': the blend argument not clamped at 1."""
    out = np.zeros((len(t), 3))
    for k, tk in enumerate(np.asarray(t, dtype=np.float64)):
        for c, (nk, wk, tkk, ak) in enumerate(CHANNELS):
            ti = a = prev = 0.0
            on = False
            for i in range(int(row[nk])):
                tt = float(row[tkk][i])
                if (tk > tt) if bug == 'gt' else (tk >= tt):
                    if bug != 'prev':
                        prev = a if on else 0.0
                    ti, a, on = tt, float(row[ak][i]), True
            v = 0.0
            if on:
                with np.errstate(all='ignore'):
                    s = np.float64(tk - ti) / np.float64(row[wk])
                    if bug != 'clamp':
                        s = s if s < 1.0 else np.float64(1.0)
                    v = prev + (a - prev) * (1.0 - float(rs.det_cospi(s))) / 2.0
            if c == 0:
                v = v + (float(row['trim_deg']) if 0.0 <= tk <= t_max else 0.0)
            out[k, c] = v * (np.pi / 180.0)
    return out

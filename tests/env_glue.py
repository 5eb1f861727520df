"""The env step around the dynamics call, restated literally from CitationEnv.reset / .step (envs/phlabenv.py:401-482 with :62-73
scale_action, :347-399 calc_error / get_reward / get_cost / incremental_control / check_bounds) and the actuator-fault wrappers
(envs/{be,jr,sa,se}/citation.py:71-79), and SCENARIOS that drive it through every branch and onto every threshold.  No GPU.

The same glue is written out by hand in about a dozen kernels (rollout_variant.inc, rollout_wave.inc, rollout_half.inc, three copies in
rollout_team.inc, rollout_team_half.inc, four in venv_variant.inc, and the one-wavefront-per-env copies of venv_wave.inc -- reset, step,
auto step -- and venv_wave_rollout.inc) and in oracle/rollout_ref.c, all from one reading of the reference.
(A few of its statements -- fault row, sensor add, observation -- are shared through serl_amd/csrc/env_glue.h in the env kernels; this file and the
oracle never include it.)
`GlueEnv` is a second reading: Python floats (IEEE f64, one rounding per operation, no contraction) and np.float32 only, around
oracle.dynamics.CitationDynamics(build, short_libm=True).  It shares no code with oracle/rollout_ref.c, oracle/rollout.py or serl_amd
(the scenario builders use refsignals.tabulate_specs for generated references and oracle.rollout.activation for a bias-only actor's
output, both held bit for bit to the kernels by other tests).

Sensor noise is added to x[0, 1, 2, 4, 5, 6, 7] after the dynamics step and does not feed back into it, so with open-loop commands
theta, phi and alpha can be put exactly on a threshold, and one ulp beyond it, at a chosen step (`_place`).  x[3] (V) and x[9] (h) take
no noise: `V < V0 / 3` and `h < 50` cannot be put on their thresholds, and `<=` for `<` there is not distinguishable (BUGS_BLIND).

Speed cost: `V < V0 / 3` is NOT reached.  Held climbs at 40 .. 59 deg on h2000_v90 and h10000_v90 were flown for 8 000 steps by the CPU
oracle (`speed_search`, run by hand): the lowest speed was 32.3 m/s against V0 / 3 = 30 (h2000_v90 at 59 deg; SPEED_SEARCH below).  The
term is covered on its false side only; V0 is not faked."""
import math
import numpy as np

PI = 3.14159265358979323846
D2R, R2D = PI / 180.0, 180.0 / PI
DT = 0.01
MAX_THETA, MAX_PHI = 60.0 * D2R, 75.0 * D2R      # np.deg2rad(60.), np.deg2rad(75.) (phlabenv.py:211-212)
ALPHA_COST = 11.0                                 # degrees (:371)
PHI_COST = 0.75 * MAX_PHI                         # radians, compared with degrees (:372, the reference's quirk)
H_MIN = 50.0
INF = float('inf')
ATTITUDE, SYMMETRIC, FULL = 0, 1, 2
NOISE_COLS = (0, 1, 2, 4, 5, 6, 7)                # envs/noise/citation.py:71-82
TERMS = ('time', 'theta', 'phi', 'h')
COSTS = ('alpha', 'phi', 'V')
# (elev_gain, elev_clip, ail_clip, rudder_jam_on, rudder_jam): envs/{be,jr,sa,se}/citation.py:71-79
FAULTS = {
    None: (1.0, INF, INF, 0.0, 0.0),
    'be': (0.3, INF, INF, 0.0, 0.0),
    'jr': (1.0, INF, INF, 1.0, 15 * 3.14159 / 180),
    'sa': (1.0, INF, float(np.deg2rad(1)), 0.0, 0.0),
    'se': (1.0, float(np.deg2rad(2.5)), INF, 0.0, 0.0),
    'gain_clip': (0.3, float(np.deg2rad(2.5)), INF, 0.0, 0.0),      # no env of the reference: the ABI's row applies the gain, then the clip
}

# planted mistakes (keyword `bug` of GlueEnv): slips a kernel copy could make; tests/test_env_glue_host.py proves SCENARIOS notices each
BUGS = ('gt_time', 'ge_theta', 'ge_phi', 'ge_alpha_cost', 'ge_phi_cost', 't_after', 'div3', 'noclip', 'penalty_sign', 'gain_after_clip',
        'nojam', 'noise_x3', 'rate_nodt', 'maxphi_deg', 'no_last_u', 'scale_f64')
# `<=` for `<` in `h < 50` and `V < V0 / 3`: x[9] and x[3] take no sensor noise, so no scenario can put them on 50.0 or V0 / 3 exactly
BUGS_BLIND = ('le_h', 'le_V')


def fault_row(fault):
    """the 8 doubles of serl_fault_row"""
    f = FAULTS[fault] if (fault is None or isinstance(fault, str)) else tuple(fault)
    return [float(v) for v in f[:5]] + [0.0, 0.0, 0.0]


def dims(config, incremental):
    A = 1 if config == SYMMETRIC else 3
    nx = {ATTITUDE: 4, SYMMETRIC: 1, FULL: 10}[config]
    return A + nx + (A if incremental else 0), A


def _clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


class GlueEnv:
    """CitationEnv(configuration, mode) on one dynamics build.  ref: f64 [T, 3] (the reference at the env's step k, radians);
    sensor_noise: f64 [T + 1, 7] (entry 0 at reset, k + 1 at step k); err0 [3] / tick0: carried error and model clock."""

    def __init__(self, build='h2000_v90', config=ATTITUDE, incremental=False, fault=None, ref=None, sensor_noise=None, t_max=20.0,
                 err0=None, tick0=None, bug=None):
        from oracle.dynamics import CitationDynamics
        assert bug is None or bug in BUGS + BUGS_BLIND, bug
        self.dyn = CitationDynamics(build, short_libm=True)
        self.config, self.incr, self.bug = config, bool(incremental), bug
        self.S, self.A = dims(config, incremental)
        self.fault = fault_row(fault)
        self.ref = None if ref is None else np.asarray(ref, dtype=np.float64)
        self.sn = None if sensor_noise is None else np.asarray(sensor_noise, dtype=np.float64)
        self.t_max = float(t_max)
        self.err = [0.0, 0.0, 0.0] if err0 is None else [float(v) for v in err0]
        self.tick0 = tick0
        self.bound = (25.0 if self.incr else 10.0) * D2R
        self.scaler = [6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0]      # :226-232

    # ---- pieces ----
    def _plant(self, u):
        """the fault wrapper around citation.step: what the plant executes for the env's command u"""
        gain, eclip, aclip, jam_on, jam = self.fault[:5]
        cmd = [0.0] * 10
        if self.bug == 'gain_after_clip':
            cmd[0] = _clip(u[0], -eclip, eclip) * gain
        else:
            cmd[0] = _clip(u[0] * gain, -eclip, eclip)
        cmd[1] = _clip(u[1], -aclip, aclip)
        cmd[2] = jam if (jam_on != 0.0 and self.bug != 'nojam') else u[2]
        return cmd

    def _sense(self, x, j):
        if self.sn is not None:
            cols = (0, 1, 2, 3, 5, 6, 7) if self.bug == 'noise_x3' else NOISE_COLS
            for c, i in enumerate(cols):
                x[i] = x[i] + float(self.sn[j, c])
        return x

    def _obs(self, x):
        o = [self.err[i] for i in range(self.A)]
        o += [x[i] for i in {ATTITUDE: (0, 1, 2, 4), SYMMETRIC: (1,), FULL: tuple(range(10))}[self.config]]
        if self.incr:
            o += [0.0] * self.A if self.bug == 'no_last_u' else [self.last_u[i] for i in range(self.A)]
        return o

    # ---- reset / step ----
    def reset(self):
        self.t, self.k = 0.0, 0
        self.dyn.initialize()
        if self.tick0 is not None:      # initialize() of the reference leaves the model clock running
            self.dyn.L.cit_set_clock(self.dyn.buf, int(self.tick0))
        self.last_u = [0.0, 0.0, 0.0]
        self.x = self._sense([float(v) for v in self.dyn.step(np.array(self._plant(self.last_u)))], 0)
        self.V0 = self.x[3]
        self.obs = self._obs(self.x)
        return list(self.obs)

    def step(self, action, noise=None):
        """action: np.float32 [A] (scaled in f32, then f64), or f64 [A] (scaled in f64, not clipped); noise f64 [A]: added to the f32 action,
        the sum clipped to [-1, 1] and scaled in f64 (base/core/agent.py:90-93).  -> dict of the step"""
        A, low, high = self.A, -self.bound, self.bound
        last_obs = list(self.obs)
        a = np.asarray(action)
        assert a.shape == (A,) and a.dtype in (np.float32, np.float64)
        act32, scl = [], [0.0, 0.0, 0.0]
        for i in range(A):
            if noise is not None:
                assert a.dtype == np.float32
                an = _clip(float(a[i]) + float(noise[i]), -1.0, 1.0)
                scl[i] = low + 0.5 * (an + 1.0) * (high - low)
                act32.append(np.float32(an))
            elif a.dtype == np.float64:
                scl[i] = low + 0.5 * (float(a[i]) + 1.0) * (high - low)
                act32.append(np.float32(a[i]))
            elif self.bug == 'scale_f64':
                scl[i] = low + 0.5 * (float(a[i]) + 1.0) * (high - low)
                act32.append(a[i])
            else:
                s = np.float32(0.5) * (a[i] + np.float32(1.0))
                assert s.dtype == np.float32
                scl[i] = low + float(s) * (high - low)
                act32.append(a[i])
        if self.incr:
            u = [self.last_u[i] + (scl[i] if self.bug == 'rate_nodt' else scl[i] * DT) for i in range(3)]
        else:
            u = list(scl)
        cmd = self._plant(u)
        x = self._sense([float(v) for v in self.dyn.step(np.array(cmd))], self.k + 1)
        self.x = x
        # reward
        rk = [float(v) for v in self.ref[self.k]]
        ctrl = [x[7], x[6], x[5]]
        scaled = []
        for i in range(A):
            self.err[i] = rk[i] - ctrl[i]
            scaled.append(self.scaler[i] * self.err[i])
        rsum = 0.0
        for i in range(A):
            rsum = rsum + abs(scaled[i] if self.bug == 'noclip' else _clip(scaled[i], -1.0, 1.0))
        reward = -rsum / (3.0 if self.bug == 'div3' else float(A))
        # cost
        bug = self.bug
        phi_cost = 0.75 * 75.0 if bug == 'maxphi_deg' else PHI_COST
        ra, rp = R2D * abs(x[4]), R2D * abs(x[6])
        costs = {'alpha': ra >= ALPHA_COST if bug == 'ge_alpha_cost' else ra > ALPHA_COST,
                 'phi': rp >= phi_cost if bug == 'ge_phi_cost' else rp > phi_cost,
                 'V': x[3] <= self.V0 / 3.0 if bug == 'le_V' else x[3] < self.V0 / 3.0}
        cost = int(any(costs.values()))
        self.last_u = u
        self.obs = self._obs(x)
        # bounds, at the pre-increment t
        t = self.t + DT if bug == 't_after' else self.t
        terms = {'time': t > self.t_max if bug == 'gt_time' else t >= self.t_max,
                 'theta': abs(x[7]) >= MAX_THETA if bug == 'ge_theta' else abs(x[7]) > MAX_THETA,
                 'phi': abs(x[6]) >= MAX_PHI if bug == 'ge_phi' else abs(x[6]) > MAX_PHI,
                 'h': x[9] <= H_MIN if bug == 'le_h' else x[9] < H_MIN}
        fin = any(terms.values())
        if fin:
            penalty = -1.0 / DT * (self.t_max - t) * 2.0
            reward += -penalty if bug == 'penalty_sign' else penalty
        self.t += DT
        self.k += 1
        done = fin or self.k >= len(self.ref)
        row = np.array(last_obs + [float(v) for v in act32] + self.obs + [reward, 1.0 if fin else 0.0, float(cost)]).astype(np.float32)
        return dict(obs=list(self.obs), x=list(x), u=list(u), cmd=cmd[:3], ref=rk, reward=reward, cost=cost, fin=fin, done=done, t=self.t,
                    row=row, terms=terms, costs=costs, scaled=scaled)


def fly(sc, bug=None, steps=None):
    """One episode of scenario `sc` -> dict: per-step arrays (the oracle's layout: actions = the executed command u [n, 3], states [n, 12],
    rewards [n], transitions [n, 2 S + A + 3] f32, obs [n, S], refs, t, cost, fin, terms [n, 4] / costs [n, 3] bool, cmd [n, 3], scaled),
    obs0, fitness (summed in step order), length_steps (negative: the table ended first), length_t, cost_steps, and err / tick to carry."""
    env = GlueEnv(sc['build'], sc['config'], sc['incremental'], sc['fault'], sc['ref'], sc.get('sensor_noise'), sc['t_max'],
                  sc.get('err0'), sc.get('tick0'), bug)
    obs0 = env.reset()
    A = env.A
    rec = {k: [] for k in ('actions', 'states', 'rewards', 'transitions', 'obs', 'refs', 't', 'cost', 'fin', 'terms', 'costs', 'cmd', 'scaled')}
    fitness, cost_steps = 0.0, 0
    n_max = len(sc['ref']) if steps is None else steps
    for k in range(n_max):
        if sc['kind'] == 'f32':
            r = env.step(np.asarray(sc['act32'][k, :A], dtype=np.float32))
        elif sc['kind'] == 'f64':
            r = env.step(np.asarray(sc['act64'][k, :A], dtype=np.float64))
        else:
            r = env.step(np.asarray(sc['actor_out'][:A], dtype=np.float32), noise=sc['noise'][k, :A])
        for key, v in (('actions', r['u']), ('states', r['x']), ('rewards', r['reward']), ('transitions', r['row']), ('obs', r['obs']),
                       ('refs', r['ref']), ('t', r['t']), ('cost', r['cost']), ('fin', r['fin']), ('cmd', r['cmd']),
                       ('terms', [r['terms'][n] for n in TERMS]), ('costs', [r['costs'][n] for n in COSTS]),
                       ('scaled', r['scaled'] + [0.0] * (3 - A))):
            rec[key].append(v)
        fitness += r['reward']
        cost_steps += r['cost']
        if r['done']:
            break
    out = {k: np.array(v) for k, v in rec.items()}
    n = len(out['rewards'])
    out.update(obs0=np.array(obs0), fitness=fitness, length_steps=n if out['fin'][-1] else -n, length_t=env.t, cost_steps=cost_steps,
               err=list(env.err), n=n, V0=env.V0)
    return out


# ---- scenarios ------------------------------------------------------------------------------------------------------------------------
def _ulps(v, n):
    for _ in range(abs(n)):
        v = math.nextafter(v, INF if n > 0 else -INF)
    return v


def _solve(x, want, reach=3):
    """an addend s with fl(x + s) == want, searched among the doubles around want - x; None if there is none"""
    s0 = want - x
    for n in sorted(range(-reach, reach + 1), key=abs):
        s = _ulps(s0, n)
        if x + s == want:
            return s
    return None


def _scenario(name, ends, costs=(), build='h2000_v90', config=ATTITUDE, incremental=False, fault=None, t_max=20.0, T=None, kind='noise',
              act=None, actor_out=None, bias=None, ref=None, sensor_noise=None, err0=None, tick0=None, note=''):
    """act [T, 3]: the action script -- kind 'noise': action noise added to the f32 actor output `actor_out` (0: the zero-weight actor; else the
    bias-only actor of `bias`) and clipped; 'f32' / 'f64': actions fed to the step kernels as they are (no fused kernel can fly these)."""
    act = np.asarray(act, dtype=np.float64)
    T = len(act) if T is None else T
    assert act.shape == (T, 3)
    sc = dict(name=name, ends=ends, costs=tuple(costs), build=build, config=config, incremental=incremental, fault=fault, t_max=float(t_max),
              kind=kind, err0=err0, tick0=tick0, note=note,
              ref=np.zeros((T, 3)) if ref is None else np.ascontiguousarray(ref, dtype=np.float64),
              sensor_noise=None if sensor_noise is None else np.ascontiguousarray(sensor_noise, dtype=np.float64))
    assert sc['ref'].shape == (T, 3)
    if kind == 'f32':
        sc['act32'] = act.astype(np.float32)
    elif kind == 'f64':
        sc['act64'] = act
    else:
        sc['noise'] = act
    sc['actor_out'] = np.zeros(3, np.float32) if actor_out is None else np.asarray(actor_out, dtype=np.float32)
    sc['bias'] = np.zeros(3, np.float32) if bias is None else np.asarray(bias, dtype=np.float32)
    return sc


def _const(T, e=0.0, a=0.0, r=0.0):
    return np.tile(np.array([e, a, r], dtype=np.float64), (T, 1))


def n_steps_for(t_max):
    """steps of an episode that runs into t_max: the first k whose accumulated pre-increment t reaches t_max, inclusive"""
    t, k = 0.0, 0
    while True:
        k += 1
        if t >= t_max:
            return k
        t += DT


def _place(sc, base, k, col, want):
    """sensor noise at step k (table entry k + 1) that puts x[col] on `want` exactly, given the episode flown without it (`base`: the noise
    does not feed back) -> the scenario with the table, or None where no addend lands exactly"""
    s = _solve(float(base['states'][k, col]), want)
    if s is None:
        return None
    sn = np.zeros((len(sc['ref']) + 1, 7))
    sn[k + 1, NOISE_COLS.index(col)] = s
    return dict(sc, sensor_noise=sn)


def _product_pair(factor, thr):
    """(v, w): adjacent doubles with fl(factor * v) == thr (the largest such v) and fl(factor * w) > thr"""
    v = thr / factor
    while factor * v <= thr:
        v = math.nextafter(v, INF)
    w = v
    v = math.nextafter(w, -INF)
    assert factor * v == thr and factor * w > thr, 'no double v with fl(%r * v) == %r' % (factor, thr)
    return v, w


def _twins(name, base, k, col, on, above, term, is_cost, sign=1.0):
    """two scenarios: x[col] exactly `on` the threshold at step k (must not fire) and on `above` (must fire)"""
    flown_ = fly(dict(base, sensor_noise=None), steps=k + 12)
    for kk in range(k, k + 12):      # the first step at which both values can be hit exactly
        a = _place(dict(base, name=name + '_on'), flown_, kk, col, sign * on)
        b = _place(dict(base, name=name + '_above'), flown_, kk, col, sign * above)
        if a is not None and b is not None:
            break
    else:
        raise AssertionError('%s: no step with an exact hit of both values' % name)
    ka = kb = kk
    a.update(twin=(term, is_cost, ka, False))
    b.update(twin=(term, is_cost, kb, True))
    if is_cost:
        b['costs'] = tuple(sorted(set(b['costs']) | {term}))
    else:
        b['ends'] = term
    return [a, b]


def _reward_clip(T=24):
    """the reference of one step set so that scaler[i] * err[i] is exactly 1, nextafter(1) and -1, for each channel in turn (steps 2 .. 10)"""
    sc = _scenario('reward_clip', 'table', act=_const(T), note='scaler * err on 1, nextafter(1), -1 per channel')
    base = fly(sc)
    ref = sc['ref'].copy()
    scaler = [6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0]
    marks = []
    k = 2
    for i, col in enumerate((7, 6, 5)):
        for want in (1.0, math.nextafter(1.0, INF), -1.0):
            while True:
                x = float(base['states'][k, col])
                r0 = want / scaler[i] + x
                hit = [r for r in (_ulps(r0, n) for n in range(-40, 41)) if scaler[i] * (r - x) == want]
                if hit:
                    break
                k += 1
            ref[k, i] = hit[0]
            marks.append((k, i, want))
            k += 1
    assert k < T
    return dict(sc, ref=ref, marks=marks)


def _dive_script(T=1900):
    """elevator = clip(3 (theta - theta_t) + q, +-10 deg) holding theta_t = -55 deg: flown once in closed loop here, then frozen as a table"""
    from oracle.dynamics import CitationDynamics
    dyn = CitationDynamics('h2000_v90', short_libm=True)
    x = dyn.step(np.zeros(10))
    act = np.zeros((T, 3))
    for k in range(T):
        de = _clip(3.0 * (float(x[7]) - -55.0 * D2R) + float(x[1]), -10.0 * D2R, 10.0 * D2R)
        a = _clip(de / (10.0 * D2R), -1.0, 1.0)
        act[k, 0] = a
        cmd = np.zeros(10)
        cmd[0] = -10.0 * D2R + 0.5 * (a + 1.0) * (20.0 * D2R)
        x = dyn.step(cmd)
    return act


def speed_search(build='h10000_v90', hold_deg=59.0, steps=8000):
    """the lowest V of a climb held at hold_deg by the same law as the dive (run by hand; the figures are in SPEED_SEARCH)"""
    from oracle.dynamics import CitationDynamics
    dyn = CitationDynamics(build, short_libm=True)
    x = dyn.step(np.zeros(10))
    V0, vmin, n = float(x[3]), float(x[3]), 0
    for k in range(steps):
        de = _clip(3.0 * (float(x[7]) - hold_deg * D2R) + float(x[1]), -10.0 * D2R, 10.0 * D2R)
        cmd = np.zeros(10)
        cmd[0] = de
        x = dyn.step(cmd)
        n += 1
        vmin = min(vmin, float(x[3]))
        if abs(x[7]) > MAX_THETA or abs(x[6]) > MAX_PHI or x[9] < H_MIN:
            break
    return V0, vmin, n


# lowest V [m/s] in 8 000 steps of a held climb, against V0 / 3 = 30.0 (speed_search; V0 = 90 in both builds)
SPEED_SEARCH = {('h2000_v90', 40): 44.972, ('h2000_v90', 50): 38.196, ('h2000_v90', 55): 34.854, ('h2000_v90', 58): 32.897,
                ('h2000_v90', 59): 32.257, ('h10000_v90', 40): 75.980, ('h10000_v90', 59): 75.980}      # (h10000_v90: the elevator saturates, the climb is never reached)

_SCENARIOS = None


def scenarios():
    """the list, built once per process (the closed-loop dive and the threshold placements fly the CPU oracle)"""
    global _SCENARIOS
    if _SCENARIOS is not None:
        return _SCENARIOS
    from oracle import rollout as R
    L = []
    add = L.append
    # ---- open-loop commands of exactly +-1 to each terminator and cost term (the issue's table; t_max beyond the crossing)
    add(_scenario('nose_up', 'theta', ('alpha',), act=_const(760, e=-1.0), note='alpha cost k = 57; theta > 60 deg'))
    add(_scenario('nose_down', 'theta', act=_const(420, e=1.0), note='theta < -60 deg'))
    add(_scenario('aileron_pos', 'phi', ('phi',), act=_const(200, a=1.0), note='phi cost k = 10; |phi| > 75 deg'))
    add(_scenario('aileron_neg', 'phi', ('phi',), act=_const(200, a=-1.0)))
    add(_scenario('rudder', 'phi', ('phi',), act=_const(1060, r=1.0), note='phi cost k = 85; |phi| > 75 deg k = 1018'))
    add(_scenario('dive', 'h', act=_dive_script(), t_max=25.0, note='theta held at -55 deg: h < 50 and no other terminator first'))
    add(_scenario('zero_table', 'table', act=_const(300), note='zero command: the table ends first'))
    for b in ('cg_timed', 'gust', 'test', 'ice'):
        add(_scenario('aileron_' + b, 'phi', ('phi',), build=b, act=_const(260, a=1.0)))
    # ---- the other configurations: theta and the time-out
    for cfg, tag in ((SYMMETRIC, 'sym'), (FULL, 'full')):
        add(_scenario('nose_down_' + tag, 'theta', config=cfg, act=_const(420, e=1.0)))
        add(_scenario('timeout_' + tag, 'time', ('phi',) if cfg == FULL else (), config=cfg, t_max=0.6, act=_const(80, e=0.25, a=-0.1, r=0.05),
                      ref=_const(80, 0.02, -0.01, 0.001), note='t = 0.6000000000000003 first reaches t_max = 0.6: penalty residue'))
        add(_scenario('timeout_%s_incr' % tag, 'time', ('phi',) if cfg == FULL else (), config=cfg, incremental=True, t_max=0.6, act=_const(80, e=0.5, a=-0.5, r=0.3),
                      ref=_const(80, 0.02, -0.01, 0.001)))
    # ---- time-out endings
    add(_scenario('timeout_residue', 'time', t_max=0.6, act=_const(80, e=0.1), ref=_const(80, 0.01, 0.01, 0.0),
                  note='accumulated t reaches 0.6 from below as 0.6000000000000003: penalty -200 * (t_max - t) != 0'))
    add(_scenario('timeout_exact', 'time', t_max=0.05, act=_const(20, e=0.1), note='t == t_max exactly at k = 5: `>` for `>=` flies on'))
    tk = 0.0
    for _ in range(164):
        tk += DT
    add(_scenario('timeout_and_phi', 'phi', ('phi',), t_max=tk, act=_const(200, a=1.0), note='|phi| > 75 deg and t >= t_max on one step'))
    # ---- actions: exactly +-1, noise sums that clip, a bias-only actor (f32 scaling), f32 / f64 fed to the step kernels, beyond +-1
    rng = np.random.default_rng(3)
    bias = np.array([0.3, -0.7, 1.9], np.float32)
    out = R.activation('tanh', bias)
    add(_scenario('bias_actor', 'table', ('phi',), act=np.zeros((60, 3)), kind='f32', T=60, actor_out=out, bias=bias))
    L[-1]['act32'] = np.tile(out, (60, 1))      # (what the bias-only actor outputs at every step: the f32 path of the fused kernels)
    mix = rng.uniform(-1.6, 1.6, (60, 3)) * np.array([0.5, 0.3, 0.3])
    mix[5], mix[6], mix[7] = (1.0, -1.0, 1.0), (-1.0, 1.0, -1.0), (3.0, -3.0, 1.5)
    add(_scenario('noise_clips', 'table', ('phi',), act=mix, actor_out=out, bias=bias, note='f32 actor output + noise, sums beyond +-1 clipped'))
    add(_scenario('f32_script', 'table', (), act=rng.uniform(-1, 1, (60, 3)) * 0.4, kind='f32', note='step kernels only'))
    beyond = rng.uniform(-1.25, 1.25, (60, 3)) * np.array([1.2, 0.8, 0.8])
    add(_scenario('f64_beyond', 'table', ('phi',), act=beyond, kind='f64', note='step kernels only: f64 actions outside [-1, 1], not clipped'))
    add(_scenario('f32_beyond', 'table', ('phi',), act=beyond, kind='f32', note='step kernels only'))
    # ---- faults: a script on which the gain, the clip or the jam bites
    wave = np.stack([np.sin(np.arange(120) * 0.11), np.sin(np.arange(120) * 0.07 + 1.0), 0.5 * np.cos(np.arange(120) * 0.05)], axis=1)
    for f in ('be', 'jr', 'sa', 'se', 'gain_clip'):
        add(_scenario('fault_' + f, 'table', ('phi',), fault=f, act=wave * 0.9))
    add(_scenario('fault_se_full_incr', 'table', ('phi',), fault='se', config=FULL, incremental=True, act=wave))
    # ---- incremental control: a rate script that drives last_u past +-10 deg (25 deg/s for 0.5 s and back)
    rate = np.zeros((140, 3))
    rate[:60] = (1.0, -1.0, 0.5)
    rate[60:] = (-1.0, 1.0, -0.5)
    add(_scenario('incr_rates', 'table', ('phi',), incremental=True, act=rate, note='last_u past +-10 deg; not clipped by the env'))
    add(_scenario('incr_sym', 'table', config=SYMMETRIC, incremental=True, act=rate[:100], ref=_const(100, 0.3, 0.0, 0.0),
                  note='A = 1: reward / 1, one error, scaler * err beyond the clip'))
    # ---- carried error, model clock, generated references, sensor noise on every column
    from serl_amd import refsignals as rs
    spec = rs.ref_specs([rs.SmoothedStepSequence([0.0, 0.2, 0.4], [5.0, -3.0, 2.0], 0.15)], [rs.SmoothedStepSequence([0.1, 0.3], [4.0, -4.0], 0.1)], 0.2106)
    sn = rng.normal(0, 1, (n_steps_for(0.6) + 1, 7)) * np.array([6e-4, 6e-4, 6e-4, 4e-10, 3e-4, 4e-3, 4e-3])
    add(_scenario('spec_noise_carry', 'time', ('phi',), build='gust', t_max=0.6, act=wave[:n_steps_for(0.6)] * 0.5, sensor_noise=sn,
                  ref=rs.tabulate_specs(spec, 0.6)[0], err0=[0.01, -0.02, 0.003], tick0=1990,
                  note='serl_ref_spec row, noise on all seven columns, err0, the gust 10 steps away on the model clock'))
    L[-1]['spec'] = spec
    # ---- exact thresholds by sensor noise: on the threshold (does not fire), one ulp beyond (fires)
    zero = _scenario('thr', 'table', act=_const(40))
    up = math.nextafter
    L += _twins('theta_pos', zero, 5, 7, MAX_THETA, up(MAX_THETA, INF), 'theta', False)
    L += _twins('theta_neg_full', dict(zero, config=FULL), 6, 7, MAX_THETA, up(MAX_THETA, INF), 'theta', False, sign=-1.0)
    L += _twins('theta_pos_sym', dict(zero, config=SYMMETRIC), 6, 7, MAX_THETA, up(MAX_THETA, INF), 'theta', False)
    L += _twins('phi_pos', zero, 7, 6, MAX_PHI, up(MAX_PHI, INF), 'phi', False)
    L += _twins('phi_neg', zero, 8, 6, MAX_PHI, up(MAX_PHI, INF), 'phi', False, sign=-1.0)
    for s in L[-4:]:
        s['costs'] = ('phi',)      # 75 deg is far beyond the cost threshold
    L += _twins('alpha_cost', zero, 9, 4, *_product_pair(R2D, ALPHA_COST), 'alpha', True)
    L += _twins('alpha_cost_neg', zero, 9, 4, *_product_pair(R2D, ALPHA_COST), 'alpha', True, sign=-1.0)
    L += _twins('phi_cost', zero, 10, 6, *_product_pair(R2D, PHI_COST), 'phi', True)
    L += _twins('phi_cost_neg', zero, 10, 6, *_product_pair(R2D, PHI_COST), 'phi', True, sign=-1.0)
    L.append(_reward_clip())
    names = [s['name'] for s in L]
    assert len(set(names)) == len(names)
    for s in L:
        s['fused'] = s['kind'] == 'noise' or s['name'] == 'bias_actor'
        s['S'], s['A'] = dims(s['config'], s['incremental'])
    _SCENARIOS = L
    return L


_FLOWN = {}


def flown(name, bug=None):
    """fly(scenario) cached per process: computed once, shared by every test, never changed"""
    if (name, bug) not in _FLOWN:
        sc = [s for s in scenarios() if s['name'] == name][0]
        _FLOWN[name, bug] = fly(sc, bug)
    return _FLOWN[name, bug]

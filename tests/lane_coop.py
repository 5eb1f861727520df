"""Shared by tests/test_lane_coop_host.py (CPU) and tests/test_gpu_lane_coop.py (GPU): the case table of the lane
kernels' WAVE-COOPERATIVE actor (rollout_variant.inc: one serl_actor_forward_wave per live lane, all 64 lanes of the wavefront working for that lane
through v_readlane and DPP row sums, around per-lane divergent env and noise code), its inputs, the CPU oracle's flight of them, the bit-for-bit
comparison and a launch through the C ABI whose every input and output lies between guard values.  A plain module (not a conftest).

Every lane-family rollout of an actor that is not hidden 32 runs that branch: `lane` (lanes_per_wave > 0), `lanern` (the same with the in-kernel
noise generator) and `laneq` (the work queue).  A case names one of the three; what it flies is compared with the oracle alone (twins can share a
mistake), at zero tolerance.  Device noise is replayed on the oracle through serl_amd.venv_noise's rows; without a GPU the host file flies the oracle
on stand-in tables of the same masks, which is all the mask conditions need.

Guard values, not guard pages: weights lie in a tensor whose row stride exceeds P, the gap and one whole row in front and behind are NaN; the
reference rows, err0, the noise tables and their row indices, the members and the generator's keys have a poisoned row or entry on either side; the
outputs start as a sentinel that entries no episode owns must keep.  Everything is an ordinary allocation and every poisoned INDEX addresses a
poisoned row inside it, so a read beside a row shows as a NaN in the comparison and nothing can fault."""
import ctypes
import functools
import itertools
import numpy as np

import actor_shapes as X

KEYS = ('fitness', 'length_steps', 'length_t', 'cost_steps', 'actions', 'states', 'rewards', 'transitions')
KERNELS = ('lane', 'lanern', 'laneq')
S72 = X._shape(72, 3)
MASK = (0, -1, 0, 0, -1)
ON, OFF = (0,) * 5, (-1,) * 5
COMPLEMENT = tuple(-1 - m for m in MASK)
SEED = 0x5EED1A9E0C0FFEE5
SD, CLIP = 0.3, 0.5
# output sentinels: finite, so that `==` finds them; tests/test_lane_coop_host.py holds them apart from everything the oracle returns
SENT_F64, SENT_F32, SENT_I32 = -7.0e300, np.float32(-7.0e30), np.int32(-0x5A5A5A5B)
HIDDEN, LAYERS, ACTS = (20, 36, 64, 68, 72, 96, 128), (0, 1, 3), ('tanh', 'elu', 'relu')
LANES, EPISODES = (64, 32, 16, 4, 1), (1, 5, 64, 65)
QUEUE_WAVES = 1      # SERL_LANEQ_WAVES of the engine the `laneq` cases fly on: one wavefront, so that every episode beyond its lanes waits in the queue


def _case(section, kernel, s=S72, E=5, lanes=64, sensor=None, action=None, t_max=0.5, crash=None, tag=''):
    """sensor / action: None (no such noise) or the mask over the episodes, 0 = noisy, -1 = none (sensor_row / noise_row); crash: 'first' / 'last' =
    the flight of _crashing_and_benign's members with a crashing one at that episode"""
    assert kernel in KERNELS and (kernel != 'lanern' or sensor is not None or action is not None)
    bits = lambda m: ''.join('x' if v else 'n' for v in m[:5]) + ('+' if len(m) > 5 else '')      # n = noisy, x = masked out, + = MASK tiled on
    parts = [section, kernel, X.shape_id(s)[len('att_S7A3_'):], 'E%d' % E, 'l%d' % lanes]
    parts += ['s' + bits(sensor)] if sensor is not None else []
    parts += ['a' + bits(action)] if action is not None else []
    parts += [tag] if tag else []
    return dict(id='-'.join(parts), section=section, kernel=kernel, s=s, E=E, lanes=lanes, sensor=None if sensor is None else tuple(sensor),
                action=None if action is None else tuple(action), t_max=t_max, crash=crash)


def _tile(mask, E):
    return tuple((mask * (E // len(mask) + 1))[:E])


def _pairwise_shapes():
    """hidden x layers x activation thinned to pairwise coverage: every (hidden, layers), (hidden, activation) and (layers, activation) pair occurs
    -- a 7 x 3 Latin arrangement -- and every hidden width flies at 3 layers"""
    out = []
    for i, H in enumerate(HIDDEN):
        for j, L in enumerate(LAYERS):
            out.append(X._shape(H, L, ACTS[(i + j) % 3]))
    return out


def _cases():
    out = []
    patterns = list(itertools.product((0, -1), repeat=5))
    # 1. masks: hidden 72 x 3 tanh, 5 episodes, 64 lanes per wavefront
    for m in patterns:
        out.append(_case('mask', 'lanern', sensor=m))
    for m in patterns:
        out.append(_case('mask', 'lanern', action=m))
    for sm, am in ((MASK, MASK), (MASK, ON), (MASK, OFF), (MASK, COMPLEMENT), (ON, MASK), (OFF, MASK), (COMPLEMENT, MASK), (COMPLEMENT, COMPLEMENT)):
        out.append(_case('mask', 'lanern', sensor=sm, action=am))
    for kernel in ('lane', 'laneq'):      # no generator: the same masks select rows of pre-drawn tables
        for m in patterns:
            out.append(_case('mask', kernel, sensor=m))
        for m in patterns:
            out.append(_case('mask', kernel, action=m))
        for sm, am in ((MASK, MASK), (MASK, COMPLEMENT), (ON, MASK), (COMPLEMENT, OFF)):
            out.append(_case('mask', kernel, sensor=sm, action=am))
    # 2. occupancy: lanes per wavefront x episodes (65 at 64 lanes: a second wavefront with one live lane; on the queue's single wavefront: one refill)
    for kernel in KERNELS:
        for lanes in LANES:
            for E in EPISODES:
                out.append(_case('occ', kernel, E=E, lanes=lanes, sensor=_tile(MASK, E)))
    for kernel in KERNELS:      # lane 0 ends first while higher lanes fly on; the crashing member again at the last episode
        for crash in ('first', 'last'):
            out.append(_case('ends', kernel, E=6, lanes=64, sensor=_tile(MASK, 6), t_max=2.0, crash=crash, tag=crash))
    # 3. shapes: every hidden width at 3 layers under the generator and MASK at 64 lanes; the pairwise set on the plain kernel and the queue
    for H in HIDDEN:
        if H != 72:
            out.append(_case('shape', 'lanern', s=X._shape(H, 3), sensor=MASK))
    for i, s in enumerate(_pairwise_shapes()):
        out.append(_case('shape', ('lane', 'laneq', 'lanern')[i % 3], s=s, sensor=MASK, action=COMPLEMENT if i % 2 else None))
    return out


CASES = _cases()
BY_ID = {c['id']: c for c in CASES}


def select(section=None, kernel=None, hidden=None):
    return [c for c in CASES if (section is None or c['section'] == section) and (kernel is None or c['kernel'] == kernel)
            and (hidden is None or c['s']['hidden'] == hidden)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(sid, members, seed):
    s = [c['s'] for c in CASES if X.shape_id(c['s']) == sid][0]
    w = np.ascontiguousarray(X.make_weights(s, members, seed))
    w.setflags(write=False)
    return w


def crashing_and_benign():
    """tests/test_gpu_rollout_laneg.py _crashing_and_benign: members 0 and 2 saturate the command and end on the env's bounds, 1 and 3 fly the table out"""
    w = np.array(_weights(X.shape_id(S72), 4, 7))
    P = param_count(S72)
    w[0, P - 3:P] = 6.0
    w[2, P - 3:P] = [6.0, -6.0, 6.0]
    return w


def param_count(s):
    S, A, H, L = s['state_dim'], s['action_dim'], s['hidden'], s['num_layers']
    return H * S + H + L * (H * H + 3 * H) + A * H + A


def references(E, t_max, seed):
    from serl_amd import refsignals as rs
    r = np.ascontiguousarray(rs.synthetic_reference_tables(E, 2, 20, seed=seed)[:, :rs.n_steps_for(t_max)])
    assert np.isfinite(r).all()
    return r


def inputs(case):
    """everything a flight of `case` reads, as numpy arrays: w [M, P4], moe, refs [E, T, 3], err0 [E, 3], env / episode (the generator's counter
    words), and for the table kernels the pre-drawn tables sn [E, T + 1, 7] / an [E, T, 3] with sensor_row / noise_row = the row the mask selects
    (the rows in reverse order of the episodes: a row is not its episode's index) or -1.  For `lanern` sn / an are absent until noise_rows() or
    stand_in_rows() puts them there."""
    s, E = case['s'], case['E']
    if case['crash']:
        w = crashing_and_benign()
        moe = np.array({'first': [0, 1, 3, 1, 3, 1], 'last': [1, 3, 1, 3, 1, 2]}[case['crash']], np.int32)
        assert E == len(moe)
        refs = references(E, case['t_max'], 3)
    else:
        M = min(E, 5)
        w = np.array(_weights(X.shape_id(s), M, 400 + s['hidden'] + s['num_layers']))
        moe = (np.arange(E, dtype=np.int32)[::-1] % M).astype(np.int32)
        refs = references(E, case['t_max'], 41 + E)
    T = refs.shape[1]
    inp = dict(w=w, moe=moe, refs=refs, T=T, err0=(np.arange(E * 3).reshape(E, 3) % 7 - 3) * 2.0e-3,
               env=(7 + 3 * np.arange(E)).astype(np.int32), episode=(np.arange(E) % 3).astype(np.int32))
    for key, mask in (('sr', case['sensor']), ('nr', case['action'])):
        if mask is not None:
            m = np.asarray(mask, np.int32)
            inp[key] = np.where(m == 0, (E - 1 - np.arange(E)) if case['kernel'] != 'lanern' else np.arange(E), -1).astype(np.int32)
    if case['kernel'] != 'lanern':
        stand_in_rows(case, inp)
    return inp


def stand_in_rows(case, inp):
    """pre-drawn tables: the sensor model's addends (builds.sensor_noise_table) and clipped normal exploration noise"""
    from serl_amd import builds
    E, T = case['E'], inp['T']
    if case['sensor'] is not None:
        inp['sn'] = np.stack([builds.sensor_noise_table(T, np.random.RandomState(40 + e)) for e in range(E)])
        assert inp['sn'].shape == (E, T + 1, 7)
    if case['action'] is not None:
        inp['an'] = np.clip(SD * np.random.RandomState(90 + E).standard_normal((E, T, 3)), -CLIP, CLIP)
    return inp


def noise_rows(engine, case, inp):
    """`lanern`: what the generator draws for the case's episodes, written out by the kernels' own device functions (serl_amd.venv_noise) -- the
    rows the oracle replays"""
    import serl_amd
    T = inp['T']
    if case['sensor'] is not None:
        inp['sn'] = serl_amd.venv_noise(SEED, inp['env'], inp['episode'], T + 1, 'sensor', engine=engine).cpu().numpy()
    if case['action'] is not None:
        inp['an'] = serl_amd.venv_noise(SEED, inp['env'], inp['episode'], T, 'action', noise_sd=SD, noise_clip=CLIP, engine=engine).cpu().numpy()
        assert (np.abs(inp['an']) == CLIP).any() and (np.abs(inp['an']) < CLIP).any()
    return inp


def oracle(case, inp, threads=8):
    """the CPU oracle's same-libm flavour (tests/test_gpu_rollout.py _oracle) on the case's inputs"""
    from oracle import rollout as R
    kw = {}
    if case['sensor'] is not None:
        kw.update(sensor_noise=inp['sn'], sensor_row=inp['sr'])
    if case['action'] is not None:
        kw.update(action_noise=inp['an'], noise_row=inp['nr'])
    return R.rollout(inp['w'], X.net_of(case['s']), inp['moe'], inp['refs'], t_max=case['t_max'], err0=inp['err0'], traces=True, transitions=True,
                     threads=min(threads, case['E']), short_libm=True, **kw)


def same_as_oracle(g, o, what):
    """bit for bit: the results of every episode, and the traces and transitions over the steps an episode flew (tests/test_gpu_rollout_laneg.py
    _same_as_oracle)"""
    for k in ('fitness', 'length_steps', 'length_t', 'cost_steps'):
        np.testing.assert_array_equal(g[k], o[k], err_msg='%s: oracle %s' % (what, k))
    for e, n in enumerate(np.abs(g['length_steps'])):
        for k in ('actions', 'states', 'rewards', 'transitions'):
            np.testing.assert_array_equal(g[k][e, :n], o[k][e, :n], err_msg='%s: oracle %s of episode %d' % (what, k, e))


# ---- the guarded launch ----------------------------------------------------------------------------------------------------------------------------
def _guarded(rows, fill, dtype, device, gap=0):
    """rows [n, ...] between one row of `fill` in front and one behind, each row followed by `gap` more leading-axis entries of `fill` -> (the whole
    tensor, the view of the rows)"""
    import torch
    rows = np.asarray(rows, dtype)
    shape = (rows.shape[0] + 2,) + ((rows.shape[1] + gap,) + rows.shape[2:] if rows.ndim > 1 else ())
    big = np.full(shape, fill, dtype)
    if rows.ndim > 1:
        big[1:-1, :rows.shape[1]] = rows
    else:
        big[1:-1] = rows
    t = torch.from_numpy(big).to(device)
    return t, t[1:-1]


def _flip(mask_value):
    return np.int32(-1 if mask_value >= 0 else 0)


def fly(engine, case, inp):
    """ONE guarded launch of the case through the C ABI -> numpy outputs of its E episodes.  Asserts that the lane family flew the wave-cooperative
    branch (family 'lane', lanes per wavefront and queue as the case says, no regrouped copy: the per-lane actor exists at hidden 32 alone), that
    every episode was written, and that no entry outside the episodes' own lost its sentinel."""
    import torch
    from serl_amd import _capi, builds
    s, E, T, lanes, kernel = case['s'], case['E'], inp['T'], case['lanes'], case['kernel']
    assert s['hidden'] != 32
    dev = engine.device
    spec = X.spec_of(s)
    P, M = spec.param_count, inp['w'].shape[0]
    assert P == param_count(s)
    nan = float('nan')
    keep = []

    def g(rows, fill, dtype, gap=0):
        big, view = _guarded(rows, fill, dtype, dev, gap)
        keep.append(big)
        return big, view

    stride = (P + 3) // 4 * 4 + 8
    wbig = np.full((M + 2, stride), nan, np.float32)
    wbig[1:-1, :P] = inp['w'][:, :P]
    wbig = torch.from_numpy(wbig).to(dev); keep.append(wbig)
    # a member index read beside its row addresses the NaN row behind the members
    _, moe = g(inp['moe'], M, np.int32)
    _, ref = g(inp['refs'], nan, np.float64, gap=1)      # a NaN entry behind every episode's table (ref_stride = (T + 1) x 3)
    _, err0 = g(inp['err0'], nan, np.float64)
    out = {}
    for k, shape, dtype, fill in (('fitness', (), np.float64, SENT_F64), ('length_steps', (), np.int32, SENT_I32), ('length_t', (), np.float64, SENT_F64),
                                  ('cost_steps', (), np.int32, SENT_I32), ('actions', (T, 3), np.float64, SENT_F64), ('states', (T, 12), np.float64, SENT_F64),
                                  ('rewards', (T,), np.float64, SENT_F64), ('transitions', (T, 20), np.float32, SENT_F32)):
        out[k] = g(np.full((E,) + shape, fill, dtype), fill, dtype)
    d = _capi.RolloutDesc(state_dim=7, action_dim=3, hidden=s['hidden'], num_layers=s['num_layers'], activation=spec.activation_id, n_members=M,
                          weights=wbig[1].data_ptr(), weight_stride=stride, n_episodes=E, build_slot=engine.slot_of('h2000_v90'),
                          member_of_episode=moe.data_ptr(), ref=ref.data_ptr(), ref_stride=(T + 1) * 3, err0=err0.data_ptr(), t_max=float(case['t_max']),
                          max_steps=T, lanes_per_wave=lanes, kernel_hint=_capi.KERNEL_HINTS['laneq' if kernel == 'laneq' else None],
                          **{k: v[1].data_ptr() for k, v in out.items()})
    nz = None
    if kernel == 'lanern':
        # the masks alone: an entry read beside its own is the opposite of its neighbour's, and the keys beside the episodes' draw other noise
        if case['sensor'] is not None:
            sr = np.concatenate([[_flip(inp['sr'][0])], inp['sr'], [_flip(inp['sr'][-1])]]).astype(np.int32)
            t = torch.from_numpy(sr).to(dev); keep.append(t); d.sensor_row = t[1:].data_ptr()
        if case['action'] is not None:
            nr = np.concatenate([[_flip(inp['nr'][0])], inp['nr'], [_flip(inp['nr'][-1])]]).astype(np.int32)
            t = torch.from_numpy(nr).to(dev); keep.append(t); d.noise_row = t[1:].data_ptr()
        bias, scale = builds.sensor_bias_scale()
        nz = _capi.RolloutNoiseDesc(seed=SEED, sensor=int(case['sensor'] is not None), sensor_bias=(ctypes.c_double * 7)(*bias),
                                    sensor_scale=(ctypes.c_double * 7)(*scale), action=int(case['action'] is not None),
                                    action_sd=SD if case['action'] is not None else 0.0, action_clip=CLIP if case['action'] is not None else 0.0)
        _, env = g(inp['env'], 0x7FFFFFF0, np.int32)
        _, epi = g(inp['episode'], 0x7FFFFFF1, np.int32)
        nz.env, nz.episode = env.data_ptr(), epi.data_ptr()
    else:
        # tables between NaN rows; a row index read beside its own addresses the NaN row behind the table
        if case['sensor'] is not None:
            _, sn = g(inp['sn'], nan, np.float64)
            _, sr = g(inp['sr'], inp['sn'].shape[0], np.int32)
            d.sensor_noise, d.sensor_row = sn.data_ptr(), sr.data_ptr()
        if case['action'] is not None:
            _, an = g(inp['an'], nan, np.float64)
            _, nr = g(inp['nr'], inp['an'].shape[0], np.int32)
            d.action_noise, d.noise_row = an.data_ptr(), nr.data_ptr()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if nz is not None:
        _capi.check(engine.lib.serl_rollout_noise(engine.ctx, ctypes.byref(d), ctypes.byref(nz), stream), 'serl_rollout_noise')
    else:
        _capi.check(engine.lib.serl_rollout(engine.ctx, ctypes.byref(d), stream), 'serl_rollout')
    info = engine.last_rollout_info()
    assert info['family'] == 'lane' and info['episodes_per_team'] == lanes and info['launches'] == 1 and info['actor_streamed'], info
    if kernel == 'laneq':      # (the queue's engine has ONE wavefront: QUEUE_WAVES)
        assert info['workgroups'] == 1 and info['work_queue'] == (E > lanes), info
    else:
        assert not info['work_queue'] and info['workgroups'] * 4 >= -(-E // lanes), info
    assert engine.last_rollout_weights()['regrouped'] == 0
    torch.cuda.synchronize()
    res = {k: v[1].cpu().numpy() for k, v in out.items()}
    whole = {k: v[0].cpu().numpy() for k, v in out.items()}
    del keep
    assert (res['length_steps'] != SENT_I32).all() and (res['length_steps'] != 0).all(), '%s: an episode was not written: %s' % (case['id'], res['length_steps'])
    fills = dict(fitness=SENT_F64, length_steps=SENT_I32, length_t=SENT_F64, cost_steps=SENT_I32, actions=SENT_F64, states=SENT_F64, rewards=SENT_F64,
                 transitions=SENT_F32)
    for k, a in whole.items():      # the rows in front of episode 0 and behind episode E - 1
        assert (a[0] == fills[k]).all() and (a[-1] == fills[k]).all(), '%s: %s was written outside the episodes' % (case['id'], k)
    for e, n in enumerate(np.abs(res['length_steps'])):      # the steps behind an episode's end
        for k in ('actions', 'states', 'rewards', 'transitions'):
            assert (res[k][e, n:] == fills[k]).all(), '%s: %s of episode %d was written behind its end (step %d)' % (case['id'], k, e, n)
    return res


def run_case(engine, case, queue_engine=None):
    """the case's inputs, its guarded flight and the oracle's; raises AssertionError where they differ -> (outputs, oracle's)"""
    eng = queue_engine if case['kernel'] == 'laneq' else engine
    inp = inputs(case)
    if case['kernel'] == 'lanern':
        noise_rows(eng, case, inp)
    got = fly(eng, case, inp)
    want = oracle(case, inp)
    same_as_oracle(got, want, case['id'])
    return got, want

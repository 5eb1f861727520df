"""The lane-per-episode population kernel for every actor shape (kernel_hint SERL_KERNEL_LANEG, family SERL_FAMILY_LANEG; csrc/family_laneg.hip,
family_lanegn.hip) as far as no GPU is needed: the numbers of the hint and the family in the header and in the ctypes mirror, the plans the library
makes for the hint at 256 CUs (serl_host_plan_rollout), every refusal with the limit it names, the `kernel` keyword through the package, the build's
units and the ABI it did not move."""
import ctypes, os, re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -3
LANEG, FAMILY_LANEG, FAMILY_LANE = 7, 14, 12
AUTO, WAVE, LANEQ = 0, 2, 6


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()


def _header():
    with open(os.path.join(ROOT, 'include', 'serl_amd.h')) as f:
        return f.read()


def _enum(name):
    """the enumerators of `enum name { ... };` in the header with their values, as a C compiler counts them"""
    body = re.search(r'enum\s+%s\s*\{(.*?)\};' % name, _header(), re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    vals, nxt = {}, 0
    for item in body.split(','):
        if not item.strip():
            continue
        k, _, expr = item.partition('=')
        assert re.fullmatch(r'[\w\s+]*', expr), expr
        v = eval(expr, {'__builtins__': {}}, dict(vals)) if expr.strip() else nxt
        vals[k.strip()] = v
        nxt = v + 1
    return vals


def _caps(num_cus=256, kernel=0, wpb=-1, laneq_waves=-1, split=0, remote=1, regroup=1):
    return (ctypes.c_int32 * 7)(num_cus, kernel, wpb, laneq_waves, split, remote, regroup)


def _param_count(S, A, H, L):
    return H * S + H + L * (H * H + 3 * H) + A * H + A


def _desc(n, S=7, A=3, H=72, L=3, hint=LANEG, lanes=0, conc=0, env=0, incremental=0, members=1):
    from serl_amd import _capi
    return _capi.RolloutDesc(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=0, n_members=members, weight_stride=(_param_count(S, A, H, L) + 3) // 4 * 4,
                             n_episodes=n, max_steps=1, lanes_per_wave=lanes, kernel_hint=hint, concurrent_episodes=conc, env_config=env, incremental=incremental)


def _plan(L, d, noise=0, caps=None):
    """(status, dict of the 16 words by name, the library's message)"""
    out = (ctypes.c_int32 * 16)()
    st = L.serl_host_plan_rollout(caps if caps is not None else _caps(), ctypes.byref(d), noise, out)
    names = ('family', 'grid', 'per_team', 'queue', 'actor_waves', 'streamed', 'launches', 'code', 'block', 'lanes', 'q0', 'regroup', 'mail_bytes', 'timed', 'chunk')
    return st, dict(zip(names, list(out))), L.serl_last_error().decode()


def test_header_and_mirror_name_the_hint_and_the_family():
    from serl_amd import _capi
    hints, fams = _enum('serl_kernel_hint'), _enum('serl_kernel_family')
    assert hints['SERL_KERNEL_LANEG'] == LANEG == _capi.KERNEL_HINTS['laneg'] == _capi.KERNEL_LANEG
    assert fams['SERL_FAMILY_LANEG'] == FAMILY_LANEG == _capi.FAMILY_LANEG and _capi.FAMILIES[FAMILY_LANEG] == 'laneg'
    # the earlier numbers stay
    assert {k: v for k, v in hints.items() if k != 'SERL_KERNEL_LANEG'} == {'SERL_KERNEL_AUTO': 0, 'SERL_KERNEL_TEAM': 1, 'SERL_KERNEL_WAVE': 2, 'SERL_KERNEL_HALF': 3,
                                                                           'SERL_KERNEL_TEAM2': 4, 'SERL_KERNEL_TEAM4': 5, 'SERL_KERNEL_LANEQ': 6}
    assert sorted(v for k, v in fams.items() if k != 'SERL_FAMILY_LANEG') == list(range(14)) and fams['SERL_FAMILY_LANE'] == FAMILY_LANE
    assert 'laneg' in _capi.KERNEL_HINTS and _capi.KERNEL_HINTS.get('laneg') == LANEG and _capi.KERNEL_HINTS.get('no such', 0) == 0
    h = _header()
    assert re.search(r'SERL_KERNEL=[\w|]*\blaneg\b', h), 'SERL_KERNEL=laneg is not listed with the other development overrides'
    assert re.search(r'#define\s+SERL_ABI_VERSION\s+9\b', h)


def test_abi_version_and_layout_are_unchanged():
    from serl_amd import _capi
    L = _lib()
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()


def test_the_build_has_units_of_their_own_per_code_variant():
    from serl_amd import build
    for fam in ('laneg', 'lanegn'):
        assert fam in build.FAMILIES
        for code, v in enumerate(build.VARIANTS):
            assert build.UNITS['rollout_%s_%s' % (fam, v)] == ('family_%s.hip' % fam, ['-DSERL_DYN=%d' % code])
        assert os.path.exists(os.path.join(build.CSRC, 'family_%s.hip' % fam))
    for v in build.VARIANTS:      # the existing units are what they were
        assert build.UNITS['rollout_' + v] == ('family_lane.hip', ['-DSERL_DYN=%d' % build.VARIANTS.index(v)])
        assert build.UNITS['rollout_lanern_' + v][0] == 'family_lanern.hip'
    assert not any(u.startswith('rollout_laneg') for u in build.TEAM_UNITS)      # (the jitter library recompiles the team units only)


def test_plan_at_256_cus():
    L = _lib()
    # hidden 72 x 3, 65 536 episodes: 64 lanes, ceil(65 536 / 64) = 1 024 wavefronts, four per workgroup (serl_plan_lanes: more wavefronts than CUs)
    st, p, msg = _plan(L, _desc(65536, members=50))
    assert st == OK, msg
    assert (p['family'], p['lanes'], p['per_team'], p['block'], p['grid']) == (FAMILY_LANEG, 64, 64, 256, 256)
    assert p['grid'] * (p['block'] // 64) == (65536 + 63) // 64
    assert (p['queue'], p['q0'], p['regroup'], p['streamed'], p['actor_waves'], p['launches'], p['chunk'], p['mail_bytes'], p['timed']) == (0, 0, 0, 1, 0, 1, 65536, 0, 1)
    # the workgroup shape is serl_plan_lanes': what lanes_per_wave = 64 without the hint launches
    st2, q, _ = _plan(L, _desc(65536, hint=AUTO, lanes=64, members=50))
    assert st2 == OK and q['family'] == FAMILY_LANE and (q['grid'], q['block'], q['lanes']) == (p['grid'], p['block'], p['lanes'])
    # lanes_per_wave = 64 with the hint is the same plan as 0 with it, and 65 clamps to 64
    for lanes in (64, 65):
        assert _plan(L, _desc(65536, lanes=lanes, members=50))[1] == p
    # no more wavefronts than CUs: one per workgroup
    st, p, _ = _plan(L, _desc(70))
    assert st == OK and (p['family'], p['lanes'], p['grid'], p['block']) == (FAMILY_LANEG, 64, 2, 64)
    # lanes_per_wave = 3 with 5 episodes: 2 wavefronts
    st, p, _ = _plan(L, _desc(5, lanes=3))
    assert st == OK and (p['family'], p['lanes'], p['grid'] * (p['block'] // 64), p['queue'], p['regroup']) == (FAMILY_LANEG, 3, 2, 0, 0)
    # hidden 32 x 3 under the hint: still the rows as they lie, no regrouped copy
    st, p, _ = _plan(L, _desc(4096, H=32, members=64))
    assert st == OK and (p['family'], p['regroup']) == (FAMILY_LANEG, 0)
    # beside other launches: planned the same way, not timed (as every launch that shares the GPU)
    st, p, _ = _plan(L, _desc(4096, conc=4096))
    assert st == OK and (p['family'], p['grid'], p['block'], p['timed']) == (FAMILY_LANEG, 64, 64, 0)


def test_noise_is_accepted_with_the_same_shape():
    L = _lib()
    for n, lanes in ((65536, 0), (5, 3), (70, 64), (1, 1)):
        plain, noisy = _plan(L, _desc(n, lanes=lanes)), _plan(L, _desc(n, lanes=lanes), noise=1)
        assert plain[0] == OK == noisy[0] and plain[1] == noisy[1] and plain[1]['family'] == FAMILY_LANEG, (n, lanes)
    st, _, msg = _plan(L, _desc(64, hint=LANEQ), noise=1)      # the work queue still has no noise instantiation
    assert st == UNSUPPORTED and 'no noise instantiation' in msg


REFUSALS = [
    (dict(env=1, S=2, A=1), 'env_config'), (dict(env=2, S=13, A=3), 'env_config'), (dict(incremental=1, S=10), 'incremental'),
    (dict(H=132), 'hidden'), (dict(H=30), 'hidden'), (dict(H=0), 'hidden'), (dict(L=17), 'num_layers'), (dict(L=-1), 'num_layers'),
    (dict(S=13), 'state_dim'), (dict(A=1), 'action_dim'),
]


@pytest.mark.parametrize('kw,limit', REFUSALS, ids=['-'.join('%s%s' % kv for kv in kw.items()) for kw, _ in REFUSALS])
def test_refusals_name_the_limit(kw, limit):
    L = _lib()
    for noise in (0, 1):
        for lanes in (0, 64):
            st, p, msg = _plan(L, _desc(4096, lanes=lanes, **kw), noise=noise)
            assert st == UNSUPPORTED and 'LANEG' in msg and limit in msg, (st, msg)
            assert not any(p.values())      # nothing was planned


def test_the_environment_override_resolves_to_the_hint():
    from serl_amd import evaluator
    L = _lib()
    caps = evaluator.planner_caps(256, {'SERL_KERNEL': 'laneg'})
    assert caps[1] == LANEG
    st, p, _ = _plan(L, _desc(4096, hint=AUTO), caps=(ctypes.c_int32 * 7)(*caps))
    assert st == OK and p['family'] == FAMILY_LANEG
    st, p, _ = _plan(L, _desc(4096, hint=WAVE), caps=(ctypes.c_int32 * 7)(*caps))      # a descriptor's own hint comes first
    assert st == OK and p['family'] == 10
    st, _, msg = _plan(L, _desc(8, hint=AUTO, env=1, S=2, A=1), caps=(ctypes.c_int32 * 7)(*caps))
    assert st == UNSUPPORTED and 'env_config' in msg


def test_every_other_hint_plans_as_before():
    """hint 8 is out of range, and the plans of AUTO with 72 x 3 are untouched by the new block (spot checks of the table in serl_plan.h)"""
    L = _lib()
    st, _, msg = _plan(L, _desc(8, hint=8))
    assert st == INVALID and 'kernel_hint' in msg
    st, p, _ = _plan(L, _desc(65536, hint=AUTO))
    assert st == OK and p['family'] == 10      # one wavefront per episode: what runs today
    st, p, _ = _plan(L, _desc(65537, hint=LANEQ))      # one episode beyond the lane slots of 4 x 256 wavefronts
    assert st == OK and p['family'] == FAMILY_LANE and (p['queue'], p['q0']) == (1, 65536)


def test_through_the_package():
    import inspect
    import serl_amd
    from serl_amd import evaluator
    _lib()
    spec = serl_amd.NetSpec(7, 3, 72, 3, 'tanh')
    p = evaluator.plan_rollout(spec, 65536, num_cus=256, kernel='laneg', n_members=50)
    assert (p['family'], p['workgroups'], p['episodes_per_team'], p['work_queue'], p['lanes'], p['block'], p['regroup'], p['actor_streamed']) == \
        ('laneg', 256, 64, False, 64, 256, False, True)
    p = evaluator.plan_rollout(spec, 5, num_cus=256, kernel='laneg', lanes_per_wave=3, noise=True)
    assert (p['family'], p['workgroups'], p['lanes']) == ('laneg', 2, 3)
    with pytest.raises(RuntimeError, match=r'\(-3\).*LANEG.*hidden'):
        evaluator.plan_rollout(serl_amd.NetSpec(7, 3, 132, 1, 'tanh'), 8, num_cus=256, kernel='laneg')
    with pytest.raises(RuntimeError, match=r'\(-3\).*LANEG.*env_config'):
        evaluator.plan_rollout(serl_amd.NetSpec(2, 1, 32, 1, 'tanh'), 8, num_cus=256, kernel='laneg', env_config=1)
    with pytest.raises(RuntimeError, match=r'kernel_hint must be AUTO, TEAM or WAVE'):      # the dynamics alone have no actor: the hint means nothing there
        evaluator.plan_rollout(None, 8, num_cus=256, kernel='laneg', open_loop=True)
    assert 'laneg' in evaluator.evaluate_pop.__doc__ and 'laneg' in evaluator.RolloutEngine.rollout.__doc__
    # device noise takes the hint: the argument check that lists the kernels without a noise instantiation lets it through
    assert evaluator.RolloutEngine._check_device_noise(4, 'device', None, None, None, 1, None, None, None, None, 'laneg', True) == (True, False)
    with pytest.raises(ValueError, match='laneg'):
        evaluator.RolloutEngine._check_device_noise(4, 'device', None, None, None, 1, None, None, None, None, 'laneq', True)
    assert inspect.signature(evaluator.evaluate_pop).parameters['kernel'].default is None

"""kernel='laneg' over a REGROUPED copy of the weights (C ABI serl_rollout_regrouped / serl_host_plan_rollout_regrouped / serl_last_rollout_weights;
csrc/family_lanegt.hip, family_lanegtn.hip around lane_actor.h serl_actor_forward_lane_general_t) as far as no GPU is needed: the three symbols in the
header, the binding and the library; the ABI and the two enums it did not move; the build's ten new units; the property of the packed layout the forward
rests on, for every shape it takes; the plans at 256 CUs word for word against the LANEG plans of serl_host_plan_rollout; every refusal with the limit it
names; the `lane_weights` keyword through the package."""
import ctypes, inspect, os, re
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -3
AUTO, WAVE, LANEQ, LANEG = 0, 2, 6, 7
FAMILY_LANEG = 14
SYMBOLS = ('serl_rollout_regrouped', 'serl_host_plan_rollout_regrouped', 'serl_last_rollout_weights')
NAMES = ('family', 'grid', 'per_team', 'queue', 'actor_waves', 'streamed', 'launches', 'code', 'block', 'lanes', 'q0', 'regroup', 'mail_bytes', 'timed', 'chunk', 'zero')
# the two enums as they stand (tests/test_rollout_laneg_host.py pins the literals of the first, tests/test_host_api.py the set of the second)
HINTS = {'SERL_KERNEL_AUTO': 0, 'SERL_KERNEL_TEAM': 1, 'SERL_KERNEL_WAVE': 2, 'SERL_KERNEL_HALF': 3, 'SERL_KERNEL_TEAM2': 4, 'SERL_KERNEL_TEAM4': 5,
         'SERL_KERNEL_LANEQ': 6, 'SERL_KERNEL_LANEG': 7}
FAMILIES = {'SERL_FAMILY_NONE': 0, 'SERL_FAMILY_TEAM': 1, 'SERL_FAMILY_TEAMS': 2, 'SERL_FAMILY_TEAMS2': 3, 'SERL_FAMILY_TEAMX': 4, 'SERL_FAMILY_TEAM2': 5,
            'SERL_FAMILY_TEAM2S': 6, 'SERL_FAMILY_TEAM4': 7, 'SERL_FAMILY_TEAM4_MIXED': 8, 'SERL_FAMILY_HALF': 9, 'SERL_FAMILY_WAVE': 10, 'SERL_FAMILY_WAVEX': 11,
            'SERL_FAMILY_LANE': 12, 'SERL_FAMILY_TEAMR': 13, 'SERL_FAMILY_LANEG': 14}


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


def _plan(L, d, noise=0, caps=None, regrouped=True):
    """(status, dict of the 16 words by name, the library's message) of serl_host_plan_rollout_regrouped (regrouped=False: of serl_host_plan_rollout)"""
    out = (ctypes.c_int32 * 16)()
    fn = L.serl_host_plan_rollout_regrouped if regrouped else L.serl_host_plan_rollout
    st = fn(caps if caps is not None else _caps(), ctypes.byref(d), noise, out)
    return st, dict(zip(NAMES, list(out))), L.serl_last_error().decode()


# ---- 1. header, binding, build ---------------------------------------------------------------------------------------------------------------------------

def test_header_binding_and_library_have_the_three_symbols():
    from serl_amd import _capi
    L = _lib()
    hdr = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    for f in SYMBOLS:
        assert re.search(r'^int %s\(' % f, hdr, re.M), '%s is not declared in include/serl_amd.h' % f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    assert re.search(r'^int serl_rollout_regrouped\(serl_ctx \*\w+, const serl_rollout_desc \*\w+, const serl_rollout_noise_desc \*\w+\s*, void \*\w+\);', hdr, re.M)
    assert re.search(r'^int serl_host_plan_rollout_regrouped\(const int32_t caps\[7\], const serl_rollout_desc \*\w+, int32_t noise, int32_t out\[16\]\);', hdr, re.M)
    assert re.search(r'^int serl_last_rollout_weights\(serl_ctx \*\w+, int64_t out\[4\]\);', hdr, re.M)
    # the memory cost is stated where the entry point is declared
    doc = _header()
    doc = doc[:doc.index('int serl_rollout_regrouped(')]
    doc = doc[doc.rindex('/*'):]
    assert 'x 16 bytes' in doc and 'SERL_WT_SLOTS' in doc and '7.75 GB' in doc and '65 536 members' in doc
    assert (_param_count(7, 3, 96, 3) + 3) // 4 * 65536 * 16 == 7_752_122_368      # the 7.75 GB of the header


def test_abi_and_enums_are_unchanged():
    from serl_amd import _capi
    L = _lib()
    assert re.search(r'#define\s+SERL_ABI_VERSION\s+9\b', _header())
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    assert _enum('serl_kernel_hint') == HINTS
    assert _enum('serl_kernel_family') == FAMILIES
    assert len(_capi.KERNEL_HINTS) == 8 and len(_capi.FAMILIES) == 14      # (the pinned lengths of the mirror's tables: no new hint, no new family)


def test_the_build_has_ten_units_on_files_of_their_own():
    from serl_amd import build
    new = {}
    for fam in ('lanegt', 'lanegtn'):
        assert fam in build.FAMILIES
        src = os.path.join(build.CSRC, 'family_%s.hip' % fam)
        assert os.path.exists(src)
        text = open(src).read()
        assert '#define SERL_LANE_GENERAL_ACTOR 1' in text and '#define SERL_LANE_REGROUPED_WEIGHTS 1' in text
        assert ('#define SERL_ROLLOUT_NOISE 1' in text) == (fam == 'lanegtn')
        for code, v in enumerate(build.VARIANTS):
            new['rollout_%s_%s' % (fam, v)] = ('family_%s.hip' % fam, ['-DSERL_DYN=%d' % code])
    assert len(new) == 10 and all(build.UNITS[k] == v for k, v in new.items())
    assert not any(u in build.TEAM_UNITS for u in new)      # (the jitter library recompiles the team units only)
    # every existing unit is what it was
    old = {s: (s + '.hip', []) for s in ('serl_capi', 'serl_ga', 'serl_metrics', 'serl_distill', 'serl_td3', 'serl_noise')}
    for f in ('lane', 'lanenz', 'lanern', 'laneg', 'lanegn', 'venvw', 'venvwr', 'wave', 'wavern', 'half', 'team', 'teamr', 'teams2', 'team2', 'team2s', 'team4'):
        for code, v in enumerate(build.VARIANTS):
            old[('rollout_' if f == 'lane' else 'rollout_%s_' % f) + v] = ('family_%s.hip' % f, ['-DSERL_DYN=%d' % code])
    old['rollout_team4_mixed'] = ('rollout_team4_mixed.hip', [])
    assert {k: v for k, v in build.UNITS.items() if k not in new} == old
    for fam in ('laneg', 'lanegn'):      # the row kernels' units select no regrouped forward
        assert 'SERL_LANE_REGROUPED_WEIGHTS' not in open(os.path.join(build.CSRC, 'family_%s.hip' % fam)).read()


# ---- 2. the layout property ------------------------------------------------------------------------------------------------------------------------------

def test_every_tensor_and_row_of_the_packed_layout_starts_at_a_multiple_of_four():
    """state_dim 7, action_dim 3, hidden % 4 == 0: the offsets of the packed layout (W0 [H][7], b0 [H], per hidden layer W [H][H], b, gamma, beta [H], then
    Wout [3][H], bout [3]) by plain arithmetic, their sum against serl_param_count"""
    L = _lib()
    L.serl_param_count.restype = ctypes.c_int
    for H in range(4, 129, 4):
        for layers in range(17):
            off, starts, rows = 0, [], []
            starts.append(off); off += 7 * H                      # W0: rows of 7 floats are NOT aligned, blocks of four rows are
            for i in range(0, H, 4):
                assert 7 * i == 28 * (i // 4) and (7 * i) % 4 == 0 and 7 * i // 4 == 7 * (i // 4)      # seven groups per block of four rows
            starts.append(off); off += H                          # b0
            assert off == 8 * H
            for _ in range(layers):
                starts.append(off); rows += [off + r * H for r in range(H)]; off += H * H
                for _ in range(3):                                # bias, gamma, beta
                    starts.append(off); off += H
            assert off == 8 * H + layers * (H * H + 3 * H)
            starts.append(off); rows += [off + r * H for r in range(3)]; off += 3 * H
            starts.append(off)                                    # the output bias: the first three elements of the last group
            P = off + 3
            assert P == L.serl_param_count(7, H, layers, 3) == _param_count(7, 3, H, layers)
            assert all(s % 4 == 0 for s in starts) and all(r % 4 == 0 for r in rows), (H, layers)
            groups = (P + 3) // 4
            assert starts[-1] // 4 == groups - 1 and P == 4 * (groups - 1) + 3      # ... whose fourth element is the zero padding
    assert _param_count(7, 3, 4, 0) == 47


# ---- 3. plans --------------------------------------------------------------------------------------------------------------------------------------------

PLAN_CASES = [dict(n=65536, members=50), dict(n=65536, members=65536), dict(n=70), dict(n=5, lanes=3), dict(n=70, lanes=64), dict(n=70, lanes=65),
              dict(n=4096, H=32, members=64), dict(n=4096, H=32, lanes=64, members=64), dict(n=4096, conc=4096), dict(n=1, lanes=3), dict(n=16384, H=96),
              dict(n=5, H=4, L=0, lanes=3), dict(n=5, H=128, L=1), dict(n=5, H=8, L=16), dict(n=4, members=1 << 22)]


@pytest.mark.parametrize('kw', PLAN_CASES, ids=['-'.join('%s%s' % kv for kv in kw.items()) for kw in PLAN_CASES])
def test_plan_is_the_laneg_plan_with_regroup(kw):
    L = _lib()
    for noise in (0, 1):
        for caps in (_caps(), _caps(regroup=0)):      # SERL_LANE_WEIGHTS=rows does not apply: the caller asked for the copy
            st, rows, msg = _plan(L, _desc(**kw), noise=noise, caps=caps, regrouped=False)
            assert st == OK and rows['family'] == FAMILY_LANEG and rows['regroup'] == 0, msg      # serl_host_plan_rollout still streams the rows
            st, p, msg = _plan(L, _desc(**kw), noise=noise, caps=caps)
            assert st == OK, msg
            assert p['regroup'] == 1 and p['family'] == FAMILY_LANEG
            assert dict(p, regroup=0) == rows, (p, rows)


def test_plan_shapes_at_256_cus():
    L = _lib()
    st, p, _ = _plan(L, _desc(65536, members=65536))
    assert st == OK and (p['family'], p['lanes'], p['per_team'], p['block'], p['grid'], p['regroup']) == (FAMILY_LANEG, 64, 64, 256, 256, 1)
    assert (p['queue'], p['q0'], p['streamed'], p['actor_waves'], p['launches'], p['chunk'], p['mail_bytes'], p['timed'], p['code']) == (0, 0, 1, 0, 1, 65536, 0, 1, -1)
    for lanes in (0, 64, 65):
        assert _plan(L, _desc(65536, lanes=lanes, members=65536))[1] == p
    st, p, _ = _plan(L, _desc(5, lanes=3))
    assert st == OK and (p['lanes'], p['grid'] * (p['block'] // 64), p['regroup']) == (3, 2, 1)
    # the environment override resolves to the hint here too
    st, p, _ = _plan(L, _desc(4096, hint=AUTO), caps=_caps(kernel=LANEG))
    assert st == OK and (p['family'], p['regroup']) == (FAMILY_LANEG, 1)


@pytest.mark.parametrize('hint,lanes', [(AUTO, 0), (AUTO, 64), (WAVE, 0), (WAVE, 64), (LANEQ, 0), (LANEQ, 64), (1, 0), (4, 0)])
def test_other_hints_are_refused(hint, lanes):
    L = _lib()
    for noise in (0, 1):
        for H in (72, 32):
            st, p, msg = _plan(L, _desc(4096, H=H, hint=hint, lanes=lanes, members=64), noise=noise)
            assert st == UNSUPPORTED and 'only the LANEG kernels read a regrouped copy through this entry' in msg and 'serl_rollout_regrouped' in msg, (st, msg)
            assert not any(p.values())


def test_member_limit():
    L = _lib()
    assert _plan(L, _desc(64, members=1 << 22))[0] == OK
    for noise in (0, 1):
        st, p, msg = _plan(L, _desc(64, members=(1 << 22) + 1), noise=noise)
        assert st == UNSUPPORTED and 'n_members' in msg and '1 << 22' in msg, (st, msg)
        assert not any(p.values())
    assert _plan(L, _desc(64, members=(1 << 22) + 1), regrouped=False)[0] == OK      # the rows have no such limit


REFUSALS = [
    (dict(env=1, S=2, A=1), 'env_config'), (dict(env=2, S=13, A=3), 'env_config'), (dict(incremental=1, S=10), 'incremental'),
    (dict(S=13), 'state_dim'), (dict(A=1), 'action_dim'), (dict(H=6), 'hidden'), (dict(H=132), 'hidden'), (dict(H=0), 'hidden'),
    (dict(L=17), 'num_layers'), (dict(L=-1), 'num_layers'),
]


@pytest.mark.parametrize('kw,limit', REFUSALS, ids=['-'.join('%s%s' % kv for kv in kw.items()) for kw, _ in REFUSALS])
def test_every_laneg_refusal_names_its_limit(kw, limit):
    L = _lib()
    for noise in (0, 1):
        for lanes in (0, 64):
            st, p, msg = _plan(L, _desc(4096, lanes=lanes, **kw), noise=noise)
            assert st == UNSUPPORTED and 'LANEG' in msg and limit in msg, (st, msg)
            assert not any(p.values())
            assert _plan(L, _desc(4096, lanes=lanes, **kw), noise=noise, regrouped=False)[2] == msg      # the same words as for the rows


def test_bad_arguments():
    L = _lib()
    out = (ctypes.c_int32 * 16)()
    d = _desc(8)
    assert L.serl_host_plan_rollout_regrouped(None, ctypes.byref(d), 0, out) == INVALID
    assert L.serl_host_plan_rollout_regrouped(_caps(), None, 0, out) == INVALID
    assert L.serl_host_plan_rollout_regrouped(_caps(), ctypes.byref(d), 0, None) == INVALID
    assert L.serl_host_plan_rollout_regrouped(_caps(num_cus=0), ctypes.byref(d), 0, out) == INVALID
    assert _plan(L, _desc(0))[0] == INVALID
    st, _, msg = _plan(L, _desc(8, hint=8))
    assert st == INVALID and 'kernel_hint' in msg
    # NULL contexts: refused, nothing dereferenced
    assert L.serl_last_rollout_weights(None, (ctypes.c_int64 * 4)()) == INVALID
    assert L.serl_rollout_regrouped(None, ctypes.byref(d), None, None) == INVALID


# ---- 4. Python -------------------------------------------------------------------------------------------------------------------------------------------

def test_through_the_package():
    import serl_amd
    from serl_amd import evaluator
    _lib()
    spec = serl_amd.NetSpec(7, 3, 72, 3, 'tanh')
    rows = evaluator.plan_rollout(spec, 65536, num_cus=256, kernel='laneg', n_members=65536)
    assert rows['family'] == 'laneg' and rows['regroup'] is False
    for lw in (None, 'rows'):
        assert evaluator.plan_rollout(spec, 65536, num_cus=256, kernel='laneg', n_members=65536, lane_weights=lw) == rows
    p = evaluator.plan_rollout(spec, 65536, num_cus=256, kernel='laneg', n_members=65536, lane_weights='regrouped')
    assert p['regroup'] is True and dict(p, regroup=False) == rows
    p = evaluator.plan_rollout(spec, 5, num_cus=256, kernel='laneg', lanes_per_wave=3, noise=True, lane_weights='regrouped')
    assert (p['family'], p['workgroups'], p['lanes'], p['regroup']) == ('laneg', 2, 3, True)
    # 'regrouped' needs the kernel: refused before the library is called
    for kernel in ('wave', None, 'laneq', 'team'):
        with pytest.raises(ValueError, match="lane_weights='regrouped' needs kernel='laneg'"):
            evaluator.plan_rollout(spec, 8, num_cus=256, kernel=kernel, lane_weights='regrouped')
    for bad in ('regroup', 'groups', '', 1, True):
        with pytest.raises(ValueError, match='lane_weights'):
            evaluator.plan_rollout(spec, 8, num_cus=256, kernel='laneg', lane_weights=bad)
    for lw in (None, 'rows'):      # ... and means nothing to the other kernels
        assert evaluator.plan_rollout(spec, 8, num_cus=256, kernel='wave', lane_weights=lw)['family'] == 'wave'
    # the library's refusals come through as RuntimeError with its text
    with pytest.raises(RuntimeError, match=r'\(-3\).*LANEG.*hidden'):
        evaluator.plan_rollout(serl_amd.NetSpec(7, 3, 132, 1, 'tanh'), 8, num_cus=256, kernel='laneg', lane_weights='regrouped')
    with pytest.raises(RuntimeError, match=r'\(-3\).*n_members.*1 << 22'):
        evaluator.plan_rollout(spec, 8, num_cus=256, kernel='laneg', lane_weights='regrouped', n_members=(1 << 22) + 1)
    # the keyword on every function of the issue, default None; the engine's method
    for fn in (evaluator.plan_rollout, evaluator.RolloutEngine.rollout, evaluator.evaluate_pop):
        assert inspect.signature(fn).parameters['lane_weights'].default is None
        assert 'regrouped' in fn.__doc__
    assert 'lane_weights' in inspect.getsource(evaluator.RolloutEngine.plan_rollout) or 'kw' in inspect.signature(evaluator.RolloutEngine.plan_rollout).parameters
    assert callable(evaluator.RolloutEngine.last_rollout_weights)
    assert evaluator.check_lane_weights('regrouped', 'laneg') is True and evaluator.check_lane_weights(None, 'wave') is False

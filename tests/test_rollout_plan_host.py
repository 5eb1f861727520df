"""The launch planner (csrc/serl_plan.h behind serl_host_plan_rollout / _dyn / _multi) without a GPU: every launch the parent commit made on the card for the
cases of tools/record_rollout_plan.py (tests/golden/rollout_plan.npz) is planned again from the recorded CU count and override, the AUTO tables the code's
comments state hold at 4 and 32 CUs, every plan of an exhaustive sweep covers its episodes exactly once within the device, and the ABI has not moved."""
import ctypes, itertools, os
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED = 0, -3
FAM = dict(team=1, teams=2, teams2=3, teamx=4, team2=5, team2s=6, team4=7, team4_mixed=8, half=9, wave=10, wavex=11, lane=12, teamr=13)
AUTO, TEAM, WAVE, HALF, TEAM2, TEAM4, LANEQ = range(7)
_PER_WAVE = (FAM['lane'], FAM['wave'], FAM['wavex'], FAM['half'])
_ONE_PER_CU = (FAM['team'], FAM['teams'], FAM['teamr'])


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()


def _caps(num_cus, kernel=0, wpb=-1, laneq_waves=-1, split=0, remote=1, regroup=1):
    return (ctypes.c_int32 * 7)(num_cus, kernel, wpb, laneq_waves, split, remote, regroup)


def _param_count(S, A, H, L):
    return H * S + H + L * (H * H + 3 * H) + A * H + A


def _desc(n, S=7, A=3, H=32, L=3, hint=AUTO, lanes=0, conc=0, env=0, incremental=0, members=1):
    from serl_amd import _capi
    return _capi.RolloutDesc(state_dim=S, action_dim=A, hidden=H, num_layers=L, activation=0, n_members=members, weight_stride=(_param_count(S, A, H, L) + 3) // 4 * 4,
                             n_episodes=n, max_steps=1, lanes_per_wave=lanes, kernel_hint=hint, concurrent_episodes=conc, env_config=env, incremental=incremental)


def _plan(L, caps, d, noise=0):
    """(status, the 16 words)"""
    out = (ctypes.c_int32 * 16)()
    st = L.serl_host_plan_rollout(caps, ctypes.byref(d), noise, out)
    return st, list(out)


@pytest.fixture(scope='module')
def recorded():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'rollout_plan.npz')) as z:
        return {k: z[k] for k in z.files}


def test_every_recorded_launch_is_planned_again(recorded):
    golden = recorded
    L = _lib()
    cols = [str(c) for c in golden['cols']]
    assert len(golden['cases']) > 300 and set(golden['info'][:, 0]) >= set(FAM.values()) - {FAM['team4_mixed']}      # (every family was recorded)
    bad = []
    for row, status, info in zip(golden['cases'], golden['status'], golden['info']):
        r = dict(zip(cols, (int(v) for v in row)))
        caps = (ctypes.c_int32 * 7)(*[int(v) for v in golden['caps'][r['override']]])
        out = (ctypes.c_int32 * 16)()
        if r['entry'] == 2:
            st = L.serl_host_plan_dyn(caps, r['n_episodes'], r['lanes_per_wave'], r['kernel_hint'], out)
        else:
            d = _desc(r['n_episodes'], r['state_dim'], r['action_dim'], r['hidden'], r['num_layers'], r['kernel_hint'], r['lanes_per_wave'],
                      r['concurrent_episodes'], r['env_config'], r['incremental'], r['n_members'])
            st = L.serl_host_plan_rollout(caps, ctypes.byref(d), r['entry'], out)
        got = list(out)[:8]
        if st == OK:
            got[7] = int(info[7])      # (the code variant is the build's, not the planner's)
        if st != int(status) or got != [int(v) for v in info]:
            bad.append((r, int(status), [int(v) for v in info], st, got))
    assert not bad, '%d of %d rows differ, first: %s' % (len(bad), len(golden['cases']), bad[:3])


def test_recorded_multi_splits(recorded):
    golden = recorded
    L = _lib()
    cus = int(golden['num_cus'])
    for parts, status, info in zip(golden['multi_parts'], golden['multi_status'], golden['multi_info']):
        parts = [int(p) for p in parts if p > 0]
        n = len(parts)
        grids, queue, place = (ctypes.c_int32 * 4)(), ctypes.c_int32(), ctypes.c_int32()
        assert L.serl_host_plan_multi(cus, n, (ctypes.c_int32 * n)(*parts), 2, grids, ctypes.byref(queue), ctypes.byref(place)) == OK
        g = list(grids)[:n]
        assert int(status) == OK and int(info[0]) == FAM['team4_mixed']
        assert sum(g) == int(info[1]) and any(4 * gk < p for gk, p in zip(g, parts)) == bool(info[3]), (parts, g, list(info))
        assert queue.value == (sum(parts) > 4 * cus) and place.value == 2


def test_multi_split_fits_the_device():
    L = _lib()
    cus = 256
    for parts in itertools.product((1, 85, 341, 342, 2000), repeat=3):
        grids, queue, place = (ctypes.c_int32 * 4)(), ctypes.c_int32(), ctypes.c_int32()
        assert L.serl_host_plan_multi(cus, 3, (ctypes.c_int32 * 3)(*parts), 2, grids, ctypes.byref(queue), ctypes.byref(place)) == OK
        g = list(grids)[:3]
        assert all(1 <= gk <= (p + 3) // 4 for gk, p in zip(g, parts)), (parts, g)
        assert sum(g) <= cus or all(gk == 1 for gk in g), (parts, g)
        # a part whose workgroups do not hold all its episodes drains a queue: serl_rollout_multi gives exactly these parts a counter, and only a
        # launch beyond four per CU, or one the overflow was cut from, has any
        short = [4 * gk < p for gk, p in zip(g, parts)]
        assert not any(short) or queue.value or sum((p + 3) // 4 for p in parts) > cus, (parts, g)
        assert place.value == (1 if sum(g) > cus else 2)


def _auto(lib, cus, n, **kw):
    st, o = _plan(lib, _caps(cus), _desc(n, **kw))
    assert st == OK, (cus, n, kw)
    return dict(family=o[0], grid=o[1], per_team=o[2], queue=o[3], launches=o[6], block=o[8], lanes=o[9], q0=o[10], regroup=o[11], mail=o[12], chunk=o[14])


def test_auto_table_at_4_cus_hidden_32():
    L = _lib()
    for n in range(1, 400):
        p = _auto(L, 4, n)
        if n <= 4:
            want = dict(family=FAM['team'], grid=n, per_team=1, queue=0)
        elif n <= 8:
            want = dict(family=FAM['team2'], grid=(n + 1) // 2, per_team=2, queue=0)
        elif n <= 16:
            want = dict(family=FAM['team4'], grid=(n + 3) // 4, per_team=4, queue=0)
        elif n < 320:
            want = dict(family=FAM['team4'], grid=4, per_team=4, queue=1, q0=16)
        else:
            want = dict(family=FAM['lane'], lanes=64, per_team=64, regroup=1, queue=0)
        assert {k: p[k] for k in want} == want, (n, p)


def test_auto_table_at_32_cus_hidden_72():
    L = _lib()
    for n in range(1, 200):
        p = _auto(L, 32, n, H=72, L=1)
        if n <= 16:
            want = dict(family=FAM['teamr'], grid=16 * ((n + 7) // 8), mail=256 * n, block=512)
        elif n <= 32:
            want = dict(family=FAM['teams'], grid=n, mail=0, block=128)
        elif n <= 64:
            want = dict(family=FAM['team2s'], grid=(n + 1) // 2, per_team=2, queue=0)
        else:
            want = dict(family=FAM['wave'], per_team=1, queue=0)
        assert {k: p[k] for k in want} == want, (n, p)


def test_auto_table_of_the_general_env_configurations_at_4_cus():
    L = _lib()
    for env, incremental, S, A in ((0, 1, 10, 3), (1, 0, 2, 1), (2, 0, 13, 3)):
        for n in range(1, 40):
            p = _auto(L, 4, n, S=S, A=A, L=1, env=env, incremental=incremental)
            if n <= 8:
                want = dict(family=FAM['teamx'], launches=1 if n <= 4 else 2, grid=n if n <= 4 else n - 4, chunk=n if n <= 4 else 4, block=512)
            else:
                want = dict(family=FAM['wavex'], launches=1, per_team=1)
            assert {k: p[k] for k in want} == want, (env, incremental, n, p)


def _covers(v, cus, n, conc, hint):
    """an accepted plan `v` (the 16 words) starts every one of n episodes exactly once, within a device of `cus` CUs"""
    family, grid, per_team, queue, launches, block, pl, q0, mail, chunk = v[0], v[1], v[2], v[3], v[6], v[8], v[9], v[10], v[12], v[14]
    ok = block % 64 == 0 and 64 <= block <= 512 and 1 <= pl <= 64 and grid >= 1 and launches >= 1
    wpb = block // 64
    # episodes one workgroup starts on: a team's lane groups, or one per wavefront / `lanes` per wavefront of the wave and lane kernels
    unit = per_team * (wpb if family in _PER_WAVE else 1)
    if family == FAM['teamr']:      # (two workgroups per episode, in groups of sixteen; every workgroup of the launches together resident)
        ok = ok and grid == 16 * ((n + 7) // 8) and mail == 256 * n and 16 * ((n + conc + 7) // 8) <= cus
    elif queue:      # (the lane kernel's slots are those of its wavefronts; a last workgroup may hold wavefronts beyond them)
        ok = ok and 0 < q0 < n and (q0 == grid * unit if family != FAM['lane'] else (grid - 1) * unit < q0 <= grid * unit)
    elif launches > 1:
        ok = ok and family == FAM['teamx'] and (launches - 1) * chunk + grid == n and grid <= chunk
    else:
        ok = ok and grid * unit >= n and chunk == n
    if family != FAM['teamr']:
        ok = ok and mail == 0
    if queue or (family in _ONE_PER_CU and hint == AUTO):      # alone on the GPU: one workgroup per CU
        ok = ok and (conc > 0 or grid <= cus)
    return ok


def test_every_plan_covers_its_episodes_within_the_device():
    L = _lib()
    plan = L.serl_host_plan_rollout
    seen = 0
    for cus in (1, 4, 32):
        caps = _caps(cus)
        for H, layers in ((32, 3), (72, 1)):
            for hint, lanes, conc in itertools.product(range(7), (0, 1, 64, 65), (0, 3)):
                d = _desc(1, H=H, L=layers, hint=hint, lanes=lanes, conc=conc)
                ref, out, out_nz = ctypes.byref(d), (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)()
                for n in range(1, 100 * cus + 1):
                    d.n_episodes = n
                    st, st_nz = plan(caps, ref, 0, out), plan(caps, ref, 1, out_nz)
                    seen += 2
                    assert st in (OK, UNSUPPORTED) and st_nz in (OK, UNSUPPORTED)
                    if st == OK and out[0] in (FAM['lane'], FAM['wave'], FAM['wavex']) and (hint in (AUTO, WAVE) or (lanes > 0 and hint != LANEQ)):
                        assert st_nz == OK and out_nz[:] == out[:], (cus, H, hint, lanes, conc, n)
                    for s, o in ((st, out), (st_nz, out_nz)):
                        v = o[:]
                        assert (not any(v)) if s != OK else _covers(v, cus, n, conc, hint), (cus, H, hint, lanes, conc, n, s, v)
    assert seen == 2 * 2 * 7 * 4 * 2 * 100 * (1 + 4 + 32)


def test_planner_through_the_package():
    import serl_amd
    from serl_amd import evaluator
    _lib()
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    p = evaluator.plan_rollout(spec, 1023, num_cus=256)
    assert (p['family'], p['workgroups'], p['episodes_per_team'], p['work_queue'], p['code'], p['block'], p['timed']) == ('team4', 256, 4, False, -1, 512, True)
    p = evaluator.plan_rollout(spec, 1025, num_cus=256, concurrent_episodes=1025)
    assert (p['family'], p['workgroups'], p['work_queue'], p['first_queued'], p['timed']) == ('team4', 128, True, 512, False)
    p = evaluator.plan_rollout(None, 300, num_cus=256, open_loop=True)
    assert (p['family'], p['workgroups'], p['block'], p['actor_streamed']) == ('wave', 150, 128, False)
    assert evaluator.plan_rollout(spec, 200, caps=evaluator.planner_caps(256, {'SERL_LANEQ_WAVES': '2'}), kernel='laneq')['work_queue']
    with pytest.raises(RuntimeError, match=r'\(-3\).*no noise instantiation'):
        evaluator.plan_rollout(spec, 8, num_cus=256, kernel='team', noise=True)
    with pytest.raises(RuntimeError, match=r'\(-3\).*TEAM or WAVE kernels'):
        evaluator.plan_rollout(serl_amd.NetSpec(2, 1, 32, 1, 'tanh'), 8, num_cus=256, kernel='half', env_config=1)


def test_the_abi_has_not_moved():
    from serl_amd import _capi
    L = _lib()
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 == len(_capi.expected_layout())
    for name, want in (('serl_venv_auto_layout', _capi.expected_venv_auto_layout()), ('serl_venv_rollout_layout', _capi.expected_venv_rollout_layout()),
                       ('serl_venv_noise_layout', _capi.expected_venv_noise_layout()), ('serl_rollout_noise_layout', _capi.expected_rollout_noise_layout()),
                       ('serl_td3_layout', _capi.expected_td3_layout()), ('serl_td3_rng_layout', _capi.expected_td3_rng_layout())):
        got = (ctypes.c_int32 * len(want))()
        assert getattr(L, name)(got, len(want)) == len(want) and list(got) == want, name
    got = (ctypes.c_int32 * 62)()
    L.serl_abi_layout(got, 62)
    assert list(got) == _capi.expected_layout()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    for f in ('serl_host_plan_rollout', 'serl_host_plan_dyn', 'serl_host_plan_multi'):
        assert f in _capi.EXPORTS and hasattr(L, f) and ('int %s(' % f) in hdr

"""The env's counter-based noise generator without a GPU (serl_amd/csrc/serl_rng.h through the host exports serl_host_philox /
serl_host_uniform, compiled from the kernels' text): the bits against a NumPy restatement of Philox4x32-10 (tests/rng_ref.py), the
uniform against its formula, the layout of serl_venv_noise_desc against its ctypes mirror and the header, and every refusal of the
serl_venv_*_noise entries, which come before the context is read."""
import ctypes, os, re
import numpy as np
import pytest

import rng_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from serl_amd import build, _capi
    build.build()
    return _capi.lib()                    # raises when a ctypes mirror differs from the library's layout self-checks


def _host_philox(L, seed, c):
    out = (ctypes.c_uint32 * 4)()
    L.serl_host_philox(int(seed), int(c[0]), int(c[1]), int(c[2]), int(c[3]), out)
    return list(out)


def test_host_philox_equals_the_numpy_restatement():
    L = _lib()
    rng = np.random.RandomState(20261018)
    ctr = rng.randint(0, 2**32, size=(1002, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.randint(0, 2**32, size=(1002, 2), dtype=np.uint64).astype(np.uint32)
    ctr[1000], key[1000] = 0, 0
    ctr[1001], key[1001] = 0xFFFFFFFF, 0xFFFFFFFF
    want = rng_ref.philox4x32_10(key, ctr)
    for i in range(len(ctr)):
        seed = int(key[i, 0]) | int(key[i, 1]) << 32         # the key is the 64-bit seed: low word, high word
        assert _host_philox(L, seed, ctr[i]) == [int(v) for v in want[i]], (i, ctr[i], key[i])


def test_known_answers_of_random123():
    """The known-answer vectors of Random123's kat_vectors for philox4x32 with 10 rounds, as remembered -- the restatement in tests/rng_ref.py,
    written from the published round function and constants, is the authority: a vector that disagreed with it would be the one to drop.
    All three agree with it (asserted here), and the library agrees with them."""
    L = _lib()
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        ref = rng_ref.philox4x32_10(np.array(key, np.uint32), np.array(ctr, np.uint32))
        assert [int(v) for v in ref] == list(out), 'remembered vector differs from the restatement'
        assert _host_philox(L, key[0] | key[1] << 32, ctr) == list(out)


def test_counter_layout_of_the_streams():
    """words(seed; env, episode, entry, stream, block) of the restatement is the call with counter (env, episode, entry, stream << 16 | block)"""
    L = _lib()
    seed = 0x0123456789abcdef
    for env, ep, entry, stream, block in ((0, 0, 0, 0, 0), (69, 3, 6, 0, 3), (65535, 2**31 - 1, 8000, 1, 1), (5, 0, 1, 1, 0)):
        want = rng_ref.words(seed, env, ep, entry, stream, block)
        assert _host_philox(L, seed, (env, ep, entry, stream << 16 | block)) == [int(v) for v in want]


def test_host_uniform_is_exact_and_strictly_inside_the_unit_interval():
    L = _lib()
    rng = np.random.RandomState(7)
    w = rng.randint(0, 2**32, size=(1000, 2), dtype=np.uint64)
    w = np.concatenate([w, [[0, 0], [0xffffffff, 0xffffffff], [0, 0xfff], [0, 0x1000], [0xffffffff, 0], [1, 0]]]).astype(np.uint64)
    for w0, w1 in w:
        k = (int(w0) << 20) | (int(w1) >> 12)
        want = (2 * k + 1) * 2.0 ** -53                       # 2 k + 1 < 2^53: exact
        got = L.serl_host_uniform(int(w0), int(w1))
        assert got == want and 0.0 < got < 1.0, (w0, w1, got, want)
        assert got == float(rng_ref.uniform(w0, w1))
    assert L.serl_host_uniform(0, 0) == 2.0 ** -53
    assert L.serl_host_uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53


def test_noise_layout_equals_the_ctypes_mirror_and_the_header():
    from serl_amd import _capi
    L = _lib()
    for f in ('serl_venv_noise_layout', 'serl_venv_reset_noise', 'serl_venv_step_auto_noise', 'serl_venv_rollout_noise',
              'serl_venv_rollout_general_noise', 'serl_venv_noise_fill', 'serl_venv_actor_forward', 'serl_host_philox', 'serl_host_uniform'):
        assert f in _capi.EXPORTS and hasattr(L, f)
    D = _capi.VenvNoiseDesc
    want = _capi.expected_venv_noise_layout()
    assert want == [ctypes.sizeof(D)] + [getattr(D, f).offset for f, _ in D._fields_] == [160, 0, 8, 16, 20, 24, 80, 136, 140, 144, 152]
    assert L.serl_venv_noise_layout(None, 0) == len(want) == 11
    got = (ctypes.c_int32 * len(want))()
    assert L.serl_venv_noise_layout(got, len(want)) == len(want) and list(got) == want
    short = (ctypes.c_int32 * 3)(-1, -1, -1)
    assert L.serl_venv_noise_layout(short, 2) == len(want) and list(short) == want[:2] + [-1]
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    body = re.search(r'typedef struct serl_venv_noise_desc \{(.*?)\} serl_venv_noise_desc;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'(\w+)(?:\[\d+\])?\s*[;,]', body)
    assert names == [f for f, _ in D._fields_], names
    # nothing else moved
    assert L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert L.serl_abi_layout(None, 0) == 62 and L.serl_venv_auto_layout(None, 0) == 10 and L.serl_venv_rollout_layout(None, 0) == 25


def test_noise_entries_refuse_bad_descriptors_before_reading_the_context():
    """Every refusal of the serl_venv_*_noise entries that belongs to `nz` comes before anything reads the context or the stream: the
    context here is NULL or a pointer that is never dereferenced, the stream NULL."""
    from serl_amd import _capi
    L = _lib()
    E = _capi.E_INVALID
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    p -= p % 16
    ref = lambda s: None if s is None else ctypes.byref(s)

    def nzd(**kw):
        d = dict(seed=1, episode_count=p, sensor=1, action=0, action_sd=0.3, action_clip=0.5)
        d.update(kw)
        return _capi.VenvNoiseDesc(**d)
    desc = lambda **kw: _capi.VenvDesc(**dict(dict(n_envs=4, state_dim=7, action_dim=3, max_steps=10, t_max=0.1), **kw))
    ro = lambda **kw: _capi.VenvRolloutDesc(**dict(dict(state_dim=7, action_dim=3, hidden=32, num_layers=3, activation=0, n_members=1, weights=p,
                                                        weight_stride=3716, n_steps=5, obs=p), **kw))
    au = _capi.VenvAutoDesc(final_obs=p, ep_return=p, ep_length=p, run_return=p, run_length=p, cursor=p)
    nul = [None] * 7
    calls = {
        'reset': lambda c, d, r, nz: L.serl_venv_reset_noise(c, ref(d), None, p, ref(nz), None),
        'step_auto': lambda c, d, r, nz: L.serl_venv_step_auto_noise(c, ref(d), p, 1, p, p, p, None, None, None, None, ref(au), ref(nz), None),
        'rollout': lambda c, d, r, nz: L.serl_venv_rollout_noise(c, ref(d), ref(au), ref(r), ref(nz), None),
        'rollout_general': lambda c, d, r, nz: L.serl_venv_rollout_general_noise(c, ref(d), ref(au), ref(r), ref(nz), None),
    }
    for name, call in calls.items():
        for ctx in (None, ctypes.c_void_p(8)):
            assert call(ctx, desc(), ro(), None) == E and b'nz is NULL' in L.serl_last_error(), name
            assert call(ctx, desc(), ro(), nzd(episode_count=None)) == E and b'episode_count' in L.serl_last_error(), name
            assert call(ctx, desc(sensor_noise=p), ro(), nzd()) == E and b'desc->sensor_noise together with nz->sensor' in L.serl_last_error(), name
            for kw in (dict(action_sd=-0.1), dict(action_clip=-1.0), dict(action_sd=float('nan'))):
                assert call(ctx, desc(), ro(), nzd(**kw)) == E and b'action_sd' in L.serl_last_error(), (name, kw)
            assert call(ctx, desc(), ro(), nzd(sensor=2)) == E
            if name.startswith('rollout'):
                assert call(ctx, desc(), ro(action_noise=p), nzd(action=1)) == E and b'ro->action_noise together with nz->action' in L.serl_last_error(), name
        # a table beside a generator that is switched off is no conflict: with a NULL context the call gets as far as the context check
        assert call(None, desc(sensor_noise=p), ro(action_noise=p), nzd(sensor=0, action=0)) == E and b'NULL argument' in L.serl_last_error(), name
    # the fill entry
    i32 = (ctypes.c_int32 * 4)()
    q = ctypes.cast(i32, ctypes.c_void_p)
    fill = lambda c, nz, mode, rows, entries, out=q: L.serl_venv_noise_fill(c, ref(nz), mode, rows, q, q, q, entries, out, None)
    assert fill(None, nzd(), 0, 1, 1) == E and fill(ctypes.c_void_p(8), None, 0, 1, 1) == E and fill(ctypes.c_void_p(8), nzd(), 0, 1, 1, None) == E
    for mode, rows, entries in ((-1, 1, 1), (4, 1, 1), (0, 0, 1), (1, 1, 0)):
        assert fill(ctypes.c_void_p(8), nzd(), mode, rows, entries) == E, (mode, rows, entries)
    assert fill(ctypes.c_void_p(8), nzd(action_sd=-1.0), 3, 1, 1) == E and b'action_sd' in L.serl_last_error()
    # the stand-alone actor forward
    fwd = lambda c, r, n=4, o=p, a=p: L.serl_venv_actor_forward(c, ref(r), n, o, a, None)
    ctx = ctypes.c_void_p(8)
    assert fwd(None, ro()) == E and fwd(ctx, None) == E and fwd(ctx, ro(), 4, None) == E and fwd(ctx, ro(), 4, p, None) == E
    for kw, rc in ((dict(weights=None), E), (dict(n_members=0), E), (dict(state_dim=17), E), (dict(action_dim=4), E), (dict(activation=3), E),
                   (dict(weight_stride=3715), E), (dict(weights=p + 4), E), (dict(hidden=132), _capi.E_UNSUPPORTED), (dict(hidden=30), _capi.E_UNSUPPORTED),
                   (dict(num_layers=17), _capi.E_UNSUPPORTED)):
        assert fwd(ctx, ro(**kw)) == rc, kw
    assert fwd(ctx, ro(), 0) == E and b'n_envs' in L.serl_last_error()


def test_python_arguments_are_checked_before_any_device_work():
    import serl_amd
    from serl_amd import builds
    with pytest.raises(ValueError, match='auto_reset'):
        serl_amd.CitationVecEnv(4, mode='noise', sensor_noise='device')
    with pytest.raises(ValueError, match='auto_reset'):
        serl_amd.CitationVecEnv(4, mode='noise', seed=3)
    with pytest.raises(ValueError, match='sensor_noise'):
        serl_amd.CitationVecEnv(4, mode='noise', sensor_noise='host', auto_reset=True)
    with pytest.raises(ValueError, match='seed'):
        serl_amd.CitationVecEnv(4, mode='noise', sensor_noise='device', auto_reset=True, seed=-1)
    for kw in (dict(kind='words'), dict(kind='action'), dict(kind='action', noise_sd=-1.0, noise_clip=0.5), dict(entries=0), dict(seed=2**64)):
        args = dict(dict(seed=1, env=0, episode=0, entries=3), **kw)
        with pytest.raises(ValueError):
            serl_amd.venv_noise(**args)
    # sensor_bias_scale holds sensor_terms' own sub-expressions: bias + scale z is sensor_terms(z) bit for bit
    bias, scale = builds.sensor_bias_scale()
    z = np.random.RandomState(3).randn(1000, 7)
    np.testing.assert_array_equal(bias + scale * z, builds.sensor_terms(z))
    env = object.__new__(serl_amd.CitationVecEnv)      # (never touched a device: only what rollout()'s argument checks read)
    env.n_envs, env.state_dim, env.action_dim, env.auto_reset = 6, 7, 3, True
    for kw in (dict(action_noise='device'), dict(action_noise='device', noise_sd=0.3), dict(action_noise='device', noise_sd=-0.3, noise_clip=0.5),
               dict(action_noise='host', noise_sd=0.3, noise_clip=0.5), dict(noise_sd=0.3)):
        with pytest.raises(ValueError, match='noise'):
            env.rollout(None, 5, **kw)

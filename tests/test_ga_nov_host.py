"""serl_ga_novelty_general without a GPU: the float64 contract of tests/nov64.py (the Actor module's get_novelty against the kernel's
steps written out by hand over the ring layout, the planted slips, the float32 reference under the bound), ga.distance_plan against
ring.sample_from_latest call for call, the new symbol and its argument checks in their documented order, and the kernel / dense choices
of the Python layer."""
import ctypes, os, random, re, sys, types
import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nov64 as Z

KEYS = list(range(len(Z.GRID)))


def _id(key):
    return Z.case_id(Z.GRID[key])


@pytest.mark.parametrize('key', KEYS, ids=_id)
def test_by_hand_equals_the_module_and_the_f32_path_is_under_the_bound(key):
    case, ref = Z.reference(key)
    rings, slots = Z.ring_layout(case)
    np.testing.assert_allclose(Z.by_hand64(case, rings, slots), ref, rtol=1e-12)
    got = [Z.novelty32_torch(case['c'], case['weights'][m], case['states'][k], case['actions'][k]) for k, m in enumerate(case['members'])]
    assert Z.rel_err(got, ref).max() <= Z.WORST_REF * 1.0001 < Z.TOL
    assert ref.min() > 0.05                       # no case rests on cancellation: the values are of order 1
    assert ref[0] == ref[2] and len(set(ref.tolist())) == 3          # the member listed twice is judged on the same batch


def test_the_grid_is_the_issues():
    assert Z.GRID == [(7, 3, 4, 0, 'tanh', 1), (7, 3, 32, 3, 'tanh', 86), (7, 3, 72, 3, 'elu', 256), (7, 3, 96, 3, 'relu', 128),
                      (7, 3, 128, 4, 'tanh', 129), (16, 4, 128, 3, 'elu', 512), (1, 1, 8, 1, 'relu', 127), (13, 3, 100, 2, 'tanh', 2)]
    assert list(Z.MEMBERS) == [2, 0, 2, 1] and Z.TOL == 4 * Z.WORST_REF


@pytest.mark.parametrize('slip', Z.SLIPS)
def test_planted_slips_exceed_the_bound(slip):
    """every slip moves some evaluation of the grid by more than TOL (by orders of magnitude), and the cases it cannot show on are the
    expected ones"""
    seen = {}
    for key in KEYS:
        case, ref = Z.reference(key)
        rings, slots = Z.ring_layout(case)
        seen[case['B']] = float(Z.rel_err(Z.by_hand64(case, rings, slots, slip), ref).max())
    print(slip, seen)
    assert max(seen.values()) > 1000 * Z.TOL
    if slip == 'mean_128':
        assert seen[128] < 1e-12 and all(v > 1e-3 for B, v in seen.items() if B != 128)
    if slip == 'padded_counted':
        assert all((v < 1e-12) == (B % Z.CHUNK == 0) for B, v in seen.items()) and all(v < 1e-12 or v > 1e-3 for v in seen.values())
    if slip == 'first_chunk_only':
        assert all((v > 1e-3) == (B > Z.CHUNK) for B, v in seen.items())
    if slip in ('action_offset', 'neighbour_slots', 'square_of_sum'):
        assert all(v > 1e-3 for B, v in seen.items() if not (slip == 'square_of_sum' and B == 127))      # (B 127 is the A = 1 case)


# ---- distance_plan ------------------------------------------------------------------------------------------------------------------
def _rings(seed=3):
    """five CPU rings: partly filled, wrapped (capacity below 1000 -> the whole ring, rotated), shorter than 1000, longer than 1000 and
    wrapped past its capacity, and one of 120 rows: fills 300, 700, 40, 2600, 120"""
    from serl_amd.replay import DeviceReplay
    g = torch.Generator().manual_seed(seed)
    out = []
    for cap, n in ((5000, 300), (700, 1900), (5000, 40), (2600, 4000), (1500, 120)):
        r = DeviceReplay(cap, 'cpu')
        for lo in range(0, n, 900):                # (several appends: the position wraps)
            r.append_rows(torch.rand(min(900, n - lo), r.row, generator=g))
        out.append(r)
    assert [len(r) for r in out] == [300, 700, 40, 2600, 120]
    assert out[1].position == 1900 % 700 and out[3].position == 4000 % 2600
    return out


def test_distance_plan_equals_sample_from_latest_call_for_call():
    from serl_amd import ga
    rings = _rings()
    genomes = [3, 0, 4, 1, 2]
    buffers = {k: rings[k] for k in range(5)}
    rng = random.Random(11)
    plan = ga.distance_plan(genomes, buffers, rng)
    ref = random.Random(11)
    pairs, e = [], 0
    for i, first in enumerate(genomes):
        for second in genomes[i + 1:]:
            bs = min(256, len(rings[first]), len(rings[second]))
            b1 = rings[first].sample_from_latest(bs, 1000, ref)             # mod_neuro_evo.py:411-417: gene1's buffer first
            b2 = rings[second].sample_from_latest(bs, 1000, ref)
            pairs.append((second, first, bs))
            # evaluation e: `first` on second's batch; e + 1: `second` on first's
            for ev, member, ring, want in ((e, first, rings[second], b2), (e + 1, second, rings[first], b1)):
                assert plan['members'][ev] == member and plan['rings'][ev] is ring and plan['batch'][ev] == bs
                got = ring.split(ring.rows[torch.from_numpy(plan['slots'][ev, :bs].astype(np.int64))])
                for a, b in zip(got, want):
                    assert torch.equal(a, b)
                assert (plan['slots'][ev, bs:] == 0).all() and 0 <= plan['slots'][ev].min() and plan['slots'][ev].max() < ring.capacity
            assert plan['calls'][e:e + 2] == [e + 1, e]
            e += 2
    assert plan['pairs'] == pairs and e == 20 == len(plan['members'])
    assert plan['slots'].shape == (20, 256) and plan['slots'].dtype == np.int32 and plan['batch'].dtype == np.int32
    assert sorted(set(plan['batch'].tolist())) == [40, 120, 256]
    assert rng.getstate() == ref.getstate()
    # no pairs: nothing drawn
    state = rng.getstate()
    assert ga.distance_plan([2], buffers, rng)['pairs'] == [] and rng.getstate() == state


def test_choices_are_checked_before_any_draw():
    import serl_amd
    from serl_amd import ga, ssne
    spec = serl_amd.NetSpec(7, 3, 32, 3, 'tanh')
    w, st, ac = torch.zeros(2, spec.param_count), torch.zeros(1, 4, 7), torch.zeros(1, 4, 3)
    rings = _rings()
    rng = random.Random(5)
    state = rng.getstate()
    for kw, msg in ((dict(kernel='bogus'), 'kernel must be one of'), (dict(dense='bogus'), 'dense must be one of'),
                    (dict(kernel='lds', dense='mfma'), 'needs kernel'), (dict(dense='mfma'), 'needs kernel')):
        with pytest.raises(ValueError, match=msg):
            ga.novelty(None, w, [0], spec, st, ac, **kw)
        with pytest.raises(ValueError, match=msg):
            ga.sort_groups_by_distance(None, w, [0, 1], {0: rings[0], 1: rings[1]}, spec, rng, **kw)
        args = types.SimpleNamespace(pop_size=4, elite_fraction=0.25, mut_type='normal')
        with pytest.raises(ValueError, match=msg):
            ssne.SSNE(args, None, spec, **{'novelty_' + k: v for k, v in kw.items()})
    assert rng.getstate() == state
    s = ssne.SSNE(args, None, spec, novelty_kernel='general', novelty_dense='mfma')
    assert (s.novelty_kernel, s.novelty_dense) == ('general', 'mfma')
    assert (ssne.SSNE(args, None, spec).novelty_kernel, ssne.SSNE(args, None, spec).novelty_dense) == ('lds', 'valu')
    # an empty buffer is refused before anything reaches a kernel (no engine here)
    from serl_amd.replay import DeviceReplay
    with pytest.raises(ValueError, match='empty buffer'):
        ga.sort_groups_by_distance(None, w, [0, 1], {0: rings[0], 1: DeviceReplay(100, 'cpu')}, spec, rng, kernel='general')


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------
def test_export_header_and_argument_checks_in_the_documented_order_without_a_gpu():
    """INVALID (pointers, count) -> INVALID (dense) -> UNSUPPORTED (shape, max_batch) -> OK (no evaluations) -> INVALID (strides): none of
    them reads the context or launches (a NULL context is itself refused), and the output keeps its sentinel"""
    from serl_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, 'include', 'serl_amd.h')).read()
    assert 'serl_ga_novelty_general' in _capi.EXPORTS and hasattr(L, 'serl_ga_novelty_general')
    assert re.search(r'^int serl_ga_novelty_general\(', hdr, re.M)
    assert re.search(r'#define SERL_ABI_VERSION 9\b', hdr) and L.serl_abi_version() == 9 == _capi.ABI_VERSION
    assert 'serl_ga_novelty_general_work_bytes' not in hdr            # tapeless: no workspace, no size entry
    buf = np.zeros(64, np.float32)
    out = np.full(8, 777.0, np.float32)
    p, o = buf.ctypes.data, out.ctypes.data
    ctx = ctypes.c_void_p(p)                            # never dereferenced: every call below returns from the argument checks
    P = 72 * 7 + 72 + 3 * (72 * 72 + 3 * 72) + 3 * 72 + 3

    def call(ctx=ctx, weights=p, stride=P, S=7, H=72, L_=3, A=3, act=0, members=p, n=2, sb=p, ss=20, ab=p, as_=20, slots=p, n_rows=p, batch=p,
             max_batch=256, novelty=o, dense=0):
        return L.serl_ga_novelty_general(ctx, weights, stride, S, H, L_, A, act, members, n, sb, ss, ab, as_, slots, n_rows, batch, max_batch,
                                         novelty, dense, None)
    for kw in (dict(ctx=None), dict(weights=None), dict(members=None), dict(sb=None), dict(ab=None), dict(n_rows=None), dict(batch=None),
               dict(novelty=None), dict(n=-1), dict(dense=2), dict(dense=-1)):
        assert call(**kw) == _capi.E_INVALID, kw
        assert b'serl_ga_novelty_general' in L.serl_last_error()
    for kw in (dict(H=132), dict(H=70), dict(H=0), dict(L_=5), dict(L_=-1), dict(S=17), dict(S=0), dict(A=5), dict(A=0), dict(act=3), dict(act=-1),
               dict(max_batch=513), dict(max_batch=0), dict(max_batch=-1)):
        assert call(**kw) == _capi.E_UNSUPPORTED, kw
        assert b'serl_ga_novelty_general' in L.serl_last_error() and b'4 .. 128' in L.serl_last_error()
    # the sentence of the other two general entries
    tail = b'compiled for hidden a multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, state_dim 1 .. 16, action_dim 1 .. 4, the three activations, minibatches of 1 .. 512 rows'
    assert L.serl_last_error().endswith(tail)
    assert call(novelty=None, dense=7, H=70) == _capi.E_INVALID and b'bad argument' in L.serl_last_error()
    assert call(dense=7, H=70) == _capi.E_INVALID and b'dense' in L.serl_last_error()
    assert call(H=70, n=0) == _capi.E_UNSUPPORTED and call(H=70, stride=1) == _capi.E_UNSUPPORTED
    assert call(n=0, stride=1, ss=0, as_=0, slots=None) == 0
    assert call(stride=P - 1) == _capi.E_INVALID and b'stride' in L.serl_last_error()
    assert call(ss=6) == _capi.E_INVALID and b'stride' in L.serl_last_error()
    assert call(as_=2) == _capi.E_INVALID and b'stride' in L.serl_last_error()
    assert (out == 777.0).all() and (buf == 0).all()

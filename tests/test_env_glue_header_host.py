"""serl_amd/csrc/env_glue.h on the host: the statements of the env step the kernels share (no-fault row, fault row on a command, sensor add,
observation), compiled with g++ -O2 -ffp-contract=off (tests/tools/env_glue_host.cpp) and held bit for bit to the flown records of
tests/env_glue.py -- a reading of the reference that shares nothing with the header.  Every step of every scenario: the plant's command from
the env's deflections and the fault row, and the observation from the errors, the observed states and last_u.  No dynamics run.  No GPU."""
import os, subprocess, types
import numpy as np
import pytest
import env_glue as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 3 + 16      # per step: cmd, obs (16 slots)
# fault rows beyond the scenarios': a negative gain (reset()'s 0 * gain is -0.0 and stays so), zero clips, gain + clip + jam together
EXTRA_FAULTS = [(-0.5, G.INF, G.INF, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 0.0), (-2.0, 0.0, G.INF, 1.0, -0.1)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _plant(fault, u):
    """GlueEnv._plant without a dynamics build behind it"""
    return G.GlueEnv._plant(types.SimpleNamespace(fault=G.fault_row(fault), bug=None), u)


def _cases():
    """the scenarios, and the record of fault_be under each extra fault row (the deflections come from the record: only the plant's command changes)"""
    out = [(s, G.flown(s['name'])) for s in G.scenarios()]
    base = [s for s in G.scenarios() if s['name'] == 'fault_be'][0]
    for i, f in enumerate(EXTRA_FAULTS):
        out.append((dict(base, name='extra_fault_%d' % i, fault=f), G.flown('fault_be')))
    return out


@pytest.fixture(scope='module')
def replay(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('env_glue_host')
    exe = str(tmp / 'env_glue_host')
    subprocess.run(['g++', '-O2', '-ffp-contract=off', '-I', os.path.join(ROOT, 'serl_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'tools', 'env_glue_host.cpp'), '-o', exe], check=True)
    cases = _cases()
    words = [float(len(cases))]
    for sc, o in cases:
        n, A = o['n'], sc['A']
        err = np.zeros((n, 3))
        err[:, :A] = o['obs'][:, :A]      # the error of step k is the head of its observation
        words += [sc['config'], int(sc['incremental']), n] + G.fault_row(sc['fault'])
        words += list(np.concatenate([err, o['states'], o['actions']], axis=1).ravel())
    rng = np.random.default_rng(11)
    sens = [(rng.normal(0, 1, 12), rng.normal(0, 1e-3, 7)) for _ in range(4)]
    words.append(float(len(sens)))
    for x, sn in sens:
        words += list(x) + list(sn)
    fin, fout = str(tmp / 'in.f64'), str(tmp / 'out.f64')
    np.asarray(words, dtype=np.float64).tofile(fin)
    subprocess.run([exe, fin, fout], check=True)
    w = np.fromfile(fout, dtype=np.float64)
    res, p = {}, 0
    for sc, o in cases:
        n = o['n']
        res[sc['name']] = dict(none=w[p:p + 8], cmd0=w[p + 8:p + 11], steps=w[p + 11:p + 11 + n * ROW].reshape(n, ROW))
        p += 11 + n * ROW
    sx = w[p:].reshape(len(sens), 12)
    return cases, res, sens, sx


def test_the_cases_cover_every_configuration_and_fault():
    S = G.scenarios()
    assert {(s['config'], bool(s['incremental'])) for s in S} == {(c, i) for c in (G.ATTITUDE, G.SYMMETRIC, G.FULL) for i in (False, True)}
    assert {s['kind'] for s in S} == {'noise', 'f32', 'f64'}
    assert {s['fault'] for s in S} >= {None, 'be', 'jr', 'sa', 'se', 'gain_clip'}


def test_the_header_gives_every_flown_command_and_observation_bit_for_bit(replay):
    cases, res, _, _ = replay
    for sc, o in cases:
        r, S, name = res[sc['name']], sc['S'], sc['name']
        st = r['steps']
        assert (_bits(r['none']) == _bits(G.fault_row(None))).all(), name
        assert (_bits(r['cmd0']) == _bits(_plant(sc['fault'], [0.0, 0.0, 0.0])[:3])).all(), name
        want_cmd = np.array([_plant(sc['fault'], list(u))[:3] for u in o['actions']]) if name.startswith('extra_fault_') else o['cmd']
        assert (_bits(st[:, 0:3]) == _bits(want_cmd)).all(), name
        assert (_bits(st[:, 3:3 + S]) == _bits(o['obs'])).all(), name
        assert (st[:, 3 + S:] == 0.0).all(), name      # nothing beyond the S entries of the configuration


def test_the_sensor_add_reaches_the_seven_columns(replay):
    _, _, sens, sx = replay
    for (x, sn), got in zip(sens, sx):
        want = x.copy()
        for c, i in enumerate(G.NOISE_COLS):
            want[i] = want[i] + sn[c]
        assert (_bits(got) == _bits(want)).all()

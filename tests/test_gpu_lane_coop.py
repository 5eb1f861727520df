"""The wave-cooperative actor of the lane kernels (rollout_variant.inc: one serl_actor_forward_wave per live lane) under every lane mask, occupancy
and shape of tests/lane_coop.py, at ZERO tolerance against the CPU oracle alone: `lane` (lanes_per_wave > 0), `lanern` (the same with the in-kernel
noise generator, replayed on the oracle through serl_amd.venv_noise's rows) and `laneq` (the work queue, on an engine of one wavefront).

Every launch is guarded (lane_coop.fly): NaN around the weight rows and between them, around the reference, err0 and noise rows, poisoned row
indices and keys beside the episodes' own, sentinels in every output -- a value read beside its row is a NaN in the comparison, a value written
beside an episode's own entries a lost sentinel.  Every launch asserts through last_rollout_info() / last_rollout_weights() that the lane family ran
without a regrouped copy at a hidden width other than 32, i.e. the wave-cooperative branch.  tests/test_lane_coop_host.py holds the table, the
conditions and the comparison to what they claim."""
import numpy as np
import pytest
import torch

import actor_shapes as X
import lane_coop as C
from test_gpu_lane_queue import _engine
from test_gpu_rollout import ran

pytestmark = pytest.mark.gpu


def _run(engine, case):
    return C.run_case(engine, case, _engine(C.QUEUE_WAVES))


@pytest.mark.parametrize('case', C.select('mask'), ids=lambda c: c['id'])
def test_masks(engine, case):
    """hidden 72 x 3, 5 episodes in the first five lanes of one wavefront of 64: every pattern of sensor_row and of noise_row, both generators"""
    got, want = _run(engine, case)
    assert (got['length_steps'] == 51).all()


@pytest.mark.parametrize('case', C.select('occ'), ids=lambda c: c['id'])
def test_occupancy(engine, case):
    """lanes per wavefront x episodes: one live lane, a partly filled wavefront, a full one, a second wavefront with one live lane (on the queue: one
    refill of one lane while 63 have retired)"""
    got, want = _run(engine, case)
    assert got['fitness'].shape == (case['E'],)


@pytest.mark.parametrize('case', C.select('ends'), ids=lambda c: c['id'])
def test_lanes_end_at_different_steps(engine, case):
    """the crashing member in lane 0 (it ends first, the higher lanes fly on) and in the last live lane"""
    got, want = _run(engine, case)
    ls, T = got['length_steps'], 201
    e = 0 if case['crash'] == 'first' else case['E'] - 1
    assert 20 < ls[e] < T - 20 and (np.delete(ls, e) == T).all(), ls


@pytest.mark.parametrize('case', C.select('shape'), ids=lambda c: c['id'])
def test_shapes(engine, case):
    """one and two weight rows per lane, full and partial 32-column chunks, exactly 64; 0, 1 and 3 hidden layers; every activation"""
    _run(engine, case)


def test_independent_of_the_predecessor(engine):
    """the masked hidden-72 flight under the generator after a hidden-32 lane launch (the per-lane actor: other registers, the regrouped copy), after
    a `wave` launch of another shape (its LDS rows) and after itself: three equal results, each the oracle's"""
    case = C.BY_ID['mask-lanern-H72_L3_tanh-E5-l64-snxnnx']
    inp = C.noise_rows(engine, case, C.inputs(case))
    want = C.oracle(case, inp)
    s32, s96 = X._shape(32, 3), X._shape(96, 3, 'relu')
    refs = C.references(70, 0.5, 5)
    flights = []
    for before in ('lane32', 'wave96', 'itself'):
        if before == 'lane32':
            engine.rollout(torch.from_numpy(X.make_weights(s32, 5, 1)), X.spec_of(s32), np.arange(70, dtype=np.int32) % 5, refs, t_max=0.5, lanes_per_wave=64, sync=False)
            ran(engine, 'lane', episodes_per_team=64)
            assert engine.last_rollout_weights()['regrouped'] == 1
        elif before == 'wave96':
            engine.rollout(torch.from_numpy(X.make_weights(s96, 5, 2)), X.spec_of(s96), np.arange(70, dtype=np.int32) % 5, refs, t_max=0.5, kernel='wave', sync=False)
            ran(engine, 'wave')
        got = C.fly(engine, case, inp)
        C.same_as_oracle(got, want, 'after ' + before)
        flights.append(got)
    for got in flights[1:]:
        for k in C.KEYS:
            np.testing.assert_array_equal(got[k], flights[0][k], err_msg=k)

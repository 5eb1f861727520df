"""tests/noise_replay.py on hand-written recordings: every expected ordinal, row, step, clock and carried-error row below is written out
by hand from the env's rules (an episode start takes the env's next ordinal; the model clock counts one tick per reset and one per step;
the first observation carries the error of the env's last step).  No GPU."""
import numpy as np
import pytest

from noise_replay import Episode, episodes, ordinals, starts

F, T = False, True


def _col(*flags):
    return np.array(flags, bool)[:, None]


def test_an_env_that_never_starts():
    # env 0: reset in front of row 0, three-step episodes; env 1: never reset, frozen (done in every row)
    done = np.array([[F, T], [F, T], [T, T], [F, T]])
    eps = episodes(done, [(0, np.array([T, F]))])
    assert eps == [Episode(0, 0, 0, 3, 0, True, 0, -1, ('reset', 0)),
                   Episode(0, 1, 3, 1, 0, False, 4, 2, ('row', 2))]
    o, k = ordinals(done, eps)
    np.testing.assert_array_equal(o, [[0, -1], [0, -1], [0, -1], [1, -1]])
    np.testing.assert_array_equal(k, [[0, -1], [1, -1], [2, -1], [0, -1]])
    np.testing.assert_array_equal(starts(eps, 2), [2, 0])
    # no reset at all: nothing
    assert episodes(np.ones((3, 2), bool)) == []
    # a never-reset env that is not done is no recording of these envs
    with pytest.raises(ValueError, match='never reset'):
        episodes(done, [(0, np.array([F, T]))])


def test_an_explicit_reset_in_the_middle_of_an_episode():
    # three-step episodes; the reset in front of row 5 abandons ordinal 1 after two steps (rows 3, 4): 1 + 2 ticks, a new ordinal
    done = _col(F, F, T, F, F, F, F)
    eps = episodes(done, [(0, None), (5, None)])
    assert eps == [Episode(0, 0, 0, 3, 0, True, 0, -1, ('reset', 0)),
                   Episode(0, 1, 3, 2, 0, False, 4, 2, ('row', 2)),
                   Episode(0, 2, 5, 2, 0, False, 7, 4, ('reset', 1))]
    o, k = ordinals(done, eps)
    np.testing.assert_array_equal(o[:, 0], [0, 0, 0, 1, 1, 2, 2])
    np.testing.assert_array_equal(k[:, 0], [0, 1, 2, 0, 1, 0, 1])
    np.testing.assert_array_equal(starts(eps, 1), [3])


def test_a_restart_on_the_last_recorded_step():
    # the restart inside row 2 starts ordinal 1, of which no step is recorded: its first observation is the one after row 2
    eps = episodes(_col(F, F, T), [(0, None)])
    assert eps == [Episode(0, 0, 0, 3, 0, True, 0, -1, ('reset', 0)),
                   Episode(0, 1, 3, 0, 0, False, 4, 2, ('row', 2))]
    np.testing.assert_array_equal(starts(eps, 1), [2])
    # ... and a reset behind the last row abandons it at once
    eps = episodes(_col(F, F, T), [(0, None), (3, None)])
    assert eps[1:] == [Episode(0, 1, 3, 0, 0, False, 4, 2, ('row', 2)),
                       Episode(0, 2, 3, 0, 0, False, 5, 2, ('reset', 1))]


def test_a_trailing_partial_episode_and_a_running_one_at_row_0():
    # the env is two steps into ordinal 0 at row 0 (one reset and two steps: clock 3); six-step episodes
    eps = episodes(_col(F, F, F, T, F), count0=[1], live0=[T], clock0=[3], step0=[2])
    assert eps == [Episode(0, 0, 0, 4, 2, True, 0, -1, None),
                   Episode(0, 1, 4, 1, 0, False, 7, 3, ('row', 3))]
    o, k = ordinals(np.zeros((5, 1), bool), eps)
    np.testing.assert_array_equal(k[:, 0], [2, 3, 4, 5, 0])
    np.testing.assert_array_equal(starts(eps, 1, [1]), [2])
    with pytest.raises(ValueError, match='counts no start'):
        episodes(_col(F, T), live0=[T])


SIX = np.zeros((20, 4), bool)
SIX[[5, 11, 17]] = True                                   # six-step episodes of four envs that started together
THIRD = np.array([T, F, F, T])


def test_two_segments_joined():
    """reset(), 12 steps, reset(every third env), 8 steps: the restart inside row 11 starts ordinal 2, which envs 0 and 3 abandon without a
    step (one tick); they fly ordinal 3 in rows 12 .. 17 and two steps of ordinal 4, the others ordinal 2 and two steps of ordinal 3"""
    eps = episodes(SIX, [(0, None), (12, THIRD)])
    third = [Episode(0, 0, 0, 6, 0, True, 0, -1, ('reset', 0)),
             Episode(0, 1, 6, 6, 0, True, 7, 5, ('row', 5)),
             Episode(0, 2, 12, 0, 0, False, 14, 11, ('row', 11)),
             Episode(0, 3, 12, 6, 0, True, 15, 11, ('reset', 1)),
             Episode(0, 4, 18, 2, 0, False, 22, 17, ('row', 17))]
    other = [Episode(1, 0, 0, 6, 0, True, 0, -1, ('reset', 0)),
             Episode(1, 1, 6, 6, 0, True, 7, 5, ('row', 5)),
             Episode(1, 2, 12, 6, 0, True, 14, 11, ('row', 11)),
             Episode(1, 3, 18, 2, 0, False, 21, 17, ('row', 17))]
    assert eps == third + other + [ep._replace(env=2) for ep in other] + [ep._replace(env=3) for ep in third]
    np.testing.assert_array_equal(starts(eps, 4), [5, 4, 4, 5])
    o, k = ordinals(SIX, eps)
    assert (o >= 0).all()
    np.testing.assert_array_equal(o[:, 0], [0] * 6 + [1] * 6 + [3] * 6 + [4] * 2)
    np.testing.assert_array_equal(o[:, 1], [0] * 6 + [1] * 6 + [2] * 6 + [3] * 2)
    np.testing.assert_array_equal(k[:, 0], list(range(6)) * 3 + [0, 1])
    # the second segment on its own, picking up what the first left: three starts, clock 15 (two episodes of 1 + 6 ticks and the restart's)
    first = episodes(SIX[:12], [(0, None)])
    np.testing.assert_array_equal(starts(first, 4), [3, 3, 3, 3])
    second = episodes(SIX[12:], [(0, THIRD)], count0=[3] * 4, live0=[T] * 4, clock0=[15] * 4)
    assert [ep for ep in second if ep.env == 0] == [Episode(0, 2, 0, 0, 0, False, 14, -1, None),
                                                    Episode(0, 3, 0, 6, 0, True, 15, -1, ('reset', 0)),
                                                    Episode(0, 4, 6, 2, 0, False, 22, 5, ('row', 5))]
    assert [ep for ep in second if ep.env == 1] == [Episode(1, 2, 0, 6, 0, True, 14, -1, None),
                                                    Episode(1, 3, 6, 2, 0, False, 21, 5, ('row', 5))]
    np.testing.assert_array_equal(starts(second, 4, [3] * 4), [5, 4, 4, 5])
    # every (env, ordinal) of the joined recording is in one of the two, with the same clock
    joined = {(ep.env, ep.ordinal): ep.tick0 for ep in eps}
    parts = {(ep.env, ep.ordinal): ep.tick0 for ep in first + second}
    assert joined == parts


def test_bad_resets():
    with pytest.raises(ValueError, match='outside'):
        episodes(_col(F, T), [(3, None)])
    with pytest.raises(ValueError, match='mask'):
        episodes(_col(F, T), [(0, np.array([T, F]))])


def test_ordinals_generalise_the_running_envs_form():
    """for envs that all fly ordinal `first` from step 0 at row 0, (ordinal, step) are what a plain count of the done flags gives"""
    rng = np.random.default_rng(3)
    done = rng.random((40, 9)) < 0.2
    first = rng.integers(0, 5, 9)
    want_o, want_k = np.zeros((40, 9), np.int64), np.zeros((40, 9), np.int64)
    o, j = first.astype(np.int64).copy(), np.zeros(9, np.int64)
    for k in range(40):
        want_o[k], want_k[k] = o, j
        j = np.where(done[k], 0, j + 1)
        o = o + done[k]
    got_o, got_k = ordinals(done, episodes(done, count0=first + 1, live0=np.ones(9, bool), clock0=np.ones(9)))
    np.testing.assert_array_equal(got_o, want_o)
    np.testing.assert_array_equal(got_k, want_k)

"""Shared by tests/test_noise_replay_host.py (CPU) and tests/test_gpu_venv_noise_replay.py / tests/test_gpu_venv_noise.py (GPU): the episode
bookkeeping of a recording of auto-reset envs -- which rows of a rollout belong to which episode of which env, and what that episode
started from -- so that every episode of a device-noise run can be flown again on the CPU oracle from (noise_seed, env, ordinal).
A plain module (not a conftest): nothing here is a fixture.

The rules are the env's (include/serl_amd.h, serl_venv_desc / serl_venv_noise_desc):
  ordinal   every episode start of an env, an explicit reset and an in-kernel restart alike, takes the next ordinal of that env
  clock     the model clock counts one tick per reset and one per step and is never set back: an episode that flew n steps cost 1 + n ticks
  error     reset never clears the tracking error: the first observation of an episode carries the error of the env's last step before it
  frozen    an env that was never reset is not running: every row of it is done and belongs to no episode"""
import collections
import numpy as np

# env, ordinal   the env's index and the episode's ordinal (the `episode` of serl_amd.venv_noise)
# row0, n        the n rows row0 .. row0 + n - 1 of the recording are the episode's steps k0 .. k0 + n - 1 (n = 0: started, no step recorded)
# k0             in-episode step of row row0: 0, but for an episode that was already running at row 0
# finished       True: the last of those rows is the episode's last step (done); False: a prefix -- abandoned by an explicit reset, or
#                cut by the end of the recording
# tick0          the model clock the episode's reset started from
# err_row        the row whose tracking error the episode's first observation carries (the env's last step before the start), -1: none
#                in this recording (a fresh env: zero)
# obs0           where the first observation is: ('reset', j) -- what the j-th explicit reset of `resets` returned; ('row', r) -- the
#                observation after row r (the restart inside that step); None for an episode that was already running at row 0
Episode = collections.namedtuple('Episode', 'env ordinal row0 n k0 finished tick0 err_row obs0')


def episodes(done, resets=(), count0=None, live0=None, clock0=None, step0=None):
    """Every episode or episode prefix of a recording, sorted by (env, ordinal).

    done     bool [K, N]: the done flags of K consecutive steps of N auto-reset envs (several rollouts: concatenated)
    resets   the explicit resets the caller made, [(step, mask), ...] in call order: `mask` (bool [N]; None = all) was reset in front of
             row `step` (0 .. K; K = behind the last row)
    count0   i32 [N]: episode starts of every env in front of row 0 and of every reset (noise_episode; default 0)
    live0    bool [N]: envs that are flying an episode (ordinal count0 - 1) at row 0 without a reset of `resets` (default: none)
    clock0   i32 [N]: model clock of every env in front of row 0 (default 0)
    step0    i32 [N]: in-episode step of row 0 for the envs of live0 (default 0)"""
    done = np.asarray(done, bool)
    K, N = done.shape
    count = np.zeros(N, np.int64) if count0 is None else np.array(count0, np.int64).copy()
    clock = np.zeros(N, np.int64) if clock0 is None else np.array(clock0, np.int64).copy()
    live = np.zeros(N, bool) if live0 is None else np.array(live0, bool).copy()
    k_in = np.zeros(N, np.int64) if step0 is None else np.array(step0, np.int64).copy()
    last_row = np.full(N, -1, np.int64)
    run = [None] * N                                      # the running episode of every env: [ordinal, row0, k0, tick0, err_row, obs0]
    for e in np.nonzero(live)[0]:
        if count[e] < 1:
            raise ValueError('env %d flies an episode at row 0 but counts no start' % e)
        run[e] = [int(count[e]) - 1, 0, int(k_in[e]), int(clock[e]) - 1 - int(k_in[e]), -1, None]
    by_step = collections.defaultdict(list)
    for j, (step, mask) in enumerate(resets):
        if not 0 <= int(step) <= K:
            raise ValueError('reset %d at step %r: outside 0 .. %d' % (j, step, K))
        m = np.ones(N, bool) if mask is None else np.asarray(mask, bool)
        if m.shape != (N,):
            raise ValueError('reset %d: mask bool [%d]' % (j, N))
        by_step[int(step)].append((j, m))
    out = []

    def close(e, row, finished):
        o, r0, k0, t0, er, ob = run[e]
        out.append(Episode(int(e), o, r0, row - r0, k0, finished, t0, er, ob))

    def start(e, row, obs0):
        run[e] = [int(count[e]), row, 0, int(clock[e]), int(last_row[e]), obs0]
        count[e] += 1
        clock[e] += 1                                     # the reset's own step with the zero command
        live[e] = True

    for k in range(K + 1):
        for j, m in by_step.get(k, ()):
            for e in np.nonzero(m)[0]:
                if live[e]:
                    close(e, k, False)                    # abandoned
                start(e, k, ('reset', j))
        if k == K:
            break
        for e in range(N):
            if not live[e]:
                if not done[k, e]:
                    raise ValueError('env %d was never reset but is not done at row %d' % (e, k))
                continue
            clock[e] += 1
            last_row[e] = k
            if done[k, e]:
                close(e, k + 1, True)
                start(e, k + 1, ('row', k))               # the restart inside step k
    for e in np.nonzero(live)[0]:
        close(e, K, False)                                # cut by the end of the recording
    return sorted(out, key=lambda ep: (ep.env, ep.ordinal))


def ordinals(done, eps):
    """(episode ordinal, in-episode step) i64 [K, N] of every row from its episode, -1 where a row belongs to none"""
    K, N = np.asarray(done).shape
    ordinal, kin = np.full((K, N), -1, np.int64), np.full((K, N), -1, np.int64)
    for ep in eps:
        ordinal[ep.row0:ep.row0 + ep.n, ep.env] = ep.ordinal
        kin[ep.row0:ep.row0 + ep.n, ep.env] = ep.k0 + np.arange(ep.n)
    return ordinal, kin


def starts(eps, N, count0=None):
    """i64 [N]: episode starts of every env behind the recording (what noise_episode must hold): count0 + the episodes that started in it"""
    c = np.zeros(N, np.int64) if count0 is None else np.array(count0, np.int64).copy()
    for ep in eps:
        if ep.obs0 is not None:
            c[ep.env] += 1
    return c

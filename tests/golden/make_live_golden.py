#!/usr/bin/env python3
"""Record what the REFERENCE ITSELF returns for the two step-by-step comparisons of the suite (run in the build container only).

  python tests/golden/make_live_golden.py          (cwd anywhere; a few seconds)

  ref_live.npz        the reference's prebuilt dynamics library of every one of the 14 build directories, driven by the seeded
                      400-step command sequence of live_commands(): a SHA-256 of that sequence, a 64-bit digest (digest64) of the
                      12 outputs and of the 19 continuous states rtX after every step and of all block signals rtB every 50th
                      step, and the outputs of the first step after re-initialisation
                      (tests/test_oracle_dynamics.py::test_live_reference_library_step_by_step imports live_commands / digest64)
  replay_memory.npz   the reference's ReplayMemory (base/core/replay_memory.py) under a seeded sequence of add / add_content_of /
                      add_latest_from / shuffle / reset / sample / sample_from_latest on three capacity pairs: length, position and
                      a SHA-256 of the stored rows after every operation, and every sampled batch
                      (tests/test_ga_host.py::test_device_replay_ring_matches_reference_replay_memory)
"""
import hashlib, os, random, sys, zlib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

BUILDS14 = ['h2000_v90', 'h2000_v150', 'h10000_v90', 'cg', 'cg_for', 'cg_timed', 'ice', 'gust', 'test', 'be', 'jr', 'sa', 'se', 'noise']
LIVE_STEPS = 400
REPLAY_CAPS = ((16, 16), (16, 40), (40, 16))
REPLAY_STEPS = 120


def live_commands(build):
    """the seeded command sequence of one build: elevator / aileron / rudder in +-6 deg (zero every 37th step), throttles after step 200"""
    rng = np.random.default_rng(zlib.crc32(build.encode()) % 1000)
    cmd = np.zeros((LIVE_STEPS, 10))
    for k in range(LIVE_STEPS):
        cmd[k, :3] = np.deg2rad(rng.uniform(-6, 6, 3)) * (k % 37 != 0)
        if k > 200:
            cmd[k, 8:10] = rng.uniform(0, 0.2)
    return cmd


def digest64(a):
    """the first 8 bytes of the SHA-256 of an array's f64 bytes: bit-exact equality, step by step, in 8 bytes per step"""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest()[:8], np.uint64)[0]


def make_live():
    from oracle.refso import RefCitation
    out = {}
    for b in BUILDS14:
        ref = RefCitation(b)
        cmd = live_commands(b)
        y, X, B = [], [], []
        for k in range(LIVE_STEPS):
            y.append(digest64(ref.step(cmd[k])))
            X.append(digest64(ref.X))
            if k % 50 == 0:
                B.append(digest64(ref.B))
        ref.initialize()
        out.update({b + '_cmd_sha256': np.frombuffer(hashlib.sha256(cmd.tobytes()).digest(), np.uint8), b + '_y': np.array(y), b + '_X': np.array(X),
                    b + '_B': np.array(B), b + '_nB': np.array(len(ref.B)), b + '_y_reinit': ref.step(np.zeros(10))})
    return out


def replay_rows(mem):
    """the stored transitions in list order, one f32 row of 19 (state 7, action 3, next state 7, reward, done) each"""
    if not len(mem):
        return np.zeros((0, 19), np.float32)
    return np.stack([np.concatenate([np.ravel(x) for x in t]) for t in mem.memory]).astype(np.float32)


def digest(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, dtype=np.float32).tobytes()).hexdigest()


def make_replay():
    import refshim
    refshim.install()
    from core.replay_memory import ReplayMemory
    rs = np.random.RandomState(3)

    def tup():
        return rs.randn(7), rs.randn(3), rs.randn(7), float(rs.randn()), float(rs.rand() < 0.1)
    out = {}
    for c, (cap, other_cap) in enumerate(REPLAY_CAPS):
        ref, ref2 = ReplayMemory(cap, 'cpu'), ReplayMemory(other_cap, 'cpu')
        state, digests, sample_n, samples = [], [], [], []
        for step in range(REPLAY_STEPS):
            op = rs.randint(0, 9)
            got = None
            if op <= 3:
                for _ in range(rs.randint(1, 9)):
                    ref.add(*tup())
                    ref2.add(*tup())
            elif op == 4 and len(ref2):
                ref.reset(); ref.add_content_of(ref2)
            elif op == 5 and len(ref2):
                ref.add_latest_from(ref2, int(rs.randint(1, other_cap + 4)))
            elif op == 6:
                random.seed(step); ref.shuffle()
            elif op == 7 and len(ref) >= 3:
                k = int(rs.randint(1, len(ref) + 1))
                random.seed(step); got = ref.sample(k)
            elif op == 8 and len(ref) >= 3:
                latest = int(rs.randint(1, cap + 6)); k = int(rs.randint(1, min(latest, len(ref)) + 1))
                random.seed(step); got = ref.sample_from_latest(k, latest)
            if got is not None:
                assert [tuple(x.shape) for x in got] == [(k, 7), (k, 3), (k, 7), (k, 1), (k, 1)]
                samples.append(np.concatenate([x.numpy() for x in got], 1))
            sample_n.append(0 if got is None else len(samples[-1]))
            state.append([len(ref), ref.position, len(ref2), ref2.position])
            digests.append([digest(replay_rows(ref)), digest(replay_rows(ref2))])
        out.update({'c%d_caps' % c: np.array([cap, other_cap]), 'c%d_state' % c: np.array(state), 'c%d_digest' % c: np.array(digests),
                    'c%d_sample_n' % c: np.array(sample_n), 'c%d_sample' % c: np.concatenate(samples).astype(np.float32)})
    return out


if __name__ == '__main__':
    np.savez_compressed(os.path.join(HERE, 'ref_live.npz'), **make_live())
    np.savez_compressed(os.path.join(HERE, 'replay_memory.npz'), **make_replay())

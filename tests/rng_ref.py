"""NumPy restatement of the env's counter-based noise generator (serl_amd/csrc/serl_rng.h), written from the published description of
Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the constants of the interface
(include/serl_amd.h, serl_venv_noise_desc) -- not from the kernel's text.  Shared by tests/test_rng_host.py and tests/test_gpu_venv_noise.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl increments of the key
MASK = np.uint64(0xFFFFFFFF)
SENSOR, ACTION = 0, 1                    # stream of counter word 3 = stream << 16 | block


def philox4x32_10(key, ctr):
    """key u32 [..., 2], ctr u32 [..., 4] -> u32 [..., 4]"""
    k = [np.asarray(key[..., i], np.uint64) for i in range(2)]
    c = [np.asarray(ctr[..., i], np.uint64) for i in range(4)]
    for r in range(10):
        p0 = np.uint64(M0) * c[0]         # 32 x 32 -> 64 bits: exact in u64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def words(seed, env, episode, entry, stream, block):
    """the four words of one call: key = (seed low, seed high), counter = (env, episode, entry, stream << 16 | block)"""
    env, episode, entry, block = np.broadcast_arrays(*[np.asarray(v, np.int64) for v in (env, episode, entry, block)])
    ctr = np.stack([env, episode, entry, (stream << 16) | block], -1).astype(np.uint32)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32), ctr.shape[:-1] + (2,))
    return philox4x32_10(key, ctr)


def uniform(w0, w1, dtype=np.float64):
    """(2 k + 1) 2^-53 with k = w0 << 20 | w1 >> 12: exact in f64, inside (0, 1)"""
    k = (np.asarray(w0, np.uint64) << np.uint64(20)) | (np.asarray(w1, np.uint64) >> np.uint64(12))
    return (2 * k + 1).astype(dtype) * dtype(2.0) ** -53


def normals(seed, env, episode, entry, stream, blocks, dtype=np.longdouble):
    """-> (z [..., 2 blocks], radius [..., 2 blocks]) in `dtype`: per block one Box-Muller pair r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 log u0)"""
    z, rad = [], []
    for b in range(blocks):
        w = words(seed, env, episode, entry, stream, b)
        u0, u1 = uniform(w[..., 0], w[..., 1], dtype), uniform(w[..., 2], w[..., 3], dtype)
        r = np.sqrt(-2 * np.log(u0))
        a = 2 * dtype(np.pi) * u1 if dtype is not np.longdouble else 2 * np.longdouble('3.14159265358979323846264338327950288') * u1
        z += [r * np.cos(a), r * np.sin(a)]
        rad += [r, r]
    return np.stack(z, -1), np.stack(rad, -1)

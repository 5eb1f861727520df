// serl_rng.h -- the counter-based generator of the vector env's sensor and exploration noise (include/serl_amd.h serl_venv_noise_desc):
// no table, no host draw, no state -- a draw is a function of (seed, env, episode ordinal, entry within the episode, stream, block), so
// any episode's noise can be replayed on demand and every episode of every env gets a realisation of its own.
//
//   bits     Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
//            key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.  key = the 64-bit seed (low word, high word); counter = (env, episode,
//            entry, stream << 16 | block), stream 0 = sensor, 1 = action.
//   uniform  two words -> k = w0 << 20 | w1 >> 12 (52 bits), u = (2 k + 1) 2^-53: exact in f64, strictly inside (0, 1).
//   normal   one Philox call = two uniforms = one Box-Muller pair: r = sqrt(-2 log u0), (s, c) = sincospi(2 u1), normals r c, r s
//            (the device library's log / sqrt / sincospi; the build contracts nothing).
//   sensor   blocks 0 .. 3 = 8 normals, the first 7 in channel order p q r | alpha | beta | phi theta; addend bias[i] + scale[i] z
//   action   blocks 0 .. 1 = 4 normals, the first A are used; addend clip(sd z, -clip, clip)
//
//
// The fused TD3 learner (include/serl_amd.h serl_td3_rng_desc) draws its minibatches and its noise from the same bits: counter = (learner
// key, absolute iteration, index, stream << 16 | block), streams 2 .. 4.
//   target   stream 3, index = sample b, blocks 0 .. 1 = 4 normals (the Box-Muller pairs above), the first A cast to f32
//   caps     stream 4, index = sample b, blocks 0 .. 3 = 16 words; uniform j = (float)(word j >> 8) * 2^-24: exact, in [0, 1), the grid of
//            torch.rand.  The first S are used; drawn at actor updates only
//   slots    stream 2, block 0, index = step i: B distinct rows of [0, n_rows), uniform over the subsets, by Floyd's algorithm.  Step
//            i = 0 .. B - 1 has j = n_rows - B + i and the candidate t = floor(w64 (j + 1) / 2^64) in [0, j], w64 = w0 << 32 | w1 of the
//            step's Philox call (serl_td3_slot_candidate); column i of the minibatch is t unless an earlier column holds t, else j (no
//            earlier column can hold j: they are all below it).  Integer only, B Philox calls, no loop without a bound.
//
// The bit-level parts are __host__ __device__ plain C++ (serl_host_philox / serl_host_uniform are compiled from this text); the
// normals exist on the device only.  Integer VALU work plus one log and one sincospi per pair: no memory access, no cross-lane traffic.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#define SERL_RNG_FN static __host__ __device__ __forceinline__
#else
#define SERL_RNG_FN static inline
#endif

enum { SERL_RNG_SENSOR = 0, SERL_RNG_ACTION = 1, SERL_RNG_TD3_SLOT = 2, SERL_RNG_TD3_TARGET = 3, SERL_RNG_TD3_CAPS = 4 };      // the stream of counter word 3
enum { SERL_RNG_SENSOR_BLOCKS = 4, SERL_RNG_ACTION_BLOCKS = 2, SERL_RNG_TD3_TARGET_BLOCKS = 2, SERL_RNG_TD3_CAPS_BLOCKS = 4 };

SERL_RNG_FN void serl_philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4])
{
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;      // (the bump after the tenth round is not used)
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of (seed; env, episode, entry, stream, block)
SERL_RNG_FN void serl_rng_words(uint64_t seed, int32_t env, int32_t episode, int32_t entry, int stream, int block, uint32_t out[4])
{
  serl_philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)env, (uint32_t)episode, (uint32_t)entry,
                     ((uint32_t)stream << 16) | (uint32_t)block, out);
}

SERL_RNG_FN double serl_rng_uniform(uint32_t w0, uint32_t w1)
{
  const uint64_t k = ((uint64_t)w0 << 20) | (uint64_t)(w1 >> 12);
  return (double)(2 * k + 1) * 0x1.0p-53;      // 2 k + 1 < 2^53: both the conversion and the product are exact
}

// floor(a b / 2^64) for b < 2^32, in 64-bit pieces (the same text on both sides: no __int128, no __umul64hi)
SERL_RNG_FN uint64_t serl_rng_mulhi_u32(uint64_t a, uint32_t b)
{
  const uint64_t lo = (a & 0xFFFFFFFFu) * b, hi = (a >> 32) * b;      // hi + (lo >> 32) <= (2^32 - 1)^2 + 2^32 - 2 < 2^64
  return (hi + (lo >> 32)) >> 32;
}

// the candidate row of Floyd step `step` of a TD3 minibatch (see the head of this file): uniform in [0, j], j = n_rows - batch + step
SERL_RNG_FN int32_t serl_td3_slot_candidate(uint64_t seed, int32_t learner, int32_t iteration, int32_t step, int32_t j)
{
  uint32_t w[4];
  serl_rng_words(seed, learner, iteration, step, SERL_RNG_TD3_SLOT, 0, w);
  return (int32_t)serl_rng_mulhi_u32(((uint64_t)w[0] << 32) | w[1], (uint32_t)j + 1u);
}

// the whole minibatch by one thread: out[i] = column i.  1 <= batch <= n_rows; batch^2 / 2 comparisons (the kernels hold the chosen rows
// across a wavefront instead and test membership by ballot: serl_td3.hip)
SERL_RNG_FN void serl_td3_slots_serial(uint64_t seed, int32_t learner, int32_t iteration, int32_t n_rows, int32_t batch, int32_t *out)
{
  for (int32_t i = 0; i < batch; ++i) {
    const int32_t j = n_rows - batch + i;
    const int32_t t = serl_td3_slot_candidate(seed, learner, iteration, i, j);
    bool taken = false;
    for (int32_t q = 0; q < i; ++q) taken |= out[q] == t;
    out[i] = taken ? j : t;
  }
}

// uniform j of a CAPS block from its word
SERL_RNG_FN float serl_td3_caps_uniform(uint32_t w) { return (float)(w >> 8) * 0x1.0p-24f; }

#if defined(__HIPCC__)
// one Box-Muller pair from the four words of one Philox call
static __device__ __forceinline__ void serl_rng_normal_pair(const uint32_t w[4], double &z0, double &z1)
{
  const double u0 = serl_rng_uniform(w[0], w[1]), u1 = serl_rng_uniform(w[2], w[3]);
  const double r = sqrt(-2.0 * log(u0));
  double s, c;
  sincospi(2.0 * u1, &s, &c);
  z0 = r * c; z1 = r * s;
}

// the standard normals of one entry: 2 * blocks values (sensor: 8, the first 7 used; action: 4, the first A used)
template <int BLOCKS>
static __device__ __forceinline__ void serl_rng_normals(uint64_t seed, int32_t env, int32_t episode, int32_t entry, int stream, double (&z)[2 * BLOCKS])
{
#pragma unroll
  for (int b = 0; b < BLOCKS; ++b) {
    uint32_t w[4];
    serl_rng_words(seed, env, episode, entry, stream, b, w);
    serl_rng_normal_pair(w, z[2 * b], z[2 * b + 1]);
  }
}

// the sensor addends of one entry, channel order p q r | alpha | beta | phi theta: bias + scale z (multiply, then add)
static __device__ __forceinline__ void serl_rng_sensor(uint64_t seed, const double (&bias)[7], const double (&scale)[7], int32_t env, int32_t episode,
                                                       int32_t entry, double (&out)[7])
{
  double z[8];
  serl_rng_normals<SERL_RNG_SENSOR_BLOCKS>(seed, env, episode, entry, SERL_RNG_SENSOR, z);
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const double m = scale[i] * z[i];
    out[i] = bias[i] + m;
  }
}

// the exploration-noise addends of one entry: clip(sd z, -clip, clip) (base/core/agent.py:90-93), three columns
static __device__ __forceinline__ void serl_rng_action(uint64_t seed, double sd, double clip, int32_t env, int32_t episode, int32_t entry, double (&out)[3])
{
  double z[4];
  serl_rng_normals<SERL_RNG_ACTION_BLOCKS>(seed, env, episode, entry, SERL_RNG_ACTION, z);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double m = sd * z[i];
    out[i] = m < -clip ? -clip : (m > clip ? clip : m);
  }
}
#endif

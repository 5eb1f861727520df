// rollout_noise.h -- what the noise instantiations of the population rollout kernels (SERL_ROLLOUT_NOISE: family_lanern.hip around
// rollout_variant.inc, family_wavern.hip around rollout_wave.inc; serl_rollout_noise in include/serl_amd.h) put where the plain kernels
// read a row of desc->sensor_noise / desc->action_noise: the draws of serl_rng.h for (nz.seed; env, episode, entry).  Integer VALU work
// plus one log and one sincospi per pair -- no memory access, no cross-lane traffic; the per-episode key is read once at the episode's start.
#pragma once
#include "serl_rng.h"

// the generator's part of one episode's state: whether the episode draws at all, and counter words 0 and 1
struct SerlRolloutNoiseKey {
  bool sensor, action;
  int32_t env, episode;
};

// episode e of the launch: the generator flags under the per-episode masks desc->sensor_row / desc->noise_row (< 0: no noise), the key from
// nz.env / nz.episode (NULL: e / 0)
static __device__ __forceinline__ SerlRolloutNoiseKey serl_rollout_noise_key(const serl_rollout_desc &d, const serl_rollout_noise_desc &nz, int e)
{
  SerlRolloutNoiseKey k;
  k.sensor = nz.sensor != 0 && (!d.sensor_row || d.sensor_row[e] >= 0);
  k.action = nz.action != 0 && (!d.noise_row || d.noise_row[e] >= 0);
  k.env = nz.env ? nz.env[e] : (int32_t)e;
  k.episode = nz.episode ? nz.episode[e] : 0;
  return k;
}

// the sensor model on top of what step() returned: entry 0 behind initialize()'s step, entry k + 1 behind env step k
static __device__ __forceinline__ void serl_rollout_noise_sensor(const serl_rollout_noise_desc &nz, const SerlRolloutNoiseKey &key, int32_t entry, double (&x)[12])
{
  double sn[7];
  serl_rng_sensor(nz.seed, nz.sensor_bias, nz.sensor_scale, key.env, key.episode, entry, sn);
  x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
}

// the exploration-noise addends of env step k (three columns; the caller uses the first action_dim)
static __device__ __forceinline__ void serl_rollout_noise_action(const serl_rollout_noise_desc &nz, const SerlRolloutNoiseKey &key, int32_t k, double (&an)[3])
{
  serl_rng_action(nz.seed, nz.action_sd, nz.action_clip, key.env, key.episode, k, an);
}

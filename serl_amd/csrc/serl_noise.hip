// serl_noise.hip -- what the noise instantiations of the env kernels draw (serl_rng.h; family_lanenz.hip), written out: serl_venv_noise_fill
// replays any episode's sensor or exploration noise into a table that the table arguments of the env, the evaluator and the oracle take, and
// serl_host_philox / serl_host_uniform are the generator's bit-level parts compiled for the host from the same text.  No LDS tables, no
// dynamics: a unit of its own beside the lane units.  serl_venv_actor_forward is the in-kernel actor of the rollout kernels alone (rollout_device.h
// serl_actor_forward_lane32 / _lane_general, one lane per env): the step loop of CitationVecEnv.rollout on a device-noise env runs it, so that the
// loop computes the bits the fused kernels compute.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include "rollout_device.h"
#include "serl_ctx.h"
#include "serl_rng.h"

namespace {

constexpr int NF_THREADS = 256;

// one thread = one (row, entry); out [rows][entries][W]
__global__ void __launch_bounds__(NF_THREADS) serl_noise_fill_kernel(serl_venv_noise_desc nz, int mode, int rows, const int32_t *__restrict__ env,
                                                                     const int32_t *__restrict__ episode, const int32_t *__restrict__ entry0,
                                                                     int entries, void *out)
{
  const int64_t i = (int64_t)blockIdx.x * NF_THREADS + threadIdx.x;
  if (i >= (int64_t)rows * entries) return;
  const int row = (int)(i / entries), j = (int)(i % entries);
  const int32_t e = env[row], ep = episode[row], entry = entry0[row] + j;
  if (mode == 0) {
    uint32_t *o = (uint32_t *)out + i * 24;
    for (int b = 0; b < SERL_RNG_SENSOR_BLOCKS + SERL_RNG_ACTION_BLOCKS; ++b) {
      uint32_t w[4];
      if (b < SERL_RNG_SENSOR_BLOCKS) serl_rng_words(nz.seed, e, ep, entry, SERL_RNG_SENSOR, b, w);
      else serl_rng_words(nz.seed, e, ep, entry, SERL_RNG_ACTION, b - SERL_RNG_SENSOR_BLOCKS, w);
      for (int q = 0; q < 4; ++q) o[4 * b + q] = w[q];
    }
  } else if (mode == 1) {
    double z[8];
    serl_rng_normals<SERL_RNG_SENSOR_BLOCKS>(nz.seed, e, ep, entry, SERL_RNG_SENSOR, z);
    double *o = (double *)out + i * 7;
    for (int q = 0; q < 7; ++q) o[q] = z[q];
  } else if (mode == 2) {
    double t[7];
    serl_rng_sensor(nz.seed, nz.sensor_bias, nz.sensor_scale, e, ep, entry, t);
    double *o = (double *)out + i * 7;
    for (int q = 0; q < 7; ++q) o[q] = t[q];
  } else {
    double t[3];
    serl_rng_action(nz.seed, nz.action_sd, nz.action_clip, e, ep, entry, t);
    double *o = (double *)out + i * 3;
    for (int q = 0; q < 3; ++q) o[q] = t[q];
  }
}

// one lane = one env: obsf[i] = (float)obs[i], the env's member's forward, act f32 [n][A]
__global__ void __launch_bounds__(NF_THREADS) serl_actor_forward_kernel(serl_rollout_desc d, serl_venv_rollout_desc rd, int n, int lane32,
                                                                        const double *__restrict__ obs, float *__restrict__ out)
{
  const int e = blockIdx.x * NF_THREADS + threadIdx.x;
  if (e >= n) return;
  const int S = d.state_dim, A = d.action_dim;
  const unsigned member = rd.member_of_env ? (unsigned)rd.member_of_env[e] % (unsigned)rd.n_members : 0u;
  const float *w = rd.weights + (size_t)member * rd.weight_stride;
  float act[3] = {0.0f, 0.0f, 0.0f};
  if (lane32) {
    float o[7];
    for (int i = 0; i < 7; ++i) o[i] = (float)obs[(size_t)e * 7 + i];
    serl_actor_forward_lane32(d, w, o, act);
  } else {
    float o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = i < S ? (float)obs[(size_t)e * S + i] : 0.0f;
    serl_actor_forward_lane_general(d, w, o, act);
  }
  for (int i = 0; i < 3; ++i) if (i < A) out[(size_t)e * A + i] = act[i];
}

}  // namespace

int serl_venv_actor_forward(serl_ctx *c, const serl_venv_rollout_desc *rd, int32_t n_envs, const double *obs, float *actions, void *stream_)
{
  const std::string w("serl_venv_actor_forward");
  if (!c || !rd || !obs || !actions) return serl_fail(SERL_E_INVALID, w + ": NULL argument");
  if (!rd->weights) return serl_fail(SERL_E_INVALID, w + ": weights is NULL");
  if (n_envs < 1) return serl_fail(SERL_E_INVALID, w + ": n_envs < 1");
  if (rd->n_members < 1) return serl_fail(SERL_E_INVALID, w + ": n_members < 1");
  if (rd->state_dim < 1 || rd->state_dim > 16 || rd->action_dim < 1 || rd->action_dim > 3)
    return serl_fail(SERL_E_INVALID, w + ": state_dim must be 1 .. 16, action_dim 1 .. 3");
  if (rd->hidden < 4 || rd->hidden > SERL_MAX_HIDDEN || rd->hidden % 4 != 0)
    return serl_fail(SERL_E_UNSUPPORTED, w + ": hidden must be a multiple of 4 in 4 .. 128");
  if (rd->num_layers < 0 || rd->num_layers > 16) return serl_fail(SERL_E_UNSUPPORTED, w + ": num_layers must be 0 .. 16");
  if (rd->activation != SERL_ACT_TANH && rd->activation != SERL_ACT_ELU && rd->activation != SERL_ACT_LEAKY_RELU)
    return serl_fail(SERL_E_INVALID, w + ": unknown activation");
  if (rd->weight_stride < (int64_t)serl_param_count(rd->state_dim, rd->hidden, rd->num_layers, rd->action_dim) || (rd->weight_stride & 3) != 0 ||
      ((uintptr_t)rd->weights & 15) != 0)
    return serl_fail(SERL_E_INVALID, w + ": weight_stride below the parameter count or not a multiple of 4 floats, or weights not 16-byte aligned");
  HIP_TRY(hipSetDevice(c->device));
  serl_rollout_desc d;
  memset(&d, 0, sizeof(d));
  d.state_dim = rd->state_dim; d.action_dim = rd->action_dim; d.hidden = rd->hidden; d.num_layers = rd->num_layers; d.activation = rd->activation;
  const int lane32 = rd->hidden == 32 && rd->state_dim == 7 && rd->action_dim == 3;      // (the shape serl_venv_rollout takes: its forward)
  hipLaunchKernelGGL(serl_actor_forward_kernel, dim3((unsigned)((n_envs + NF_THREADS - 1) / NF_THREADS)), dim3(NF_THREADS), 0, (hipStream_t)stream_, d, *rd,
                     (int)n_envs, lane32, obs, actions);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

int serl_venv_noise_fill(serl_ctx *c, const serl_venv_noise_desc *nz, int32_t mode, int32_t rows, const int32_t *env, const int32_t *episode,
                         const int32_t *entry0, int32_t entries, void *out, void *stream_)
{
  const std::string w("serl_venv_noise_fill");
  if (!c || !nz || !env || !episode || !entry0 || !out) return serl_fail(SERL_E_INVALID, w + ": NULL argument");
  if (mode < 0 || mode > 3) return serl_fail(SERL_E_INVALID, w + ": mode must be 0 (words), 1 (normals), 2 (sensor addends) or 3 (action addends)");
  if (rows < 1 || entries < 1) return serl_fail(SERL_E_INVALID, w + ": rows / entries < 1");
  if (mode == 3 && (!(nz->action_sd >= 0.0) || !(nz->action_clip >= 0.0))) return serl_fail(SERL_E_INVALID, w + ": action_sd / action_clip < 0");
  HIP_TRY(hipSetDevice(c->device));
  const int64_t n = (int64_t)rows * entries;
  const int64_t grid = (n + NF_THREADS - 1) / NF_THREADS;
  if (grid > 0x7fffffffLL) return serl_fail(SERL_E_INVALID, w + ": rows x entries too large for one launch");
  hipLaunchKernelGGL(serl_noise_fill_kernel, dim3((unsigned)grid), dim3(NF_THREADS), 0, (hipStream_t)stream_, *nz, (int)mode, (int)rows, env, episode,
                     entry0, (int)entries, out);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

void serl_host_philox(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out4[4])
{
  serl_philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), c0, c1, c2, c3, out4);
}

double serl_host_uniform(uint32_t w0, uint32_t w1) { return serl_rng_uniform(w0, w1); }

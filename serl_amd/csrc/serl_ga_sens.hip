// serl_ga_sens.hip -- the output sensitivity of proximal_mutate / safe_mutate (base/core/mod_neuro_evo.py:183-223, :254-298) for
// every actor shape the TD3 learner takes, batch-parallel: serl_ga_sensitivity_general.
//
// serl_ga_sensitivity (serl_ga.hip) walks the minibatch one sample at a time and keeps the Jacobian of one output over the whole genome
// in LDS, which ties it to genomes of at most ~38 000 weights (hidden 128 x 3 is 50 432).  What it computes per output i is a backward
// pass over the whole batch from the seed d out[b][i] = 1, and per 2-D weight the batch-reduction product dZ^T A_prev: the learner's
// weight-gradient phase.  Here that is what runs -- the learner's phases (serl_td3_core.inc: [feature][sample] tiles in LDS, the dense
// phases in their VALU and f32-MFMA flavours, which give the same bits), one workgroup of NT threads per listed member:
//   * ONE forward pass over the minibatch, in chunks of up to BP samples, keeps every layer's outputs (and the LayerNorm's normalised
//     values and standard deviations) on a tape in the caller's workspace;
//   * per output i and chunk: the seed goes back through the output tanh, the Linear layers, the activations and the LayerNorm
//     (unbiased std, eps added to the std; the std's own term masked to 0 where sd == 0, as torch's std_backward does); the weight
//     gradient of every 2-D weight is added into J [G] (the workspace, genome order), chunk after chunk, before anything is squared;
//   * sc += J^2 over i, then sqrt, == 0 -> 1, < 0.01 -> 0.01 (mod_neuro_evo.py:213-217), written in genome order: W0, W1 .. WL, Wo --
//     biases and LayerNorm parameters have no gradient here and no place in `scaling`, exactly serl_ga_sensitivity's layout.
// Phases are separated by __syncthreads only; no workgroup waits on another, a member listed twice is simply computed twice (each
// workgroup owns row m of `scaling` and region m of `work`).  f32 like torch; the summation order is the learner's.
#include <hip/hip_runtime.h>
#include <math.h>
#include "serl_ctx.h"
#include "serl_td3_mfma.h"

namespace {

#include "serl_td3_core.inc"

struct SensArgs {
  const float *weights;         // [pop][stride]
  int64_t stride;
  const int32_t *members;       // [n]
  const float *states;          // [n][B][S]
  float *scaling;               // [n][G]
  float *work;                  // [n][work_floats]
  int64_t work_floats;
  int32_t S, A, H, L, act, B, G;
};

// a member's workspace: J [G rounded up to 4] | per chunk of BP samples: the states [S][BP] | the tape.  Every access is one float wide.
__host__ __device__ inline int sens_genome(int S, int A, int H, int L) { return H * S + L * H * H + A * H; }
__host__ __device__ inline int64_t sens_chunk_floats(int S, int H, int L) { return (int64_t)S * BP + tape_floats(L + 2, H); }
__host__ __device__ inline int64_t sens_work_floats(int S, int A, int H, int L, int B)
{
  return (int64_t)((sens_genome(S, A, H, L) + 3) & ~3) + (int64_t)((B + BP - 1) / BP) * sens_chunk_floats(S, H, L);
}

// genome offset of layer l's weight (layer 0: W0, 1 .. L: the hidden layers, L + 1: Wo)
__device__ __forceinline__ int sens_goff(const Net &n, int l) { return l == 0 ? 0 : n.H * n.S + (l - 1) * n.H * n.H; }

// mlp_bwd for the 2-D weights alone: from D = d/d(the last Linear's output) (an LDS tile) the gradient of every layer's W goes to
// J + sens_goff (added to when accum); biases and LayerNorm parameters are not formed.  Ends with the workgroup's barrier.
template <bool MFMA>
__device__ __forceinline__ void sens_bwd(const Ctx &c, const Net &net, const float *w, const float *x, const float *tape, float *D, float *J, bool accum)
{
  const int nl = net_layers(net), Wd = net_width(net);
  float *X = D == c.T0 ? c.T1 : c.T0;
  for (int l = nl - 1; l >= 0; --l) {
    const Layer y = net_layer(net, l);
    __syncthreads();
    stage(c, l == 0 ? x : tape + (size_t)(2 * (l - 1) + 1) * Wd * BP, y.K, X);
    __syncthreads();
    dense_bwd_w_k<MFMA>(c, D, X, y.N, y.K, J + sens_goff(net, l), accum);
    __syncthreads();
    if (l == 0) break;
    dense_bwd_x_k<MFMA>(c, w + y.oW, y.N, y.K, D, X);
    __syncthreads();
    float *s = D; D = X; X = s;
    const Layer p = net_layer(net, l - 1);
    const float *tn = tape + (size_t)(2 * (l - 1)) * Wd * BP, *th = tn + (size_t)Wd * BP;
    if (p.ln) ln_act_bwd(c, D, w + p.og, p.N, tn, th, tape + (size_t)2 * nl * Wd * BP + (size_t)(l - 1) * BP, nullptr, nullptr, false);
    else
      for (int i = c.g; i < p.N; i += NG) D[i * LP + c.b] *= t_dact(th[i * BP + c.b], c.act);
  }
  __syncthreads();
}

template <bool MFMA>
__global__ void __launch_bounds__(NT) sens_general_kernel(SensArgs a)
{
  extern __shared__ float lds[];
  const int m = blockIdx.x;
  const int S = a.S, A = a.A, H = a.H, L = a.L, G = a.G, nl = L + 2;
  Ctx c;
  c.T0 = lds; c.T1 = c.T0 + TILE_ROWS * LP; c.red4 = c.T1 + TILE_ROWS * LP; c.red = c.red4 + NG * BP;
  c.t = threadIdx.x; c.b = c.t & (BP - 1); c.g = __builtin_amdgcn_readfirstlane(c.t >> 7);
  c.wave = __builtin_amdgcn_readfirstlane(c.t >> 6); c.lane = c.t & 63;
  c.act = a.act;
  const Net actor = {0, S, H, L, A};
  const float *w = a.weights + (size_t)uniform_i(a.members[m]) * a.stride;
  float *J = a.work + (size_t)m * a.work_floats, *chunk0 = J + ((G + 3) & ~3);
  const int64_t chunk_fl = sens_chunk_floats(S, H, L);
  const int chunks = (a.B + BP - 1) / BP;
  const float *st = a.states + (size_t)m * a.B * S;
  float *sc = a.scaling + (size_t)m * G;
  const int b = c.b;
  // the chunk at hand: its rows are samples ch BP .. of the minibatch; c.B / c.B4 / c.live are the chunk's
  auto enter = [&](int ch) {
    const int B = min(a.B - ch * BP, BP);
    c.B = B; c.B4 = (B + 3) & ~3; c.live = (b & 64) < B;
    return B;
  };
  // ---------------- forward, once: samples from B on are zeros (their seeds below are zeros too: they reach no sum)
  for (int ch = 0; ch < chunks; ++ch) {
    const int B = enter(ch);
    float *in_s = chunk0 + ch * chunk_fl;
    if (c.g == 0)
      for (int j = 0; j < S; ++j) in_s[j * BP + b] = b < B ? st[((size_t)ch * BP + b) * S + j] : 0.0f;
    mlp_fwd<MFMA>(c, actor, w, in_s, in_s + (size_t)S * BP);
  }
  for (int e = c.t; e < G; e += NT) sc[e] = 0.0f;
  // ---------------- per output: d sum_b out[b][i] / d genome -> J, chunk after chunk; then sc += J^2
  for (int i = 0; i < A; ++i) {
    for (int ch = 0; ch < chunks; ++ch) {
      const int B = enter(ch);
      const float *in_s = chunk0 + ch * chunk_fl, *tape = in_s + (size_t)S * BP;
      const float *out = tape + (size_t)(2 * (nl - 1) + 1) * H * BP;           // the output layer's tanh values
      float *D = c.T0;
      if (c.g == 0) {
        const float o = out[i * BP + b];
        for (int k = 0; k < A; ++k) D[k * LP + b] = (k == i && b < B) ? 1.0f - o * o : 0.0f;
      }
      sens_bwd<MFMA>(c, actor, w, in_s, tape, D, J, ch > 0);
    }
    for (int e = c.t; e < G; e += NT) sc[e] += J[e] * J[e];
    __syncthreads();                                                         // (J is rewritten by the next output's first chunk)
  }
  // mod_neuro_evo.py:213-217: scaling = sqrt(sum); scaling[scaling == 0] = 1; scaling[scaling < 0.01] = 0.01
  for (int e = c.t; e < G; e += NT) {
    float s = sqrtf(sc[e]);
    if (s == 0.0f) s = 1.0f;
    if (s < 0.01f) s = 0.01f;
    sc[e] = s;
  }
}

}  // namespace

extern "C" {

int64_t serl_ga_sensitivity_general_work_bytes(int32_t n_members, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers,
                                               int32_t batch)
{
  if (n_members < 1 || !serl_learner_range(state_dim, action_dim, hidden, num_layers, batch, BIG_B)) return 0;
  return (int64_t)n_members * sens_work_floats(state_dim, action_dim, hidden, num_layers, batch) * (int64_t)sizeof(float);
}

int serl_ga_sensitivity_general(serl_ctx *c, const float *weights, int64_t stride, int32_t state_dim, int32_t hidden, int32_t num_layers,
                                int32_t action_dim, int32_t activation, const int32_t *members, int32_t n_members, const float *states,
                                int32_t batch, float *scaling, void *work, int64_t work_bytes, int32_t dense, void *stream)
{
  const std::string who("serl_ga_sensitivity_general");
  if (!c || !weights || !members || !states || !scaling || n_members < 0 || batch <= 0) return serl_fail(SERL_E_INVALID, who + ": bad argument");
  if (dense != 0 && dense != 1) return serl_fail(SERL_E_INVALID, who + ": dense must be 0 (valu) or 1 (mfma)");
  SerlShape v = serl_shape_of(SERL_SHAPE_GA_SENSITIVITY_GENERAL, state_dim, action_dim, hidden, num_layers, activation, batch);
  if (v.why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  if (n_members == 0) return SERL_OK;
  if (stride < actor_params(state_dim, action_dim, hidden, num_layers))
    return serl_fail(SERL_E_INVALID, who + ": the row stride is smaller than the parameter count");
  SensArgs a;
  a.work_floats = sens_work_floats(state_dim, action_dim, hidden, num_layers, batch);
  if (!work || work_bytes < (int64_t)n_members * a.work_floats * (int64_t)sizeof(float))
    return serl_fail(SERL_E_INVALID, who + ": workspace NULL or smaller than serl_ga_sensitivity_general_work_bytes");
  const size_t lds = (size_t)v.lds_bytes;
  if ((v = serl_shape_here(c, v)).why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  HIP_TRY(hipSetDevice(c->device));
  a.weights = weights; a.stride = stride; a.members = members; a.states = states; a.scaling = scaling; a.work = (float *)work;
  a.S = state_dim; a.A = action_dim; a.H = hidden; a.L = num_layers; a.act = activation; a.B = batch;
  a.G = sens_genome(state_dim, action_dim, hidden, num_layers);
  void (*kernel)(SensArgs) = dense == 1 ? sens_general_kernel<true> : sens_general_kernel<false>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(n_members), dim3(NT), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

}  // extern "C"

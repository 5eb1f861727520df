// serl_ga_nov.hip -- Actor.get_novelty (base/core/genetic_agent.py:111-115), the key of SSNE.sort_groups_by_distance
// (base/core/mod_neuro_evo.py:411-445), for every actor shape the TD3 learner takes, batch-parallel: serl_ga_novelty_general.
//
// serl_ga_novelty (serl_ga.hip) walks the minibatch one sample at a time, a chain of block reductions per sample, and is fed batches that
// the host gathered from the replay rings, one torch gather per evaluation.  Here one workgroup of NT threads per evaluation e runs the
// learner's forward phases (serl_td3_core.inc: [feature][sample] tiles in LDS, the dense phase in its VALU and f32-MFMA flavours, which
// give the same bits) over chunks of BP samples, and reads its minibatch itself:
//   * gather: sample b of evaluation e is row r = clamp(slots[e][b], 0, n_rows[e] - 1) (slots NULL: r = clamp(b, ..)) of its two bases,
//     state_base[e] + r state_stride and action_base[e] + r action_stride -- a replay ring (base rows, rows + S, both strides 2 S + A + 3)
//     or dense [B][S] / [B][A] arrays; the states go straight into the input tile, no workspace, no tape;
//   * forward: mlp_fwd's layers without a tape (nov_fwd below); B = clamp(batch[e], 0, max_batch), 0 when n_rows[e] < 1; samples from B
//     on are zero columns of the input tile and reach no sum;
//   * reduction, f32, in ONE order whatever the flavour, the launch and the layout:
//       s_b   = ((0 + d_0^2) + d_1^2) + ..          d_a = action[b][a] - out[b][a], a ascending, product and sum rounded separately
//       t_c   = ((s_c + s_(c + 128)) + s_(c + 256)) + s_(c + 384)          column c < 128 over the chunks, ascending; absent samples skipped
//       u_w   = the butterfly x += x[lane ^ o], o = 32, 16, 8, 4, 2, 1, over t_(64 w + lane) (absent columns: +0), w = 0, 1
//       novelty[e] = (u_0 + u_1) / (float)B;  B == 0: NaN (torch's mean of an empty batch)
// Phases are separated by __syncthreads only; no workgroup waits on another; workgroup e writes novelty[e] and nothing else.
#include <hip/hip_runtime.h>
#include <math.h>
#include "serl_ctx.h"
#include "serl_td3_mfma.h"

namespace {

#include "serl_td3_core.inc"

struct NovArgs {
  const float *weights;                 // [pop][stride]
  int64_t stride;
  const int32_t *members;               // [n]
  const float *const *state_base;       // [n]
  const float *const *action_base;      // [n]
  int64_t state_stride, action_stride;  // floats per row
  const int32_t *slots;                 // [n][max_batch] or NULL
  const int32_t *n_rows, *batch;        // [n]
  float *novelty;                       // [n]
  int32_t S, A, H, L, act, max_batch;
};

// mlp_fwd from behind its stage, for an input that already stands in c.T0, without a tape: the same phases in the same order, so an
// output is bit for bit the learner's.  -> the LDS tile that holds the output rows.  Begins and ends with the workgroup's barrier.
template <bool MFMA>
__device__ __forceinline__ float *nov_fwd(const Ctx &c, const Net &net, const float *w)
{
  const int nl = net_layers(net);
  float *Tin = c.T0, *Tout = c.T1;
  __syncthreads();
  for (int l = 0; l < nl; ++l) {
    const Layer y = net_layer(net, l);
    dense_fwd_k<MFMA>(c, w + y.oW, w + y.ob, y.N, y.K, Tin, Tout);
    __syncthreads();
    if (y.ln) ln_act(c, Tout, w + y.og, w + y.obe, y.N, nullptr, nullptr, nullptr);
    else
      for (int i = c.g; i < y.N; i += NG) {
        const float v = Tout[i * LP + c.b];
        Tout[i * LP + c.b] = y.fin == 1 ? tanhf(v) : t_act(v, c.act);
      }
    __syncthreads();
    float *s = Tin; Tin = Tout; Tout = s;
  }
  return Tin;
}

template <bool MFMA>
__global__ void __launch_bounds__(NT) nov_general_kernel(NovArgs a)
{
  extern __shared__ float lds[];
  const int e = blockIdx.x;
  const int S = a.S, A = a.A;
  Ctx c;
  c.T0 = lds; c.T1 = c.T0 + TILE_ROWS * LP; c.red4 = c.T1 + TILE_ROWS * LP; c.red = c.red4 + NG * BP;
  c.t = threadIdx.x; c.b = c.t & (BP - 1); c.g = __builtin_amdgcn_readfirstlane(c.t >> 7);
  c.wave = __builtin_amdgcn_readfirstlane(c.t >> 6); c.lane = c.t & 63;
  c.act = a.act;
  const Net actor = {0, S, a.H, a.L, A};
  const float *w = a.weights + (size_t)uniform_i(a.members[e]) * a.stride;
  const int rows = uniform_i(a.n_rows[e]);
  const int Bt = rows < 1 ? 0 : min(max(uniform_i(a.batch[e]), 0), a.max_batch);
  const float *sp = a.state_base[e], *ap = a.action_base[e];
  const int32_t *sl = a.slots ? a.slots + (size_t)e * a.max_batch : nullptr;
  const int b = c.b;
  float acc = 0.0f;                                                            // t_c of the header, in the threads of group 0
  for (int ch = 0; ch * BP < Bt; ++ch) {
    const int B = min(Bt - ch * BP, BP);
    c.B = B; c.B4 = (B + 3) & ~3; c.live = (b & 64) < B;
    const int idx = ch * BP + b;
    size_t r = 0;
    if (b < B) r = (size_t)min(max(sl ? sl[idx] : idx, 0), rows - 1);
    __syncthreads();                                                           // (the last chunk's outputs may stand in T0)
    for (int j = c.g; j < S; j += NG) c.T0[j * LP + b] = b < B ? sp[r * a.state_stride + j] : 0.0f;
    float av[4] = {0.0f, 0.0f, 0.0f, 0.0f};                                    // A <= 4; fetched ahead of the forward pass
    if (c.g == 0 && b < B)
      for (int k = 0; k < A; ++k) av[k] = ap[r * a.action_stride + k];
    const float *out = nov_fwd<MFMA>(c, actor, w);
    if (c.g == 0 && b < B) {
      float s = 0.0f;
      for (int k = 0; k < A; ++k) { const float d = av[k] - out[k * LP + b]; s = s + d * d; }
      acc = acc + s;
    }
  }
  if (c.g == 0) {                                                              // wavefronts 0 and 1, whole
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (c.lane == 0) c.red[c.wave] = acc;
  }
  __syncthreads();
  if (c.t == 0) a.novelty[e] = Bt > 0 ? (c.red[0] + c.red[1]) / (float)Bt : __int_as_float(0x7fc00000);
}

}  // namespace

extern "C" {

int serl_ga_novelty_general(serl_ctx *c, const float *weights, int64_t stride, int32_t state_dim, int32_t hidden, int32_t num_layers,
                            int32_t action_dim, int32_t activation, const int32_t *members, int32_t n_evals, const float *const *state_base,
                            int64_t state_stride, const float *const *action_base, int64_t action_stride, const int32_t *slots,
                            const int32_t *n_rows, const int32_t *batch, int32_t max_batch, float *novelty, int32_t dense, void *stream)
{
  const std::string who("serl_ga_novelty_general");
  if (!c || !weights || !members || !state_base || !action_base || !n_rows || !batch || !novelty || n_evals < 0)
    return serl_fail(SERL_E_INVALID, who + ": bad argument");
  if (dense != 0 && dense != 1) return serl_fail(SERL_E_INVALID, who + ": dense must be 0 (valu) or 1 (mfma)");
  SerlShape v = serl_shape_of(SERL_SHAPE_GA_NOVELTY_GENERAL, state_dim, action_dim, hidden, num_layers, activation, max_batch);
  if (v.why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  if (n_evals == 0) return SERL_OK;
  if (stride < actor_params(state_dim, action_dim, hidden, num_layers))
    return serl_fail(SERL_E_INVALID, who + ": the row stride is smaller than the parameter count");
  if (state_stride < state_dim || action_stride < action_dim)
    return serl_fail(SERL_E_INVALID, who + ": a row stride of the minibatch is smaller than its row (state_dim, action_dim)");
  const size_t lds = (size_t)v.lds_bytes;
  if ((v = serl_shape_here(c, v)).why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  HIP_TRY(hipSetDevice(c->device));
  NovArgs a;
  a.weights = weights; a.stride = stride; a.members = members; a.state_base = state_base; a.action_base = action_base;
  a.state_stride = state_stride; a.action_stride = action_stride; a.slots = slots; a.n_rows = n_rows; a.batch = batch; a.novelty = novelty;
  a.S = state_dim; a.A = action_dim; a.H = hidden; a.L = num_layers; a.act = activation; a.max_batch = max_batch;
  void (*kernel)(NovArgs) = dense == 1 ? nov_general_kernel<true> : nov_general_kernel<false>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(n_evals), dim3(NT), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

}  // extern "C"

// serl_distill_general.inc -- the training loop of the distillation crossover for every actor shape the TD3 learner takes, as ONE
// launch for all pairs of an epoch.  Included by serl_td3.hip inside its unnamed namespace: the kernel is built from that file's
// training core (mlp_fwd / mlp_bwd over a Net, the dense phases in their VALU and f32-MFMA flavours, clip_adam without the clip).
//
// serl_distill.hip keeps the whole training state of a pair -- parameters, gradients, both Adam moments and the activations of every
// layer -- in LDS, which is what makes it fast and what ties it to hidden 32 x 3 (158 KB there; at hidden 72 x 3 the four parameter
// vectors alone are 4 x 16 995 floats = 272 KB at S 7, A 3).  Here the child's row is trained in place in global memory, gradients and moments
// live in the caller's workspace beside the gathered inputs and the tape (all L2-resident: < 1 MB per pair), and only the activations
// of the layer at hand are in LDS (the learner's two tiles).  The semantics are serl_distill.hip's, restated in tests/distill64.py:
//   * the rows of step `step` are slots[pair][step][0 .. B); a slot outside [0, rows) is clamped into it, batch[pair] into [0, BP] and
//     n_steps[pair] into [0, steps]: what the caller's tables hold is never trusted with an address
//   * keep is a flag, not a weight: a row is kept when keep != 0 as f32 compares (2, -1, 0.5 and a subnormal keep it like 1 does; +0
//     and -0 drop it)
//   * loss = sum((out - target)^2) + mean(out^2) over the rows the keep mask keeps, the mean over kept x A
//   * a minibatch with no kept row takes its Adam step with zero gradients
//   * torch.optim.Adam's defaults with bias correction, no gradient clipping
//   * n_steps[pair] == 0: the row is not written
// One workgroup of NT threads per pair; thread map, tiles and phase barriers are the learner's (the top of serl_td3.hip).

struct DistillGArgs {
  float *child;                 // [pairs][stride]  in: the second parent's parameters, out: the trained child
  int64_t stride;
  const float *states;          // [pairs][rows][S]
  const float *targets;         // [pairs][rows][A]
  const float *keep;            // [pairs][rows]
  const int32_t *slots;         // [pairs][steps][BP]
  const int32_t *n_steps;       // [pairs]
  const int32_t *batch;         // [pairs]
  float *work;                  // [pairs][work_floats]
  int64_t work_floats;
  int32_t rows, steps, S, A, H, L, act;
  float lr;
};

// a pair's workspace: gradients | first moments | second moments | the gathered states [S][BP] | the tape.  Every access to it is one
// float wide: the workspace needs the alignment of a float (4 B) and no more, and so does the child row (f4u above is 4 B aligned).
__host__ __device__ inline int distill_g_param_floats(int S, int A, int H, int L) { return (actor_params(S, A, H, L) + 3) & ~3; }
__host__ __device__ inline int64_t distill_g_work_floats(int S, int A, int H, int L)
{
  return (int64_t)3 * distill_g_param_floats(S, A, H, L) + (int64_t)S * BP + tape_floats(L + 2, H);
}

template <bool MFMA>
__global__ void __launch_bounds__(NT) distill_general_kernel(DistillGArgs a)
{
  extern __shared__ float lds[];
  const int p = blockIdx.x;
  const int S = a.S, A = a.A, H = a.H, L = a.L;
  const int B = min(max(uniform_i(a.batch[p]), 0), BP);
  const int steps = min(max(uniform_i(a.n_steps[p]), 0), a.steps);
  if (steps == 0) return;
  Ctx c;
  c.T0 = lds; c.T1 = c.T0 + TILE_ROWS * LP; c.red4 = c.T1 + TILE_ROWS * LP; c.red = c.red4 + NG * BP;
  c.t = threadIdx.x; c.b = c.t & (BP - 1); c.g = __builtin_amdgcn_readfirstlane(c.t >> 7);
  c.wave = __builtin_amdgcn_readfirstlane(c.t >> 6); c.lane = c.t & 63;
  c.B = B; c.B4 = (B + 3) & ~3; c.act = a.act;
  c.live = (c.b & 64) < B;
  const Net actor = {0, S, H, L, A};
  const int P = actor_params(S, A, H, L), P4 = distill_g_param_floats(S, A, H, L);
  float *w = a.child + (size_t)p * a.stride;
  float *g = a.work + (size_t)p * a.work_floats, *m = g + P4, *v = m + P4, *in_s = v + P4, *tape = in_s + (size_t)S * BP;
  const float *st_p = a.states + (size_t)p * a.rows * S;
  const float *tg_p = a.targets + (size_t)p * a.rows * A;
  const float *kp_p = a.keep + (size_t)p * a.rows;
  const int32_t *sl_p = a.slots + (size_t)p * a.steps * BP;
  for (int e = c.t; e < P; e += NT) { m[e] = 0.0f; v[e] = 0.0f; }
  const int b = c.b;
  const bool on = b < B, mine = on && c.g == 0;          // mine: the thread that holds sample b's target, keep flag and loss gradient
  for (int step = 0; step < steps; ++step) {
    // ---------------- the minibatch: samples from B on are zeros and read no slot
    int slot = mine ? sl_p[(size_t)step * BP + b] : 0;
    slot = min(max(slot, 0), a.rows - 1);
    float tgt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float keep = 0.0f;
    if (c.g == 0) {
      for (int j = 0; j < S; ++j) in_s[j * BP + b] = on ? st_p[(size_t)slot * S + j] : 0.0f;
      if (on) {
        keep = kp_p[slot] != 0.0f ? 1.0f : 0.0f;
        for (int k = 0; k < A; ++k) tgt[k] = tg_p[(size_t)slot * A + k];
      }
    }
    // ---------------- forward, loss (genetic_agent.py:49-52), backward
    float *out = mlp_fwd<MFMA>(c, actor, w, in_s, tape);
    const float kept = block_sum(c, keep);                // (a count of at most 128 ones: exact)
    const float inv_n = kept > 0.0f ? 1.0f / (kept * (float)A) : 0.0f;
    if (c.g == 0)
      for (int k = 0; k < A; ++k) {
        const float o = out[k * LP + b];
        out[k * LP + b] = keep != 0.0f ? (2.0f * (o - tgt[k]) + 2.0f * o * inv_n) * (1.0f - o * o) : 0.0f;
      }
    mlp_bwd<MFMA>(c, actor, w, in_s, tape, out, g, false, DX_NONE);
    // ---------------- Adam (torch.optim.Adam defaults; genetic_agent.py:17), no clip; ends with the workgroup's barrier
    clip_adam<false>(c, w, m, v, g, P, step + 1, a.lr, 0.0f);
  }
}

int distill_general(serl_ctx *c, float *child, int64_t stride, int32_t n_pairs, int32_t state_dim, int32_t hidden, int32_t num_layers,
                    int32_t action_dim, int32_t activation, const float *states, const float *targets, const float *keep, int32_t rows,
                    const int32_t *slots, int32_t steps, const int32_t *n_steps, const int32_t *batch, float lr, void *work, int64_t work_bytes,
                    int32_t dense, void *stream)
{
  const std::string who("serl_ga_distill_general");
  if (!c || !child || !states || !targets || !keep || !slots || !n_steps || !batch || n_pairs < 0 || rows <= 0 || steps < 0 || !(lr > 0.0f))
    return serl_fail(SERL_E_INVALID, who + ": bad argument");
  if (dense != 0 && dense != 1) return serl_fail(SERL_E_INVALID, who + ": dense must be 0 (valu) or 1 (mfma)");
  const SerlShape v = serl_shape_here(c, serl_shape_of(SERL_SHAPE_GA_DISTILL_GENERAL, state_dim, action_dim, hidden, num_layers, activation, 1));
  if (v.why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  const size_t lds = (size_t)v.lds_bytes;
  if (n_pairs == 0 || steps == 0) return SERL_OK;       // (behind every check: a call with nothing to train still says whether it would run)
  const int P = actor_params(state_dim, action_dim, hidden, num_layers);
  if (stride < P) return serl_fail(SERL_E_INVALID, who + ": the row stride is smaller than the parameter count");
  DistillGArgs a;
  a.work_floats = distill_g_work_floats(state_dim, action_dim, hidden, num_layers);
  if (!work || work_bytes < (int64_t)n_pairs * a.work_floats * (int64_t)sizeof(float))
    return serl_fail(SERL_E_INVALID, who + ": workspace NULL or smaller than serl_ga_distill_general_work_bytes");
  HIP_TRY(hipSetDevice(c->device));
  a.child = child; a.stride = stride; a.states = states; a.targets = targets; a.keep = keep; a.slots = slots; a.n_steps = n_steps;
  a.batch = batch; a.work = (float *)work; a.rows = rows; a.steps = steps; a.S = state_dim; a.A = action_dim; a.H = hidden;
  a.L = num_layers; a.act = activation; a.lr = lr;
  void (*kernel)(DistillGArgs) = dense == 1 ? distill_general_kernel<true> : distill_general_kernel<false>;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, dim3(n_pairs), dim3(NT), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

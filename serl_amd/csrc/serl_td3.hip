// serl_td3.hip -- a generation's TD3 gradient updates as ONE launch.
//
// Reference: Agent.train_rl (base/core/agent.py:155-186) calls TD3.update_parameters (base/core/td3.py:123-198) once per frame the
// generation produced -- up to ~100 000 strictly sequential updates of a minibatch of 86 rows through a 7-72x4-3 actor and a twin
// 10-64-64-1 critic, as eager PyTorch a few hundred tiny launches each.  Here one workgroup per learner runs the whole chain of
// updates: minibatches are read straight from the device replay ring through slots the host drew, the Gaussian / uniform draws come
// pre-drawn, parameters and Adam moments live in global memory (four rows plus gradients of a 17 k-parameter actor and a 10 k-parameter
// critic do not fit an LDS; they stay L2-resident), activations move through two LDS tiles in [feature][sample] layout, and what the
// backward passes need again is kept on a tape in the caller's workspace in the same layout.  Phases are separated by __syncthreads
// only; no workgroup ever waits on another (but in the wide flavours, td3_signal / td3_wait below).  f32 like torch; summation orders are this file's (agreement with float64 to rounding,
// tests/test_gpu_td3.py).
//
// Thread map of the dense phases (512 threads): sample b = t & 127, output group g = t >> 7 (uniform per wavefront, so a weight is
// a scalar operand and an activation one LDS read per four multiply-adds).  Weight gradients are batch-reduction products over the
// two tiles: one 4 x 4 block of dW per thread, rows and columns interleaved so that a wavefront's 16 B reads fall into different banks
// (row stride 132 floats).
#include <hip/hip_runtime.h>
#include <math.h>
#include "serl_ctx.h"
#include "serl_rng.h"
#include "serl_td3_mfma.h"

namespace {

#include "serl_td3_core.inc"

// the generator flavours (serl_td3_train_rng): what replaces d.slots / d.target_noise / d.caps_noise
struct Td3Rng {
  uint64_t seed;
  int n_rows, learner0, caps;
};

// what every learner kernel is launched with; a flavour reads the members its source of values has
struct Td3Args {
  serl_td3_desc d;
  int64_t work_floats;                  // per learner
  Td3Rng rg;                            // the generator flavours
  const serl_td3_learner_row *rows;     // the group flavours (serl_td3_train_group): what is per launch above is per learner here, one row each
  int32_t *status;
};

// What one learner's updates run on, in scalar registers: the group flavours fill it from the learner's row (td3_read_row), the others
// from the descriptor and the generator (td3_read_desc); members named like the descriptor's and the generator's they stand in for.
struct Td3Learner {
  const float *ring;
  uint64_t seed;
  int capacity, n_rows, n_updates, iteration0, key, policy_update_freq, update_actor_target, caps;
  float lr, gamma, tau, noise_sd, noise_clip, lambda_s, lambda_t, eps_sd;
};

__device__ __forceinline__ uint64_t uniform_u64(uint64_t v)
{
  return (uint64_t)(uint32_t)uniform_i((int)(uint32_t)v) | (uint64_t)(uint32_t)uniform_i((int)(uint32_t)(v >> 32)) << 32;
}

// a learner's row, read once, every value in scalar registers
__device__ __forceinline__ Td3Learner td3_read_row(const serl_td3_learner_row *row, int caps)
{
  Td3Learner q;
  q.ring = reinterpret_cast<const float *>(uniform_u64(reinterpret_cast<uint64_t>(row->ring)));
  q.seed = uniform_u64(row->seed);
  q.capacity = uniform_i(row->capacity); q.n_rows = uniform_i(row->n_rows); q.n_updates = uniform_i(row->n_updates);
  q.iteration0 = uniform_i(row->iteration0); q.key = uniform_i(row->key); q.policy_update_freq = uniform_i(row->policy_update_freq);
  q.update_actor_target = uniform_i(row->update_actor_target); q.caps = caps;
  q.lr = uniform_f(row->lr); q.gamma = uniform_f(row->gamma); q.tau = uniform_f(row->tau); q.noise_sd = uniform_f(row->noise_sd);
  q.noise_clip = uniform_f(row->noise_clip); q.lambda_s = uniform_f(row->lambda_s); q.lambda_t = uniform_f(row->lambda_t);
  q.eps_sd = uniform_f(row->eps_sd);
  return q;
}

// learner p of a launch whose values are the launch's: kernel arguments, scalar as they come
__device__ __forceinline__ Td3Learner td3_read_desc(const serl_td3_desc &d, const Td3Rng &rg, int p)
{
  Td3Learner q;
  q.ring = d.ring + (size_t)p * d.ring_stride;
  q.seed = rg.seed;
  q.capacity = d.capacity; q.n_rows = rg.n_rows; q.n_updates = d.n_updates; q.iteration0 = d.iteration0; q.key = rg.learner0 + p;
  q.policy_update_freq = d.policy_update_freq; q.update_actor_target = d.update_actor_target; q.caps = rg.caps;
  q.lr = d.lr; q.gamma = d.gamma; q.tau = d.tau; q.noise_sd = d.noise_sd; q.noise_clip = d.noise_clip; q.lambda_s = d.lambda_s;
  q.lambda_t = d.lambda_t; q.eps_sd = d.eps_sd;
  return q;
}

// The host cannot read a device row without a synchronisation: the checks td3_train makes of the same values in a descriptor, made by
// the learner's workgroup.  -> 0, or the code of the first check that fails (enum serl_td3_row_status)
__device__ __forceinline__ int td3_check_row(const Td3Learner &q, int batch, int max_updates)
{
  if (!q.ring) return SERL_TD3_ROW_RING;
  if (q.n_updates < 0 || q.n_updates > max_updates) return SERL_TD3_ROW_UPDATES;
  if (q.iteration0 < 0 || (long long)q.iteration0 + q.n_updates > 2147483646LL) return SERL_TD3_ROW_ITERATION;
  if (q.n_rows < batch || q.n_rows > q.capacity) return SERL_TD3_ROW_ROWS;
  if (q.policy_update_freq < 1) return SERL_TD3_ROW_FREQ;
  if (!(q.lr > 0.0f) || !(q.gamma >= 0.0f) || !(q.tau >= 0.0f && q.tau <= 1.0f) || !(q.noise_sd >= 0.0f) || !(q.noise_clip >= 0.0f) ||
      !(q.eps_sd >= 0.0f) || q.lambda_s != q.lambda_s || q.lambda_t != q.lambda_t)
    return SERL_TD3_ROW_HYPER;
  return SERL_TD3_ROW_OK;
}

// nn.utils.clip_grad_norm_ (coef = max_norm / (norm + 1e-6), applied when below 1) and torch.optim.Adam's step `step` (defaults).
// CLIP = false (the distillation, serl_distill_general.inc) is the same step on the gradients as they are: no norm, max_norm not read.
template <bool CLIP = true>
__device__ __forceinline__ void clip_adam(const Ctx &c, float *w, float *m, float *v, const float *g, int P, int step, float lr, float max_norm)
{
  float coef = 1.0f;
  if constexpr (CLIP) {
    float s = 0.0f;
    for (int e = c.t; e < P; e += NT) s = fmaf(g[e], g[e], s);
    const float norm = sqrtf(block_sum(c, s));
    coef = max_norm / (norm + 1e-6f);
    if (!(coef < 1.0f)) coef = 1.0f;
  }
  const double b1t = pow(0.9, (double)step), b2t = pow(0.999, (double)step);
  const float step_size = (float)((double)lr / (1.0 - b1t));
  const float bc2_sqrt = (float)sqrt(1.0 - b2t);
  // (1 - beta as torch forms them: in double, rounded once -- 1.0f - 0.999f is off by 1.3e-5 of its value)
  const float beta2 = 0.999f, omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
  for (int e = c.t; e < P; e += NT) {
    const float ge = CLIP ? g[e] * coef : g[e];
    const float m1 = m[e] + (ge - m[e]) * omb1;
    const float v1 = v[e] * beta2 + ge * ge * omb2;
    m[e] = m1; v[e] = v1;
    w[e] -= step_size * m1 / (sqrtf(v1) / bc2_sqrt + eps);
  }
  __syncthreads();
}

// The minibatch of (seed; key, iteration) by ONE wavefront: Floyd's algorithm as serl_rng.h defines it (serl_td3_slots_serial is the same
// draw by one thread).  Lane l computes the candidates of steps l, l + 64, .. up front (NR Philox calls), then the steps run in order: the
// chosen rows are held across the lanes (column i in lane i & 63, register i >> 6), a candidate is broadcast by readlane and tested
// against all of them by one ballot.  At most 64 NR steps: NR = 2 for minibatches of up to BP rows, BIG_B / 64 = 8 for the chunked
// flavours -- the same draw, step for step.  out: LDS [B].
template <int NR>
__device__ __forceinline__ void td3_draw_slots_n(uint64_t seed, int key, int iteration, int n_rows, int B, int lane, int *out)
{
  const int j0 = n_rows - B;
  int cand[NR], col[NR];                // col: columns lane + 64 r once chosen (-1: not yet; rows are >= 0)
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    cand[r] = lane + 64 * r < B ? serl_td3_slot_candidate(seed, key, iteration, lane + 64 * r, j0 + lane + 64 * r) : 0;
    col[r] = -1;
  }
#pragma unroll
  for (int r = 0; r < NR; ++r)
    for (int i = 64 * r; i < min(B, 64 * r + 64); ++i) {
      const int t = __shfl(cand[r], i & 63);
      bool held = false;
#pragma unroll
      for (int q = 0; q <= r; ++q) held |= col[q] == t;
      const bool taken = __ballot(held) != 0ull;
      if (lane == (i & 63)) col[r] = taken ? j0 + i : t;
    }
#pragma unroll
  for (int r = 0; r < NR; ++r)
    if (lane + 64 * r < B) out[lane + 64 * r] = col[r];
}

// the target-policy noise of sample b: standard normals, the first A of four
__device__ __forceinline__ void td3_draw_target(uint64_t seed, int key, int iteration, int b, float (&z)[4])
{
  double zd[2 * SERL_RNG_TD3_TARGET_BLOCKS];
  serl_rng_normals<SERL_RNG_TD3_TARGET_BLOCKS>(seed, key, iteration, b, SERL_RNG_TD3_TARGET, zd);
#pragma unroll
  for (int k = 0; k < 4; ++k) z[k] = (float)zd[k];
}

// uniform j of sample b's CAPS draw; w holds the block of the previous call (j ascending: one Philox call per four uniforms)
__device__ __forceinline__ float td3_draw_caps(uint64_t seed, int key, int iteration, int b, int j, uint32_t (&w)[4])
{
  if ((j & 3) == 0) serl_rng_words(seed, key, iteration, b, SERL_RNG_TD3_CAPS, j >> 2, w);
  return serl_td3_caps_uniform(w[j & 3]);
}

// what the phases of a learner's update share; filled once at the top of the kernel
struct Td3Run {
  Td3Learner my;
  Net actor, critic;
  int S, A, B, Pa, Pc1;                 // B: rows of the minibatch; Pa, Pc1: parameters of the actor, of one twin
  float *wa, *wat, *ma, *va, *wc, *wct, *mc, *vc;
  const int32_t *slots;                 // the caller's tables (RNG = false)
  const float *tnoise, *cnoise;
  int slot_cols;
  bool caps;                            // CAPS on: the generator's switch, or the presence of the caller's table
  float *tq;                            // LDS [BP] target Q
  int *slot_l;                          // LDS [BP] or [BIG_B] the minibatch's slots (RNG only: serl_shapes.h slot_rows)
  float max_grad_norm, invB, invBA;
};

// One chunk of BP samples of the minibatch (the only one but in the chunked flavours): sample b of the chunk is sample b0 + b of the
// minibatch, c.B / c.B4 / c.live are the chunk's, k its region of the workspace; gradients are added to from the second chunk on.
struct Td3Chunk {
  Ctx c;
  Td3Work k;
  int b0;
  bool on, accum;                       // on: this thread's sample is one of the minibatch
  float *g_caps;                        // where the spatial CAPS pass puts its gradients: k.g, added to what the main pass left there
  bool accum_caps;                      // -- but in the wide flavours, a vector of its own that nothing is added to
};

// ---- the minibatch: rows slots[u][0 .. B) of the ring; samples from B on are zeros
template <bool RNG>
__device__ __forceinline__ void td3_gather(const Td3Run &r, const Td3Chunk &h, int u, float &rew, float &done)
{
  const Ctx &c = h.c;
  const int S = r.S, A = r.A, SA = S + A, b = c.b;
  const bool on = h.on;
  float *in_s = h.k.in_s, *in_s2 = h.k.in_s2, *in_sa = h.k.in_sa, *in_sa2 = h.k.in_sa2;
  int slot = on ? (RNG ? r.slot_l[h.b0 + b] : r.slots[(size_t)u * r.slot_cols + h.b0 + b]) : 0;
  slot = min(max(slot, 0), r.my.capacity - 1);
  const float *row = r.my.ring + (size_t)slot * (2 * S + A + 3);
  if constexpr (!RNG) __syncthreads();
  if (c.g == 0) {
    for (int j = 0; j < S; ++j) {
      const float s = on ? row[j] : 0.0f, s2 = on ? row[SA + j] : 0.0f;
      in_s[j * BP + b] = s; in_sa[j * BP + b] = s; in_s2[j * BP + b] = s2; in_sa2[j * BP + b] = s2;
    }
    for (int k = 0; k < A; ++k) in_sa[(S + k) * BP + b] = on ? row[S + k] : 0.0f;
  }
  rew = on ? row[2 * S + A] : 0.0f; done = on ? row[2 * S + A + 1] : 0.0f;
}

// ---- target action and target Q (td3.py:137-146) -> r.tq
template <bool MFMA, bool RNG>
__device__ __forceinline__ void td3_target(const Td3Run &r, const Td3Chunk &h, int u, int iteration, float rew, float done)
{
  const Ctx &c = h.c;
  const int S = r.S, A = r.A, B = r.B, b = c.b;
  const bool on = h.on;
  float *in_sa2 = h.k.in_sa2;
  const float *out = mlp_fwd<MFMA>(c, r.actor, r.wat, h.k.in_s2, nullptr);
  float tz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (RNG) {
    if (c.g == 0 && on) td3_draw_target(r.my.seed, r.my.key, iteration, h.b0 + b, tz);
  }
  if (c.g == 0)
    for (int k = 0; k < A; ++k) {
      float nz = on ? (RNG ? tz[k] : r.tnoise[((size_t)u * B + h.b0 + b) * A + k]) * r.my.noise_sd : 0.0f;
      nz = fminf(fmaxf(nz, -r.my.noise_clip), r.my.noise_clip);
      in_sa2[(S + k) * BP + b] = fminf(fmaxf(nz + out[k * LP + b], -1.0f), 1.0f);
    }
  const float q1 = mlp_fwd<MFMA>(c, r.critic, r.wct, in_sa2, nullptr)[b];
  const float q2 = mlp_fwd<MFMA>(c, r.critic, r.wct + r.Pc1, in_sa2, nullptr)[b];
  if (c.g == 0) r.tq[b] = rew + r.my.gamma * (fminf(q1, q2) * (1.0f - done));
}

// ---- critic loss and gradients of both twins (td3.py:149-158); the chunk's share of the loss is added to td, twin by twin; `terms`
// (thread 0 only; NULL but in the wide flavours) gets the two twins' terms one by one, for another workgroup to add in that order
template <bool MFMA>
__device__ __forceinline__ void td3_critic(const Td3Run &r, const Td3Chunk &h, float &td, float *terms = nullptr)
{
  const Ctx &c = h.c;
  const int b = c.b;
  for (int k = 0; k < 2; ++k) {
    float *out = mlp_fwd<MFMA>(c, r.critic, r.wc + k * r.Pc1, h.k.in_sa, h.k.tape_c);
    const float e = (h.on && c.g == 0) ? out[b] - r.tq[b] : 0.0f;
    const float term = block_sum(c, e * e) * r.invB;
    td += term;
    if (terms && c.t == 0) terms[k] = term;
    if (c.g == 0) out[b] = 2.0f * e * r.invB;
    mlp_bwd<MFMA>(c, r.critic, r.wc + k * r.Pc1, h.k.in_sa, h.k.tape_c, out, h.k.g + k * r.Pc1, h.accum, DX_NONE);
  }
}

// ---- actor loss and gradients (td3.py:177-198) with the critic just stepped, both CAPS terms -> the chunk's share of the loss
template <bool MFMA, bool RNG>
__device__ __forceinline__ float td3_actor(const Td3Run &r, const Td3Chunk &h, int iteration, int n_actor)
{
  const Ctx &c = h.c;
  const int S = r.S, A = r.A, SA = S + A, B = r.B, b = c.b;
  const bool on = h.on;
  const float invB = r.invB, invBA = r.invBA;
  float *g = h.k.g, *in_s = h.k.in_s, *in_s2 = h.k.in_s2, *in_sa = h.k.in_sa, *in_sa2 = h.k.in_sa2, *tape_a = h.k.tape_a, *tape_c = h.k.tape_c;
  float *out = mlp_fwd<MFMA>(c, r.actor, r.wa, in_s, tape_a);
  float acur[4] = {0.0f, 0.0f, 0.0f, 0.0f}, abat[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < A; ++k) { acur[k] = out[k * LP + b]; abat[k] = in_sa[(S + k) * BP + b]; }
  __syncthreads();
  if (c.g == 0)
    for (int j = 0; j < SA; ++j) in_sa2[j * BP + b] = j < S ? in_s[j * BP + b] : acur[j - S];
  float *q = mlp_fwd<MFMA>(c, r.critic, r.wc, in_sa2, tape_c);
  float loss = (on && c.g == 0) ? -q[b] * invB : 0.0f;
  if (c.g == 0) q[b] = on ? -invB : 0.0f;
  float *dx = mlp_bwd<MFMA>(c, r.critic, r.wc, in_sa2, tape_c, q, nullptr, false, DX_INPUT);
  float da[4];
  for (int k = 0; k < A; ++k) da[k] = dx[(S + k) * LP + b];
  __syncthreads();
  if (r.caps && on && c.g == 0)
    for (int k = 0; k < A; ++k) {
      const float df = abat[k] - acur[k];
      loss += r.my.lambda_t * df * df * invBA;
      da[k] -= r.my.lambda_t * 2.0f * df * invBA;
    }
  if (c.g == 0)
    for (int k = 0; k < A; ++k) dx[k * LP + b] = da[k] * (1.0f - acur[k] * acur[k]);
  mlp_bwd<MFMA>(c, r.actor, r.wa, in_s, tape_a, dx, g, h.accum, DX_NONE);
  if (r.caps) {
    // state_bar = state + rand * eps_sd; lambda_s * mse(action_batch, actor(state_bar))
    if (c.g == 0) {
      uint32_t cw[4] = {0u, 0u, 0u, 0u};
      for (int j = 0; j < S; ++j) {
        float z = 0.0f;                 // (a sample past the minibatch neither draws nor reads the table: its row is not there)
        if (on) {
          if constexpr (RNG) z = td3_draw_caps(r.my.seed, r.my.key, iteration, h.b0 + b, j, cw);
          else z = r.cnoise[((size_t)n_actor * B + h.b0 + b) * S + j];
        }
        in_s2[j * BP + b] = on ? in_s[j * BP + b] + z * r.my.eps_sd : 0.0f;
      }
    }
    float *ob = mlp_fwd<MFMA>(c, r.actor, r.wa, in_s2, tape_a);
    float abar[4];
    for (int k = 0; k < A; ++k) abar[k] = ob[k * LP + b];
    __syncthreads();
    if (c.g == 0)
      for (int k = 0; k < A; ++k) {
        const float df = on ? abat[k] - abar[k] : 0.0f;
        loss += r.my.lambda_s * df * df * invBA;
        ob[k * LP + b] = -r.my.lambda_s * 2.0f * df * invBA * (1.0f - abar[k] * abar[k]);
      }
    mlp_bwd<MFMA>(c, r.actor, r.wa, in_s2, tape_a, ob, h.g_caps, h.accum_caps, DX_NONE);
  }
  return block_sum(c, loss);
}

// ---- once per actor update: soft updates (mod_utils.py:25-28): target = target * (1 - tau) + param * tau
__device__ __forceinline__ void td3_soft_updates(const Td3Run &r, int t)
{
  const float tau = r.my.tau;
  for (int e = t; e < 2 * r.Pc1; e += NT) r.wct[e] = r.wct[e] * (1.0f - tau) + r.wc[e] * tau;
  if (r.my.update_actor_target)
    for (int e = t; e < r.Pa; e += NT) r.wat[e] = r.wat[e] * (1.0f - tau) + r.wa[e] * tau;
  __syncthreads();
}

// ---- the wide flavours (serl_td3_train_wide): chunk ch of learner p on a workgroup of its own, grid (chunks, learners) ---------------
// Behind the chunked flavours' workspace a learner has, per chunk, three partial gradient vectors of grad_floats each -- the critic's,
// the actor's main pass, the actor's spatial CAPS pass -- and WIDE_LOSS_WORDS floats: the two twins' TD terms, the chunk's pg term.
// In front of all learners' workspaces stand WIDE_SYNC_WORDS words per learner, zeroed by the launch function before every launch:
// arrivals (workgroups 1 .. at workgroup 0), epoch (workgroup 0 to the others), the time-out word, one spare.
constexpr int WIDE_SYNC_WORDS = 4;
constexpr int WIDE_LOSS_WORDS = 4;
constexpr unsigned long long WIDE_SPIN_TICKS = 400000000ull;   // 4 s of wall_clock64's 100 MHz: the other workgroups may not be resident yet
__host__ __device__ inline int64_t wide_chunk_floats(int S, int A, int H, int L) { return (int64_t)3 * grad_floats(S, A, H, L) + WIDE_LOSS_WORDS; }

// The producer's side of a hand-over: every wavefront's stores have left it, the workgroup has met, then ONE lane releases at agent
// scope and bumps (add) or sets the word the other side polls.
__device__ __forceinline__ void td3_signal(const Ctx &c, unsigned *word, bool add, unsigned value)
{
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (c.t == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (add) __hip_atomic_fetch_add(word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_store(word, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The consumer's side: wavefront 0 polls the word relaxed until it has reached `target`, then ONE agent-scope acquire, its loads
// drained, and the workgroup's barrier before any other wavefront loads what was handed over.  The spin is bounded: after
// WIDE_SPIN_TICKS the time-out word is set to `code` (the first one to expire wins), and a set time-out word ends every wait of the
// learner.  -> 0, or the time-out word (uniform over the workgroup, through c.red[NW])
__device__ __forceinline__ unsigned td3_wait(const Ctx &c, unsigned *word, unsigned target, unsigned *tmo, unsigned code)
{
  if (c.wave == 0) {
    unsigned lost = 0;
    const unsigned long long t0 = wall_clock64();
    while ((int)(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      lost = __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lost) break;
      if (wall_clock64() - t0 > WIDE_SPIN_TICKS) {
        unsigned seen = 0;
        if (c.lane == 0 && !__hip_atomic_compare_exchange_strong(tmo, &seen, code, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
          code = seen;
        lost = (unsigned)uniform_i((int)code);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (c.lane == 0) c.red[NW] = __uint_as_float(lost);
  }
  __syncthreads();
  return __float_as_uint(c.red[NW]);
}

// Workgroup 0 of a wide learner: g[e] = the chunks' partial vectors added in serl_td3_train_big's order -- chunk 0's, + chunk 1's, ..;
// with `second`, per chunk first `part` (the main pass), then `second` (the CAPS pass), as that kernel's passes add to one vector
__device__ __forceinline__ void td3_reduce(const Ctx &c, float *g, const float *part, const float *second, int64_t stride, int G, int P)
{
  for (int e = c.t; e < P; e += NT) {
    float s = part[e];
    if (second) s += second[e];
    for (int ch = 1; ch < G; ++ch) {
      s += part[ch * stride + e];
      if (second) s += second[ch * stride + e];
    }
    g[e] = s;
  }
  __syncthreads();
}

// The learner kernel, one workgroup per learner, every flavour an instantiation of this one update.
// RNG = false: slots and draws from the caller's tables (serl_td3_train / _mfma).  RNG = true: the same source, with the slot read from
// an LDS array one wavefront fills at the top of each update and both draws generated in registers by the thread that would read them.
// GROUP = true (with RNG; serl_td3_train_group, with BIG / WIDE _group_big / _group_wide): the same source again, with what is one value per launch elsewhere -- the ring, the
// counts, the hyper-parameters, the generator's seed and key -- taken from the learner's row, which the workgroup reads and checks
// itself before it touches any other memory.
// BIG = true (the chunked flavours, serl_td3_train_big): minibatches of up to BIG_B rows, walked in chunks of BP samples (the last one
// may be partial).  Everything per sample -- the gather, the forward and backward passes, the draws -- runs per chunk with the thread
// map, the tiles and the device functions above; every chunk has its own inputs and tapes in the workspace; a batch sum (a gradient, a
// loss) is chunk 0's partial sum, then + chunk 1's, + chunk 2's, + chunk 3's (include/serl_amd.h states the order); the means divide by
// the minibatch's B; the clip, Adam and the soft updates run once, after the last chunk.  BIG = false is the one chunk at sample 0 that
// nothing is added to, known when the flavour is compiled.
// WIDE = true (with BIG; serl_td3_train_wide): the same chunks, chunk ch of learner p on workgroup (ch, p) of a grid (chunks, learners)
// for the whole call.  A workgroup runs the per-sample phases of its chunk only and writes partial sums nothing is added to; workgroup 0
// of the learner adds them up in the chunked flavours' order (td3_reduce, and the loss terms one by one) and alone runs the clip, Adam,
// the soft updates and the stores of the losses.  Four hand-overs per update (td3_signal / td3_wait):
//   A  every workgroup's critic partials and TD terms -> workgroup 0        B  the stepped critic -> every workgroup
//   C  (actor updates) the actor partials and pg terms -> workgroup 0       D  the stepped actor and the targets -> every workgroup
// B is left out when nothing follows it (no actor step, last update), D behind the last update.  A minibatch of one chunk runs as the
// chunked flavour does, with no hand-over at all.
// In a group (GROUP with WIDE) status[p] is the row check's word too, so a time-out is reported with a code above the check's
// (SERL_TD3_ROW_HANDOVER_A ..); every condition above is decided from the learner's own row, so that all workgroups of a learner leave
// the loop behind the same hand-over, and a learner with no updates makes none.
enum Td3Handover { TD3_HO_A = SERL_TD3_WIDE_A, TD3_HO_B = SERL_TD3_WIDE_B, TD3_HO_C = SERL_TD3_WIDE_C, TD3_HO_D = SERL_TD3_WIDE_D };
static_assert(SERL_TD3_ROW_HANDOVER_B - SERL_TD3_ROW_HANDOVER_A == TD3_HO_B - TD3_HO_A && SERL_TD3_ROW_HANDOVER_C - SERL_TD3_ROW_HANDOVER_A == TD3_HO_C - TD3_HO_A &&
              SERL_TD3_ROW_HANDOVER_D - SERL_TD3_ROW_HANDOVER_A == TD3_HO_D - TD3_HO_A, "a group's time-out codes follow the single learner's, offset");

template <bool MFMA, bool RNG, bool GROUP, bool BIG, bool WIDE = false>
__global__ void __launch_bounds__(NT) td3_kernel(Td3Args a)
{
  static_assert(RNG || !GROUP, "the group flavours draw inside the kernel");
  static_assert(BIG || !WIDE, "the wide flavours are chunked ones");
  extern __shared__ float lds[];
  const serl_td3_desc &d = a.d;
  const int p = WIDE ? blockIdx.y : blockIdx.x;
  const int my_ch = WIDE ? blockIdx.x : 0;
  Td3Run r;
  if constexpr (GROUP) {
    r.my = td3_read_row(a.rows + p, a.rg.caps);
    const int refused = td3_check_row(r.my, d.batch, d.n_updates);
    // (a wide group: all workgroups of the learner read the same row and decide alike without talking; the lead reports)
    if (threadIdx.x == 0 && my_ch == 0) a.status[p] = refused;
    if (refused != SERL_TD3_ROW_OK) return;
  } else {
    r.my = td3_read_desc(d, a.rg, p);
  }
  const Td3Learner &my = r.my;
  Ctx c;
  c.T0 = lds; c.T1 = c.T0 + TILE_ROWS * LP; c.red4 = c.T1 + TILE_ROWS * LP; c.red = c.red4 + NG * BP;
  r.tq = c.red + 64;
  r.slot_l = reinterpret_cast<int *>(r.tq + BP);
  c.t = threadIdx.x; c.b = c.t & (BP - 1); c.g = __builtin_amdgcn_readfirstlane(c.t >> 7);
  c.wave = __builtin_amdgcn_readfirstlane(c.t >> 6); c.lane = c.t & 63;
  c.B = d.batch; c.B4 = (d.batch + 3) & ~3; c.act = d.activation;
  c.live = (c.b & 64) < c.B;
  const int S = d.state_dim, A = d.action_dim, B = d.batch;
  r.S = S; r.A = A; r.B = B;
  r.actor = {0, S, d.hidden, d.num_layers, A}; r.critic = {1, S, d.hidden, d.num_layers, A};
  r.Pa = actor_params(S, A, d.hidden, d.num_layers); r.Pc1 = twin_params(S, A);
  r.wa = d.actor + (size_t)p * d.actor_stride; r.wat = d.actor_target + (size_t)p * d.actor_stride;
  r.ma = d.actor_m + (size_t)p * d.actor_stride; r.va = d.actor_v + (size_t)p * d.actor_stride;
  r.wc = d.critic + (size_t)p * d.critic_stride; r.wct = d.critic_target + (size_t)p * d.critic_stride;
  r.mc = d.critic_m + (size_t)p * d.critic_stride; r.vc = d.critic_v + (size_t)p * d.critic_stride;
  r.slots = RNG ? nullptr : d.slots + (size_t)p * d.slots_stride;
  r.slot_cols = d.slot_cols;
  r.tnoise = RNG ? nullptr : d.target_noise + (size_t)p * d.noise_stride;
  r.cnoise = RNG || !d.caps_noise ? nullptr : d.caps_noise + (size_t)p * d.caps_stride;
  r.caps = RNG ? my.caps != 0 : d.caps_noise != nullptr;
  r.max_grad_norm = d.max_grad_norm; r.invB = 1.0f / (float)B; r.invBA = 1.0f / (float)(B * A);
  float *td_loss = d.td_loss + (size_t)p * d.loss_stride, *pg_loss = d.pg_loss + (size_t)p * d.loss_stride;
  float *wk = (float *)d.work + (WIDE ? (size_t)WIDE_SYNC_WORDS * d.n_learners : 0) + (size_t)p * a.work_floats;
  const int Pc = 2 * r.Pc1;
  int step_c = d.adam_steps[2 * p], step_a = d.adam_steps[2 * p + 1];
  int n_actor = 0;
  const int n_chunks = BIG ? (B + BP - 1) / BP : 1;
  // the wide flavours: this workgroup's chunk only; `spread`: the learner has more workgroups than this one, which is `lead` when it is
  // workgroup 0; part: the chunks' partial vectors and loss terms behind the chunked flavours' workspace
  const int ch0 = WIDE ? my_ch : 0, ch1 = WIDE ? my_ch + 1 : n_chunks;
  const bool spread = WIDE && n_chunks > 1, lead = !WIDE || my_ch == 0;
  const int gf = grad_floats(S, A, d.hidden, d.num_layers);
  const int64_t part_stride = wide_chunk_floats(S, A, d.hidden, d.num_layers);
  float *part = wk + gf + n_chunks * chunk_floats(d.hidden, d.num_layers);
  float *my_part = part + my_ch * part_stride;
  unsigned *sync = reinterpret_cast<unsigned *>(d.work) + WIDE_SYNC_WORDS * p;
  unsigned arrivals = 0, epoch = 0;             // what workgroup 0 waits for next in sync[0], the others in sync[1]; sync[2]: the time-out word
  auto chunk = [&](int ch, bool actor_phase) {
    Td3Chunk h;
    h.c = c;
    h.b0 = BIG ? ch * BP : 0;
    if constexpr (BIG) { h.c.B = min(BP, B - h.b0); h.c.B4 = (h.c.B + 3) & ~3; h.c.live = (c.b & 64) < h.c.B; }
    h.k = td3_carve(wk, S, A, d.hidden, d.num_layers, BIG ? ch : 0);
    h.on = h.b0 + c.b < B;
    h.accum = BIG && ch > 0;
    h.g_caps = h.k.g; h.accum_caps = true;
    if constexpr (WIDE) {
      if (spread) { h.accum = false; h.k.g = my_part + (actor_phase ? gf : 0); h.g_caps = my_part + 2 * gf; h.accum_caps = false; }
    }
    return h;
  };
  // hand-over `code` of a spread learner, towards workgroup 0 (in) or from it; -> false: a wait of the learner ran out of time, the
  // status says so and the workgroup is done
  auto handover = [&](bool in, unsigned code) {
    if constexpr (GROUP) code += SERL_TD3_ROW_HANDOVER_A - TD3_HO_A;
    unsigned lost = 0;
    if (in) {
      arrivals += n_chunks - 1;
      if (lead) lost = td3_wait(c, sync, arrivals, sync + 2, code);
      else td3_signal(c, sync, true, 0u);
    } else {
      ++epoch;
      if (lead) td3_signal(c, sync + 1, false, epoch);
      else lost = td3_wait(c, sync + 1, epoch, sync + 2, code);
    }
    if (lost && c.t == 0) a.status[p] = (int32_t)lost;
    return lost == 0;
  };

  for (int u = 0; u < my.n_updates; ++u) {
    const int iteration = my.iteration0 + u + 1;
    if constexpr (RNG) {
      if (c.wave == 0) td3_draw_slots_n<(BIG ? BIG_B : BP) / 64>(my.seed, my.key, iteration, my.n_rows, B, c.lane, r.slot_l);
      __syncthreads();
    }
    float td = 0.0f;
    for (int ch = ch0; ch < ch1; ++ch) {
      const Td3Chunk h = chunk(ch, false);
      float rew, done;
      td3_gather<RNG>(r, h, u, rew, done);
      td3_target<MFMA, RNG>(r, h, u, iteration, rew, done);
      td3_critic<MFMA>(r, h, td, spread ? my_part + 3 * gf : nullptr);
    }
    if constexpr (WIDE) {
      if (spread) {
        if (!handover(true, TD3_HO_A)) return;
        if (lead) {
          td3_reduce(c, wk, part, nullptr, part_stride, n_chunks, Pc);
          td = 0.0f;
          for (int ch = 0; ch < n_chunks; ++ch) { td += part[ch * part_stride + 3 * gf]; td += part[ch * part_stride + 3 * gf + 1]; }
        }
      }
    }
    ++step_c;
    if (lead) {
      clip_adam(c, r.wc, r.mc, r.vc, wk, Pc, step_c, my.lr, r.max_grad_norm);
      if (c.t == 0) td_loss[u] = td;
    }
    const bool actor_step = iteration % my.policy_update_freq == 0;
    if constexpr (WIDE) {
      if (spread && (actor_step || u + 1 < my.n_updates) && !handover(false, TD3_HO_B)) return;
    }
    if (!actor_step) continue;
    float pg = 0.0f;
    for (int ch = ch0; ch < ch1; ++ch) {
      const float chunk_pg = td3_actor<MFMA, RNG>(r, chunk(ch, true), iteration, n_actor);
      pg = ch == ch0 ? chunk_pg : pg + chunk_pg;
    }
    if constexpr (WIDE) {
      if (spread) {
        if (c.t == 0) my_part[3 * gf + 2] = pg;
        if (!handover(true, TD3_HO_C)) return;
        if (lead) {
          td3_reduce(c, wk, part + gf, r.caps ? part + 2 * gf : nullptr, part_stride, n_chunks, r.Pa);
          pg = part[3 * gf + 2];
          for (int ch = 1; ch < n_chunks; ++ch) pg += part[ch * part_stride + 3 * gf + 2];
        }
      }
    }
    ++step_a; ++n_actor;
    if (lead) {
      clip_adam(c, r.wa, r.ma, r.va, wk, r.Pa, step_a, my.lr, r.max_grad_norm);
      if (c.t == 0) pg_loss[u] = pg;
      td3_soft_updates(r, c.t);
    }
    if constexpr (WIDE) {
      if (spread && u + 1 < my.n_updates && !handover(false, TD3_HO_D)) return;
    }
  }
  if (lead && c.t == 0 && my.n_updates > 0) {
    d.adam_steps[2 * p] = step_c; d.adam_steps[2 * p + 1] = step_a;
    if constexpr (WIDE && !GROUP) a.status[p] = 0;      // (a group's status is the row check's, written at the top)
  }
}

// what serl_td3_train_rng draws, written out as the tables serl_td3_train takes: one workgroup of THREADS (BP; BIG_B for the chunked
// flavours' tables) per update, the slots by its first wavefront (td3_draw_slots_n), thread b the draws of sample b (td3_draw_target /
// td3_draw_caps)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) td3_rng_fill_kernel(Td3Rng rg, int key, int S, int A, int B, int iteration0, int freq, int32_t *slots,
                                                               float *tn, float *cn)
{
  __shared__ int slot_l[THREADS];
  const int u = blockIdx.x, b = threadIdx.x, iteration = iteration0 + u + 1;
  if (b < 64) td3_draw_slots_n<THREADS / 64>(rg.seed, key, iteration, rg.n_rows, B, b, slot_l);
  __syncthreads();
  if (b >= B) return;
  slots[(size_t)u * B + b] = slot_l[b];
  float tz[4];
  td3_draw_target(rg.seed, key, iteration, b, tz);
  for (int k = 0; k < A; ++k) tn[((size_t)u * B + b) * A + k] = tz[k];
  if (!cn || iteration % freq != 0) return;
  const int n_actor = iteration / freq - iteration0 / freq - 1;      // actor updates of the call before this one
  uint32_t cw[4] = {0u, 0u, 0u, 0u};
  for (int j = 0; j < S; ++j) cn[((size_t)n_actor * B + b) * S + j] = td3_draw_caps(rg.seed, key, iteration, b, j, cw);
}

// per learner; `chunks` chunks of BP samples (1 but for the chunked flavours): the gradients once, inputs and tapes per chunk
int64_t td3_work_floats(int S, int A, int H, int L, int chunks = 1) { return grad_floats(S, A, H, L) + chunks * chunk_floats(H, L); }

// What an entry point asks of td3_train: its name for serl_last_error(), where a learner's values and draws come from, and the flavour.
//   TABLES     the descriptor holds everything (serl_td3_train / _mfma; _big without a generator)
//   GENERATOR  slots and noise are drawn in the kernel: the descriptor's tables -- slots, slot_cols, target_noise, caps_noise and their
//              strides -- are not looked at, `rng` is checked last and rng->dense picks the dense phases (serl_td3_train_rng; _big)
//   GROUP      drawn in the kernel too, and what a learner's row holds -- ring, ring_stride, capacity, iteration0, policy_update_freq,
//              update_actor_target and the eight hyper-parameters -- is not looked at either: the row's workgroup checks it
//              (td3_check_row); `group` takes the generator's place, and the launch is made for n_updates == 0 too, since the status
//              array is the report (serl_td3_train_group)
// big (serl_td3_train_big; with GROUP serl_td3_train_group_big): the minibatch may have up to BIG_B rows, the workspace is that of serl_td3_big_work_bytes,
// the chunked flavours are launched, and with GENERATOR rng->dense must name the flavour `mfma` asks for.
// wide (serl_td3_train_wide; with GROUP serl_td3_train_group_wide; with big): the workspace is that of serl_td3_wide_work_bytes, the launch is refused when its workgroups
// outnumber the device's CUs, the learners' synchronisation words are zeroed on the stream and the wide flavours are launched on a grid
// (chunks, learners); `status` is the learners' report (a group's is its descriptor's, which the row checks write too).
enum Td3Source { TD3_TABLES, TD3_GENERATOR, TD3_GROUP };
struct Td3Call {
  const char *fn;
  Td3Source source;
  const serl_td3_rng_desc *rng = nullptr;
  const serl_td3_group_desc *group = nullptr;
  bool mfma = false, big = false, wide = false;
  int32_t *status = nullptr;
};

// the twelve learner kernels of one workgroup per learner by [big][group][rng][mfma]; a flavour that does not exist is NULL (a group
// draws inside the kernel)
typedef void (*Td3Kernel)(Td3Args);
#define TD3_K(rng, group, big) {td3_kernel<false, rng, group, big>, td3_kernel<true, rng, group, big>}
const Td3Kernel TD3_KERNELS[2][2][2][2] = {{{TD3_K(false, false, false), TD3_K(true, false, false)}, {{nullptr, nullptr}, TD3_K(true, true, false)}},
                                           {{TD3_K(false, false, true), TD3_K(true, false, true)}, {{nullptr, nullptr}, TD3_K(true, true, true)}}};
#undef TD3_K
// the six wide kernels by [group][rng][mfma]
const Td3Kernel TD3_WIDE_KERNELS[2][2][2] = {{{td3_kernel<false, false, false, true, true>, td3_kernel<true, false, false, true, true>},
                                              {td3_kernel<false, true, false, true, true>, td3_kernel<true, true, false, true, true>}},
                                             {{nullptr, nullptr}, {td3_kernel<false, true, true, true, true>, td3_kernel<true, true, true, true, true>}}};

int td3_launch(Td3Kernel kernel, const Td3Args &a, size_t lds, void *stream, dim3 grid)
{
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, dim3(NT), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

// every entry: the checks in one order, then the launch of the flavour asked for
int td3_train(serl_ctx *c, const serl_td3_desc *d, void *stream, const Td3Call &call)
{
  const std::string who(call.fn);
  const bool tables = call.source == TD3_TABLES;        // the descriptor's tables are read
  const bool own = call.source != TD3_GROUP;            // the descriptor's ring, counts and hyper-parameters are the learners'
  const bool big = call.big;
  if (!c || !d) return serl_fail(SERL_E_INVALID, who + ": NULL context or descriptor");
  if (!d->actor || !d->actor_target || !d->actor_m || !d->actor_v || !d->critic || !d->critic_target || !d->critic_m || !d->critic_v ||
      !d->adam_steps || (own && !d->ring) || (tables && (!d->slots || !d->target_noise)) || !d->td_loss || !d->pg_loss || !d->work)
    return serl_fail(SERL_E_INVALID, who + ": NULL array (only caps_noise may be NULL: CAPS off)");
  // (the shape's two refusals stand where they always stood among the others: arguments first, the range behind the hyper-parameters, the LDS last)
  SerlShape v = serl_shape_td3(d->state_dim, d->action_dim, d->hidden, d->num_layers, d->activation, d->batch, big, tables ? 0 : big ? BIG_B : BP);
  if (v.code == SERL_E_INVALID) return serl_refuse(who, v);
  if (d->n_learners < 1 || d->n_updates < 0 || (own && d->capacity < 1) || (tables && d->slot_cols < d->batch) ||
      (own && (d->policy_update_freq < 1 || d->iteration0 < 0)))
    return serl_fail(SERL_E_INVALID, who + ": n_learners >= 1, n_updates >= 0, capacity >= 1, slot_cols >= batch, policy_update_freq >= 1, iteration0 >= 0");
  if (own && (long long)d->iteration0 + d->n_updates > 2147483646LL) return serl_fail(SERL_E_INVALID, who + ": iteration0 + n_updates overflows");
  if (!(d->max_grad_norm > 0.0f) ||
      (own && (!(d->lr > 0.0f) || !(d->gamma >= 0.0f) || !(d->tau >= 0.0f && d->tau <= 1.0f) || !(d->noise_sd >= 0.0f) || !(d->noise_clip >= 0.0f) ||
               !(d->eps_sd >= 0.0f) || d->lambda_s != d->lambda_s || d->lambda_t != d->lambda_t)))
    return serl_fail(SERL_E_INVALID, who + ": lr > 0, gamma >= 0, 0 <= tau <= 1, noise_sd >= 0, noise_clip >= 0, max_grad_norm > 0, eps_sd >= 0");
  if (v.why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  const int Pa = serl_param_count(d->state_dim, d->hidden, d->num_layers, d->action_dim), Pc = serl_td3_param_count(d->state_dim, d->action_dim);
  if (d->actor_stride < Pa || d->critic_stride < Pc) return serl_fail(SERL_E_INVALID, who + ": a row stride is smaller than its parameter count");
  if ((own && d->ring_stride < 0) || (tables && (d->slots_stride < 0 || d->noise_stride < 0 || d->caps_stride < 0)) || d->loss_stride < d->n_updates)
    return serl_fail(SERL_E_INVALID, who + ": negative learner stride, or loss_stride < n_updates");
  Td3Args a = {};
  a.d = *d;
  const int chunks = big ? (d->batch + BP - 1) / BP : 1;
  a.work_floats = td3_work_floats(d->state_dim, d->action_dim, d->hidden, d->num_layers, chunks) +
                  (call.wide ? chunks * wide_chunk_floats(d->state_dim, d->action_dim, d->hidden, d->num_layers) : 0);
  if (d->work_bytes < (int64_t)d->n_learners * (a.work_floats + (call.wide ? WIDE_SYNC_WORDS : 0)) * (int64_t)sizeof(float))
    return serl_fail(SERL_E_INVALID, who + ": workspace smaller than " +
                                         (call.wide ? "serl_td3_wide_work_bytes" : big ? "serl_td3_big_work_bytes" : "serl_td3_work_bytes"));
  const size_t lds = (size_t)v.lds_bytes;
  if ((v = serl_shape_here(c, v)).why != SERL_SHAPE_WHY_TAKES) return serl_refuse(who, v);
  bool mfma = call.mfma;
  if (call.source == TD3_GROUP) {
    const serl_td3_group_desc *gd = call.group;
    if (!gd || !gd->rows || !gd->status) return serl_fail(SERL_E_INVALID, who + ": NULL group descriptor, rows or status");
    if (gd->dense != 0 && gd->dense != 1) return serl_fail(SERL_E_INVALID, who + ": dense must be 0 (valu) or 1 (mfma)");
    if (gd->caps != 0 && gd->caps != 1) return serl_fail(SERL_E_INVALID, who + ": caps must be 0 or 1");
    mfma = gd->dense == 1;
    a.rows = gd->rows; a.status = gd->status; a.rg.caps = gd->caps;
  } else if (call.source == TD3_GENERATOR) {
    const serl_td3_rng_desc *rg = call.rng;
    if (!rg) return serl_fail(SERL_E_INVALID, who + ": NULL generator descriptor");
    if (rg->n_rows < d->batch || rg->n_rows > d->capacity) return serl_fail(SERL_E_INVALID, who + ": batch <= n_rows <= capacity");
    if ((long long)rg->learner0 + d->n_learners > 2147483647LL) return serl_fail(SERL_E_INVALID, who + ": learner0 + n_learners overflows");
    if (rg->dense != 0 && rg->dense != 1) return serl_fail(SERL_E_INVALID, who + ": dense must be 0 (valu) or 1 (mfma)");
    if (rg->caps != 0 && rg->caps != 1) return serl_fail(SERL_E_INVALID, who + ": caps must be 0 or 1");
    if (big && (rg->dense == 1) != mfma) return serl_fail(SERL_E_INVALID, who + ": the generator's dense differs from the big descriptor's");
    mfma = rg->dense == 1;
    a.rg = {rg->seed, rg->n_rows, rg->learner0, rg->caps};
  }
  if (call.wide && (int64_t)d->n_learners * chunks > c->caps.num_cus)
    return serl_fail(SERL_E_UNSUPPORTED, who + ": n_learners x chunks workgroups wait on each other and must all be resident: more than the device's CUs");
  if (d->n_updates == 0 && own) return SERL_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (call.wide) {
    // (one workgroup per CU by LDS size; a learner of one chunk polls nothing, but the block is zeroed all the same)
    if (own) a.status = call.status;
    HIP_TRY(hipMemsetAsync(d->work, 0, (size_t)d->n_learners * WIDE_SYNC_WORDS * sizeof(uint32_t), (hipStream_t)stream));
    return td3_launch(TD3_WIDE_KERNELS[!own][!tables][mfma], a, lds, stream, dim3(chunks, d->n_learners));
  }
  return td3_launch(TD3_KERNELS[big][!own][!tables][mfma], a, lds, stream, dim3(d->n_learners));
}

// serl_td3_rng_fill / _big: one set of checks, then the fill kernel of BP or BIG_B threads per update
int td3_rng_fill(serl_ctx *c, const serl_td3_rng_desc *rg, int32_t learner, int32_t state_dim, int32_t action_dim, int32_t batch, int32_t iteration0,
                 int32_t n_updates, int32_t policy_update_freq, int32_t *slots, float *target_noise, float *caps_noise, void *stream, bool big, const char *fn)
{
  const std::string who(fn);
  if (!c || !rg || !slots || !target_noise) return serl_fail(SERL_E_INVALID, who + ": NULL argument (only caps_noise may be NULL: not written)");
  if (state_dim < 1 || state_dim > 16 || action_dim < 1 || action_dim > 4 || batch < 1 || batch > (big ? BIG_B : BP))
    return serl_fail(SERL_E_INVALID, who + ": state_dim 1 .. 16, action_dim 1 .. 4, batch 1 .. " + (big ? "512" : "128"));
  if (learner < 0 || n_updates < 0 || policy_update_freq < 1 || iteration0 < 0 || (long long)iteration0 + n_updates > 2147483646LL ||
      (long long)rg->learner0 + learner > 2147483647LL)
    return serl_fail(SERL_E_INVALID, who + ": learner >= 0, n_updates >= 0, policy_update_freq >= 1, iteration0 >= 0, no overflow");
  if (rg->n_rows < batch) return serl_fail(SERL_E_INVALID, who + ": n_rows < batch");
  if (n_updates == 0) return SERL_OK;
  HIP_TRY(hipSetDevice(c->device));
  const Td3Rng r = {rg->seed, rg->n_rows, rg->learner0, rg->caps};
  hipLaunchKernelGGL(big ? td3_rng_fill_kernel<BIG_B> : td3_rng_fill_kernel<BP>, dim3(n_updates), dim3(big ? BIG_B : BP), 0, (hipStream_t)stream, r,
                     (int)(rg->learner0 + learner), (int)state_dim, (int)action_dim, (int)batch, (int)iteration0, (int)policy_update_freq, slots,
                     target_noise, caps_noise);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

// what a layout function answers: the n values of v, up to `capacity` of them copied to out when given
template <int N>
int td3_layout_out(const int32_t (&v)[N], int32_t *out, int32_t capacity)
{
  for (int i = 0; i < N && i < capacity; ++i)
    if (out) out[i] = v[i];
  return N;
}

#include "serl_distill_general.inc"

}  // namespace

extern "C" {

int serl_td3_param_count(int state_dim, int action_dim)
{
  if (state_dim < 1 || action_dim < 1) return 0;
  return 2 * twin_params(state_dim, action_dim);
}

int64_t serl_td3_work_bytes(int32_t n_learners, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t batch)
{
  if (n_learners < 1 || !serl_learner_range(state_dim, action_dim, hidden, num_layers, batch, BP)) return 0;
  return (int64_t)n_learners * td3_work_floats(state_dim, action_dim, hidden, num_layers) * (int64_t)sizeof(float);
}

int serl_td3_layout(int32_t *out, int32_t capacity)
{
#define TD3_OFF(m) (int32_t)offsetof(serl_td3_desc, m)
  const int32_t v[] = {
    (int32_t)sizeof(serl_td3_desc),
    TD3_OFF(state_dim), TD3_OFF(action_dim), TD3_OFF(hidden), TD3_OFF(num_layers), TD3_OFF(activation), TD3_OFF(n_learners), TD3_OFF(batch),
    TD3_OFF(n_updates), TD3_OFF(capacity), TD3_OFF(slot_cols), TD3_OFF(policy_update_freq), TD3_OFF(iteration0), TD3_OFF(update_actor_target),
    TD3_OFF(pad0), TD3_OFF(lr), TD3_OFF(gamma), TD3_OFF(tau), TD3_OFF(noise_sd), TD3_OFF(noise_clip), TD3_OFF(lambda_s), TD3_OFF(lambda_t),
    TD3_OFF(eps_sd), TD3_OFF(max_grad_norm), TD3_OFF(pad1), TD3_OFF(actor), TD3_OFF(actor_target), TD3_OFF(actor_m), TD3_OFF(actor_v),
    TD3_OFF(actor_stride), TD3_OFF(critic), TD3_OFF(critic_target), TD3_OFF(critic_m), TD3_OFF(critic_v), TD3_OFF(critic_stride),
    TD3_OFF(adam_steps), TD3_OFF(ring), TD3_OFF(ring_stride), TD3_OFF(slots), TD3_OFF(slots_stride), TD3_OFF(target_noise),
    TD3_OFF(noise_stride), TD3_OFF(caps_noise), TD3_OFF(caps_stride), TD3_OFF(td_loss), TD3_OFF(pg_loss), TD3_OFF(loss_stride),
    TD3_OFF(work), TD3_OFF(work_bytes)};
#undef TD3_OFF
  return td3_layout_out(v, out, capacity);
}

int serl_td3_train(serl_ctx *c, const serl_td3_desc *d, void *stream) { return td3_train(c, d, stream, {"serl_td3_train", TD3_TABLES}); }

int serl_td3_train_mfma(serl_ctx *c, const serl_td3_desc *d, void *stream)
{
  Td3Call call = {"serl_td3_train_mfma", TD3_TABLES};
  call.mfma = true;
  return td3_train(c, d, stream, call);
}

int serl_td3_rng_layout(int32_t *out, int32_t capacity)
{
#define TD3_OFF(m) (int32_t)offsetof(serl_td3_rng_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_td3_rng_desc), TD3_OFF(seed), TD3_OFF(n_rows), TD3_OFF(learner0), TD3_OFF(dense), TD3_OFF(caps)};
#undef TD3_OFF
  return td3_layout_out(v, out, capacity);
}

int serl_td3_train_rng(serl_ctx *c, const serl_td3_desc *d, const serl_td3_rng_desc *rg, void *stream)
{
  return td3_train(c, d, stream, {"serl_td3_train_rng", TD3_GENERATOR, rg});
}

int serl_td3_group_layout(int32_t *out, int32_t capacity)
{
#define TD3_OFF(m) (int32_t)offsetof(serl_td3_learner_row, m)
#define TD3_GOFF(m) (int32_t)offsetof(serl_td3_group_desc, m)
  const int32_t v[] = {
    (int32_t)sizeof(serl_td3_learner_row),
    TD3_OFF(ring), TD3_OFF(seed), TD3_OFF(capacity), TD3_OFF(n_rows), TD3_OFF(n_updates), TD3_OFF(iteration0), TD3_OFF(key),
    TD3_OFF(policy_update_freq), TD3_OFF(update_actor_target), TD3_OFF(pad0), TD3_OFF(lr), TD3_OFF(gamma), TD3_OFF(tau), TD3_OFF(noise_sd),
    TD3_OFF(noise_clip), TD3_OFF(lambda_s), TD3_OFF(lambda_t), TD3_OFF(eps_sd),
    (int32_t)sizeof(serl_td3_group_desc), TD3_GOFF(rows), TD3_GOFF(status), TD3_GOFF(dense), TD3_GOFF(caps)};
#undef TD3_OFF
#undef TD3_GOFF
  return td3_layout_out(v, out, capacity);
}

int serl_td3_train_group(serl_ctx *c, const serl_td3_desc *d, const serl_td3_group_desc *gd, void *stream)
{
  return td3_train(c, d, stream, {"serl_td3_train_group", TD3_GROUP, nullptr, gd});
}

int serl_td3_train_group_big(serl_ctx *c, const serl_td3_desc *d, const serl_td3_group_desc *gd, void *stream)
{
  Td3Call call = {"serl_td3_train_group_big", TD3_GROUP, nullptr, gd};
  call.big = true;
  return td3_train(c, d, stream, call);
}

int serl_td3_train_group_wide(serl_ctx *c, const serl_td3_desc *d, const serl_td3_group_desc *gd, void *stream)
{
  Td3Call call = {"serl_td3_train_group_wide", TD3_GROUP, nullptr, gd};
  call.big = true; call.wide = true;
  return td3_train(c, d, stream, call);
}

int serl_td3_rng_fill(serl_ctx *c, const serl_td3_rng_desc *rg, int32_t learner, int32_t state_dim, int32_t action_dim, int32_t batch,
                      int32_t iteration0, int32_t n_updates, int32_t policy_update_freq, int32_t *slots, float *target_noise, float *caps_noise,
                      void *stream)
{
  return td3_rng_fill(c, rg, learner, state_dim, action_dim, batch, iteration0, n_updates, policy_update_freq, slots, target_noise, caps_noise, stream,
                      false, "serl_td3_rng_fill");
}

int serl_td3_rng_fill_big(serl_ctx *c, const serl_td3_rng_desc *rg, int32_t learner, int32_t state_dim, int32_t action_dim, int32_t batch,
                          int32_t iteration0, int32_t n_updates, int32_t policy_update_freq, int32_t *slots, float *target_noise, float *caps_noise,
                          void *stream)
{
  return td3_rng_fill(c, rg, learner, state_dim, action_dim, batch, iteration0, n_updates, policy_update_freq, slots, target_noise, caps_noise, stream,
                      true, "serl_td3_rng_fill_big");
}

int64_t serl_td3_big_work_bytes(int32_t n_learners, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t batch)
{
  if (n_learners < 1 || !serl_learner_range(state_dim, action_dim, hidden, num_layers, batch, BIG_B)) return 0;
  return (int64_t)n_learners * td3_work_floats(state_dim, action_dim, hidden, num_layers, (batch + BP - 1) / BP) * (int64_t)sizeof(float);
}

int serl_td3_big_layout(int32_t *out, int32_t capacity)
{
#define TD3_OFF(m) (int32_t)offsetof(serl_td3_big_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_td3_big_desc), TD3_OFF(rng), TD3_OFF(dense), TD3_OFF(pad0)};
#undef TD3_OFF
  return td3_layout_out(v, out, capacity);
}

int serl_td3_train_big(serl_ctx *c, const serl_td3_desc *d, const serl_td3_big_desc *bd, void *stream)
{
  if (!bd) return serl_fail(SERL_E_INVALID, "serl_td3_train_big: NULL big descriptor");
  if (bd->dense != 0 && bd->dense != 1) return serl_fail(SERL_E_INVALID, "serl_td3_train_big: dense must be 0 (valu) or 1 (mfma)");
  Td3Call call = {"serl_td3_train_big", bd->rng ? TD3_GENERATOR : TD3_TABLES, bd->rng};
  call.mfma = bd->dense == 1; call.big = true;
  return td3_train(c, d, stream, call);
}

int64_t serl_td3_wide_work_bytes(int32_t n_learners, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t batch)
{
  const int64_t big = serl_td3_big_work_bytes(n_learners, state_dim, action_dim, hidden, num_layers, batch);
  if (big == 0) return 0;
  const int chunks = (batch + BP - 1) / BP;
  return big + (int64_t)n_learners * (chunks * wide_chunk_floats(state_dim, action_dim, hidden, num_layers) + WIDE_SYNC_WORDS) * (int64_t)sizeof(float);
}

int serl_td3_wide_layout(int32_t *out, int32_t capacity)
{
#define TD3_OFF(m) (int32_t)offsetof(serl_td3_wide_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_td3_wide_desc), TD3_OFF(rng), TD3_OFF(status), TD3_OFF(dense), TD3_OFF(pad0)};
#undef TD3_OFF
  return td3_layout_out(v, out, capacity);
}

int serl_td3_train_wide(serl_ctx *c, const serl_td3_desc *d, const serl_td3_wide_desc *wd, void *stream)
{
  if (!wd) return serl_fail(SERL_E_INVALID, "serl_td3_train_wide: NULL wide descriptor");
  if (wd->dense != 0 && wd->dense != 1) return serl_fail(SERL_E_INVALID, "serl_td3_train_wide: dense must be 0 (valu) or 1 (mfma)");
  if (!wd->status) return serl_fail(SERL_E_INVALID, "serl_td3_train_wide: NULL status");
  Td3Call call = {"serl_td3_train_wide", wd->rng ? TD3_GENERATOR : TD3_TABLES, wd->rng};
  call.mfma = wd->dense == 1; call.big = true; call.wide = true; call.status = wd->status;
  return td3_train(c, d, stream, call);
}

int64_t serl_ga_distill_general_work_bytes(int32_t n_pairs, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers)
{
  if (n_pairs < 1 || !serl_learner_range(state_dim, action_dim, hidden, num_layers, 1, BP)) return 0;
  return (int64_t)n_pairs * distill_g_work_floats(state_dim, action_dim, hidden, num_layers) * (int64_t)sizeof(float);
}

int serl_ga_distill_general(serl_ctx *c, float *child, int64_t stride, int32_t n_pairs, int32_t state_dim, int32_t hidden, int32_t num_layers,
                            int32_t action_dim, int32_t activation, const float *states, const float *targets, const float *keep, int32_t rows,
                            const int32_t *slots, int32_t steps, const int32_t *n_steps, const int32_t *batch, float lr, void *work,
                            int64_t work_bytes, int32_t dense, void *stream)
{
  return distill_general(c, child, stride, n_pairs, state_dim, hidden, num_layers, action_dim, activation, states, targets, keep, rows, slots, steps,
                         n_steps, batch, lr, work, work_bytes, dense, stream);
}

int serl_host_td3_slots(uint64_t seed, int32_t learner, int32_t iteration, int32_t n_rows, int32_t batch, int32_t *out)
{
  if (!out || batch < 1 || n_rows < batch) return serl_fail(SERL_E_INVALID, "serl_host_td3_slots: NULL out, batch < 1 or n_rows < batch");
  serl_td3_slots_serial(seed, learner, iteration, n_rows, batch, out);
  return SERL_OK;
}

}  // extern "C"

// serl_shapes.h -- WHICH actor shapes each kernel runs: one predicate per kernel contract over (S, A, H, L, activation, batch), pure host
// functions like serl_plan.h.  No HIP: every entry point refuses through its predicate (serl_refuse, serl_ctx.h), serl_shape_query
// (include/serl_amd.h) hands the same answer to callers and tests without a device.  A predicate answers for the range and says what LDS a
// workgroup of the kernel takes for the shape; serl_shape_fit holds that against the LDS at hand, where the entry point reads its context.
// The LDS footprints stand next to the ranges they belong to.
#pragma once
#include <stdint.h>
#include "../../include/serl_amd.h"
#include "serl_plan.h"

// why (enum serl_shape_why): takes, or outside the compiled range, or in range and too large for the LDS at hand.  A refusal carries the entry
// point's return code and what follows the entry point's name in serl_last_error.
struct SerlShape {
  int32_t why, code;
  const char *text;
  int64_t lds_bytes;                // in range: the dynamic LDS of a workgroup (0: the kernel asks for none) ...
  const char *lds_text;             // ... and the text of the refusal where that is more than there is
};

static inline SerlShape serl_shape_takes(int64_t lds_bytes, const char *lds_text) { return SerlShape{SERL_SHAPE_WHY_TAKES, SERL_OK, "", lds_bytes, lds_text}; }
static inline SerlShape serl_shape_range(int32_t code, const char *text) { return SerlShape{SERL_SHAPE_WHY_RANGE, code, text, 0, ""}; }
static inline SerlShape serl_shape_fit(SerlShape v, int64_t lds)
{
  if (v.why == SERL_SHAPE_WHY_TAKES && v.lds_bytes > lds) { v.why = SERL_SHAPE_WHY_LDS; v.code = SERL_E_UNSUPPORTED; v.text = v.lds_text; }
  return v;
}
static inline bool serl_shape_act_ok(int act) { return act >= SERL_ACT_TANH && act <= SERL_ACT_LEAKY_RELU; }

// ---- serl_ga_sensitivity / serl_ga_novelty (serl_ga.hip): one sample at a time, the forward buffers (FwdBuf) in LDS ----------------------
// floats of the forward buffers; within the range at most 12 928 (51 712 bytes, at 64 -> 256 x 16 -> 16): serl_ga_novelty, which holds
// nothing else, is refused for LDS on no device with the 64 KB per workgroup every device has
static inline int64_t serl_ga_fwd_floats(int S, int A, int H, int L) { return S + 2 * (int64_t)(L + 1) * H + (int64_t)L * H + L + 2 * A + 16; }
static inline int64_t serl_ga_genome_floats(int S, int A, int H, int L) { return (int64_t)H * S + (int64_t)L * H * H + (int64_t)A * H; }

// genome: serl_ga_sensitivity, which holds one output's gradient of the whole genome besides (~208 KB at 128 x 3)
static inline SerlShape serl_shape_ga(bool genome, int S, int A, int H, int L, int act, int batch)
{
  if (batch <= 0) return serl_shape_range(SERL_E_INVALID, ": bad argument");
  if (S < 1 || S > 64 || A < 1 || A > 16 || H < 2 || H > 256 || L < 0 || L > 16 || !serl_shape_act_ok(act))
    return serl_shape_range(SERL_E_UNSUPPORTED, ": network shape out of range");
  return serl_shape_takes(4 * (serl_ga_fwd_floats(S, A, H, L) + (genome ? serl_ga_genome_floats(S, A, H, L) + 2 * (int64_t)H : 0)),
                          ": network too large for the LDS-resident accumulators");
}

// ---- serl_ga_distill (serl_distill.hip): hidden 32 x 3, the training state in LDS ------------------------------------------------------
#define SERL_DISTILL_THREADS 128      // (serl_distill.hip DB) threads per workgroup = the largest minibatch
#define SERL_DISTILL_MAX_S 16         // (serl_distill.hip DS_MAX) observations of the widest env configuration

static inline SerlShape serl_shape_ga_distill(int S, int A, int H, int L, int act)
{
  if (H != 32 || L != 3 || S < 1 || S > SERL_DISTILL_MAX_S || A < 1 || A > 4 || !serl_shape_act_ok(act))
    return serl_shape_range(SERL_E_UNSUPPORTED, ": compiled for the SERL50 actor family (hidden 32, 3 hidden layers); other shapes train in PyTorch");
  // parameters, Adam moments and gradient (4 x P rounded up to 4), and (L + 3) activation rows of H per thread: ~158 KB
  const int64_t P = serl_plan_param_count(S, H, L, A);
  return serl_shape_takes(4 * (4 * ((P + 3) & ~(int64_t)3) + (int64_t)(L + 3) * H * SERL_DISTILL_THREADS),
                          ": the training state does not fit this device's LDS per workgroup; the caller trains pair by pair in PyTorch");
}

// ---- the learner shape (serl_td3_core.inc): serl_td3_train* and the kernels built from its phases ---------------------------------------
#define SERL_LEARNER_THREADS 512      // (serl_td3_core.inc NT)
#define SERL_LEARNER_BP 128           // (BP) samples of a chunk = the largest minibatch but for the chunked flavours
#define SERL_LEARNER_BIG_B 512        // (BIG_B) the largest minibatch of the chunked flavours and of the GA kernels
#define SERL_LEARNER_LP 132           // (LP) floats per row of an LDS tile
#define SERL_LEARNER_TILE_ROWS 128    // (TILE_ROWS) the widest layer

static inline bool serl_learner_range(int S, int A, int H, int L, int B, int max_batch)
{
  return H >= 4 && H <= SERL_LEARNER_TILE_ROWS && H % 4 == 0 && L >= 0 && L <= 4 && S >= 1 && S <= 16 && A >= 1 && A <= 4 && B >= 1 && B <= max_batch;
}
// two activation tiles, the reduction arrays and, with the in-kernel generator, the minibatch's slots (slot_rows: BP or BIG_B; 0 with tables): ~135 KB
static inline SerlShape serl_shape_learner_takes(int slot_rows)
{
  return serl_shape_takes(4 * ((int64_t)2 * SERL_LEARNER_TILE_ROWS * SERL_LEARNER_LP + SERL_LEARNER_THREADS + 64 + SERL_LEARNER_BP + slot_rows),
                          ": the activation tiles do not fit this device's LDS per workgroup");
}
#define SERL_LEARNER_RANGE_TEXT ": compiled for hidden a multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, state_dim 1 .. 16, action_dim 1 .. 4, "

// serl_td3_train and its flavours; big: minibatches of up to 512 rows
static inline SerlShape serl_shape_td3(int S, int A, int H, int L, int act, int B, bool big, int slot_rows)
{
  if (S < 1 || A < 1 || H < 1 || L < 0 || B < 1 || !serl_shape_act_ok(act))
    return serl_shape_range(SERL_E_INVALID, ": network shape / minibatch / activation");
  if (!serl_learner_range(S, A, H, L, B, big ? SERL_LEARNER_BIG_B : SERL_LEARNER_BP))
    return serl_shape_range(SERL_E_UNSUPPORTED, big ? SERL_LEARNER_RANGE_TEXT "minibatches of 1 .. 512 rows; other shapes train in PyTorch"
                                                    : SERL_LEARNER_RANGE_TEXT "minibatches of 1 .. 128 rows; other shapes train in PyTorch");
  return serl_shape_learner_takes(slot_rows);
}

// the GA kernels on the learner's actor: serl_ga_sensitivity_general and serl_ga_novelty_general (batched: minibatches of 1 .. 512 rows),
// serl_ga_distill_general (its minibatches are the caller's tables)
static inline SerlShape serl_shape_learner_actor(bool batched, int S, int A, int H, int L, int act, int B)
{
  if (!serl_learner_range(S, A, H, L, batched ? B : 1, SERL_LEARNER_BIG_B) || !serl_shape_act_ok(act))
    return serl_shape_range(SERL_E_UNSUPPORTED, batched ? SERL_LEARNER_RANGE_TEXT "the three activations, minibatches of 1 .. 512 rows"
                                                        : SERL_LEARNER_RANGE_TEXT "the three activations");
  return serl_shape_learner_takes(0);
}

// ---- the env rollout kernels (serl_venv_rollout*; serl_capi.hip): no dynamic LDS, and in place of a minibatch the env ------------------
// env_config + 3 x (incremental control), -1 for an unknown env_config
static inline int serl_shape_env(int env_config, int incremental) { return env_config < 0 || env_config > 2 ? -1 : env_config + 3 * (incremental != 0); }

// serl_venv_rollout: the lane actor's shape (lane_actor.h serl_lane_actor_ok) on the attitude task without rate control
static inline SerlShape serl_shape_venv_lane32(int S, int A, int H, int L, int act, int env)
{
  if (env != serl_shape_env(SERL_ENV_ATTITUDE, 0))
    return serl_shape_range(SERL_E_INVALID, ": the attitude task without rate control only (env_config SERL_ENV_ATTITUDE, incremental 0)");
  if (H != 32 || S != 7 || A != 3)
    return serl_shape_range(SERL_E_INVALID, ": the in-kernel actor is 7 -> 32 .. -> 3 only (hidden 32, state_dim 7, action_dim 3)");
  if (L < 0) return serl_shape_range(SERL_E_INVALID, ": num_layers < 0");
  if (!serl_shape_act_ok(act)) return serl_shape_range(SERL_E_INVALID, ": unknown activation");
  return serl_shape_takes(0, "");
}

// serl_venv_rollout_general and serl_venv_rollout_wave: every env configuration, an actor that fits it
static inline SerlShape serl_shape_venv_general(int S, int A, int H, int L, int act, int env)
{
  if (env < 0 || env > 5)
    return serl_shape_range(SERL_E_INVALID, ": env_config must be SERL_ENV_ATTITUDE, SERL_ENV_SYMMETRIC or SERL_ENV_FULL");
  if (S != serl_plan_env_state_dim(env % 3, env / 3) || A != serl_plan_env_action_dim(env % 3))
    return serl_shape_range(SERL_E_INVALID, ": the actor's state_dim / action_dim do not match the env configuration (attitude 7 / 3, symmetric 2 / 1, full 13 / 3; incremental adds action_dim observations)");
  if (H < 4 || H > SERL_PLAN_MAX_HIDDEN || H % 4 != 0) return serl_shape_range(SERL_E_UNSUPPORTED, ": hidden must be a multiple of 4 in 4 .. 128");
  if (L < 0 || L > 16) return serl_shape_range(SERL_E_UNSUPPORTED, ": num_layers must be 0 .. 16");
  if (!serl_shape_act_ok(act)) return serl_shape_range(SERL_E_INVALID, ": unknown activation");
  return serl_shape_takes(0, "");
}

// ---- by enum serl_shape_kernel (serl_shape_query): the entry point's name, and its predicate -------------------------------------------
static inline const char *serl_shape_who(int kernel)
{
  static const char *const who[SERL_SHAPE_KERNELS] = {
    "serl_ga_sensitivity", "serl_ga_novelty", "serl_ga_distill", "serl_td3_train", "serl_td3_train_big", "serl_ga_sensitivity_general",
    "serl_ga_novelty_general", "serl_ga_distill_general", "serl_venv_rollout", "serl_venv_rollout_general"};
  return kernel >= 0 && kernel < SERL_SHAPE_KERNELS ? who[kernel] : nullptr;
}

static inline SerlShape serl_shape_of(int kernel, int S, int A, int H, int L, int act, int batch)
{
  switch (kernel) {
    case SERL_SHAPE_GA_SENSITIVITY: return serl_shape_ga(true, S, A, H, L, act, batch);
    case SERL_SHAPE_GA_NOVELTY: return serl_shape_ga(false, S, A, H, L, act, batch);
    case SERL_SHAPE_GA_DISTILL: return serl_shape_ga_distill(S, A, H, L, act);
    case SERL_SHAPE_TD3_TRAIN: return serl_shape_td3(S, A, H, L, act, batch, false, 0);
    case SERL_SHAPE_TD3_TRAIN_BIG: return serl_shape_td3(S, A, H, L, act, batch, true, 0);
    case SERL_SHAPE_GA_SENSITIVITY_GENERAL:
      if (batch <= 0) return serl_shape_range(SERL_E_INVALID, ": bad argument");
      return serl_shape_learner_actor(true, S, A, H, L, act, batch);
    case SERL_SHAPE_GA_NOVELTY_GENERAL: return serl_shape_learner_actor(true, S, A, H, L, act, batch);
    case SERL_SHAPE_GA_DISTILL_GENERAL: return serl_shape_learner_actor(false, S, A, H, L, act, batch);
    case SERL_SHAPE_VENV_ROLLOUT: return serl_shape_venv_lane32(S, A, H, L, act, batch);
    case SERL_SHAPE_VENV_ROLLOUT_GENERAL: return serl_shape_venv_general(S, A, H, L, act, batch);
  }
  return serl_shape_range(SERL_E_INVALID, ": unknown kernel");
}

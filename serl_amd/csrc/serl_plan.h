// serl_plan.h -- WHICH kernel family a rollout call runs on and with what launch shape: pure host functions of the device's capabilities and the
// descriptor.  No HIP: serl_capi.hip carries a plan out (serl_execute_plan), the serl_host_plan_* exports hand it to tests at any CU count.
#pragma once
#include <stdint.h>
#include "../../include/serl_amd.h"

#define SERL_PLAN_MAX_HIDDEN 128      // (rollout_device.h SERL_MAX_HIDDEN)
#define SERL_PLAN_MAIL_BYTES 256      // (rollout_device.h sizeof(SerlMail))
#define SERL_PLAN_MIXED_MAX 4         // (serl_mixed.h SERL_MIXED_MAX)

// what the decision reads from the context
struct SerlCaps {
  int32_t num_cus;                  // multiProcessorCount of the context's device
  // environment overrides, read once when the context is made (-1 = not set)
  int32_t env_kernel;               // serl_kernel_hint from SERL_KERNEL
  int32_t env_waves_per_block;      // SERL_WAVES_PER_BLOCK
  int32_t env_laneq_waves;          // SERL_LANEQ_WAVES: cap on the wavefronts of a SERL_KERNEL_LANEQ launch (default 4 x CUs)
  int32_t env_split_actor;          // SERL_SPLIT_ACTOR=1: streamed actors of one-episode teams (hidden > 64) on TWO actor wavefronts that share the forward pass
                                    // (family_teams2.hip; measured slower than one wavefront with the specialised forward: profiles/r04_experiments.md)
  int32_t env_remote_actor;         // SERL_REMOTE_ACTOR=0: streamed actors of one-episode teams stay on the team's CU (family_team.hip serl_rollout_teams_kernel_; A/B)
  int32_t env_lane_regroup;         // SERL_LANE_WEIGHTS=rows: the lane-per-episode kernels walk [members][P] rows instead of the regrouped copy (A/B)
};
static inline SerlCaps serl_default_caps(void) { return SerlCaps{256, SERL_KERNEL_AUTO, -1, -1, 0, 1, 1}; }

// everything an executor needs and everything serl_last_rollout_info records
struct SerlPlan {
  int32_t status;                   // SERL_OK, or the refusal the plan makes ...
  const char *message;              // ... and its (static) text
  int32_t family;                   // enum serl_kernel_family
  int32_t laneq;                    // family LANE: the kernel behind the work queue (kernel_hint LANEQ), whether or not the queue is engaged
  int32_t grid, block;              // workgroups (of the LAST launch), threads per workgroup
  int32_t lanes;                    // RolloutArgs.lanes: active lanes per wavefront
  int32_t per_team;                 // episodes per team (family LANE: per wavefront)
  int32_t queue, q0;                // a work-queue counter is taken; RolloutArgs.q0: the first queued episode (the episode count without a queue, 0 for kernels without one)
  int32_t regroup;                  // the weights are regrouped in front of the launch
  int32_t mailbox, mail_bytes;      // a mailbox region is taken; bytes of it zeroed
  int32_t timed;                    // the context's timing events are recorded
  int32_t actor_waves, streamed;
  int32_t launches, chunk;          // launch i runs the episodes [i * chunk, min((i + 1) * chunk, n_episodes)); with more than one launch, one workgroup per episode of the chunk
};

static inline SerlPlan serl_plan_refuse(SerlPlan p, const char *message)
{
  p.status = SERL_E_UNSUPPORTED; p.message = message;
  return p;
}

// one launch of `grid` workgroups of `wpb` wavefronts for all n_episodes, no queue
static inline SerlPlan serl_plan_one(int timed, int n_episodes, int family, int grid, int wpb, int lanes, int per_team, int actor_waves, int streamed)
{
  SerlPlan p = {};
  p.status = SERL_OK; p.message = "";
  p.family = family; p.grid = grid; p.block = 64 * wpb; p.lanes = lanes; p.per_team = per_team;
  p.timed = timed; p.actor_waves = actor_waves; p.streamed = streamed;
  p.launches = 1; p.chunk = n_episodes;
  return p;
}

// ... of a kernel with a work queue: the episodes beyond the `slots` the launch starts on wait in it
static inline void serl_plan_queue(SerlPlan &p, int n_episodes, long long slots)
{
  p.queue = n_episodes > slots;
  p.q0 = p.queue ? (int32_t)slots : n_episodes;
}

// envs/phlabenv.py:84-97 (obs_idx per configuration), :213-220 (n_obs)
static inline int serl_plan_env_action_dim(int env_config) { return env_config == SERL_ENV_SYMMETRIC ? 1 : 3; }
static inline int serl_plan_env_state_dim(int env_config, int incremental)
{
  if (env_config < 0 || env_config > 2) return 0;
  const int A = serl_plan_env_action_dim(env_config);
  const int nx = env_config == SERL_ENV_ATTITUDE ? 4 : (env_config == SERL_ENV_SYMMETRIC ? 1 : 10);
  return A + nx + (incremental ? A : 0);
}
static inline int serl_plan_param_count(int S, int H, int L, int A) { return H * S + H + L * (H * H + 3 * H) + A * H + A; }
static inline bool serl_plan_general_env(const serl_rollout_desc *d) { return d->env_config != SERL_ENV_ATTITUDE || d->incremental != 0; }

// Episodes per team, 0 = use another kernel.  Measured per env step: 21.6 us with one episode per team, 22.2 with two,
// 25.6 with four (the scalar glue is paid once for all lane groups; only the lane-parallel passes multiply, and the team's
// helpers share them), and one team fits a CU -- so up to 2 x CUs episodes run two per team and up to 4 x CUs four per team,
// in ONE round of workgroups, against 57 us of the one-wavefront kernel (1 023 episodes: 39.2 M env-steps/s against 16).
// H = 32 only.  kernel_hint SERL_KERNEL_TEAM2 / TEAM4 force it.
static inline int serl_use_teamg(const SerlCaps *c, const serl_rollout_desc *d, int hint, int episodes)
{
  if (d->hidden != 32) {
    // actors without one hidden row per lane (SERL10's 72, the TD3 actor's 96): the actor wavefront runs the episodes' forward
    // passes one after the other -- two per team (~33 us per env step for the pair, actor-bound) beat one wavefront per episode
    // (57 - 61 us) while every pair has a CU: CUs < episodes <= 2 x CUs; four per team would be slower than four lone wavefronts
    if (hint == SERL_KERNEL_TEAM2) return 2;
    if (hint != SERL_KERNEL_AUTO) return 0;
    return (episodes > c->num_cus && episodes <= 2 * c->num_cus) ? 2 : 0;
  }
  if (hint == SERL_KERNEL_TEAM2) return 2;
  if (hint == SERL_KERNEL_TEAM4) return 4;
  if (hint != SERL_KERNEL_AUTO) return 0;
  if (episodes <= c->num_cus || episodes > 4 * c->num_cus) return 0;
  return episodes <= 2 * c->num_cus ? 2 : 4;
}

// Beyond 4 x CUs episodes the team kernels still win when the launch has the GPU to itself: 4 x CUs episodes per 30.8 us
// is the rate of the two-episodes-per-wavefront kernel (8 x CUs per 62.9 us) at half the granularity, and the remainder runs
// at the rate of its own size class.  Side-by-side launches (concurrent_episodes > 0) split the CUs by episode share (below; a
// team needs a whole CU).  H = 32 only; any kernel_hint other than AUTO switches it off.
static inline bool serl_use_team_rounds(const SerlCaps *c, const serl_rollout_desc *d, int hint, int episodes)
{
  if (d->hidden != 32 || hint != SERL_KERNEL_AUTO) return false;
  return episodes > 4 * c->num_cus;
}

// The one-wavefront-per-episode kernel runs up to 4 x CUs episodes at once (one per SIMD); beyond that the launch needs a
// second round of wavefronts, and packing two episodes into a wavefront (1.1 x the time per env step) is the better deal.
// H = 32 only (the lane group of an episode holds one hidden row per lane).  kernel_hint SERL_KERNEL_HALF forces it.
static inline bool serl_use_half(const SerlCaps *c, const serl_rollout_desc *d, int hint, int episodes)
{
  if (d->hidden != 32) return false;
  if (hint != SERL_KERNEL_AUTO) return hint == SERL_KERNEL_HALF;
  return episodes > 4 * c->num_cus;
}

// One episode per workgroup and one workgroup per CU (the LDS copy of the tables): a team finishes an env step in
// ~0.37 of the time a lone wavefront needs (21.2 vs 57 us), but only one team fits a CU where four lone wavefronts
// would: teams while every episode gets a CU of its own (measured: 320 episodes as teams 88 us, 400 alone 59 us),
// lone wavefronts beyond.  kernel_hint SERL_KERNEL_TEAM forces it (any other hint excludes it).
static inline bool serl_use_team(const SerlCaps *c, int hint, int episodes)
{
  if (hint != SERL_KERNEL_AUTO) return hint == SERL_KERNEL_TEAM;
  return episodes <= c->num_cus;
}

// (rollout_device.h: serl_lds_actor_ok) the actor shape whose weights live in LDS for the episode
static inline bool serl_lds_actor_shape(const serl_rollout_desc &d) { return d.hidden == 32 && d.num_layers <= 3 && d.state_dim == 7 && d.action_dim == 3; }

// (lane_actor.h serl_lane_actor_ok) the actor shape the lane-per-episode kernels read from the regrouped copy of the weights
static inline bool serl_lane_regroup_shape(const SerlCaps *c, const serl_rollout_desc *d)
{
  return c->env_lane_regroup && d->hidden == 32 && d->state_dim == 7 && d->action_dim == 3 && d->n_members <= (1 << 22);
}

// Round 6: streamed actors (hidden 65 .. 128: SERL10's 72, the TD3 actor's 96) of the attitude task with the actor in a workgroup of its own on another CU
// (family_teamr.hip): two workgroups per episode, pairs (b, b + 8) of a group of sixteen.  Only while every workgroup of the launch -- and of the launches it
// was told about -- can be resident at once: a team spins on its partner's mailbox.  0 = not eligible, else the grid.
static inline int serl_remote_actor_grid(const SerlCaps *c, const serl_rollout_desc *d, int together)
{
  if (!c->env_remote_actor || (d->hidden != 72 && d->hidden != 96 && d->hidden != 128) || d->state_dim != 7 || d->action_dim != 3) return 0;      // (rollout_device.h serl_cu_actor_ok)
  const int grid = 16 * ((d->n_episodes + 7) / 8), all = 16 * ((together + 7) / 8);
  return all <= c->num_cus ? grid : 0;
}

// Wavefronts per workgroup of the wave-cooperative kernels: one per CU while there are no more episodes than CUs,
// then up to four (one per SIMD) sharing the workgroup's LDS copy of the tables.
static inline int serl_wave_kernel_waves_per_block(const SerlCaps *c, int episodes)
{
  if (c->env_waves_per_block >= 1 && c->env_waves_per_block <= 8) return c->env_waves_per_block;     // (8 only with a library built with -DCITW_MAX_WAVES=8)
  int w = (episodes + c->num_cus - 1) / c->num_cus;
  return w < 1 ? 1 : (w > 4 ? 4 : w);
}

// Wavefronts per workgroup.  One workgroup stages one LDS copy of the tables (94 KiB of the CU's 160 KiB), so
// only one workgroup fits a CU: while there are no more wavefronts than CUs each gets a CU of its own (the
// code streams through the instruction cache and co-resident waves slow each other down); beyond that, waves
// share a CU four at a time (one per SIMD, each with the full 512-register budget).
static inline int serl_waves_per_block(const SerlCaps *c, int waves)
{
  if (c->env_waves_per_block >= 1 && c->env_waves_per_block <= 4) return c->env_waves_per_block;
  return waves <= c->num_cus ? 1 : 4;
}

// descriptor hint first, then the context's development override (SERL_KERNEL, read once by serl_ctx_create)
static inline int serl_resolve_hint(const SerlCaps *c, int desc_hint) { return desc_hint != SERL_KERNEL_AUTO ? desc_hint : c->env_kernel; }

// The argument checks of serl_rollout / serl_rollout_multi that read no context state but the overrides (serl_check_desc runs them behind its own);
// *hint_out = the resolved kernel hint, *message = the text of a refusal.
static inline int serl_plan_check(const SerlCaps *c, const serl_rollout_desc *d, int *hint_out, const char **message)
{
#define SERL_PLAN_FAIL(code, text) return (*message = (text), (code))
  const bool general_env = serl_plan_general_env(d);
  if (serl_resolve_hint(c, d->kernel_hint) == SERL_KERNEL_LANEG) {
    // the limits of the lane kernel around the general lane actor (family_laneg.hip; lane_actor.h serl_actor_forward_lane_general), each by its name,
    // in front of every other check: nothing is planned for a call the hint refuses
    if (d->env_config != SERL_ENV_ATTITUDE)
      SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: kernel_hint LANEG: env_config must be SERL_ENV_ATTITUDE (the lane-per-episode kernels exist for the attitude task only)");
    if (d->incremental != 0)
      SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: kernel_hint LANEG: incremental must be 0 (the lane-per-episode kernels exist for the attitude task only)");
    if (d->state_dim != 7 || d->action_dim != 3)
      SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: kernel_hint LANEG: state_dim must be 7 and action_dim 3");
    if (d->hidden % 4 != 0 || d->hidden < 4 || d->hidden > SERL_PLAN_MAX_HIDDEN)
      SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: kernel_hint LANEG: hidden must be a multiple of 4 in 4 .. 128");
    if (d->num_layers < 0 || d->num_layers > 16)
      SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: kernel_hint LANEG: num_layers must be 0 .. 16");
  }
  if (serl_plan_env_state_dim(d->env_config, d->incremental) == 0)
    SERL_PLAN_FAIL(SERL_E_INVALID, "serl_rollout: env_config must be SERL_ENV_ATTITUDE, SERL_ENV_SYMMETRIC or SERL_ENV_FULL");
  if (d->state_dim != serl_plan_env_state_dim(d->env_config, d->incremental) || d->action_dim != serl_plan_env_action_dim(d->env_config))
    SERL_PLAN_FAIL(SERL_E_INVALID, "serl_rollout: state_dim / action_dim do not match the env configuration (attitude 7 / 3, symmetric 2 / 1, full 13 / 3; incremental adds action_dim observations)");
  if (general_env && (d->lanes_per_wave > 0 || serl_resolve_hint(c, d->kernel_hint) == SERL_KERNEL_LANEQ))
    SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: the lane-per-episode kernels exist for the attitude task only");
  if (d->hidden < 2 || d->hidden > SERL_PLAN_MAX_HIDDEN || d->num_layers < 0 || d->num_layers > 16)
    SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: hidden size / layer count out of range");
  if (d->hidden % 4 != 0 || d->weight_stride % 4 != 0 || ((uintptr_t)d->weights & 15) != 0)
    SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: hidden size and weight_stride must be multiples of 4 and weights 16-byte aligned (dwordx4 row loads)");
  if (d->activation < 0 || d->activation > 2) SERL_PLAN_FAIL(SERL_E_INVALID, "serl_rollout: activation");
  if (d->weight_stride < serl_plan_param_count(d->state_dim, d->hidden, d->num_layers, d->action_dim))
    SERL_PLAN_FAIL(SERL_E_INVALID, "serl_rollout: weight_stride smaller than the parameter count");
  if (d->max_steps <= 0) SERL_PLAN_FAIL(SERL_E_INVALID, "serl_rollout: max_steps");
  if (d->kernel_hint < SERL_KERNEL_AUTO || d->kernel_hint > SERL_KERNEL_LANEG) SERL_PLAN_FAIL(SERL_E_INVALID, "serl_rollout: kernel_hint");
  // (LANEQ and LANEG are the hints lanes_per_wave > 0 does not switch off: there it is the lanes per wavefront of the work-queue kernel / of the general lane kernel)
  const int rhint = serl_resolve_hint(c, d->kernel_hint);
  const int hint = (d->lanes_per_wave > 0 && rhint != SERL_KERNEL_LANEQ && rhint != SERL_KERNEL_LANEG) ? SERL_KERNEL_AUTO : rhint;
  if (d->hidden != 32 && (hint == SERL_KERNEL_TEAM4 || hint == SERL_KERNEL_HALF))
    SERL_PLAN_FAIL(SERL_E_UNSUPPORTED, "serl_rollout: kernel_hint TEAM4 / HALF needs hidden = 32 (other shapes: TEAM2, the actor wavefront runs the two episodes one after the other)");
#undef SERL_PLAN_FAIL
  *hint_out = hint;
  *message = "";
  return SERL_OK;
}

// One episode per lane, `lanes` of them per wavefront (rollout_variant.inc): the launch shape of serl_rollout's lanes_per_wave > 0, of the saturating regime
// below and of serl_dyn_open_loop's lane kernel.
static inline SerlPlan serl_plan_lanes(const SerlCaps *c, int timed, int n_episodes, int lanes, int streamed)
{
  if (lanes > 64) lanes = 64;
  const int waves = (n_episodes + lanes - 1) / lanes;
  const int wpb = serl_waves_per_block(c, waves);
  return serl_plan_one(timed, n_episodes, SERL_FAMILY_LANE, (waves + wpb - 1) / wpb, wpb, lanes, lanes, 0, streamed);
}

// serl_rollout (noise == 0) and serl_rollout_noise (noise != 0: the sensor / exploration noise drawn inside the kernels -- the noise instantiations of the
// lane-per-episode kernel (lanes_per_wave > 0, or AUTO where serl_rollout's AUTO runs the lane kernel) and of the one-wavefront-per-episode kernels (everything
// else; the team, half and work-queue kernels have no such instantiation)).  `hint`: serl_plan_check's.
static inline SerlPlan serl_plan_rollout(const SerlCaps *c, const serl_rollout_desc *d, int hint, int noise)
{
  const bool general_env = serl_plan_general_env(d);
  const int n = d->n_episodes;
  int lanes = d->lanes_per_wave;
  // launches that share the GPU with others run on streams of their own: the context's one pair of timing events is
  // not recorded for them (an event in flight on one stream must not be re-recorded on another)
  const int timed = d->concurrent_episodes <= 0;
  const int together = n + (d->concurrent_episodes > 0 ? d->concurrent_episodes : 0);   // episodes sharing the GPU
  if (noise && hint != SERL_KERNEL_AUTO && hint != SERL_KERNEL_WAVE && hint != SERL_KERNEL_LANEG)
    return serl_plan_refuse(SerlPlan{}, "serl_rollout_noise: the TEAM / TEAM2 / TEAM4 / HALF / LANEQ kernels have no noise instantiation (kernel_hint AUTO, WAVE or LANEG, or lanes_per_wave > 0)");
  if (general_env) {
    // observation set / number of actions / incremental control from the descriptor: the team kernel while the episodes fit two
    // rounds of workgroups (2 x ~23 us per env step against 57 of one wavefront per episode), one wavefront per episode beyond
    if (!noise && hint != SERL_KERNEL_AUTO && hint != SERL_KERNEL_TEAM && hint != SERL_KERNEL_WAVE)
      return serl_plan_refuse(SerlPlan{}, "serl_rollout: env configurations other than the attitude task run on the TEAM or WAVE kernels");
    const bool team = hint != SERL_KERNEL_AUTO ? hint == SERL_KERNEL_TEAM : (d->concurrent_episodes <= 0 ? together <= 2 * c->num_cus : together <= c->num_cus);
    if (!noise && team) {      // launches of at most one workgroup per CU, one after the other
      const int launches = (n + c->num_cus - 1) / c->num_cus;
      SerlPlan p = serl_plan_one(timed, n, SERL_FAMILY_TEAMX, n - (launches - 1) * c->num_cus, 8, 1, 1, 1, 1);
      p.launches = launches;
      if (launches > 1) p.chunk = c->num_cus;
      return p;
    }
    const int wpb = serl_wave_kernel_waves_per_block(c, together + (timed ? 0 : 16));
    return serl_plan_one(timed, n, SERL_FAMILY_WAVEX, (n + wpb - 1) / wpb, wpb, 1, 1, 0, 1);
  }
  if (hint == SERL_KERNEL_LANEQ) {
    // One episode per lane behind a work queue (rollout_variant.inc serl_rollout_laneq_kernel_<v>): at most W wavefronts -- four per workgroup, one workgroup per
    // CU, which is what the LDS copy of the tables allows; beside other launches the launch's share of them -- and the episodes beyond their lane slots in the queue.
    lanes = (lanes <= 0 || lanes > 64) ? 64 : lanes;
    long long W = 4LL * c->num_cus;
    if (c->env_laneq_waves >= 1 && c->env_laneq_waves < W) W = c->env_laneq_waves;
    if (d->concurrent_episodes > 0) W = W * n / together;
    W = W < 1 ? 1 : W;
    const int need = (n + lanes - 1) / lanes;
    const int waves = need < W ? need : (int)W;
    const int wpb = serl_waves_per_block(c, waves);
    SerlPlan p = serl_plan_one(timed, n, SERL_FAMILY_LANE, (waves + wpb - 1) / wpb, wpb, lanes, lanes, 0, 1);
    p.laneq = 1;
    p.regroup = serl_lane_regroup_shape(c, d);
    // the lane slots are those of `waves` wavefronts (a last workgroup may hold wavefronts beyond them: their lanes find no episode and leave)
    serl_plan_queue(p, n, (long long)waves * lanes);
    return p;
  }
  if (hint == SERL_KERNEL_LANEG) {
    // One episode per lane, every lane its own actor of any shape over its member's row (family_laneg.hip / family_lanegn.hip: rollout_variant.inc under
    // SERL_LANE_GENERAL_ACTOR): the launch shape of lanes_per_wave > 0 (0 = 64 lanes), no queue, no regrouped copy -- the rows are streamed as they lie.
    // serl_plan_check has refused every shape and env configuration the kernel does not take.
    SerlPlan p = serl_plan_lanes(c, timed, n, (lanes <= 0 || lanes > 64) ? 64 : lanes, 1);
    p.family = SERL_FAMILY_LANEG;
    return p;
  }
  if (!noise && lanes <= 0 && serl_use_team(c, hint, together)) {
    const int rgrid = serl_remote_actor_grid(c, d, together);
    if (rgrid > 0) {
      // mailboxes of this launch: a region of the ring, zeroed on the launch's stream in front of it
      SerlPlan p = serl_plan_one(timed, n, SERL_FAMILY_TEAMR, rgrid, 8, 1, 1, 4, 1);
      p.mailbox = 1; p.mail_bytes = n * SERL_PLAN_MAIL_BYTES;
      return p;
    }
    // (rollout_device.h: serl_lds_actor_ok) shapes whose weights the actor wavefront streams have a kernel of their own
    const bool lds_actor = serl_lds_actor_shape(*d);
    // (development override SERL_SPLIT_ACTOR=1) two actor wavefronts share ONE forward pass beside a six-wavefront team: round 4
    // built it for the shapes whose lone actor wavefront needed a whole step (H = 72: 43 k cycles) -- and then found that a
    // shape-specialised forward (serl_actor_forward_big: 25 k) on ONE wavefront beside the seven-wavefront team is faster
    const bool split = !lds_actor && c->env_split_actor != 0 && d->hidden > 64 && d->hidden <= 128;
    return serl_plan_one(timed, n, lds_actor ? SERL_FAMILY_TEAM : split ? SERL_FAMILY_TEAMS2 : SERL_FAMILY_TEAMS, n, 2, 1, 1, split ? 2 : 1, !lds_actor);
  }
  const int teamg = (!noise && lanes <= 0) ? serl_use_teamg(c, d, hint, together) : 0;
  if (teamg) {
    // (two per team with a streamed actor -- hidden != 32 -- is a kernel of its own: six team wavefronts + two actor wavefronts)
    SerlPlan p = serl_plan_one(timed, n, teamg == 4 ? SERL_FAMILY_TEAM4 : d->hidden != 32 ? SERL_FAMILY_TEAM2S : SERL_FAMILY_TEAM2, (n + teamg - 1) / teamg, 8, 1, teamg,
                               (teamg == 2 && d->hidden != 32) ? 2 : 1, 1 /* the lane-group kernels' actor wavefronts stream the weights */);
    // at most one team per CU; the episodes without a lane group at the start wait in the work queue (rollout_team_half.inc)
    if (p.grid > c->num_cus && d->concurrent_episodes <= 0) p.grid = c->num_cus;
    serl_plan_queue(p, n, (long long)p.grid * teamg);
    return p;
  }
  // Round 6, the saturating regime: from 80 episodes per CU on, one episode per LANE -- 64 per wavefront, the lane's own actor in its registers over
  // the regrouped weights (lane_actor.h serl_actor_forward_lane32_t), at most two tables in flight and hinted index searches in the generated evaluation
  // (tools/dag/codegen_lane.py) -- outruns the queue launch of four-episode teams (episodes x 2 001 steps, M env-steps/s: 16 384: 47.4 against 49.1; 20 480: 53.0
  // against 49.0; 32 768: 82.8; 65 536: 165.6 against 49.6; profiles/r06_saturate.jsonl).  The SERL50 actor shape, nominal / ice code, the attitude task, alone on the GPU.
  if (lanes <= 0 && hint == SERL_KERNEL_AUTO && d->concurrent_episodes <= 0 && d->hidden == 32 && d->state_dim == 7 && d->action_dim == 3 && n >= 80 * c->num_cus)
    lanes = 64;
  if (!noise && lanes <= 0 && serl_use_team_rounds(c, d, hint, together)) {
    // more than 4 x CUs episodes, alone on the GPU: rounds of 4 x CUs episodes (four per team, every CU busy), then the rest
    // with whichever team kernel suits its count -- 4 x CUs + 2 episodes cost 30.8 + 21.6 us per env step, not 62.9
    // ONE launch: a team of four lane groups per CU, the other episodes in the work queue (rollout_team_half.inc) -- a lane group
    // takes the next episode when its own ends, so episodes of different lengths (training: untrained actors crash within
    // seconds) keep every lane group busy instead of rounds that each wait for their longest episode.  (Round 2 ran rounds of
    // 4 x CUs episodes; with equal-length episodes the tail of a queue run costs the four-per-team step where a round of its own
    // could use the two-per-team kernel: 1 536 x 8 001 steps 7 % slower, any mix of lengths faster.)
    // alone on the GPU: a team on every CU.  Beside other launches (a mixed-fault sweep: one launch per dynamics build on streams of
    // their own, each told the episodes of the others) the CUs are split by episode share, so that the teams of all launches are
    // resident together and every launch drains its own queue at the four-per-team rate (round 3 fell back to two episodes per
    // WAVEFRONT here: 24.1 M env-steps/s where the queue kernel gives 33.6 M on the nominal workload)
    int grid = c->num_cus;
    if (d->concurrent_episodes > 0) {
      grid = (int)((long long)c->num_cus * n / together);
      grid = grid < 1 ? 1 : grid;
    }
    if (grid * 4 >= n) grid = (n + 3) / 4;          // (a small share of a large sweep: every episode has a lane group, no queue)
    SerlPlan p = serl_plan_one(timed, n, SERL_FAMILY_TEAM4, grid, 8, 1, 4, 1, 1);
    serl_plan_queue(p, n, 4LL * grid);
    return p;
  }
  if (!noise && lanes <= 0 && serl_use_half(c, d, hint, together)) {
    const int waves = (n + 1) / 2;
    int wpb = (waves + c->num_cus - 1) / c->num_cus;
    wpb = wpb < 1 ? 1 : (wpb > 4 ? 4 : wpb);
    return serl_plan_one(timed, n, SERL_FAMILY_HALF, (waves + wpb - 1) / wpb, wpb, 1, 2, 0, 1);
  }
  if (lanes <= 0) {
    // default: one wavefront per episode (model glue wave-uniform, look-ups / actor rows / ODE5 states per lane)
    // side-by-side launches round their workgroup counts up separately: leave room for a few partial workgroups
    const int wpb = serl_wave_kernel_waves_per_block(c, together + (timed ? 0 : 16));
    return serl_plan_one(timed, n, SERL_FAMILY_WAVE, (n + wpb - 1) / wpb, wpb, 1, 1, 0, 1);
  }
  SerlPlan p = serl_plan_lanes(c, timed, n, lanes, 1);
  p.regroup = serl_lane_regroup_shape(c, d);
  return p;
}

// serl_rollout_regrouped: the LANEG plan with the weights regrouped in front of the launch (family_lanegt.hip / family_lanegtn.hip read the copy; the family
// reported stays SERL_FAMILY_LANEG).  The caller asked for the copy by name, so SERL_LANE_WEIGHTS=rows (caps env_lane_regroup == 0) does not apply.
// `hint`: serl_plan_check's, which has refused every shape and env configuration the LANEG kernels do not take.
#define SERL_PLAN_REGROUP_MAX_MEMBERS (1 << 22)      // (lane_actor.h serl_actor_forward_lane_general_t: the lane's 32-bit byte offset member x 16)
static inline SerlPlan serl_plan_rollout_regrouped(const SerlCaps *c, const serl_rollout_desc *d, int hint, int noise)
{
  if (hint != SERL_KERNEL_LANEG)
    return serl_plan_refuse(SerlPlan{}, "serl_rollout_regrouped: only the LANEG kernels read a regrouped copy through this entry (kernel_hint SERL_KERNEL_LANEG; the hidden-32 lane kernels of lanes_per_wave > 0 regroup on their own)");
  if (d->n_members > SERL_PLAN_REGROUP_MAX_MEMBERS)
    return serl_plan_refuse(SerlPlan{}, "serl_rollout_regrouped: n_members must be at most 1 << 22 = 4 194 304 (a lane addresses its member's 16 bytes of a group with a 32-bit offset)");
  SerlPlan p = serl_plan_rollout(c, d, hint, noise);
  if (p.status == SERL_OK) p.regroup = 1;
  return p;
}

// serl_dyn_open_loop: the dynamics alone (the team without an actor wavefront, one wavefront or one lane per episode); always timed
static inline SerlPlan serl_plan_dyn(const SerlCaps *c, int n_episodes, int lanes_per_wave, int kernel_hint)
{
  const int hint = lanes_per_wave > 0 ? SERL_KERNEL_AUTO : serl_resolve_hint(c, kernel_hint);
  if (hint != SERL_KERNEL_AUTO && hint != SERL_KERNEL_TEAM && hint != SERL_KERNEL_WAVE)
    return serl_plan_refuse(SerlPlan{}, "serl_dyn_open_loop: kernel_hint must be AUTO, TEAM or WAVE");
  if (lanes_per_wave > 0) return serl_plan_lanes(c, 1, n_episodes, lanes_per_wave, 0);
  if (serl_use_team(c, hint, n_episodes)) return serl_plan_one(1, n_episodes, SERL_FAMILY_TEAM, n_episodes, 2, 1, 1, 0, 0);      // (dynamics only: the team without an actor wavefront)
  const int wpb = serl_wave_kernel_waves_per_block(c, n_episodes);
  return serl_plan_one(1, n_episodes, SERL_FAMILY_WAVE, (n_episodes + wpb - 1) / wpb, wpb, 1, 1, 0, 0);
}

// The two launch shapes of the step-wise vector env (family, grid, block, lanes).
static inline SerlPlan serl_plan_venv(const SerlCaps *c, int n_envs, int wave)
{
  if (wave) {      // one wavefront per env (venv_wave.inc), the launch shape of the wave rollout kernels: the CUs fill before the workgroups do
    int wpb = serl_wave_kernel_waves_per_block(c, n_envs);
    if (wpb > 4) wpb = 4;
    return serl_plan_one(0, n_envs, SERL_FAMILY_WAVE, (n_envs + wpb - 1) / wpb, wpb, 1, 1, 0, 0);
  }
  // the launch shape of the lane kernels: lanes per wavefront from the batch, so that small batches still spread over the CUs.
  // A wavefront takes the same time per env step whether it carries 1 or 64 episodes, and wavefronts that
  // share a CU slow each other down (measured: profiles/r01_microbench.md), so episodes are spread one
  // wavefront per CU first (256 CUs) and only then packed into lanes.
  return serl_plan_lanes(c, 0, n_envs, (n_envs + 255) / 256, 0);
}

// serl_rollout_multi: the workgroups grids[k] of every part (episodes[k] of them, four per team), *queue = more than four episodes per CU together,
// *place_out = the placement the launch uses.
static inline void serl_plan_multi(int num_cus, int n, const int32_t *episodes, int place, int32_t *grids, int32_t *queue, int32_t *place_out)
{
  int together = 0, total_wg = 0;
  for (int k = 0; k < n; ++k) together += episodes[k];
  *queue = together > 4 * num_cus;      // beyond four per CU: every part drains a work queue of its own on its share of the CUs
  // workgroups of every part: one per four episodes, or (queue) the part's share of the CUs
  for (int k = 0; k < n; ++k) {
    grids[k] = (episodes[k] + 3) / 4;
    if (*queue) {
      int share = (int)((long long)num_cus * episodes[k] / together);
      share = share < 1 ? 1 : share;
      if (share * 4 < episodes[k]) grids[k] = share;
    }
    total_wg += grids[k];
  }
  // The census placement needs every workgroup resident, one per CU (a team fills a CU's LDS).  The parts round up on their own -- 341 / 341 / 342
  // episodes on 256 CUs are 86 + 86 + 86 = 258 workgroups, and a share bumped to 1 does the same in queue mode -- so the overflow is taken from the
  // largest part, which drains the episodes it loses through its work queue.
  while (total_wg > num_cus) {
    int big = 0;
    for (int k = 1; k < n; ++k) big = grids[k] > grids[big] ? k : big;
    if (grids[big] <= 1) break;
    const int cut = total_wg - num_cus < grids[big] - 1 ? total_wg - num_cus : grids[big] - 1;
    grids[big] -= cut; total_wg -= cut;
  }
  *place_out = (total_wg > num_cus && place == 2) ? 1 : place;      // (more parts than CUs: never all resident -- tickets at once instead of the census' time-out)
}

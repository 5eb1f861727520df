// serl_capi.hip -- C ABI (include/serl_amd.h) of the MI355X-native SERL population-rollout evaluator:
// context / build-table management, rollout dispatch with HIP-event timing, and the SSNE
// weight-tensor kernels.  No torch types cross this boundary: plain pointers, sizes, a hipStream_t.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "rollout_device.h"
#include "serl_ctx.h"

static thread_local std::string g_err;
int serl_fail(int code, const std::string &msg) { g_err = msg; return code; }
static int fail(int code, const std::string &msg) { return serl_fail(code, msg); }

// The kernel families, each compiled once per dynamics code variant (serl_amd/build.py: csrc/family_<f>.hip with -DSERL_DYN=<code>), and the launcher
// every unit exports for its variant v.  X(type, member of SerlLaunchers, function of variant v):
typedef void SerlLaunch(const RolloutArgs &a, int grid, hipStream_t stream);
typedef void SerlLaunchDyn(const RolloutArgs &a, const double *cmds, double *states, int T, int grid, hipStream_t stream);
typedef void SerlLaunchVenv(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream);
typedef void SerlLaunchVenvAuto(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, int grid, hipStream_t stream);
typedef void SerlLaunchVenvRollout(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd, int grid,
                                   hipStream_t stream);
#define SERL_LAUNCHERS(X, v)                                                                                                                     \
  X(SerlLaunch, lane, serl_launch_rollout_##v)              /* one episode per lane (family_lane.hip, rollout_variant.inc) */                   \
  X(SerlLaunch, laneq, serl_launch_rollout_laneq_##v)       /* ... finished lanes take the next episode from a work queue */                    \
  X(SerlLaunch, laneg, serl_launch_rollout_laneg_##v)       /* ... every lane its own actor of any shape (family_laneg.hip) */                  \
  X(SerlLaunch, lanegt, serl_launch_rollout_lanegt_##v)     /* ... over the regrouped copy of the weights (family_lanegt.hip) */                \
  X(SerlLaunchDyn, dyn_lane, serl_launch_dyn_##v)                                                                                                \
  X(SerlLaunchVenv, venv_reset, serl_launch_venv_reset_##v) /* the step-wise vector env, one lane per env (venv_variant.inc) */                  \
  X(SerlLaunchVenv, venv_step, serl_launch_venv_step_##v)                                                                                        \
  X(SerlLaunchVenvAuto, venv_step_auto, serl_launch_venv_step_auto_##v) /* ... step with auto-reset */                                           \
  X(SerlLaunchVenvRollout, venv_rollout, serl_launch_venv_rollout_##v)  /* ... K steps under the lane actor */                                   \
  X(SerlLaunchVenvRollout, venv_rollout_general, serl_launch_venv_rollout_general_##v) /* ... any env configuration and actor shape */          \
  X(SerlLaunch, wave, serl_launch_rollout_wave_##v)         /* one wavefront per episode (rollout_wave.inc) ... */                               \
  X(SerlLaunch, wavex, serl_launch_rollout_wavex_##v)       /* ... env configurations other than the attitude task */                           \
  X(SerlLaunchDyn, dyn_wave, serl_launch_dyn_wave_##v)                                                                                           \
  X(SerlLaunch, team, serl_launch_rollout_team_##v)         /* a team of wavefronts per episode (rollout_team.inc: 7 + the actor wavefront) */  \
  X(SerlLaunch, teamx, serl_launch_rollout_teamx_##v)       /* ... other env configurations */                                                  \
  X(SerlLaunch, teams, serl_launch_rollout_teams_##v)       /* ... the actor wavefront streams its weights */                                   \
  X(SerlLaunchDyn, dyn_team, serl_launch_dyn_team_##v)                                                                                           \
  X(SerlLaunch, teams2, serl_launch_rollout_teams2_##v)     /* ... one forward pass over two actor wavefronts (family_teams2.hip) */            \
  X(SerlLaunch, teamr, serl_launch_rollout_teamr_##v)       /* ... the actor in a workgroup of its own (family_teamr.hip) */                    \
  X(SerlLaunch, half, serl_launch_rollout_half_##v)         /* two episodes per wavefront (rollout_half.inc) */                                 \
  X(SerlLaunch, team2, serl_launch_rollout_team2_##v)       /* two / four episodes per team (rollout_team_half.inc) */                          \
  X(SerlLaunch, team2s, serl_launch_rollout_team2s_##v)                                                                                          \
  X(SerlLaunch, team4, serl_launch_rollout_team4_##v)
#define SERL_MEMBER(T, m, fn) T *m;
#define SERL_DECL(T, m, fn) T fn;
#define SERL_INIT(T, m, fn) fn,
struct SerlLaunchers { SERL_LAUNCHERS(SERL_MEMBER, v) };
// one record per code variant, row = serl_dyn_code (include/serl_amd.h)
#define SERL_VARIANTS(X) X(nominal, SERL_DYN_NOMINAL) X(ice, SERL_DYN_ICE) X(cg_timed, SERL_DYN_CG_TIMED) X(gust, SERL_DYN_GUST) X(test, SERL_DYN_TEST)
#define SERL_VARIANT_DECL(v, code) SERL_LAUNCHERS(SERL_DECL, v)
#define SERL_VARIANT_ROW(v, code) {SERL_LAUNCHERS(SERL_INIT, v)},
#define SERL_VARIANT_CODE(v, code) code,
SERL_VARIANTS(SERL_VARIANT_DECL)
static const SerlLaunchers k_launchers[] = {SERL_VARIANTS(SERL_VARIANT_ROW)};
static constexpr int k_launcher_code[] = {SERL_VARIANTS(SERL_VARIANT_CODE)};
static constexpr int SERL_N_VARIANTS = (int)(sizeof k_launcher_code / sizeof k_launcher_code[0]);
static constexpr bool serl_rows_in_code_order()
{
  for (int i = 0; i < SERL_N_VARIANTS; ++i)
    if (k_launcher_code[i] != i) return false;
  return true;
}
static_assert(serl_rows_in_code_order(), "k_launchers: row i must be serl_dyn_code i");

// the record of a loaded build's code variant (serl_ctx_load_build admits only codes with a row)
static const SerlLaunchers &serl_launchers(int code) { return k_launchers[code]; }

// the env kernels with the in-kernel noise generator (family_lanenz.hip: venv_variant.inc under SERL_VENV_NOISE), one record per code variant as above
typedef void SerlLaunchVenvNz(const RolloutArgs &a, const VenvArgs &v, const serl_venv_noise_desc &nz, int grid, hipStream_t stream);
typedef void SerlLaunchVenvAutoNz(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_noise_desc &nz, int grid,
                                  hipStream_t stream);
typedef void SerlLaunchVenvRolloutNz(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd,
                                     const serl_venv_noise_desc &nz, int grid, hipStream_t stream);
#define SERL_NZ_LAUNCHERS(X, v)                                                       \
  X(SerlLaunchVenvNz, reset, serl_launch_venv_reset_noise_##v)                        \
  X(SerlLaunchVenvAutoNz, step_auto, serl_launch_venv_step_auto_noise_##v)            \
  X(SerlLaunchVenvRolloutNz, rollout, serl_launch_venv_rollout_noise_##v)             \
  X(SerlLaunchVenvRolloutNz, rollout_general, serl_launch_venv_rollout_general_noise_##v)
struct SerlNzLaunchers { SERL_NZ_LAUNCHERS(SERL_MEMBER, v) };
#define SERL_NZ_VARIANT_DECL(v, code) SERL_NZ_LAUNCHERS(SERL_DECL, v)
#define SERL_NZ_VARIANT_ROW(v, code) {SERL_NZ_LAUNCHERS(SERL_INIT, v)},
SERL_VARIANTS(SERL_NZ_VARIANT_DECL)
static const SerlNzLaunchers k_nz_launchers[] = {SERL_VARIANTS(SERL_NZ_VARIANT_ROW)};

// the env kernels with one wavefront per env (family_venvw.hip: venv_wave.inc, plain and under SERL_VENV_NOISE), one record per code variant as above
#define SERL_VW_LAUNCHERS(X, v)                                                       \
  X(SerlLaunchVenv, reset, serl_launch_venv_reset_wave_##v)                           \
  X(SerlLaunchVenv, step, serl_launch_venv_step_wave_##v)                             \
  X(SerlLaunchVenvAuto, step_auto, serl_launch_venv_step_auto_wave_##v)               \
  X(SerlLaunchVenvNz, reset_nz, serl_launch_venv_reset_wave_noise_##v)                \
  X(SerlLaunchVenvAutoNz, step_auto_nz, serl_launch_venv_step_auto_wave_noise_##v)
struct SerlVwLaunchers { SERL_VW_LAUNCHERS(SERL_MEMBER, v) };
#define SERL_VW_VARIANT_DECL(v, code) SERL_VW_LAUNCHERS(SERL_DECL, v)
#define SERL_VW_VARIANT_ROW(v, code) {SERL_VW_LAUNCHERS(SERL_INIT, v)},
SERL_VARIANTS(SERL_VW_VARIANT_DECL)
static const SerlVwLaunchers k_vw_launchers[] = {SERL_VARIANTS(SERL_VW_VARIANT_ROW)};

// CitationVecEnv.rollout with one wavefront per env (family_venvwr.hip: venv_wave_rollout.inc, plain and under SERL_VENV_NOISE), one record per code variant as above
#define SERL_VWR_LAUNCHERS(X, v)                                                      \
  X(SerlLaunchVenvRollout, rollout, serl_launch_venv_rollout_wave_##v)                \
  X(SerlLaunchVenvRolloutNz, rollout_nz, serl_launch_venv_rollout_wave_noise_##v)
struct SerlVwrLaunchers { SERL_VWR_LAUNCHERS(SERL_MEMBER, v) };
#define SERL_VWR_VARIANT_DECL(v, code) SERL_VWR_LAUNCHERS(SERL_DECL, v)
#define SERL_VWR_VARIANT_ROW(v, code) {SERL_VWR_LAUNCHERS(SERL_INIT, v)},
SERL_VARIANTS(SERL_VWR_VARIANT_DECL)
static const SerlVwrLaunchers k_vwr_launchers[] = {SERL_VARIANTS(SERL_VWR_VARIANT_ROW)};

// the population rollout kernels with the in-kernel noise generator (family_lanern.hip, family_lanegn.hip, family_lanegtn.hip, family_wavern.hip: rollout_variant.inc /
// rollout_wave.inc under SERL_ROLLOUT_NOISE), one record per code variant as above
typedef void SerlLaunchNz(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int grid, hipStream_t stream);
#define SERL_RN_LAUNCHERS(X, v)                                  \
  X(SerlLaunchNz, lane, serl_launch_rollout_noise_##v)           \
  X(SerlLaunchNz, laneg, serl_launch_rollout_laneg_noise_##v)    \
  X(SerlLaunchNz, lanegt, serl_launch_rollout_lanegt_noise_##v)  \
  X(SerlLaunchNz, wave, serl_launch_rollout_wave_noise_##v)      \
  X(SerlLaunchNz, wavex, serl_launch_rollout_wavex_noise_##v)
struct SerlRnLaunchers { SERL_RN_LAUNCHERS(SERL_MEMBER, v) };
#define SERL_RN_VARIANT_DECL(v, code) SERL_RN_LAUNCHERS(SERL_DECL, v)
#define SERL_RN_VARIANT_ROW(v, code) {SERL_RN_LAUNCHERS(SERL_INIT, v)},
SERL_VARIANTS(SERL_RN_VARIANT_DECL)
static const SerlRnLaunchers k_rn_launchers[] = {SERL_VARIANTS(SERL_RN_VARIANT_ROW)};

#include "serl_mixed.h"

static_assert(SERL_PLAN_MAX_HIDDEN == SERL_MAX_HIDDEN && SERL_PLAN_MAIL_BYTES == sizeof(SerlMail) && SERL_PLAN_MIXED_MAX == SERL_MIXED_MAX,
              "serl_plan.h restates these for the host-only planner");

// The launcher of a planned family (serl_plan.h), looked up HERE and nowhere else: what a call launches and what serl_last_rollout_info records
// are both the plan's.  nullptr: the entry has no kernel of that family.
static SerlLaunch *SerlLaunchers::*serl_rollout_launcher(const SerlPlan &p)
{
  switch (p.family) {
    case SERL_FAMILY_TEAM: return &SerlLaunchers::team;
    case SERL_FAMILY_TEAMS: return &SerlLaunchers::teams;
    case SERL_FAMILY_TEAMS2: return &SerlLaunchers::teams2;
    case SERL_FAMILY_TEAMR: return &SerlLaunchers::teamr;
    case SERL_FAMILY_TEAMX: return &SerlLaunchers::teamx;
    case SERL_FAMILY_TEAM2: return &SerlLaunchers::team2;
    case SERL_FAMILY_TEAM2S: return &SerlLaunchers::team2s;
    case SERL_FAMILY_TEAM4: return &SerlLaunchers::team4;
    case SERL_FAMILY_HALF: return &SerlLaunchers::half;
    case SERL_FAMILY_WAVE: return &SerlLaunchers::wave;
    case SERL_FAMILY_WAVEX: return &SerlLaunchers::wavex;
    case SERL_FAMILY_LANE: return p.laneq ? &SerlLaunchers::laneq : &SerlLaunchers::lane;
    case SERL_FAMILY_LANEG: return p.regroup ? &SerlLaunchers::lanegt : &SerlLaunchers::laneg;      // (regroup: serl_rollout_regrouped alone plans it for this family)
    default: return nullptr;
  }
}
static SerlLaunchNz *SerlRnLaunchers::*serl_noise_launcher(const SerlPlan &p)
{
  switch (p.family) {
    case SERL_FAMILY_WAVE: return &SerlRnLaunchers::wave;
    case SERL_FAMILY_WAVEX: return &SerlRnLaunchers::wavex;
    case SERL_FAMILY_LANE: return p.laneq ? nullptr : &SerlRnLaunchers::lane;
    case SERL_FAMILY_LANEG: return p.regroup ? &SerlRnLaunchers::lanegt : &SerlRnLaunchers::laneg;
    default: return nullptr;
  }
}
static SerlLaunchDyn *SerlLaunchers::*serl_dyn_launcher(const SerlPlan &p)
{
  switch (p.family) {
    case SERL_FAMILY_TEAM: return &SerlLaunchers::dyn_team;
    case SERL_FAMILY_WAVE: return &SerlLaunchers::dyn_wave;
    case SERL_FAMILY_LANE: return &SerlLaunchers::dyn_lane;
    default: return nullptr;
  }
}

// Work-queue counter of ONE launch: a ring of counters, so that queue launches in flight on different streams (a mixed-fault sweep;
// validation beside training) never share one -- a second launch's memset or atomicAdd on a shared counter would make the first
// skip or repeat episodes.  (64 launches later a counter is reused: far beyond what a context keeps in flight.)
static int32_t *serl_next_queue_counter(serl_ctx *c)
{
  int32_t *p = c->queue + c->queue_next;
  c->queue_next = (c->queue_next + 1) % SERL_QUEUE_COUNTERS;
  return p;
}


// Lane-per-episode kernels (lane_actor.h serl_actor_forward_lane32_t): the population [members][stride] regrouped to [ceil(P / 4)][mpad][4], so that parameter
// group g of 64 consecutive members is ONE run of 1 KB.  Reads run along a member's row, writes are 16 B pieces (30 MB for 2 048 SERL50 actors: microseconds in front of a
// launch of hundreds of milliseconds).
__global__ void serl_regroup_weights_kernel(const float *w, int64_t stride, int32_t n_members, int32_t P, float *out, int32_t mpad)
{
  const int g = blockIdx.y * blockDim.x + threadIdx.x, m = blockIdx.x;
  if (4 * g >= P) return;
  const float *row = w + (size_t)m * stride + 4 * (size_t)g;
  float4 v;
  v.x = row[0];
  v.y = 4 * g + 1 < P ? row[1] : 0.0f;
  v.z = 4 * g + 2 < P ? row[2] : 0.0f;
  v.w = 4 * g + 3 < P ? row[3] : 0.0f;
  *(float4 *)(out + ((size_t)g * mpad + m) * 4) = v;
}

static int serl_regroup_weights(serl_ctx *c, const serl_rollout_desc *d, RolloutArgs &a, hipStream_t stream)
{
  const int P = d->hidden * d->state_dim + d->hidden + d->num_layers * (d->hidden * d->hidden + 3 * d->hidden) + d->action_dim * d->hidden + d->action_dim;
  const int groups = (P + 3) / 4, mpad = (d->n_members + 63) / 64 * 64;
  const size_t bytes = (size_t)groups * mpad * 16;
  const int slot = c->wt_next;
  c->wt_next = (c->wt_next + 1) % SERL_WT_SLOTS;
  // a launch on another stream may still read the copy this slot held (more than SERL_WT_SLOTS lane launches in flight): order this launch behind it
  if (c->wt_done[slot]) HIP_TRY(hipStreamWaitEvent(stream, c->wt_done[slot], 0));
  else HIP_TRY(hipEventCreateWithFlags(&c->wt_done[slot], hipEventDisableTiming));
  c->wt_slot_of_launch = slot;
  if (c->wt_cap[slot] < bytes) {
    if (c->wt[slot]) HIP_TRY(hipFree(c->wt[slot]));      // (waits for the launches that read it)
    c->wt[slot] = nullptr; c->wt_cap[slot] = 0;
    HIP_TRY(hipMalloc(&c->wt[slot], bytes));
    c->wt_cap[slot] = bytes;
  }
  hipLaunchKernelGGL(serl_regroup_weights_kernel, dim3(d->n_members, (groups + 255) / 256), dim3(256), 0, stream, d->weights, d->weight_stride, d->n_members, P,
                     (float *)c->wt[slot], mpad);
  HIP_TRY(hipGetLastError());
  a.wt = (const float *)c->wt[slot];
  a.wt_members = mpad;
  const int64_t rec[4] = {1, mpad, groups, (int64_t)bytes};      // serl_last_rollout_weights: serl_note_launch makes it the launch's record
  for (int i = 0; i < 4; ++i) c->wt_pending[i] = rec[i];
  return SERL_OK;
}


// serl_last_rollout_info's record of a call (include/serl_amd.h)
static void serl_note_launch(serl_ctx *c, int family, int grid, int per_team, bool queue, int actor_waves, bool streamed, int launches, int code)
{
  const int32_t v[8] = {family, grid, per_team, queue ? 1 : 0, actor_waves, streamed ? 1 : 0, launches, code};
  for (int i = 0; i < 8; ++i) c->last_info[i] = v[i];
  // serl_last_rollout_weights: the copy serl_regroup_weights made for THIS launch, zeros for a launch that regrouped nothing
  for (int i = 0; i < 4; ++i) { c->last_weights[i] = c->wt_pending[i]; c->wt_pending[i] = 0; }
}

// RolloutArgs of n_episodes on a build's tables (what every launch path starts from) ...
static void serl_fill_args(serl_ctx *c, int slot, int n_episodes, RolloutArgs &a)
{
  const BuildSlot &s = c->slots[slot];
  memset(&a, 0, sizeof(a));
  a.d.n_episodes = n_episodes;
  a.ro = s.blob; a.t3 = s.blob + s.n_ro; a.x0 = a.t3 + 46; a.dw0 = a.x0 + 19;
  a.dyn_dt = s.dt;
}

// ... of one descriptor
static void serl_fill_args(serl_ctx *c, const serl_rollout_desc *d, RolloutArgs &a)
{
  serl_fill_args(c, d->build_slot, d->n_episodes, a);
  a.d = *d;
  a.jitter = c->env_jitter; a.jitter_sites = c->env_jitter_sites;
}

// Carries a plan out on `stream`: `launch(a, grid)` is the entry's kernel of the plan's family, `code` the build's code variant.  Everything the launch
// needs goes in front of it first, then ev0: the kernel alone is timed.
template <class Launch>
static int serl_execute_plan(serl_ctx *c, const SerlPlan &p, RolloutArgs &a, int code, bool profile, hipStream_t stream, Launch launch)
{
  const serl_rollout_desc *d = &a.d;
  a.lanes = p.lanes;
  a.block = p.block;
  if (profile && c->env_profile) {
    if (!c->prof) HIP_TRY(hipMalloc((void **)&c->prof, 32 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c->prof, 0, 32 * sizeof(unsigned long long), stream));
    a.prof = c->prof;
  }
  for (int i = 0; i < 4; ++i) c->wt_pending[i] = 0;
  if (p.regroup) {
    const int rc = serl_regroup_weights(c, d, a, stream);
    if (rc != SERL_OK) return rc;
  }
  a.q0 = p.q0;
  if (p.queue) {
    a.queue = serl_next_queue_counter(c);
    HIP_TRY(hipMemsetAsync(a.queue, 0, sizeof(int32_t), stream));
  }
  if (p.mailbox) {
    const size_t region = (size_t)c->caps.num_cus * sizeof(SerlMail);
    if (!c->mail) HIP_TRY(hipMalloc(&c->mail, SERL_MAIL_REGIONS * region));
    a.mail = (char *)c->mail + (size_t)c->mail_next * region;
    c->mail_next = (c->mail_next + 1) % SERL_MAIL_REGIONS;
    HIP_TRY(hipMemsetAsync(a.mail, 0, (size_t)p.mail_bytes, stream));
  }
  if (p.timed) HIP_TRY(hipEventRecord(c->ev0, stream));
  for (int i = 0; i < p.launches; ++i) {
    a.e0 = i * p.chunk;
    a.e_end = a.e0 + p.chunk < d->n_episodes ? a.e0 + p.chunk : d->n_episodes;
    launch(a, p.launches > 1 ? a.e_end - a.e0 : p.grid);
    HIP_TRY(hipGetLastError());
  }
  if (p.regroup) HIP_TRY(hipEventRecord(c->wt_done[c->wt_slot_of_launch], stream));
  serl_note_launch(c, p.family, p.grid, p.per_team, p.queue != 0, p.actor_waves, p.streamed != 0, p.launches, code);
  if (p.timed) HIP_TRY(hipEventRecord(c->ev1, stream));
  c->timed = p.timed != 0;
  return SERL_OK;
}

extern "C" {

int serl_abi_version(void) { return SERL_ABI_VERSION; }

int serl_abi_layout(int32_t *out, int32_t capacity)
{
#define SERL_OFF(m) (int32_t)offsetof(serl_rollout_desc, m)
  const int32_t v[] = {
    (int32_t)sizeof(serl_rollout_desc),
    SERL_OFF(state_dim), SERL_OFF(action_dim), SERL_OFF(hidden), SERL_OFF(num_layers), SERL_OFF(activation), SERL_OFF(n_members),
    SERL_OFF(weights), SERL_OFF(weight_stride), SERL_OFF(n_episodes), SERL_OFF(build_slot), SERL_OFF(member_of_episode),
    SERL_OFF(faults), SERL_OFF(ref), SERL_OFF(ref_stride), SERL_OFF(err0), SERL_OFF(action_noise), SERL_OFF(noise_row),
    SERL_OFF(sensor_noise), SERL_OFF(sensor_row), SERL_OFF(tick0), SERL_OFF(t_max), SERL_OFF(max_steps), SERL_OFF(lanes_per_wave),
    SERL_OFF(concurrent_episodes), SERL_OFF(kernel_hint), SERL_OFF(fitness), SERL_OFF(length_steps), SERL_OFF(length_t),
    SERL_OFF(cost_steps), SERL_OFF(actions), SERL_OFF(states), SERL_OFF(rewards), SERL_OFF(transitions), SERL_OFF(ref_spec),
    SERL_OFF(ref_spec_stride), SERL_OFF(env_config), SERL_OFF(incremental),
    (int32_t)sizeof(serl_build_desc), (int32_t)sizeof(serl_fault_row), (int32_t)sizeof(serl_ref_spec), (int32_t)sizeof(serl_replay_job),
#undef SERL_OFF
#define SERL_OFF(m) (int32_t)offsetof(serl_venv_desc, m)
    (int32_t)sizeof(serl_venv_desc),
    SERL_OFF(n_envs), SERL_OFF(build_slot), SERL_OFF(env_config), SERL_OFF(incremental), SERL_OFF(state_dim), SERL_OFF(action_dim),
    SERL_OFF(max_steps), SERL_OFF(pad0), SERL_OFF(t_max), SERL_OFF(faults), SERL_OFF(ref), SERL_OFF(ref_stride), SERL_OFF(ref_spec),
    SERL_OFF(ref_spec_stride), SERL_OFF(sensor_noise), SERL_OFF(sensor_row), SERL_OFF(err0), SERL_OFF(tick0), SERL_OFF(state)};
#undef SERL_OFF
  const int32_t n = (int32_t)(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = v[i];
  return n;
}

int serl_env_action_dim(int env_config) { return serl_plan_env_action_dim(env_config); }
int serl_env_state_dim(int env_config, int incremental) { return serl_plan_env_state_dim(env_config, incremental); }
const char *serl_last_error(void) { return g_err.c_str(); }

int serl_ctx_create(int device, serl_ctx **out)
{
  if (!out) return fail(SERL_E_INVALID, "serl_ctx_create: out is NULL");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(SERL_E_INVALID, "serl_ctx_create: no such device");
  HIP_TRY(hipSetDevice(device));
  serl_ctx *c = new (std::nothrow) serl_ctx();
  if (!c) return fail(SERL_E_NOMEM, "serl_ctx_create: out of memory");
  c->device = device;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
      if (prop.multiProcessorCount > 0) c->caps.num_cus = prop.multiProcessorCount;
      if (prop.sharedMemPerBlockOptin > 0) c->lds_per_block = (int)prop.sharedMemPerBlockOptin;
    }
  }
  {   // development overrides: the library's only look at the process environment
    const char *e;
    c->caps.env_kernel = SERL_KERNEL_AUTO;
    if ((e = getenv("SERL_KERNEL")) != nullptr) {
      const std::string k(e);
      c->caps.env_kernel = k == "team" ? SERL_KERNEL_TEAM : k == "team2" ? SERL_KERNEL_TEAM2 : k == "team4" ? SERL_KERNEL_TEAM4
                    : k == "wave" ? SERL_KERNEL_WAVE : k == "half" ? SERL_KERNEL_HALF : k == "laneq" ? SERL_KERNEL_LANEQ : k == "laneg" ? SERL_KERNEL_LANEG : SERL_KERNEL_AUTO;
    }
    c->caps.env_laneq_waves = (e = getenv("SERL_LANEQ_WAVES")) ? atoi(e) : -1;
    c->caps.env_waves_per_block = (e = getenv("SERL_WAVES_PER_BLOCK")) ? atoi(e) : -1;
    c->env_profile = getenv("SERL_PROFILE") != nullptr;
    c->caps.env_split_actor = (e = getenv("SERL_SPLIT_ACTOR")) ? atoi(e) : 0;
    c->caps.env_remote_actor = (e = getenv("SERL_REMOTE_ACTOR")) ? atoi(e) : 1;
    c->caps.env_lane_regroup = ((e = getenv("SERL_LANE_WEIGHTS")) && !strcmp(e, "rows")) ? 0 : 1;
    c->env_mixed_place = (e = getenv("SERL_MIXED_PLACE")) ? atoi(e) : SERL_MIXED_PLACE_DEFAULT;
    c->env_jitter = (e = getenv("SERL_JITTER_SEED")) ? (unsigned)strtoul(e, nullptr, 0) : 0u;
    c->env_jitter_sites = (e = getenv("SERL_JITTER_SITES")) ? (unsigned)strtoul(e, nullptr, 0) : ~0u;
  }
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipMalloc((void **)&c->queue, SERL_QUEUE_COUNTERS * sizeof(int32_t)));
  *out = c;
  return SERL_OK;
}

int serl_ctx_destroy(serl_ctx *c)
{
  if (!c) return SERL_OK;
  (void)hipSetDevice(c->device);
  for (auto &s : c->slots) if (s.blob) (void)hipFree(s.blob);
  if (c->mail) (void)hipFree(c->mail);
  for (int i = 0; i < SERL_WT_SLOTS; ++i) { if (c->wt[i]) (void)hipFree(c->wt[i]); if (c->wt_done[i]) (void)hipEventDestroy(c->wt_done[i]); }
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->prof) (void)hipFree(c->prof);
  if (c->queue) (void)hipFree(c->queue);
  if (c->mixed_state) (void)hipFree(c->mixed_state);
  for (auto &e : c->mixed_ev) if (e) (void)hipEventDestroy(e);
  delete c;
  return SERL_OK;
}

int serl_ctx_load_build(serl_ctx *c, int slot, const serl_build_desc *b)
{
  if (!c || !b || slot < 0 || slot >= SERL_MAX_SLOTS) return fail(SERL_E_INVALID, "serl_ctx_load_build: bad argument");
  if (!b->ro || !b->t3 || !b->x0 || !b->dw0 || b->n_ro <= 0) return fail(SERL_E_INVALID, "serl_ctx_load_build: NULL table");
  if (b->code < 0 || b->code >= SERL_N_VARIANTS)      // (every family has a kernel for every code variant with a row: the dispatch never asks again)
    return fail(SERL_E_UNSUPPORTED, "serl_ctx_load_build: dynamics code variant not compiled into this library");
  HIP_TRY(hipSetDevice(c->device));
  BuildSlot &s = c->slots[slot];
  if (s.blob) { HIP_TRY(hipFree(s.blob)); s.blob = nullptr; s.loaded = false; }
  const size_t n = (size_t)b->n_ro + 46 + 19 + 31;
  std::vector<double> host(n);
  memcpy(host.data(), b->ro, sizeof(double) * b->n_ro);
  memcpy(host.data() + b->n_ro, b->t3, sizeof(double) * 46);
  memcpy(host.data() + b->n_ro + 46, b->x0, sizeof(double) * 19);
  memcpy(host.data() + b->n_ro + 65, b->dw0, sizeof(double) * 31);
  HIP_TRY(hipMalloc((void **)&s.blob, sizeof(double) * n));
  HIP_TRY(hipMemcpy(s.blob, host.data(), sizeof(double) * n, hipMemcpyHostToDevice));
  s.n_ro = b->n_ro; s.code = b->code; s.ro_base = b->ro_base; s.dt = b->dt; s.loaded = true;
  return SERL_OK;
}

int serl_param_count(int S, int H, int L, int A) { return serl_plan_param_count(S, H, L, A); }

// argument checks of serl_rollout / serl_rollout_multi; *hint_out = the resolved kernel hint
static int serl_check_desc(serl_ctx *c, const serl_rollout_desc *d, int *hint_out)
{
  if (!c || !d) return fail(SERL_E_INVALID, "serl_rollout: NULL argument");
  if (d->build_slot < 0 || d->build_slot >= SERL_MAX_SLOTS || !c->slots[d->build_slot].loaded)
    return fail(SERL_E_INVALID, "serl_rollout: build slot not loaded");
  if (d->n_episodes <= 0) return fail(SERL_E_INVALID, "serl_rollout: n_episodes <= 0");
  if (!d->weights || !d->member_of_episode || (!d->ref && !d->ref_spec) || !d->fitness || !d->length_steps || !d->length_t || !d->cost_steps)
    return fail(SERL_E_INVALID, "serl_rollout: required device pointer is NULL");
  const char *message = "";
  const int rc = serl_plan_check(&c->caps, d, hint_out, &message);
  return rc == SERL_OK ? SERL_OK : fail(rc, message);
}

// serl_rollout and serl_rollout_noise (nz != NULL): check, plan, refuse if the plan refuses, execute
static int serl_rollout_impl(serl_ctx *c, const serl_rollout_desc *d, const serl_rollout_noise_desc *nz, int hint, void *stream_, bool regrouped = false)
{
  const SerlPlan p = regrouped ? serl_plan_rollout_regrouped(&c->caps, d, hint, nz != nullptr) : serl_plan_rollout(&c->caps, d, hint, nz != nullptr);
  if (p.status != SERL_OK) return fail(p.status, p.message);
  HIP_TRY(hipSetDevice(c->device));
  const int code = c->slots[d->build_slot].code;
  hipStream_t stream = (hipStream_t)stream_;
  RolloutArgs a;
  serl_fill_args(c, d, a);
  if (nz) {
    SerlLaunchNz *launch = k_rn_launchers[code].*serl_noise_launcher(p);
    return serl_execute_plan(c, p, a, code, false, stream, [&](const RolloutArgs &a, int grid) { launch(a, *nz, grid, stream); });
  }
  SerlLaunch *launch = serl_launchers(code).*serl_rollout_launcher(p);
  return serl_execute_plan(c, p, a, code, true, stream, [&](const RolloutArgs &a, int grid) { launch(a, grid, stream); });
}

int serl_rollout(serl_ctx *c, const serl_rollout_desc *d, void *stream_)
{
  int hint = SERL_KERNEL_AUTO;
  { const int rc_ = serl_check_desc(c, d, &hint); if (rc_ != SERL_OK) return rc_; }
  return serl_rollout_impl(c, d, nullptr, hint, stream_);
}

int serl_rollout_noise_layout(int32_t *out, int32_t capacity)
{
#define SERL_OFF(m) (int32_t)offsetof(serl_rollout_noise_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_rollout_noise_desc), SERL_OFF(seed), SERL_OFF(env), SERL_OFF(episode), SERL_OFF(sensor), SERL_OFF(pad0),
                       SERL_OFF(sensor_bias), SERL_OFF(sensor_scale), SERL_OFF(action), SERL_OFF(pad1), SERL_OFF(action_sd), SERL_OFF(action_clip)};
#undef SERL_OFF
  const int32_t n = (int32_t)(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = v[i];
  return n;
}

// the argument checks of serl_rollout_noise behind serl_check_desc's
static int serl_check_noise(const serl_rollout_desc *d, const serl_rollout_noise_desc *nz)
{
  if (!nz) return fail(SERL_E_INVALID, "serl_rollout_noise: nz is NULL");
  if ((nz->sensor != 0 && nz->sensor != 1) || (nz->action != 0 && nz->action != 1)) return fail(SERL_E_INVALID, "serl_rollout_noise: nz->sensor / nz->action must be 0 or 1");
  if (d->sensor_noise && nz->sensor) return fail(SERL_E_INVALID, "serl_rollout_noise: desc->sensor_noise together with nz->sensor");
  if (d->action_noise && nz->action) return fail(SERL_E_INVALID, "serl_rollout_noise: desc->action_noise together with nz->action");
  if (!(nz->action_sd >= 0.0) || !(nz->action_clip >= 0.0)) return fail(SERL_E_INVALID, "serl_rollout_noise: nz->action_sd / nz->action_clip < 0");
  return SERL_OK;
}

// serl_rollout with the sensor / exploration noise drawn inside the kernels.  Launch geometry, weight regrouping, timing events and the launch record are
// serl_rollout's for the same family: one planner decides both (serl_plan.h serl_plan_rollout).
int serl_rollout_noise(serl_ctx *c, const serl_rollout_desc *d, const serl_rollout_noise_desc *nz, void *stream_)
{
  int hint = SERL_KERNEL_AUTO;
  { const int rc_ = serl_check_desc(c, d, &hint); if (rc_ != SERL_OK) return rc_; }
  { const int rc_ = serl_check_noise(d, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_rollout_impl(c, d, nz, hint, stream_);
}

// serl_rollout (nz == NULL) / serl_rollout_noise of kernel_hint SERL_KERNEL_LANEG over a REGROUPED copy of the weights (family_lanegt.hip / family_lanegtn.hip:
// lane_actor.h serl_actor_forward_lane_general_t): the same checks, then the LANEG plan with regroup = 1 (serl_plan.h serl_plan_rollout_regrouped), carried
// out by serl_execute_plan as every plan -- the copy goes into the ring of SERL_WT_SLOTS slots the hidden-32 lane kernels use.
int serl_rollout_regrouped(serl_ctx *c, const serl_rollout_desc *d, const serl_rollout_noise_desc *nz, void *stream_)
{
  int hint = SERL_KERNEL_AUTO;
  { const int rc_ = serl_check_desc(c, d, &hint); if (rc_ != SERL_OK) return rc_; }
  if (nz) { const int rc_ = serl_check_noise(d, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_rollout_impl(c, d, nz, hint, stream_, true);
}

// Several descriptors -- one per dynamics build of a mixed-fault population -- in ONE launch of one code object (rollout_team4_mixed.hip).
// Eligible: 2 .. SERL_MIXED_MAX descriptors of the attitude task with the LDS-sized actor shape (hidden 32), code variants nominal / ice, automatic
// kernel choice, more than 2 x CUs episodes together (the four-episodes-per-team size class).  Anything else returns SERL_E_UNSUPPORTED and the
// caller launches the descriptors one by one (serl_rollout with concurrent_episodes, streams of their own).
int serl_rollout_multi(serl_ctx *c, int32_t n, const serl_rollout_desc *descs, void *stream_)
{
  if (!c || !descs) return fail(SERL_E_INVALID, "serl_rollout_multi: NULL argument");
  if (n < 2 || n > SERL_MIXED_MAX) return fail(SERL_E_UNSUPPORTED, "serl_rollout_multi: 2 .. 4 descriptors");
  int together = 0;
  for (int k = 0; k < n; ++k) {
    const serl_rollout_desc *d = descs + k;
    int hint = SERL_KERNEL_AUTO;
    const int rc_ = serl_check_desc(c, d, &hint);
    if (rc_ != SERL_OK) return rc_;
    const int code = c->slots[d->build_slot].code;
    if (d->env_config != SERL_ENV_ATTITUDE || d->incremental != 0 || d->hidden != 32 || d->num_layers > 3 || d->lanes_per_wave > 0 ||
        hint != SERL_KERNEL_AUTO || (code != SERL_DYN_NOMINAL && code != SERL_DYN_ICE))
      return fail(SERL_E_UNSUPPORTED, "serl_rollout_multi: attitude task, hidden 32, code variants nominal / ice, kernel_hint AUTO");
    together += d->n_episodes;
  }
  if (together <= 2 * c->caps.num_cus) return fail(SERL_E_UNSUPPORTED, "serl_rollout_multi: for more than 2 x CUs episodes (four per team)");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_;
  SerlMixedArgs m;
  memset(&m, 0, sizeof(m));
  m.n = n;
  m.place = c->env_mixed_place;
  int state_slot = -1;
  c->mixed_last = -1;
  if (m.place != 0) {
    if (!c->mixed_state) HIP_TRY(hipMalloc((void **)&c->mixed_state, SERL_MIXED_STATES * SERL_MIXED_STATE * sizeof(int32_t)));
    state_slot = c->mixed_state_next;
    c->mixed_last = state_slot;
    m.state = c->mixed_state + (size_t)state_slot * SERL_MIXED_STATE;
    c->mixed_state_next = (c->mixed_state_next + 1) % SERL_MIXED_STATES;
    // (two launches must never count into one census: the workgroups would disagree about the assignment)
    if (c->mixed_ev[state_slot]) HIP_TRY(hipStreamWaitEvent(stream, c->mixed_ev[state_slot], 0));
    else HIP_TRY(hipEventCreateWithFlags(&c->mixed_ev[state_slot], hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(m.state, 0, SERL_MIXED_STATE * sizeof(int32_t), stream));
  }
  int32_t episodes[SERL_MIXED_MAX], grids[SERL_MIXED_MAX], queue = 0;
  for (int k = 0; k < n; ++k) episodes[k] = descs[k].n_episodes;
  serl_plan_multi(c->caps.num_cus, n, episodes, m.place, grids, &queue, &m.place);
  int wg = 0;
  for (int k = 0; k < n; ++k) {
    const serl_rollout_desc *d = descs + k;
    RolloutArgs &a = m.a[k];
    serl_fill_args(c, d, a);
    a.lanes = 1;
    a.block = 512;
    const int grid = grids[k];
    a.queue = nullptr; a.q0 = d->n_episodes;
    if (grid * 4 < d->n_episodes) {
      a.queue = serl_next_queue_counter(c);
      a.q0 = 4 * grid;
      HIP_TRY(hipMemsetAsync(a.queue, 0, sizeof(int32_t), stream));
    }
    m.first_wg[k] = wg;
    m.code[k] = c->slots[d->build_slot].code;
    // the lane-group kernels find their episodes at e0 + blockIdx.x * 4 + group: shift e0 (and the queue's first episode stays absolute)
    a.e0 = -4 * wg; a.e_end = d->n_episodes;
    wg += grid;
  }
  m.first_wg[n] = wg;
  HIP_TRY(hipEventRecord(c->ev0, stream));
  serl_launch_rollout_team4_mixed(m, wg, stream);
  HIP_TRY(hipGetLastError());
  {
    bool one_code = true;
    for (int k = 1; k < n; ++k) one_code = one_code && m.code[k] == m.code[0];
    bool any_queue = false;
    for (int k = 0; k < n; ++k) any_queue = any_queue || m.a[k].queue != nullptr;
    serl_note_launch(c, SERL_FAMILY_TEAM4_MIXED, wg, 4, any_queue, 1, true, 1, one_code ? m.code[0] : -1);
  }
  if (state_slot >= 0) HIP_TRY(hipEventRecord(c->mixed_ev[state_slot], stream));
  HIP_TRY(hipEventRecord(c->ev1, stream));
  c->timed = true;
  return SERL_OK;
}

int serl_dyn_open_loop(serl_ctx *c, int slot, int32_t n_episodes, int32_t T, const double *cmds, double *states,
                       int32_t lanes_per_wave, int32_t kernel_hint, void *stream_)
{
  if (!c || !cmds || !states || n_episodes <= 0 || T <= 0) return fail(SERL_E_INVALID, "serl_dyn_open_loop: bad argument");
  const SerlPlan p = serl_plan_dyn(&c->caps, n_episodes, lanes_per_wave, kernel_hint);
  if (p.status != SERL_OK) return fail(p.status, p.message);
  if (slot < 0 || slot >= SERL_MAX_SLOTS || !c->slots[slot].loaded) return fail(SERL_E_INVALID, "serl_dyn_open_loop: build slot not loaded");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t stream = (hipStream_t)stream_;
  RolloutArgs a;
  serl_fill_args(c, slot, n_episodes, a);
  a.jitter = c->env_jitter; a.jitter_sites = c->env_jitter_sites;
  const int code = c->slots[slot].code;
  SerlLaunchDyn *launch = serl_launchers(code).*serl_dyn_launcher(p);
  return serl_execute_plan(c, p, a, code, false, stream, [&](const RolloutArgs &a, int grid) { launch(a, cmds, states, T, grid, stream); });
}

// ---- the step-wise vector env (include/serl_amd.h, ABI v9) ----------------------------------------------------------------------
int64_t serl_venv_state_bytes(int32_t n_envs)
{
  if (n_envs < 1) return 0;
  return serl_venv_npad(n_envs) * (int64_t)(SERL_VENV_F64 * sizeof(double) + SERL_VENV_I32 * sizeof(int32_t));
}

static int serl_venv_check(serl_ctx *c, const serl_venv_desc *d, const char *what)
{
  const std::string w(what);
  if (!c || !d) return fail(SERL_E_INVALID, w + ": NULL argument");
  if (d->n_envs <= 0) return fail(SERL_E_INVALID, w + ": n_envs <= 0");
  if (d->build_slot < 0 || d->build_slot >= SERL_MAX_SLOTS || !c->slots[d->build_slot].loaded)
    return fail(SERL_E_INVALID, w + ": build slot not loaded");
  if (c->slots[d->build_slot].code < 0 || c->slots[d->build_slot].code >= SERL_N_VARIANTS) return fail(SERL_E_UNSUPPORTED, w + ": unknown code variant");
  if (serl_env_state_dim(d->env_config, d->incremental) == 0)
    return fail(SERL_E_INVALID, w + ": env_config must be SERL_ENV_ATTITUDE, SERL_ENV_SYMMETRIC or SERL_ENV_FULL");
  if (d->state_dim != serl_env_state_dim(d->env_config, d->incremental) || d->action_dim != serl_env_action_dim(d->env_config))
    return fail(SERL_E_INVALID, w + ": state_dim / action_dim do not match the env configuration (attitude 7 / 3, symmetric 2 / 1, full 13 / 3; incremental adds action_dim observations)");
  if (d->max_steps <= 0) return fail(SERL_E_INVALID, w + ": max_steps <= 0");
  if (!(d->t_max > 0.0)) return fail(SERL_E_INVALID, w + ": t_max <= 0");
  if (!d->ref && !d->ref_spec) return fail(SERL_E_INVALID, w + ": neither ref nor ref_spec");
  if (d->ref && !d->ref_spec && d->ref_stride != 0 && d->ref_stride < (int64_t)d->max_steps * 3)
    return fail(SERL_E_INVALID, w + ": ref_stride smaller than max_steps x 3");
  if (d->ref_spec && d->ref_spec_stride != 0 && d->ref_spec_stride != 1) return fail(SERL_E_INVALID, w + ": ref_spec_stride must be 0 or 1");
  if (!d->state) return fail(SERL_E_INVALID, w + ": state is NULL");
  if (((uintptr_t)d->state & 7) != 0) return fail(SERL_E_INVALID, w + ": state must be 8-byte aligned");
  return SERL_OK;
}

// serl_venv_last_info's record of an env call (include/serl_amd.h)
static void serl_note_venv_launch(serl_ctx *c, int family, int grid, int waves_per_block, int code)
{
  c->last_venv_info[0] = family; c->last_venv_info[1] = grid; c->last_venv_info[2] = waves_per_block; c->last_venv_info[3] = code;
}

// which env kernel a call launches, beside the descriptor and the VenvArgs
struct SerlVenvCall {
  bool step = false;                               // serl_venv_step (otherwise reset)
  const serl_venv_auto_desc *au = nullptr;         // the step with auto-reset, or with rd: K steps
  const serl_venv_rollout_desc *rd = nullptr;      // K steps under the in-kernel actor ...
  bool general = false;                            // ... of any env configuration and actor shape (lane kernels)
  const serl_venv_noise_desc *nz = nullptr;        // the instantiations with the in-kernel noise generator (there is no plain step among them)
  bool wave = false;                               // one wavefront per env
};

static int serl_venv_launch(serl_ctx *c, const serl_venv_desc *d, VenvArgs &v, hipStream_t stream, const SerlVenvCall &k)
{
  const int code = c->slots[d->build_slot].code;
  const SerlPlan p = serl_plan_venv(&c->caps, d->n_envs, k.wave);
  const int grid = p.grid;
  RolloutArgs a;
  serl_fill_args(c, d->build_slot, d->n_envs, a);
  a.lanes = p.lanes;
  a.block = p.block;
  v.d = *d;
  v.npad = serl_venv_npad(d->n_envs);
  if (k.rd) {      // the actor shape the forward passes read (lane_actor.h serl_actor_forward_lane32 / _lane_general; venv_wave_rollout.inc reads it the same way)
    a.d.state_dim = k.rd->state_dim; a.d.action_dim = k.rd->action_dim; a.d.hidden = k.rd->hidden;
    a.d.num_layers = k.rd->num_layers; a.d.activation = k.rd->activation;
  }
  if (k.wave) {      // (venv_wave.inc, venv_wave_rollout.inc)
    const SerlVwLaunchers &W = k_vw_launchers[code];
    const SerlVwrLaunchers &R = k_vwr_launchers[code];
    if (k.rd && k.nz) R.rollout_nz(a, v, *k.au, *k.rd, *k.nz, grid, stream);
    else if (k.rd) R.rollout(a, v, *k.au, *k.rd, grid, stream);
    else if (k.nz && k.au) W.step_auto_nz(a, v, *k.au, *k.nz, grid, stream);
    else if (k.nz) W.reset_nz(a, v, *k.nz, grid, stream);
    else if (k.au) W.step_auto(a, v, *k.au, grid, stream);
    else (k.step ? W.step : W.reset)(a, v, grid, stream);
  } else {
    const SerlLaunchers &L = serl_launchers(code);
    const SerlNzLaunchers &Z = k_nz_launchers[code];
    if (k.rd && k.nz) (k.general ? Z.rollout_general : Z.rollout)(a, v, *k.au, *k.rd, *k.nz, grid, stream);
    else if (k.rd) (k.general ? L.venv_rollout_general : L.venv_rollout)(a, v, *k.au, *k.rd, grid, stream);
    else if (k.nz && k.au) Z.step_auto(a, v, *k.au, *k.nz, grid, stream);
    else if (k.nz) Z.reset(a, v, *k.nz, grid, stream);
    else if (k.au) L.venv_step_auto(a, v, *k.au, grid, stream);
    else (k.step ? L.venv_step : L.venv_reset)(a, v, grid, stream);
  }
  HIP_TRY(hipGetLastError());
  serl_note_venv_launch(c, p.family, grid, p.block / 64, code);
  return SERL_OK;
}

static int serl_venv_reset_impl(const char *w, serl_ctx *c, const serl_venv_desc *d, const uint8_t *mask, double *obs, const serl_venv_noise_desc *nz,
                               void *stream_, bool wave)
{
  { const int rc_ = serl_venv_check(c, d, w); if (rc_ != SERL_OK) return rc_; }
  if (!obs) return fail(SERL_E_INVALID, std::string(w) + ": obs is NULL");
  HIP_TRY(hipSetDevice(c->device));
  VenvArgs v;
  memset(&v, 0, sizeof(v));
  v.mask = mask;
  v.obs = obs;
  SerlVenvCall k;
  k.nz = nz; k.wave = wave;
  return serl_venv_launch(c, d, v, (hipStream_t)stream_, k);
}

int serl_venv_reset(serl_ctx *c, const serl_venv_desc *d, const uint8_t *mask, double *obs, void *stream_)
{
  return serl_venv_reset_impl("serl_venv_reset", c, d, mask, obs, nullptr, stream_, false);
}

int serl_venv_reset_wave(serl_ctx *c, const serl_venv_desc *d, const uint8_t *mask, double *obs, void *stream_)
{
  return serl_venv_reset_impl("serl_venv_reset_wave", c, d, mask, obs, nullptr, stream_, true);
}

// what the serl_venv_*_noise entries refuse in `nz` (none of these checks reads the context)
static int serl_venv_noise_check(const std::string &w, const serl_venv_desc *d, const serl_venv_rollout_desc *rd, const serl_venv_noise_desc *nz)
{
  if (!nz) return fail(SERL_E_INVALID, w + ": nz is NULL");
  if (!nz->episode_count) return fail(SERL_E_INVALID, w + ": nz->episode_count is NULL");
  if ((nz->sensor != 0 && nz->sensor != 1) || (nz->action != 0 && nz->action != 1)) return fail(SERL_E_INVALID, w + ": nz->sensor / nz->action must be 0 or 1");
  if (d && d->sensor_noise && nz->sensor) return fail(SERL_E_INVALID, w + ": desc->sensor_noise together with nz->sensor");
  if (rd && rd->action_noise && nz->action) return fail(SERL_E_INVALID, w + ": ro->action_noise together with nz->action");
  if (!(nz->action_sd >= 0.0) || !(nz->action_clip >= 0.0)) return fail(SERL_E_INVALID, w + ": nz->action_sd / nz->action_clip < 0");
  return SERL_OK;
}

int serl_venv_noise_layout(int32_t *out, int32_t capacity)
{
#define SERL_OFF(m) (int32_t)offsetof(serl_venv_noise_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_venv_noise_desc), SERL_OFF(seed), SERL_OFF(episode_count), SERL_OFF(sensor), SERL_OFF(pad0),
                       SERL_OFF(sensor_bias), SERL_OFF(sensor_scale), SERL_OFF(action), SERL_OFF(pad1), SERL_OFF(action_sd), SERL_OFF(action_clip)};
#undef SERL_OFF
  const int32_t n = (int32_t)(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = v[i];
  return n;
}

int serl_venv_reset_noise(serl_ctx *c, const serl_venv_desc *d, const uint8_t *mask, double *obs, const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_reset_noise", d, nullptr, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_reset_impl("serl_venv_reset_noise", c, d, mask, obs, nz, stream_, false);
}

int serl_venv_reset_wave_noise(serl_ctx *c, const serl_venv_desc *d, const uint8_t *mask, double *obs, const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_reset_wave_noise", d, nullptr, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_reset_impl("serl_venv_reset_wave_noise", c, d, mask, obs, nz, stream_, true);
}

static int serl_venv_step_impl(const char *w, serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                              double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost, void *stream_, bool wave)
{
  { const int rc_ = serl_venv_check(c, d, w); if (rc_ != SERL_OK) return rc_; }
  if (!actions || !obs || !reward || !done) return fail(SERL_E_INVALID, std::string(w) + ": actions / obs / reward / done is NULL");
  if (actions_f64 != 0 && actions_f64 != 1) return fail(SERL_E_INVALID, std::string(w) + ": actions_f64 must be 0 (f32) or 1 (f64)");
  HIP_TRY(hipSetDevice(c->device));
  VenvArgs v;
  memset(&v, 0, sizeof(v));
  v.actions = actions; v.actions_f64 = actions_f64;
  v.obs = obs; v.reward = reward; v.done = done; v.x = x; v.ref = ref; v.t = t; v.cost = cost;
  SerlVenvCall k;
  k.step = true; k.wave = wave;
  return serl_venv_launch(c, d, v, (hipStream_t)stream_, k);
}

int serl_venv_step(serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                   double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost, void *stream_)
{
  return serl_venv_step_impl("serl_venv_step", c, d, actions, actions_f64, obs, reward, done, x, ref, t, cost, stream_, false);
}

int serl_venv_step_wave(serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                        double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost, void *stream_)
{
  return serl_venv_step_impl("serl_venv_step_wave", c, d, actions, actions_f64, obs, reward, done, x, ref, t, cost, stream_, true);
}

int serl_venv_auto_layout(int32_t *out, int32_t capacity)
{
#define SERL_OFF(m) (int32_t)offsetof(serl_venv_auto_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_venv_auto_desc), SERL_OFF(final_obs), SERL_OFF(ep_return), SERL_OFF(ep_length),
                       SERL_OFF(run_return), SERL_OFF(run_length), SERL_OFF(cursor), SERL_OFF(ref_pool), SERL_OFF(pool_rows), SERL_OFF(pad0)};
#undef SERL_OFF
  const int32_t n = (int32_t)(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = v[i];
  return n;
}

static int serl_venv_step_auto_impl(const char *w, serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                                    double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                                    const serl_venv_auto_desc *au, const serl_venv_noise_desc *nz, void *stream_, bool wave = false)
{
  if (!c || !d || !au) return fail(SERL_E_INVALID, std::string(w) + ": NULL argument");
  if (au->ref_pool && d->ref) return fail(SERL_E_INVALID, std::string(w) + ": ref_pool together with desc->ref");
  if (au->ref_pool && au->pool_rows < 1) return fail(SERL_E_INVALID, std::string(w) + ": pool_rows < 1");
  serl_venv_desc dd = *d;
  if (au->ref_pool) { dd.ref_spec = au->ref_pool; dd.ref_spec_stride = 1; }      // (the kernel reads the pool: desc->ref_spec may be NULL)
  { const int rc_ = serl_venv_check(c, &dd, w); if (rc_ != SERL_OK) return rc_; }
  if (!actions || !obs || !reward || !done) return fail(SERL_E_INVALID, std::string(w) + ": actions / obs / reward / done is NULL");
  if (!au->final_obs || !au->ep_return || !au->ep_length || !au->run_return || !au->run_length || !au->cursor)
    return fail(SERL_E_INVALID, std::string(w) + ": final_obs / ep_return / ep_length / run_return / run_length / cursor is NULL");
  if (actions_f64 != 0 && actions_f64 != 1) return fail(SERL_E_INVALID, std::string(w) + ": actions_f64 must be 0 (f32) or 1 (f64)");
  HIP_TRY(hipSetDevice(c->device));
  VenvArgs v;
  memset(&v, 0, sizeof(v));
  v.actions = actions; v.actions_f64 = actions_f64;
  v.obs = obs; v.reward = reward; v.done = done; v.x = x; v.ref = ref; v.t = t; v.cost = cost;
  SerlVenvCall k;
  k.step = true; k.au = au; k.nz = nz; k.wave = wave;
  return serl_venv_launch(c, &dd, v, (hipStream_t)stream_, k);
}

int serl_venv_step_auto(serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                        double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                        const serl_venv_auto_desc *au, void *stream_)
{
  return serl_venv_step_auto_impl("serl_venv_step_auto", c, d, actions, actions_f64, obs, reward, done, x, ref, t, cost, au, nullptr, stream_);
}

int serl_venv_step_auto_noise(serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                              double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                              const serl_venv_auto_desc *au, const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_step_auto_noise", d, nullptr, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_step_auto_impl("serl_venv_step_auto_noise", c, d, actions, actions_f64, obs, reward, done, x, ref, t, cost, au, nz, stream_);
}

int serl_venv_step_auto_wave(serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                             double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                             const serl_venv_auto_desc *au, void *stream_)
{
  return serl_venv_step_auto_impl("serl_venv_step_auto_wave", c, d, actions, actions_f64, obs, reward, done, x, ref, t, cost, au, nullptr, stream_, true);
}

int serl_venv_step_auto_wave_noise(serl_ctx *c, const serl_venv_desc *d, const void *actions, int32_t actions_f64, double *obs,
                                   double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                                   const serl_venv_auto_desc *au, const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_step_auto_wave_noise", d, nullptr, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_step_auto_impl("serl_venv_step_auto_wave_noise", c, d, actions, actions_f64, obs, reward, done, x, ref, t, cost, au, nz, stream_, true);
}

int serl_venv_last_info(serl_ctx *c, int32_t out[4])
{
  if (!c || !out) return fail(SERL_E_INVALID, "serl_venv_last_info: NULL argument");
  if (c->last_venv_info[0] == SERL_FAMILY_NONE) return fail(SERL_E_INVALID, "serl_venv_last_info: no env call recorded");
  for (int i = 0; i < 4; ++i) out[i] = c->last_venv_info[i];
  return SERL_OK;
}

int serl_venv_rollout_layout(int32_t *out, int32_t capacity)
{
#define SERL_OFF(m) (int32_t)offsetof(serl_venv_rollout_desc, m)
  const int32_t v[] = {(int32_t)sizeof(serl_venv_rollout_desc), SERL_OFF(state_dim), SERL_OFF(action_dim), SERL_OFF(hidden), SERL_OFF(num_layers),
                       SERL_OFF(activation), SERL_OFF(n_members), SERL_OFF(weights), SERL_OFF(weight_stride), SERL_OFF(member_of_env),
                       SERL_OFF(n_steps), SERL_OFF(pad0), SERL_OFF(action_noise), SERL_OFF(obs), SERL_OFF(actions), SERL_OFF(reward), SERL_OFF(done),
                       SERL_OFF(final_obs), SERL_OFF(ep_return), SERL_OFF(ep_length), SERL_OFF(x), SERL_OFF(ref), SERL_OFF(t), SERL_OFF(cost),
                       SERL_OFF(transitions)};
#undef SERL_OFF
  const int32_t n = (int32_t)(sizeof(v) / sizeof(v[0]));
  for (int32_t i = 0; out && i < n && i < capacity; ++i) out[i] = v[i];
  return n;
}

// serl_venv_rollout* in one order: the descriptors (none of these checks reads the context), the kernel's shape contract (serl_shapes.h: the lane-32
// kernel's, or with `general` that of the general and wave kernels), the weights and the auto-reset descriptor, the env descriptor; then the launch
static int serl_venv_rollout_call(const char *what, serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd,
                                  const serl_venv_noise_desc *nz, void *stream_, bool general, bool wave)
{
  const std::string w(what);
  if (!c || !d || !au || !rd) return fail(SERL_E_INVALID, w + ": NULL argument");
  if (!rd->obs || !rd->weights) return fail(SERL_E_INVALID, w + ": obs / weights is NULL");
  if (rd->n_steps < 1) return fail(SERL_E_INVALID, w + ": n_steps < 1");
  if (rd->n_members < 1) return fail(SERL_E_INVALID, w + ": n_members < 1");
  const SerlShape sv = serl_shape_of(general ? SERL_SHAPE_VENV_ROLLOUT_GENERAL : SERL_SHAPE_VENV_ROLLOUT, rd->state_dim, rd->action_dim, rd->hidden, rd->num_layers,
                                     rd->activation, serl_shape_env(d->env_config, d->incremental));
  if (sv.why != SERL_SHAPE_WHY_TAKES) return serl_refuse(w, sv);
  if (rd->weight_stride < (int64_t)serl_param_count(rd->state_dim, rd->hidden, rd->num_layers, rd->action_dim) || (rd->weight_stride & 3) != 0 ||
      ((uintptr_t)rd->weights & 15) != 0)
    return fail(SERL_E_INVALID, w + ": weight_stride below the parameter count or not a multiple of 4 floats, or weights not 16-byte aligned");
  if (au->ref_pool && d->ref) return fail(SERL_E_INVALID, w + ": ref_pool together with desc->ref");
  if (au->ref_pool && au->pool_rows < 1) return fail(SERL_E_INVALID, w + ": pool_rows < 1");
  if (!au->run_return || !au->run_length || !au->cursor) return fail(SERL_E_INVALID, w + ": run_return / run_length / cursor is NULL");
  serl_venv_desc dd = *d;
  if (au->ref_pool) { dd.ref_spec = au->ref_pool; dd.ref_spec_stride = 1; }
  { const int rc_ = serl_venv_check(c, &dd, w.c_str()); if (rc_ != SERL_OK) return rc_; }
  HIP_TRY(hipSetDevice(c->device));
  VenvArgs v;
  memset(&v, 0, sizeof(v));
  SerlVenvCall k;
  k.step = true; k.au = au; k.rd = rd; k.general = general; k.nz = nz; k.wave = wave;
  return serl_venv_launch(c, &dd, v, (hipStream_t)stream_, k);
}

int serl_venv_rollout(serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd, void *stream_)
{
  return serl_venv_rollout_call("serl_venv_rollout", c, d, au, rd, nullptr, stream_, false, false);
}

int serl_venv_rollout_noise(serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd,
                            const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_rollout_noise", d, rd, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_rollout_call("serl_venv_rollout_noise", c, d, au, rd, nz, stream_, false, false);
}

int serl_venv_rollout_general(serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd, void *stream_)
{
  return serl_venv_rollout_call("serl_venv_rollout_general", c, d, au, rd, nullptr, stream_, true, false);
}

int serl_venv_rollout_general_noise(serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd,
                                    const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_rollout_general_noise", d, rd, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_rollout_call("serl_venv_rollout_general_noise", c, d, au, rd, nz, stream_, true, false);
}

int serl_venv_rollout_wave(serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd, void *stream_)
{
  return serl_venv_rollout_call("serl_venv_rollout_wave", c, d, au, rd, nullptr, stream_, true, true);
}

int serl_venv_rollout_wave_noise(serl_ctx *c, const serl_venv_desc *d, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *rd,
                                 const serl_venv_noise_desc *nz, void *stream_)
{
  { const int rc_ = serl_venv_noise_check("serl_venv_rollout_wave_noise", d, rd, nz); if (rc_ != SERL_OK) return rc_; }
  return serl_venv_rollout_call("serl_venv_rollout_wave_noise", c, d, au, rd, nz, stream_, true, true);
}

// ---- the launch planner on the host (include/serl_amd.h): no context, no device ------------------------------------------------------
static SerlCaps serl_caps_of(const int32_t v[7]) { return SerlCaps{v[0], v[1], v[2], v[3], v[4], v[5], v[6]}; }

static int serl_plan_out(const SerlPlan &p, int32_t out[16])
{
  for (int i = 0; i < 16; ++i) out[i] = 0;
  if (p.status != SERL_OK) return fail(p.status, p.message);
  const int32_t v[16] = {p.family, p.grid, p.per_team, p.queue, p.actor_waves, p.streamed, p.launches, -1,
                         p.block, p.lanes, p.q0, p.regroup, p.mail_bytes, p.timed, p.chunk, 0};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
  return SERL_OK;
}

int serl_host_plan_rollout(const int32_t caps[7], const serl_rollout_desc *desc, int32_t noise, int32_t out[16])
{
  if (!caps || !desc || !out || caps[0] < 1 || desc->n_episodes < 1) return fail(SERL_E_INVALID, "serl_host_plan_rollout: bad argument");
  const SerlCaps c = serl_caps_of(caps);
  int hint = SERL_KERNEL_AUTO;
  const char *message = "";
  const int rc = serl_plan_check(&c, desc, &hint, &message);
  if (rc != SERL_OK) { for (int i = 0; i < 16; ++i) out[i] = 0; return fail(rc, message); }
  return serl_plan_out(serl_plan_rollout(&c, desc, hint, noise), out);
}

int serl_host_plan_rollout_regrouped(const int32_t caps[7], const serl_rollout_desc *desc, int32_t noise, int32_t out[16])
{
  if (!caps || !desc || !out || caps[0] < 1 || desc->n_episodes < 1) return fail(SERL_E_INVALID, "serl_host_plan_rollout_regrouped: bad argument");
  const SerlCaps c = serl_caps_of(caps);
  int hint = SERL_KERNEL_AUTO;
  const char *message = "";
  const int rc = serl_plan_check(&c, desc, &hint, &message);
  if (rc != SERL_OK) { for (int i = 0; i < 16; ++i) out[i] = 0; return fail(rc, message); }
  return serl_plan_out(serl_plan_rollout_regrouped(&c, desc, hint, noise), out);
}

int serl_host_plan_dyn(const int32_t caps[7], int32_t n_episodes, int32_t lanes_per_wave, int32_t kernel_hint, int32_t out[16])
{
  if (!caps || !out || caps[0] < 1 || n_episodes < 1) return fail(SERL_E_INVALID, "serl_host_plan_dyn: bad argument");
  const SerlCaps c = serl_caps_of(caps);
  return serl_plan_out(serl_plan_dyn(&c, n_episodes, lanes_per_wave, kernel_hint), out);
}

int serl_host_plan_multi(int32_t num_cus, int32_t n, const int32_t *episodes, int32_t place, int32_t *grids, int32_t *queue, int32_t *place_out)
{
  if (num_cus < 1 || n < 1 || n > SERL_MIXED_MAX || !episodes || !grids || !queue || !place_out) return fail(SERL_E_INVALID, "serl_host_plan_multi: bad argument");
  for (int k = 0; k < n; ++k) if (episodes[k] < 1) return fail(SERL_E_INVALID, "serl_host_plan_multi: bad argument");
  serl_plan_multi(num_cus, n, episodes, place, grids, queue, place_out);
  return SERL_OK;
}

// ---- which kernel takes an actor shape (include/serl_amd.h): the predicates of serl_shapes.h, no device ---------------------------------
int serl_shape_query(const serl_ctx *c, int32_t kernel, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t activation,
                     int32_t batch, int64_t lds_bytes, int32_t *why)
{
  const char *who = serl_shape_who(kernel);
  const SerlShape v = serl_shape_fit(serl_shape_of(kernel, state_dim, action_dim, hidden, num_layers, activation, batch), c ? c->lds_per_block : lds_bytes);
  if (why) *why = v.why;
  return v.why == SERL_SHAPE_WHY_TAKES ? SERL_OK : serl_refuse(who ? who : "serl_shape_query", v);
}

/* development aid (SERL_PROFILE=1): shader-clock cycles wave 0 of workgroup 0 spent in the actor forward, the
 * dynamics step and the env bookkeeping during the last serl_rollout, and its number of env steps */
int serl_debug_profile(serl_ctx *c, unsigned long long out[32])
{
  if (!c || !out || !c->prof) return fail(SERL_E_INVALID, "serl_debug_profile: profiling not enabled (SERL_PROFILE=1)");
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, c->prof, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return SERL_OK;
}

int serl_debug_mixed_placement(serl_ctx *c, int32_t out[4])
{
  if (!c || !out) return fail(SERL_E_INVALID, "serl_debug_mixed_placement: NULL argument");
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!c->mixed_state || c->mixed_last < 0) return SERL_OK;          // no launch, or SERL_MIXED_PLACE=0
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());
  int32_t h[SERL_MIXED_STATE];
  HIP_TRY(hipMemcpy(h, c->mixed_state + (size_t)c->mixed_last * SERL_MIXED_STATE, sizeof(h), hipMemcpyDeviceToHost));
  out[0] = c->env_mixed_place == 1 ? 2 : h[SERL_MIXED_UNITS + 1]; out[1] = h[SERL_MIXED_UNITS];
  for (int u = 0; u < SERL_MIXED_UNITS; ++u) { out[2] += h[u] == 2; out[3] += h[u] == 1; }
  return SERL_OK;
}

int serl_last_rollout_ms(serl_ctx *c, float *ms)
{
  if (!c || !ms || !c->timed) return fail(SERL_E_INVALID, "serl_last_rollout_ms: no rollout recorded");
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return SERL_OK;
}

int serl_last_rollout_info(serl_ctx *c, int32_t out[8])
{
  if (!c || !out) return fail(SERL_E_INVALID, "serl_last_rollout_info: NULL argument");
  if (c->last_info[0] == SERL_FAMILY_NONE) return fail(SERL_E_INVALID, "serl_last_rollout_info: no rollout recorded");
  for (int i = 0; i < 8; ++i) out[i] = c->last_info[i];
  return SERL_OK;
}

int serl_last_rollout_weights(serl_ctx *c, int64_t out[4])
{
  if (!c || !out) return fail(SERL_E_INVALID, "serl_last_rollout_weights: NULL argument");
  if (c->last_info[0] == SERL_FAMILY_NONE) return fail(SERL_E_INVALID, "serl_last_rollout_weights: no rollout recorded");
  for (int i = 0; i < 4; ++i) out[i] = c->last_weights[i];
  return SERL_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// SSNE weight-tensor edits (base/core/mod_neuro_evo.py) -- elementwise / row kernels
// ---------------------------------------------------------------------------------------------
__global__ void ga_clone_kernel(float *w, int64_t stride, int32_t P, const int32_t *src, const int32_t *dst, int32_t n)
{
  const int pair = blockIdx.y;
  if (pair >= n) return;
  const float *s = w + (size_t)src[pair] * stride;
  float *d = w + (size_t)dst[pair] * stride;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) d[i] = s[i];
}

// ops[i] = {offset, length, dir}; applied IN ORDER (later ops see earlier ones, like the reference's
// sequential row copies), one workgroup, threads stride over the row.
__global__ void ga_crossover_kernel(float *w, int64_t stride, int32_t ma, int32_t mb, const int32_t *ops, int32_t n_ops)
{
  float *a = w + (size_t)ma * stride, *b = w + (size_t)mb * stride;
  for (int o = 0; o < n_ops; ++o) {
    const int off = ops[3 * o], len = ops[3 * o + 1], dir = ops[3 * o + 2];
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
      if (dir == 0) a[off + i] = b[off + i]; else b[off + i] = a[off + i];
    }
    __syncthreads();
  }
}

// Sequential sparse edits of one member (edits may hit the same weight twice; order matters).
// kind 0: w += z * (strength * w)   [random.gauss(0, strength*w) = z*sigma]   kind 1: w = z
// followed by the reference's hard clamp to +-1e6 (mod_neuro_evo.py:57-59,366): torch.clamp keeps a NaN, so the clamp is two
// comparisons (fminf(fmaxf(v, lo), hi) returns lo for a NaN: a diverged actor would come back finite).
__global__ void ga_mutate_kernel(float *w, int64_t stride, int32_t member, const int32_t *idx, const int32_t *kind,
                                 const float *z, const float *strength, int32_t n)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float *p = w + (size_t)member * stride;
  for (int i = 0; i < n; ++i) {
    float v = p[idx[i]];
    if (kind[i] == 0) v = v + z[i] * (strength[i] * v); else v = z[i];
    v = v > 1000000.0f ? 1000000.0f : (v < -1000000.0f ? -1000000.0f : v);
    p[idx[i]] = v;
  }
}

__global__ void ga_scaled_perturb_kernel(float *w, int64_t stride, int32_t member, const int32_t *seg_off,
                                         const int32_t *seg_len, int32_t n_seg, const float *delta, const float *scaling)
{
  float *p = w + (size_t)member * stride;
  int base = 0;
  for (int s = 0; s < n_seg; ++s) {
    const int off = seg_off[s], len = seg_len[s];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x)
      p[off + i] = p[off + i] + delta[base + i] / scaling[base + i];
    base += len;
  }
}

extern "C" {

int serl_ga_clone(serl_ctx *c, float *weights, int64_t stride, int32_t P, const int32_t *src, const int32_t *dst,
                  int32_t n, void *stream)
{
  if (!c || !weights || !src || !dst || n < 0 || P <= 0) return fail(SERL_E_INVALID, "serl_ga_clone: bad argument");
  if (n == 0) return SERL_OK;
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(ga_clone_kernel, dim3((P + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, weights, stride, P, src, dst, n);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

int serl_ga_crossover(serl_ctx *c, float *weights, int64_t stride, int32_t ma, int32_t mb, const int32_t *ops,
                      int32_t n_ops, void *stream)
{
  if (!c || !weights || (!ops && n_ops > 0) || n_ops < 0) return fail(SERL_E_INVALID, "serl_ga_crossover: bad argument");
  if (n_ops == 0) return SERL_OK;
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(ga_crossover_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, weights, stride, ma, mb, ops, n_ops);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

int serl_ga_mutate(serl_ctx *c, float *weights, int64_t stride, int32_t member, const int32_t *idx, const int32_t *kind,
                   const float *z, const float *strength, int32_t n, void *stream)
{
  if (!c || !weights || n < 0 || (n > 0 && (!idx || !kind || !z || !strength))) return fail(SERL_E_INVALID, "serl_ga_mutate: bad argument");
  if (n == 0) return SERL_OK;
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(ga_mutate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, weights, stride, member, idx, kind, z, strength, n);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

int serl_ga_scaled_perturb(serl_ctx *c, float *weights, int64_t stride, int32_t member, const int32_t *seg_offset,
                           const int32_t *seg_length, int32_t n_seg, const float *delta, const float *scaling, void *stream)
{
  if (!c || !weights || !seg_offset || !seg_length || !delta || !scaling || n_seg <= 0)
    return fail(SERL_E_INVALID, "serl_ga_scaled_perturb: bad argument");
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(ga_scaled_perturb_kernel, dim3(32), dim3(256), 0, (hipStream_t)stream, weights, stride, member,
                     seg_offset, seg_length, n_seg, delta, scaling);
  HIP_TRY(hipGetLastError());
  return SERL_OK;
}

}  // extern "C"

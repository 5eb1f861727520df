/* serl_amd.h -- C ABI of the MI355X-native population-rollout fitness evaluator for SERL.
 *
 * Drop-in boundary.  The reference has no FFI for this path: its seam is Python
 * (`Agent.evaluate`, base/core/agent.py:63-138, driven by the GA loop at :229-256) on top of the
 * SWIG surface of its native dynamics library,
 *       void initialize(void);  void step(real_T *cmd, real_T *out);  void ..._terminate(void);
 * (DWARF citation_to_python.h:1600-1604; envs/h2000_v90/citation.py:65-72).  This library replaces
 * that whole inner loop -- actor MLP forward (base/core/genetic_agent.py:104-109,
 * base/core/mod_utils.py:39-50) -> CitationEnv.step (envs/phlabenv.py:430-482) -> native step() ->
 * reward/cost/bounds (envs/phlabenv.py:347-399) -- with one fused HIP kernel batched over episodes.
 *
 * Conventions: every entry point returns 0 on success or a negative SERL_E_* code and never
 * throws; `serl_last_error()` returns a thread-local message.  All array arguments of
 * `serl_rollout` / `serl_ga_*` are DEVICE pointers owned by the caller (PyTorch allocates them);
 * the context owns only the read-only model tables it uploaded.  Calls are asynchronous on the
 * `hipStream_t` passed as `void *stream` (NULL = default stream); the caller synchronises.
 * The CPU oracle (oracle/rollout_ref.c, test infrastructure) implements `serl_oracle_rollout` with
 * the same descriptor and HOST pointers.
 */
#ifndef SERL_AMD_H
#define SERL_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SERL_ABI_VERSION 9

enum serl_error {
  SERL_OK = 0,
  SERL_E_INVALID = -1,      /* bad argument / descriptor */
  SERL_E_HIP = -2,          /* HIP runtime error (message in serl_last_error) */
  SERL_E_UNSUPPORTED = -3,  /* network shape / build variant not compiled in */
  SERL_E_NOMEM = -4
};

/* activation_actor of base/core/mod_utils.py:14-18 ('relu' IS LeakyReLU(0.01) there) */
enum serl_activation { SERL_ACT_TANH = 0, SERL_ACT_ELU = 1, SERL_ACT_LEAKY_RELU = 2 };

/* code variants of the dynamics library (14 build dirs = 5 code variants) */
enum serl_dyn_code { SERL_DYN_NOMINAL = 0, SERL_DYN_ICE = 1, SERL_DYN_CG_TIMED = 2, SERL_DYN_GUST = 3,
                     SERL_DYN_TEST = 4 };

typedef struct serl_ctx serl_ctx;

/* Tables + post-initialize() state image of ONE dynamics build (what the reference's
 * initialize() @0xb4e0 sets up).  HOST pointers; copied by serl_ctx_load_build. */
typedef struct serl_build_desc {
  int32_t code;            /* enum serl_dyn_code */
  int32_t n_ro;            /* number of f64 in ro[] */
  uint64_t ro_base;        /* virtual address of ro[0] in the reference binary (.rodata start) */
  const double *ro;        /* .rodata as f64: rtConstP aero tables, rtConstB, literal pool */
  const double *t3;        /* table3 S-function parameters P1[3] P2[4] P3[3] P4[36] = 46 */
  const double *x0;        /* rtX after initialize(): 19 continuous states */
  const double *dw0;       /* rtDW after initialize(): 31 f64 (IWORK in the last 12 bytes) */
  double dt;               /* fixed step, 0.01 */
} serl_build_desc;

/* Per-episode actuator-fault row (envs/{be,jr,sa,se}/citation.py:71-79): what the PLANT sees is
 *   cmd[0] = clip(cmd[0] * elev_gain, -elev_clip, +elev_clip)
 *   cmd[1] = clip(cmd[1], -ail_clip, +ail_clip)
 *   cmd[2] = rudder_jam_on ? rudder_jam : cmd[2]
 * while the logged action (env.last_u) stays the commanded one.  Nominal row: {1, +inf, +inf, 0, 0}. */
typedef struct serl_fault_row {
  double elev_gain, elev_clip, ail_clip, rudder_jam_on, rudder_jam, pad0, pad1, pad2;
} serl_fault_row;

/* A reference signal of one episode as PARAMETERS instead of a table: theta and phi are
 * `signals.SmoothedStepSequence(times, amplitudes, smooth_width)` objects (call sites envs/phlabenv.py:303-345,
 * base/evaluate.py:173-180, base/evaluation_utils.py:51), beta is Const(0): at the env's accumulated time t
 *   i = last index with t >= times[i] (none: the channel is 0);  prev = i ? amps[i-1] : 0;  s = min((t - times[i]) / w, 1)
 *   v = prev + (amps[i] - prev) * (1 - cos(pi * s)) / 2                                      [degrees]
 *   ref = (pi/180) * [v_theta + (0 <= t <= t_max ? trim_deg : 0),  v_phi,  0]
 * cos(pi s) is evaluated with + - * only (det_cospi: reflection to [0, 1/4], Taylor polynomials of cos / sin through
 * x^20 / x^21 in Horner form) so that the kernels and the CPU oracle agree bit for bit; against a libm cosine the
 * reference value differs by <= 2 ulp.  Per env step this replaces the 24 B read of ref[k] by arithmetic.
 * Contract of a row (the library does not read rows on the host; serl_amd.refsignals.check_specs enforces it for the Python callers):
 *   0 <= n_theta, n_phi <= SERL_REF_MAX_STEPS;  w_theta, w_phi finite and > 0 (at w = 0 the formula above is 0 / 0 on the step, where
 *   the kernels' `s < 1 ? s : 1` gives the level);  t_*[0 .. n) finite and NON-DECREASING (ties are legal: the last of tied steps is
 *   `i`, and prev is the amplitude of the step hit before it -- for non-decreasing times that is amps[i-1], as written above; for
 *   decreasing times it is not, and `signals` would blend from another level);  a_*[0 .. n) and trim_deg finite.
 *   Entries [n .. SERL_REF_MAX_STEPS) of the four arrays are NOT USED: they may hold anything, NaN included. */
#define SERL_REF_MAX_STEPS 8
typedef struct serl_ref_spec {
  int32_t n_theta, n_phi;            /* number of steps of each channel, <= SERL_REF_MAX_STEPS */
  double w_theta, w_phi;             /* smooth widths, seconds */
  double trim_deg;                   /* theta trim (envs/phlabenv.py:202,319-320,344) */
  double t_theta[SERL_REF_MAX_STEPS], a_theta[SERL_REF_MAX_STEPS];
  double t_phi[SERL_REF_MAX_STEPS], a_phi[SERL_REF_MAX_STEPS];
} serl_ref_spec;

typedef struct serl_rollout_desc {
  /* -- actor network (base/core/genetic_agent.py:69-102).  f32 arithmetic, part of this ABI (the HIP kernels and the CPU
   *    oracle implement it bit for bit): a dot product is four interleaved partial sums p[j & 3] = fmaf(w[j], h[j],
   *    p[j & 3]) over ascending j, then bias + ((p0 + p1) + (p2 + p3)); a LayerNorm sum is a balanced pairwise tree per
   *    block of 16 consecutive rows (zero padded), the blocks added in order; mean = sum / H, std = sqrtf(sum((x-mean)^2)
   *    / (H - 1)), y = gamma * (x - mean) / (std + 1e-6f) + beta; tanh / ELU through det_tanhf / det_expm1f_neg
   *    (f64 + - x / only, rounded to f32 once).
   *    Linear(S,H) act, L x [Linear(H,H)
   *    LayerNorm(H) act], Linear(H,A) tanh.  weights: f32 [n_members][param_count], packed in
   *    state_dict order: W0[H][S] b0[H]  { Wl[H][H] bl[H] gamma_l[H] beta_l[H] } x L  Wo[A][H] bo[A] */
  int32_t state_dim, action_dim, hidden, num_layers, activation;
  int32_t n_members;
  const float *weights;
  int64_t weight_stride;            /* in floats, >= param_count */
  /* -- episodes */
  int32_t n_episodes;
  int32_t build_slot;               /* slot given to serl_ctx_load_build */
  const int32_t *member_of_episode; /* [n_episodes] */
  const serl_fault_row *faults;     /* [n_episodes] or NULL (nominal) */
  const double *ref;                /* reference signals, radians, sampled at the accumulated env
                                       time t_k (envs/phlabenv.py:347-349,473): [.., max_steps, 3] */
  int64_t ref_stride;               /* doubles between consecutive episodes' tables (0 = shared) */
  const double *err0;               /* [n_episodes][3] tracking error carried into obs0
                                       (envs/phlabenv.py:401-428 never clears self.error) or NULL=0 */
  const double *action_noise;       /* [rows][max_steps][3] pre-drawn clipped Gaussian noise
                                       (base/core/agent.py:90-93) or NULL */
  const int32_t *noise_row;         /* [n_episodes] row of action_noise an episode adds to its actions, -1 = none
                                       (a population evaluation and the RL actor's exploration episode share one
                                       launch); NULL = row e for every episode */
  const double *sensor_noise;       /* [rows][max_steps + 1][7] additive sensor noise of the `noise` / `gust` wrappers
                                       (envs/noise/citation.py:71-82, envs/gust/citation.py:72-86): bias + sd * randn,
                                       pre-drawn in the wrapper's draw order, for the channels p q r | alpha | beta |
                                       phi theta of what step() RETURNS (the plant state stays clean); entry 0 belongs
                                       to the step reset() takes, entry k + 1 to env step k.  NULL = none */
  const int32_t *sensor_row;        /* [n_episodes] row of sensor_noise, -1 = none; NULL = row e for every episode */
  const int32_t *tick0;             /* [n_episodes] model clock (clockTick0) the episode starts with, or NULL = 0.
                                       The reference's initialize() @0xb4e0 resets the states but NOT the model
                                       clock (rtM clockTick0/1 and t keep counting across episodes of one process;
                                       probed on the live library), which only matters to the time-switched builds
                                       cg_timed ("CG aft after 20 s") and gust: there every episode after the first
                                       of a process starts at tick0 = steps simulated so far (incl. one per reset) */
  double t_max;                     /* 80 (eval) / 20 (train) seconds */
  int32_t max_steps;                /* rows in ref / trace buffers; 8001 for t_max = 80 */
  int32_t lanes_per_wave;           /* 0 = auto: wave-cooperative kernels chosen from the episode count -- a team of eight
                                       wavefronts per episode while every episode can have a CU of its own (episodes <=
                                       CUs), two / four episodes per team up to 4 x CUs (hidden 32; other hidden sizes: two
                                       per team up to 2 x CUs, six team + two actor wavefronts), beyond that ONE launch of
                                       four-episode teams with a work queue (a lane group takes the next episode when its
                                       own ends) -- and from 80 x CUs episodes on (hidden 32) the lane-per-episode kernels with 64 episodes per wavefront --
                                       or one wavefront per episode; 1..64 = lane-per-episode kernels with that
                                       many episodes per wavefront (every code variant, attitude task only).  With
                                       kernel_hint SERL_KERNEL_LANEQ: the lanes per wavefront of the lane work-queue kernel, 0 = 64 */
  int32_t concurrent_episodes;      /* episodes of OTHER serl_rollout calls expected to run at the same time on other
                                       streams (mixed-build sweeps: one call per dynamics build); the kernel and the
                                       wavefronts per workgroup are chosen for n_episodes + concurrent_episodes so that
                                       the launches fit the GPU side by side.  0 = this call has the GPU to itself */
  int32_t kernel_hint;              /* enum serl_kernel_hint: SERL_KERNEL_AUTO (0) = chosen from the episode count as
                                       described at lanes_per_wave; the others force one of the wave-cooperative kernel
                                       families (tests and A/B measurements compare them: results are bit-identical).
                                       Ignored when lanes_per_wave > 0, except SERL_KERNEL_LANEQ (the lane-per-episode kernels
                                       behind a work queue: see the enum).  SERL_E_UNSUPPORTED when the forced kernel does not
                                       exist for the actor shape (two / four episodes per team, half: hidden 32 only) or the
                                       env configuration (LANEQ: attitude task only) */
  /* -- results (per episode) */
  double *fitness;                  /* sum of rewards incl. termination penalty */
  int32_t *length_steps;            /* number of env steps taken */
  double *length_t;                 /* info['t'] after the final increment */
  int32_t *cost_steps;              /* number of steps with get_cost() == 1 */
  /* -- optional traces (NULL = not exported) */
  double *actions;                  /* env.last_u per step:  [n_episodes][max_steps][3] */
  double *states;                   /* env.x per step:       [n_episodes][max_steps][12] */
  double *rewards;                  /* reward per step:      [n_episodes][max_steps] */
  float *transitions;               /* (obs7,a3,next_obs7,r,done,cost) f32 x20 per step:
                                       [n_episodes][max_steps][20]  (base/core/agent.py:101-112); other env
                                       configurations: 2 S + A + 3 floats per step, see env_config */
  /* -- reference generation in the kernel (NULL = table mode: `ref` is read) */
  const serl_ref_spec *ref_spec;    /* [n_episodes] (ref_spec_stride 1) or one shared spec (stride 0); `ref` may be NULL */
  int64_t ref_spec_stride;
  /* -- env configuration (CitationEnv(configuration, mode), envs/phlabenv.py:84-97,174-176,205-220,377-380,415-428,
   *    446-470); zeros = the attitude task every BASELINE configuration uses.
   *      env_config   SERL_ENV_ATTITUDE   A = 3 actions (de da dr), observed states x[0 1 2 4] (p q r alpha)
   *                   SERL_ENV_SYMMETRIC  A = 1 (de; one reference: theta), observed state x[1] (q)
   *                   SERL_ENV_FULL       A = 3, observed states x[0..9]
   *      incremental  the action is an actuator RATE: scaled to +-25 deg/s instead of +-10 deg, u = last_u + scaled * dt
   *                   (last_u = 0 at reset), and last_u is part of the observation
   *    observation = [error (A), observed states, last_u (A, incremental only)]; state_dim must equal its length and
   *    action_dim must equal A.  reward = -sum_i<A |clip(scaler_i * error_i, -1, 1)| / A.  The per-episode tables keep
   *    their 3-column layouts (ref, err0, action_noise, actions: the first A columns are used / written, the others
   *    are 0); a transition row is (obs S, action A, next_obs S, reward, done, cost) = 2 S + A + 3 floats.
   *    Configurations other than the default run on kernel instantiations of their own that read the widths from the
   *    descriptor (serl_rollout_teamx_kernel_<variant>: rounds of one-episode teams while the episodes fit two rounds of
   *    workgroups, i.e. <= 2 x CUs; serl_rollout_wavex_kernel_<variant>, one wavefront per episode, beyond). */
  int32_t env_config;
  int32_t incremental;
} serl_rollout_desc;

enum serl_env_config { SERL_ENV_ATTITUDE = 0, SERL_ENV_SYMMETRIC = 1, SERL_ENV_FULL = 2 };
/* serl_rollout_desc.kernel_hint -- which wave-cooperative kernel family runs the episodes (all bit-identical):
 *   TEAM   eight wavefronts = one episode (seven integrate, one runs the actor); rounds of CUs episodes
 *   TEAM2 / TEAM4   the same team carrying two / four episodes in lane groups of 32 / 16 (hidden 32)
 *   WAVE   one wavefront = one episode, up to four per workgroup
 *   HALF   one wavefront = two episodes (hidden 32)
 *   LANEQ  one LANE = one episode, and a lane whose episode ends takes the next one from a work queue (serl_rollout_laneq_kernel_<variant>): at most
 *          4 x CUs wavefronts of lanes_per_wave lanes (0 = 64) are launched -- four per workgroup, one workgroup per CU, scaled by the launch's share of
 *          the episodes when concurrent_episodes > 0 -- and the episodes beyond those lane slots wait behind a device counter.  The only hint that is
 *          not ignored when lanes_per_wave > 0.  Attitude task, every code variant, every actor shape; serl_rollout only (serl_rollout_multi and
 *          serl_dyn_open_loop refuse it).  serl_last_rollout_info reports family SERL_FAMILY_LANE and whether the queue was engaged.  Opt-in:
 *          SERL_KERNEL_AUTO never chooses it.
 *   LANEG  (hint 7) one LANE = one episode for EVERY actor shape: each live lane runs the whole forward pass of its own actor over its member's row of
 *          [n_members][weight_stride] (serl_rollout_laneg_kernel_<variant>: activations in private memory, no LDS, no regrouped copy, weights streamed),
 *          where the lane kernels of lanes_per_wave > 0 run up to 64 wavefront-wide passes per env step for any shape but hidden 32.  ceil(n_episodes /
 *          lanes) wavefronts of lanes_per_wave lanes (0 = 64), no work queue; like LANEQ it is not ignored when lanes_per_wave > 0.  Accepted by
 *          serl_rollout and serl_rollout_noise (serl_rollout_laneg_noise_kernel_<variant>); serl_rollout_multi and serl_dyn_open_loop refuse it.
 *          SERL_E_UNSUPPORTED, before anything is planned, unless: the attitude task (env_config SERL_ENV_ATTITUDE, incremental 0), state_dim 7,
 *          action_dim 3, hidden a multiple of 4 in 4 .. 128, num_layers 0 .. 16.  Every code variant.  serl_last_rollout_info reports family
 *          SERL_FAMILY_LANEG.  Opt-in: SERL_KERNEL_AUTO never chooses it (measured: profiles/rollout_laneg_timing.json). */
enum serl_kernel_hint { SERL_KERNEL_AUTO = 0, SERL_KERNEL_TEAM = 1, SERL_KERNEL_WAVE = 2, SERL_KERNEL_HALF = 3,
                        SERL_KERNEL_TEAM2 = 4, SERL_KERNEL_TEAM4 = 5, SERL_KERNEL_LANEQ = 6, SERL_KERNEL_LANEG = SERL_KERNEL_LANEQ + 1 };
/* length of the observation of a configuration (0 = invalid) and its number of actions */
int serl_env_state_dim(int env_config, int incremental);
int serl_env_action_dim(int env_config);

int serl_abi_version(void);
/* Layout self-check for bindings that mirror the structs by hand (ctypes, cgo ...): fills out[0 .. n) with
 *   sizeof(serl_rollout_desc), then offsetof of each of its members in declaration order,
 *   then sizeof(serl_build_desc), sizeof(serl_fault_row), sizeof(serl_ref_spec), sizeof(serl_replay_job),
 *   then (ABI v9) sizeof(serl_venv_desc) and offsetof of each of its members in declaration order
 * as this library was compiled, and returns the number of values (written or not: call with capacity 0 to size). */
int serl_abi_layout(int32_t *out, int32_t capacity);
/* number of f32 parameters of an actor: H*S+H + L*(H*H+3H) + A*H+A */
int serl_param_count(int state_dim, int hidden, int num_layers, int action_dim);
const char *serl_last_error(void);

int serl_ctx_create(int device, serl_ctx **out);
int serl_ctx_destroy(serl_ctx *ctx);
int serl_ctx_load_build(serl_ctx *ctx, int slot, const serl_build_desc *build);
/* Development overrides, read from the environment ONCE, by serl_ctx_create (the only getenv of the library):
 *   SERL_KERNEL=team|team2|team4|wave|half|laneq|laneg   kernel family for descriptors with kernel_hint == SERL_KERNEL_AUTO
 *   SERL_WAVES_PER_BLOCK=n                   wavefronts per workgroup of the one-wavefront kernels
 *   SERL_LANEQ_WAVES=n                       SERL_KERNEL_LANEQ: at most n wavefronts per launch instead of 4 x CUs (tests engage the work queue with a handful of episodes)
 *   SERL_PROFILE=1                           cycle counters for serl_debug_profile
 *   SERL_SPLIT_ACTOR=1                       one-episode teams with a streamed actor (hidden > 64): two actor wavefronts share the forward pass
 *   SERL_REMOTE_ACTOR=0                      one-episode teams with a streamed actor: the actor stays on the team's CU (default 1: a workgroup of its own on another CU
 *                                            while two workgroups per episode fit the GPU at once -- serl_rollout_teamr_kernel_<variant>)
 *   SERL_JITTER_SEED=n, SERL_JITTER_SITES=m  acted on only by the TEST-ONLY stress build of the team kernels (libserl_amd_jitter.so:
 *                                            poisoned LDS blackboards, seeded pauses around every hand-over; the product ignores them;
 *                                            a development build -DSERL_DEV_ROLE_MAP=1 reads SERL_JITTER_SITES as the role <-> wavefront map of
 *                                            the one-episode team kernels, a nibble per hardware wavefront: tools/sweep_roles.py) */

/* One population evaluation: all episodes of the descriptor, one fused kernel launch per call. */
int serl_rollout(serl_ctx *ctx, const serl_rollout_desc *desc, void *stream);
/* ABI v7.  A mixed-fault population (fault mode per episode, /root/reference/envs/phlabenv.py:114-165: the builds be / jr / sa / se / cg share the
 * nominal code on different tables, ice has code of its own) as ONE launch of ONE code object: `n` descriptors (2 .. 4), one per dynamics build,
 * each exactly what serl_rollout would take (its own build_slot, episodes, outputs; concurrent_episodes is ignored).  Results are those of n
 * separate serl_rollout calls, bit for bit.  Eligible: attitude task, hidden 32, code variants nominal / ice, kernel_hint AUTO, more than
 * 2 x CUs episodes together; otherwise SERL_E_UNSUPPORTED and nothing was launched (the caller falls back to one serl_rollout per descriptor,
 * side by side on streams of their own).  `descs` is an array of n descriptors, contiguous in HOST memory.  The launch places its workgroups so that
 * CUs which share an instruction cache run the same code variant (SERL_MIXED_PLACE=0|1|2, read by serl_ctx_create, selects the placement for A/B;
 * results do not depend on it). */
int serl_rollout_multi(serl_ctx *ctx, int32_t n, const serl_rollout_desc *descs, void *stream);

/* Dynamics only (test / micro-benchmark entry): per episode initialize() followed by T calls of the
 * reference's step(cmd) -- cmds f64 [n_episodes][T][10] -> states f64 [n_episodes][T][12] (device). */
int serl_dyn_open_loop(serl_ctx *ctx, int slot, int32_t n_episodes, int32_t T, const double *cmds,
                       double *states, int32_t lanes_per_wave, int32_t kernel_hint /* AUTO, TEAM or WAVE */, void *stream);

/* ---- ABI v9: the env step-wise -- a batched vector env (CitationEnv.reset / .step, envs/phlabenv.py:401-482) ------------------
 * For callers that drive the dynamics with a policy of their own (any torch module, a PID / MPC baseline, an RL library) instead of
 * the fused actor of serl_rollout.  One lane = one env; one launch per call covers all envs; nothing is allocated and nothing is
 * synchronised.  Env state lives in a caller-owned opaque DEVICE buffer of serl_venv_state_bytes(n_envs) bytes that must be
 * zero-filled before its first use: a zero state is a fresh env (carried error 0, model clock 0) that is not running -- stepping
 * it returns zeros and done = 1 until it is reset.  The glue is the fused kernels' (rollout_variant.inc / rollout_wave.inc):
 *   reset  initialize() -- the model clock keeps counting (see tick0) --, one step with a zero command (fault row applied), sensor
 *          noise entry 0, V0 = x[3], t = 0, k = 0, last_u = 0;  obs0 = [carried error (A), x[obs_idx], last_u (A, incremental)].
 *          The error is NOT cleared (envs/phlabenv.py:401-428 never clears self.error): a re-used env's obs0 carries its last error.
 *   step   action scaled as scale_action (envs/phlabenv.py:62-73) with the fused kernels' precision: f32 actions compute
 *          s = 0.5f * (a + 1.0f) in f32, then low + s * (high - low) in f64; f64 actions are f64 throughout.  The env does NOT
 *          clip (the reference's agent does, base/core/agent.py:93).  Incremental control: u = last_u + scaled * dt.  Fault row,
 *          step(), sensor noise entry k + 1, reference row k (or generated at the pre-increment t), reward / cost / bounds /
 *          penalty as envs/phlabenv.py:347-399, then t += dt, k += 1.
 *   done   done = bounds hit (envs/phlabenv.py:391-399) OR k == max_steps (the reference tables are exhausted).  A done env is
 *          FROZEN: stepping it returns its last obs, x, ref, t and cost with reward 0 and done = 1 and changes nothing until it
 *          is reset, so no step ever reads ref / sensor_noise past max_steps.  The reference env would keep integrating: a
 *          deliberate difference.  serl_venv_reset / serl_venv_step do not auto-reset; serl_venv_step_auto (below) does. */
typedef struct serl_venv_desc {
  int32_t n_envs;                   /* envs of the batch, >= 1 */
  int32_t build_slot;               /* slot given to serl_ctx_load_build: one dynamics build per env object */
  int32_t env_config;               /* enum serl_env_config, as serl_rollout_desc.env_config */
  int32_t incremental;              /* 1 = the action is an actuator rate (serl_rollout_desc.incremental) */
  int32_t state_dim, action_dim;    /* must equal serl_env_state_dim(env_config, incremental) / serl_env_action_dim(env_config) */
  int32_t max_steps;                /* rows of every env's ref table; sensor_noise rows hold max_steps + 1 entries */
  int32_t pad0;
  double t_max;                     /* episode length, seconds (bounds and termination penalty) */
  const serl_fault_row *faults;     /* [n_envs] or NULL (nominal) */
  const double *ref;                /* [.., max_steps, 3] radians, as serl_rollout_desc.ref; NULL when ref_spec is given */
  int64_t ref_stride;               /* doubles between consecutive envs' tables (0 = one shared table) */
  const serl_ref_spec *ref_spec;    /* [n_envs] (stride 1) or one shared spec (stride 0): references generated in the kernel, or NULL */
  int64_t ref_spec_stride;
  const double *sensor_noise;       /* [rows][max_steps + 1][7] additive sensor noise, as serl_rollout_desc.sensor_noise, or NULL */
  const int32_t *sensor_row;        /* [n_envs] row of sensor_noise, -1 = none; NULL = row e for env e */
  const double *err0;               /* serl_venv_reset only: [n_envs][3] error put into obs0 instead of the carried one, or NULL */
  const int32_t *tick0;             /* serl_venv_reset only: [n_envs] model clock to start from instead of the carried one, or NULL.
                                       The carried clock counts one tick per reset and one per step (initialize() does not reset
                                       clockTick0, see serl_rollout_desc.tick0); a fresh env starts at 0 */
  void *state;                      /* DEVICE, serl_venv_state_bytes(n_envs) bytes, zero-filled before first use; opaque */
} serl_venv_desc;
/* bytes of the state buffer of n_envs envs (SoA: [field][n_envs rounded up to 64]); 0 for n_envs < 1 */
int64_t serl_venv_state_bytes(int32_t n_envs);
/* reset the envs with mask[e] != 0 (mask: DEVICE u8 [n_envs], NULL = all).  obs: DEVICE f64 [n_envs][state_dim], written for
 * EVERY env: obs0 of the reset ones, the current observation of the others. */
int serl_venv_reset(serl_ctx *ctx, const serl_venv_desc *desc, const uint8_t *mask, double *obs, void *stream);
/* one env step of every env.  actions: DEVICE [n_envs][action_dim], f32 (actions_f64 = 0) or f64 (actions_f64 = 1).
 * Outputs (DEVICE): obs f64 [n_envs][state_dim], reward f64 [n_envs], done u8 [n_envs]; optional (NULL = not written):
 * x f64 [n_envs][12] (what step() returned, sensor noise included), ref f64 [n_envs][3] (theta, phi, beta reference of the step),
 * t f64 [n_envs] (info['t'], after the increment), cost i32 [n_envs] (get_cost of the step). */
int serl_venv_step(serl_ctx *ctx, const serl_venv_desc *desc, const void *actions, int32_t actions_f64, double *obs,
                   double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost, void *stream);

/* ---- auto-reset inside the step (SERL_ABI_VERSION stays 9: serl_abi_layout, serl_venv_desc, the state buffer and the two entry
 * points above are unchanged; this descriptor has a layout self-check of its own, serl_venv_auto_layout) -------------------------
 * serl_venv_step_auto is serl_venv_step for envs that restart themselves: a running env takes the step exactly as above, and if that
 * step ends its episode (bounds hit, or k == max_steps) the same launch then does what serl_venv_reset does for that env -- carried
 * error kept, the carried model clock takes the reset's tick, the same fault row, initialize() and one step with the zero command,
 * sensor-noise entry 0 of the env's table, V0 = x[3], t = 0, k = 0, last_u = 0 -- so the env is running again when the call returns.
 * The "same-step" convention of vector envs: obs is obs0 of the NEW episode; reward, done = 1, x, ref, t and cost are the terminal
 * step's; final_obs holds the terminal observation and ep_return / ep_length the finished episode's sum of rewards (f64,
 * ret = ret + reward in step order) and number of steps.  An env that did not finish gets final_obs = obs and leaves ep_return /
 * ep_length as they were.  An env that is not running (never reset) stays frozen exactly as in serl_venv_step, with final_obs =
 * obs: auto-reset restarts episodes, it does not start the first one.  desc->err0 / tick0 are not read.  Sensor-noise tables are
 * reused by the restarted episodes.  A wavefront in which some env finishes pays two dynamics steps in that call.
 *   references  desc->ref / desc->ref_spec as given: the restarted episode flies them again.  Or ref_pool: `pool_rows` specs per env,
 *               [n_envs][pool_rows]; the step reads row cursor[e] of env e and a restart advances the cursor to (cursor + 1) %
 *               pool_rows, so the pool recycles after pool_rows episodes.  With a pool desc->ref must be NULL and desc->ref_spec
 *               is not read (it may be NULL).
 *   run state   run_return / run_length / cursor are the caller's: zero them for the envs serl_venv_reset starts (the episode an
 *               explicit reset starts uses pool row 0).  They are not part of desc->state.  Without a pool the cursor counts restarts (wrapping
 *               to 0 after 2^31 - 1). */
typedef struct serl_venv_auto_desc {
  double *final_obs;                /* out [n_envs][state_dim]: the observation of this step in front of a restart */
  double *ep_return;                /* out [n_envs]: written where done */
  int32_t *ep_length;               /* out [n_envs]: written where done */
  double *run_return;               /* in / out [n_envs]: sum of rewards of the running episode */
  int32_t *run_length;              /* in / out [n_envs]: steps of the running episode */
  int32_t *cursor;                  /* in / out [n_envs]: pool row of the running episode */
  const serl_ref_spec *ref_pool;    /* [n_envs][pool_rows], or NULL: references from desc->ref / desc->ref_spec */
  int32_t pool_rows;                /* >= 1 with a pool */
  int32_t pad0;
} serl_venv_auto_desc;
/* layout self-check like serl_abi_layout: sizeof(serl_venv_auto_desc), then offsetof of each member in declaration order */
int serl_venv_auto_layout(int32_t *out, int32_t capacity);
/* arguments as serl_venv_step, all outputs of `au` required.  SERL_E_INVALID before any launch for a NULL argument, pool_rows < 1
 * with a pool, a pool together with desc->ref, actions_f64 other than 0 / 1. */
int serl_venv_step_auto(serl_ctx *ctx, const serl_venv_desc *desc, const void *actions, int32_t actions_f64, double *obs,
                        double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                        const serl_venv_auto_desc *au, void *stream);

/* ---- K policy-driven steps of persistent envs in one launch (SERL_ABI_VERSION stays 9: nothing above has moved; this descriptor has
 * a layout self-check of its own, serl_venv_rollout_layout) -----------------------------------------------------------------------------
 * serl_venv_rollout collects n_steps steps of experience from the envs of `desc` under a given policy: per env and step the actor
 * forward on the current observation (obsf[i] = (float)obs[i]; the arithmetic of serl_rollout_desc, bit for bit; every lane runs its
 * own actor on its member's plain row of `weights`), the action path of serl_rollout -- without noise the f32 action scaled as an f32
 * action of serl_venv_step; with action_noise an = clip((double)act + noise, -1, 1) scaled as an f64 action -- and then exactly the step
 * of serl_venv_step_auto, restart included.  The env state, `au`'s run state (run_return / run_length / cursor: read once, written once
 * per call) and the reference pool are those of serl_venv_step_auto: serl_venv_step / _step_auto may follow a rollout and vice versa.
 * Attitude task without rate control only (state_dim 7, action_dim 3), and the actor shape of the lane kernels only: hidden 32, any
 * num_layers >= 0 and activation.  Outputs are step-major, [n_steps][n_envs] rows; all but obs are optional (NULL = not written):
 *   obs          f64 [n_steps + 1][n_envs][7]  row 0: the observation the segment starts from; row k + 1: what serl_venv_step_auto returns
 *                                              after step k (obs0 of the new episode where done)
 *   actions      f64 [n_steps][n_envs][3]      the executed action in actor units: (double)act without noise, the clipped an with noise
 *   reward f64, done u8, final_obs f64 [..][7], x f64 [..][12], ref f64 [..][3], t f64, cost i32: as serl_venv_step_auto per step
 *   ep_return f64, ep_length i32 [n_steps][n_envs]: written where done only
 *   transitions  f32 [n_steps][n_envs][20]     (obs 7, executed action 3 as f32, final_obs 7, reward, fin, cost): the row of
 *                                              serl_rollout_desc.transitions; fin = bounds hit or t >= t_max, NOT the end of the tables
 * An env that was never reset stays frozen in every row as serl_venv_step_auto leaves it (reward 0, done 1, its obs, final_obs = obs);
 * its actions are 0 and its transition rows (obs, 0, obs, 0, 1, cost).  member_of_env indices are taken modulo n_members. */
typedef struct serl_venv_rollout_desc {
  int32_t state_dim, action_dim, hidden, num_layers, activation;   /* the actor, as serl_rollout_desc */
  int32_t n_members;                /* rows of weights, >= 1 */
  const float *weights;             /* DEVICE f32 [n_members][weight_stride], packed as serl_rollout_desc.weights, 16-byte aligned rows */
  int64_t weight_stride;            /* in floats, >= param_count, a multiple of 4 */
  const int32_t *member_of_env;     /* DEVICE [n_envs], or NULL: every env runs member 0 (one shared policy) */
  int32_t n_steps;                  /* K >= 1 */
  int32_t pad0;
  const double *action_noise;       /* DEVICE [n_steps][n_envs][3] added to the actor's output, or NULL */
  double *obs;
  double *actions;
  double *reward;
  uint8_t *done;
  double *final_obs;
  double *ep_return;
  int32_t *ep_length;
  double *x;
  double *ref;
  double *t;
  int32_t *cost;
  float *transitions;
} serl_venv_rollout_desc;
/* layout self-check: sizeof(serl_venv_rollout_desc), then offsetof of each member in declaration order */
int serl_venv_rollout_layout(int32_t *out, int32_t capacity);
/* Asynchronous on `stream`, one launch, no host synchronisation.  SERL_E_INVALID before any launch for a NULL argument, NULL obs or
 * weights, n_steps < 1, n_members < 1, an env other than the attitude task without rate control, an actor other than 7 -> 32 .. -> 3
 * (or num_layers < 0, an unknown activation, a weight_stride below the parameter count or not a multiple of 4), and for what
 * serl_venv_step_auto refuses in `desc` / `au` (run_return / run_length / cursor are required; au->final_obs is not used; au->ep_return /
 * ep_length, where given, receive the last finished episode's values as the same steps of serl_venv_step_auto would leave them). */
int serl_venv_rollout(serl_ctx *ctx, const serl_venv_desc *desc, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *ro,
                      void *stream);

/* serl_venv_rollout for every env configuration and actor shape: the same three descriptors (no member added, the layout functions and
 * SERL_ABI_VERSION unchanged), the same semantics, one launch of a second kernel whose actor keeps its activations in private memory.
 * state_dim / action_dim of `ro` must be those of the env configuration of `desc` (attitude 7 / 3, symmetric 2 / 1, full 13 / 3;
 * incremental adds action_dim observations, and the action is then a rate, integrated as serl_venv_step does); hidden a multiple of 4
 * in 4 .. 128, num_layers 0 .. 16, every activation.  Rows are [n_steps][n_envs][state_dim], [..][action_dim] and, for transitions,
 * [..][2 state_dim + action_dim + 3] = (obs, executed action, final_obs, reward, fin, cost), the row of serl_rollout_desc.transitions
 * in that configuration.  action_noise keeps its [n_steps][n_envs][3] layout; its first action_dim columns are read.
 * SERL_E_INVALID / SERL_E_UNSUPPORTED (hidden, num_layers out of range) before any launch: a NULL argument, NULL obs or weights, n_steps
 * < 1, n_members < 1, an actor that does not fit the env configuration, an unknown activation, a weight_stride below the parameter count
 * or not a multiple of 4, weights not 16-byte aligned, and what serl_venv_step_auto refuses in `desc` / `au`.  serl_venv_rollout itself
 * keeps its one shape: where both take a call they return the same bits. */
int serl_venv_rollout_general(serl_ctx *ctx, const serl_venv_desc *desc, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *ro,
                              void *stream);

/* ---- sensor and exploration noise drawn inside the env kernels (SERL_ABI_VERSION stays 9: nothing above has moved; this descriptor has
 * a layout self-check of its own, serl_venv_noise_layout) --------------------------------------------------------------------------------
 * A counter-based generator (csrc/serl_rng.h) replaces the pre-drawn tables: no table, no host draw, a fresh and reproducible realisation
 * per (seed, env, episode, step), and any single episode's noise can be written out again on demand (serl_venv_noise_fill).
 *   bits     Philox4x32-10, key = seed (low word, high word), counter = (env index, episode ordinal of that env, entry within the episode,
 *            stream << 16 | block); stream 0 = sensor, 1 = action
 *   uniform  from two words: k = (uint64)w0 << 20 | w1 >> 12, u = (2 k + 1) 2^-53 -- exact in f64, strictly inside (0, 1)
 *   normal   one Philox call = two uniforms = one Box-Muller pair: r = sqrt(-2 log u0), (s, c) = sincospi(2 u1), normals r c and r s
 *   sensor   blocks 0 .. 3 = 8 normals, the first 7 in channel order p q r | alpha | beta | phi theta; the addend of channel i is
 *            sensor_bias[i] + sensor_scale[i] z (multiply, then add).  Entry 0 belongs to the step of the reset, entry k + 1 to env step k:
 *            where the table path reads its row
 *   action   blocks 0 .. 1 = 4 normals, the first action_dim are used; the addend is clip(action_sd z, -action_clip, action_clip)
 *            (base/core/agent.py:90-93).  The entry is the env's in-episode step index, so two rollouts of K1 and K2 steps draw what one of
 *            K1 + K2 steps draws
 *   episode  episode_count[e] counts the episode starts of env e, explicit resets and in-kernel restarts alike; the running episode's
 *            ordinal is episode_count[e] - 1.  The caller owns the array (zeroed for fresh envs) and may save / restore it with the seed. */
typedef struct serl_venv_noise_desc {
  uint64_t seed;
  int32_t *episode_count;           /* DEVICE in / out [n_envs] */
  int32_t sensor;                   /* 1 = sensor noise from the generator (desc->sensor_noise must then be NULL); 0 = as desc says */
  int32_t pad0;
  double sensor_bias[7];
  double sensor_scale[7];
  int32_t action;                   /* 1 = exploration noise from the generator (ro->action_noise must then be NULL); 0 = as ro says */
  int32_t pad1;
  double action_sd;                 /* >= 0 */
  double action_clip;               /* >= 0 */
} serl_venv_noise_desc;
/* layout self-check: sizeof(serl_venv_noise_desc), then offsetof of each member in declaration order */
int serl_venv_noise_layout(int32_t *out, int32_t capacity);
/* serl_venv_reset / _step_auto / _rollout / _rollout_general with `nz` (required): one launch each of a second instantiation of the same
 * kernels.  Besides what their namesakes refuse, SERL_E_INVALID before any launch for a NULL nz or episode_count, desc->sensor_noise
 * together with nz->sensor, ro->action_noise together with nz->action, action_sd < 0 or action_clip < 0 (or NaN).  With nz->sensor = 0
 * and nz->action = 0 they compute what their namesakes compute (and still count episodes).  There is no serl_venv_step with `nz`. */
int serl_venv_reset_noise(serl_ctx *ctx, const serl_venv_desc *desc, const uint8_t *mask, double *obs, const serl_venv_noise_desc *nz,
                          void *stream);
int serl_venv_step_auto_noise(serl_ctx *ctx, const serl_venv_desc *desc, const void *actions, int32_t actions_f64, double *obs,
                              double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                              const serl_venv_auto_desc *au, const serl_venv_noise_desc *nz, void *stream);
int serl_venv_rollout_noise(serl_ctx *ctx, const serl_venv_desc *desc, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *ro,
                            const serl_venv_noise_desc *nz, void *stream);
int serl_venv_rollout_general_noise(serl_ctx *ctx, const serl_venv_desc *desc, const serl_venv_auto_desc *au,
                                    const serl_venv_rollout_desc *ro, const serl_venv_noise_desc *nz, void *stream);
/* What the env kernels draw, written out by the same device functions: row i of `out` holds `entries` consecutive entries, entry0[i]
 * onwards, of (nz->seed; env[i], episode[i]).  env / episode / entry0: DEVICE i32 [rows]; out: DEVICE [rows][entries][W];
 * nz->episode_count is not read.  mode 0: the raw Philox words of the sensor stream's four blocks followed by the action stream's two,
 * u32, W = 24;  1: the sensor stream's standard normals, f64, W = 7;  2: the sensor addends, f64, W = 7;  3: the action addends,
 * f64, W = 3.  SERL_E_INVALID for a NULL argument, rows or entries < 1, an unknown mode, action_sd / action_clip < 0 in mode 3. */
int serl_venv_noise_fill(serl_ctx *ctx, const serl_venv_noise_desc *nz, int32_t mode, int32_t rows, const int32_t *env,
                         const int32_t *episode, const int32_t *entry0, int32_t entries, void *out, void *stream);
/* The in-kernel actor of serl_venv_rollout / _rollout_general alone, one lane per env: actions f32 [n_envs][action_dim] = the forward pass of
 * the env's member (member_of_env modulo n_members, NULL = member 0) on obsf[i] = (float)obs[i], obs f64 [n_envs][state_dim] -- the bits those
 * kernels compute (hidden 32, state_dim 7, action_dim 3 runs serl_venv_rollout's forward, every other shape the general one).  Of `ro` only the actor
 * members are read (state_dim .. member_of_env); refusals as serl_venv_rollout_general's for them, and n_envs < 1.  The step loop of a device-noise
 * env uses it, so that it stays interchangeable with the kernels bit for bit. */
int serl_venv_actor_forward(serl_ctx *ctx, const serl_venv_rollout_desc *ro, int32_t n_envs, const double *obs, float *actions, void *stream);
/* The small-batch path of the step-wise env: the same calls with ONE WAVEFRONT PER ENV (csrc/venv_wave.inc) instead of one lane per env.  A lane flies
 * the whole model evaluation serially, so a lane call lasts one lane env step however few envs there are; here the evaluation's table look-ups and the 19
 * ODE5 states are spread over the wavefront's lanes (the wave rollout kernels' evaluation), 1 .. 4 wavefronts to a workgroup.  Timings of both families:
 * profiles/venv_wave_timing.json.  Arguments, semantics, outputs and refusals are those of the namesakes without `_wave` above, bit for bit in every
 * output.  The descriptors, serl_venv_state_bytes and the state buffer's layout are the same, and every output of a call of either family behind calls of
 * the other has been equal to an all-lane run's; of the opaque state, eleven i32 words are not those of an all-lane run: the eight interval hints of the lane
 * evaluation (which verifies a hint before it uses it) and the three words of the table3 interval cache, which the lane step walks from a work word it
 * does not initialise (csrc/venv_wave.inc).  A wave step leaves all eleven as it finds them, a wave reset stores initialize()'s image of the cache.
 * serl_amd.CitationVecEnv.rollout therefore does not run the lane rollout kernels on an env that steps through these entry points.  There is no serl_venv_step_wave with `nz`, as there is no serl_venv_step_noise. */
int serl_venv_reset_wave(serl_ctx *ctx, const serl_venv_desc *desc, const uint8_t *mask, double *obs, void *stream);
int serl_venv_step_wave(serl_ctx *ctx, const serl_venv_desc *desc, const void *actions, int32_t actions_f64, double *obs,
                        double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost, void *stream);
int serl_venv_step_auto_wave(serl_ctx *ctx, const serl_venv_desc *desc, const void *actions, int32_t actions_f64, double *obs,
                             double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                             const serl_venv_auto_desc *au, void *stream);
int serl_venv_reset_wave_noise(serl_ctx *ctx, const serl_venv_desc *desc, const uint8_t *mask, double *obs, const serl_venv_noise_desc *nz,
                               void *stream);
int serl_venv_step_auto_wave_noise(serl_ctx *ctx, const serl_venv_desc *desc, const void *actions, int32_t actions_f64, double *obs,
                                   double *reward, uint8_t *done, double *x, double *ref, double *t, int32_t *cost,
                                   const serl_venv_auto_desc *au, const serl_venv_noise_desc *nz, void *stream);
/* serl_venv_rollout_general / _general_noise with ONE WAVEFRONT PER ENV (csrc/venv_wave_rollout.inc): K policy-driven steps in one launch on the kernels of
 * the small-batch path.  The env's state and run state are loaded once and stored once, the tables are staged once, and the actor is the wave-cooperative
 * forward of the fused wave kernels (one hidden row per lane).  Arguments, descriptors (no member added), semantics, every output row and the refusals
 * before any launch are those of the namesakes without `_wave`, bit for bit; the state buffer is left as the same steps of serl_venv_step_auto_wave
 * leave it (the eleven opaque words above included: a restart inside the segment stores initialize()'s image of the table3 cache, nothing else touches
 * them), so these calls may follow and be followed by any call of either family.  serl_venv_last_info records SERL_FAMILY_WAVE, the grid and the wavefronts
 * per workgroup.  Timings against the step loop and the lane kernel: profiles/venv_rollout_wave_timing.json. */
int serl_venv_rollout_wave(serl_ctx *ctx, const serl_venv_desc *desc, const serl_venv_auto_desc *au, const serl_venv_rollout_desc *ro,
                           void *stream);
int serl_venv_rollout_wave_noise(serl_ctx *ctx, const serl_venv_desc *desc, const serl_venv_auto_desc *au,
                                 const serl_venv_rollout_desc *ro, const serl_venv_noise_desc *nz, void *stream);
/* ---- population rollouts with the sensor and exploration noise drawn inside the kernels (SERL_ABI_VERSION stays 9: nothing above has
 * moved; this descriptor has a layout self-check of its own, serl_rollout_noise_layout) -------------------------------------------------
 * serl_rollout with the generator of serl_venv_noise_desc in place of the pre-drawn tables desc->sensor_noise [rows][max_steps + 1][7] and
 * desc->action_noise [rows][max_steps][3].  Counter, stream, block and entry conventions are exactly those documented at
 * serl_venv_noise_desc: episode e draws with counter words (env[e], episode[e], entry, stream << 16 | block); sensor entry 0 belongs to
 * initialize()'s step and entry k + 1 to env step k, the action entry is the env step k, of which the first action_dim columns are used.
 * What serl_venv_noise_fill writes for (seed; env[e], episode[e]) with max_steps + 1 sensor entries (mode 2) is the table path's sensor
 * row of that episode, and with max_steps action entries (mode 3) its action row: both paths return the same bits.
 *   env / episode   counter words 0 and 1 per episode, so that a realisation does not depend on where an episode sits in a launch or on how
 *                   a caller groups its episodes into launches, and so that a caller can number its generations
 *   switches        with sensor = 1, desc->sensor_row[e] < 0 still means "episode e has no sensor noise" (NULL or >= 0: it draws); with
 *                   action = 1 the same holds for desc->noise_row (the RL actor's exploration episode riding a population launch)
 *   kernels         second instantiations of the lane-per-episode kernels (attitude task; csrc/family_lanern.hip) and of the
 *                   one-wavefront-per-episode kernels (every env configuration; csrc/family_wavern.hip).  desc->lanes_per_wave > 0 runs the
 *                   lane kernels; kernel_hint WAVE the wave / wavex kernels; AUTO the lane kernels wherever serl_rollout's AUTO picks them
 *                   (hidden 32, attitude task, alone on the GPU, >= 80 x CUs episodes) and the wave / wavex kernels otherwise.  The team,
 *                   half and work-queue kernels have no noise instantiation: between 4 x CUs and 80 x CUs episodes this path therefore runs
 *                   one wavefront per episode and not the team4 queue launch serl_rollout would choose. */
typedef struct serl_rollout_noise_desc {
  uint64_t seed;
  const int32_t *env;               /* DEVICE [n_episodes]: counter word 0 of episode e; NULL = e */
  const int32_t *episode;           /* DEVICE [n_episodes]: counter word 1 of episode e; NULL = 0 */
  int32_t sensor;                   /* 1 = sensor noise from the generator (desc->sensor_noise must then be NULL); 0 = as desc says */
  int32_t pad0;
  double sensor_bias[7];
  double sensor_scale[7];
  int32_t action;                   /* 1 = exploration noise from the generator (desc->action_noise must then be NULL); 0 = as desc says */
  int32_t pad1;
  double action_sd;                 /* >= 0 */
  double action_clip;               /* >= 0 */
} serl_rollout_noise_desc;
/* layout self-check: sizeof(serl_rollout_noise_desc), then offsetof of each member in declaration order */
int serl_rollout_noise_layout(int32_t *out, int32_t capacity);
/* Asynchronous on `stream`, one launch.  Besides everything serl_rollout refuses, SERL_E_INVALID before any launch for a NULL nz, nz->sensor
 * or nz->action other than 0 / 1, desc->sensor_noise together with nz->sensor, desc->action_noise together with nz->action, action_sd < 0
 * or action_clip < 0 (or NaN); SERL_E_UNSUPPORTED before any launch where the kernel hint -- desc->kernel_hint, or SERL_KERNEL=... for a
 * descriptor that says AUTO -- resolves to TEAM, TEAM2, TEAM4, HALF or LANEQ.  With nz->sensor = 0 and nz->action = 0 the call computes
 * what serl_rollout computes.  serl_last_rollout_info records the family (LANE / WAVE / WAVEX) as for serl_rollout.  serl_rollout_multi
 * takes no such descriptor. */
int serl_rollout_noise(serl_ctx *ctx, const serl_rollout_desc *desc, const serl_rollout_noise_desc *nz, void *stream);
/* serl_rollout (nz == NULL: no generator) / serl_rollout_noise (nz != NULL) of kernel_hint SERL_KERNEL_LANEG over a REGROUPED copy of the weights: in front
 * of the launch the population [n_members][weight_stride] is copied to [ceil(P / 4)][roundup(n_members, 64)][4] (parameter p of member m at float
 * ((p >> 2) * members + m) * 4 + (p & 3)), and every lane reads its member's 16 bytes of a group at a wave-uniform base: 64 lanes whose members are
 * consecutive read one run of 1 KB per load where the rows of LANEG cost 64 cache lines (serl_rollout_lanegt_kernel_<variant> /
 * serl_rollout_lanegt_noise_kernel_<variant>; the arithmetic, and so every result, is LANEG's bit for bit).  Opt-in; kernel_hint LANEG through serl_rollout
 * keeps streaming the rows.
 * MEMORY: one copy is ceil(P / 4) x roundup(n_members, 64) x 16 bytes, P = serl_param_count(...) -- 7.75 GB for 65 536 members of hidden 96 x 3 layers
 * (4.46 GB at 72 x 3; 1.11 GB at 72 x 3 for 16 384), 4.4 MB for 50 members of 72 x 3 -- and up to SERL_WT_SLOTS = 4 copies live at once: the copy of a launch goes into a ring of
 * four slots that the context keeps (each grown to the largest copy it has held, freed by serl_ctx_destroy), so that launches in flight on different streams
 * never share one; the fifth launch waits on its stream for the launch that used its slot.  serl_last_rollout_weights reports the size.  A failed
 * allocation is SERL_E_HIP.
 * Runs the checks of serl_rollout (and, with nz, of serl_rollout_noise), then SERL_E_UNSUPPORTED before any launch unless the kernel hint -- desc->kernel_hint,
 * or SERL_KERNEL=... for a descriptor that says AUTO -- resolves to SERL_KERNEL_LANEG ("only the LANEG kernels read a regrouped copy through this entry"),
 * and unless n_members <= 1 << 22 (a lane's 32-bit offset into a group).  serl_last_rollout_info reports family SERL_FAMILY_LANEG as for the rows. */
int serl_rollout_regrouped(serl_ctx *ctx, const serl_rollout_desc *desc, const serl_rollout_noise_desc *nz /* NULL: no generator */, void *stream);

/* the generator's bit-level parts on the host, compiled from the kernels' text (csrc/serl_rng.h) */
void serl_host_philox(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out4[4]);
double serl_host_uniform(uint32_t w0, uint32_t w1);

/* Development aid: with SERL_PROFILE=1 in the environment serl_rollout records shader-clock cycles of wave 0 of
 * workgroup 0: out[0..3] = {actor forward, dynamics step, env bookkeeping, env steps}; out[4..31] = phase
 * counters of the model evaluation (non-zero only in builds compiled with -DCITW_PROFILE). */
int serl_debug_profile(serl_ctx *ctx, unsigned long long out[32]);
/* Development aid: how the most recent serl_rollout_multi launch placed its workgroups.  out[0]: 0 = by blockIdx range (SERL_MIXED_PLACE=0, or one
 * code variant only), 1 = by the census of the CU pairs, 2 = by tickets (SERL_MIXED_PLACE=1, or the census timed out: the GPU was shared);
 * out[1] = workgroups that registered in the census; out[2] = CU pairs that held two of them, out[3] = one.  Blocks until the device is idle. */
int serl_debug_mixed_placement(serl_ctx *ctx, int32_t out[4]);

/* ABI v8.  WHAT the most recent serl_rollout / serl_rollout_multi call of this context launched -- the kernel family is chosen by the library
 * (episode count, actor shape, env configuration, kernel_hint), so a caller that compares families, or a test that names one, asks here which
 * one actually ran (the seam being replaced is the one loop `for net in pop: for i in range(num_evals): evaluate(net)`,
 * /root/reference/base/core/agent.py:234-241, which has no such choice).  Host-side record of the call: does not wait for the device.
 *   out[0] enum serl_kernel_family        out[1] workgroups of the (last) launch     out[2] episodes per team / per wavefront (LANE: lanes)
 *   out[3] 1 = the launch drains a work queue (a lane group takes the next episode when its own ends)
 *   out[4] actor wavefronts beside the team wavefronts (0: the family has none)       out[5] 1 = the actor streams its weights from L2 (0: LDS-resident)
 *   out[6] launches the call made (rounds of workgroups)                              out[7] enum serl_dyn_code of the launch, -1 = several (mixed sweep)
 * serl_dyn_open_loop records its launch too (families TEAM / WAVE / LANE, no actor wavefront).  SERL_E_INVALID before the first launch of the context. */
enum serl_kernel_family { SERL_FAMILY_NONE = 0, SERL_FAMILY_TEAM = 1 /* eight wavefronts = one episode, actor weights in LDS */,
                          SERL_FAMILY_TEAMS = 2 /* ... the actor wavefront streams its weights (hidden 72 / 96) */,
                          SERL_FAMILY_TEAMS2 = 3 /* ... two actor wavefronts share the forward pass (SERL_SPLIT_ACTOR=1) */,
                          SERL_FAMILY_TEAMX = 4 /* ... env configurations other than the attitude task */,
                          SERL_FAMILY_TEAM2 = 5 /* two episodes per team */, SERL_FAMILY_TEAM2S = 6 /* ... six team + two streaming actor wavefronts */,
                          SERL_FAMILY_TEAM4 = 7 /* four episodes per team */, SERL_FAMILY_TEAM4_MIXED = 8 /* ... several code variants in one launch */,
                          SERL_FAMILY_HALF = 9 /* one wavefront = two episodes */, SERL_FAMILY_WAVE = 10 /* one wavefront = one episode */,
                          SERL_FAMILY_WAVEX = 11 /* ... other env configurations */, SERL_FAMILY_LANE = 12 /* one lane = one episode */,
                          SERL_FAMILY_TEAMR = 13 /* eight wavefronts = one episode, its streamed actor (two wavefronts) in a workgroup of its own on another CU */,
                          SERL_FAMILY_LANEG = SERL_FAMILY_TEAMR + 1 /* (family 14) one lane = one episode, every actor shape: kernel_hint SERL_KERNEL_LANEG */ };
int serl_last_rollout_info(serl_ctx *ctx, int32_t out[8]);
/* Host-side record of the weights the most recent rollout launch read (the launch serl_last_rollout_info describes): out[0] 1 = a regrouped copy
 * [groups][padded members][4] was made in front of it (serl_rollout_regrouped; the hidden-32 lane kernels of lanes_per_wave > 0), 0 = the rows as they lie;
 * out[1] members padded to a multiple of 64, out[2] groups = ceil(P / 4), out[3] bytes of the copy = out[1] x out[2] x 16 (all 0 when out[0] is 0).  Does
 * not wait for the device.  SERL_E_INVALID before the first launch. */
int serl_last_rollout_weights(serl_ctx *ctx, int64_t out[4]);
/* The same for the step-wise env: WHAT the most recent serl_venv_reset* / _step* / _rollout* call of this context launched (a record of its own:
 * serl_last_rollout_info keeps describing the last serl_rollout).  out[0] enum serl_kernel_family: SERL_FAMILY_LANE (one lane = one env) or
 * SERL_FAMILY_WAVE (one wavefront = one env, the `_wave` entry points); out[1] workgroups; out[2] wavefronts per workgroup; out[3] enum serl_dyn_code.
 * Host-side, does not wait for the device.  SERL_E_INVALID before the first env call of the context. */
int serl_venv_last_info(serl_ctx *ctx, int32_t out[4]);

/* Duration (ms) of the most recent serl_rollout kernel on its stream, measured with HIP events
 * recorded around the launch; blocks until that kernel has finished. */
int serl_last_rollout_ms(serl_ctx *ctx, float *ms);

/* ---- SSNE weight-tensor edits (base/core/mod_neuro_evo.py) as elementwise kernels.  `weights` is
 * the same [n_members][stride] f32 tensor; index lists are DEVICE int32/float arrays generated by
 * the host from the reference's RNG streams so that selection stays bit-compatible. ------------ */
/* clone (mod_neuro_evo.py:371-382): weights[dst[i]][0 .. param_count) = weights[src[i]][0 .. param_count), i < n; the columns from
 * param_count to stride are left alone.  The pairs of one call are copied IN PARALLEL and must be independent: a destination
 * that is another pair's source (or two pairs with one destination) has no defined result; src[i] == dst[i] is fine.  The pairs
 * are a dimension of the launch grid: n = 65 536 and 65 537 are served on the MI355X (tests/test_gpu_support_kernels.py), no
 * smaller limit than int32 was found; a launch the runtime refuses returns SERL_E_HIP and has written nothing.  n = 0: no-op. */
int serl_ga_clone(serl_ctx *ctx, float *weights, int64_t stride, int32_t param_count,
                  const int32_t *src, const int32_t *dst, int32_t n, void *stream);
/* crossover_inplace (mod_neuro_evo.py:61-93): n row/element swaps between two members:
 *   ops[i] = {offset, length, dir}: dir 0 copies member b -> a, dir 1 copies a -> b, at
 *   weights[.. + offset .. offset+length) */
int serl_ga_crossover(serl_ctx *ctx, float *weights, int64_t stride, int32_t member_a, int32_t member_b,
                      const int32_t *ops, int32_t n_ops, void *stream);
/* mutate_inplace (mod_neuro_evo.py:329-369): n sparse edits of one member applied IN ORDER:
 *   kind 0:  w[idx] += z * (strength * w[idx])   (normal / super mutation: random.gauss(0, strength*w) = z*sigma)
 *   kind 1:  w[idx]  = z                          (reset: random.gauss(0, 1))
 * each followed by the reference's hard clamp to +-1e6 (regularize_weight, :57-59,366) with torch.clamp's semantics: a value that
 * is NaN (a NaN weight, a NaN draw, inf - inf, 0 * inf) STAYS NaN -- a diverged actor does not come back as a finite one --
 * and +-inf becomes +-1e6.  idx / kind / z / strength may be NULL only when n == 0 (SERL_E_INVALID otherwise). */
int serl_ga_mutate(serl_ctx *ctx, float *weights, int64_t stride, int32_t member,
                   const int32_t *idx, const int32_t *kind, const float *z, const float *strength,
                   int32_t n, void *stream);
/* proximal / safe mutation update (mod_neuro_evo.py:183-223, 254-298):
 *   theta[i] += delta[i] / scaling[i]   over the flat 2-D-weights genome given as (offset,length)
 *   segments of the packed parameter row */
int serl_ga_scaled_perturb(serl_ctx *ctx, float *weights, int64_t stride, int32_t member,
                           const int32_t *seg_offset, const int32_t *seg_length, int32_t n_seg,
                           const float *delta, const float *scaling, void *stream);

/* Output sensitivity of proximal_mutate / safe_mutate (mod_neuro_evo.py:183-223, 254-298): for every listed member,
 *   jacobian_i = d( sum_b actor(states[m][b])[i] ) / d genome,  i < action_dim   (the reference: one backward pass per output)
 *   scaling    = sqrt(sum_i jacobian_i^2);  scaling[scaling == 0] = 1;  scaling[scaling < 0.01] = 0.01
 * genome = the 2-D weights in named_parameters order (extract_parameters, genetic_agent.py:131-141), G = H*S + L*H*H + A*H.
 * states: f32 [n_members][batch][state_dim], scaling: f32 [n_members][G] (device).  The update itself is
 * serl_ga_scaled_perturb with delta drawn by the host (torch.distributions.Normal, the reference's generator). */
int serl_ga_sensitivity(serl_ctx *ctx, const float *weights, int64_t stride, int32_t state_dim, int32_t hidden,
                        int32_t num_layers, int32_t action_dim, int32_t activation, const int32_t *members,
                        int32_t n_members, const float *states, int32_t batch, float *scaling, void *stream);
/* The same sensitivity, batch-parallel, for every actor shape the TD3 learner takes (SERL_ABI_VERSION stays 9: added entry points):
 * hidden a multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, state_dim 1 .. 16, action_dim 1 .. 4, the three activations, minibatches
 * of 1 .. 512 rows -- hidden 128 x 3, which serl_ga_sensitivity refuses for LDS, included.  weights, members, states and scaling are
 * serl_ga_sensitivity's, scaling in the same genome order (W0, W1 .. WL, Wo); plus
 *   work   DEVICE scratch of serl_ga_sensitivity_general_work_bytes(n_members, .., batch) bytes: per member the gradient of one output
 *          over the genome and, per chunk of 128 samples, the states and the forward pass's tape.  Aligned as a float (4 B); what it
 *          holds on entry does not matter, and no byte beyond work_bytes is touched.
 *   dense  0 = the dense phases on the VALU, 1 = on the f32 matrix cores (v_mfma_f32_16x16x4_f32); the two give the same bits.
 * One workgroup of 512 threads per member, built from the learner's phases (serl_td3_train): one forward pass over the minibatch in
 * chunks of up to 128 samples, then per output a backward pass over every chunk whose weight gradients are batch-reduction products,
 * accumulated over the chunks before they are squared.  `members` may repeat and need not be sorted; `stride` >= the row's parameter
 * count; nothing outside scaling[n_members][G] and `work` is written.  Checks, in this order, all before any launch:
 *   SERL_E_INVALID      a NULL ctx / weights / members / states / scaling, n_members < 0, batch <= 0;  dense not 0 or 1
 *   SERL_E_UNSUPPORTED  a shape, an activation or a batch outside the ranges above
 *   SERL_OK             n_members == 0 (nothing launched; `work` may be NULL)
 *   SERL_E_INVALID      stride < the parameter count;  work NULL or work_bytes too small
 *   SERL_E_UNSUPPORTED  the activation tiles (~135 KB) do not fit the device's LDS per workgroup
 * serl_ga_sensitivity_general_work_bytes returns 0 for a shape or batch that is refused or n_members < 1. */
int64_t serl_ga_sensitivity_general_work_bytes(int32_t n_members, int32_t state_dim, int32_t action_dim, int32_t hidden,
                                               int32_t num_layers, int32_t batch);
int serl_ga_sensitivity_general(serl_ctx *ctx, const float *weights, int64_t stride, int32_t state_dim, int32_t hidden,
                                int32_t num_layers, int32_t action_dim, int32_t activation, const int32_t *members,
                                int32_t n_members, const float *states, int32_t batch, float *scaling, void *work,
                                int64_t work_bytes, int32_t dense, void *stream);
/* Actor.get_novelty (genetic_agent.py:111-115) for n_pairs (actor, batch) pairs in one launch:
 *   novelty[p] = mean_b sum_a (actions[p][b][a] - actor_{members[p]}(states[p][b])[a])^2
 * -- the two halves of SSNE.get_distance (mod_neuro_evo.py:411-417), i.e. the keys of sort_groups_by_distance (:426-445). */
int serl_ga_novelty(serl_ctx *ctx, const float *weights, int64_t stride, int32_t state_dim, int32_t hidden,
                    int32_t num_layers, int32_t action_dim, int32_t activation, const int32_t *members, int32_t n_pairs,
                    const float *states, const float *actions, int32_t batch, float *novelty, void *stream);
/* The same novelty, batch-parallel, for every actor shape the TD3 learner takes (SERL_ABI_VERSION stays 9: an added entry point): hidden
 * a multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, state_dim 1 .. 16, action_dim 1 .. 4, the three activations, minibatches of up to
 * max_batch <= 512 rows.  One workgroup of 512 threads per evaluation e < n_evals, built from the learner's forward phases
 * (serl_td3_train) over chunks of 128 samples; no workspace.  An evaluation reads its minibatch itself:
 *   state_base[e], action_base[e]   DEVICE arrays [n_evals] of device pointers; sample b of evaluation e is the state_dim floats at
 *                  state_base[e] + r state_stride and the action_dim floats at action_base[e] + r action_stride (strides in floats),
 *                  r = clamp(slots[e][b], 0, n_rows[e] - 1)
 *   slots          DEVICE int32 [n_evals][max_batch], or NULL: slot b is b
 *   n_rows, batch  DEVICE int32 [n_evals]: the rows behind the bases, and the minibatch B_e = clamp(batch[e], 0, max_batch); n_rows[e] < 1
 *                  makes B_e 0.  Entries of slots[e] from B_e on are not read.
 *   dense          0 = the dense phase on the VALU, 1 = on the f32 matrix cores (v_mfma_f32_16x16x4_f32); the two give the same bits.
 * So one entry serves a replay ring (state_base = rows, action_base = rows + state_dim, both strides 2 state_dim + action_dim + 3,
 * slots = physical ring slots) and the dense states [n][B][S] / actions [n][B][A] of serl_ga_novelty (bases = the rows of evaluation e,
 * strides state_dim and action_dim, slots NULL, n_rows = batch = B).  Every table is read on the device: the entry reads nothing back
 * and does not synchronise.  Samples from B_e on are zero columns and reach no sum.
 *   novelty[e] = (sum_b sum_a (action[b][a] - actor_{members[e]}(state[b])[a])^2) / B_e     f32; B_e == 0: NaN (torch's mean of nothing)
 * in one fixed order, so that the result is the same bits for both values of `dense`, for any n_evals and max_batch and for either
 * layout: per sample a ascending, s_b = ((0 + d_0^2) + d_1^2) + .. (product and sum rounded separately); per column c < 128 the chunks
 * ascending, t_c = ((s_c + s_(c+128)) + s_(c+256)) + s_(c+384), absent samples skipped; per half h of 64 columns the butterfly
 * x_l += x_(l xor o), o = 32, 16, 8, 4, 2, 1, over t_(64 h + l) (absent columns +0); then (u_0 + u_1) / (float)B_e.
 * `members` may repeat; `stride` >= the row's parameter count; nothing but novelty[0 .. n_evals) is written.  Checks, in this order, all
 * before any launch (novelty untouched):
 *   SERL_E_INVALID      a NULL ctx / weights / members / state_base / action_base / n_rows / batch / novelty, n_evals < 0;  dense not 0 or 1
 *   SERL_E_UNSUPPORTED  a shape or an activation outside the ranges above, max_batch outside 1 .. 512
 *   SERL_OK             n_evals == 0 (nothing launched)
 *   SERL_E_INVALID      stride < the parameter count;  state_stride < state_dim or action_stride < action_dim
 *   SERL_E_UNSUPPORTED  the activation tiles (~135 KB) do not fit the device's LDS per workgroup */
int serl_ga_novelty_general(serl_ctx *ctx, const float *weights, int64_t stride, int32_t state_dim, int32_t hidden,
                            int32_t num_layers, int32_t action_dim, int32_t activation, const int32_t *members, int32_t n_evals,
                            const float *const *state_base, int64_t state_stride, const float *const *action_base,
                            int64_t action_stride, const int32_t *slots, const int32_t *n_rows, const int32_t *batch,
                            int32_t max_batch, float *novelty, int32_t dense, void *stream);

/* ---- device replay rings (base/core/replay_memory.py:21-31 `add`, base/core/agent.py:101-112) ---------------------------
 * A ring is f32 [capacity][W] rows (obs S, action A, next_obs S, r, done, cost), W = 2 S + A + 3, in HBM -- the dense
 * layout serl_rollout writes to `transitions`, so a ring row equals a staged row bit for bit.  One job appends the rows of
 * one stored episode -- staged[episode][0 .. length) -- to ring slots (position + k) % capacity in step order, k = rank of
 * the row among the rows taken: all of them, or (cost_only) the cost-flagged ones (row[W - 1] != 0), compacted
 * (agent.critical_buffer).  The first `skip` ranks are not written (an episode longer than the ring leaves only its tail,
 * as sequential add() calls would).  The host keeps position / fill of every ring.
 *   serl_replay_scatter        rows of the attitude task: S = 7, A = 3, W = 20.
 *   serl_replay_scatter_rows   rows of any env configuration: 1 <= state_dim <= 64, 1 <= action_dim <= 16 (the range of
 *                              the networks; SERL_E_UNSUPPORTED outside it, nothing launched).  staged is
 *                              [episodes][rows_per_episode][W].  Same jobs, same meaning; any W, odd ones included: rows
 *                              move with 16 B accesses when W % 4 == 0 and the ring and the episode are 16 B aligned, with
 *                              8 B accesses likewise for even W, with 4 B accesses otherwise.  A job without a ring, with
 *                              capacity < 1, position outside [0, capacity), length > rows_per_episode or a negative
 *                              field is skipped; length == 0 and skip == rows taken are no-ops, as in serl_replay_scatter. */
typedef struct serl_replay_job {
  float *ring;
  int32_t capacity, position, episode, length, cost_only, skip;
} serl_replay_job;
int serl_replay_scatter(serl_ctx *ctx, const float *staged, int64_t rows_per_episode, const serl_replay_job *jobs /* device */,
                        int32_t n_jobs, void *stream);
int serl_replay_scatter_rows(serl_ctx *ctx, const float *staged, int64_t rows_per_episode, int32_t state_dim, int32_t action_dim,
                             const serl_replay_job *jobs /* device */, int32_t n_jobs, void *stream);

/* calc_smoothness (base/core/utils.py:82-120) of n_episodes action traces of DIFFERENT lengths in one launch:
 *   Y = fft(y, N) per channel, N = |lengths[e]|;  S = sum_c sum_{1 <= i < N/2} |Y_i,c|^2 * dt * f_i * 2 / N  with
 *   f = linspace(dt, 1 / (2 dt), N/2 - 1);  out[e] = -sqrt(S) * 100 * (80 / (N dt))   (0 for N < 4)
 * evaluated as a direct DFT (one thread per frequency, the N twiddles in LDS), so there is no per-length FFT plan.
 * actions: f64 [n_episodes][episode_stride / 3][3] (env.last_u per step: serl_rollout_desc.actions), rows past N ignored;
 * work: f64 [serl_smoothness_work_size(n_episodes, max_len)] scratch; max_len >= every |length|, <= 8192 (SERL_E_UNSUPPORTED above).
 * The summation order is fixed: out[e] depends on the episode's own samples, |length| and dt only -- not on max_len,
 * episode_stride, n_episodes or the episode's place in the batch.  The episodes are a dimension of the launch grid:
 * n_episodes = 65 536 (the saturating configuration) and 65 537 are served on the MI355X (tests/test_gpu_support_kernels.py); the
 * limit that remains is the int result of serl_smoothness_work_size, n_episodes * ceil((max_len / 2 - 1) / 256) < 2^31.  A launch
 * the runtime refuses returns SERL_E_HIP with `out` untouched. */
int serl_smoothness_work_size(int32_t n_episodes, int32_t max_len);
int serl_smoothness(serl_ctx *ctx, const double *actions, int64_t episode_stride, const int32_t *lengths, int32_t n_episodes,
                    int32_t max_len, double dt, double *work, double *out, void *stream);

/* The training loop of SSNE.distilation_crossover (base/core/mod_neuro_evo.py:131-147) for all pairs of an epoch in one
 * launch: n_steps[p] Adam steps (torch.optim.Adam defaults, lr) of GeneticAgent.update_parameters
 * (base/core/genetic_agent.py:22-59) per pair, on minibatches slots[p][step][0 .. batch[p]) of the child's buffer:
 *   loss = sum_kept (actor(state) - target)^2 + mean_kept(actor(state)^2)
 * `targets` (the better parent's action per state) and `keep` (1 where the critic's Q-filter keeps the state) are what
 * the parents and the critic contribute; they do not depend on the child and are computed once by the caller.
 * child: f32 [n_pairs][stride], in = the second parent's parameters, out = the trained child.  states [n_pairs][rows][S],
 * targets [n_pairs][rows][A], keep [n_pairs][rows], slots i32 [n_pairs][steps][128].  Compiled for hidden 32 x 3 layers
 * (SERL_E_UNSUPPORTED otherwise).
 * What the device tables hold is clamped, never trusted with an address: a slot into [0, rows), batch[p] into [0, 128] (0: every
 * step is a minibatch with no kept row -- an Adam step with zero gradients, which from zero moments leaves the row bit for bit as
 * it was), n_steps[p] into [0, steps].  keep is a flag, not a weight: a row is kept when keep != 0 as f32 compares -- 2, -1, 0.5
 * and a subnormal keep it exactly as 1 does, +0 and -0 drop it. */
int serl_ga_distill(serl_ctx *ctx, float *child, int64_t stride, int32_t n_pairs, int32_t state_dim, int32_t hidden, int32_t num_layers,
                    int32_t action_dim, int32_t activation, const float *states, const float *targets, const float *keep, int32_t rows,
                    const int32_t *slots, int32_t steps, const int32_t *n_steps, const int32_t *batch, float lr, void *stream);
/* The same training loop for every actor shape the TD3 learner takes (SERL_ABI_VERSION stays 9: an added entry point): hidden a
 * multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, state_dim 1 .. 16, action_dim 1 .. 4, the three activations, minibatches of
 * 1 .. 128 rows -- hidden 32 x 3 included.  SERL_E_UNSUPPORTED otherwise, nothing touched.  Arguments and semantics are
 * serl_ga_distill's (a slot outside [0, rows) is clamped into it; n_steps[p] == 0 leaves row p bit for bit unchanged; columns past the
 * row and rows outside the launch are not written; an all-dropped minibatch takes its Adam step with zero gradients; batch[p],
 * n_steps[p] and keep are read by serl_ga_distill's rules above, n_steps[p] <= 0 writing nothing), plus
 *   lr     > 0 (SERL_E_INVALID otherwise, NaN included); `stride` >= the row's parameter count, any remainder by 4: `child` and its
 *          rows need the alignment of a float only.
 *   work   DEVICE scratch of serl_ga_distill_general_work_bytes(n_pairs, ..) bytes: per pair the gradients, Adam's two moments (zeroed
 *          by the kernel), the gathered minibatch and the backward pass's tape.  The child row itself is trained in place in `child`:
 *          at these shapes parameters, gradients and moments no longer fit the LDS serl_ga_distill keeps them in.  Aligned as a
 *          float (4 B), no more; what it holds on entry does not matter (NaN included), and no byte beyond work_bytes is touched.
 *          NULL or too small: SERL_E_INVALID, nothing launched.
 *   dense  0 = the dense phases on the VALU, 1 = on the f32 matrix cores (v_mfma_f32_16x16x4_f32); the two give the same bits.
 * One workgroup per pair, built from the learner's phases (serl_td3_train); n_pairs == 0 is the probe "would this shape run here?",
 * for which `work` may be NULL.  serl_ga_distill_general_work_bytes returns 0 for a shape that is refused or n_pairs < 1. */
int64_t serl_ga_distill_general_work_bytes(int32_t n_pairs, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers);
int serl_ga_distill_general(serl_ctx *ctx, float *child, int64_t stride, int32_t n_pairs, int32_t state_dim, int32_t hidden,
                            int32_t num_layers, int32_t action_dim, int32_t activation, const float *states, const float *targets,
                            const float *keep, int32_t rows, const int32_t *slots, int32_t steps, const int32_t *n_steps,
                            const int32_t *batch, float lr, void *work, int64_t work_bytes, int32_t dense, void *stream);
/* Host helper (no GPU work): the rows `random.sample(memory, k)` of base/core/replay_memory.py:72-73,83-85 picks from n
 * transitions in `calls` consecutive calls, replayed from the generator's raw 32-bit outputs (CPython's selection
 * algorithm: set-based above its set-size threshold, pool-based below).  Returns the number of outputs consumed,
 * -1 = n_words too small, -2 = bad arguments.  out: i32 [calls][out_stride], out_stride >= k. */
long long serl_host_sample_slots(const uint32_t *words, long long n_words, int32_t n, int32_t k, int32_t calls, int32_t *out,
                                 int32_t out_stride);

/* ---- the TD3 learner: K consecutive gradient updates as one launch (SERL_ABI_VERSION stays 9: serl_abi_layout and every struct
 * above are unchanged; this descriptor has a layout self-check of its own, serl_td3_layout) ---------------------------------------
 * Agent.train_rl (base/core/agent.py:155-186) calls TD3.update_parameters (base/core/td3.py:123-198) once per frame of the
 * generation.  serl_td3_train runs n_updates of them back to back for n_learners independent learners, one workgroup each, reading
 * the minibatches straight from a device replay ring.  Every array is a DEVICE pointer owned by the caller; the call is asynchronous
 * on the stream; nothing is allocated or synchronised.
 *   networks   actor / actor_target: the packed actor row of serl_rollout_desc (state_dict order).  critic / critic_target: the
 *              TRAINED parameters of the reference's Critic (td3.py:17-85; 64-64 hidden units, activation_actor, the project's
 *              LayerNorm: unbiased std, eps 1e-6 on the std) as one row, critic 1 then critic 2, each
 *                W1[64][S+A] b1[64] g1[64] be1[64]  W2[64][64] b2[64] g2[64] be2[64]  Wo[64] bo[1]
 *              = serl_td3_param_count(S, A) floats in all (10 370 at S + A = 10).  The reference's bnorm_* parameters take no part
 *              in forward, get no gradient (their .grad stays None: Adam and the norm clip skip them) and are not in the row.
 *   state      per learner, updated in place: the four rows, Adam's first and second moments of actor and critic (actor_m / _v,
 *              critic_m / _v, laid out like the rows) and adam_steps i32 [n_learners][2] = {critic steps, actor steps} taken so
 *              far, so that a second call continues the first.
 *   inputs     ring f32 [capacity][2 S + A + 3] (the rows serl_rollout writes: obs, action, next_obs, reward, done, cost);
 *              slots i32 [n_updates][slot_cols], the first `batch` columns of a row are the minibatch of that update, drawn by the
 *              host (a slot outside [0, capacity) is clamped into it); target_noise f32 [n_updates][batch][A] standard-normal draws
 *              (the kernel applies * noise_sd and the clamp to +-noise_clip); caps_noise f32 [actor updates][batch][S] uniform
 *              [0, 1) draws, one block per ACTOR update of the call in order, or NULL = CAPS off (lambda_s, lambda_t, eps_sd unused).
 *   update u   iteration = iteration0 + u + 1, exactly td3.py:123-198:
 *                next_a = clamp(noise + actor_target(s'), -1, 1);  target_q = r + gamma * (1 - done) * min(Q1', Q2')
 *                td = mse(Q1, target_q) + mse(Q2, target_q); one gradient-norm clip over BOTH critics (coef = max_grad_norm /
 *                (norm + 1e-6), applied when below 1); Adam (torch defaults, torch.optim.Adam's bias correction) with lr
 *                if iteration % policy_update_freq == 0:  pg = -mean(Q1(s, actor(s))) [+ lambda_t * mse(a, actor(s)) + lambda_s *
 *                mse(a, actor(s + eps_sd * u)) with a the BATCH action in both terms, as the reference writes them]; clip; Adam;
 *                critic_target <- (1 - tau) critic_target + tau critic; the same for actor_target unless update_actor_target == 0
 *                (the reference's use_champion_target).
 *   outputs    td_loss f32 [n_updates]; pg_loss f32 [n_updates], written at actor updates only (other entries left as given).
 *              n_updates == 0 leaves every buffer bit for bit unchanged.
 *   learners   every per-learner array has a stride (in elements) between learners; ring_stride / slots_stride / noise_stride /
 *              caps_stride may be 0 (shared).  A learner's result does not depend on the others or on its place in the grid.
 *   work       serl_td3_work_bytes(n_learners, S, A, hidden, num_layers, batch) bytes of scratch (0 = shape not compiled).
 * Arithmetic is f32 with this library's summation order: agreement with a float64 run is to rounding, not bit for bit.
 * Compiled for hidden a multiple of 4 in 4 .. 128, 0 .. 4 hidden layers, S 1 .. 16, A 1 .. 4, batch 1 .. 128: any other positive
 * shape returns SERL_E_UNSUPPORTED with nothing launched (the caller trains in PyTorch); NULL or out-of-range arguments return
 * SERL_E_INVALID before any device work. */
typedef struct serl_td3_desc {
  int32_t state_dim, action_dim, hidden, num_layers, activation;   /* the actor (enum serl_activation also drives the critic) */
  int32_t n_learners, batch, n_updates;
  int32_t capacity, slot_cols;
  int32_t policy_update_freq, iteration0, update_actor_target, pad0;
  float lr, gamma, tau, noise_sd, noise_clip, lambda_s, lambda_t, eps_sd, max_grad_norm, pad1;
  float *actor, *actor_target, *actor_m, *actor_v;
  int64_t actor_stride;             /* floats between learners, >= serl_param_count */
  float *critic, *critic_target, *critic_m, *critic_v;
  int64_t critic_stride;            /* >= serl_td3_param_count */
  int32_t *adam_steps;              /* [n_learners][2] */
  const float *ring;
  int64_t ring_stride;
  const int32_t *slots;
  int64_t slots_stride;
  const float *target_noise;
  int64_t noise_stride;
  const float *caps_noise;
  int64_t caps_stride;
  float *td_loss, *pg_loss;
  int64_t loss_stride;              /* >= n_updates */
  void *work;
  int64_t work_bytes;
} serl_td3_desc;
/* floats of the critic row: 2 * (64 (S + A) + 64 * 64 + 6 * 64 + 64 + 1); 0 for dims < 1 */
int serl_td3_param_count(int state_dim, int action_dim);
int64_t serl_td3_work_bytes(int32_t n_learners, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t batch);
/* layout self-check like serl_abi_layout: sizeof(serl_td3_desc), then offsetof of each member in declaration order */
int serl_td3_layout(int32_t *out, int32_t capacity);
int serl_td3_train(serl_ctx *ctx, const serl_td3_desc *desc, void *stream);
/* serl_td3_train with the three dense phases (Linear forward, backward to the input, weight gradient) on the f32-in / f32-accumulate
 * matrix cores (v_mfma_f32_16x16x4_f32) instead of scalar fmaf; everything else is the same code.  Opt-in: serl_td3_train is
 * unchanged.  Same descriptor, same checks in the same order with the same return codes, same serl_td3_work_bytes.  Contract: every
 * array it writes -- the four rows, the four moment rows, adam_steps, td_loss, pg_loss -- equals what serl_td3_train writes for the
 * same descriptor, bit for bit: the matrix instruction is an f32 fmaf chain in k order with one rounding per product, and each
 * output element's chain is fed in the scalar kernel's order (serl_amd/csrc/serl_td3_mfma.h).  `work` is scratch for both; its
 * contents after a call are unspecified and may differ between the two (columns of samples from `batch` on). */
int serl_td3_train_mfma(serl_ctx *ctx, const serl_td3_desc *desc, void *stream);

/* ---- the TD3 learner with its minibatch slots and its noise drawn inside the kernel (SERL_ABI_VERSION stays 9: nothing above has
 * moved; this descriptor has a layout self-check of its own, serl_td3_rng_layout) ---------------------------------------------------
 * serl_td3_train / _mfma with the counter-based generator of serl_venv_noise_desc (csrc/serl_rng.h) in place of the three tables: no
 * table, no host draw, memory independent of n_updates, and a result that is a function of (seed, learner key, absolute iteration).
 *   bits     Philox4x32-10, key = seed, counter = (learner key, iteration, index, stream << 16 | block); the learner key of learner p of
 *            a launch is learner0 + p; iteration = iteration0 + u + 1, so two calls of n1 and n2 updates draw what one of n1 + n2 draws
 *   slots    stream 2, block 0, index = step i: `batch` distinct rows of [0, n_rows), uniform over the subsets, by Floyd's algorithm.
 *            Step i = 0 .. batch - 1: j = n_rows - batch + i, t = floor(w64 (j + 1) / 2^64) with w64 = w0 << 32 | w1 of the step's
 *            four words; column i is t unless an earlier column holds t, else j.  Column b is sample b of the kernel.  Integer only
 *   target   stream 3, index = sample b, blocks 0 .. 1 = 4 standard normals (the Box-Muller pairs of serl_venv_noise_desc), the first
 *            action_dim cast to f32; * noise_sd and the clamp are applied where the table path applies them
 *   caps     stream 4, index = sample b, blocks 0 .. 3 = 16 words; uniform j = (float)(word j >> 8) * 2^-24, in [0, 1) on torch.rand's
 *            grid; the first state_dim are used.  Drawn at actor updates (iteration % policy_update_freq == 0) only
 * Contract: every array serl_td3_train_rng writes -- the four rows, the four moment rows, adam_steps, td_loss, pg_loss -- equals, bit
 * for bit, what serl_td3_train (dense 0) or serl_td3_train_mfma (dense 1) writes when fed the tables of serl_td3_rng_fill: the
 * kernels are second instantiations of the same source that differ at the slot read and the two noise reads only. */
typedef struct serl_td3_rng_desc {
  uint64_t seed;
  int32_t n_rows;      /* filled rows of the ring the slots are drawn from: batch <= n_rows <= capacity */
  int32_t learner0;    /* learner p of the launch draws with key learner0 + p */
  int32_t dense;       /* 0 = valu, 1 = mfma */
  int32_t caps;        /* 0 = CAPS off (as caps_noise == NULL), 1 = on */
} serl_td3_rng_desc;
/* layout self-check: sizeof(serl_td3_rng_desc), then offsetof of each member in declaration order */
int serl_td3_rng_layout(int32_t *out, int32_t capacity);
/* Asynchronous on `stream`, one launch.  desc->slots, slot_cols, target_noise, caps_noise and slots_stride / noise_stride / caps_stride
 * are ignored (the pointers may be NULL).  Every other check of serl_td3_train runs in the same order with the same codes; then
 * SERL_E_INVALID before any device work for a NULL rng, n_rows < batch, n_rows > capacity, learner0 + n_learners past INT32_MAX, dense
 * or caps other than 0 / 1.  The same serl_td3_work_bytes; n_updates == 0 leaves every buffer unchanged. */
int serl_td3_train_rng(serl_ctx *ctx, const serl_td3_desc *desc, const serl_td3_rng_desc *rng, void *stream);
/* The replay tool: the tables serl_td3_train needs to reproduce a serl_td3_train_rng call of learner `learner` of the launch (key
 * rng->learner0 + learner), written by the kernels' own device functions.  slots i32 [n_updates][batch], target_noise f32
 * [n_updates][batch][action_dim], caps_noise f32 [actor updates of the call][batch][state_dim] or NULL (not written); all DEVICE.
 * rng->dense and rng->caps are not read.  SERL_E_INVALID for a NULL argument, state_dim outside 1 .. 16, action_dim outside 1 .. 4,
 * batch outside 1 .. 128, rng->n_rows < batch, learner < 0, n_updates < 0, policy_update_freq < 1, iteration0 < 0. */
int serl_td3_rng_fill(serl_ctx *ctx, const serl_td3_rng_desc *rng, int32_t learner, int32_t state_dim, int32_t action_dim, int32_t batch,
                      int32_t iteration0, int32_t n_updates, int32_t policy_update_freq, int32_t *slots, float *target_noise,
                      float *caps_noise, void *stream);
/* the slot draw of (seed; learner key, iteration) on the host, compiled from the kernels' text (csrc/serl_rng.h): out i32 [batch], any
 * 1 <= batch <= n_rows (batch^2 / 2 comparisons).  SERL_E_INVALID for a NULL out, batch < 1 or n_rows < batch. */
int serl_host_td3_slots(uint64_t seed, int32_t learner, int32_t iteration, int32_t n_rows, int32_t batch, int32_t *out);

/* ---- a group of independent TD3 learners in one launch (SERL_ABI_VERSION stays 9: new symbols only, nothing above has moved; the two
 * structs have a layout self-check of their own, serl_td3_group_layout) -------------------------------------------------------------
 * serl_td3_train_rng runs n_learners learners too, but with one ring allocation, one n_updates / iteration0 / n_rows and one set of
 * hyper-parameters for all of them.  Independent experiments of one network shape -- several seeds, a few settings -- differ in all of
 * these every generation.  serl_td3_train_group takes them per learner from a DEVICE array of rows: one workgroup per learner as
 * before, no grid-wide synchronisation, no workgroup waiting on another, the workspace of serl_td3_work_bytes(n_learners, ...).
 *   desc     shape, n_learners, batch, max_grad_norm, the eight state rows with their strides, adam_steps, td_loss / pg_loss /
 *            loss_stride, work and work_bytes mean what they mean for serl_td3_train and get its checks, in its order, with its codes.
 *            n_updates is the most any learner of the launch may run (a row's bound, and loss_stride's).  ring, ring_stride, capacity,
 *            iteration0, policy_update_freq, update_actor_target, the eight hyper-parameters lr .. eps_sd and all table fields are
 *            ignored and may be zero or NULL.
 *   rows     one serl_td3_learner_row per learner.  Like serl_ref_spec rows, the library does NOT read them on the host (that would
 *            take a synchronisation): workgroup p reads rows[p] once, checks it before it touches any other memory, and reports in
 *            status[p] (DEVICE i32 [n_learners]): 0 = the learner ran, else the first failed check (enum serl_td3_row_status).  A
 *            refused learner writes its status and nothing else; every other array of it stays bit for bit unchanged, and the other
 *            learners of the launch are not affected.  A row with n_updates == 0 is valid and leaves all but its status unchanged.
 *            The status array is the report: the return value only tells that the launch was made.
 *   dense    0 = valu, 1 = mfma;  caps 0 = CAPS off for every learner (lambda_s, lambda_t, eps_sd must still pass the checks), 1 = on.
 * Contract: every array learner p writes -- its four rows, its four moment rows, its adam_steps pair, td_loss[p] and pg_loss[p] --
 * equals, bit for bit, what a single-learner serl_td3_train_rng call writes whose descriptor holds the row's ring, capacity, n_updates,
 * iteration0, policy_update_freq, update_actor_target and hyper-parameters and whose rng = {seed, n_rows, learner0 = key, dense, caps}.
 * The kernels are further instantiations of the one source: they differ from serl_td3_train_rng's where these values are read only.
 * A learner's result does not depend on the other learners or on its place in the grid. */
typedef struct serl_td3_learner_row {
  const float *ring;                /* DEVICE f32 [capacity][2 S + A + 3], this learner's own */
  uint64_t seed;                    /* with key: the generator's (seed, learner key) of serl_td3_rng_desc */
  int32_t capacity, n_rows;         /* batch <= n_rows <= capacity: the filled rows the slots are drawn from */
  int32_t n_updates, iteration0;    /* 0 <= n_updates <= desc->n_updates; iteration0 >= 0, iteration0 + n_updates <= INT32_MAX - 1 */
  int32_t key;
  int32_t policy_update_freq;       /* >= 1 */
  int32_t update_actor_target, pad0;
  float lr, gamma, tau, noise_sd, noise_clip, lambda_s, lambda_t, eps_sd;     /* the ranges serl_td3_train checks; none may be NaN */
} serl_td3_learner_row;
enum serl_td3_row_status {
  SERL_TD3_ROW_OK = 0,
  SERL_TD3_ROW_RING = 1,            /* ring is NULL */
  SERL_TD3_ROW_UPDATES = 2,         /* n_updates < 0 or above desc->n_updates */
  SERL_TD3_ROW_ITERATION = 3,       /* iteration0 < 0, or iteration0 + n_updates overflows */
  SERL_TD3_ROW_ROWS = 4,            /* n_rows < batch or n_rows > capacity */
  SERL_TD3_ROW_FREQ = 5,            /* policy_update_freq < 1 */
  SERL_TD3_ROW_HYPER = 6,           /* lr <= 0, gamma < 0, tau outside [0, 1], noise_sd / noise_clip / eps_sd < 0, or a NaN */
  /* serl_td3_train_group_wide only: the row passed its checks, then a wait of the learner's hand-over A .. D ran out of time
   * (16 + enum serl_td3_wide_status, so that the one status word tells the two kinds of report apart) */
  SERL_TD3_ROW_HANDOVER_A = 17,
  SERL_TD3_ROW_HANDOVER_B = 18,
  SERL_TD3_ROW_HANDOVER_C = 19,
  SERL_TD3_ROW_HANDOVER_D = 20
};
typedef struct serl_td3_group_desc {
  const serl_td3_learner_row *rows; /* DEVICE [n_learners] */
  int32_t *status;                  /* DEVICE i32 [n_learners], written by every workgroup */
  int32_t dense;                    /* 0 = valu, 1 = mfma */
  int32_t caps;                     /* 0 = CAPS off, 1 = on */
} serl_td3_group_desc;
/* layout self-check: sizeof(serl_td3_learner_row), offsetof of each member in declaration order, then the same of serl_td3_group_desc */
int serl_td3_group_layout(int32_t *out, int32_t capacity);
/* Asynchronous on `stream`, ONE launch (made for desc->n_updates == 0 too: the status is still written); nothing is allocated or
 * synchronised.  SERL_E_INVALID / SERL_E_UNSUPPORTED for `desc` exactly where serl_td3_train_rng returns them for the fields that are
 * not ignored; then SERL_E_INVALID for a NULL group, NULL rows or status, dense or caps other than 0 / 1; all with nothing launched. */
int serl_td3_train_group(serl_ctx *ctx, const serl_td3_desc *desc, const serl_td3_group_desc *group, void *stream);

/* ---- the TD3 learner on minibatches of up to 512 rows (SERL_ABI_VERSION stays 9: new symbols only, nothing above has moved; the struct
 * has a layout self-check of its own, serl_td3_big_layout) ---------------------------------------------------------------------------
 * The entries above are compiled for batch 1 .. 128 and keep refusing 129 (SERL_E_UNSUPPORTED; serl_td3_work_bytes 0).
 * serl_td3_train_big takes the same serl_td3_desc with batch 1 .. 512: further instantiations of the one kernel source that walk the
 * minibatch in chunks of 128 samples, chunk c = samples 128 c .. min(batch, 128 c + 128) - 1 (columns 128 c .. of a slots row, rows
 * 128 c .. of a noise block, index b of the generator), at most four, the last one possibly partial.  One workgroup per learner,
 * __syncthreads only, no workgroup waits on another.
 * Summation contract.  Everything per sample (gather, forward and backward passes, LayerNorm, the target, the CAPS terms, the draws) is
 * computed per chunk exactly as the entries above compute it for a minibatch of that chunk's size.  Every sum over the samples of the
 * minibatch -- a weight, bias, LayerNorm gain or bias gradient, td_loss, pg_loss -- is
 *     ((P0 + P1) + P2) + P3        (as many terms as there are chunks; f32, one rounding per +)
 * where Pc is the partial sum over chunk c's samples in the order the entries above use for a minibatch of that size (a sample at or
 * past `batch` reaches no sum), with every term already scaled by the means' divisors 1 / batch and 1 / (batch * A) -- the minibatch's,
 * not the chunk's.  td_loss sums the partials chunk by chunk, within a chunk critic 1's then critic 2's:
 *     td = 0 + P0(Q1) + P0(Q2) + P1(Q1) + P1(Q2) + ..      with Pc(Qk) = (sum over chunk c of (Qk - target_q)^2) * (1 / batch)
 * The norm clip, Adam and the soft updates run once per update over the whole minibatch's gradients.  Consequences: with batch <= 128
 * every array written equals, bit for bit, what serl_td3_train / _mfma / _rng writes; dense 1 equals dense 0 bit for bit at every
 * batch; in-kernel draws equal the tables of serl_td3_rng_fill_big bit for bit; against float64 the agreement is to rounding.
 *   rng      NULL = slots and noise from desc's tables (slot_cols >= batch).  Else the generator of serl_td3_train_rng with the same
 *            checks; desc's table fields are ignored; rng->dense must equal `dense`.  The slot draw is serl_host_td3_slots' for any batch.
 *   dense    0 = valu, 1 = mfma
 *   work     serl_td3_big_work_bytes(n_learners, S, A, hidden, num_layers, batch): the gradients once, inputs and tapes per chunk --
 *            serl_td3_work_bytes' value up to batch 128, about four times that at 512; 0 = shape not compiled (batch outside 1 .. 512,
 *            or a network shape serl_td3_work_bytes refuses). */
typedef struct serl_td3_big_desc {
  const serl_td3_rng_desc *rng;     /* HOST; NULL = tables */
  int32_t dense;                    /* 0 = valu, 1 = mfma */
  int32_t pad0;
} serl_td3_big_desc;
/* layout self-check: sizeof(serl_td3_big_desc), then offsetof of each member in declaration order */
int serl_td3_big_layout(int32_t *out, int32_t capacity);
int64_t serl_td3_big_work_bytes(int32_t n_learners, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t batch);
/* Asynchronous on `stream`, one launch.  SERL_E_INVALID for a NULL big or dense other than 0 / 1; then the checks of serl_td3_train
 * (rng == NULL) or serl_td3_train_rng in their order with their codes, with batch up to 512 (513: SERL_E_UNSUPPORTED) and the workspace
 * of serl_td3_big_work_bytes; all before any device work.  n_updates == 0 leaves every buffer unchanged. */
int serl_td3_train_big(serl_ctx *ctx, const serl_td3_desc *desc, const serl_td3_big_desc *big, void *stream);
/* serl_td3_rng_fill for batch 1 .. 512: the tables with which serl_td3_train_big (rng == NULL) reproduces a call with rng != NULL */
int serl_td3_rng_fill_big(serl_ctx *ctx, const serl_td3_rng_desc *rng, int32_t learner, int32_t state_dim, int32_t action_dim, int32_t batch,
                          int32_t iteration0, int32_t n_updates, int32_t policy_update_freq, int32_t *slots, float *target_noise,
                          float *caps_noise, void *stream);

/* ---- the TD3 learner with a large minibatch's chunks on parallel workgroups (SERL_ABI_VERSION stays 9: new symbols only, nothing above
 * has moved; the struct has a layout self-check of its own, serl_td3_wide_layout) ---------------------------------------------------
 * serl_td3_train_big walks the G = ceil(batch / 128) chunks of a minibatch one after the other on the learner's one workgroup.
 * serl_td3_train_wide takes the same serl_td3_desc (batch 1 .. 512) and runs a grid of G x n_learners workgroups: workgroup (ch, p) owns
 * chunk ch of learner p for the whole call and runs everything per sample of that chunk; workgroup (0, p) alone adds the chunks'
 * partial sums, runs the norm clip, Adam and the soft updates and stores the losses and adam_steps.
 * Summation contract: serl_td3_train_big's.  A workgroup writes its partial gradient vectors and loss terms with nothing added to them;
 * workgroup 0 adds them in exactly the order that kernel's passes add to its one vector: a critic gradient ((P0 + P1) + P2) + P3; an
 * actor gradient with CAPS on  M0 + C0 + M1 + C1 + ..  left to right (Mc: chunk c's main pass, Cc: its spatial CAPS pass; Mc and Cc are
 * never added to each other first); td = 0 + P0(Q1) + P0(Q2) + P1(Q1) + ..; pg = P0 + P1 + ..; the clip norm over the summed vector
 * with one workgroup's thread stride.  So every array written equals serl_td3_train_big's bit for bit, and with batch <= 128
 * serl_td3_train / _mfma / _rng's (G = 1: one workgroup per learner that waits on nothing).
 * Hand-overs (G > 1), per update: A every workgroup's critic partials and TD terms -> workgroup 0; B the stepped critic -> every
 * workgroup; at actor updates C the actor partials and pg terms -> workgroup 0; D the stepped actor and both targets -> every
 * workgroup (B and D are left out when nothing follows them).  Producer: its stores drained, the workgroup's barrier, one lane's
 * agent-scope release fence, then that lane's relaxed agent-scope atomic on the learner's word -- an add to the arrival count (A, C) or
 * a store of the epoch, which counts the learner's B / D hand-overs of the call from 1 (never 0).  Consumer: one wavefront polls the
 * word relaxed with s_sleep, then one agent-scope acquire fence, its loads drained, the workgroup's barrier, and only then plain vector
 * loads of what was handed over.  The polled words and a time-out word, 16 bytes per learner, stand at the start of `work` and are
 * zeroed on the stream (hipMemsetAsync) before every launch.  Every spin is bounded by 4 s of the 100 MHz wall clock: the workgroup
 * whose wait expires writes the hand-over's code to the time-out word, every workgroup of that learner sees it at its next poll and
 * returns, and status[p] holds the code -- whatever the rows of that learner hold then is unfinished.  A launch cannot hang.
 *   rng, dense  as in serl_td3_big_desc
 *   status      DEVICE i32 [n_learners]: 0 = the learner ran, else enum serl_td3_wide_status.  Written by the kernel only (not by a call
 *               with n_updates == 0 or a refused one); read it behind the stream's synchronisation.
 *   work        serl_td3_wide_work_bytes(n_learners, S, A, hidden, num_layers, batch) =
 *                   serl_td3_big_work_bytes(...) + n_learners * (G * (3 * gf + 4) * 4 + 16)   bytes
 *               with gf = max(actor parameters, serl_td3_param_count(S, A)) rounded up to a multiple of 4: per chunk three partial gradient
 *               vectors (critic, actor main pass, actor CAPS pass) and four loss words, per learner the 16-byte synchronisation block;
 *               a multiple of 16; 0 where serl_td3_big_work_bytes is 0.  The library zeroes the synchronisation blocks itself. */
typedef struct serl_td3_wide_desc {
  const serl_td3_rng_desc *rng;     /* HOST; NULL = tables */
  int32_t *status;                  /* DEVICE [n_learners] */
  int32_t dense;                    /* 0 = valu, 1 = mfma */
  int32_t pad0;
} serl_td3_wide_desc;
enum serl_td3_wide_status {
  SERL_TD3_WIDE_OK = 0,
  SERL_TD3_WIDE_A = 1,              /* a wait of hand-over A ran out of time */
  SERL_TD3_WIDE_B = 2,
  SERL_TD3_WIDE_C = 3,
  SERL_TD3_WIDE_D = 4
};
/* layout self-check: sizeof(serl_td3_wide_desc), then offsetof of each member in declaration order */
int serl_td3_wide_layout(int32_t *out, int32_t capacity);
int64_t serl_td3_wide_work_bytes(int32_t n_learners, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers, int32_t batch);
/* Asynchronous on `stream`: one memset of the synchronisation blocks and one launch.  SERL_E_INVALID for a NULL wide, dense other than
 * 0 / 1 or a NULL status; then the checks of serl_td3_train_big in their order with their codes (the workspace that of
 * serl_td3_wide_work_bytes); then SERL_E_UNSUPPORTED when n_learners * G exceeds the device's CU count (the workgroups wait on each
 * other, so all must be resident: one per CU by LDS size); all before any device work.  n_updates == 0 leaves every buffer unchanged. */
int serl_td3_train_wide(serl_ctx *ctx, const serl_td3_desc *desc, const serl_td3_wide_desc *wide, void *stream);

/* ---- a group of independent TD3 learners on minibatches of up to 512 rows, chunks serial or parallel (SERL_ABI_VERSION stays 9: two new
 * symbols and four enumerators, no struct added or moved) -------------------------------------------------------------------------------
 * serl_td3_train_group is compiled for batch 1 .. 128.  These two take its descriptors -- the same serl_td3_desc with everything a row
 * holds ignored, the same serl_td3_group_desc and serl_td3_learner_row -- with batch 1 .. 512, G = ceil(batch / 128) chunks:
 *   serl_td3_train_group_big    one workgroup per learner that walks the chunks one after the other, as serl_td3_train_big does;
 *                               workspace serl_td3_big_work_bytes(n_learners, ...), laid out per learner as that entry lays it out.
 *   serl_td3_train_group_wide   a grid of G x n_learners workgroups, workgroup (ch, p) on chunk ch of learner p with serl_td3_train_wide's
 *                               hand-overs inside the learner; workspace serl_td3_wide_work_bytes(n_learners, ...): the 16-byte
 *                               synchronisation blocks of all learners first (zeroed on the stream before the launch), then per learner
 *                               what serl_td3_train_wide lays out.
 * Further instantiations of the one kernel source.  No workgroup of one learner ever waits on a workgroup of another, and there is no
 * grid-wide synchronisation.
 * Rows and status.  Every workgroup of learner p reads rows[p] and checks it itself before it touches any other memory; the check is a
 * function of the row and the descriptor alone, so the G workgroups of a learner agree without talking.  A refused learner's workgroups
 * all return at once: they write nothing, the synchronisation words included, and none of them is ever waited for; workgroup (0, p) alone
 * writes status[p].  The learners of a launch run their own rows' n_updates, 0 included: every hand-over of a learner is decided from its
 * own row's count (B is left out when nothing follows, D behind ITS last update), so all its workgroups leave behind the same hand-over;
 * a learner with n_updates == 0 makes none and leaves everything but its status unchanged, adam_steps too.
 * status[p] (enum serl_td3_row_status): 0 = the row was accepted and the learner ran to its end; 1 .. 6 = the first failed check, nothing
 * of the learner written; SERL_TD3_ROW_HANDOVER_A .. _D (serl_td3_train_group_wide only) = the row was accepted, then a wait of that
 * hand-over ran out of serl_td3_train_wide's bounded spin: that learner's rows are unfinished, the others are not affected.
 * Contract: every array learner p writes -- its four rows, its four moment rows, its adam_steps pair, td_loss[p], pg_loss[p] -- equals,
 * bit for bit, what a single-learner serl_td3_train_big call (for serl_td3_train_group_wide: serl_td3_train_wide) writes whose
 * descriptor holds the row's ring, capacity, n_updates, iteration0, policy_update_freq, update_actor_target and hyper-parameters and
 * whose rng = {seed, n_rows, learner0 = key, dense, caps}.  Through the contracts of those two it is also what the other of the two
 * writes, and with batch <= 128 what serl_td3_train_group writes.  A learner's result depends neither on the other learners nor on its
 * place in the grid.
 * Asynchronous on `stream`; the launch is made for desc->n_updates == 0 too (the status array is the report).  The checks are
 * serl_td3_train_group's in its order with its codes, with batch up to 512 (513: SERL_E_UNSUPPORTED) and the workspaces above; then, for
 * serl_td3_train_group_wide, SERL_E_UNSUPPORTED when n_learners * G exceeds the device's CU count (the workgroups of a learner wait on
 * each other, so all must be resident); all with nothing launched.  serl_last_error() names the entry. */
int serl_td3_train_group_big(serl_ctx *ctx, const serl_td3_desc *desc, const serl_td3_group_desc *group, void *stream);
int serl_td3_train_group_wide(serl_ctx *ctx, const serl_td3_desc *desc, const serl_td3_group_desc *group, void *stream);

/* ---- the launch planner on the host (SERL_ABI_VERSION stays 9: new symbols only) --------------------------------------------------
 * WHAT serl_rollout / serl_rollout_noise (noise != 0) would launch for `desc` on a device of caps[0] CUs: the library's own decision
 * (csrc/serl_plan.h), without a context or a device.  caps[7] = {CUs, SERL_KERNEL as enum serl_kernel_hint (0 = unset),
 * SERL_WAVES_PER_BLOCK (-1 = unset), SERL_LANEQ_WAVES (-1), SERL_SPLIT_ACTOR (0), SERL_REMOTE_ACTOR (1), 1 unless SERL_LANE_WEIGHTS=rows}.
 * Reads the integer fields of desc and the alignment of desc->weights, never what a pointer points to.  Runs the descriptor checks of
 * serl_rollout that need no context, then the plan: returns the status serl_rollout would, message in serl_last_error.  out[0..7] = the
 * words of serl_last_rollout_info with code = -1; out[8] threads per workgroup, [9] RolloutArgs.lanes, [10] first queued episode, [11]
 * weights regrouped, [12] mailbox bytes zeroed, [13] timing events recorded, [14] episodes per launch, [15] 0.  All zero on a refusal.
 * SERL_E_INVALID for a NULL argument, caps[0] < 1 or n_episodes < 1. */
int serl_host_plan_rollout(const int32_t caps[7], const serl_rollout_desc *desc, int32_t noise, int32_t out[16]);
/* ... of serl_rollout_regrouped (noise != 0: with a noise descriptor): the words of serl_host_plan_rollout for the same descriptor with out[11] == 1, and
 * the refusals of the entry point (a hint that does not resolve to LANEG, n_members > 1 << 22, everything LANEG refuses).  caps[6] == 0
 * (SERL_LANE_WEIGHTS=rows) does not apply: the caller asked for the copy by name. */
int serl_host_plan_rollout_regrouped(const int32_t caps[7], const serl_rollout_desc *desc, int32_t noise, int32_t out[16]);
/* ... of serl_dyn_open_loop */
int serl_host_plan_dyn(const int32_t caps[7], int32_t n_episodes, int32_t lanes_per_wave, int32_t kernel_hint, int32_t out[16]);
/* ... the workgroups serl_rollout_multi gives its n <= 4 parts of episodes[k] episodes under placement `place` (SERL_MIXED_PLACE): grids
 * i32 [n], *queue = every part drains a work queue on its share of the CUs, *place_out = the placement the launch uses. */
int serl_host_plan_multi(int32_t num_cus, int32_t n, const int32_t *episodes, int32_t place, int32_t *grids, int32_t *queue, int32_t *place_out);

/* ---- which kernel takes an actor shape (SERL_ABI_VERSION stays 9: new symbols only) --------------------------------------------------
 * The shape contract of an entry point -- the library's own predicate (csrc/serl_shapes.h), the one the entry point refuses through --
 * without a launch and without a device. */
enum serl_shape_kernel {
  SERL_SHAPE_GA_SENSITIVITY = 0,           /* serl_ga_sensitivity */
  SERL_SHAPE_GA_NOVELTY = 1,               /* serl_ga_novelty */
  SERL_SHAPE_GA_DISTILL = 2,               /* serl_ga_distill (batch is not read) */
  SERL_SHAPE_TD3_TRAIN = 3,                /* serl_td3_train: minibatches of up to 128 rows; the LDS of the flavours that read tables */
  SERL_SHAPE_TD3_TRAIN_BIG = 4,            /* serl_td3_train_big: up to 512 rows */
  SERL_SHAPE_GA_SENSITIVITY_GENERAL = 5,   /* serl_ga_sensitivity_general */
  SERL_SHAPE_GA_NOVELTY_GENERAL = 6,       /* serl_ga_novelty_general (batch: its max_batch) */
  SERL_SHAPE_GA_DISTILL_GENERAL = 7,       /* serl_ga_distill_general (batch is not read) */
  SERL_SHAPE_VENV_ROLLOUT = 8,             /* serl_venv_rollout; these two have no minibatch: `batch` is the env, env_config + 3 x (incremental != 0) */
  SERL_SHAPE_VENV_ROLLOUT_GENERAL = 9,     /* serl_venv_rollout_general and serl_venv_rollout_wave */
  SERL_SHAPE_KERNELS = 10
};
enum serl_shape_why { SERL_SHAPE_WHY_TAKES = 0, SERL_SHAPE_WHY_RANGE = 1, SERL_SHAPE_WHY_LDS = 2 };
/* Returns what the entry point returns for this shape when nothing else is wrong with the call -- SERL_OK, or the code of its refusal with
 * the entry point's own message in serl_last_error.  The LDS a workgroup may take is the context's (the device's sharedMemPerBlockOptin);
 * with a NULL ctx, lds_bytes.  *why (may be NULL) tells the two refusals apart: outside the compiled range, or in range and too large for
 * the LDS.  SERL_E_INVALID (why RANGE) for an unknown kernel. */
int serl_shape_query(const serl_ctx *ctx, int32_t kernel, int32_t state_dim, int32_t action_dim, int32_t hidden, int32_t num_layers,
                     int32_t activation, int32_t batch, int64_t lds_bytes, int32_t *why);

#ifdef __cplusplus
}
#endif
#endif /* SERL_AMD_H */

// venv_variant.inc -- the step-wise vector env (CitationEnv.reset / .step, envs/phlabenv.py:401-482; serl_venv_reset /
// serl_venv_step in include/serl_amd.h), instantiated once per dynamics code variant (VARIANT) behind rollout_variant.inc, whose
// LDS staging (serl_stage_and_index_<v>) and dynamics step (cit_step_<v>) it reuses.  Inside namespace bdag.
//
// One lane = one env, per call: load the env's state from the caller's SoA buffer (rollout_device.h SerlVenvF64 / SerlVenvI32) into
// a CitCtx in the kernel's stack frame -- so that CitCtx.dwm points at this lane's private copy of the banks, as in the lane
// rollout kernels --, run one reset() or step(), store the state back.  The glue is the lane / wave rollout kernels' own
// (rollout_variant.inc, rollout_wave.inc X = true): all three env configurations and incremental control, widths from the descriptor.
#define VV_PASTE2(a, b) a##b
#define VV_PASTE(a, b) VV_PASTE2(a, b)
#define VV_NAME(x) VV_PASTE(x, VARIANT)
// SERL_VENV_NOISE (family_lanenz.hip): the same text a second time as the kernels of serl_venv_*_noise (include/serl_amd.h serl_venv_noise_desc), in which
// the sensor-noise row and the action-noise row come out of the counter-based generator (serl_rng.h) where nz.sensor / nz.action say so, and every episode
// start counts in nz.episode_count.  Without it the VV_NZ_* macros are empty and VV_SENSOR / VV_ACTION_NOISE_* are the table reads they replace.
#ifdef SERL_VENV_NOISE
#define VV_KNAME(x) VV_PASTE(VV_PASTE(x, noise_), VARIANT)
#define VV_NZ_PARAM , serl_venv_noise_desc nz
#define VV_NZ_LOCALS double nzsn[7], nzan[3]; int32_t nzep = 0; (void)nzan;
#define VV_NZ_START nzep = nz.episode_count[e]; nz.episode_count[e] = nzep + 1;      /* an explicit reset: the episode it starts has the ordinal the count had */
#define VV_NZ_LOAD nzep = nz.episode_count[e] - 1;                                   /* the running episode's ordinal */
#define VV_NZ_RESTART nzep += 1;
#define VV_NZ_STORE nz.episode_count[e] = nzep + 1;
#define VV_SENSOR(j) serl_venv_sensor_nz(d, nz, e, nzep, j, nzsn)
#define VV_ACTION_NOISE_ON (rd.action_noise || nz.action)
#define VV_ACTION_NOISE_ROW serl_venv_action_nz(rd, nz, kn, e, nzep, k, nzan)
#else
#define VV_KNAME(x) VV_NAME(x)
#define VV_NZ_PARAM
#define VV_NZ_LOCALS
#define VV_NZ_START
#define VV_NZ_LOAD
#define VV_NZ_RESTART
#define VV_NZ_STORE
#define VV_SENSOR(j) serl_venv_sensor(d, e, j)
#define VV_ACTION_NOISE_ON rd.action_noise
#define VV_ACTION_NOISE_ROW rd.action_noise + kn * 3
#endif

#ifndef SERL_VENV_COMMON
#define SERL_VENV_COMMON
// the outputs of an env that does not move in this call (not in the reset mask; stepped while done / never reset): its current
// observation from the stored state, and (step) the stored x / ref / t / cost with reward 0 and done = 1
static __device__ __forceinline__ void serl_venv_write_frozen(const VenvArgs &v, int e, bool step)
{
  const serl_venv_desc &d = v.d;
  const double *S = (const double *)d.state;
  const int32_t *I = (const int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  double err[3], u[3], x[12];
  for (int i = 0; i < 3; ++i) { err[i] = S[(SERL_VF_ERR + i) * np + e]; u[i] = S[(SERL_VF_LASTU + i) * np + e]; }
  for (int i = 0; i < 12; ++i) x[i] = S[(SERL_VF_XO + i) * np + e];
  serl_write_obs(d.env_config, d.incremental != 0, err, x, u, v.obs + (size_t)e * d.state_dim);
  if (!step) return;
  v.reward[e] = 0.0;
  v.done[e] = 1;
  if (v.x) for (int i = 0; i < 12; ++i) v.x[(size_t)e * 12 + i] = x[i];
  if (v.ref) for (int i = 0; i < 3; ++i) v.ref[(size_t)e * 3 + i] = S[(SERL_VF_REF + i) * np + e];
  if (v.t) v.t[e] = S[SERL_VF_T * np + e];
  if (v.cost) v.cost[e] = I[SERL_VI_COST * np + e];
}

// the row of pre-drawn sensor noise env e adds to what step() returns at entry j (0: the step of reset(), k + 1: env step k), or nullptr
static __device__ __forceinline__ const double *serl_venv_sensor(const serl_venv_desc &d, int e, int j)
{
  if (!d.sensor_noise) return nullptr;
  const int sr = d.sensor_row ? d.sensor_row[e] : e;
  return sr < 0 ? nullptr : d.sensor_noise + ((size_t)sr * ((size_t)d.max_steps + 1) + (size_t)j) * 7;
}
#ifdef SERL_VENV_NOISE
// ... or, where nz.sensor is set, the row the generator draws for (env e, episode ordinal ep, entry j), into the caller's buffer
static __device__ __forceinline__ const double *serl_venv_sensor_nz(const serl_venv_desc &d, const serl_venv_noise_desc &nz, int e, int32_t ep, int j,
                                                                    double (&buf)[7])
{
  if (!nz.sensor) return serl_venv_sensor(d, e, j);
  serl_rng_sensor(nz.seed, nz.sensor_bias, nz.sensor_scale, e, ep, j, buf);
  return buf;
}

// the action-noise row of step kn: the caller's table, or, where nz.action is set, clip(sd z, +-clip) drawn for (env e, episode ordinal ep, in-episode step k)
static __device__ __forceinline__ const double *serl_venv_action_nz(const serl_venv_rollout_desc &rd, const serl_venv_noise_desc &nz, size_t kn, int e,
                                                                    int32_t ep, int k, double (&buf)[3])
{
  if (!nz.action) return rd.action_noise + kn * 3;
  serl_rng_action(nz.seed, nz.action_sd, nz.action_clip, e, ep, k, buf);
  return buf;
}
#endif
#endif  // SERL_VENV_COMMON

// the dynamics state of env e: state buffer <-> a CitCtx in the caller's stack frame
static __device__ __forceinline__ void VV_NAME(serl_venv_load_ctx_)(const RolloutArgs &a, const VenvArgs &v, int e, CitCtx &ctx)
{
  const double *S = (const double *)v.d.state;
  const int32_t *I = (const int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  for (int i = 0; i < 19; ++i) ctx.X[i] = S[(SERL_VF_X + i) * np + e];
  for (int i = 0; i < 29; ++i) ctx.DW[i] = S[(SERL_VF_DW + i) * np + e];
  for (int i = 0; i < 4; ++i) ctx.IW[i] = I[(SERL_VI_IW + i) * np + e];
  for (int i = 0; i < 8; ++i) ctx.hint[i] = (uint32_t)I[(SERL_VI_HINT + i) * np + e];
  ctx.t = S[SERL_VF_CT * np + e]; ctx.stop_time = S[SERL_VF_CSTOP * np + e];
  ctx.tick = (uint32_t)I[SERL_VI_TICK * np + e]; ctx.err = I[SERL_VI_CERR * np + e];
  ctx.ro = a.ro; ctx.t3 = a.t3; ctx.dt = a.dyn_dt; ctx.major = 1;
  ctx.bslot = 0;      // (SERL_FLAVOUR_LDS == 0 in the lane units: the block signals live in registers)
}

static __device__ __forceinline__ void VV_NAME(serl_venv_store_ctx_)(const VenvArgs &v, int e, const CitCtx &ctx)
{
  double *S = (double *)v.d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  for (int i = 0; i < 19; ++i) S[(SERL_VF_X + i) * np + e] = ctx.X[i];
  for (int i = 0; i < 29; ++i) S[(SERL_VF_DW + i) * np + e] = ctx.DW[i];
  for (int i = 0; i < 4; ++i) I[(SERL_VI_IW + i) * np + e] = ctx.IW[i];
  for (int i = 0; i < 8; ++i) I[(SERL_VI_HINT + i) * np + e] = (int32_t)ctx.hint[i];
  S[SERL_VF_CT * np + e] = ctx.t; S[SERL_VF_CSTOP * np + e] = ctx.stop_time;
  I[SERL_VI_TICK * np + e] = (int32_t)ctx.tick; I[SERL_VI_CERR * np + e] = ctx.err;
}

// reset() of the envs in the mask (envs/phlabenv.py:401-428)
__global__ void __launch_bounds__(SERL_BLOCK) VV_KNAME(serl_venv_reset_kernel_)(RolloutArgs a, VenvArgs v VV_NZ_PARAM)
{
  const int e = VV_NAME(serl_stage_and_index_)(a);
  if (e < 0) return;
  if (v.mask && !v.mask[e]) { serl_venv_write_frozen(v, e, false); return; }
  const serl_venv_desc &d = v.d;
  double *S = (double *)d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  const int A = d.action_dim;
  VV_NZ_LOCALS
  VV_NZ_START
  double err[3], u[3] = {0.0, 0.0, 0.0}, x[12], cmd[10];
  for (int i = 0; i < 3; ++i) err[i] = S[(SERL_VF_ERR + i) * np + e];      // self.error is never cleared
  if (d.err0) for (int i = 0; i < 3; ++i) err[i] = i < A ? d.err0[(size_t)e * 3 + i] : 0.0;
  const uint32_t tick = d.tick0 ? (uint32_t)d.tick0[e] : (uint32_t)I[SERL_VI_TICK * np + e];   // initialize() leaves the clock running
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  CitCtx ctx;
  cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
  if (tick) { ctx.tick = tick; ctx.t = (double)ctx.tick * ctx.dt; }
  ctx.bslot = 0;
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  cmd[0] = serl_clip(cmd[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
  cmd[1] = serl_clip(cmd[1], -f.ail_clip, f.ail_clip);
  if (f.rudder_jam_on != 0.0) cmd[2] = f.rudder_jam;
  VV_NAME(cit_step_)(&ctx, cmd, x);
  if (const double *sn = VV_SENSOR(0)) {
    serl_sensor_add(x, sn);
  }
  VV_NAME(serl_venv_store_ctx_)(v, e, ctx);
  for (int i = 0; i < 3; ++i) {
    S[(SERL_VF_ERR + i) * np + e] = err[i]; S[(SERL_VF_LASTU + i) * np + e] = 0.0; S[(SERL_VF_REF + i) * np + e] = 0.0;
  }
  for (int i = 0; i < 12; ++i) S[(SERL_VF_XO + i) * np + e] = x[i];
  S[SERL_VF_V0 * np + e] = x[3];
  S[SERL_VF_T * np + e] = 0.0;
  I[SERL_VI_K * np + e] = 0;
  I[SERL_VI_LIVE * np + e] = 1;
  I[SERL_VI_COST * np + e] = 0;
  serl_write_obs(d.env_config, d.incremental != 0, err, x, u, v.obs + (size_t)e * d.state_dim);
}

#ifndef SERL_VENV_NOISE      // (the plain step has no noise instantiation: device noise needs auto-reset)
// step(action) of every env (envs/phlabenv.py:430-482)
__global__ void __launch_bounds__(SERL_BLOCK) VV_NAME(serl_venv_step_kernel_)(RolloutArgs a, VenvArgs v)
{
  const int e = VV_NAME(serl_stage_and_index_)(a);
  if (e < 0) return;
  const serl_venv_desc &d = v.d;
  double *S = (double *)d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  if (!I[SERL_VI_LIVE * np + e]) { serl_venv_write_frozen(v, e, true); return; }
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const int cfg = d.env_config, A = d.action_dim;
  const bool incr = d.incremental != 0;
  const double bound = (incr ? 25.0 : 10.0) * deg2rad, low = -bound, high = bound;   // rate bound [rad/s] / deflection bound [rad]
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  double err[3], u[3], x[12], cmd[10];
  for (int i = 0; i < 3; ++i) { err[i] = S[(SERL_VF_ERR + i) * np + e]; u[i] = S[(SERL_VF_LASTU + i) * np + e]; }
  const double V0 = S[SERL_VF_V0 * np + e];
  double t = S[SERL_VF_T * np + e];
  const int k = I[SERL_VI_K * np + e];
  // scale_action (envs/phlabenv.py:62-73) without clipping; incremental control integrates the rate (:377-380,446-450)
  double scl[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i) {
    if (i >= A) continue;
    if (v.actions_f64) {
      const double ai = ((const double *)v.actions)[(size_t)e * A + i];
      scl[i] = low + 0.5 * (ai + 1.0) * (high - low);
    } else {
      const float s = 0.5f * (((const float *)v.actions)[(size_t)e * A + i] + 1.0f);
      scl[i] = low + (double)s * (high - low);
    }
  }
  for (int i = 0; i < 3; ++i) u[i] = incr ? u[i] + scl[i] * dt : scl[i];
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  serl_fault_apply(f, u, cmd);
  CitCtx ctx;
  VV_NAME(serl_venv_load_ctx_)(a, v, e, ctx);
  VV_NAME(cit_step_)(&ctx, cmd, x);
  if (const double *sn = serl_venv_sensor(d, e, k + 1)) {      // k < max_steps: entry k + 1 <= max_steps exists
    serl_sensor_add(x, sn);
  }
  double rk[3];
  if (d.ref_spec) serl_ref_generate(d.ref_spec + (size_t)e * d.ref_spec_stride, t, d.t_max, rk[0], rk[1], rk[2]);   // at the pre-increment t
  else {
    const double *r = d.ref + (size_t)e * d.ref_stride + (size_t)k * 3;
    rk[0] = r[0]; rk[1] = r[1]; rk[2] = r[2];
  }
  err[0] = rk[0] - x[7];
  if (A > 1) { err[1] = rk[1] - x[6]; err[2] = rk[2] - x[5]; }
  double rsum = 0.0;
  for (int i = 0; i < 3; ++i) if (i < A) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
  double reward = -rsum / (double)A;
  const int cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
  const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
  if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
  t += dt;
  const bool done = fin || k + 1 >= d.max_steps;     // (the tables end: the env freezes instead of reading past them)
  VV_NAME(serl_venv_store_ctx_)(v, e, ctx);
  for (int i = 0; i < 3; ++i) {
    S[(SERL_VF_ERR + i) * np + e] = err[i]; S[(SERL_VF_LASTU + i) * np + e] = u[i]; S[(SERL_VF_REF + i) * np + e] = rk[i];
  }
  for (int i = 0; i < 12; ++i) S[(SERL_VF_XO + i) * np + e] = x[i];
  S[SERL_VF_T * np + e] = t;
  I[SERL_VI_K * np + e] = k + 1;
  I[SERL_VI_LIVE * np + e] = done ? 0 : 1;
  I[SERL_VI_COST * np + e] = cost;
  serl_write_obs(cfg, incr, err, x, u, v.obs + (size_t)e * d.state_dim);
  v.reward[e] = reward;
  v.done[e] = done ? 1 : 0;
  if (v.x) for (int i = 0; i < 12; ++i) v.x[(size_t)e * 12 + i] = x[i];
  if (v.ref) for (int i = 0; i < 3; ++i) v.ref[(size_t)e * 3 + i] = rk[i];
  if (v.t) v.t[e] = t;
  if (v.cost) v.cost[e] = cost;
}
#endif

// step(action) of every env, and reset() of those whose episode that step ends, in the same launch (serl_venv_step_auto in
// include/serl_amd.h).  cit_step_<v> is the whole cost and tens of KB inlined, so there is ONE call site in a two-trip loop: the first
// trip is serl_venv_step_kernel_'s step, the second -- entered only by lanes whose episode ended -- is serl_venv_reset_kernel_'s
// initialize() + step with the zero command.  The glue around it is those two kernels', statement for statement.
__global__ void __launch_bounds__(SERL_BLOCK) VV_KNAME(serl_venv_step_auto_kernel_)(RolloutArgs a, VenvArgs v, serl_venv_auto_desc au VV_NZ_PARAM)
{
  const int e = VV_NAME(serl_stage_and_index_)(a);
  if (e < 0) return;
  const serl_venv_desc &d = v.d;
  double *S = (double *)d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  double *fobs = au.final_obs + (size_t)e * d.state_dim;
  if (!I[SERL_VI_LIVE * np + e]) {      // never reset: frozen, as in serl_venv_step
    serl_venv_write_frozen(v, e, true);
    for (int i = 0; i < d.state_dim; ++i) fobs[i] = v.obs[(size_t)e * d.state_dim + i];
    return;
  }
  VV_NZ_LOCALS
  VV_NZ_LOAD
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const int cfg = d.env_config, A = d.action_dim;
  const bool incr = d.incremental != 0;
  const double bound = (incr ? 25.0 : 10.0) * deg2rad, low = -bound, high = bound;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  double err[3], u[3], x[12], cmd[10], rk[3];
  for (int i = 0; i < 3; ++i) { err[i] = S[(SERL_VF_ERR + i) * np + e]; u[i] = S[(SERL_VF_LASTU + i) * np + e]; }
  const double V0 = S[SERL_VF_V0 * np + e];
  double t = S[SERL_VF_T * np + e];
  int k = I[SERL_VI_K * np + e];
  double scl[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i) {
    if (i >= A) continue;
    if (v.actions_f64) {
      const double ai = ((const double *)v.actions)[(size_t)e * A + i];
      scl[i] = low + 0.5 * (ai + 1.0) * (high - low);
    } else {
      const float s = 0.5f * (((const float *)v.actions)[(size_t)e * A + i] + 1.0f);
      scl[i] = low + (double)s * (high - low);
    }
  }
  for (int i = 0; i < 3; ++i) u[i] = incr ? u[i] + scl[i] * dt : scl[i];
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  serl_fault_apply(f, u, cmd);
  // the running episode's reference: its row of the pool (the cursor is the caller's memory: kept inside the pool whatever it holds)
  const int32_t cur = au.cursor[e];
  const int row = au.ref_pool ? (int)((uint32_t)cur % (uint32_t)au.pool_rows) : 0;
  const serl_ref_spec *spec = au.ref_pool ? au.ref_pool + (size_t)e * au.pool_rows + row
                            : d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
  int cost = 0;
  double V0n = V0;
  bool restart = false;
  CitCtx ctx;
  VV_NAME(serl_venv_load_ctx_)(a, v, e, ctx);
#pragma nounroll
  for (int trip = 0; trip < 2; ++trip) {
    VV_NAME(cit_step_)(&ctx, cmd, x);
    if (const double *sn = VV_SENSOR(restart ? 0 : k + 1)) {
      serl_sensor_add(x, sn);
    }
    if (restart) { V0n = x[3]; break; }
    if (spec) serl_ref_generate(spec, t, d.t_max, rk[0], rk[1], rk[2]);
    else {
      const double *r = d.ref + (size_t)e * d.ref_stride + (size_t)k * 3;
      rk[0] = r[0]; rk[1] = r[1]; rk[2] = r[2];
    }
    err[0] = rk[0] - x[7];
    if (A > 1) { err[1] = rk[1] - x[6]; err[2] = rk[2] - x[5]; }
    double rsum = 0.0;
    for (int i = 0; i < 3; ++i) if (i < A) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
    double reward = -rsum / (double)A;
    cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
    const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
    if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
    t += dt;
    k += 1;
    const bool done = fin || k >= d.max_steps;
    serl_write_obs(cfg, incr, err, x, u, fobs);
    v.reward[e] = reward;
    v.done[e] = done ? 1 : 0;
    if (v.x) for (int i = 0; i < 12; ++i) v.x[(size_t)e * 12 + i] = x[i];
    if (v.ref) for (int i = 0; i < 3; ++i) v.ref[(size_t)e * 3 + i] = rk[i];
    if (v.t) v.t[e] = t;
    if (v.cost) v.cost[e] = cost;
    const double ret = au.run_return[e] + reward;
    const int32_t len = au.run_length[e] + 1;
    if (!done) { au.run_return[e] = ret; au.run_length[e] = len; break; }
    au.ep_return[e] = ret; au.ep_length[e] = len;
    au.run_return[e] = 0.0; au.run_length[e] = 0;
    au.cursor[e] = au.ref_pool ? (row + 1) % au.pool_rows : (int32_t)(((uint32_t)cur + 1u) & 0x7fffffffu);      // (no pool: restarts counted, wrapping to 0)
    // reset() of this env (serl_venv_reset_kernel_ without err0 / tick0): the error stays, the clock keeps counting
    restart = true;
    VV_NZ_RESTART
    const uint32_t tick = ctx.tick;
    cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
    if (tick) { ctx.tick = tick; ctx.t = (double)ctx.tick * ctx.dt; }
    ctx.bslot = 0;
    for (int i = 0; i < 3; ++i) { u[i] = 0.0; rk[i] = 0.0; }
    t = 0.0; k = 0; cost = 0;
    for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
    cmd[0] = serl_clip(cmd[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
    cmd[1] = serl_clip(cmd[1], -f.ail_clip, f.ail_clip);
    if (f.rudder_jam_on != 0.0) cmd[2] = f.rudder_jam;
  }
  VV_NAME(serl_venv_store_ctx_)(v, e, ctx);
  for (int i = 0; i < 3; ++i) {
    S[(SERL_VF_ERR + i) * np + e] = err[i]; S[(SERL_VF_LASTU + i) * np + e] = u[i]; S[(SERL_VF_REF + i) * np + e] = rk[i];
  }
  for (int i = 0; i < 12; ++i) S[(SERL_VF_XO + i) * np + e] = x[i];
  S[SERL_VF_V0 * np + e] = V0n;
  S[SERL_VF_T * np + e] = t;
  I[SERL_VI_K * np + e] = k;
  I[SERL_VI_LIVE * np + e] = 1;
  I[SERL_VI_COST * np + e] = cost;
  VV_NZ_STORE
  serl_write_obs(cfg, incr, err, x, u, v.obs + (size_t)e * d.state_dim);
}

// K policy-driven steps of every env in one launch (serl_venv_rollout in include/serl_amd.h): per step the lane's own actor on the
// current observation (lane_actor.h serl_actor_forward_lane32 on the member's plain row, a.d holds the actor shape), the action path
// of rollout_variant.inc, then serl_venv_step_auto_kernel_'s step, statement for statement.  The CitCtx, the env scalars and the run
// state are loaded once and stored once; the outputs are step-major rows [k][n_envs].  Attitude task without rate control only
// (7 observations, 3 actions: the lane actor's shape), so cfg / A / incr are constants here.  ONE call site of the actor and ONE of
// cit_step_<v>: the two-trip loop sits inside the K loop, both rolled.
__global__ void __launch_bounds__(SERL_BLOCK) VV_KNAME(serl_venv_rollout_kernel_)(RolloutArgs a, VenvArgs v, serl_venv_auto_desc au, serl_venv_rollout_desc rd VV_NZ_PARAM)
{
  const int e = VV_NAME(serl_stage_and_index_)(a);
  if (e < 0) return;
  const serl_venv_desc &d = v.d;
  double *S = (double *)d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  const size_t N = (size_t)d.n_envs;
  const int K = rd.n_steps;
  constexpr int cfg = SERL_ENV_ATTITUDE, A = 3;
  constexpr bool incr = false;
  double err[3], u[3], x[12], obs[7];
  for (int i = 0; i < 3; ++i) { err[i] = S[(SERL_VF_ERR + i) * np + e]; u[i] = S[(SERL_VF_LASTU + i) * np + e]; }
  for (int i = 0; i < 12; ++i) x[i] = S[(SERL_VF_XO + i) * np + e];
  serl_write_obs(cfg, incr, err, x, u, obs);      // the current observation, as serl_venv_write_frozen rebuilds it
  for (int i = 0; i < 7; ++i) rd.obs[(size_t)e * 7 + i] = obs[i];
  if (!I[SERL_VI_LIVE * np + e]) {      // never reset: frozen in every row, as in serl_venv_step_auto (no action: zeros; the transition marks itself terminal)
    const double rf[3] = {S[(SERL_VF_REF + 0) * np + e], S[(SERL_VF_REF + 1) * np + e], S[(SERL_VF_REF + 2) * np + e]};
    const double tf = S[SERL_VF_T * np + e];
    const int32_t cf = I[SERL_VI_COST * np + e];
#pragma nounroll
    for (int kk = 0; kk < K; ++kk) {
      const size_t kn = (size_t)kk * N + (size_t)e;
      for (int i = 0; i < 7; ++i) rd.obs[(kn + N) * 7 + i] = obs[i];
      if (rd.actions) for (int i = 0; i < 3; ++i) rd.actions[kn * 3 + i] = 0.0;
      if (rd.reward) rd.reward[kn] = 0.0;
      if (rd.done) rd.done[kn] = 1;
      if (rd.final_obs) for (int i = 0; i < 7; ++i) rd.final_obs[kn * 7 + i] = obs[i];
      if (rd.x) for (int i = 0; i < 12; ++i) rd.x[kn * 12 + i] = x[i];
      if (rd.ref) for (int i = 0; i < 3; ++i) rd.ref[kn * 3 + i] = rf[i];
      if (rd.t) rd.t[kn] = tf;
      if (rd.cost) rd.cost[kn] = cf;
      if (rd.transitions) {
        float *tr = rd.transitions + kn * 20;
        for (int i = 0; i < 7; ++i) { tr[i] = (float)obs[i]; tr[10 + i] = (float)obs[i]; }
        tr[7] = 0.0f; tr[8] = 0.0f; tr[9] = 0.0f;
        tr[17] = 0.0f; tr[18] = 1.0f; tr[19] = cf ? 1.0f : 0.0f;
      }
    }
    return;
  }
  VV_NZ_LOCALS
  VV_NZ_LOAD
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const double bound = (incr ? 25.0 : 10.0) * deg2rad, low = -bound, high = bound;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  double cmd[10], rk[3] = {0.0, 0.0, 0.0};
  double V0 = S[SERL_VF_V0 * np + e];
  double t = S[SERL_VF_T * np + e];
  int k = I[SERL_VI_K * np + e];
  int cost = 0;
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  // the env's member of the packed population (the index is the caller's memory: kept inside the population whatever it holds)
  const unsigned member = rd.member_of_env ? (unsigned)rd.member_of_env[e] % (unsigned)rd.n_members : 0u;
  const float *w = rd.weights + (size_t)member * rd.weight_stride;
  int32_t cur = au.cursor[e];
  double run_return = au.run_return[e];
  int32_t run_length = au.run_length[e];
  CitCtx ctx;
  VV_NAME(serl_venv_load_ctx_)(a, v, e, ctx);
#pragma nounroll
  for (int kk = 0; kk < K; ++kk) {
    const size_t kn = (size_t)kk * N + (size_t)e;
    float obsf[7], act[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 7; ++i) obsf[i] = (float)obs[i];
    serl_actor_forward_lane32(a.d, w, obsf, act);
    // ---- the action path of rollout_variant.inc
    if (VV_ACTION_NOISE_ON) {
      const double *noise = VV_ACTION_NOISE_ROW;
      for (int i = 0; i < 3; ++i) {
        double an = serl_clip((double)act[i] + noise[i], -1.0, 1.0);
        u[i] = low + 0.5 * (an + 1.0) * (high - low);
        act[i] = (float)an;     // the transition holds the action that was executed (agent.py:93,103)
        if (rd.actions) rd.actions[kn * 3 + i] = an;
      }
    } else {
      for (int i = 0; i < 3; ++i) {
        float s = 0.5f * (act[i] + 1.0f);
        u[i] = low + (double)s * (high - low);
        if (rd.actions) rd.actions[kn * 3 + i] = (double)act[i];
      }
    }
    // ---- the step of serl_venv_step_auto_kernel_
    for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
    serl_fault_apply(f, u, cmd);
    const int row = au.ref_pool ? (int)((uint32_t)cur % (uint32_t)au.pool_rows) : 0;
    const serl_ref_spec *spec = au.ref_pool ? au.ref_pool + (size_t)e * au.pool_rows + row
                              : d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
    double V0n = V0;
    bool restart = false;
#pragma nounroll
    for (int trip = 0; trip < 2; ++trip) {
      VV_NAME(cit_step_)(&ctx, cmd, x);
      if (const double *sn = VV_SENSOR(restart ? 0 : k + 1)) {
        serl_sensor_add(x, sn);
      }
      if (restart) { V0n = x[3]; break; }
      if (spec) serl_ref_generate(spec, t, d.t_max, rk[0], rk[1], rk[2]);
      else {
        const double *r = d.ref + (size_t)e * d.ref_stride + (size_t)k * 3;
        rk[0] = r[0]; rk[1] = r[1]; rk[2] = r[2];
      }
      err[0] = rk[0] - x[7];
      if (A > 1) { err[1] = rk[1] - x[6]; err[2] = rk[2] - x[5]; }
      double rsum = 0.0;
      for (int i = 0; i < 3; ++i) if (i < A) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
      double reward = -rsum / (double)A;
      cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
      const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
      if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
      t += dt;
      k += 1;
      const bool done = fin || k >= d.max_steps;
      if (rd.final_obs) serl_write_obs(cfg, incr, err, x, u, rd.final_obs + kn * 7);
      if (rd.reward) rd.reward[kn] = reward;
      if (rd.done) rd.done[kn] = done ? 1 : 0;
      if (rd.x) for (int i = 0; i < 12; ++i) rd.x[kn * 12 + i] = x[i];
      if (rd.ref) for (int i = 0; i < 3; ++i) rd.ref[kn * 3 + i] = rk[i];
      if (rd.t) rd.t[kn] = t;
      if (rd.cost) rd.cost[kn] = cost;
      if (rd.transitions) {      // the row of rollout_variant.inc: the next observation is the terminal-aware one, never the restarted one
        float *tr = rd.transitions + kn * 20;
        double nobs[7];
        serl_write_obs(cfg, incr, err, x, u, nobs);
        for (int i = 0; i < 7; ++i) tr[i] = (float)obs[i];
        for (int i = 0; i < 3; ++i) tr[7 + i] = act[i];
        for (int i = 0; i < 7; ++i) tr[10 + i] = (float)nobs[i];
        tr[17] = (float)reward; tr[18] = fin ? 1.0f : 0.0f; tr[19] = cost ? 1.0f : 0.0f;
      }
      const double ret = run_return + reward;
      const int32_t len = run_length + 1;
      if (!done) { run_return = ret; run_length = len; break; }
      if (rd.ep_return) rd.ep_return[kn] = ret;
      if (rd.ep_length) rd.ep_length[kn] = len;
      if (au.ep_return) au.ep_return[e] = ret;      // (the env's own "last finished episode", as a step() at this point would leave it)
      if (au.ep_length) au.ep_length[e] = len;
      run_return = 0.0; run_length = 0;
      cur = au.ref_pool ? (row + 1) % au.pool_rows : (int32_t)(((uint32_t)cur + 1u) & 0x7fffffffu);
      // reset() of this env, as in serl_venv_step_auto_kernel_: the error stays, the clock keeps counting
      restart = true;
      VV_NZ_RESTART
      const uint32_t tick = ctx.tick;
      cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
      if (tick) { ctx.tick = tick; ctx.t = (double)ctx.tick * ctx.dt; }
      ctx.bslot = 0;
      for (int i = 0; i < 3; ++i) { u[i] = 0.0; rk[i] = 0.0; }
      t = 0.0; k = 0; cost = 0;
      for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
      cmd[0] = serl_clip(cmd[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
      cmd[1] = serl_clip(cmd[1], -f.ail_clip, f.ail_clip);
      if (f.rudder_jam_on != 0.0) cmd[2] = f.rudder_jam;
    }
    V0 = V0n;
    serl_write_obs(cfg, incr, err, x, u, obs);
    for (int i = 0; i < 7; ++i) rd.obs[(kn + N) * 7 + i] = obs[i];
  }
  VV_NAME(serl_venv_store_ctx_)(v, e, ctx);
  for (int i = 0; i < 3; ++i) {
    S[(SERL_VF_ERR + i) * np + e] = err[i]; S[(SERL_VF_LASTU + i) * np + e] = u[i]; S[(SERL_VF_REF + i) * np + e] = rk[i];
  }
  for (int i = 0; i < 12; ++i) S[(SERL_VF_XO + i) * np + e] = x[i];
  S[SERL_VF_V0 * np + e] = V0;
  S[SERL_VF_T * np + e] = t;
  I[SERL_VI_K * np + e] = k;
  I[SERL_VI_LIVE * np + e] = 1;
  I[SERL_VI_COST * np + e] = cost;
  au.run_return[e] = run_return; au.run_length[e] = run_length; au.cursor[e] = cur;
  VV_NZ_STORE
}

// The same K policy-driven steps for EVERY env configuration and actor shape (serl_venv_rollout_general in include/serl_amd.h): cfg, incr, S and A
// come from the env descriptor at run time, as in serl_venv_step_auto_kernel_ -- whose action path, err / reward / write_obs handling for A == 1 and
// incremental command are taken statement for statement, the noise and f32 forms from the general-env branch of the wave kernels (rollout_wave.inc) --
// and the actor is lane_actor.h serl_actor_forward_lane_general (its two activation vectors in private memory).  Rows are [k][N][S], [k][N][A] and
// [k][N][2 S + A + 3]; action_noise stays [K][N][3], of which the first A columns are read.  ONE call site of the actor and ONE of cit_step_<v>, both loops
// rolled, exactly as above.
__global__ void __launch_bounds__(SERL_BLOCK) VV_KNAME(serl_venv_rollout_general_kernel_)(RolloutArgs a, VenvArgs v, serl_venv_auto_desc au, serl_venv_rollout_desc rd VV_NZ_PARAM)
{
  const int e = VV_NAME(serl_stage_and_index_)(a);
  if (e < 0) return;
  const serl_venv_desc &d = v.d;
  double *S_ = (double *)d.state;
  int32_t *I = (int32_t *)(S_ + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  const size_t N = (size_t)d.n_envs;
  const int K = rd.n_steps;
  const int cfg = d.env_config, A = d.action_dim, S = d.state_dim;
  const bool incr = d.incremental != 0;
  const int TW = 2 * S + A + 3;
  double err[3], u[3], x[12], obs[16];
  for (int i = 0; i < 3; ++i) { err[i] = S_[(SERL_VF_ERR + i) * np + e]; u[i] = S_[(SERL_VF_LASTU + i) * np + e]; }
  for (int i = 0; i < 12; ++i) x[i] = S_[(SERL_VF_XO + i) * np + e];
#pragma unroll
  for (int i = 0; i < 16; ++i) obs[i] = 0.0;
  serl_write_obs(cfg, incr, err, x, u, obs);      // the current observation, as serl_venv_write_frozen rebuilds it
#pragma unroll
  for (int i = 0; i < 16; ++i) if (i < S) rd.obs[(size_t)e * S + i] = obs[i];
  if (!I[SERL_VI_LIVE * np + e]) {      // never reset: frozen in every row, as in serl_venv_step_auto (no action: zeros; the transition marks itself terminal)
    const double rf[3] = {S_[(SERL_VF_REF + 0) * np + e], S_[(SERL_VF_REF + 1) * np + e], S_[(SERL_VF_REF + 2) * np + e]};
    const double tf = S_[SERL_VF_T * np + e];
    const int32_t cf = I[SERL_VI_COST * np + e];
#pragma nounroll
    for (int kk = 0; kk < K; ++kk) {
      const size_t kn = (size_t)kk * N + (size_t)e;
#pragma unroll
      for (int i = 0; i < 16; ++i) if (i < S) rd.obs[(kn + N) * S + i] = obs[i];
      if (rd.actions) for (int i = 0; i < 3; ++i) if (i < A) rd.actions[kn * A + i] = 0.0;
      if (rd.reward) rd.reward[kn] = 0.0;
      if (rd.done) rd.done[kn] = 1;
      if (rd.final_obs) {
#pragma unroll
        for (int i = 0; i < 16; ++i) if (i < S) rd.final_obs[kn * S + i] = obs[i];
      }
      if (rd.x) for (int i = 0; i < 12; ++i) rd.x[kn * 12 + i] = x[i];
      if (rd.ref) for (int i = 0; i < 3; ++i) rd.ref[kn * 3 + i] = rf[i];
      if (rd.t) rd.t[kn] = tf;
      if (rd.cost) rd.cost[kn] = cf;
      if (rd.transitions) {
        float *tr = rd.transitions + kn * TW;
#pragma unroll
        for (int i = 0; i < 16; ++i) if (i < S) { tr[i] = (float)obs[i]; tr[S + A + i] = (float)obs[i]; }
        for (int i = 0; i < 3; ++i) if (i < A) tr[S + i] = 0.0f;
        tr[2 * S + A] = 0.0f; tr[2 * S + A + 1] = 1.0f; tr[2 * S + A + 2] = cf ? 1.0f : 0.0f;
      }
    }
    return;
  }
  VV_NZ_LOCALS
  VV_NZ_LOAD
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const double bound = (incr ? 25.0 : 10.0) * deg2rad, low = -bound, high = bound;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  double cmd[10], rk[3] = {0.0, 0.0, 0.0};
  double V0 = S_[SERL_VF_V0 * np + e];
  double t = S_[SERL_VF_T * np + e];
  int k = I[SERL_VI_K * np + e];
  int cost = 0;
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  // the env's member of the packed population (the index is the caller's memory: kept inside the population whatever it holds)
  const unsigned member = rd.member_of_env ? (unsigned)rd.member_of_env[e] % (unsigned)rd.n_members : 0u;
  const float *w = rd.weights + (size_t)member * rd.weight_stride;
  int32_t cur = au.cursor[e];
  double run_return = au.run_return[e];
  int32_t run_length = au.run_length[e];
  CitCtx ctx;
  VV_NAME(serl_venv_load_ctx_)(a, v, e, ctx);
#pragma nounroll
  for (int kk = 0; kk < K; ++kk) {
    const size_t kn = (size_t)kk * N + (size_t)e;
    float obsf[16], act[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 16; ++i) obsf[i] = (float)obs[i];
    serl_actor_forward_lane_general(a.d, w, obsf, act);
    // ---- the action path of serl_venv_step_auto_kernel_ (noise / f32: the general-env branch of the wave kernels)
    double scl[3] = {0.0, 0.0, 0.0};
    if (VV_ACTION_NOISE_ON) {
      const double *noise = VV_ACTION_NOISE_ROW;
      for (int i = 0; i < 3; ++i) {
        if (i >= A) continue;
        double an = serl_clip((double)act[i] + noise[i], -1.0, 1.0);
        scl[i] = low + 0.5 * (an + 1.0) * (high - low);
        act[i] = (float)an;     // the transition holds the action that was executed (agent.py:93,103)
        if (rd.actions) rd.actions[kn * A + i] = an;
      }
    } else {
      for (int i = 0; i < 3; ++i) {
        if (i >= A) continue;
        const float s = 0.5f * (act[i] + 1.0f);
        scl[i] = low + (double)s * (high - low);
        if (rd.actions) rd.actions[kn * A + i] = (double)act[i];
      }
    }
    for (int i = 0; i < 3; ++i) u[i] = incr ? u[i] + scl[i] * dt : scl[i];
    // ---- the step of serl_venv_step_auto_kernel_
    for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
    serl_fault_apply(f, u, cmd);
    const int row = au.ref_pool ? (int)((uint32_t)cur % (uint32_t)au.pool_rows) : 0;
    const serl_ref_spec *spec = au.ref_pool ? au.ref_pool + (size_t)e * au.pool_rows + row
                              : d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
    double V0n = V0;
    bool restart = false;
#pragma nounroll
    for (int trip = 0; trip < 2; ++trip) {
      VV_NAME(cit_step_)(&ctx, cmd, x);
      if (const double *sn = VV_SENSOR(restart ? 0 : k + 1)) {
        serl_sensor_add(x, sn);
      }
      if (restart) { V0n = x[3]; break; }
      if (spec) serl_ref_generate(spec, t, d.t_max, rk[0], rk[1], rk[2]);
      else {
        const double *r = d.ref + (size_t)e * d.ref_stride + (size_t)k * 3;
        rk[0] = r[0]; rk[1] = r[1]; rk[2] = r[2];
      }
      err[0] = rk[0] - x[7];
      if (A > 1) { err[1] = rk[1] - x[6]; err[2] = rk[2] - x[5]; }
      double rsum = 0.0;
      for (int i = 0; i < 3; ++i) if (i < A) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
      double reward = -rsum / (double)A;
      cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
      const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
      if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
      t += dt;
      k += 1;
      const bool done = fin || k >= d.max_steps;
      double nobs[16];
      serl_write_obs(cfg, incr, err, x, u, nobs);      // the terminal-aware next observation: final_obs and the transition row
      if (rd.final_obs) {
#pragma unroll
        for (int i = 0; i < 16; ++i) if (i < S) rd.final_obs[kn * S + i] = nobs[i];
      }
      if (rd.reward) rd.reward[kn] = reward;
      if (rd.done) rd.done[kn] = done ? 1 : 0;
      if (rd.x) for (int i = 0; i < 12; ++i) rd.x[kn * 12 + i] = x[i];
      if (rd.ref) for (int i = 0; i < 3; ++i) rd.ref[kn * 3 + i] = rk[i];
      if (rd.t) rd.t[kn] = t;
      if (rd.cost) rd.cost[kn] = cost;
      if (rd.transitions) {      // (obs S, executed action A, next obs S, reward, fin, cost): the row of the general-env rollout kernels
        float *tr = rd.transitions + kn * TW;
#pragma unroll
        for (int i = 0; i < 16; ++i) if (i < S) { tr[i] = (float)obs[i]; tr[S + A + i] = (float)nobs[i]; }
        for (int i = 0; i < 3; ++i) if (i < A) tr[S + i] = act[i];
        tr[2 * S + A] = (float)reward; tr[2 * S + A + 1] = fin ? 1.0f : 0.0f; tr[2 * S + A + 2] = cost ? 1.0f : 0.0f;
      }
      const double ret = run_return + reward;
      const int32_t len = run_length + 1;
      if (!done) { run_return = ret; run_length = len; break; }
      if (rd.ep_return) rd.ep_return[kn] = ret;
      if (rd.ep_length) rd.ep_length[kn] = len;
      if (au.ep_return) au.ep_return[e] = ret;      // (the env's own "last finished episode", as a step() at this point would leave it)
      if (au.ep_length) au.ep_length[e] = len;
      run_return = 0.0; run_length = 0;
      cur = au.ref_pool ? (row + 1) % au.pool_rows : (int32_t)(((uint32_t)cur + 1u) & 0x7fffffffu);
      // reset() of this env, as in serl_venv_step_auto_kernel_: the error stays, the clock keeps counting
      restart = true;
      VV_NZ_RESTART
      const uint32_t tick = ctx.tick;
      cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
      if (tick) { ctx.tick = tick; ctx.t = (double)ctx.tick * ctx.dt; }
      ctx.bslot = 0;
      for (int i = 0; i < 3; ++i) { u[i] = 0.0; rk[i] = 0.0; }
      t = 0.0; k = 0; cost = 0;
      for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
      cmd[0] = serl_clip(cmd[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
      cmd[1] = serl_clip(cmd[1], -f.ail_clip, f.ail_clip);
      if (f.rudder_jam_on != 0.0) cmd[2] = f.rudder_jam;
    }
    V0 = V0n;
    serl_write_obs(cfg, incr, err, x, u, obs);
#pragma unroll
    for (int i = 0; i < 16; ++i) if (i < S) rd.obs[(kn + N) * S + i] = obs[i];
  }
  VV_NAME(serl_venv_store_ctx_)(v, e, ctx);
  for (int i = 0; i < 3; ++i) {
    S_[(SERL_VF_ERR + i) * np + e] = err[i]; S_[(SERL_VF_LASTU + i) * np + e] = u[i]; S_[(SERL_VF_REF + i) * np + e] = rk[i];
  }
  for (int i = 0; i < 12; ++i) S_[(SERL_VF_XO + i) * np + e] = x[i];
  S_[SERL_VF_V0 * np + e] = V0;
  S_[SERL_VF_T * np + e] = t;
  I[SERL_VI_K * np + e] = k;
  I[SERL_VI_LIVE * np + e] = 1;
  I[SERL_VI_COST * np + e] = cost;
  au.run_return[e] = run_return; au.run_length[e] = run_length; au.cursor[e] = cur;
  VV_NZ_STORE
}

#ifdef SERL_VENV_NOISE
void VV_KNAME(serl_launch_venv_rollout_general_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd,
                                                 const serl_venv_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_KNAME(serl_venv_rollout_general_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, rd, nz);
}

void VV_KNAME(serl_launch_venv_rollout_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd,
                                         const serl_venv_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_KNAME(serl_venv_rollout_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, rd, nz);
}

void VV_KNAME(serl_launch_venv_step_auto_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_noise_desc &nz, int grid,
                                           hipStream_t stream)
{
  hipLaunchKernelGGL(VV_KNAME(serl_venv_step_auto_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, nz);
}

void VV_KNAME(serl_launch_venv_reset_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_KNAME(serl_venv_reset_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, nz);
}
#else
void VV_NAME(serl_launch_venv_rollout_general_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd,
                                                int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_NAME(serl_venv_rollout_general_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, rd);
}

void VV_NAME(serl_launch_venv_rollout_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd, int grid,
                                        hipStream_t stream)
{
  hipLaunchKernelGGL(VV_NAME(serl_venv_rollout_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, rd);
}

void VV_NAME(serl_launch_venv_step_auto_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_NAME(serl_venv_step_auto_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au);
}

void VV_NAME(serl_launch_venv_reset_)(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_NAME(serl_venv_reset_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v);
}

void VV_NAME(serl_launch_venv_step_)(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VV_NAME(serl_venv_step_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v);
}
#endif
#undef VV_SENSOR
#undef VV_ACTION_NOISE_ON
#undef VV_ACTION_NOISE_ROW
#undef VV_NZ_PARAM
#undef VV_NZ_LOCALS
#undef VV_NZ_START
#undef VV_NZ_LOAD
#undef VV_NZ_RESTART
#undef VV_NZ_STORE
#undef VV_KNAME
#undef VV_NAME
#undef VV_PASTE
#undef VV_PASTE2

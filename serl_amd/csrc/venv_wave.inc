// venv_wave.inc -- the step-wise vector env with ONE WAVEFRONT PER ENV (serl_venv_reset_wave / serl_venv_step_wave / serl_venv_step_auto_wave in
// include/serl_amd.h), instantiated once per dynamics code variant (VARIANT) behind rollout_wave.inc, whose LDS staging (citw_stage_<v>), dynamics step
// (citw_step_<v>) and initialize() (citw_reset_<v>) it reuses.  The small-batch path: a lane kernel (venv_variant.inc) flies the 19-state ODE5 evaluation
// serially per lane, so a call lasts one lane env step however few envs there are; here the evaluation's look-ups and states are spread over the 64 lanes.
//
// Per call and env: load the dynamics state from the caller's SoA buffer (rollout_device.h SerlVenvF64 / SerlVenvI32: lane i < 19 takes X[i], the 29 bank
// words go to g_dw, clock and time are wave-uniform), run one reset() or step() with the env glue of rollout_wave.inc (X = true) / venv_variant.inc computed
// wave-uniformly, store the state back in the same layout.  Outputs leave from lane 0.  1 .. CITW_MAX_WAVES wavefronts share a workgroup's LDS copy of the
// tables; the only barrier is the one behind the staging, and the auto-reset kernel's second trip is entered per wavefront.
//
// The same buffer may be handed to the lane kernels at any call.  What CitCtx carries and the wave family does not:
//   IW[0..2]   the table3 S-function's interval cache, which the wave family's citw_table3 does not use.  NOT REPRODUCIBLE: the lane step walks it from
//              RWORK, and its working context never loads RWORK (citation_step_dev.h under CIT_DW_IN_MEMORY: lc.DW[26..28]), so what a lane kernel leaves
//              there depends on how it was compiled.  A reset stores initialize()'s image, a step leaves the words as it finds them; no output of either
//              family has been seen to depend on them, but CitationVecEnv.rollout() does not hand such a state to the lane rollout kernels.
//   IW[3]      0 at initialize(), never written by a step: reset stores 0, step leaves it.
//   CERR       no generated evaluation raises a flag: reset stores 0, step leaves it.
//   CSTOP      the solver stop time of the last major step, which is also the clock t behind it: stored as t.
//   hint[8]    left as they are, reset included: cit_lookup_index_h (citation_leaves.h) verifies whatever its hint holds and falls back to the count.
#define VW_PASTE2(a, b) a##b
#define VW_PASTE(a, b) VW_PASTE2(a, b)
#define VW_NAME(x) VW_PASTE(x, VARIANT)
// SERL_VENV_NOISE: the same text a second time as the kernels of serl_venv_*_wave_noise, as in venv_variant.inc; every lane of the wavefront makes the
// same generator call (serl_rng.h), so the row is wave-uniform.
#ifdef SERL_VENV_NOISE
#define VW_KNAME(x) VW_PASTE(VW_PASTE(x, noise_), VARIANT)
#define VW_NZ_PARAM , serl_venv_noise_desc nz
#define VW_NZ_LOCALS double nzsn[7]; int32_t nzep = 0;
#define VW_NZ_START nzep = nz.episode_count[e]; if (lane == 0) nz.episode_count[e] = nzep + 1;
#define VW_NZ_LOAD nzep = nz.episode_count[e] - 1;
#define VW_NZ_RESTART nzep += 1;
#define VW_NZ_STORE if (lane == 0) nz.episode_count[e] = nzep + 1;
#define VW_SENSOR(j) serl_venvw_sensor_nz(d, nz, e, nzep, j, nzsn)
#else
#define VW_KNAME(x) VW_NAME(x)
#define VW_NZ_PARAM
#define VW_NZ_LOCALS
#define VW_NZ_START
#define VW_NZ_LOAD
#define VW_NZ_RESTART
#define VW_NZ_STORE
#define VW_SENSOR(j) serl_venvw_sensor(d, e, j)
#endif

#ifndef SERL_VENVW_COMMON      // (family_venvw.hip includes this file twice: what follows up to the kernels is shared by both passes)
#define SERL_VENVW_COMMON
// the outputs of an env that does not move in this call (venv_variant.inc serl_venv_write_frozen); fobs: serl_venv_step_auto's final_obs row, or nullptr.
// One lane calls it.
static __device__ __forceinline__ void serl_venvw_write_frozen(const VenvArgs &v, int e, bool step, double *fobs)
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
  if (fobs) serl_write_obs(d.env_config, d.incremental != 0, err, x, u, fobs);
  v.reward[e] = 0.0;
  v.done[e] = 1;
  if (v.x) for (int i = 0; i < 12; ++i) v.x[(size_t)e * 12 + i] = x[i];
  if (v.ref) for (int i = 0; i < 3; ++i) v.ref[(size_t)e * 3 + i] = S[(SERL_VF_REF + i) * np + e];
  if (v.t) v.t[e] = S[SERL_VF_T * np + e];
  if (v.cost) v.cost[e] = I[SERL_VI_COST * np + e];
}

static __device__ __forceinline__ const double *serl_venvw_sensor(const serl_venv_desc &d, int e, int j)
{
  if (!d.sensor_noise) return nullptr;
  const int sr = d.sensor_row ? d.sensor_row[e] : e;
  return sr < 0 ? nullptr : d.sensor_noise + ((size_t)sr * ((size_t)d.max_steps + 1) + (size_t)j) * 7;
}

// the command the model sees: the fault row on top of the env's deflections (venv_variant.inc)
static __device__ __forceinline__ void serl_venvw_cmd(const serl_fault_row &f, const double (&u)[3], double (&cmd)[10])
{
#pragma unroll
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  serl_fault_apply(f, u, cmd);
}

// the dynamics state of env e: state buffer -> the wave family's state (lane i < 19: X[i]; the banks to g_dw[wv]; clock and time wave-uniform)
static __device__ __forceinline__ void VW_NAME(serl_venvw_load_)(const VenvArgs &v, const int e, const int wv, CitwState &s)
{
  const int lane = threadIdx.x & 63;
  const double *S = (const double *)v.d.state;
  const int32_t *I = (const int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  s.xi = S[(SERL_VF_X + (lane < 19 ? lane : 18)) * np + e];
  if (lane < 19) g_xs[wv][lane] = s.xi;
  if (lane < 29) g_dw[wv][lane] = S[(SERL_VF_DW + lane) * np + e];
  s.t = S[SERL_VF_CT * np + e];
  s.tick = (unsigned)I[SERL_VI_TICK * np + e];
  CITW_WAVE_FENCE();
}

// ... and back.  iw0: behind an initialize(), its image of table3's cache (IW[3] and the error word start at 0); a step (nullptr) leaves all five as they are
static __device__ __forceinline__ void VW_NAME(serl_venvw_store_)(const VenvArgs &v, const int e, const int wv, const CitwState &s, const int32_t *iw0)
{
  const int lane = threadIdx.x & 63;
  double *S = (double *)v.d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  if (lane < 19) S[(SERL_VF_X + lane) * np + e] = s.xi;
  if (lane < 29) S[(SERL_VF_DW + lane) * np + e] = g_dw[wv][lane];
  if (lane == 0) {
    S[SERL_VF_CT * np + e] = s.t; S[SERL_VF_CSTOP * np + e] = s.t;
    I[SERL_VI_TICK * np + e] = (int32_t)s.tick;
    if (iw0) {
      for (int i = 0; i < 3; ++i) I[(SERL_VI_IW + i) * np + e] = iw0[i];
      I[(SERL_VI_IW + 3) * np + e] = 0; I[SERL_VI_CERR * np + e] = 0;
    }
  }
}

// initialize() (citation_dev.h cit_reset as the lane kernels call it): the state images, the clock kept running
static __device__ __forceinline__ void VW_NAME(serl_venvw_init_)(const RolloutArgs &a, const int wv, CitwState &s, const uint32_t tick)
{
  VW_NAME(citw_reset_)(wv, s, a);
  if (tick) { s.tick = tick; s.t = (double)tick * a.dyn_dt; }
}

#endif  // SERL_VENVW_COMMON

#ifdef SERL_VENV_NOISE
static __device__ __forceinline__ const double *serl_venvw_sensor_nz(const serl_venv_desc &d, const serl_venv_noise_desc &nz, int e, int32_t ep, int j,
                                                                     double (&buf)[7])
{
  if (!nz.sensor) return serl_venvw_sensor(d, e, j);
  serl_rng_sensor(nz.seed, nz.sensor_bias, nz.sensor_scale, e, ep, j, buf);
  return buf;
}
#endif

#ifndef SERL_VENVW_HELPERS_ONLY      // (family_venvwr.hip takes the helpers above and brings the rollout kernels of venv_wave_rollout.inc)
// reset() of the envs in the mask (serl_venv_reset_kernel_<v>)
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) VW_KNAME(serl_venv_reset_wave_kernel_)(RolloutArgs a, VenvArgs v VW_NZ_PARAM)
{
  VW_NAME(citw_stage_)(a);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * (blockDim.x >> 6) + wv;
  if (e >= v.d.n_envs) return;
  if (v.mask && !v.mask[e]) {
    if (lane == 0) serl_venvw_write_frozen(v, e, false, nullptr);
    return;
  }
  const serl_venv_desc &d = v.d;
  double *S = (double *)d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  const int A = d.action_dim;
  VW_NZ_LOCALS
  VW_NZ_START
  double err[3], u[3] = {0.0, 0.0, 0.0}, x[12], cmd[10];
  for (int i = 0; i < 3; ++i) err[i] = S[(SERL_VF_ERR + i) * np + e];      // self.error is never cleared
  if (d.err0) for (int i = 0; i < 3; ++i) err[i] = i < A ? d.err0[(size_t)e * 3 + i] : 0.0;
  const uint32_t tick = d.tick0 ? (uint32_t)d.tick0[e] : (uint32_t)I[SERL_VI_TICK * np + e];   // initialize() leaves the clock running
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  CitwState s;
  VW_NAME(serl_venvw_init_)(a, wv, s, tick);
  serl_venvw_cmd(f, u, cmd);
  VW_NAME(citw_step_)(wv, s, cmd, x);
  if (const double *sn = VW_SENSOR(0)) {
    serl_sensor_add(x, sn);
  }
  VW_NAME(serl_venvw_store_)(v, e, wv, s, (const int32_t *)(a.dw0 + 29));      // (table3's cache image sits behind the banks)
  if (lane == 0) {
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
}

// step(action) of every env, and -- AUTO, serl_venv_step_auto -- reset() of the env whose episode that step ends, in the same launch.  As in
// serl_venv_step_auto_kernel_<v> there is ONE call site of the step in a two-trip loop; the second trip is entered by the wavefront whose env finished and by
// no other.  Without AUTO (serl_venv_step_kernel_<v>) the loop ends behind the first trip and a finished env freezes.
template <bool AUTO>
static __device__ __forceinline__ void VW_KNAME(serl_venvw_step_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au VW_NZ_PARAM)
{
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * (blockDim.x >> 6) + wv;
  if (e >= v.d.n_envs) return;
  const serl_venv_desc &d = v.d;
  double *S = (double *)d.state;
  int32_t *I = (int32_t *)(S + SERL_VENV_F64 * v.npad);
  const int64_t np = v.npad;
  double *fobs = AUTO ? au.final_obs + (size_t)e * d.state_dim : nullptr;
  if (!I[SERL_VI_LIVE * np + e]) {      // done or never reset: frozen
    if (lane == 0) serl_venvw_write_frozen(v, e, true, fobs);
    return;
  }
  VW_NZ_LOCALS
  VW_NZ_LOAD
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const int cfg = d.env_config, A = d.action_dim;
  const bool incr = d.incremental != 0;
  const double bound = (incr ? 25.0 : 10.0) * deg2rad, low = -bound, high = bound;   // rate bound [rad/s] / deflection bound [rad]
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  double err[3], u[3], x[12], cmd[10], rk[3];
  for (int i = 0; i < 3; ++i) { err[i] = S[(SERL_VF_ERR + i) * np + e]; u[i] = S[(SERL_VF_LASTU + i) * np + e]; }
  const double V0 = S[SERL_VF_V0 * np + e];
  double t = S[SERL_VF_T * np + e];
  int k = I[SERL_VI_K * np + e];
  // scale_action (envs/phlabenv.py:62-73) without clipping; incremental control integrates the rate (:377-380,446-450)
  double scl[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < 3; ++i) {
    if (i >= A) continue;
    if (v.actions_f64) {
      const double ai = ((const double *)v.actions)[(size_t)e * A + i];
      scl[i] = low + 0.5 * (ai + 1.0) * (high - low);
    } else {
      const float sc = 0.5f * (((const float *)v.actions)[(size_t)e * A + i] + 1.0f);
      scl[i] = low + (double)sc * (high - low);
    }
  }
  for (int i = 0; i < 3; ++i) u[i] = incr ? u[i] + scl[i] * dt : scl[i];
  serl_fault_row f = serl_fault_none();
  if (d.faults) f = d.faults[e];
  serl_venvw_cmd(f, u, cmd);
  // the running episode's reference: its row of the pool (the cursor is the caller's memory: kept inside the pool whatever it holds)
  int32_t cur = 0;
  int row = 0;
  const serl_ref_spec *spec = d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
  double run_return = 0.0;
  int32_t run_length = 0;
  if constexpr (AUTO) {
    cur = au.cursor[e];
    row = au.ref_pool ? (int)((uint32_t)cur % (uint32_t)au.pool_rows) : 0;
    if (au.ref_pool) spec = au.ref_pool + (size_t)e * au.pool_rows + row;
    run_return = au.run_return[e]; run_length = au.run_length[e];
  }
  int cost = 0;
  double V0n = V0;
  bool restart = false, live = true, fresh = false;
  CitwState s;
  VW_NAME(serl_venvw_load_)(v, e, wv, s);
#pragma nounroll
  for (int trip = 0; trip < 2; ++trip) {
    VW_NAME(citw_step_)(wv, s, cmd, x);
    if (const double *sn = VW_SENSOR(restart ? 0 : k + 1)) {      // k < max_steps: entry k + 1 <= max_steps exists
      serl_sensor_add(x, sn);
    }
    if (restart) { V0n = x[3]; break; }
    if (spec) serl_ref_generate(spec, t, d.t_max, rk[0], rk[1], rk[2]);      // at the pre-increment t
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
    const bool done = fin || k >= d.max_steps;     // (the tables end: the env freezes or restarts instead of reading past them)
    if (lane == 0) {
      if constexpr (AUTO) serl_write_obs(cfg, incr, err, x, u, fobs);
      v.reward[e] = reward;
      v.done[e] = done ? 1 : 0;
      if (v.x) for (int i = 0; i < 12; ++i) v.x[(size_t)e * 12 + i] = x[i];
      if (v.ref) for (int i = 0; i < 3; ++i) v.ref[(size_t)e * 3 + i] = rk[i];
      if (v.t) v.t[e] = t;
      if (v.cost) v.cost[e] = cost;
    }
    if constexpr (!AUTO) { live = !done; break; }
    const double ret = run_return + reward;
    const int32_t len = run_length + 1;
    if (!done) {
      if (lane == 0) { au.run_return[e] = ret; au.run_length[e] = len; }
      break;
    }
    if (lane == 0) {
      au.ep_return[e] = ret; au.ep_length[e] = len;
      au.run_return[e] = 0.0; au.run_length[e] = 0;
      au.cursor[e] = au.ref_pool ? (row + 1) % au.pool_rows : (int32_t)(((uint32_t)cur + 1u) & 0x7fffffffu);      // (no pool: restarts counted, wrapping to 0)
    }
    // reset() of this env (serl_venv_reset_wave_kernel_ without err0 / tick0): the error stays, the clock keeps counting
    restart = true; fresh = true;
    VW_NZ_RESTART
    VW_NAME(serl_venvw_init_)(a, wv, s, s.tick);
    for (int i = 0; i < 3; ++i) { u[i] = 0.0; rk[i] = 0.0; }
    t = 0.0; k = 0; cost = 0;
    serl_venvw_cmd(f, u, cmd);
  }
  VW_NAME(serl_venvw_store_)(v, e, wv, s, fresh ? (const int32_t *)(a.dw0 + 29) : nullptr);
  if (lane == 0) {
    for (int i = 0; i < 3; ++i) {
      S[(SERL_VF_ERR + i) * np + e] = err[i]; S[(SERL_VF_LASTU + i) * np + e] = u[i]; S[(SERL_VF_REF + i) * np + e] = rk[i];
    }
    for (int i = 0; i < 12; ++i) S[(SERL_VF_XO + i) * np + e] = x[i];
    if constexpr (AUTO) S[SERL_VF_V0 * np + e] = V0n;
    S[SERL_VF_T * np + e] = t;
    I[SERL_VI_K * np + e] = k;
    I[SERL_VI_LIVE * np + e] = live ? 1 : 0;
    I[SERL_VI_COST * np + e] = cost;
    serl_write_obs(cfg, incr, err, x, u, v.obs + (size_t)e * d.state_dim);
  }
  VW_NZ_STORE
}

#ifndef SERL_VENV_NOISE      // (the plain step has no noise instantiation: device noise needs auto-reset)
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) VW_NAME(serl_venv_step_wave_kernel_)(RolloutArgs a, VenvArgs v)
{
  VW_NAME(citw_stage_)(a);
  serl_venv_auto_desc none = {};
  VW_NAME(serl_venvw_step_)<false>(a, v, none);
}

__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) VW_NAME(serl_venv_step_auto_wave_kernel_)(RolloutArgs a, VenvArgs v, serl_venv_auto_desc au)
{
  VW_NAME(citw_stage_)(a);
  VW_NAME(serl_venvw_step_)<true>(a, v, au);
}

void VW_NAME(serl_launch_venv_reset_wave_)(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VW_NAME(serl_venv_reset_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v);
}

void VW_NAME(serl_launch_venv_step_wave_)(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VW_NAME(serl_venv_step_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v);
}

void VW_NAME(serl_launch_venv_step_auto_wave_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VW_NAME(serl_venv_step_auto_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au);
}
#else
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) VW_KNAME(serl_venv_step_auto_wave_kernel_)(RolloutArgs a, VenvArgs v, serl_venv_auto_desc au, serl_venv_noise_desc nz)
{
  VW_NAME(citw_stage_)(a);
  VW_KNAME(serl_venvw_step_)<true>(a, v, au, nz);
}

void VW_KNAME(serl_launch_venv_reset_wave_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VW_KNAME(serl_venv_reset_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, nz);
}

void VW_KNAME(serl_launch_venv_step_auto_wave_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_noise_desc &nz, int grid,
                                                hipStream_t stream)
{
  hipLaunchKernelGGL(VW_KNAME(serl_venv_step_auto_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, nz);
}
#endif
#endif  // SERL_VENVW_HELPERS_ONLY
#undef VW_SENSOR
#undef VW_NZ_PARAM
#undef VW_NZ_LOCALS
#undef VW_NZ_START
#undef VW_NZ_LOAD
#undef VW_NZ_RESTART
#undef VW_NZ_STORE
#undef VW_KNAME
#undef VW_NAME
#undef VW_PASTE
#undef VW_PASTE2

// venv_wave_rollout.inc -- K policy-driven steps of the step-wise vector env with ONE WAVEFRONT PER ENV (serl_venv_rollout_wave / _wave_noise in
// include/serl_amd.h), instantiated once per dynamics code variant (VARIANT) behind rollout_wave.inc and the helpers of venv_wave.inc, and a second time
// under SERL_VENV_NOISE with the in-kernel noise generator.  What it puts together, none of it new arithmetic:
//   staging, step, initialize()   citw_stage_<v> / citw_step_<v> / citw_reset_<v> (rollout_wave.inc)
//   the env's state               serl_venvw_load_<v> / serl_venvw_store_<v> (venv_wave.inc): loaded once, stored once
//   the actor                     the wave-cooperative forward, one hidden row per lane (rollout_device.h): serl_actor_forward for the attitude task's
//                                 7 -> H -> 3 (whole rows up to H = 64, chunked for 72 / 96), serl_actor_forward_wave<true> for every other width
//   the action path, bookkeeping  serl_venv_rollout_general_kernel_<v> (venv_variant.inc), statement for statement
//   the two-trip step             serl_venvw_step_<true> (venv_wave.inc): the second trip is the in-launch restart
// Every scalar is wave-uniform (all 64 lanes hold the same value); the step-major rows leave from lane 0, a frozen env's rows one step per lane.
// ONE call site of citw_step_<v> and ONE of the actor dispatch, the K loop and the trip loop both rolled.  No barrier behind the staging: the wavefronts of
// a workgroup leave at different times (e >= n_envs, frozen envs), so the actor runs with SerlNoSync, and no wavefront waits for another workgroup.
#define VR_PASTE2(a, b) a##b
#define VR_PASTE(a, b) VR_PASTE2(a, b)
#define VR_NAME(x) VR_PASTE(x, VARIANT)
#ifdef SERL_VENV_NOISE
#define VR_KNAME(x) VR_PASTE(VR_PASTE(x, noise_), VARIANT)
#define VR_NZ_PARAM , serl_venv_noise_desc nz
#define VR_NZ_LOCALS double nzsn[7], nzan[3]; int32_t nzep = 0; (void)nzan;
#define VR_NZ_LOAD nzep = nz.episode_count[e] - 1;
#define VR_NZ_RESTART nzep += 1;
#define VR_NZ_STORE if (lane == 0) nz.episode_count[e] = nzep + 1;
#define VR_SENSOR(j) serl_venvw_sensor_nz(d, nz, e, nzep, j, nzsn)
#define VR_ACTION_NOISE_ON (rd.action_noise || nz.action)
#define VR_ACTION_NOISE_ROW serl_venvw_action_nz(rd, nz, kn, e, nzep, k, nzan)
#else
#define VR_KNAME(x) VR_NAME(x)
#define VR_NZ_PARAM
#define VR_NZ_LOCALS
#define VR_NZ_LOAD
#define VR_NZ_RESTART
#define VR_NZ_STORE
#define VR_SENSOR(j) serl_venvw_sensor(d, e, j)
#define VR_ACTION_NOISE_ON rd.action_noise
#define VR_ACTION_NOISE_ROW rd.action_noise + kn * 3
#endif

#ifdef SERL_VENV_NOISE
// the action-noise row of step kn: the caller's table, or, where nz.action is set, clip(sd z, +-clip) drawn for (env e, episode ordinal ep, in-episode step k)
// (venv_variant.inc serl_venv_action_nz; every lane makes the same generator call)
static __device__ __forceinline__ const double *serl_venvw_action_nz(const serl_venv_rollout_desc &rd, const serl_venv_noise_desc &nz, size_t kn, int e,
                                                                     int32_t ep, int k, double (&buf)[3])
{
  if (!nz.action) return rd.action_noise + kn * 3;
  serl_rng_action(nz.seed, nz.action_sd, nz.action_clip, e, ep, k, buf);
  return buf;
}
#endif

__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) VR_KNAME(serl_venv_rollout_wave_kernel_)(RolloutArgs a, VenvArgs v, serl_venv_auto_desc au,
                                                                                                serl_venv_rollout_desc rd VR_NZ_PARAM)
{
  VR_NAME(citw_stage_)(a);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * (blockDim.x >> 6) + wv;
  if (e >= v.d.n_envs) return;
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
  serl_write_obs(cfg, incr, err, x, u, obs);      // the current observation, as serl_venvw_write_frozen rebuilds it
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) if (i < S) rd.obs[(size_t)e * S + i] = obs[i];
  }
  if (!I[SERL_VI_LIVE * np + e]) {      // never reset: frozen in every row, as in the lane kernels (no action: zeros; the transition marks itself terminal)
    const double rf[3] = {S_[(SERL_VF_REF + 0) * np + e], S_[(SERL_VF_REF + 1) * np + e], S_[(SERL_VF_REF + 2) * np + e]};
    const double tf = S_[SERL_VF_T * np + e];
    const int32_t cf = I[SERL_VI_COST * np + e];
#pragma nounroll
    for (int kk = lane; kk < K; kk += 64) {      // (the rows are all alike: one step per lane)
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
  VR_NZ_LOCALS
  VR_NZ_LOAD
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
  // the attitude task without rate control has the forward with whole rows / chunks (7 observations, 3 actions); every other width the generic one
  const bool att = __builtin_amdgcn_readfirstlane((int)(cfg == SERL_ENV_ATTITUDE && !incr)) != 0;
  int32_t cur = au.cursor[e];
  double run_return = au.run_return[e];
  int32_t run_length = au.run_length[e];
  bool fresh = false;      // an initialize() ran inside this segment: its image of table3's cache goes to the state, as behind a wave step that restarted
  CitwState s;
  VR_NAME(serl_venvw_load_)(v, e, wv, s);
#pragma nounroll
  for (int kk = 0; kk < K; ++kk) {
    const size_t kn = (size_t)kk * N + (size_t)e;
    float obsf[16], act[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 16; ++i) obsf[i] = (float)obs[i];
    {
      SerlNoSync none;
      if (att) serl_actor_forward<false>(a.d, w, obsf, act, none);
      else serl_actor_forward_wave<true>(a.d, w, obsf, act, none);
    }
    // ---- the action path of serl_venv_rollout_general_kernel_
    double scl[3] = {0.0, 0.0, 0.0};
    if (VR_ACTION_NOISE_ON) {
      const double *noise = VR_ACTION_NOISE_ROW;
      for (int i = 0; i < 3; ++i) {
        if (i >= A) continue;
        double an = serl_clip((double)act[i] + noise[i], -1.0, 1.0);
        scl[i] = low + 0.5 * (an + 1.0) * (high - low);
        act[i] = (float)an;     // the transition holds the action that was executed (agent.py:93,103)
        if (rd.actions && lane == 0) rd.actions[kn * A + i] = an;
      }
    } else {
      for (int i = 0; i < 3; ++i) {
        if (i >= A) continue;
        const float sc = 0.5f * (act[i] + 1.0f);
        scl[i] = low + (double)sc * (high - low);
        if (rd.actions && lane == 0) rd.actions[kn * A + i] = (double)act[i];
      }
    }
    for (int i = 0; i < 3; ++i) u[i] = incr ? u[i] + scl[i] * dt : scl[i];
    // ---- the step of serl_venvw_step_<true>
    serl_venvw_cmd(f, u, cmd);
    const int row = au.ref_pool ? (int)((uint32_t)cur % (uint32_t)au.pool_rows) : 0;
    const serl_ref_spec *spec = au.ref_pool ? au.ref_pool + (size_t)e * au.pool_rows + row
                              : d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
    double V0n = V0;
    bool restart = false;
#pragma nounroll
    for (int trip = 0; trip < 2; ++trip) {
      VR_NAME(citw_step_)(wv, s, cmd, x);
      if (const double *sn = VR_SENSOR(restart ? 0 : k + 1)) {      // k < max_steps: entry k + 1 <= max_steps exists
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
      const bool done = fin || k >= d.max_steps;     // (the tables end: the env restarts instead of reading past them)
      double nobs[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) nobs[i] = 0.0;
      serl_write_obs(cfg, incr, err, x, u, nobs);      // the terminal-aware next observation: final_obs and the transition row
      if (lane == 0) {
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
      }
      const double ret = run_return + reward;
      const int32_t len = run_length + 1;
      if (!done) { run_return = ret; run_length = len; break; }
      if (lane == 0) {
        if (rd.ep_return) rd.ep_return[kn] = ret;
        if (rd.ep_length) rd.ep_length[kn] = len;
        if (au.ep_return) au.ep_return[e] = ret;      // (the env's own "last finished episode", as a step() at this point would leave it)
        if (au.ep_length) au.ep_length[e] = len;
      }
      run_return = 0.0; run_length = 0;
      cur = au.ref_pool ? (row + 1) % au.pool_rows : (int32_t)(((uint32_t)cur + 1u) & 0x7fffffffu);      // (no pool: restarts counted, wrapping to 0)
      // reset() of this env, as in serl_venvw_step_<true>: the error stays, the clock keeps counting
      restart = true; fresh = true;
      VR_NZ_RESTART
      VR_NAME(serl_venvw_init_)(a, wv, s, s.tick);
      for (int i = 0; i < 3; ++i) { u[i] = 0.0; rk[i] = 0.0; }
      t = 0.0; k = 0; cost = 0;
      serl_venvw_cmd(f, u, cmd);
    }
    V0 = V0n;
    serl_write_obs(cfg, incr, err, x, u, obs);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) if (i < S) rd.obs[(kn + N) * S + i] = obs[i];
    }
  }
  VR_NAME(serl_venvw_store_)(v, e, wv, s, fresh ? (const int32_t *)(a.dw0 + 29) : nullptr);      // (table3's cache image sits behind the banks)
  if (lane == 0) {
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
  }
  VR_NZ_STORE
}

#ifdef SERL_VENV_NOISE
void VR_KNAME(serl_launch_venv_rollout_wave_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd,
                                              const serl_venv_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VR_KNAME(serl_venv_rollout_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, rd, nz);
}
#else
void VR_NAME(serl_launch_venv_rollout_wave_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd,
                                             int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(VR_NAME(serl_venv_rollout_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, v, au, rd);
}
#endif
#undef VR_SENSOR
#undef VR_ACTION_NOISE_ON
#undef VR_ACTION_NOISE_ROW
#undef VR_NZ_PARAM
#undef VR_NZ_LOCALS
#undef VR_NZ_LOAD
#undef VR_NZ_RESTART
#undef VR_NZ_STORE
#undef VR_KNAME
#undef VR_NAME
#undef VR_PASTE
#undef VR_PASTE2

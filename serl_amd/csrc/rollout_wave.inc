// rollout_wave.inc -- wave-cooperative rollout kernels, instantiated once per dynamics code variant (VARIANT).
//
// One WAVEFRONT = one episode (base/core/agent.py:63-138).  Everything that is scalar in the reference -- the
// env bookkeeping of envs/phlabenv.py:430-482, the model glue -- is computed wave-uniformly (all 64 lanes hold
// the same value), and the parts with internal parallelism are spread over the lanes:
//   actor MLP       one hidden row per lane  (rollout_device.h: serl_actor_forward_wave)
//   table look-ups  one table per lane       (citation_wave.h, gen/citation_<variant>_wave.inc)
//   ODE5            one state per lane       (citw_step below)
// A workgroup of 1..4 wavefronts shares one LDS copy of the model tables; wavefronts never synchronise after the
// staging barrier, so episodes of different length do not hold each other up.
#define W_PASTE2(a, b) a##b
#define W_PASTE(a, b) W_PASTE2(a, b)
#define W_NAME(x) W_PASTE(x, VARIANT)
#define W_EVAL W_PASTE(W_PASTE(citw_, VARIANT), _eval)

// One call of the reference's exported step(cmd[10], out[12]) @0x6030: the outputs are the states BEFORE integrating
// (rtY latch), then one Dormand-Prince ode5 macro step (inlined rt_ertODEUpdateContinuousStates @0x9eb8..0xa4f3:
// six model evaluations, the first in major-step mode) and the clock update.
static __device__ __forceinline__ void W_NAME(citw_step_)(const int wv, CitwState &s, const double (&cmd)[10], double (&out)[12])
{
  const int lane = threadIdx.x & 63;
  const int li = lane < 19 ? lane : 18;
  const double h = 0.01, t0 = s.t;
  const double yi = s.xi;
  double stop = 0.0, T = t0;
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = g_xs[wv][i];
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 10; ++i) g_cmd[wv][i] = cmd[i];
  }
  CITW_WAVE_FENCE();      // lane 0 stored, every lane loads (citation_wave.h)
  W_PASTE(W_PASTE(citw_, VARIANT), _step_invariants)(wv, wv);     // what does not change over the six evaluations
#pragma nounroll
  for (int st = 0; st < 6; ++st) {
    const double r = W_EVAL(wv, st, T, s.tick);
    CITW_T0();
    if (st == 0) stop = r;
    // lane i < 19: X_i = y_i + sum_j f_j,i * (B[st][j] * h), accumulated in j order like the reference
    const double xn = citw_ode5_combine(st, g_f[wv], li, yi);
    if (lane < 19) g_xs[wv][lane] = xn;
    CITW_WAVE_FENCE();
    if (st == 5) s.xi = xn;
    T = (st == 4) ? stop : (st == 0 ? citw_ode5_b(0, 0) * h + t0 : h * citw_ode5_a(st) + t0);
    CITW_T(20);
  }
  s.tick += 1;
  s.t = stop;
}

static __device__ __forceinline__ void W_NAME(citw_reset_)(const int wv, CitwState &s, const RolloutArgs &a)
{
  const int lane = threadIdx.x & 63;
  s.xi = a.x0[lane < 19 ? lane : 18];
  s.t = 0.0; s.tick = 0;
  if (lane < 19) g_xs[wv][lane] = s.xi;
  if (lane < 29) g_dw[wv][lane] = a.dw0[lane];
  CITW_WAVE_FENCE();
}

#ifndef SERL_WAVE_STEP_ONLY      // (family_venvw.hip takes the step, initialize() and the staging from here and brings kernels of its own)
// X = false: the attitude task (7 observations, 3 actions) every BASELINE configuration uses.  X = true: observation set, number
// of actions and incremental (rate) control from the descriptor (serl_rollout_desc.env_config / incremental;
// envs/phlabenv.py:84-97,174-176,205-220,377-380) -- a second instantiation, so that the default path stays as it is.
#ifdef SERL_ROLLOUT_NOISE      // (family_wavern.hip: the same text a second time, drawing where nz.sensor / nz.action say so -- rollout_noise.h; wave-uniform)
template <bool X>
static __device__ void W_NAME(serl_wave_episode_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, const int wv, int e)
#else
template <bool X>
static __device__ void W_NAME(serl_wave_episode_)(const RolloutArgs &a, const int wv, int e)
#endif
{
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const int cfg = X ? __builtin_amdgcn_readfirstlane(d.env_config) : 0;
  const bool incr = X && __builtin_amdgcn_readfirstlane(d.incremental) != 0;
  const int A = X ? __builtin_amdgcn_readfirstlane(d.action_dim) : 3, S = X ? __builtin_amdgcn_readfirstlane(d.state_dim) : 7;
  constexpr int NO = X ? 16 : 7;                      // entries of the observation arrays
  const double bound = (incr ? 25.0 : 10.0) * deg2rad, low = -bound, high = bound;   // rate bound [rad/s] / deflection bound [rad]
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  serl_fault_row f = {1.0, __longlong_as_double(0x7ff0000000000000LL), __longlong_as_double(0x7ff0000000000000LL),
                      0.0, 0.0, 0, 0, 0};
  if (d.faults) f = d.faults[e];
  const float *wts = d.weights + (size_t)d.member_of_episode[e] * d.weight_stride;
  const double *ref = d.ref ? d.ref + (size_t)e * d.ref_stride : nullptr;
  const serl_ref_spec *rspec = d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;   // generated instead of read
  const double *snoise = nullptr;     // this episode's row of pre-drawn sensor noise (envs/noise/citation.py:71-82), if any
  if (d.sensor_noise) {
    const int sr = d.sensor_row ? d.sensor_row[e] : e;
    if (sr >= 0) snoise = d.sensor_noise + (size_t)sr * ((size_t)d.max_steps + 1) * 7;
  }
  const double *noise = nullptr;      // this episode's row of pre-drawn action noise (agent.py:90-93), if any
  if (d.action_noise) {
    const int nr = d.noise_row ? d.noise_row[e] : e;
    if (nr >= 0) noise = d.action_noise + (size_t)nr * d.max_steps * 3;
  }
#ifdef SERL_ROLLOUT_NOISE
  const SerlRolloutNoiseKey nzk = serl_rollout_noise_key(d, nz, e);
#endif
  CitwState s;
  double cmd[10], x[12], err[3] = {0, 0, 0}, obs[NO], u[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < NO; ++i) obs[i] = 0.0;
  float act[3] = {0.0f, 0.0f, 0.0f};
  // observation = [error (A), observed states, last_u (A, incremental only)]; static indices per configuration
  auto build_obs = [&](double (&o)[NO]) {
    if constexpr (X) {
      if (cfg == SERL_ENV_SYMMETRIC) {
        o[0] = err[0]; o[1] = x[1];
        if (incr) o[2] = u[0];
      } else if (cfg == SERL_ENV_FULL) {
        o[0] = err[0]; o[1] = err[1]; o[2] = err[2];
#pragma unroll
        for (int i = 0; i < 10; ++i) o[3 + i] = x[i];
        if (incr) { o[13] = u[0]; o[14] = u[1]; o[15] = u[2]; }
      } else {
        o[0] = err[0]; o[1] = err[1]; o[2] = err[2];
        o[3] = x[0]; o[4] = x[1]; o[5] = x[2]; o[6] = x[4];
        if (incr) { o[7] = u[0]; o[8] = u[1]; o[9] = u[2]; }
      }
    } else {
      o[0] = err[0]; o[1] = err[1]; o[2] = err[2];
      o[3] = x[0]; o[4] = x[1]; o[5] = x[2]; o[6] = x[4];
    }
  };
  W_NAME(citw_reset_)(wv, s, a);
  if (d.tick0) { s.tick = (unsigned)d.tick0[e]; s.t = (double)s.tick * 0.01; }   // initialize() leaves the model clock running
#pragma unroll
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  if (d.err0) for (int i = 0; i < 3; ++i) if (i < A) err[i] = d.err0[(size_t)e * 3 + i];
  double V0 = 0.0, t = 0.0, fitness = 0.0;
  int k = -1, cost_steps = 0;      // k == -1: the step env.reset() takes with a zero command (envs/phlabenv.py:409-413)

  const bool prof = a.prof != nullptr && blockIdx.x == 0 && threadIdx.x < 64;
  unsigned long long pc_actor = 0, pc_dyn = 0, pc_env = 0, tc0 = 0, tc1 = 0, tc2 = 0;
  for (;;) {
    if (prof) tc0 = __builtin_readcyclecounter();
    // the reference sample of this step: fetched now, used behind the dynamics (an HBM / L2 round trip off the serial path)
    const int kr = k < 0 ? 0 : k;
    double rk0, rk1, rk2;
    if (rspec) serl_ref_generate(rspec, t, d.t_max, rk0, rk1, rk2);      // at the pre-increment time t_k (envs/phlabenv.py:349,473)
    else { rk0 = ref[(size_t)kr * 3]; rk1 = ref[(size_t)kr * 3 + 1]; rk2 = ref[(size_t)kr * 3 + 2]; }
    if (k >= 0) {
      float obsf[NO];
#pragma unroll
      for (int i = 0; i < NO; ++i) obsf[i] = (float)obs[i];
      if constexpr (X) {
        SerlNoSync none;
        serl_actor_forward_wave<true>(d, wts, obsf, act, none);
      } else {
        serl_actor_forward(d, wts, obsf, act);
      }
      // ---- env step (envs/phlabenv.py:430-482), wave-uniform
      double scl[3] = {0.0, 0.0, 0.0};
#ifdef SERL_ROLLOUT_NOISE
      if (nzk.action) {      // every lane makes the same draw; the first A columns of the entry are used
        double dn[3];
        serl_rollout_noise_action(nz, nzk, k, dn);
        for (int i = 0; i < 3; ++i) {
          if (i >= A) continue;
          double an = serl_clip((double)act[i] + dn[i], -1.0, 1.0);
          scl[i] = low + 0.5 * (an + 1.0) * (high - low);
          act[i] = (float)an;
        }
      } else
#endif
      if (noise) {
        for (int i = 0; i < 3; ++i) {
          if (i >= A) continue;
          double an = serl_clip((double)act[i] + noise[(size_t)k * 3 + i], -1.0, 1.0);
          scl[i] = low + 0.5 * (an + 1.0) * (high - low);
          act[i] = (float)an;     // the transition holds the action that was executed (agent.py:93,103)
        }
      } else {
        for (int i = 0; i < 3; ++i) {
          if (i >= A) continue;
          float sc = 0.5f * (act[i] + 1.0f);
          scl[i] = low + (double)sc * (high - low);
        }
      }
      // incremental control integrates the commanded rate (envs/phlabenv.py:377-380,446-450)
      for (int i = 0; i < 3; ++i) u[i] = incr ? u[i] + scl[i] * dt : scl[i];
    }
    if (prof) { tc1 = __builtin_readcyclecounter(); pc_actor += tc1 - tc0; }
    cmd[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
    cmd[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
    cmd[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
    W_NAME(citw_step_)(wv, s, cmd, x);     // the only call site: one copy of the model in the code object
    if (snoise) {      // what step() returns gets the sensor model on top; the plant state stays clean
      const double *sn = snoise + (size_t)(k + 1) * 7;
      x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
    }
#ifdef SERL_ROLLOUT_NOISE
    if (nzk.sensor) serl_rollout_noise_sensor(nz, nzk, k + 1, x);      // (k == -1: entry 0, initialize()'s step)
#endif
    if (prof) { tc2 = __builtin_readcyclecounter(); pc_dyn += tc2 - tc1; }
    if (k < 0) {
      V0 = x[3];
      build_obs(obs);
      k = 0;
      continue;
    }
    err[0] = rk0 - x[7];
    if (A > 1) { err[1] = rk1 - x[6]; err[2] = rk2 - x[5]; }
    double rsum = 0.0;
    for (int i = 0; i < 3; ++i) if (i < A) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
    double reward = -rsum / (X ? (double)A : 3.0);
    const int cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
    double nobs[NO];
#pragma unroll
    for (int i = 0; i < NO; ++i) nobs[i] = 0.0;
    build_obs(nobs);
    const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
    if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
    t += dt;
    if (d.actions) {
      // the action trace (input of calc_smoothness, base/core/utils.py:82-120) leaves in bursts of 16 env steps:
      // 48 consecutive f64 by 48 lanes instead of three 8-byte stores per step (5x write amplification, PMC WRITE_SIZE)
      if (lane == 0) { g_act[wv][k & 15][0] = u[0]; g_act[wv][k & 15][1] = u[1]; g_act[wv][k & 15][2] = u[2]; }
      CITW_WAVE_FENCE();
      if ((k & 15) == 15 || fin || k + 1 >= d.max_steps) {
        const int n = 3 * ((k & 15) + 1);
        if (lane < n) d.actions[((size_t)e * d.max_steps + (k & ~15)) * 3 + lane] = (&g_act[wv][0][0])[lane];
      }
    }
    if (lane == 0) {
      if (d.states) for (int i = 0; i < 12; ++i) d.states[((size_t)e * d.max_steps + k) * 12 + i] = x[i];
      if (d.rewards) d.rewards[(size_t)e * d.max_steps + k] = reward;
      if (d.transitions) {
        if constexpr (X) {      // (obs S, action A, next_obs S, reward, done, cost)
          float *tr = d.transitions + ((size_t)e * d.max_steps + k) * (2 * S + A + 3);
#pragma unroll
          for (int i = 0; i < NO; ++i) if (i < S) { tr[i] = (float)obs[i]; tr[S + A + i] = (float)nobs[i]; }
          for (int i = 0; i < 3; ++i) if (i < A) tr[S + i] = act[i];
          tr[2 * S + A] = (float)reward; tr[2 * S + A + 1] = fin ? 1.0f : 0.0f; tr[2 * S + A + 2] = cost ? 1.0f : 0.0f;
        } else {
          float *tr = d.transitions + ((size_t)e * d.max_steps + k) * 20;
          for (int i = 0; i < 7; ++i) tr[i] = (float)obs[i];
          for (int i = 0; i < 3; ++i) tr[7 + i] = act[i];
          for (int i = 0; i < 7; ++i) tr[10 + i] = (float)nobs[i];
          tr[17] = (float)reward; tr[18] = fin ? 1.0f : 0.0f; tr[19] = cost ? 1.0f : 0.0f;
        }
      }
    }
    fitness += reward;
    cost_steps += cost;
#pragma unroll
    for (int i = 0; i < NO; ++i) obs[i] = nobs[i];
    ++k;
    if (prof) pc_env += __builtin_readcyclecounter() - tc2;
    if (fin || k >= d.max_steps) {
      if (lane == 0) {
        d.fitness[e] = fitness;
        d.length_steps[e] = fin ? k : -k;     // negative: reference table exhausted before `done`
        d.length_t[e] = t;
        d.cost_steps[e] = cost_steps;
      }
      break;
    }
  }
  if (prof && lane == 0) {
    a.prof[0] = pc_actor; a.prof[1] = pc_dyn; a.prof[2] = pc_env; a.prof[3] = (unsigned long long)k;
#ifdef CITW_PROFILE
    for (int i = 0; i < 28; ++i) a.prof[4 + i] = g_prof[i];
#endif
  }
}

#endif  // SERL_WAVE_STEP_ONLY

// stage the build's tables, the table3 parameters and the look-up descriptors into LDS (whole workgroup)
static __device__ __forceinline__ void W_NAME(citw_stage_)(const RolloutArgs &a)
{
  const int nw = W_PASTE(W_PASTE(citw_, VARIANT), _RO_HI_W) - W_PASTE(W_PASTE(citw_, VARIANT), _RO_LO_W);
  const double *src = a.ro + (W_PASTE(W_PASTE(citw_, VARIANT), _RO_LO_W) - W_PASTE(W_PASTE(citw_, VARIANT), _RO_BASE_W));
  for (int i = threadIdx.x; i < nw; i += blockDim.x) g_ro[i] = src[i];
  for (int i = threadIdx.x; i < 46; i += blockDim.x) g_t3[i] = a.t3[i];
  // interval-index slots: the hinted search (citation_wave.h) re-verifies whatever they hold, starting from interval 0
  for (int i = threadIdx.x; i < (int)(sizeof(g_sidx) / sizeof(int)); i += blockDim.x) (&g_sidx[0][0])[i] = 0;
  for (int i = threadIdx.x; i < W_PASTE(W_PASTE(citw_, VARIANT), _NBP) * CITW_BP_PAD; i += blockDim.x) {
    const CitwBpVec bv = W_PASTE(W_PASTE(citw_, VARIANT), _bpvec)[i / CITW_BP_PAD];
    const int j = i % CITW_BP_PAD;
    g_bp[i / CITW_BP_PAD][j] = j < bv.n ? src[bv.xw + j] : __longlong_as_double(0x7ff0000000000000LL);
  }
  for (int i = threadIdx.x; i < W_PASTE(W_PASTE(citw_, VARIANT), _NK); i += blockDim.x) g_k[i] = W_PASTE(W_PASTE(citw_, VARIANT), _k)[i];
  const int nr = W_PASTE(W_PASTE(citw_, VARIANT), _ROUNDS);
  const CitwSearch *S = &W_PASTE(W_PASTE(citw_, VARIANT), _search)[0][0];
  const CitwLookup *L = &W_PASTE(W_PASTE(citw_, VARIANT), _lookup)[0][0][0];
  for (int i = threadIdx.x; i < nr * 64; i += blockDim.x) (&g_S[0][0])[i] = S[i];
  for (int i = threadIdx.x; i < nr * 128; i += blockDim.x) (&g_L[0][0][0])[i] = L[i];
  __syncthreads();
}

#ifndef SERL_WAVE_STEP_ONLY
#ifdef SERL_ROLLOUT_NOISE      // (family_wavern.hip: the two episode kernels with the generator, nothing else)
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) W_NAME(serl_rollout_wave_noise_kernel_)(RolloutArgs a, const serl_rollout_noise_desc nz)
{
  W_NAME(citw_stage_)(a);
  const int wave = threadIdx.x >> 6;
  const int e = blockIdx.x * (blockDim.x >> 6) + wave;
  if (e >= a.d.n_episodes) return;
  W_NAME(serl_wave_episode_)<false>(a, nz, wave, e);
}

__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) W_NAME(serl_rollout_wavex_noise_kernel_)(RolloutArgs a, const serl_rollout_noise_desc nz)
{
  W_NAME(citw_stage_)(a);
  const int wave = threadIdx.x >> 6;
  const int e = blockIdx.x * (blockDim.x >> 6) + wave;
  if (e >= a.d.n_episodes) return;
  W_NAME(serl_wave_episode_)<true>(a, nz, wave, e);
}

void W_NAME(serl_launch_rollout_wave_noise_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_wave_noise_kernel_), dim3(grid), dim3(a.block), 0, stream, a, nz);
}

void W_NAME(serl_launch_rollout_wavex_noise_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_wavex_noise_kernel_), dim3(grid), dim3(a.block), 0, stream, a, nz);
}
#else
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) W_NAME(serl_rollout_wave_kernel_)(RolloutArgs a)
{
#ifdef CITW_PROFILE
  if (threadIdx.x < 32) g_prof[threadIdx.x] = 0;
#endif
  W_NAME(citw_stage_)(a);
  const int wave = threadIdx.x >> 6;
  const int e = blockIdx.x * (blockDim.x >> 6) + wave;
  if (e >= a.d.n_episodes) return;
  W_NAME(serl_wave_episode_)<false>(a, wave, e);
}

// the env configurations other than the attitude task (symmetric / full observation sets, incremental control)
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) W_NAME(serl_rollout_wavex_kernel_)(RolloutArgs a)
{
  W_NAME(citw_stage_)(a);
  const int wave = threadIdx.x >> 6;
  const int e = blockIdx.x * (blockDim.x >> 6) + wave;
  if (e >= a.d.n_episodes) return;
  W_NAME(serl_wave_episode_)<true>(a, wave, e);
}

// dynamics only: initialize() then T calls of step(cmd[k]) per episode (test / micro-benchmark entry)
__global__ void __launch_bounds__(64 * CITW_MAX_WAVES) W_NAME(serl_dyn_wave_kernel_)(RolloutArgs a, const double *cmds, double *states, int T)
{
  W_NAME(citw_stage_)(a);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int e = blockIdx.x * (blockDim.x >> 6) + wave;
  if (e >= a.d.n_episodes) return;
  CitwState s;
  double cmd[10], x[12];
  W_NAME(citw_reset_)(wave, s, a);
  for (int k = 0; k < T; ++k) {
#pragma unroll
    for (int i = 0; i < 10; ++i) cmd[i] = cmds[((size_t)e * T + k) * 10 + i];
    W_NAME(citw_step_)(wave, s, cmd, x);
    if (lane == 0) for (int i = 0; i < 12; ++i) states[((size_t)e * T + k) * 12 + i] = x[i];
  }
}

void W_NAME(serl_launch_dyn_wave_)(const RolloutArgs &a, const double *cmds, double *states, int T, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_dyn_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a, cmds, states, T);
}

void W_NAME(serl_launch_rollout_wave_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_wave_kernel_), dim3(grid), dim3(a.block), 0, stream, a);
}

void W_NAME(serl_launch_rollout_wavex_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_wavex_kernel_), dim3(grid), dim3(a.block), 0, stream, a);
}
#endif  // SERL_ROLLOUT_NOISE
#endif  // SERL_WAVE_STEP_ONLY
#undef W_NAME
#undef W_EVAL
#undef W_PASTE
#undef W_PASTE2

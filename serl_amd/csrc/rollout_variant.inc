// rollout_variant.inc -- instantiated once per dynamics code variant (VARIANT = nominal, ice, ...).
// Defines  serl_launch_rollout_<VARIANT>(const RolloutArgs&, dim3 grid, dim3 block, hipStream_t).
// (included inside namespace breg / blds)
#define V_PASTE2(a, b) a##b
#define V_PASTE(a, b) V_PASTE2(a, b)
#define V_NAME(x) V_PASTE(x, VARIANT)

#ifndef SERL_VENV_NOISE      // (family_lanenz.hip instantiates venv_variant.inc alone: it needs serl_stage_and_index_<v> only)
// All 64 lanes of a wavefront enter; lanes with `active` own one episode each.  The actor forward is
// wave-cooperative (serl_actor_forward_wave), everything else is per lane.
#ifdef SERL_ROLLOUT_NOISE      // (family_lanern.hip: the same text a second time, drawing where nz.sensor / nz.action say so -- rollout_noise.h)
static __device__ void V_NAME(serl_wave_episodes_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int e, bool active)
#else
static __device__ void V_NAME(serl_wave_episodes_)(const RolloutArgs &a, int e, bool active)
#endif
{
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const double bound = 10.0 * deg2rad, low = -bound, high = bound;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  serl_fault_row f = {1.0, __longlong_as_double(0x7ff0000000000000LL), __longlong_as_double(0x7ff0000000000000LL),
                      0.0, 0.0, 0, 0, 0};
  const float *w = d.weights;
  const double *ref = d.ref;
  const serl_ref_spec *rspec = nullptr;
  const double *noise = nullptr;      // this episode's row of pre-drawn action noise (agent.py:90-93), if any
  const double *snoise = nullptr;     // ... of pre-drawn sensor noise (envs/noise/citation.py:71-82), if any
  CitCtx ctx;
  double cmd[10], x[12], err[3] = {0, 0, 0}, obs[7] = {0, 0, 0, 0, 0, 0, 0};
  double V0 = 0.0, t = 0.0, fitness = 0.0;
  int k = 0, cost_steps = 0;
  unsigned member = 0;
  bool done = !active;
#ifdef SERL_ROLLOUT_NOISE
  SerlRolloutNoiseKey nzk = {false, false, 0, 0};
#endif

  if (active) {
    if (d.faults) f = d.faults[e];
    member = (unsigned)d.member_of_episode[e];
    w = d.weights + (size_t)member * d.weight_stride;
    ref = d.ref ? d.ref + (size_t)e * d.ref_stride : nullptr;
    rspec = d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
    if (d.sensor_noise) {
      const int sr = d.sensor_row ? d.sensor_row[e] : e;
      if (sr >= 0) snoise = d.sensor_noise + (size_t)sr * ((size_t)d.max_steps + 1) * 7;
    }
    if (d.action_noise) {
      const int nr = d.noise_row ? d.noise_row[e] : e;
      if (nr >= 0) noise = d.action_noise + (size_t)nr * d.max_steps * 3;
    }
#ifdef SERL_ROLLOUT_NOISE
    nzk = serl_rollout_noise_key(d, nz, e);
#endif
    cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
    if (d.tick0) { ctx.tick = (uint32_t)d.tick0[e]; ctx.t = (double)ctx.tick * ctx.dt; }   // initialize() leaves the clock running
    ctx.bslot = SERL_FLAVOUR_LDS ? ((threadIdx.x >> 6) * SERL_LDS_B_LANES_PER_WAVE + lane) * CIT_MAX_NB : 0;
    for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
    cmd[0] = serl_clip(cmd[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
    cmd[1] = serl_clip(cmd[1], -f.ail_clip, f.ail_clip);
    if (f.rudder_jam_on != 0.0) cmd[2] = f.rudder_jam;
    V_NAME(cit_step_)(&ctx, cmd, x);
    if (snoise) {
      const double *sn = snoise;
      x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
    }
#ifdef SERL_ROLLOUT_NOISE
    if (nzk.sensor) serl_rollout_noise_sensor(nz, nzk, 0, x);
#endif
    V0 = x[3];
    if (d.err0) for (int i = 0; i < 3; ++i) err[i] = d.err0[(size_t)e * 3 + i];
    obs[0] = err[0]; obs[1] = err[1]; obs[2] = err[2];
    obs[3] = x[0]; obs[4] = x[1]; obs[5] = x[2]; obs[6] = x[4];
  }

  const bool prof = a.prof != nullptr && blockIdx.x == 0 && threadIdx.x < 64;
  unsigned long long pc_actor = 0, pc_dyn = 0, pc_env = 0, pc_steps = 0, tc0 = 0, tc1 = 0, tc2 = 0;
#ifndef SERL_LANE_GENERAL_ACTOR
  const bool lane_actor = __builtin_amdgcn_readfirstlane((int)serl_lane_actor_ok(d)) != 0;
#endif
  for (;;) {
    const unsigned long long live = __ballot(!done);
    if (live == 0ULL) break;
    if (prof) tc0 = __builtin_readcyclecounter();
#ifdef SERL_LANE_GENERAL_ACTOR
    // ---- actor forward (family_laneg.hip, kernel_hint SERL_KERNEL_LANEG): every live lane runs its own actor of ANY shape over its member's row of
    // [members][P] (lane_actor.h serl_actor_forward_lane_general: activations in private memory, no LDS, no regrouped copy); a lane without an
    // episode or with a finished one sits the pass out and loads no weight
    float act[3] = {0.0f, 0.0f, 0.0f};
    if (!done) {
      float obs16[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) obs16[i] = i < 7 ? (float)obs[i] : 0.0f;
#ifdef SERL_LANE_REGROUPED_WEIGHTS      // (family_lanegt.hip / family_lanegtn.hip, serl_rollout_regrouped: the same forward over the regrouped copy [P / 4][members][4])
      serl_actor_forward_lane_general_t(d, a.wt, a.wt_members, member, obs16, act);
#else
      serl_actor_forward_lane_general(d, w, obs16, act);
#endif
    }
#else
    // ---- actor forward for every live episode of this wavefront, one after the other, 64 lanes each
    float obsf[7], act[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 7; ++i) obsf[i] = (float)obs[i];
    const unsigned wlo = (unsigned)(uintptr_t)w, whi = (unsigned)((uintptr_t)w >> 32);
    if (lane_actor) {      // every lane runs its own actor in its own registers (lane_actor.h serl_actor_forward_lane32 / _t: the regrouped weights)
      if (a.wt) serl_actor_forward_lane32_t(d, a.wt, a.wt_members, member, obsf, act);
      else serl_actor_forward_lane32(d, w, obsf, act);
    } else
    for (int l = 0; l < a.lanes; ++l) {
      if (!((live >> l) & 1ULL)) continue;
      float o[7], r[3];
      for (int i = 0; i < 7; ++i) o[i] = serl_bcast(obsf[i], l);
      const uintptr_t wp = (uintptr_t)(unsigned)__builtin_amdgcn_readlane((int)wlo, l) |
                           ((uintptr_t)(unsigned)__builtin_amdgcn_readlane((int)whi, l) << 32);
      serl_actor_forward_wave(d, (const float *)wp, o, r);
      if (lane == l) { act[0] = r[0]; act[1] = r[1]; act[2] = r[2]; }
    }
#endif
    if (prof) { tc1 = __builtin_readcyclecounter(); pc_actor += tc1 - tc0; }
    if (done) continue;
    // ---- env step (envs/phlabenv.py:430-482), per lane
    double u[3];
#ifdef SERL_ROLLOUT_NOISE
    if (nzk.action) {      // the row entry of THIS lane's step k: the lanes of a wavefront are at different steps once episodes have ended
      double dn[3];
      serl_rollout_noise_action(nz, nzk, k, dn);
      for (int i = 0; i < 3; ++i) {
        double an = serl_clip((double)act[i] + dn[i], -1.0, 1.0);
        u[i] = low + 0.5 * (an + 1.0) * (high - low);
        act[i] = (float)an;
      }
    } else
#endif
    if (noise) {
      for (int i = 0; i < 3; ++i) {
        double an = serl_clip((double)act[i] + noise[(size_t)k * 3 + i], -1.0, 1.0);
        u[i] = low + 0.5 * (an + 1.0) * (high - low);
        act[i] = (float)an;     // the transition holds the action that was executed (agent.py:93,103)
      }
    } else {
      for (int i = 0; i < 3; ++i) {
        float s = 0.5f * (act[i] + 1.0f);
        u[i] = low + (double)s * (high - low);
      }
    }
    for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
    cmd[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
    cmd[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
    cmd[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
    V_NAME(cit_step_)(&ctx, cmd, x);
    if (snoise) {
      const double *sn = snoise + (size_t)(k + 1) * 7;
      x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
    }
#ifdef SERL_ROLLOUT_NOISE
    if (nzk.sensor) serl_rollout_noise_sensor(nz, nzk, k + 1, x);
#endif
    if (prof) { tc2 = __builtin_readcyclecounter(); pc_dyn += tc2 - tc1; }
    double rk[3];
    if (rspec) serl_ref_generate(rspec, t, d.t_max, rk[0], rk[1], rk[2]);
    else { rk[0] = ref[(size_t)k * 3]; rk[1] = ref[(size_t)k * 3 + 1]; rk[2] = ref[(size_t)k * 3 + 2]; }
    err[0] = rk[0] - x[7]; err[1] = rk[1] - x[6]; err[2] = rk[2] - x[5];
    double rsum = 0.0;
    for (int i = 0; i < 3; ++i) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
    double reward = -rsum / 3.0;
    int cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
    double nobs[7] = {err[0], err[1], err[2], x[0], x[1], x[2], x[4]};
    bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
    if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
    t += dt;
    if (d.actions) for (int i = 0; i < 3; ++i) d.actions[((size_t)e * d.max_steps + k) * 3 + i] = u[i];
    if (d.states) for (int i = 0; i < 12; ++i) d.states[((size_t)e * d.max_steps + k) * 12 + i] = x[i];
    if (d.rewards) d.rewards[(size_t)e * d.max_steps + k] = reward;
    if (d.transitions) {
      float *tr = d.transitions + ((size_t)e * d.max_steps + k) * 20;
      for (int i = 0; i < 7; ++i) tr[i] = (float)obs[i];
      for (int i = 0; i < 3; ++i) tr[7 + i] = act[i];
      for (int i = 0; i < 7; ++i) tr[10 + i] = (float)nobs[i];
      tr[17] = (float)reward; tr[18] = fin ? 1.0f : 0.0f; tr[19] = cost ? 1.0f : 0.0f;
    }
    fitness += reward;
    cost_steps += cost;
    for (int i = 0; i < 7; ++i) obs[i] = nobs[i];
    ++k;
    if (prof) { pc_env += __builtin_readcyclecounter() - tc2; pc_steps += 1; }
    if (fin || k >= d.max_steps) {
      done = true;
      d.fitness[e] = fitness;
      d.length_steps[e] = fin ? k : -k;     // negative: reference table exhausted before `done`
      d.length_t[e] = t;
      d.cost_steps[e] = ctx.err ? -(1 << 30) : cost_steps;   // negative: internal model error flag (CIT_ERR_*)
    }
  }
  if (prof && lane == 0) { a.prof[0] = pc_actor; a.prof[1] = pc_dyn; a.prof[2] = pc_env; a.prof[3] = pc_steps; }
}

#ifdef SERL_LANE_QUEUE      // (family_lane.hip)
// The same episodes behind a work queue (kernel_hint SERL_KERNEL_LANEQ): lane slot `slot` of the launch starts on episode `slot` (slot < a.q0), and a lane whose
// episode ends takes the next of the episodes [a.q0, a.e_end) from the device counter a.queue -- one atomicAdd per wavefront and pass for all the lanes that ask,
// each adding its rank among them.  A lane that draws an episode beyond e_end (or finds no queue) retires; the wavefront leaves when all its lanes have.  Nothing
// here waits on another wavefront.  The model is evaluated at ONE site: a lane that has just taken an episode flies initialize()'s step (zero command through the
// fault row, sensor-noise row 0, V0) in the call in which its neighbours fly an env step, and the actor pass of such a lane is discarded -- per-lane arithmetic does
// not depend on what the neighbours execute, so every episode is bit-identical to serl_wave_episodes_<v>.
static __device__ void V_NAME(serl_wave_episodes_q_)(const RolloutArgs &a, const int slot)
{
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const double bound = 10.0 * deg2rad, low = -bound, high = bound;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  serl_fault_row f = {1.0, __longlong_as_double(0x7ff0000000000000LL), __longlong_as_double(0x7ff0000000000000LL),
                      0.0, 0.0, 0, 0, 0};
  const float *w = d.weights;
  const double *ref = d.ref;
  const serl_ref_spec *rspec = nullptr;
  const double *noise = nullptr;
  const double *snoise = nullptr;
  CitCtx ctx;
  double cmd[10], x[12], err[3] = {0, 0, 0}, obs[7] = {0, 0, 0, 0, 0, 0, 0};
  double V0 = 0.0, t = 0.0, fitness = 0.0;
  int k = 0, cost_steps = 0, e = slot;
  unsigned member = 0;
  bool retired = slot < 0;      // no episode left for this lane
  bool take = !retired;         // e is an episode this lane has not set up yet
  bool fresh = false;           // set up, initialize()'s step still to fly

  const bool lane_actor = __builtin_amdgcn_readfirstlane((int)serl_lane_actor_ok(d)) != 0;
  for (;;) {
    if (__ballot(!retired) == 0ULL) break;
    if (take) {      // everything serl_wave_episodes_<v> sets up for its episode, for this lane's new e
      f = serl_fault_row{1.0, __longlong_as_double(0x7ff0000000000000LL), __longlong_as_double(0x7ff0000000000000LL), 0.0, 0.0, 0, 0, 0};
      if (d.faults) f = d.faults[e];
      member = (unsigned)d.member_of_episode[e];
      w = d.weights + (size_t)member * d.weight_stride;
      ref = d.ref ? d.ref + (size_t)e * d.ref_stride : nullptr;
      rspec = d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
      snoise = nullptr; noise = nullptr;
      if (d.sensor_noise) {
        const int sr = d.sensor_row ? d.sensor_row[e] : e;
        if (sr >= 0) snoise = d.sensor_noise + (size_t)sr * ((size_t)d.max_steps + 1) * 7;
      }
      if (d.action_noise) {
        const int nr = d.noise_row ? d.noise_row[e] : e;
        if (nr >= 0) noise = d.action_noise + (size_t)nr * d.max_steps * 3;
      }
      cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
      if (d.tick0) { ctx.tick = (uint32_t)d.tick0[e]; ctx.t = (double)ctx.tick * ctx.dt; }
      ctx.bslot = SERL_FLAVOUR_LDS ? ((threadIdx.x >> 6) * SERL_LDS_B_LANES_PER_WAVE + lane) * CIT_MAX_NB : 0;
      for (int i = 0; i < 3; ++i) err[i] = d.err0 ? d.err0[(size_t)e * 3 + i] : 0.0;
      t = 0.0; fitness = 0.0; k = 0; cost_steps = 0;
      take = false; fresh = true;
    }
    // ---- actor forward of every lane in flight (the pass of a fresh lane has no observation yet: skipped, or its result unused)
    const unsigned long long flying = __ballot(!retired && !fresh);
    float obsf[7], act[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 7; ++i) obsf[i] = (float)obs[i];
    const unsigned wlo = (unsigned)(uintptr_t)w, whi = (unsigned)((uintptr_t)w >> 32);
    if (lane_actor) {
      if (a.wt) serl_actor_forward_lane32_t(d, a.wt, a.wt_members, member, obsf, act);
      else serl_actor_forward_lane32(d, w, obsf, act);
    } else
    for (int l = 0; l < a.lanes; ++l) {
      if (!((flying >> l) & 1ULL)) continue;
      float o[7], r[3];
      for (int i = 0; i < 7; ++i) o[i] = serl_bcast(obsf[i], l);
      const uintptr_t wp = (uintptr_t)(unsigned)__builtin_amdgcn_readlane((int)wlo, l) |
                           ((uintptr_t)(unsigned)__builtin_amdgcn_readlane((int)whi, l) << 32);
      serl_actor_forward_wave(d, (const float *)wp, o, r);
      if (lane == l) { act[0] = r[0]; act[1] = r[1]; act[2] = r[2]; }
    }
    bool ask = false;      // this lane's episode ended in this pass
    if (!retired) {
      // ---- the command: initialize()'s zero command for a fresh lane, else the env step's (envs/phlabenv.py:430-482)
      double u[3];
      if (fresh) {
        for (int i = 0; i < 3; ++i) u[i] = 0.0;
      } else if (noise) {
        for (int i = 0; i < 3; ++i) {
          double an = serl_clip((double)act[i] + noise[(size_t)k * 3 + i], -1.0, 1.0);
          u[i] = low + 0.5 * (an + 1.0) * (high - low);
          act[i] = (float)an;
        }
      } else {
        for (int i = 0; i < 3; ++i) {
          float s = 0.5f * (act[i] + 1.0f);
          u[i] = low + (double)s * (high - low);
        }
      }
      for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
      cmd[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
      cmd[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
      cmd[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
      V_NAME(cit_step_)(&ctx, cmd, x);
      if (snoise) {
        const double *sn = snoise + (size_t)(fresh ? 0 : k + 1) * 7;
        x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
      }
      if (fresh) {
        V0 = x[3];
        obs[0] = err[0]; obs[1] = err[1]; obs[2] = err[2];
        obs[3] = x[0]; obs[4] = x[1]; obs[5] = x[2]; obs[6] = x[4];
        fresh = false;
      } else {
        double rk[3];
        if (rspec) serl_ref_generate(rspec, t, d.t_max, rk[0], rk[1], rk[2]);
        else { rk[0] = ref[(size_t)k * 3]; rk[1] = ref[(size_t)k * 3 + 1]; rk[2] = ref[(size_t)k * 3 + 2]; }
        err[0] = rk[0] - x[7]; err[1] = rk[1] - x[6]; err[2] = rk[2] - x[5];
        double rsum = 0.0;
        for (int i = 0; i < 3; ++i) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
        double reward = -rsum / 3.0;
        int cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
        double nobs[7] = {err[0], err[1], err[2], x[0], x[1], x[2], x[4]};
        bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
        if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
        t += dt;
        if (d.actions) for (int i = 0; i < 3; ++i) d.actions[((size_t)e * d.max_steps + k) * 3 + i] = u[i];
        if (d.states) for (int i = 0; i < 12; ++i) d.states[((size_t)e * d.max_steps + k) * 12 + i] = x[i];
        if (d.rewards) d.rewards[(size_t)e * d.max_steps + k] = reward;
        if (d.transitions) {
          float *tr = d.transitions + ((size_t)e * d.max_steps + k) * 20;
          for (int i = 0; i < 7; ++i) tr[i] = (float)obs[i];
          for (int i = 0; i < 3; ++i) tr[7 + i] = act[i];
          for (int i = 0; i < 7; ++i) tr[10 + i] = (float)nobs[i];
          tr[17] = (float)reward; tr[18] = fin ? 1.0f : 0.0f; tr[19] = cost ? 1.0f : 0.0f;
        }
        fitness += reward;
        cost_steps += cost;
        for (int i = 0; i < 7; ++i) obs[i] = nobs[i];
        ++k;
        if (fin || k >= d.max_steps) {
          ask = true;
          d.fitness[e] = fitness;
          d.length_steps[e] = fin ? k : -k;
          d.length_t[e] = t;
          d.cost_steps[e] = ctx.err ? -(1 << 30) : cost_steps;
        }
      }
    }
    // ---- refill: the asking lanes of the wavefront draw consecutive episodes with one atomicAdd
    const unsigned long long asking = __ballot(ask);
    if (asking != 0ULL) {
      int base = a.e_end;      // no queue: every lane is dry after its first episode
      if (a.queue) {
        int got = 0;
        if (lane == __ffsll((long long)asking) - 1) got = atomicAdd(a.queue, __popcll(asking));
        got = __builtin_amdgcn_readlane(got, __ffsll((long long)asking) - 1);
        // (the counter never runs past (e_end - q0) + 64 x wavefronts: a lane asks once more than it is served, then never again)
        base = a.q0 + got;
      }
      if (ask) {
        const long long ne = (long long)base + __popcll(asking & ((1ULL << lane) - 1ULL));
        if (ne >= (long long)a.e_end) retired = true;
        else { e = (int)ne; take = true; }
      }
    }
  }
}
#endif

#endif

// stage the build's tables into LDS (all threads of the workgroup), then keep `lanes` lanes per wavefront
static __device__ __forceinline__ int V_NAME(serl_stage_and_index_)(const RolloutArgs &a)
{
  const int nw = CIT_RO_HI_W - CIT_RO_LO_W;
  const double *src = a.ro + (CIT_RO_LO_W - (int)(RO_BASE_W));
  for (int i = threadIdx.x; i < nw; i += blockDim.x) g_ro[i] = src[i];
  __syncthreads();
#ifdef CIT_SLOPE_DESC      // the x-direction quotients of the tables' intervals (gen/citation_<v>_lane.inc, citation_leaves.h cit_lookup2d_at_s): the interpolation's own operations
  for (int t = 0; t < CIT_SLOPE_TABLES; ++t) {
    const int kind = CIT_SLOPE_DESC[t][0], zw = CIT_SLOPE_DESC[t][1], nr = CIT_SLOPE_DESC[t][2], nc = CIT_SLOPE_DESC[t][3], xw = CIT_SLOPE_DESC[t][4], off = CIT_SLOPE_DESC[t][5];
    const double *z = &g_ro[zw], *x = &g_ro[xw];
    const int per = nr - 1, total = kind == 2 ? per * nc : per;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int ix = i % per, iy = i / per;
      double q = z[ix + 1 + nr * iy] - z[ix + nr * iy];
      q = q / (x[ix + 1] - x[ix]);
      g_sl[off + i] = q;
    }
  }
  __syncthreads();
#endif
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = (blockIdx.x * (blockDim.x >> 6) + wave) * a.lanes + lane;
  return (lane >= a.lanes || e >= a.d.n_episodes) ? -1 : e;
}

#ifndef SERL_VENV_NOISE
// One episode kernel and its launcher per unit, the same two bodies under the unit's name: serl_rollout_<stem>kernel_<v> / serl_launch_rollout_<stem><v>, with the
// generator's descriptor behind the arguments in the noise units
#ifdef SERL_ROLLOUT_NOISE
#define V_NZ_PARAM , const serl_rollout_noise_desc nz
#define V_NZ_REF , const serl_rollout_noise_desc &nz
#define V_NZ_ARG , nz
#else
#define V_NZ_PARAM
#define V_NZ_REF
#define V_NZ_ARG
#endif
#define V_EPISODE_KERNEL(stem)                                                                                                                   \
  __global__ void __launch_bounds__(SERL_BLOCK) V_NAME(V_PASTE(V_PASTE(serl_rollout_, stem), kernel_))(RolloutArgs a V_NZ_PARAM)                  \
  {                                                                                                                                              \
    const int e = V_NAME(serl_stage_and_index_)(a);                                                                                              \
    V_NAME(serl_wave_episodes_)(a V_NZ_ARG, e < 0 ? 0 : e, e >= 0);                                                                              \
  }                                                                                                                                              \
  void V_NAME(V_PASTE(serl_launch_rollout_, stem))(const RolloutArgs &a V_NZ_REF, int grid, hipStream_t stream)                                   \
  {                                                                                                                                              \
    hipLaunchKernelGGL(V_NAME(V_PASTE(V_PASTE(serl_rollout_, stem), kernel_)), dim3(grid), dim3(a.block), 0, stream, a V_NZ_ARG);                 \
  }
#if defined(SERL_LANE_GENERAL_ACTOR) && defined(SERL_LANE_REGROUPED_WEIGHTS) && defined(SERL_ROLLOUT_NOISE)      // (family_lanegtn.hip: the general lane actor over the regrouped copy of the weights, with the generator, nothing else)
V_EPISODE_KERNEL(lanegt_noise_)
#elif defined(SERL_LANE_GENERAL_ACTOR) && defined(SERL_LANE_REGROUPED_WEIGHTS)      // (family_lanegt.hip: the same, plain)
V_EPISODE_KERNEL(lanegt_)
#elif defined(SERL_LANE_GENERAL_ACTOR) && defined(SERL_ROLLOUT_NOISE)      // (family_lanegn.hip: the episode kernel around the general lane actor with the generator, nothing else)
V_EPISODE_KERNEL(laneg_noise_)
#elif defined(SERL_LANE_GENERAL_ACTOR)      // (family_laneg.hip: the same, plain)
V_EPISODE_KERNEL(laneg_)
#elif defined(SERL_ROLLOUT_NOISE)      // (family_lanern.hip: the episode kernel with the generator, nothing else)
V_EPISODE_KERNEL(noise_)
#else
V_EPISODE_KERNEL()

// dynamics only: initialize() then T calls of step(cmd[k]) per episode (test / micro-benchmark entry)
__global__ void __launch_bounds__(SERL_BLOCK) V_NAME(serl_dyn_kernel_)(RolloutArgs a, const double *cmds, double *states, int T)
{
  const int e = V_NAME(serl_stage_and_index_)(a);
  if (e < 0) return;
  CitCtx ctx;
  double cmd[10], x[12];
  cit_reset(&ctx, a.ro, a.t3, a.x0, a.dw0, a.dyn_dt);
  ctx.bslot = SERL_FLAVOUR_LDS ? ((threadIdx.x >> 6) * SERL_LDS_B_LANES_PER_WAVE + (threadIdx.x & 63)) * CIT_MAX_NB : 0;
  for (int k = 0; k < T; ++k) {
    for (int i = 0; i < 10; ++i) cmd[i] = cmds[((size_t)e * T + k) * 10 + i];
    V_NAME(cit_step_)(&ctx, cmd, x);
    for (int i = 0; i < 12; ++i) states[((size_t)e * T + k) * 12 + i] = x[i];
  }
}

void V_NAME(serl_launch_dyn_)(const RolloutArgs &a, const double *cmds, double *states, int T, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(V_NAME(serl_dyn_kernel_), dim3(grid), dim3(a.block), 0, stream, a, cmds, states, T);
}

#ifdef SERL_LANE_QUEUE
// the lane slots [0, a.q0) of the launch start on the episode of their own number, the episodes [a.q0, a.e_end) wait behind a.queue
__global__ void __launch_bounds__(SERL_BLOCK) V_NAME(serl_rollout_laneq_kernel_)(RolloutArgs a)
{
  const int e = V_NAME(serl_stage_and_index_)(a);
  V_NAME(serl_wave_episodes_q_)(a, e < a.q0 ? e : -1);
}

void V_NAME(serl_launch_rollout_laneq_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(V_NAME(serl_rollout_laneq_kernel_), dim3(grid), dim3(a.block), 0, stream, a);
}
#endif
#endif  // SERL_ROLLOUT_NOISE
#undef V_EPISODE_KERNEL
#undef V_NZ_PARAM
#undef V_NZ_REF
#undef V_NZ_ARG
#endif
#undef V_NAME
#undef V_PASTE
#undef V_PASTE2

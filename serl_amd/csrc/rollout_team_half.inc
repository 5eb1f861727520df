// rollout_team_half.inc -- TWO or FOUR episodes per team (included by rollout_team.inc when CITW_GROUP_LANES is 32 or 16).
//
// The team kernels run one episode on eight wavefronts of a CU (seven integrate, one runs the actor) -- the fastest way
// through an episode, but only while every episode can have a CU of its own.  Between CUs and 4 x CUs episodes the
// one-wavefront-per-episode kernel (rollout_wave.inc) took over at 2.6 x the time per env step.  Here the lanes of the
// team's wavefronts carry two episodes (lanes 0-31 / 32-63), like rollout_half.inc does for the one-wavefront kernel: the
// generated team evaluation is compiled once more with CITW_GROUP_LANES = 32, so that the row macros of its LDS
// blackboards (CITW_TROW / CITW_MROW / CITW_XOFF, citation_wave.h) select the lane group's rows and every state-derived
// value is a per-lane quantity; barriers and hand-over flags are shared (the episodes of a team advance in lock step, the
// flags count the TEAM's env steps).  Results are bit-identical to the other kernels.
//
// With CITW_GROUP_LANES = 16 four episodes share the team (kernels serl_rollout_kernel_team4_<variant>): the look-up phases
// take up to four passes of 16 lanes, the 19 states two, the actor lanes own two hidden rows each (serl_actor_forward_quarter32)
// -- the lane-parallel phases get longer, the scalar glue (most of the step) is still paid once for all four.
//
// WORK QUEUE (round 3).  Episodes have different lengths -- an untrained actor leaves the flight envelope within seconds
// (envs/phlabenv.py:391-399), a trained one flies the whole t_max -- and a lane group whose episode is over used to idle,
// masked, until the longest episode of its team was done; launches of more than 4 x CUs episodes ran as rounds that each
// waited for their longest episode.  Now a launch starts at most one team per CU; the episodes that do not get a lane group at
// the start wait in a queue (a device counter, RolloutArgs.queue / q0), and a lane group that finishes its episode takes the
// next one: it resets its rows of the blackboards and its per-lane env state, the actor wavefront switches to the new member's
// weights (g_qe), everything else of the team carries on.  A refill costs the group ONE idle env step (the request is made
// by wave 0 and read by every wavefront behind that step's barriers).  Every episode still sees exactly its own inputs:
// results are bit-identical to one-episode-per-team runs (tests/test_gpu_rollout.py).
//
// ACTORS THAT DO NOT HAVE ONE HIDDEN ROW PER LANE (hidden != 32: SERL10's 72, the TD3 actor's 96): the actor wavefront runs the
// episodes' forward passes one after the other with the streaming forward of the one-episode kernels
// (serl_actor_forward), paying the step's barriers in proportion -- two passes of H = 72 take longer than the team's step (measured:
// 40.6 us per env step for the pair).  The kernels for these shapes (family_team2s.hip, SERL_ACTOR_WAVES = 2) therefore
// run a team of SIX wavefronts (gen/citation_<v>_team6.inc) and TWO actor wavefronts, one per episode: eight wavefronts as before,
// the two forward passes side by side.

#ifndef SERL_TEAMG_WG
#define SERL_TEAMG_WG ((int)blockIdx.x)      // which workgroup of the launch this is (rollout_team4_mixed.hip hands out tickets instead)
#endif
#ifndef SERL_TEAMG_PASS_CACHE
#define SERL_TEAMG_PASS_CACHE 1      // the lane-group teams keep the interval-dependent half of their look-up passes in registers (citation_wave.h CitwPassCache; round 5)
#endif
// The actor wavefront: action j of every episode = actor(observation j), computed while the team integrates env step j - 1.
static __device__ __forceinline__ void W_NAME(serl_teamg_actor_wave_)(const RolloutArgs &a)
{
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63, grp = lane / CITW_GROUP_LANES, gl = lane % CITW_GROUP_LANES;
  // one hidden row (two at 16 lanes) per lane: hidden == 32, the only shape serl_capi.hip launches the one-actor-wavefront units with (serl_use_teamg; the streamed
  // shapes run family_team2s.hip, SERL_ACTOR_WAVES = 2, and only those).  A compile-time fact: the other forward pass -- 15.8 KB of the four-per-team kernel's
  // 82.5 KB, in the middle of the actor wavefront's loop -- is not compiled into a kernel that never runs it (the 64 KB instruction cache is shared by two CUs)
#ifdef SERL_TEAMG_ROWS32_RUNTIME      // (A/B builds: the round-5 code, both forward passes in every kernel)
  const bool rows32 = __builtin_amdgcn_readfirstlane(d.hidden) == 32;
#else
  constexpr bool rows32 = SERL_ACTOR_WAVES == 1;
#endif
  const int aw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) - W_TEAM_WAVES;      // which actor wavefront (SERL_ACTOR_WAVES > 1)
  if (!rows32) __builtin_amdgcn_s_setprio(1);     // (a streaming actor needs most of a step: it wins the issue arbitration on its SIMD)
  for (unsigned j = 0;; ++j) {
    unsigned f;
    while ((f = __hip_atomic_load(&g_oflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != SERL_OBS_DONE && (int)(f - (j + 1u)) < 0)
      __builtin_amdgcn_s_sleep(2);
    if (f == SERL_OBS_DONE) break;
    SerlBarrierCredit credit{0, SERL_TEAM_BARRIERS};
#if CITW_JITTER
    credit.salt = j;
#endif
    if (rows32) {
      const int e = g_qe[grp];                                                   // this lane group's episode (changes when the group refills)
      const float *wts = d.weights + (size_t)d.member_of_episode[e] * d.weight_stride;
      float obsf[7], act[3];
#pragma unroll
      for (int i = 0; i < 7; ++i) obsf[i] = g_obsf[grp][i];
#if CITW_GROUP_LANES == 32
      serl_actor_forward_half32(d, wts, g_hx[grp], obsf, act, credit);
#else
      serl_actor_forward_quarter32(d, wts, g_hx[grp], obsf, act, credit);
#endif
      if (gl == 0) { g_actout[grp][0] = act[0]; g_actout[grp][1] = act[1]; g_actout[grp][2] = act[2]; }
    } else {
      // one episode at a time, all 64 lanes on its rows; with several actor wavefronts each takes its share of the episodes
      constexpr int PER = (CITW_GROUPS + SERL_ACTOR_WAVES - 1) / SERL_ACTOR_WAVES;
#pragma unroll 1
      for (int gi = aw * PER; gi < (aw + 1) * PER && gi < CITW_GROUPS; ++gi) {
        const int e = __builtin_amdgcn_readfirstlane(g_qe[gi]);
        const float *wts = d.weights + (size_t)d.member_of_episode[e] * d.weight_stride;
        float obsf[7], act[3];
#pragma unroll
        for (int i = 0; i < 7; ++i) obsf[i] = g_obsf[gi][i];
        SerlBarrierCreditPart part{credit, SERL_TEAM_BARRIERS * (gi - aw * PER) / PER, SERL_TEAM_BARRIERS * (gi - aw * PER + 1) / PER};
        serl_actor_forward<SERL_ACTOR_LDS_BCAST != 0, false>(d, wts, obsf, act, part, g_hrow[aw]);
        if (lane == 0) { g_actout[gi][0] = act[0]; g_actout[gi][1] = act[1]; g_actout[gi][2] = act[2]; }
      }
    }
    // (LDS operations of a wavefront complete in order: every group's action is in place before the flag)
    CITW_JIT(0xa00u, j);
    if (lane == 0) __hip_atomic_store(SERL_ACTOR_WAVES > 1 ? &g_aflagw[aw] : &g_aflag, j + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    credit(0, 1);                                                // the rest of this step's barriers
  }
}

// The team wavefronts: the episode loop of rollout_team.inc with per-lane (per-episode) state and the work queue.
static __device__ __forceinline__ void W_NAME(serl_teamg_episodes_)(const RolloutArgs &a)
{
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63, grp = lane / CITW_GROUP_LANES, gl = lane % CITW_GROUP_LANES;
  const int wv = grp;                                    // = CITW_TROW: this lane's row of the blackboards
  const bool out_wave = threadIdx.x < 64;                // wave 0 writes results
  const int slot = a.e0 + SERL_TEAMG_WG * CITW_GROUPS + grp;
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0, rad2deg = 180.0 / PI;
  const double bound = 10.0 * deg2rad, low = -bound, high = bound;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double scaler[3] = {6.0 / PI * 1.0, 6.0 / PI * 1.0, 6.0 / PI * 4.0};
  const double dt = 0.01;
  const double INF = __longlong_as_double(0x7ff0000000000000LL);
  // ---- the episode this lane group carries (per-lane values: the lane groups carry different episodes)
  int e = 0;
  serl_fault_row f = {1.0, INF, INF, 0.0, 0.0, 0, 0, 0};
  const double *ref = nullptr, *snoise = nullptr, *noise = nullptr;
  const serl_ref_spec *rspec = nullptr;
  CitwState s;
  double cmd[10], x[12], err[3] = {0, 0, 0}, obs[7] = {0, 0, 0, 0, 0, 0, 0}, u[3] = {0, 0, 0};
  float act[3] = {0.0f, 0.0f, 0.0f};
  double V0 = 0.0, t = 0.0, fitness = 0.0;
  int k = -1, cost_steps = 0;      // k == -1: the step env.reset() takes with a zero command (envs/phlabenv.py:409-413)
  // (re)start this lane group on episode `ep`: inputs of the episode, reset of the group's blackboard rows and env state
  auto start_episode = [&](const int ep) {
    e = ep;
    f = serl_fault_row{1.0, INF, INF, 0.0, 0.0, 0, 0, 0};
    if (d.faults) f = d.faults[e];
    ref = d.ref ? d.ref + (size_t)e * d.ref_stride : nullptr;
    rspec = d.ref_spec ? d.ref_spec + (size_t)e * d.ref_spec_stride : nullptr;
    snoise = nullptr;
    if (d.sensor_noise) {
      const int sr = d.sensor_row ? d.sensor_row[e] : e;
      if (sr >= 0) snoise = d.sensor_noise + (size_t)sr * ((size_t)d.max_steps + 1) * 7;
    }
    noise = nullptr;
    if (d.action_noise) {
      const int nr = d.noise_row ? d.noise_row[e] : e;
      if (nr >= 0) noise = d.action_noise + (size_t)nr * d.max_steps * 3;
    }
    W_NAME(citw_team_reset_)(wv, s, a);
    if (d.tick0) { s.tick = (unsigned)d.tick0[e]; s.t = (double)s.tick * 0.01; }   // initialize() leaves the model clock running
#pragma unroll
    for (int i = 0; i < 3; ++i) { err[i] = d.err0 ? d.err0[(size_t)e * 3 + i] : 0.0; u[i] = 0.0; }
    V0 = 0.0; t = 0.0; fitness = 0.0; k = -1; cost_steps = 0;
  };
  // this wavefront's search / table pass of round 1 with its interval-dependent half kept across evaluations (citation_wave.h CitwPassCache)
  CitwPassCache pass_cache;
  pass_cache.s_valid = false; pass_cache.t_valid = false; pass_cache.epoch = 0u;
  const bool have = slot < a.e_end;
  start_episode(have ? slot : a.e_end - 1);              // (a lane group without an episode reads a valid episode's inputs and writes nothing)
#pragma unroll
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  bool done = !have;                                     // no live episode in this lane group
  bool dry = !have;                                      // ... and none to come: the queue is exhausted (or was never needed)
  int kk = -1;                                           // the TEAM's env-step count (wave-uniform): sequence number of the actor hand-over

  for (;;) {
    const int kr = k < 0 ? 0 : (k < d.max_steps ? k : d.max_steps - 1);      // (a lane group that waits, done, for the others keeps counting: the row stays inside its table)
    double rk0, rk1, rk2;
    if (rspec) serl_ref_generate(rspec, t, d.t_max, rk0, rk1, rk2);
    else { rk0 = ref[(size_t)kr * 3]; rk1 = ref[(size_t)kr * 3 + 1]; rk2 = ref[(size_t)kr * 3 + 2]; }
    // what step() returns: the states BEFORE it integrates (every wavefront reads the team's LDS copy of its episode)
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = g_xs[wv][i];
    if (snoise) {
      const double *sn = snoise + (size_t)(k + 1) * 7;
      x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
    }
    // ---- the actions of this step: the actor wavefront computed them while the previous step was integrated
    if (kk >= 0) {
#if SERL_ACTOR_WAVES > 1
#pragma unroll
      for (int q = 0; q < SERL_ACTOR_WAVES; ++q)
        while ((int)(__hip_atomic_load(&g_aflagw[q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - (unsigned)(kk + 1)) < 0) __builtin_amdgcn_s_sleep(1);
#else
      while ((int)(__hip_atomic_load(&g_aflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - (unsigned)(kk + 1)) < 0) __builtin_amdgcn_s_sleep(1);
#endif
    }
    CITW_JIT(0xa10u, (unsigned)kk);
    bool finished = false;                               // this lane group's episode ends in this step
    if (k >= 0) {       // (per lane group: a group that has just taken a new episode is at its reset step, k == -1)
      act[0] = g_actout[wv][0]; act[1] = g_actout[wv][1]; act[2] = g_actout[wv][2];
      if (noise) {
        for (int i = 0; i < 3; ++i) {
          double an = serl_clip((double)act[i] + noise[(size_t)k * 3 + i], -1.0, 1.0);
          u[i] = low + 0.5 * (an + 1.0) * (high - low);
          act[i] = (float)an;     // the transition holds the action that was executed (agent.py:93,103)
        }
      } else {
        for (int i = 0; i < 3; ++i) {
          float sc = 0.5f * (act[i] + 1.0f);
          u[i] = low + (double)sc * (high - low);
        }
      }
      err[0] = rk0 - x[7]; err[1] = rk1 - x[6]; err[2] = rk2 - x[5];
      double rsum = 0.0;
      for (int i = 0; i < 3; ++i) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
      double reward = -rsum / 3.0;
      const int cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
      const double nobs[7] = {err[0], err[1], err[2], x[0], x[1], x[2], x[4]};
      const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
      if (fin) reward += -1.0 / dt * (d.t_max - t) * 2.0;
      t += dt;
      const bool last = fin || k + 1 >= d.max_steps;
      if (!done) {
        if (d.actions) {
          if (gl == 0) { g_act[wv][k & 15][0] = u[0]; g_act[wv][k & 15][1] = u[1]; g_act[wv][k & 15][2] = u[2]; }
          CITW_WAVE_FENCE();
          if (((k & 15) == 15 || last) && out_wave) {
            const int n = 3 * ((k & 15) + 1);
            double *dst = d.actions + ((size_t)e * d.max_steps + (k & ~15)) * 3;
            for (int i = gl; i < n; i += CITW_GROUP_LANES) dst[i] = (&g_act[wv][0][0])[i];
          }
        }
        if (gl == 0 && out_wave) {
          if (d.states) for (int i = 0; i < 12; ++i) d.states[((size_t)e * d.max_steps + k) * 12 + i] = x[i];
          if (d.rewards) d.rewards[(size_t)e * d.max_steps + k] = reward;
          if (d.transitions) {
            float *tr = d.transitions + ((size_t)e * d.max_steps + k) * 20;
            for (int i = 0; i < 7; ++i) tr[i] = (float)obs[i];
            for (int i = 0; i < 3; ++i) tr[7 + i] = act[i];
            for (int i = 0; i < 7; ++i) tr[10 + i] = (float)nobs[i];
            tr[17] = (float)reward; tr[18] = fin ? 1.0f : 0.0f; tr[19] = cost ? 1.0f : 0.0f;
          }
        }
        fitness += reward;
        cost_steps += cost;
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) obs[i] = nobs[i];
      if (!done && last) {
        if (gl == 0 && out_wave) {
          d.fitness[e] = fitness;
          d.length_steps[e] = fin ? k + 1 : -(k + 1);     // negative: reference table exhausted before `done`
          d.length_t[e] = t;
          d.cost_steps[e] = cost_steps;
        }
        done = true;
        finished = true;
      }
    } else {
      V0 = x[3];
      obs[0] = err[0]; obs[1] = err[1]; obs[2] = err[2];
      obs[3] = x[0]; obs[4] = x[1]; obs[5] = x[2]; obs[6] = x[4];
    }
    // ---- work queue: a lane group whose episode ended asks for the next one (wave 0; every wavefront reads the answer behind
    // this step's barriers).  Without a queue (a.queue == nullptr) a finished group is simply done.
    const bool ask = finished && !dry && a.queue != nullptr;
    if (finished && a.queue == nullptr) dry = true;
    if (ask && out_wave && gl == 0) g_qnext[grp] = a.q0 + atomicAdd(a.queue, 1);
    if (__builtin_amdgcn_ballot_w64(!done || ask) == 0ull) {     // (every team wavefront holds the same per-lane state: same decision)
      if (lane == 0 && out_wave) __hip_atomic_store(&g_oflag, SERL_OBS_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      break;
    }
    // ---- observations of the NEXT env step -> the actor wavefront, which works on them while this step is integrated
    CITW_JIT(0xa20u, (unsigned)(kk + 1));
    if (out_wave) {
      if (gl == 0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) g_obsf[wv][i] = (float)obs[i];
        g_qe[grp] = e;
      }
      if (lane == 0) __hip_atomic_store(&g_oflag, (unsigned)(kk + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    cmd[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
    cmd[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
    cmd[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
#if defined(SERL_DEV_ROLE_MAP) && SERL_DEV_ROLE_MAP && !CITW_JITTER
    // development builds (tools/sweep_roles.py): roles <-> wavefronts from SERL_JITTER_SITES, a nibble per hardware wavefront (all ones: the compiled map)
    W_NAME(citw_team_integrate_)(wv, s, cmd, (unsigned)(kk + 1), done,
                                 a.jitter_sites == ~0u ? -1 : (int)((a.jitter_sites >> (4 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)))) & 15u));
#else
    W_NAME(citw_team_integrate_)(wv, s, cmd, (unsigned)(kk + 1), done, -1, false, false, citw_no_kregs, false, citw_no_spec_cache, SERL_TEAMG_PASS_CACHE != 0, pass_cache);
#endif
    ++k; ++kk;
    CITW_JIT(0xa40u, (unsigned)kk);
    if (ask) {       // the step's barriers lie between wave 0's store and this load
      const int nx = g_qnext[grp];
      if (nx < a.e_end) { start_episode(nx); done = false; }
      else dry = true;
    }
  }
#ifdef CITW_PROFILE      // (profiling builds: wave 0's phase cycles of workgroup 0, like the one-episode team kernel)
  if (a.prof != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
    a.prof[0] = 0; a.prof[1] = 0; a.prof[2] = 0; a.prof[3] = (unsigned long long)(kk + 1);
    for (int i = 0; i < 27; ++i) a.prof[4 + i] = g_prof[i];
  }
#endif
}

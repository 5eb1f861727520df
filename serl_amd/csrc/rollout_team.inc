// rollout_team.inc -- a team of wavefronts per episode, instantiated once per dynamics code variant (VARIANT).
//
// Same episode loop as rollout_wave.inc, but the workgroup is ONE episode run by a TEAM of K = 7 wavefronts plus an actor
// wavefront -- eight in all, two per SIMD of the CU.  The model evaluation is split between the team
// (gen/citation_<variant>_team.inc: wave 0 = look-up path, the others = shares of the remaining glue, two workgroup barriers
// per evaluation); env bookkeeping and ODE5 combination are computed by all of them redundantly from the same LDS state, so
// they stay in lock step without further synchronisation (identical values written to identical LDS addresses); the actor
// forward of the NEXT env step runs beside them on the eighth wavefront.  Used when there are fewer episodes than CUs: a
// lone wavefront pays a 4-cycle issue slot per instruction (7.6 cycles per dependent f64 operation), so more SIMDs -- and a
// second wavefront per SIMD to issue into the first one's latency gaps -- are the only way to go faster.
#define W_PASTE2(a, b) a##b
#define W_PASTE(a, b) W_PASTE2(a, b)
#define W_NAME(x) W_PASTE(x, VARIANT)
#define W_TEAM_EVAL W_PASTE(W_PASTE(citw_, VARIANT), _team_eval)
#define W_TEAM_WAVES W_PASTE(W_PASTE(citw_, VARIANT), _team_WAVES)

// ---- hand-over between the team and its ACTOR WAVEFRONT (wave index W_TEAM_WAVES of the workgroup) ----------------------
// The model's step() latches its outputs BEFORE it integrates (the reference's one-step transport delay, SURVEY 2.1), so
// the observation of env step k+1 -- tracking error and rates of the state at the TOP of step k -- exists before step k's
// six model evaluations start, and so does everything the actor needs for action k+1.  An extra wavefront therefore runs
// the actor forward of step k+1 WHILE the team wavefronts integrate step k; the action is waiting in LDS when the
// next step begins and the actor (9.3 k of 62 k cycles per env step at H = 32, 38 k of 100 k at H = 72) leaves the
// serial path.  Observation j travels with sequence number j + 1 (release / acquire on LDS words), so does action j.
// (the struct LDS layout of citation_wave.h -- CITW_LDS_STRUCT -- measured slower and is not used by any shipped unit)
#ifndef SERL_TEAM_INC_ONCE      // what does not depend on VARIANT: once per unit (rollout_team4_mixed.hip includes this file for two code variants)
#define SERL_TEAM_INC_ONCE 1
#if CITW_GROUP_LANES == 64
__shared__ alignas(64) float g_obsf[16];                      // observation for the actor wavefront (already cast to f32; 7 entries in the attitude task)
__shared__ alignas(64) float g_actout[4];           // action handed back to the team
// SERL_GW_PAD = 1 sizes g_w to a multiple of 64 bytes.  The compiler's LDS layout fills the gap behind an over-aligned object whose size is not a
// multiple of its alignment with the next object that fits WITHOUT padding -- here the 96 KB table block -- so that every blackboard lands beyond
// the 64 KB a DS instruction reaches with its immediate offset: 496 of the kernel's 582 DS instructions carry their address in a VGPR, one
// v_mov_b32 each.  Padded, they sit in the first 48 KB: -226 static instructions, -6 % issued VALU, -7.5 % LDS instructions (ds_read2 pairs).  Round 5
// measured that slower three times and guessed at the tables' bank phase; round 6 counted it (profiles/r06_role_profile.md section 4): the bank-conflict
// cycles are identical to the last digit, the removed moves were never on a waiting chain (SQ_WAIT_INST_LDS +33 %, total wait unchanged), and on
// today's kernels the padded build is 0.3 - 0.7 % faster in four of four comparisons.  On by measurement.
#ifndef SERL_GW_PAD
#define SERL_GW_PAD 1
#endif
__shared__ alignas(64) float g_w[SERL_GW_PAD ? (SERL_LDS_ACTOR_FLOATS + 15) / 16 * 16 : SERL_LDS_ACTOR_FLOATS];      // the episode's actor weights (serl_stage_actor_lds)
__shared__ alignas(64) float g_hrow[128];                     // the actor wavefront's own row: the previous layer, read back as broadcasts (SERL_ACTOR_LDS_BCAST, rollout_device.h)
#else                                                         // two or four episodes per team: one row per lane group
__shared__ alignas(64) float g_obsf[CITW_GROUPS][8];
__shared__ alignas(64) float g_actout[CITW_GROUPS][4];
__shared__ alignas(64) float g_hx[CITW_GROUPS][32];           // previous actor layer of each episode (serl_actor_forward_half32 / _quarter32)
__shared__ alignas(64) int g_qe[CITW_GROUPS];                 // the episode every lane group carries (the actor wavefront picks the member's weights by it)
__shared__ alignas(64) int g_qnext[CITW_GROUPS];              // the episode a lane group takes next from the work queue
#endif
#if CITW_GROUP_LANES == 64 && defined(SERL_ACTOR_WAVES) && SERL_ACTOR_WAVES == 2
__shared__ alignas(64) float g_hxs[2][128];                   // one forward pass over two actor wavefronts: the layer they exchange (serl_actor_forward_split)
__shared__ alignas(64) unsigned g_xflag[2];                   // ... and its hand-over flags
__shared__ alignas(64) float g_cuh[4][128];                   // (remote actor workgroup, serl_actor_forward_cu) every wavefront's own copy of the previous layer
// exchange l of env step j carries the sequence number j * STRIDE + l + 1, l = 0 .. num_layers: the stride must exceed num_layers + 1 (serl_rollout
// accepts up to 16 layers) or a late step's first exchange is satisfied by the previous step's last one
#define SERL_SPLIT_SEQ_STRIDE 32u
#endif
__shared__ alignas(64) unsigned g_oflag;                      // sequence number of the observation; SERL_OBS_DONE = the episode(s) are over
#ifndef SERL_ACTOR_WAVES
#define SERL_ACTOR_WAVES 1            // actor wavefronts beside the team (2: streamed actors, two episodes per team, one episode each)
#endif
__shared__ alignas(64) unsigned g_aflag;            // sequence number of the action
#ifndef SERL_TEAM_SPEC_CACHE
#define SERL_TEAM_SPEC_CACHE (CITW_GROUP_LANES == 64)      // the look-up wavefront keeps its precomputed lanes across evaluations (citation_wave.h CitwSpecCache; one episode per team)
#endif
#ifndef SERL_TEAMS_KREGS
#define SERL_TEAMS_KREGS SERL_TEAM_KREGS      // ... and the team beside a STREAMING actor too (serl_rollout_teams_kernel_<v>: the kernel's register count is the actor wavefront's)
#endif
#ifndef SERL_TEAM_KREGS
#define SERL_TEAM_KREGS 0             // 1: the one-episode team keeps its role's f64 literals in registers (citation_wave.h CitwKRegs; units that define it stage g_klit)
#endif
#if SERL_TEAM_KREGS
__shared__ alignas(64) double g_klit[8][CITW_NK];             // row r: the literals of role r of the generated evaluation (citw_<v>_team_klit)
#endif
__shared__ alignas(64) double g_ttab[8];                      // (SERL_TEAM_TVEC == 2) time of the evaluation behind stage st, less t0
#if CITW_GROUP_LANES != 64
__shared__ alignas(64) float g_hrow[SERL_ACTOR_WAVES][128];   // every actor wavefront's own row: the previous layer of a streamed forward pass, read back as broadcasts (SERL_ACTOR_LDS_BCAST, rollout_device.h)
#endif
__shared__ alignas(64) unsigned g_aflagw[4];                  // ... one per actor wavefront when there are several
#define SERL_OBS_DONE 0xffffffffu
#define SERL_TEAM_BARRIERS (6 * (W_PASTE(W_PASTE(citw_, VARIANT), _team_BARRIERS) - (CITW_NO_BARRIER & 1) - ((CITW_NO_BARRIER >> 1) & 1)))     // workgroup barriers of one env step: 6 model evaluations x (B1, B2)

// Which part of the partitioned evaluation ("role", gen/citation_<variant>_team.inc) a hardware wavefront executes.
// Wavefronts w and w + 4 of a workgroup land on the same SIMD (measured: HW_ID of every wavefront, tools/ab.py); the generated
// file may name a permutation (citw_<variant>_team_ROLE_OF_WAVE) that pairs the role with the serial look-up chain (role 0)
// with a light one and keeps the heavy helper roles apart.
#ifndef SERL_TEAM_ROLES
#define SERL_TEAM_ROLES {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}
#endif
#ifndef SERL_TEAMS_ROLES
#define SERL_TEAMS_ROLES SERL_TEAM_ROLES      // the map of the kernels whose actor wavefront streams its weights (a busy neighbour: family_team.hip)
#endif
// (the map is a nibble per hardware wavefront in one 32-bit literal: readfirstlane + four scalar instructions where a chain of selects
// over the array took sixteen -- and a team wavefront asks eight times per env step)
static constexpr unsigned serl_team_role_nibbles(const int (&r)[16])
{
  unsigned m = 0;
  for (int i = 0; i < 8; ++i) m |= ((unsigned)r[i] & 15u) << (4 * i);
  return m;
}
static __device__ __forceinline__ int serl_team_role(const bool stream = false)
{
  static_assert(W_TEAM_WAVES + 1 <= 8, "eight wavefronts per workgroup at most (seven team wavefronts + the actor, or six + two): a nibble each");
  constexpr int roles_lds[16] = SERL_TEAM_ROLES, roles_stream[16] = SERL_TEAMS_ROLES;
  constexpr unsigned map_lds = serl_team_role_nibbles(roles_lds), map_stream = serl_team_role_nibbles(roles_stream);
  const unsigned sh = ((unsigned)__builtin_amdgcn_readfirstlane((int)threadIdx.x) >> 4) & 0x1cu;      // 4 x (wavefront index)
  return (int)(((stream ? map_stream : map_lds) >> sh) & 15u);
}

static __device__ __forceinline__ double serl_readlane_f64(double v, int srclane)
{
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, srclane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), srclane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
#endif      // SERL_TEAM_INC_ONCE
#if CITW_GROUP_LANES != 64
#ifdef SERL_TEAMG_TAG      // (family_team2s.hip: six team wavefronts + two actor wavefronts)
#define W_TEAMG(x) W_PASTE(W_PASTE(x, SERL_TEAMG_TAG), VARIANT)
#elif CITW_GROUP_LANES == 32
#define W_TEAMG(x) W_PASTE(W_PASTE(x, team2_), VARIANT)
#else
#define W_TEAMG(x) W_PASTE(W_PASTE(x, team4_), VARIANT)
#endif
#endif

// One ODE5 macro step of the reference's step(cmd, out) @0x6030 (inlined rt_ertODEUpdateContinuousStates @0x9eb8..0xa4f3:
// six model evaluations, the first in major-step mode) and the clock update -- without the output latch in front of it.
// fseq: the team's count of env steps, the sequence number of the hand-over flags (wave-uniform; see gen/citation_<v>_team.inc)
// hold (per lane group): the group carries no live episode in this step (it finished, or waits for the queue): its state row is
// left alone, so that the reset of the group's next episode -- written by every wavefront behind this step -- has no other writer
// role_in: the caller's copy of serl_team_role() (development builds: a role map from the environment; -1: computed here)
// stream_map: the team works beside an actor wavefront that streams its weights (SERL_TEAMS_ROLES)
static __device__ __forceinline__ void W_NAME(citw_team_integrate_)(const int wv, CitwState &s, const double (&cmd)[10], const unsigned fseq,
                                                                    const bool hold = false, const int role_in = -1, const bool stream_map = false,
                                                                    const bool HAVE_K = false, const CitwKRegs &KR = citw_no_kregs,
                                                                    const bool HAVE_SC = false, CitwSpecCache &SC = citw_no_spec_cache,
                                                                    const bool HAVE_PC = false, CitwPassCache &PC = citw_no_pass_cache)
{
#define W_ROLE() (role_in >= 0 ? role_in : serl_team_role(stream_map))      // (recomputed at every use: a copy held across the stage loop cost eight scalar spills)
  const int lane = CITW_LANE;          // lane within the episode's lane group (the whole wavefront unless two episodes share the team)
  const int li = lane < 19 ? lane : 18;
  const double h = 0.01, t0 = s.t;
  const double yi = s.xi;
  double xl = yi;                      // lane i < 19: state i of the evaluation to come (what g_xs holds), handed to the generated code in registers
  double stop = 0.0, T = t0;
#ifndef SERL_TEAM_TVEC
#define SERL_TEAM_TVEC (CITW_GROUP_LANES == 64 ? 0 : CITW_GROUP_LANES == 16 ? 2 : 1)      // (sessions ag / ah, us per env step.  Lane vector: four per team 21.46 -> 21.13, two per team with streamed actors 20.8 -> 20.6, one per team 15.71 -> 15.81 (off there); LDS table: four per team 21.13 -> 20.96, SERL10 17.17 -> 17.5, others flat)
#endif
#if SERL_TEAM_TVEC == 2
  // ... or row st of a six-entry LDS table (citw_team_stage_), fetched at the top of the stage: one ds_read in front of the evaluation
#elif SERL_TEAM_TVEC
  // the time of the evaluation behind stage st, less t0: lane st of a register (the same folded products the select chain chose from --
  // two v_readlane per stage where five 64-bit literals went through ~20 scalar compares and selects)
#if SERL_TEAM_TVEC != 2
  double tvec;
  {
    const int al = (int)(threadIdx.x & 63u);
    tvec = citw_ode5_b(0, 0) * h;
    tvec = al == 1 ? h * 0.3 : tvec;
    tvec = al == 2 ? h * 0.8 : tvec;
    tvec = al == 3 ? h * 0.8888888888888888 : tvec;
    tvec = al >= 4 ? h * 1.0 : tvec;
  }
#endif
#endif
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 10; ++i) g_cmd[wv][i] = cmd[i];
  }
  CITW_WAVE_FENCE();      // lane 0 stored, every lane of this wavefront loads (citation_wave.h)
  // what does not change over the six evaluations; every wavefront of the team computes it into its own LDS rows
  W_PASTE(W_PASTE(citw_, VARIANT), _step_invariants)(W_ROLE(), 0);
#ifdef CITW_ROLE_PRIO_MASK      // a static issue priority for roles that make no libm calls for the team (family_team.hip)
  if ((CITW_ROLE_PRIO_MASK >> W_ROLE()) & 1) __builtin_amdgcn_s_setprio(1);
#endif
#pragma nounroll
  for (int st = 0; st < 6; ++st) {
#if SERL_TEAM_TVEC == 2
    const double tnext = g_ttab[st];
#endif
    // lane i < 19: X_i = y_i + sum_j f_j,i * (B[st][j] * h), accumulated in j order like the reference.  The terms of the
    // earlier stages first, in front of the evaluation (their loads and multiply-adds overlap it) ...
#ifndef CITW_ODE_SPLIT
#define CITW_ODE_SPLIT 0      // measured (r03 sweep 3): 20.8 us per env step with the split, 20.4 without -- the loads in front of the evaluation delay its own first loads
#endif
#if CITW_ODE_SPLIT
    const double part = citw_ode5_partial(st, g_f[wv], li);
#if CITW_GROUP_LANES < 32
    const double partm = citw_ode5_partial(st, g_f[wv], lane < 3 ? lane + 16 : 18);
#endif
#endif
    // wave-uniform (scalar) branch inside: each wavefront executes exactly one part of the evaluation and its two barriers
#if CITW_ABLATE_MASK
    // timing experiments only (tools/sweep_build.py): the wavefronts of the mask skip their part of the evaluation -- they raise
    // their hand-over flags and execute the two barriers -- and the state is frozen (values stay sane, the results mean nothing)
    double r = 0.0;
    if ((CITW_ABLATE_MASK >> W_ROLE()) & 1) {
      const unsigned seq_ = fseq * 8u + (unsigned)st + 1u;
      citw_flag_raise(W_ROLE(), seq_);
      citw_flag_raise(8 + W_ROLE(), seq_);
      citw_iflag_raise(W_ROLE(), seq_);
      citw_pflag_raise(W_ROLE(), seq_ * 16u + 15u);
      CITW_TEAM_BARRIER1();
      CITW_TEAM_BARRIER2();
    } else r = W_TEAM_EVAL(W_ROLE(), st, T, s.tick, fseq, xl, HAVE_K, KR, HAVE_SC, SC, HAVE_PC, PC);
#else
    const double r = W_TEAM_EVAL(W_ROLE(), st, T, s.tick, fseq, xl, HAVE_K, KR, HAVE_SC, SC, HAVE_PC, PC);
#endif
    CITW_T0();
    if (st == 0) stop = r;
    // ... the new stage's term and the state behind its last barrier
#if CITW_ODE_SPLIT
    const double xn = citw_ode5_finish(st, part, g_f[wv], li, yi);
#else
    const double xn = (CITW_ABLATE_LOOK & 128) ? yi : citw_ode5_combine(st, g_f[wv], li, yi);
#endif
#if CITW_GROUP_LANES >= 32
    if (lane < 19 && !hold && !CITW_ABLATE) g_xs[wv][lane] = xn;
    if (!CITW_ABLATE) xl = xn;
    if (st == 5) s.xi = xn;
    CITW_WAVE_FENCE();    // lanes 0 .. 18 stored the states, every lane loads them in the next evaluation
#else     // 16 lanes per episode: states 16..18 in a second pass
#if CITW_ODE_SPLIT
    const double xm = citw_ode5_finish(st, partm, g_f[wv], lane < 3 ? lane + 16 : 18, s.xj);
#else
    const double xm = citw_ode5_combine(st, g_f[wv], lane < 3 ? lane + 16 : 18, s.xj);
#endif
    if (!hold) g_xs[wv][lane] = xn;
    if (lane < 3 && !hold) g_xs[wv][lane + 16] = xm;
    if (st == 5) { s.xi = xn; s.xj = xm; }
    CITW_WAVE_FENCE();
#endif
#if SERL_TEAM_TVEC == 2
    T = (st == 4) ? stop : tnext + t0;
#elif SERL_TEAM_TVEC
    T = (st == 4) ? stop : serl_readlane_f64(tvec, st) + t0;
#else
    T = (st == 4) ? stop : (st == 0 ? citw_ode5_b(0, 0) * h + t0 : h * citw_ode5_a(st) + t0);
#endif
    CITW_JIT(0xa30u, fseq * 8u + (unsigned)st);
    CITW_T(20);
  }
  s.tick += 1;
  s.t = stop;
}

#undef W_ROLE
// One call of the reference's exported step(cmd[10], out[12]): the outputs are the states BEFORE integrating (rtY latch)
static __device__ __forceinline__ void W_NAME(citw_team_step_)(const int wv, CitwState &s, const double (&cmd)[10], double (&out)[12], const unsigned fseq)
{
#pragma unroll
  for (int i = 0; i < 12; ++i) out[i] = g_xs[wv][i];
  W_NAME(citw_team_integrate_)(wv, s, cmd, fseq);
}

static __device__ __forceinline__ void W_NAME(citw_team_reset_)(const int wv, CitwState &s, const RolloutArgs &a)
{
  const int lane = CITW_LANE;
  s.xi = a.x0[lane < 19 ? lane : 18];
  s.xj = a.x0[lane < 3 ? lane + 16 : 18];
  s.t = 0.0; s.tick = 0;
  for (int i = lane; i < 19; i += CITW_GROUP_LANES) g_xs[wv][i] = a.x0[i];
  for (int i = lane; i < 29; i += CITW_GROUP_LANES) g_dw[wv][i] = a.dw0[i];
  CITW_WAVE_FENCE();
}

#if CITW_GROUP_LANES == 64
// The ACTOR wavefront of one episode keeps the env step's BOOKS (round 4) and computes the actions; the team wavefronts only integrate.
//
// env step k (envs/phlabenv.py:430-482) reads the state x_k at its top and needs the command of action k.  Action k is a function
// of x_(k-1) (the one-step transport delay above), so the actor wavefront has a whole step for everything that hangs on x_k and
// not on the integration of step k: tracking error, reward, cost, termination, the next observation, the traces, the forward
// pass of action k + 1 and its command (noise, scaling, incremental integration, fault clips).  Until round 4 the team's first
// wavefront kept the books at the top of every step, in front of the integration: 1.4 k of 39 k cycles per env step with the
// other six waiting at the first hand-over.  Now:
//   team, top of step k:   wave 0 raises g_oflag = k + 2 ("x_k is in g_xs"); every team wavefront tests the termination of step k
//                          (three states, the clock), waits for g_aflag >= k + 1, reads the command (three doubles) and integrates
//   actor, iteration k:    waits for g_oflag >= k + 2, reads x_k (before it arrives at the step's second barrier: the team
//                          overwrites g_xs behind it), books of step k, stops where the team stops (the same test on the same
//                          values), forward pass of action k + 1 paying the step's barriers as it goes, command k + 1 -> g_cmdout,
//                          g_aflag = k + 2 BEFORE the last piece's barriers (the team finds the command waiting), the rest of the barriers
// X: observation / action widths from the descriptor (env configurations other than the attitude task; rollout_wave.inc)
// STREAM: the kernel for the attitude-task shapes whose weights do not live in LDS (H = 72 / 96 ...): like X, the actor streams
// them and runs at priority (below) -- a kernel of its own so that the default one carries no trace of it (measured: the
// priority test alone moved the default kernel's code enough to cost it 1.2 %)
// SPLIT: two actor wavefronts share one forward pass (serl_actor_forward_split); the first keeps the books and hands the observation on
__shared__ alignas(64) double g_cmdout[4];          // command of the next env step (elevator, aileron, rudder), handed to the team
#if SERL_ACTOR_WAVES == 2
__shared__ alignas(64) unsigned g_oflag2;                     // observation hand-over from the first actor wavefront to the second (SERL_OBS_DONE: over)
#endif

// REMOTE (round 6, serl_rollout_teamr_kernel_<v>): the actor wavefront(s) of an episode run in a workgroup of their OWN on another CU -- 226 of 256 CUs idle
// at BASELINE config 2 -- so that the forward pass of a streamed actor (hidden 72 / 96: most of a step) no longer shares a SIMD with a team wavefront.  x_k arrives
// through the episode's mailbox in global memory instead of g_oflag / g_xs, the command leaves through it instead of g_aflag / g_cmdout (device-scope release /
// acquire, SerlMail), and there are no team barriers to pay (SerlNoCredit).  Everything else -- books, forward pass, command -- is the code below, unchanged.
template <bool X, bool STREAM = false, bool SPLIT = false, bool REMOTE = false>
static __device__ void W_NAME(serl_team_actor_wave_)(const RolloutArgs &a, int e, const bool lds_actor, SerlMail *mail = nullptr)
{
  using Credit = typename std::conditional<REMOTE, SerlNoCredit, SerlBarrierCredit>::type;
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  constexpr int wv = 0;
  // the activations' coefficients in registers for the episode (rollout_device.h DET_K; the LDS-resident forward pass of the kernel that staged g_klit)
  constexpr bool ACTOR_K = (SERL_TEAM_KREGS != 0) && !X && !STREAM && !SPLIT;
  CitwKRegs kregs;
#if SERL_TEAM_KREGS
  if constexpr (ACTOR_K) {
#pragma unroll
    for (int j = 0; j < SERL_DET_NK; ++j) kregs.k[j] = g_klit[7][j];
  }
#endif
  const float *wts = d.weights + (size_t)d.member_of_episode[e] * d.weight_stride;
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
  double x[12], err[3] = {0, 0, 0}, obs[NO], u[3] = {0, 0, 0};
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
  if (d.err0) for (int i = 0; i < 3; ++i) if (i < A) err[i] = d.err0[(size_t)e * 3 + i];
  double V0 = 0.0, t = 0.0, fitness = 0.0;
  int cost_steps = 0;
  const bool prof = a.prof != nullptr && blockIdx.x == 0;
  unsigned long long busy = 0, t_fwd = 0, t_x = 0, t_obs = 0;
  // An actor that streams its weights (H = 72 / 96, the other env configurations) needs most of a step for its forward pass
  // and executes the step's barriers between its pieces: it wins the issue arbitration on the SIMD it shares with a team
  // wavefront (SERL10: 26.2 -> 25.0 us per env step, TD3 actor 25.6 -> 24.5; the LDS-resident actor is done in a fifth of a step)
#ifndef SERL_STREAM_ACTOR_PRIO
#define SERL_STREAM_ACTOR_PRIO 1
#endif
#ifndef SERL_SPLIT_ACTOR_PRIO
#define SERL_SPLIT_ACTOR_PRIO 1
#endif
  if constexpr (SPLIT) { if (SERL_SPLIT_ACTOR_PRIO) __builtin_amdgcn_s_setprio(SERL_SPLIT_ACTOR_PRIO); }
  else if constexpr (X || STREAM) { if (SERL_STREAM_ACTOR_PRIO) __builtin_amdgcn_s_setprio(SERL_STREAM_ACTOR_PRIO); }
  // reference table rows are fetched one env step ahead: the HBM / L2 latency of the load passes behind the forward pass
  double pr0 = 0.0, pr1 = 0.0, pr2 = 0.0;
  if (!rspec) { pr0 = ref[0]; pr1 = ref[1]; pr2 = ref[2]; }
  // k == -1: the step env.reset() takes with a zero command (envs/phlabenv.py:409-413)
  for (int k = -1;; ++k) {
    const unsigned long long tq = prof ? __builtin_readcyclecounter() : 0ull;
    // the reference sample of this step: fetched / generated now, at the pre-increment time t_k (envs/phlabenv.py:349,473)
    double rk0 = 0.0, rk1 = 0.0, rk2 = 0.0;
    if (rspec) serl_ref_generate(rspec, t, d.t_max, rk0, rk1, rk2);
    else { rk0 = pr0; rk1 = pr1; rk2 = pr2; }      // row max(k, 0) of the table, fetched during the previous iteration
    // what step() returns: the states BEFORE it integrates
    if constexpr (REMOTE) {
      while ((int)(__hip_atomic_load(&mail->xseq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - (unsigned)(k + 2)) < 0) __builtin_amdgcn_s_sleep(4);
    } else {
      while ((int)(__hip_atomic_load(&g_oflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - (unsigned)(k + 2)) < 0) __builtin_amdgcn_s_sleep(2);
    }
    CITW_JIT(0xa20u, (unsigned)(k + 1));
    const unsigned long long t0 = prof ? __builtin_readcyclecounter() : 0ull;
    t_obs += t0 - tq;
    if constexpr (REMOTE) {
#pragma unroll
      for (int i = 0; i < 12; ++i) x[i] = __builtin_nontemporal_load(&mail->x[i]);      // (behind the acquire; the team's courier does not touch them again before our command)
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) x[i] = g_xs[wv][i];
    }
    if (snoise) {      // what step() returns gets the sensor model on top; the plant state stays clean
      const double *sn = snoise + (size_t)(k + 1) * 7;
      x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
    }
#ifndef SERL_ACTOR_EARLY_BARRIERS
#define SERL_ACTOR_EARLY_BARRIERS 0      // (measured, session ab: 1 / 2 barriers in front of the books -- SERL50 15.95 -> 15.97 / 16.18, SERL10 17.6 -> 18.9 / 18.5: off)
#endif
#if SERL_ACTOR_EARLY_BARRIERS
    Credit credit{0, SERL_TEAM_BARRIERS};
#if CITW_JITTER
    credit.salt = (unsigned)(k + 1);
#endif
    // x_k is in registers: the first barrier(s) of the step's first evaluation are paid in front of the books, so that the team never
    // finds the actor wavefront missing there (a step that ends here takes the `break` below: the team leaves at the same step without them)
    {
      const bool fin0 = k >= 0 && ((t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0) || k + 1 >= d.max_steps);
      if constexpr (!SPLIT) { if (!fin0) credit.upto(SERL_ACTOR_EARLY_BARRIERS); }      // (two actor wavefronts: the partner has not got the observation yet -- it could not follow)
    }
#endif
    if (k >= 0) {
      // ---- the books of env step k; `act`, `u` are those of action k (the end of the previous iteration)
      const bool fin = (t >= d.t_max) || (fabs(x[7]) > max_theta) || (fabs(x[6]) > max_phi) || (x[9] < 50.0);
      double nobs[NO];
#pragma unroll
      for (int i = 0; i < NO; ++i) nobs[i] = 0.0;
      err[0] = rk0 - x[7];
      if (A > 1) { err[1] = rk1 - x[6]; err[2] = rk2 - x[5]; }
      double rsum = 0.0;
      for (int i = 0; i < 3; ++i) if (i < A) rsum = rsum + fabs(serl_clip(scaler[i] * err[i], -1.0, 1.0));
      double reward = -rsum / (X ? (double)A : 3.0);
      const int cost = (rad2deg * fabs(x[4]) > 11.0) || (rad2deg * fabs(x[6]) > 0.75 * max_phi) || (x[3] < V0 / 3.0);
      build_obs(nobs);
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
      if (fin || k + 1 >= d.max_steps) {      // (the team wavefronts leave at the same step: the same test on the same values)
        if (lane == 0) {
          d.fitness[e] = fitness;
          d.length_steps[e] = fin ? k + 1 : -(k + 1);     // negative: reference table exhausted before `done`
          d.length_t[e] = t;
          d.cost_steps[e] = cost_steps;
#if SERL_ACTOR_WAVES == 2
          if constexpr (SPLIT || REMOTE) __hip_atomic_store(&g_oflag2, SERL_OBS_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
        }
        if (prof && lane == 0) a.prof[3] = (unsigned long long)(k + 1);
        break;        // (the reference integrates once more inside its last step(); nothing observes that state)
      }
    } else {
      V0 = x[3];
      build_obs(obs);
    }
    // ---- action k + 1 = actor(observation k + 1), while the team integrates step k
    float obsf[NO];
#pragma unroll
    for (int i = 0; i < NO; ++i) obsf[i] = (float)obs[i];
#if SERL_ACTOR_WAVES == 2
    if constexpr (SPLIT || REMOTE) {
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) g_obsf[i] = obsf[i];
        __hip_atomic_store(&g_oflag2, (unsigned)(k + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
#endif
    if (!rspec) { const size_t nr = (size_t)(k + 1) * 3; pr0 = ref[nr]; pr1 = ref[nr + 1]; pr2 = ref[nr + 2]; }   // (k + 1 < max_steps here)
#if !SERL_ACTOR_EARLY_BARRIERS
    Credit credit{0, SERL_TEAM_BARRIERS};
#if CITW_JITTER
    credit.salt = (unsigned)(k + 1);
#endif
#endif
    credit.defer_last = true;      // the command goes out in front of the last piece's barriers
    const unsigned long long t1 = prof ? __builtin_readcyclecounter() : 0ull;
    if constexpr (REMOTE) {
#if SERL_ACTOR_WAVES == 2
      serl_actor_forward_cu_any(d, wts, obsf, act, 0, g_hxs, &g_cuh[0][0]);      // wavefront 0 of the four that share the pass (the others: serl_remote_helper_wave_)
#endif
    } else if constexpr (SPLIT) {
#if SERL_ACTOR_WAVES == 2
      serl_actor_forward_split(d, wts, obsf, act, credit, 0, g_hxs, g_xflag, (unsigned)(k + 1) * SERL_SPLIT_SEQ_STRIDE, prof ? &t_x : nullptr);
#endif
    } else if constexpr (X) serl_actor_forward_wave<true>(d, wts, obsf, act, credit);
    else if constexpr (STREAM) serl_actor_forward<SERL_ACTOR_LDS_BCAST != 0, false>(d, wts, obsf, act, credit, g_hrow);
    else if (lds_actor) serl_actor_forward_lds<SERL_ACTOR_LDS_BCAST != 0>(d, g_w, obsf, act, credit, g_hrow, ACTOR_K, kregs);
    else __builtin_trap();      // (serl_capi.hip sends every shape without LDS-resident weights to the streaming kernels: this kernel carries none of their code)
    if (prof) t_fwd += __builtin_readcyclecounter() - t1;      // (includes the barriers it was early for and, split, the waits for the partner)
    // ---- env step k + 1, the part in front of the integration (envs/phlabenv.py:430-450), wave-uniform
    double scl[3] = {0.0, 0.0, 0.0};
    if (noise) {
      for (int i = 0; i < 3; ++i) {
        if (i >= A) continue;
        double an = serl_clip((double)act[i] + noise[(size_t)(k + 1) * 3 + i], -1.0, 1.0);
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
    CITW_JIT(0xa00u, (unsigned)(k + 1));
    if (lane == 0) {
      if constexpr (REMOTE) {
        mail->cmd[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
        mail->cmd[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
        mail->cmd[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
        __hip_atomic_store(&mail->aseq, (unsigned)(k + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        g_cmdout[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
        g_cmdout[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
        g_cmdout[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
        __hip_atomic_store(&g_aflag, (unsigned)(k + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    if (prof) busy += __builtin_readcyclecounter() - t0;        // (includes the waits at the barriers it was early for)
    credit.defer_last = false;
    credit(0, 1);                                                // the rest of this step's barriers
  }
  if (prof && lane == 0) {
    if constexpr (SPLIT) { a.prof[26] = t_fwd; a.prof[28] = t_x; a.prof[30] = t_obs; }
    else a.prof[31] = busy;
  }
}

#if SERL_ACTOR_WAVES == 2
// The second of TWO actor wavefronts that share ONE forward pass (actors that stream their weights, H > 64: SERL10's 72, the TD3
// actor's 96): each owns half of every layer's rows and half of the weight traffic (serl_actor_forward_split, rollout_device.h);
// the first one keeps the books and hands the command back.  Both pay the step's barriers as they go, with equal counts at every exchange.
template <bool REMOTE = false>
static __device__ void W_NAME(serl_team_actor_split_wave_)(const RolloutArgs &a, int e)
{
  using Credit = typename std::conditional<REMOTE, SerlNoCredit, SerlBarrierCredit>::type;
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  const float *wts = d.weights + (size_t)d.member_of_episode[e] * d.weight_stride;
  if (SERL_SPLIT_ACTOR_PRIO) __builtin_amdgcn_s_setprio(SERL_SPLIT_ACTOR_PRIO);      // (like the lone streaming actor: it pays the barriers between its pieces)
  const bool prof = a.prof != nullptr && blockIdx.x == 0;
  unsigned long long t_fwd = 0, t_x = 0, t_obs = 0;
  for (unsigned j = 0;; ++j) {
    unsigned fl;
    const unsigned long long tq = prof ? __builtin_readcyclecounter() : 0ull;
    while ((fl = __hip_atomic_load(&g_oflag2, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != SERL_OBS_DONE && (int)(fl - (j + 1u)) < 0)
      __builtin_amdgcn_s_sleep(2);
    if (fl == SERL_OBS_DONE) break;
    const unsigned long long t0 = prof ? __builtin_readcyclecounter() : 0ull;
    t_obs += t0 - tq;
    float obsf[7], act[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 7; ++i) obsf[i] = g_obsf[i];
    Credit credit{0, SERL_TEAM_BARRIERS};
    credit.defer_last = true;      // (like its partner: equal barrier counts at every exchange)
#if CITW_JITTER
    credit.salt = j;
#endif
    serl_actor_forward_split(d, wts, obsf, act, credit, 1, g_hxs, g_xflag, j * SERL_SPLIT_SEQ_STRIDE, prof ? &t_x : nullptr);
    if (prof) t_fwd += __builtin_readcyclecounter() - t0;
    credit.defer_last = false;
    credit(0, 1);                                                // the rest of this step's barriers
  }
  if (prof && lane == 0) { a.prof[27] = t_fwd; a.prof[29] = t_x; a.prof[31] = t_obs; }
}
#endif

#ifndef SERL_TEAM_FAST_TOP
#define SERL_TEAM_FAST_TOP 1
#endif
#ifndef SERL_TEAMS_FAST_TOP
#define SERL_TEAMS_FAST_TOP 0      // (session ac: beside a streaming actor the command is often not there yet and the combined read is wasted -- SERL10 17.55 with it, 17.02 without; TD3 actor 16.37 / 16.17)
#endif
// A team wavefront's walk through the episode: the termination test and the command of every env step, then its part of the
// integration.  The books are the actor wavefront's (above).
// FAST: the step top that reads nothing twice (below) -- the kernels whose actor streams its weights choose for themselves (SERL_TEAMS_FAST_TOP)
// KREGS: this wavefront's role keeps its f64 literals in registers for the episode (citation_wave.h CitwKRegs; g_klit staged by the kernel)
template <bool X, bool FAST = (SERL_TEAM_FAST_TOP != 0), bool STREAM_MAP = false, bool KREGS = false>
static __device__ __forceinline__ void W_NAME(serl_team_episode_)(const RolloutArgs &a, const int wv, int e)
{
  CitwSpecCache spec_cache;      // the look-up wavefront's precomputed lanes, kept while no interval moves (citation_wave.h CitwSpecCache)
  spec_cache.valid = false;
  CitwKRegs kregs;

  const serl_rollout_desc &d = a.d;
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double dt = 0.01;
  const double *snoise = nullptr;     // this episode's row of pre-drawn sensor noise: the termination test sees what step() returns
  if (d.sensor_noise) {
    const int sr = d.sensor_row ? d.sensor_row[e] : e;
    if (sr >= 0) snoise = d.sensor_noise + (size_t)sr * ((size_t)d.max_steps + 1) * 7;
  }
  CitwState s;
  double cmd[10];
  W_NAME(citw_team_reset_)(wv, s, a);
  if (d.tick0) { s.tick = (unsigned)d.tick0[e]; s.t = (double)s.tick * 0.01; }   // initialize() leaves the model clock running
#pragma unroll
  for (int i = 0; i < 10; ++i) cmd[i] = 0.0;
  {      // the step env.reset() takes: a zero action through the episode's faults (a jammed rudder is jammed from the start)
    serl_fault_row f = {1.0, __longlong_as_double(0x7ff0000000000000LL), __longlong_as_double(0x7ff0000000000000LL),
                        0.0, 0.0, 0, 0, 0};
    if (d.faults) f = d.faults[e];
    cmd[0] = serl_clip(0.0 * f.elev_gain, -f.elev_clip, f.elev_clip);
    cmd[1] = serl_clip(0.0, -f.ail_clip, f.ail_clip);
    cmd[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : 0.0;
  }
  double t = 0.0;
  int k = -1;      // k == -1: the step env.reset() takes with a zero command (envs/phlabenv.py:409-413)
  const bool prof = a.prof != nullptr && blockIdx.x == 0 && threadIdx.x < 64;
  unsigned long long pc_actor = 0, pc_dyn = 0, tc0 = 0, tc1 = 0;
  const bool lead = __builtin_amdgcn_readfirstlane((int)threadIdx.x) < 64;
#if defined(SERL_DEV_ROLE_MAP) && SERL_DEV_ROLE_MAP && !CITW_JITTER
  // development builds (tools/sweep_roles.py): roles <-> wavefronts from SERL_JITTER_SITES (a nibble per hardware wavefront; all ones = the compiled map)
  const int role = a.jitter_sites == ~0u ? serl_team_role(STREAM_MAP)
                   : (int)((a.jitter_sites >> (4 * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)))) & 15u);
#else
  constexpr int role = -1;      // (computed where it is used: one more SGPR live across the episode loop cost 22 scalar spills; round 5, r05s: held in an SGPR 13.83 us per env step against 13.72)
#endif
#if SERL_TEAM_KREGS
  if constexpr (KREGS) {      // this wavefront's role keeps its f64 literals in registers for the episode: its row of g_klit (citation_wave.h CITW_K)
    const int r_ = role >= 0 ? role : serl_team_role(STREAM_MAP);
#pragma unroll
    for (int j = 0; j < W_PASTE(W_PASTE(citw_, VARIANT), _team_NKLIT); ++j) kregs.k[j] = g_klit[r_][j];
  }
#endif
  for (;;) {
    if (prof) tc0 = __builtin_readcyclecounter();
    // x_k is final: every team wavefront stored the same states behind the last barrier of the integration (or the reset); the
    // first one tells the actor wavefront
    CITW_JIT(0xa20u, (unsigned)(k + 1));
    if (lead && (threadIdx.x & 63) == 0) __hip_atomic_store(&g_oflag, (unsigned)(k + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k >= 0) {
      // FAST: the three states of the termination test out of this wavefront's own registers (lane i < 19 holds state i: what it stored into
      // g_xs behind the last barrier), the hand-over flag and the command in ONE LDS round trip (below): two round trips less per env step
      double x6 = FAST ? serl_readlane_f64(s.xi, 6) : g_xs[wv][6], x7 = FAST ? serl_readlane_f64(s.xi, 7) : g_xs[wv][7];
      const double x9 = FAST ? serl_readlane_f64(s.xi, 9) : g_xs[wv][9];
      if (snoise) { const double *sn = snoise + (size_t)(k + 1) * 7; x6 += sn[5]; x7 += sn[6]; }
      const bool fin = (t >= d.t_max) || (fabs(x7) > max_theta) || (fabs(x6) > max_phi) || (x9 < 50.0);
      t += dt;
      if (fin || k + 1 >= d.max_steps) { ++k; break; }      // (the reference integrates once more inside its last step(); nothing observes that state)
      // ---- the command of this step: the actor wavefront computed it while the previous step was integrated
      if constexpr (FAST) {
      // The flag and the three doubles are read by four LDS instructions in THIS order and waited for once: a wavefront's LDS operations
      // execute in order, so a flag that reads `ready` was read in front of a command that is the ready one (the actor stored the command,
      // then the flag, in order too).  Written as one asm block because nothing in the language keeps a relaxed flag load in front of
      // plain loads (sweep 19 / 39 of round 3 was exactly that reordering); the slow path is the acquire poll.
      unsigned fl;
      double c0, c1, c2;
      {
        const unsigned fa = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned *)&g_aflag;
        const unsigned ca = (unsigned)(unsigned long long)(__attribute__((address_space(3))) double *)&g_cmdout[0];
        asm volatile("ds_read_b32 %0, %4\n\tds_read_b64 %1, %5\n\tds_read_b64 %2, %5 offset:8\n\tds_read_b64 %3, %5 offset:16\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(fl), "=&v"(c0), "=&v"(c1), "=&v"(c2) : "v"(fa), "v"(ca) : "memory");
      }
      if ((int)(fl - (unsigned)(k + 1)) < 0) {
        while ((int)(__hip_atomic_load(&g_aflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - (unsigned)(k + 1)) < 0) __builtin_amdgcn_s_sleep(1);
        c0 = g_cmdout[0]; c1 = g_cmdout[1]; c2 = g_cmdout[2];
      }
      CITW_JIT(0xa10u, (unsigned)k);
      cmd[0] = c0; cmd[1] = c1; cmd[2] = c2;
      } else {
      while ((int)(__hip_atomic_load(&g_aflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - (unsigned)(k + 1)) < 0) __builtin_amdgcn_s_sleep(1);
      CITW_JIT(0xa10u, (unsigned)k);
      cmd[0] = g_cmdout[0]; cmd[1] = g_cmdout[1]; cmd[2] = g_cmdout[2];
      }
    }
    if (prof) { tc1 = __builtin_readcyclecounter(); pc_actor += tc1 - tc0; }
    W_NAME(citw_team_integrate_)(wv, s, cmd, (unsigned)(k + 1), false, role, STREAM_MAP, KREGS && SERL_TEAM_KREGS, kregs, SERL_TEAM_SPEC_CACHE != 0, spec_cache);     // the only call site: one copy of the model in the code object
    if (prof) pc_dyn += __builtin_readcyclecounter() - tc1;
    ++k;
  }
  if (prof && (threadIdx.x & 63) == 0) {
    a.prof[0] = pc_actor; a.prof[1] = pc_dyn; a.prof[2] = 0;
#ifdef CITW_PROFILE
    for (int i = 0; i < 27; ++i) a.prof[4 + i] = g_prof[i];
#endif
  }
}

#if defined(SERL_TEAM_REMOTE) && SERL_ACTOR_WAVES == 2
// Wavefronts 1 .. 3 of the remote actor workgroup: their share of every forward pass (serl_actor_forward_cu), started by the observation wavefront 0 hands on
static __device__ void W_NAME(serl_remote_helper_wave_)(const RolloutArgs &a, int e, const int wave)
{
  const serl_rollout_desc &d = a.d;
  const float *wts = d.weights + (size_t)d.member_of_episode[e] * d.weight_stride;
  for (unsigned j = 0;; ++j) {
    unsigned fl;
    while ((fl = __hip_atomic_load(&g_oflag2, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) != SERL_OBS_DONE && (int)(fl - (j + 1u)) < 0)
      __builtin_amdgcn_s_sleep(2);
    if (fl == SERL_OBS_DONE) break;
    CITW_JIT(0xa22u, j);
    float obsf[7], act[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 7; ++i) obsf[i] = g_obsf[i];
    serl_actor_forward_cu_any(d, wts, obsf, act, wave, g_hxs, &g_cuh[wave][0]);
  }
}

// The COURIER: the eighth wavefront of a team whose actor lives in a workgroup of its own on another CU (serl_rollout_teamr_kernel_<v>).  It stands where the
// actor wavefront stood -- same LDS hand-over with the seven team wavefronts (g_oflag / g_xs in, g_cmdout / g_aflag out), same barrier credit -- and carries
// the two messages through the episode's mailbox in global memory:
//   top of step k     waits for g_oflag >= k + 2, copies x_k out of g_xs (before it reaches the step's second barrier: the team overwrites g_xs behind it),
//                     tests the termination of step k exactly as the team does (it leaves at the same step), publishes x_k behind xseq = k + 2
//   during step k     pays eleven of the step's twelve barriers (parked: it costs its SIMD nothing)
//   before the last   polls aseq >= k + 2 -- the remote forward pass finished microseconds ago, the L2 round trip of this load hides in the team's last
//                     half evaluation --, copies the command into g_cmdout, raises g_aflag = k + 2, pays the twelfth barrier
static __device__ void W_NAME(serl_team_courier_wave_)(const RolloutArgs &a, int e, SerlMail *mail)
{
  const serl_rollout_desc &d = a.d;
  const int lane = threadIdx.x & 63;
  constexpr int wv = 0;
  const double PI = 3.14159265358979323846;
  const double deg2rad = PI / 180.0;
  const double max_theta = 60.0 * deg2rad, max_phi = 75.0 * deg2rad;
  const double dt = 0.01;
  const double *snoise = nullptr;
  if (d.sensor_noise) {
    const int sr = d.sensor_row ? d.sensor_row[e] : e;
    if (sr >= 0) snoise = d.sensor_noise + (size_t)sr * ((size_t)d.max_steps + 1) * 7;
  }
  double t = 0.0;
  for (int k = -1;; ++k) {
    while ((int)(__hip_atomic_load(&g_oflag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - (unsigned)(k + 2)) < 0) __builtin_amdgcn_s_sleep(2);
    CITW_JIT(0xa20u, (unsigned)(k + 1));
    double x[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) x[i] = g_xs[wv][i];
    if (lane == 0) {      // (one lane stores the message and then its sequence number: program order + release)
#pragma unroll
      for (int i = 0; i < 12; ++i) mail->x[i] = x[i];
      CITW_JIT(0xa21u, (unsigned)(k + 1));
      __hip_atomic_store(&mail->xseq, (unsigned)(k + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (k >= 0) {      // the team's termination test of step k, on the same values (rollout_team.inc serl_team_episode_)
      double x6 = x[6], x7 = x[7];
      const double x9 = x[9];
      if (snoise) { const double *sn = snoise + (size_t)(k + 1) * 7; x6 += sn[5]; x7 += sn[6]; }
      const bool fin = (t >= d.t_max) || (fabs(x7) > max_theta) || (fabs(x6) > max_phi) || (x9 < 50.0);
      t += dt;
      if (fin || k + 1 >= d.max_steps) break;
    }
    SerlBarrierCredit credit{0, SERL_TEAM_BARRIERS};
#if CITW_JITTER
    credit.salt = (unsigned)(k + 1);
#endif
    credit.upto(SERL_TEAM_BARRIERS - 1);
    while ((int)(__hip_atomic_load(&mail->aseq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - (unsigned)(k + 2)) < 0) __builtin_amdgcn_s_sleep(2);
    CITW_JIT(0xa11u, (unsigned)(k + 1));
    const double c0 = __builtin_nontemporal_load(&mail->cmd[0]), c1 = __builtin_nontemporal_load(&mail->cmd[1]), c2 = __builtin_nontemporal_load(&mail->cmd[2]);
    if (lane == 0) {
      g_cmdout[0] = c0; g_cmdout[1] = c1; g_cmdout[2] = c2;
      CITW_JIT(0xa00u, (unsigned)(k + 1));
      __hip_atomic_store(&g_aflag, (unsigned)(k + 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    credit.upto(SERL_TEAM_BARRIERS);
  }
}
#endif

#else
#include "rollout_team_half.inc"      // the same for TWO episodes per team (lanes 0-31 / 32-63)
#endif

// stage the build's tables, the table3 parameters and the look-up descriptors into LDS (whole workgroup)
static __device__ __forceinline__ void W_NAME(citw_team_stage_)(const RolloutArgs &a)
{
  const int nw = W_PASTE(W_PASTE(citw_, VARIANT), _RO_HI_W) - W_PASTE(W_PASTE(citw_, VARIANT), _RO_LO_W);
  const double *src = a.ro + (W_PASTE(W_PASTE(citw_, VARIANT), _RO_LO_W) - W_PASTE(W_PASTE(citw_, VARIANT), _RO_BASE_W));
  for (int i = threadIdx.x; i < nw; i += blockDim.x) g_ro[i] = src[i];
  for (int i = threadIdx.x; i < 46; i += blockDim.x) g_t3[i] = a.t3[i];
  // interval-index slots: the hinted search (citation_wave.h) re-verifies whatever they hold, starting from interval 0
#if !CITW_POISON
  for (int i = threadIdx.x; i < (int)(sizeof(g_sidx) / sizeof(int)); i += blockDim.x) (&g_sidx[0][0])[i] = 0;
#endif
#if CITW_JITTER
  if (threadIdx.x == 0) { g_jseed = a.jitter; g_jsites = a.jitter_sites; }
#endif
#if CITW_POISON
  // hand-over stress builds (citation_wave.h): every blackboard starts as a signalling NaN that names its slot, the interval hints
  // as an out-of-range pattern (the hinted search clamps and re-verifies whatever it finds)
  {
#define W_POISON(arr, id) do { double *p_ = (double *)&(arr); const int n_ = (int)(sizeof(arr) / sizeof(double)); \
      for (int i = threadIdx.x; i < n_; i += blockDim.x) p_[i] = __longlong_as_double(0x7ff4000000000000LL | ((long long)(id) << 32) | (long long)i); } while (0)
    W_POISON(g_in, 1); W_POISON(g_m, 2); W_POISON(g_out0, 3); W_POISON(g_out1, 4); W_POISON(g_out2, 5); W_POISON(g_dw, 6); W_POISON(g_f, 7);
    W_POISON(g_xs, 8); W_POISON(g_cmd, 9); W_POISON(g_act, 10); W_POISON(g_inv, 11); W_POISON(g_x, 12); W_POISON(g_y, 13);
#if CITW_GROUP_LANES == 64
    W_POISON(g_cmdout, 14);
#endif
#undef W_POISON
    for (int i = threadIdx.x; i < (int)(sizeof(g_sidx) / sizeof(int)); i += blockDim.x) (&g_sidx[0][0])[i] = 0x5a5a5a5a;
    for (int i = threadIdx.x; i < (int)(sizeof(g_obsf) / sizeof(float)); i += blockDim.x) ((float *)&g_obsf)[i] = __int_as_float(0x7fa00000 | i);
    for (int i = threadIdx.x; i < (int)(sizeof(g_actout) / sizeof(float)); i += blockDim.x) ((float *)&g_actout)[i] = __int_as_float(0x7fa01000 | i);
#if CITW_GROUP_LANES != 64
    for (int i = threadIdx.x; i < (int)(sizeof(g_hx) / sizeof(float)); i += blockDim.x) ((float *)&g_hx)[i] = __int_as_float(0x7fa02000 | i);
    if (threadIdx.x < CITW_GROUPS) { g_qe[threadIdx.x] = 0x5a5a5a5a; g_qnext[threadIdx.x] = 0x5a5a5a5a; }
#endif
  }
#endif
  // hand-over flags start one below the first evaluation's sequence number (the team's env-step count * 8 + 1)
  if (threadIdx.x == 0) { g_aflag = 0; g_oflag = 0; g_smiss = 0; }
  if (threadIdx.x < 8) {
    constexpr double h_ = 0.01;
    const int al = (int)threadIdx.x;
    double tv = citw_ode5_b(0, 0) * h_;
    tv = al == 1 ? h_ * 0.3 : tv; tv = al == 2 ? h_ * 0.8 : tv; tv = al == 3 ? h_ * 0.8888888888888888 : tv; tv = al >= 4 ? h_ * 1.0 : tv;
    g_ttab[al] = tv;
  }
  if (threadIdx.x < 4) g_aflagw[threadIdx.x] = 0;
#if CITW_GROUP_LANES == 64 && SERL_ACTOR_WAVES == 2
  if (threadIdx.x < 2) g_xflag[threadIdx.x] = 0;
  if (threadIdx.x == 0) g_oflag2 = 0;
#if CITW_POISON
  for (int i = threadIdx.x; i < 256; i += blockDim.x) (&g_hxs[0][0])[i] = __int_as_float(0x7fa03000 | i);
#endif
#endif
  if (threadIdx.x < 16) g_pflag[threadIdx.x] = g_flag[threadIdx.x] = g_iflag[threadIdx.x] = 0u;
#ifdef CITW_TEAM_TABLES      // the team code carries descriptor tables of its own (its look-up rounds are cut differently)
#define W_TAB(x) W_PASTE(W_PASTE(W_PASTE(citw_, VARIANT), _team), x)
#else
#define W_TAB(x) W_PASTE(W_PASTE(citw_, VARIANT), x)
#endif
  for (int i = threadIdx.x; i < W_TAB(_NBP) * CITW_BP_PAD; i += blockDim.x) {
    const CitwBpVec bv = W_TAB(_bpvec)[i / CITW_BP_PAD];
    const int j = i % CITW_BP_PAD;
    g_bp[i / CITW_BP_PAD][j] = j < bv.n ? src[bv.xw + j] : __longlong_as_double(0x7ff0000000000000LL);
  }
#ifdef CITW_TEAM_HAS_K      // (experiment builds: f64 literals of the team code read from LDS)
  for (int i = threadIdx.x; i < W_PASTE(W_PASTE(citw_, VARIANT), _team_NK); i += blockDim.x) g_k[i] = W_PASTE(W_PASTE(citw_, VARIANT), _team_k)[i];
#else
  for (int i = threadIdx.x; i < W_PASTE(W_PASTE(citw_, VARIANT), _NK); i += blockDim.x) g_k[i] = W_PASTE(W_PASTE(citw_, VARIANT), _k)[i];
#endif
#if SERL_TEAM_KREGS
  static_assert(W_PASTE(W_PASTE(citw_, VARIANT), _team_NKLIT) <= CITW_NK && W_PASTE(W_PASTE(citw_, VARIANT), _team_WAVES) <= 8, "register set / role table too small");
  static_assert(W_PASTE(W_PASTE(citw_, VARIANT), _team_WAVES) <= 7 && SERL_DET_NK <= CITW_NK, "row 7 of g_klit is the actor wavefront's");
  for (int i = threadIdx.x; i < W_PASTE(W_PASTE(citw_, VARIANT), _team_WAVES) * W_PASTE(W_PASTE(citw_, VARIANT), _team_NKLIT); i += blockDim.x)
    g_klit[i / W_PASTE(W_PASTE(citw_, VARIANT), _team_NKLIT)][i % W_PASTE(W_PASTE(citw_, VARIANT), _team_NKLIT)] = (&W_PASTE(W_PASTE(citw_, VARIANT), _team_klit)[0][0])[i];
  if (threadIdx.x < SERL_DET_NK) g_klit[7][threadIdx.x] = serl_det_klit[threadIdx.x];      // the actor wavefront's set: the activations' coefficients (rollout_device.h DET_K)
#endif
  const int nr = W_TAB(_ROUNDS);
  const CitwSearch *S = &W_TAB(_search)[0][0];
  const CitwLookup *L = &W_TAB(_lookup)[0][0][0];
#undef W_TAB
  for (int i = threadIdx.x; i < nr * 64; i += blockDim.x) (&g_S[0][0])[i] = S[i];
  for (int i = threadIdx.x; i < nr * 128; i += blockDim.x) (&g_L[0][0][0])[i] = L[i];
  __syncthreads();
}

#if CITW_GROUP_LANES == 64 && SERL_ACTOR_WAVES == 2 && defined(SERL_TEAM_REMOTE)
// Round 6: one episode = TWO workgroups on two CUs.  Workgroup pairs (b, b + 8) -- blockIdx is dealt round-robin to the eight XCDs, so a pair shares an XCD and
// its L2 -- carry episode slot (b / 16) * 8 + b % 8: the lower index runs the ACTOR (four wavefronts sharing one forward pass, two lanes per hidden row: serl_actor_forward_cu;
// the books of every env step), the higher one the TEAM (the seven wavefronts of the LDS-actor kernel with their register sets and role map + the courier).  The
// actor half comes first in dispatch order: a team that is resident never waits for a partner that has not been dispatched.  The host launches it only while
// every workgroup of the launch can be resident at once (serl_capi.hip).
__global__ void __launch_bounds__(64 * (W_TEAM_WAVES + 1)) W_NAME(serl_rollout_teamr_kernel_)(RolloutArgs a)
{
  const int grp = (int)(blockIdx.x >> 4), pos = (int)(blockIdx.x & 15u);
  const bool remote = pos < 8;
  const int slot = grp * 8 + (pos & 7);
  const int e = a.e0 + slot;
  if (e >= a.e_end) return;                                       // (padding workgroups of the last group)
  SerlMail *mail = (SerlMail *)a.mail + slot;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (remote) {
    if (threadIdx.x < 2) g_xflag[threadIdx.x] = 0;
    if (threadIdx.x == 0) g_oflag2 = 0;
#if CITW_JITTER
    if (threadIdx.x == 0) { g_jseed = a.jitter; g_jsites = a.jitter_sites; }
#endif
#if CITW_POISON
    for (int i = threadIdx.x; i < 256; i += blockDim.x) (&g_hxs[0][0])[i] = __int_as_float(0x7fa03000 | i);
#endif
    __syncthreads();
    if (w == 0) W_NAME(serl_team_actor_wave_)<false, false, false, true>(a, e, false, mail);      // books + its quarter of the forward pass
    else if (w < 4) W_NAME(serl_remote_helper_wave_)(a, e, w);
    return;
  }
  W_NAME(citw_team_stage_)(a);
  if (w == W_TEAM_WAVES) W_NAME(serl_team_courier_wave_)(a, e, mail);
  else W_NAME(serl_team_episode_)<false, (SERL_TEAM_FAST_TOP != 0), false, (SERL_TEAM_KREGS != 0)>(a, 0, e);
}

void W_NAME(serl_launch_rollout_teamr_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_teamr_kernel_), dim3(grid), dim3(64 * (W_TEAM_WAVES + 1)), 0, stream, a);
}
#elif CITW_GROUP_LANES == 64 && SERL_ACTOR_WAVES == 2
// six team wavefronts (gen/citation_<v>_team6.inc) + two actor wavefronts that share one forward pass: eight in all
__global__ void __launch_bounds__(64 * (W_TEAM_WAVES + 2)) W_NAME(serl_rollout_teams2_kernel_)(RolloutArgs a)
{
  W_NAME(citw_team_stage_)(a);
  const int e = a.e0 + blockIdx.x;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w == W_TEAM_WAVES) W_NAME(serl_team_actor_wave_)<false, false, true>(a, e, false);      // books + the first half of the forward pass
  else if (w > W_TEAM_WAVES) W_NAME(serl_team_actor_split_wave_)<false>(a, e);
  else W_NAME(serl_team_episode_)<false>(a, 0, e);
}

void W_NAME(serl_launch_rollout_teams2_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_teams2_kernel_), dim3(grid), dim3(64 * (W_TEAM_WAVES + 2)), 0, stream, a);
}
#elif CITW_GROUP_LANES == 64
// W_TEAM_WAVES (7) wavefronts integrate the model, one more runs the actor beside them: two wavefronts per SIMD
__global__ void __launch_bounds__(64 * (W_TEAM_WAVES + 1)) W_NAME(serl_rollout_team_kernel_)(RolloutArgs a)
{
#ifdef CITW_PROFILE
  if (threadIdx.x < 32) g_prof[threadIdx.x] = 0;
#endif
  W_NAME(citw_team_stage_)(a);
  const int e = a.e0 + blockIdx.x;   // one episode per workgroup
  // the member's weights live in LDS for the whole episode when the shape allows it (SERL50: 7-32x4-3)
  const bool lds_actor = __builtin_amdgcn_readfirstlane((int)serl_lds_actor_ok(a.d)) != 0;
  if (lds_actor) {
    serl_stage_actor_lds(a.d, a.d.weights + (size_t)a.d.member_of_episode[e] * a.d.weight_stride, g_w);
    __syncthreads();
  }
  if (a.prof != nullptr && blockIdx.x == 0 && (threadIdx.x & 63) == 0)       // development aid: which SIMD each wavefront landed on (HW_ID[5:4])
    a.prof[16 + (threadIdx.x >> 6)] = 100 + __builtin_amdgcn_s_getreg(((2 - 1) << 11) | (4 << 6) | 4);
#ifdef SERL_TEAM_PRIO0
  // wave 0 owns the serial look-up chain every other wavefront waits for at B1: it wins the issue arbitration on the SIMD it
  // shares with wave 4 (static priority, set once)
  if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 0) __builtin_amdgcn_s_setprio(SERL_TEAM_PRIO0);
#endif
  if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == W_TEAM_WAVES) W_NAME(serl_team_actor_wave_)<false>(a, e, lds_actor);
  else W_NAME(serl_team_episode_)<false, (SERL_TEAM_FAST_TOP != 0), false, (SERL_TEAM_KREGS != 0)>(a, 0, e);
}

// attitude-task actors that do not fit the LDS-resident forward (hidden 72 / 96 ...): the actor wavefront streams the weights
__global__ void __launch_bounds__(64 * (W_TEAM_WAVES + 1)) W_NAME(serl_rollout_teams_kernel_)(RolloutArgs a)
{
  W_NAME(citw_team_stage_)(a);
  const int e = a.e0 + blockIdx.x;
  if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == W_TEAM_WAVES) W_NAME(serl_team_actor_wave_)<false, true>(a, e, false);
  else W_NAME(serl_team_episode_)<false, (SERL_TEAMS_FAST_TOP != 0), true, (SERL_TEAMS_KREGS != 0)>(a, 0, e);      // (the team's register sets fit under the streaming actor's budget)
}

// the env configurations other than the attitude task (symmetric / full observation sets, incremental control): actor weights
// streamed by the actor wavefront, observation / action widths from the descriptor
__global__ void __launch_bounds__(64 * (W_TEAM_WAVES + 1)) W_NAME(serl_rollout_teamx_kernel_)(RolloutArgs a)
{
  W_NAME(citw_team_stage_)(a);
  const int e = a.e0 + blockIdx.x;
  if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == W_TEAM_WAVES) W_NAME(serl_team_actor_wave_)<true>(a, e, false);
  else W_NAME(serl_team_episode_)<true, (SERL_TEAMS_FAST_TOP != 0), true, (SERL_TEAMS_KREGS != 0)>(a, 0, e);
}

#elif !defined(SERL_TEAM_NO_ENTRY)      // (rollout_team4_mixed.hip has ONE kernel of its own around the device functions of two code variants)
__global__ void __launch_bounds__(64 * (W_TEAM_WAVES + SERL_ACTOR_WAVES)) W_TEAMG(serl_rollout_kernel_)(RolloutArgs a)
{
#ifdef CITW_PROFILE
  if (threadIdx.x < 32) g_prof[threadIdx.x] = 0;
#endif
  W_NAME(citw_team_stage_)(a);
  if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) >= W_TEAM_WAVES) W_NAME(serl_teamg_actor_wave_)(a);
  else W_NAME(serl_teamg_episodes_)(a);
}
#endif

#if CITW_GROUP_LANES == 64 && SERL_ACTOR_WAVES == 2
#elif CITW_GROUP_LANES == 64
// dynamics only: initialize() then T calls of step(cmd[k]) per episode (test / micro-benchmark entry)
__global__ void __launch_bounds__(64 * W_TEAM_WAVES) W_NAME(serl_dyn_team_kernel_)(RolloutArgs a, const double *cmds, double *states, int T)
{
  W_NAME(citw_team_stage_)(a);
  const int wave = 0, lane = threadIdx.x & 63;
  const int e = blockIdx.x;
  CitwState s;
  double cmd[10], x[12];
  W_NAME(citw_team_reset_)(wave, s, a);
  for (int k = 0; k < T; ++k) {
#pragma unroll
    for (int i = 0; i < 10; ++i) cmd[i] = cmds[((size_t)e * T + k) * 10 + i];
    W_NAME(citw_team_step_)(wave, s, cmd, x, (unsigned)k);
    if (threadIdx.x == 0) for (int i = 0; i < 12; ++i) states[((size_t)e * T + k) * 12 + i] = x[i];
  }
}

void W_NAME(serl_launch_dyn_team_)(const RolloutArgs &a, const double *cmds, double *states, int T, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_dyn_team_kernel_), dim3(grid), dim3(64 * W_TEAM_WAVES), 0, stream, a, cmds, states, T);
}

void W_NAME(serl_launch_rollout_team_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_team_kernel_), dim3(grid), dim3(64 * (W_TEAM_WAVES + 1)), 0, stream, a);
}

void W_NAME(serl_launch_rollout_teams_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_teams_kernel_), dim3(grid), dim3(64 * (W_TEAM_WAVES + 1)), 0, stream, a);
}

void W_NAME(serl_launch_rollout_teamx_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_NAME(serl_rollout_teamx_kernel_), dim3(grid), dim3(64 * (W_TEAM_WAVES + 1)), 0, stream, a);
}
#else
#ifndef SERL_TEAM_NO_ENTRY
// `grid` workgroups, CITW_GROUPS episodes each: serl_launch_rollout_team2_<variant> / serl_launch_rollout_team4_<variant>
void W_TEAMG(serl_launch_rollout_)(const RolloutArgs &a, int grid, hipStream_t stream)
{
  hipLaunchKernelGGL(W_TEAMG(serl_rollout_kernel_), dim3(grid), dim3(64 * (W_TEAM_WAVES + SERL_ACTOR_WAVES)), 0, stream, a);
}
#endif
#undef W_TEAMG
#endif
#undef W_NAME
#undef W_TEAM_EVAL
#undef W_TEAM_WAVES
#undef W_PASTE
#undef W_PASTE2

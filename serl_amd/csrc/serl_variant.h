// serl_variant.h -- the dynamics code variant a family source is compiled for.
//
// serl_amd/build.py compiles each kernel family source (family_lane.hip, family_wave.hip, family_team.hip, ...) once per code variant
// with -DSERL_DYN=<serl_dyn_code> (include/serl_amd.h).  This header turns that number into VARIANT, the name the .inc files paste into every
// symbol they define, and into the paths of the variant's generated model evaluations (tools/dag):
//   SERL_GEN_LANE    one episode per lane (family_lane.hip)
//   SERL_GEN_WAVE    one wavefront per episode, and the look-up descriptor tables every wave and team kernel shares
//   SERL_GEN_TEAM    the evaluation partitioned over a team of seven wavefronts (family_team.hip, family_teamr.hip)
//   SERL_GEN_TEAM6   ... over six wavefronts beside two actor wavefronts (family_teams2.hip, family_team2s.hip)
//   SERL_GEN_TEAMG   the evaluation of the lane-group kernels, two or four episodes per team (family_team2.hip, family_team4.hip)
// rollout_team4_mixed.hip holds two variants in one code object and names its generated files itself.
#ifndef SERL_VARIANT_H
#define SERL_VARIANT_H

#define SERL_PASTE2(a, b) a##b
#define SERL_PASTE(a, b) SERL_PASTE2(a, b)

#if !defined(SERL_DYN)
#error "compile with -DSERL_DYN=<serl_dyn_code> (serl_amd/build.py)"
#elif SERL_DYN == 0
// builds h2000_v90, h2000_v150, h10000_v90, cg, cg_for and the Python-level fault wrappers be / jr / sa / se on top of h2000_v90
#define VARIANT nominal
#define SERL_GEN_LANE "gen/citation_nominal_lane.inc"
#define SERL_GEN_WAVE "gen/citation_nominal_wave.inc"
#define SERL_GEN_TEAM "gen/citation_nominal_team.inc"
#define SERL_GEN_TEAM6 "gen/citation_nominal_team6.inc"
// Only the nominal variant's lane-group kernels evaluate the lane-group partition of the model (gen/citation_<v>_teamg.inc); those of the other
// variants evaluate the one-episode-per-team partition.  rollout_team4_mixed.hip uses the lane-group partition for both of its variants.
#define SERL_GEN_TEAMG "gen/citation_nominal_teamg.inc"
#elif SERL_DYN == 1
// build `ice` (icing: lift-coefficient saturation, drag / lift offsets)
#define VARIANT ice
#define SERL_GEN_LANE "gen/citation_ice_lane.inc"
#define SERL_GEN_WAVE "gen/citation_ice_wave.inc"
#define SERL_GEN_TEAM "gen/citation_ice_team.inc"
#define SERL_GEN_TEAM6 "gen/citation_ice_team6.inc"
#define SERL_GEN_TEAMG SERL_GEN_TEAM
#elif SERL_DYN == 2
// build `cg_timed` (centre of gravity shifts aft when the model clock passes 20 s)
#define VARIANT cg_timed
#define SERL_GEN_LANE "gen/citation_cg_timed_lane.inc"
#define SERL_GEN_WAVE "gen/citation_cg_timed_wave.inc"
#define SERL_GEN_TEAM "gen/citation_cg_timed_team.inc"
#define SERL_GEN_TEAM6 "gen/citation_cg_timed_team6.inc"
#define SERL_GEN_TEAMG SERL_GEN_TEAM
#elif SERL_DYN == 3
// build `gust` (vertical gust of 15 ft/s when the model clock passes 20 s; live Derivative block)
#define VARIANT gust
#define SERL_GEN_LANE "gen/citation_gust_lane.inc"
#define SERL_GEN_WAVE "gen/citation_gust_wave.inc"
#define SERL_GEN_TEAM "gen/citation_gust_team.inc"
#define SERL_GEN_TEAM6 "gen/citation_gust_team6.inc"
#define SERL_GEN_TEAMG SERL_GEN_TEAM
#elif SERL_DYN == 4
// build `test` (the reference's 14th dynamics build, envs/test)
#define VARIANT test
#define SERL_GEN_LANE "gen/citation_test_lane.inc"
#define SERL_GEN_WAVE "gen/citation_test_wave.inc"
#define SERL_GEN_TEAM "gen/citation_test_team.inc"
#define SERL_GEN_TEAM6 "gen/citation_test_team6.inc"
#define SERL_GEN_TEAMG SERL_GEN_TEAM
#else
#error "SERL_DYN: not a serl_dyn_code"
#endif

#endif  // SERL_VARIANT_H

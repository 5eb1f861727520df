// family_lane.hip -- lane-per-episode rollout kernels (lanes_per_wave > 0: one episode per lane) and the step-wise vector env for one dynamics
// code variant (serl_variant.h), around the branch-free model evaluation tools/dag/codegen_lane.py generates from the DAG (~1 170 nodes
// per lane); block signals do not exist there, c->B only carries the 19 derivatives.  See rollout_variant.inc.
// (The same kernels compiled around the LIFTED model are test infrastructure: oracle/xcheck/, libserl_xcheck.so.)
#include "citation_dev.h"
#include "rollout_device.h"
#include "serl_variant.h"
#ifdef SERL_VENV_NOISE
#include "serl_rng.h"
#endif
#ifdef SERL_ROLLOUT_NOISE
#include "rollout_noise.h"
#endif
#define CIT_V(x) SERL_PASTE(SERL_PASTE(cit_, VARIANT), x)      // cit_<variant>x: the names gen/citation_<variant>_lane.inc defines
#define CIT_RO_LO_W CIT_V(_RO_LO_W)
#define CIT_RO_HI_W CIT_V(_RO_HI_W)
#define RO_BASE_W CIT_V(_RO_BASE_W)

namespace bdag {
#define CIT_B_AT(i) (c->B[(i)])
#define SERL_FLAVOUR_LDS 0
#define CIT_NO_AXES 1
// the banks live in the CALLER's stack frame: a private-segment pointer, so that the reads are scratch loads (vmcnt) and not flat loads, which also count on
// the LDS counter the table reads wait on (65 536 episodes: 219.6 -> 225.9 M env-steps/s)
#ifndef CIT_CTX_FLAT
#define CIT_DWM_PTR __attribute__((address_space(5))) double *
#define CIT_CMD_PTR const __attribute__((address_space(5))) double *
#else
#define CIT_DWM_PTR double *
#define CIT_CMD_PTR const double *
#endif
#include SERL_GEN_LANE
static_assert(CIT_RO_HI_W - CIT_RO_LO_W <= CIT_RO_LDS_WORDS, "LDS table window too small");
static_assert(8 * (CIT_RO_LDS_WORDS + CIT_V(_NSLOPE)) <= 160 * 1024, "tables + interval quotients beyond the 160 KB of LDS");
#define CIT_MODEL CIT_V(_dag_model)
#define CIT_DERIV CIT_V(_dag_derivatives)
#define CIT_STEP SERL_PASTE(cit_step_, VARIANT)
#define CIT_SLOPE_DESC CIT_V(_slope_desc)      // (precomputed x-direction quotients of the tables: rollout_variant.inc stages them, citation_leaves.h cit_lookup2d_at_s)
#define CIT_SLOPE_TABLES CIT_V(_NSLOPE_TABLES)
#define CIT_USE_HINTS CIT_V(_NSEARCH)      // (the index searches verify the previous evaluation's interval first: CitCtx.hint travels with the state)
#define CIT_DW_IN_MEMORY 1
#ifdef CIT_WITH_CMD_IN_MEMORY      // (A/B builds around gen files made with CITW_LANE_CMDMEM=1: measured slower)
#define CIT_CMD_IN_MEMORY 1
#endif
#if !defined(SERL_ROLLOUT_NOISE) && !defined(SERL_LANE_GENERAL_ACTOR)     // (family_lanern.hip: serl_rollout_noise_kernel_<v> alone -- the work-queue body has no noise instantiation; family_laneg.hip / family_lanegn.hip: the episode kernel around the general lane actor alone)
#define SERL_LANE_QUEUE 1      // (rollout_variant.inc: the work-queue kernel serl_rollout_laneq_kernel_<v> beside serl_rollout_kernel_<v>)
#endif
#define CIT_Y_IS_STATE 1      // (gen/citation_<variant>_lane.inc: `if (major) c->Y[i] = X[i]`, i < 12 -- the outputs of step() are the states in front of the integration)
#include "citation_step_dev.h"
#include "rollout_variant.inc"
#if !defined(SERL_ROLLOUT_NOISE) && !defined(SERL_LANE_GENERAL_ACTOR)
#include "venv_variant.inc"
#endif
#undef CIT_NO_AXES
#undef CIT_B_AT
#undef SERL_FLAVOUR_LDS
}  // namespace bdag

#define SERL_V(x) SERL_PASTE(x, VARIANT)
#if defined(SERL_LANE_GENERAL_ACTOR) && defined(SERL_LANE_REGROUPED_WEIGHTS)   // family_lanegt.hip / family_lanegtn.hip: that kernel over the regrouped copy of the weights (plain / with the generator), nothing else
#ifdef SERL_ROLLOUT_NOISE
void SERL_V(serl_launch_rollout_lanegt_noise_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_lanegt_noise_)(a, nz, grid, stream); }
#else
void SERL_V(serl_launch_rollout_lanegt_)(const RolloutArgs &a, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_lanegt_)(a, grid, stream); }
#endif
#elif defined(SERL_LANE_GENERAL_ACTOR)   // family_laneg.hip / family_lanegn.hip: the episode kernel around the general lane actor (plain / with the in-kernel noise generator), nothing else
#ifdef SERL_ROLLOUT_NOISE
void SERL_V(serl_launch_rollout_laneg_noise_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_laneg_noise_)(a, nz, grid, stream); }
#else
void SERL_V(serl_launch_rollout_laneg_)(const RolloutArgs &a, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_laneg_)(a, grid, stream); }
#endif
#elif defined(SERL_ROLLOUT_NOISE)   // family_lanern.hip: the episode kernel with the in-kernel noise generator, nothing else
void SERL_V(serl_launch_rollout_noise_)(const RolloutArgs &a, const serl_rollout_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_noise_)(a, nz, grid, stream); }
#elif defined(SERL_VENV_NOISE)     // family_lanenz.hip: the env kernels with the in-kernel noise generator, nothing else
#define SERL_VNZ(x) SERL_PASTE(SERL_PASTE(x, noise_), VARIANT)
void SERL_VNZ(serl_launch_venv_reset_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_VNZ(serl_launch_venv_reset_)(a, v, nz, grid, stream); }
void SERL_VNZ(serl_launch_venv_step_auto_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_VNZ(serl_launch_venv_step_auto_)(a, v, au, nz, grid, stream); }
void SERL_VNZ(serl_launch_venv_rollout_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd, const serl_venv_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_VNZ(serl_launch_venv_rollout_)(a, v, au, rd, nz, grid, stream); }
void SERL_VNZ(serl_launch_venv_rollout_general_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd, const serl_venv_noise_desc &nz, int grid, hipStream_t stream) { bdag::SERL_VNZ(serl_launch_venv_rollout_general_)(a, v, au, rd, nz, grid, stream); }
#else
void SERL_V(serl_launch_rollout_)(const RolloutArgs &a, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_)(a, grid, stream); }
void SERL_V(serl_launch_rollout_laneq_)(const RolloutArgs &a, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_rollout_laneq_)(a, grid, stream); }

void SERL_V(serl_launch_dyn_)(const RolloutArgs &a, const double *cmds, double *states, int T, int grid, hipStream_t stream)
{
  bdag::SERL_V(serl_launch_dyn_)(a, cmds, states, T, grid, stream);
}

void SERL_V(serl_launch_venv_reset_)(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_venv_reset_)(a, v, grid, stream); }
void SERL_V(serl_launch_venv_step_)(const RolloutArgs &a, const VenvArgs &v, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_venv_step_)(a, v, grid, stream); }
void SERL_V(serl_launch_venv_step_auto_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_venv_step_auto_)(a, v, au, grid, stream); }
void SERL_V(serl_launch_venv_rollout_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_venv_rollout_)(a, v, au, rd, grid, stream); }
void SERL_V(serl_launch_venv_rollout_general_)(const RolloutArgs &a, const VenvArgs &v, const serl_venv_auto_desc &au, const serl_venv_rollout_desc &rd, int grid, hipStream_t stream) { bdag::SERL_V(serl_launch_venv_rollout_general_)(a, v, au, rd, grid, stream); }
#endif

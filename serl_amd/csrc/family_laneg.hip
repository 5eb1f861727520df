// family_laneg.hip -- the lane-per-episode population rollout kernel a third time per dynamics code variant, for EVERY actor shape (kernel_hint
// SERL_KERNEL_LANEG, family SERL_FAMILY_LANEG in include/serl_amd.h): family_lane.hip's model evaluation and LDS staging around serl_wave_episodes_<v> of
// rollout_variant.inc under SERL_LANE_GENERAL_ACTOR, where every live lane runs lane_actor.h serl_actor_forward_lane_general over its own member's row
// of [members][P] instead of the hidden-32 lane actor / up to 64 wavefront-wide passes.  Kernel serl_rollout_laneg_kernel_<v>; the work-queue body, the
// dynamics-only kernel and the env kernels are not instantiated.  A unit of its own, so that the kernels of family_lane.hip compile as before.
#define SERL_LANE_GENERAL_ACTOR 1
#include "family_lane.hip"

// family_lanegt.hip -- family_laneg.hip's kernel over the REGROUPED copy of the weights (serl_rollout_regrouped; lane_weights='regrouped' in Python): every
// live lane runs lane_actor.h serl_actor_forward_lane_general_t -- the arithmetic of serl_actor_forward_lane_general, bit for bit -- over
// RolloutArgs.wt = [ceil(P / 4)][members padded to 64][4] (serl_capi.hip serl_regroup_weights_kernel in front of the launch), where 64 lanes with consecutive
// members read one run of 1 KB per load instead of 64 cache lines.  Kernel serl_rollout_lanegt_kernel_<v>, nothing else.  A unit of its own, so that the
// kernels of family_laneg.hip compile as before; the family reported stays SERL_FAMILY_LANEG.
#define SERL_LANE_GENERAL_ACTOR 1
#define SERL_LANE_REGROUPED_WEIGHTS 1
#include "family_lane.hip"

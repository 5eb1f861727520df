// family_lanern.hip -- the lane-per-episode population rollout kernel a second time per dynamics code variant, with the sensor and exploration noise drawn
// inside it (rollout_noise.h, serl_rng.h; serl_rollout_noise in include/serl_amd.h): family_lane.hip's model evaluation and LDS staging around
// serl_wave_episodes_<v> of rollout_variant.inc under SERL_ROLLOUT_NOISE.  The work-queue body, the dynamics-only kernel and the env kernels are not
// instantiated.  A unit of its own, so that the kernels of family_lane.hip compile as before.
#define SERL_ROLLOUT_NOISE 1
#include "family_lane.hip"

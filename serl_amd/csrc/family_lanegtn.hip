// family_lanegtn.hip -- family_lanegt.hip's kernel with the sensor and exploration noise drawn inside it (serl_rollout_regrouped with a noise descriptor;
// rollout_noise.h, serl_rng.h): serl_rollout_lanegt_noise_kernel_<v>, the device-noise twin, as family_lanegn.hip is family_laneg.hip's.
#define SERL_LANE_GENERAL_ACTOR 1
#define SERL_LANE_REGROUPED_WEIGHTS 1
#define SERL_ROLLOUT_NOISE 1
#include "family_lane.hip"

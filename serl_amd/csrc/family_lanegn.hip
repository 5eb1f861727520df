// family_lanegn.hip -- family_laneg.hip's kernel with the sensor and exploration noise drawn inside it (serl_rollout_noise with kernel_hint
// SERL_KERNEL_LANEG; rollout_noise.h, serl_rng.h): serl_rollout_laneg_noise_kernel_<v>, the device-noise twin, as family_lanern.hip is family_lane.hip's.
#define SERL_LANE_GENERAL_ACTOR 1
#define SERL_ROLLOUT_NOISE 1
#include "family_lane.hip"

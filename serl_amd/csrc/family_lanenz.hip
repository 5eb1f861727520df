// family_lanenz.hip -- the step-wise vector env's kernels a second time per dynamics code variant, with the sensor and exploration noise drawn inside
// them (serl_rng.h; serl_venv_reset_noise / _step_auto_noise / _rollout_noise / _rollout_general_noise in include/serl_amd.h): family_lane.hip's model
// evaluation and LDS staging around venv_variant.inc under SERL_VENV_NOISE.  A unit of its own, so that the kernels of family_lane.hip compile as before.
#define SERL_VENV_NOISE 1
#include "family_lane.hip"

// family_wavern.hip -- the one-wavefront-per-episode population rollout kernels (attitude task and the other env configurations) a second time per dynamics
// code variant, with the sensor and exploration noise drawn inside them (rollout_noise.h, serl_rng.h; serl_rollout_noise in include/serl_amd.h):
// family_wave.hip's sources around serl_wave_episode_<v> of rollout_wave.inc under SERL_ROLLOUT_NOISE.  The dynamics-only kernel is not instantiated.
// A unit of its own, so that the kernels of family_wave.hip compile as before.
#include "citation_wave.h"
#include "rollout_device.h"
#include "serl_variant.h"
#include "rollout_noise.h"
#include SERL_GEN_WAVE
#define SERL_ROLLOUT_NOISE 1
#include "rollout_wave.inc"

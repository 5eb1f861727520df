// family_wave.hip -- wave-cooperative rollout kernels (one wavefront per episode) for one dynamics code variant (serl_variant.h).
// See rollout_wave.inc.
#include "citation_wave.h"
#include "rollout_device.h"
#include "serl_variant.h"
#include SERL_GEN_WAVE
#include "rollout_wave.inc"

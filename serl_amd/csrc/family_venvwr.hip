// family_venvwr.hip -- CitationVecEnv.rollout with one wavefront per env (venv_wave_rollout.inc) for one dynamics code variant (serl_variant.h): the wave
// family's model evaluation, LDS staging and ODE5 step (family_wave.hip's sources), the state load / store and env glue of venv_wave.inc, the wave-cooperative
// actor of rollout_device.h, and the same kernel a second time with the in-kernel noise generator (SERL_VENV_NOISE).  A unit of its own, so that the kernels
// of family_venvw.hip, family_wave.hip and family_lane.hip compile as before.
#include "citation_wave.h"
#include "rollout_device.h"
#include "serl_variant.h"
#include "serl_rng.h"
#include SERL_GEN_WAVE
// rollout_wave.inc for citw_stage_<v> / citw_step_<v> / citw_reset_<v>; its rollout kernels and launchers belong to family_wave.hip
#define SERL_WAVE_STEP_ONLY 1
#include "rollout_wave.inc"
// venv_wave.inc for serl_venvw_load_<v> / _store_<v> / _init_<v> and the env glue; its kernels and launchers belong to family_venvw.hip
#define SERL_VENVW_HELPERS_ONLY 1

#include "venv_wave.inc"
#include "venv_wave_rollout.inc"
#define SERL_VENV_NOISE 1
#include "venv_wave.inc"
#include "venv_wave_rollout.inc"

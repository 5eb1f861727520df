// family_venvw.hip -- the step-wise vector env with one wavefront per env (venv_wave.inc) for one dynamics code variant (serl_variant.h): the wave family's
// model evaluation, LDS staging and ODE5 step (family_wave.hip's sources) around the env's reset / step / auto-reset step, and the same kernels a second time
// with the in-kernel noise generator (SERL_VENV_NOISE).  A unit of its own, so that the kernels of family_wave.hip and family_lane.hip compile as before.
#include "citation_wave.h"
#include "rollout_device.h"
#include "serl_variant.h"
#include "serl_rng.h"
#include SERL_GEN_WAVE
// rollout_wave.inc for citw_stage_<v> / citw_step_<v> / citw_reset_<v>; its rollout kernels and launchers belong to family_wave.hip
#define SERL_WAVE_STEP_ONLY 1
#include "rollout_wave.inc"

#include "venv_wave.inc"
#define SERL_VENV_NOISE 1
#include "venv_wave.inc"

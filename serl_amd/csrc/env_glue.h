// env_glue.h -- the statements of the env step around the dynamics call (CitationEnv.reset / .step, envs/phlabenv.py:401-482, and the
// actuator-fault wrappers envs/{be,jr,sa,se}/citation.py:71-79) that every rollout and env kernel used to write out again: the no-fault row,
// the fault row on top of a command, the sensor add, the observation.  Small pure functions over values and
// caller-owned arrays: no LDS, no lane logic, no memory layout beyond the pointers they are handed; the kernels built over them have the
// code objects they had with the statements written out.  Action scaling, the noise-row lookups, reward / cost / termination and the row writers are still the
// kernels' own text.  Nothing here relies on FMA contraction either way, and the file compiles as plain C++ for the
// host (tests/tools/env_glue_host.cpp).
//
// NOT shared with the checkers: oracle/rollout_ref.c and tests/env_glue.py keep readings of the reference of their own and must not
// include this file -- the bit-for-bit tests of the kernels against them would compare the text with itself.
#pragma once
#include "../../include/serl_amd.h"
#ifdef __HIPCC__
#define SERL_GLUE_FN __device__ __forceinline__
#else
#define SERL_GLUE_FN inline
#endif

static SERL_GLUE_FN double serl_clip(double v, double lo, double hi)
{
  return v < lo ? lo : (v > hi ? hi : v);
}

// ---- the actuator-fault row (include/serl_amd.h serl_fault_row); the nominal row: gain 1, clips at infinity, no jam
static SERL_GLUE_FN serl_fault_row serl_fault_none()
{
  return serl_fault_row{1.0, __builtin_inf(), __builtin_inf(), 0.0, 0.0, 0, 0, 0};
}
// what the plant sees of the env's deflections u: gain, clip, jam.  c: the first three words of cmd[10], or of a hand-over (LDS, mailbox)
template <class C>
static SERL_GLUE_FN void serl_fault_apply(const serl_fault_row &f, const double (&u)[3], C &&c)
{
  c[0] = serl_clip(u[0] * f.elev_gain, -f.elev_clip, f.elev_clip);
  c[1] = serl_clip(u[1], -f.ail_clip, f.ail_clip);
  c[2] = (f.rudder_jam_on != 0.0) ? f.rudder_jam : u[2];
}

// the sensor model on top of what step() returned (envs/noise/citation.py:71-82): p q r alpha beta phi theta; the plant state stays clean
static SERL_GLUE_FN void serl_sensor_add(double (&x)[12], const double *sn)
{
  x[0] += sn[0]; x[1] += sn[1]; x[2] += sn[2]; x[4] += sn[3]; x[5] += sn[4]; x[6] += sn[5]; x[7] += sn[6];
}

// ---- observation = [error (A), observed states, last_u (A, incremental only)] (phlabenv.py:84-97,415-428,462-466): S entries of o
static SERL_GLUE_FN void serl_write_obs(int cfg, bool incr, const double (&err)[3], const double (&x)[12], const double (&u)[3], double *o)
{
  if (cfg == SERL_ENV_SYMMETRIC) {
    o[0] = err[0]; o[1] = x[1];
    if (incr) o[2] = u[0];
  } else if (cfg == SERL_ENV_FULL) {
    o[0] = err[0]; o[1] = err[1]; o[2] = err[2];
#pragma unroll
    for (int i = 0; i < 10; ++i) o[3 + i] = x[i];
    if (incr) { o[13] = u[0]; o[14] = u[1]; o[15] = u[2]; }
  } else {
    o[0] = err[0]; o[1] = err[1]; o[2] = err[2];
    o[3] = x[0]; o[4] = x[1]; o[5] = x[2]; o[6] = x[4];
    if (incr) { o[7] = u[0]; o[8] = u[1]; o[9] = u[2]; }
  }
}

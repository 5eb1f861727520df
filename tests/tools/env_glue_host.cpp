// env_glue_host.cpp -- serl_amd/csrc/env_glue.h compiled for the host (g++ -O2 -ffp-contract=off) and driven through flown episodes.
// tests/test_env_glue_header_host.py writes records of tests/env_glue.py as f64 words; this program runs the header over every step and
// writes what it computes, again as f64 words.
//   env_glue_host <in> <out>
// in:   n_scenarios, then per scenario  cfg incr n fault[8], then per step err[3] x[12] u[3];  then n_sensor, and per case x[12] sn[7]
// out:  per scenario  the no-fault row[8], cmd0[3] (reset()'s command: u = 0), per step cmd[3] obs[16];  per sensor case x[12]
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "env_glue.h"

static std::vector<double> in;
static size_t pos = 0;
static double next() { if (pos >= in.size()) { fprintf(stderr, "input too short\n"); exit(2); } return in[pos++]; }

int main(int argc, char **argv)
{
  if (argc != 3) return 2;
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  double w;
  while (fread(&w, sizeof w, 1, fi) == 1) in.push_back(w);
  fclose(fi);
  std::vector<double> out;
  const int ns = (int)next();
  for (int sc = 0; sc < ns; ++sc) {
    const int cfg = (int)next(), incr = (int)next(), n = (int)next();
    double fw[8];
    for (int i = 0; i < 8; ++i) fw[i] = next();
    const serl_fault_row f = {fw[0], fw[1], fw[2], fw[3], fw[4], fw[5], fw[6], fw[7]};
    const serl_fault_row none = serl_fault_none();
    const double *nw = &none.elev_gain;
    for (int i = 0; i < 8; ++i) out.push_back(nw[i]);
    const double zero[3] = {0.0, 0.0, 0.0};
    double cmd[10] = {0};
    serl_fault_apply(f, zero, cmd);
    for (int i = 0; i < 3; ++i) out.push_back(cmd[i]);
    for (int k = 0; k < n; ++k) {
      double err[3], x[12], u[3], obs[16] = {0};
      for (int i = 0; i < 3; ++i) err[i] = next();
      for (int i = 0; i < 12; ++i) x[i] = next();
      for (int i = 0; i < 3; ++i) u[i] = next();
      serl_fault_apply(f, u, cmd);
      serl_write_obs(cfg, incr != 0, err, x, u, obs);
      for (int i = 0; i < 3; ++i) out.push_back(cmd[i]);
      for (int i = 0; i < 16; ++i) out.push_back(obs[i]);
    }
  }
  const int nsens = (int)next();
  for (int c = 0; c < nsens; ++c) {
    double x[12], sn[7];
    for (int i = 0; i < 12; ++i) x[i] = next();
    for (int i = 0; i < 7; ++i) sn[i] = next();
    serl_sensor_add(x, sn);
    for (int i = 0; i < 12; ++i) out.push_back(x[i]);
  }
  FILE *fo = fopen(argv[2], "wb");
  if (!fo) return 2;
  fwrite(out.data(), sizeof(double), out.size(), fo);
  fclose(fo);
  return 0;
}

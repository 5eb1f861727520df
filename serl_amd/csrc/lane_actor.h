// lane_actor.h -- the lane-per-episode actors (included by rollout_device.h): the whole forward pass of a lane's own actor in the lane's registers
// (hidden 32) or private memory (every shape), over the member's row of [members][P] or over the regrouped copy [P / 4][members][4].
#pragma once

// ---- one episode per LANE (rollout_variant.inc, round 6): the whole forward pass of the lane's own actor in the lane's registers ----------------------
// The lane-per-episode kernels ran the wave-cooperative pass once per live lane -- 64 passes of ~9 k cycles per wavefront and env step, a quarter of a
// step that already wastes no lane on the dynamics.  Here every lane walks ITS member's weights (global memory, L1 / L2: the rows of one member are
// read by its num_evals lanes together) and keeps the two layers it needs in 64 registers.  Rows are computed eight at a time in a rolled loop and
// shifted into place (static register indices, 3 KB of code per layer instead of 13), the arithmetic is the scalar statement of the ABI (oracle/rollout_ref.c
// actor_forward: dot4, tree_sum): four interleaved fma partial sums over ascending j, bias + ((p0 + p1) + (p2 + p3)); LayerNorm sums as a balanced pairwise
// tree per block of 16 rows, the blocks added in order.  H = 32, 7 observations, 3 actions (the SERL50 shape); other shapes keep the cooperative pass.
static __device__ __forceinline__ bool serl_lane_actor_ok(const serl_rollout_desc &dd)
{
  return dd.hidden == 32 && dd.state_dim == 7 && dd.action_dim == 3;
}
static __device__ __forceinline__ float serl_tree16_regs(const float (&x)[32], const int o)
{
  const float a0 = x[o + 0] + x[o + 1], a1 = x[o + 2] + x[o + 3], a2 = x[o + 4] + x[o + 5], a3 = x[o + 6] + x[o + 7];
  const float a4 = x[o + 8] + x[o + 9], a5 = x[o + 10] + x[o + 11], a6 = x[o + 12] + x[o + 13], a7 = x[o + 14] + x[o + 15];
  const float b0 = a0 + a1, b1 = a2 + a3, b2 = a4 + a5, b3 = a6 + a7;
  const float c0 = b0 + b1, c1 = b2 + b3;
  return c0 + c1;
}
static __device__ __forceinline__ void serl_shift8(float (&h)[32], const float (&t)[8])
{
#pragma unroll
  for (int i = 0; i < 24; ++i) h[i] = h[i + 8];
#pragma unroll
  for (int i = 0; i < 8; ++i) h[24 + i] = t[i];
}
static __device__ void serl_actor_forward_lane32(const serl_rollout_desc &dd, const float *w_lane, const float (&obs)[7], float (&act_out)[3])
{
  constexpr int H = 32;
  const int L = __builtin_amdgcn_readfirstlane(dd.num_layers), act = __builtin_amdgcn_readfirstlane(dd.activation);
  serl_gptr W = (serl_gptr)w_lane;                      // this lane's member
  float h0[32], h1[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) { h0[i] = 0.0f; h1[i] = 0.0f; }
  // ---- Linear(7, H) act
  {
    serl_gptr b0 = W + H * 7;
#pragma nounroll
    for (int c = 0; c < 4; ++c) {
      float t[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        serl_gptr row = W + (8 * c + r) * 7;
        float wv[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) wv[j] = row[j];
        t[r] = serl_act(serl_dot7(b0[8 * c + r], wv, obs), act);
      }
      serl_shift8(h0, t);
    }
  }
  const size_t lstride = (size_t)H * H + 3 * (size_t)H;
  serl_gptr hid = W + (size_t)H * 7 + H;
#pragma nounroll
  for (int l = 0; l < L; ++l) {
    serl_gptr Wl = hid + (size_t)l * lstride, bl = Wl + (size_t)H * H;
    // four rows at a time in two register buffers: the NEXT four rows' weights are in flight while these are summed (one L2 round trip would otherwise stand
    // in front of every chunk on a wavefront that has its SIMD to itself); the chunk loop is unrolled by two so that the buffers swap without copies
    serl_v4f wa[4][8], wb[4][8];
    float ba[4], bb[4];
    auto fetch = [&](serl_v4f (&wv)[4][8], float (&bv)[4], const int c) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        serl_gptr4 row = (serl_gptr4)(Wl + (size_t)(4 * c + r) * H);
#pragma unroll
        for (int q = 0; q < 8; ++q) wv[r][q] = row[q];
        bv[r] = bl[4 * c + r];
      }
    };
    auto rows4 = [&](const serl_v4f (&wv)[4][8], const float (&bv)[4]) {
      float t[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          p0 = __builtin_fmaf(wv[r][q].x, h0[4 * q], p0); p1 = __builtin_fmaf(wv[r][q].y, h0[4 * q + 1], p1);
          p2 = __builtin_fmaf(wv[r][q].z, h0[4 * q + 2], p2); p3 = __builtin_fmaf(wv[r][q].w, h0[4 * q + 3], p3);
        }
        t[r] = bv[r] + ((p0 + p1) + (p2 + p3));
      }
#pragma unroll
      for (int i = 0; i < 28; ++i) h1[i] = h1[i + 4];
#pragma unroll
      for (int i = 0; i < 4; ++i) h1[28 + i] = t[i];
    };
    fetch(wa, ba, 0);
#pragma nounroll
    for (int c = 0; c < 8; c += 2) {
      fetch(wb, bb, c + 1);
      rows4(wa, ba);
      if (c + 2 < 8) fetch(wa, ba, c + 2);
      rows4(wb, bb);
    }
    const float mean = (serl_tree16_regs(h1, 0) + serl_tree16_regs(h1, 16)) / (float)H;
    float d2[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) { const float dl = h1[i] - mean; d2[i] = dl * dl; }
    const float var = serl_tree16_regs(d2, 0) + serl_tree16_regs(d2, 16);
    const float den = sqrtf(var / (float)(H - 1)) + 1e-6f;
#pragma nounroll
    for (int c = 0; c < 4; ++c) {      // rows 8 c .. 8 c + 7 sit in h1[0 .. 7] (shifted as they are consumed); the new layer is shifted into h0
      float t[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) t[r] = serl_act(bl[H + 8 * c + r] * (h1[r] - mean) / den + bl[2 * H + 8 * c + r], act);
      float z[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) z[r] = 0.0f;
      serl_shift8(h1, z);
      serl_shift8(h0, t);
    }
  }
  // ---- Linear(H, 3) tanh
  serl_gptr outl = hid + (size_t)L * lstride;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    serl_gptr4 row = (serl_gptr4)(outl + (size_t)i * H);
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const serl_v4f wv = row[q];
      p0 = __builtin_fmaf(wv.x, h0[4 * q], p0); p1 = __builtin_fmaf(wv.y, h0[4 * q + 1], p1);
      p2 = __builtin_fmaf(wv.z, h0[4 * q + 2], p2); p3 = __builtin_fmaf(wv.w, h0[4 * q + 3], p3);
    }
    act_out[i] = det_tanhf((outl + (size_t)3 * H)[i] + ((p0 + p1) + (p2 + p3)));
  }
}

// ---- one env per LANE, every actor shape the ABI takes (venv_variant.inc serl_venv_rollout_general_kernel_<v>) -----------------------------------------
// hidden a multiple of 4 in 4 .. 128, 0 .. 16 hidden layers, every activation, up to 16 observations, 1 or 3 actions.  The lane kernels have no LDS left
// (the tables take 163 800 of 163 840 B) and 2 x 128 activations are no register set, so the two activation vectors live in PRIVATE memory, indexed at
// run time: scratch is lane-interleaved, the index is wave-uniform, so every access is one coalesced line per wavefront.  Four output rows per pass over the
// previous layer -- one 16-byte load of h[j .. j + 3] feeds 16 multiply-adds -- and hidden / output rows read with 16-byte loads: every tensor offset of
// the packed layout is a multiple of four floats when H % 4 == 0.  The layer-0 rows of S floats are not aligned and are read float by float.  The arithmetic
// is the scalar statement of the ABI (oracle/rollout_ref.c actor_forward: dot4, tree_sum), as in serl_actor_forward_lane32: four interleaved fma partial sums
// p[j & 3] over ascending j, bias + ((p0 + p1) + (p2 + p3)); LayerNorm sums as a balanced pairwise tree per block of 16 rows, zero padded, the blocks added in
// order.  H, L, S, A and the activation are wave-uniform (the descriptor), the weights are the lane's own member's.
static __device__ __forceinline__ float serl_tree16_v4(const serl_v4f &a, const serl_v4f &b, const serl_v4f &c, const serl_v4f &d)
{
  const float a0 = a.x + a.y, a1 = a.z + a.w, a2 = b.x + b.y, a3 = b.z + b.w;
  const float a4 = c.x + c.y, a5 = c.z + c.w, a6 = d.x + d.y, a7 = d.z + d.w;
  const float b0 = a0 + a1, b1 = a2 + a3, b2 = a4 + a5, b3 = a6 + a7;
  const float c0 = b0 + b1, c1 = b2 + b3;
  return c0 + c1;
}
// R rows of H columns from `rows` (row stride H floats, 16-byte aligned) against h[0 .. H): out[r] = (p0 + p1) + (p2 + p3), the bias is the caller's.
// Sixteen columns per trip: the 4 R + 4 loads of a trip are issued together (a lone wavefront pays one memory round trip per trip, not one per group of
// four columns); the groups beyond H -- H % 16 != 0 -- load the last group again (an address inside the row) and are left out of the sums.
template <int R>
static __device__ __forceinline__ void serl_lane_rows(serl_gptr rows, const int H, const float *h, float (&out)[R])
{
  float p[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) { p[r][0] = 0.0f; p[r][1] = 0.0f; p[r][2] = 0.0f; p[r][3] = 0.0f; }
#pragma nounroll
  for (int j = 0; j < H; j += 16) {
    serl_v4f hv[4], wv[R][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int jq = j + 4 * q < H ? j + 4 * q : H - 4;
      hv[q] = *(const serl_v4f *)(h + jq);
#pragma unroll
      for (int r = 0; r < R; ++r) wv[r][q] = *(serl_gptr4)(rows + (size_t)r * H + jq);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (j + 4 * q < H) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          p[r][0] = __builtin_fmaf(wv[r][q].x, hv[q].x, p[r][0]); p[r][1] = __builtin_fmaf(wv[r][q].y, hv[q].y, p[r][1]);
          p[r][2] = __builtin_fmaf(wv[r][q].z, hv[q].z, p[r][2]); p[r][3] = __builtin_fmaf(wv[r][q].w, hv[q].w, p[r][3]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) out[r] = (p[r][0] + p[r][1]) + (p[r][2] + p[r][3]);
}
static __device__ void serl_actor_forward_lane_general(const serl_rollout_desc &dd, const float *w_lane, const float (&obs)[16], float (&act_out)[3])
{
  const int H = __builtin_amdgcn_readfirstlane(dd.hidden), L = __builtin_amdgcn_readfirstlane(dd.num_layers);
  const int S = __builtin_amdgcn_readfirstlane(dd.state_dim), A = __builtin_amdgcn_readfirstlane(dd.action_dim);
  const int act = __builtin_amdgcn_readfirstlane(dd.activation);
  serl_gptr W = (serl_gptr)w_lane;                      // this lane's member
  __attribute__((aligned(16))) float hbuf[2][SERL_MAX_HIDDEN];
  float *h0 = hbuf[0], *h1 = hbuf[1];
  // ---- Linear(S, H) act
  {
    serl_gptr b0 = W + (size_t)H * S;
#pragma nounroll
    for (int i = 0; i < H; i += 4) {
      float p[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[r][0] = 0.0f; p[r][1] = 0.0f; p[r][2] = 0.0f; p[r][3] = 0.0f; }
      serl_gptr row = W + (size_t)i * S;
      float wv[4][16];      // (all loads of the four rows first; the columns beyond S read column S - 1 again and are left out of the sums)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int jc = j < S ? j : S - 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) wv[r][j] = row[r * S + jc];
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (j < S) {
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r][j & 3] = __builtin_fmaf(wv[r][j], obs[j], p[r][j & 3]);
        }
      }
      const serl_v4f bv = *(serl_gptr4)(b0 + i);
      serl_v4f t;
      t.x = serl_act(bv.x + ((p[0][0] + p[0][1]) + (p[0][2] + p[0][3])), act);
      t.y = serl_act(bv.y + ((p[1][0] + p[1][1]) + (p[1][2] + p[1][3])), act);
      t.z = serl_act(bv.z + ((p[2][0] + p[2][1]) + (p[2][2] + p[2][3])), act);
      t.w = serl_act(bv.w + ((p[3][0] + p[3][1]) + (p[3][2] + p[3][3])), act);
      *(serl_v4f *)(h0 + i) = t;
    }
  }
  const size_t lstride = (size_t)H * H + 3 * (size_t)H;
  serl_gptr hid = W + (size_t)H * S + H;
  const serl_v4f zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma nounroll
  for (int l = 0; l < L; ++l) {
    serl_gptr Wl = hid + (size_t)l * lstride, bl = Wl + (size_t)H * H;
#pragma nounroll
    for (int i = 0; i < H; i += 4) {
      float t[4];
      serl_lane_rows<4>(Wl + (size_t)i * H, H, h0, t);
      const serl_v4f bv = *(serl_gptr4)(bl + i);
      serl_v4f o;
      o.x = bv.x + t[0]; o.y = bv.y + t[1]; o.z = bv.z + t[2]; o.w = bv.w + t[3];
      *(serl_v4f *)(h1 + i) = o;
    }
    // LayerNorm: the two sums block by block of 16 rows (the last block zero padded: H % 4 == 0, so whole groups of four)
    float sum = 0.0f;
#pragma nounroll
    for (int b = 0; b < H; b += 16) {
      serl_v4f v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = b + 4 * q < H ? *(const serl_v4f *)(h1 + b + 4 * q) : zero4;
      const float t = serl_tree16_v4(v[0], v[1], v[2], v[3]);
      sum = b == 0 ? t : sum + t;
    }
    const float mean = sum / (float)H;
    float var = 0.0f;
#pragma nounroll
    for (int b = 0; b < H; b += 16) {
      serl_v4f v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = zero4;
        if (b + 4 * q < H) {
          const serl_v4f hv = *(const serl_v4f *)(h1 + b + 4 * q);
          const float d0 = hv.x - mean, d1 = hv.y - mean, d2 = hv.z - mean, d3 = hv.w - mean;
          v[q].x = d0 * d0; v[q].y = d1 * d1; v[q].z = d2 * d2; v[q].w = d3 * d3;
        }
      }
      const float t = serl_tree16_v4(v[0], v[1], v[2], v[3]);
      var = b == 0 ? t : var + t;
    }
    const float den = sqrtf(var / (float)(H - 1)) + 1e-6f;
#pragma nounroll
    for (int i = 0; i < H; i += 4) {
      const serl_v4f hv = *(const serl_v4f *)(h1 + i);
      const serl_v4f gm = *(serl_gptr4)(bl + H + i), bt = *(serl_gptr4)(bl + 2 * H + i);
      serl_v4f t;
      t.x = serl_act(gm.x * (hv.x - mean) / den + bt.x, act);
      t.y = serl_act(gm.y * (hv.y - mean) / den + bt.y, act);
      t.z = serl_act(gm.z * (hv.z - mean) / den + bt.z, act);
      t.w = serl_act(gm.w * (hv.w - mean) / den + bt.w, act);
      *(serl_v4f *)(h0 + i) = t;
    }
  }
  // ---- Linear(H, A) tanh
  serl_gptr outl = hid + (size_t)L * lstride;
#pragma nounroll
  for (int i = 0; i < A; ++i) {
    float t[1];
    serl_lane_rows<1>(outl + (size_t)i * H, H, h0, t);
    const float r = det_tanhf((outl + (size_t)A * H)[i] + t[0]);
    if (i == 0) act_out[0] = r; else if (i == 1) act_out[1] = r; else act_out[2] = r;
  }
}

// The same forward pass over the REGROUPED weights (RolloutArgs.wt: [ceil(P / 4)][members][4], serl_capi.hip serl_regroup_weights_kernel).  A lane that walks
// its member's row of [members][P] asks the texture path for 64 different cache lines per load instruction (a row of 32 weights is one line: four rows in
// flight x 64 lanes are the whole 32 KB L1), and the forward pass -- 3.7 k fma per lane -- cost 0.23 M cycles per wavefront and env step.  Here parameter
// group g of the members of 64 consecutive episodes is one run of 1 KB when the episodes' members are consecutive (evaluate_pop: member = episode / num_evals
// or episode mod members), every load instruction a wave-uniform base (group g) + the lane's member x 16 B.  Every parameter offset of the packed layout is
// a multiple of four for H = 32 (224, 256, 1120 per hidden layer), so a group never straddles two tensors.  Same arithmetic, same order: bit-identical.
static __device__ void serl_actor_forward_lane32_t(const serl_rollout_desc &dd, const float *wt, const int wt_members, const unsigned member, const float (&obs)[7],
                                                   float (&act_out)[3])
{
  constexpr int H = 32;
  const int L = __builtin_amdgcn_readfirstlane(dd.num_layers), act = __builtin_amdgcn_readfirstlane(dd.activation);
  typedef const __attribute__((address_space(1))) char *gbytes;
  const gbytes base = (gbytes)wt;
  const unsigned gs = (unsigned)__builtin_amdgcn_readfirstlane(wt_members) * 16u;      // bytes from group g to group g + 1 (wave-uniform)
  const unsigned moff = member * 16u;
  // a load = wave-uniform 64-bit address of the group (SGPR pair: global_load_dwordx4 v, v_off, s[..]) + the lane's 32-bit offset member x 16 (serl_capi.hip regroups at most 2^22 members)
  auto at = [&](const int g0) -> gbytes { return base + (size_t)g0 * (size_t)gs; };
  auto ld4 = [&](const gbytes gp, const int k) -> serl_v4f { const gbytes q = gp + (size_t)((unsigned)k * gs); return *(serl_gptr4)(q + moff); };
  float h0[32], h1[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) { h0[i] = 0.0f; h1[i] = 0.0f; }
  // ---- Linear(7, H) act: eight rows = 56 weights = 14 groups at a time
  {
#pragma nounroll
    for (int c = 0; c < 4; ++c) {
      float wf[56], bf[8];
      const gbytes gw = at(14 * c), gb = at(56 + 2 * c);
#pragma unroll
      for (int g = 0; g < 14; ++g) { const serl_v4f v = ld4(gw, g); wf[4 * g] = v.x; wf[4 * g + 1] = v.y; wf[4 * g + 2] = v.z; wf[4 * g + 3] = v.w; }
#pragma unroll
      for (int g = 0; g < 2; ++g) { const serl_v4f v = ld4(gb, g); bf[4 * g] = v.x; bf[4 * g + 1] = v.y; bf[4 * g + 2] = v.z; bf[4 * g + 3] = v.w; }
      float t[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float wv[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) wv[j] = wf[7 * r + j];
        t[r] = serl_act(serl_dot7(bf[r], wv, obs), act);
      }
      serl_shift8(h0, t);
    }
  }
  constexpr int lgroups = (H * H + 3 * H) / 4, hid = (H * 7 + H) / 4;      // groups per hidden layer, first group of the first hidden layer
#pragma nounroll
  for (int l = 0; l < L; ++l) {
    const int Wl = hid + l * lgroups, bl = Wl + H * H / 4;       // groups: weights (row r = groups 8 r .. 8 r + 7), then bias / gamma / beta (8 groups each)
    // (a ring of eight ROW buffers with the loads issued seven rows ahead -- 56 loads in flight instead of 33 -- measured 142 against 179 M env-steps/s: the ring
    // costs 200 more spill slots, and a scratch reload in the loop waits for every weight load issued before it: vmcnt counts in order)
    serl_v4f wa[4][8], wb[4][8], ba, bb;
    auto fetch = [&](serl_v4f (&wv)[4][8], serl_v4f &bv, const int c) {
      const gbytes gp = at(Wl + 32 * c);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 8; ++q) wv[r][q] = ld4(gp, r * 8 + q);
      bv = ld4(at(bl + c), 0);
    };
    auto rows4 = [&](const serl_v4f (&wv)[4][8], const serl_v4f &bv) {
      const float bvs[4] = {bv.x, bv.y, bv.z, bv.w};
      float t[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          p0 = __builtin_fmaf(wv[r][q].x, h0[4 * q], p0); p1 = __builtin_fmaf(wv[r][q].y, h0[4 * q + 1], p1);
          p2 = __builtin_fmaf(wv[r][q].z, h0[4 * q + 2], p2); p3 = __builtin_fmaf(wv[r][q].w, h0[4 * q + 3], p3);
        }
        t[r] = bvs[r] + ((p0 + p1) + (p2 + p3));
      }
#pragma unroll
      for (int i = 0; i < 28; ++i) h1[i] = h1[i + 4];
#pragma unroll
      for (int i = 0; i < 4; ++i) h1[28 + i] = t[i];
    };
    fetch(wa, ba, 0);
#pragma nounroll
    for (int c = 0; c < 8; c += 2) {
      fetch(wb, bb, c + 1);
      rows4(wa, ba);
      if (c + 2 < 8) fetch(wa, ba, c + 2);
      rows4(wb, bb);
    }
    const float mean = (serl_tree16_regs(h1, 0) + serl_tree16_regs(h1, 16)) / (float)H;
    float d2[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) { const float dl = h1[i] - mean; d2[i] = dl * dl; }
    const float var = serl_tree16_regs(d2, 0) + serl_tree16_regs(d2, 16);
    const float den = sqrtf(var / (float)(H - 1)) + 1e-6f;
#pragma nounroll
    for (int c = 0; c < 4; ++c) {      // rows 8 c .. 8 c + 7 sit in h1[0 .. 7] (shifted as they are consumed); the new layer is shifted into h0
      float gm[8], bt[8];
      const gbytes gg = at(bl + 8 + 2 * c);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const serl_v4f v = ld4(gg, g), u = ld4(gg, 8 + g);
        gm[4 * g] = v.x; gm[4 * g + 1] = v.y; gm[4 * g + 2] = v.z; gm[4 * g + 3] = v.w;
        bt[4 * g] = u.x; bt[4 * g + 1] = u.y; bt[4 * g + 2] = u.z; bt[4 * g + 3] = u.w;
      }
      float t[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) t[r] = serl_act(gm[r] * (h1[r] - mean) / den + bt[r], act);
      float z[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) z[r] = 0.0f;
      serl_shift8(h1, z);
      serl_shift8(h0, t);
    }
  }
  // ---- Linear(H, 3) tanh
  const gbytes go = at(hid + L * lgroups);
  const serl_v4f ob = ld4(go, 3 * H / 4);
  const float obs3[3] = {ob.x, ob.y, ob.z};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, p3 = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const serl_v4f wv = ld4(go, i * 8 + q);
      p0 = __builtin_fmaf(wv.x, h0[4 * q], p0); p1 = __builtin_fmaf(wv.y, h0[4 * q + 1], p1);
      p2 = __builtin_fmaf(wv.z, h0[4 * q + 2], p2); p3 = __builtin_fmaf(wv.w, h0[4 * q + 3], p3);
    }
    act_out[i] = det_tanhf(obs3[i] + ((p0 + p1) + (p2 + p3)));
  }
}

// ---- serl_actor_forward_lane_general over the REGROUPED weights (family_lanegt.hip / family_lanegtn.hip: serl_rollout_regrouped) ------------------------
// Every actor shape of the lane population kernel (state_dim 7, action_dim 3, hidden a multiple of 4 in 4 .. 128, 0 .. 16 hidden layers) with the addresses of
// serl_actor_forward_lane32_t: parameter p of member m lives at wt[((p >> 2) * wt_members + m) * 4 + (p & 3)], every load is one dwordx4 at a wave-uniform
// 64-bit group base (an SGPR pair) + the lane's 32-bit offset member x 16 B, so the 64 lanes of a wavefront whose members are consecutive read one run of
// 1 KB where the row version asks for 64 cache lines.  The group stride wt_members x 16 B is multiplied on the scalar side in 64 bits: ceil(P / 4) x mpad x
// 16 B is 7.75 GB for 65 536 members of 96 x 3.
// The layout property this rests on (tests/test_rollout_lanegt_host.py checks it for every shape): with S = 7, A = 3 and H % 4 == 0 every tensor of the packed
// layout starts at a multiple of four floats -- 7 H, 7 H + H = 8 H, H x H + 3 H per hidden layer, rows of H, 3 H in front of the output bias -- so no group
// straddles two tensors or two rows of H; a block of four first-layer rows is 28 floats = exactly seven groups (rows i .. i + 3 start at float 28 (i / 4)),
// which turns the row version's scalar row[r * S + jc] loads into seven dwordx4 loads per block; and the output bias is elements 0 .. 2 of the last group,
// whose fourth element serl_regroup_weights_kernel writes as zero (P = 4 g + 3).
// The arithmetic is serl_actor_forward_lane_general's, operation for operation and in the same order -- p[r][j & 3] fma chains over ascending j in the first
// layer, serl_lane_rows' four partial sums per row with the H - 4 clamp, the zero-padded 16-wide LayerNorm trees, gm * (h - mean) / den + bt, det_tanhf --:
// bit-identical.  A trip of serl_lane_rows_t issues the same 4 R + 4 loads together as a trip of serl_lane_rows.
typedef const __attribute__((address_space(1))) char *serl_gbytes;
// a group base as an SGPR pair: the two readfirstlanes keep the 64-bit group arithmetic (group index x stride) on the scalar side and apart from the lane's
// offset -- without them the compiler adds the offset to the base first and multiplies per lane --, so that the load is global_load_dwordx4 v, v_off, s[base:base+1]
static __device__ __forceinline__ serl_gbytes serl_group_base(const serl_gbytes p)
{
  const uint64_t v = (uint64_t)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return (serl_gbytes)(((uint64_t)hi << 32) | (uint64_t)lo);
}
// the lane's 32-bit offset, handed to the loads of ONE basic block: instruction selection folds base + zext(offset) into the load's address only where it
// sees the zero-extension in the block of the load, and a loop-invariant one is hoisted out of every loop (the empty statement pins it where it stands)
static __device__ __forceinline__ unsigned serl_lane_offset(unsigned moff)
{
  asm volatile("" : "+v"(moff));
  return moff;
}
template <int R>
static __device__ __forceinline__ void serl_lane_rows_t(const serl_gbytes rows, const uint64_t gs, const unsigned moff, const int H, const float *h, float (&out)[R])
{
  // rows: the group base of row 0's first group; row r's group q lies (r * H / 4 + q) groups on
  const int Hq = H >> 2;
  float p[R][4];
#pragma unroll
  for (int r = 0; r < R; ++r) { p[r][0] = 0.0f; p[r][1] = 0.0f; p[r][2] = 0.0f; p[r][3] = 0.0f; }
#pragma nounroll
  for (int j = 0; j < H; j += 16) {
    serl_v4f hv[4], wv[R][4];
    const unsigned mo = serl_lane_offset(moff);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int jq = j + 4 * q < H ? j + 4 * q : H - 4;
      hv[q] = *(const serl_v4f *)(h + jq);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const serl_gbytes gp = serl_group_base(rows + (uint64_t)(unsigned)(r * Hq + (jq >> 2)) * gs);      // (wave-uniform: scalar 64-bit)
        wv[r][q] = *(serl_gptr4)(gp + mo);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (j + 4 * q < H) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          p[r][0] = __builtin_fmaf(wv[r][q].x, hv[q].x, p[r][0]); p[r][1] = __builtin_fmaf(wv[r][q].y, hv[q].y, p[r][1]);
          p[r][2] = __builtin_fmaf(wv[r][q].z, hv[q].z, p[r][2]); p[r][3] = __builtin_fmaf(wv[r][q].w, hv[q].w, p[r][3]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) out[r] = (p[r][0] + p[r][1]) + (p[r][2] + p[r][3]);
}
static __device__ void serl_actor_forward_lane_general_t(const serl_rollout_desc &dd, const float *wt, const int wt_members, const unsigned member, const float (&obs)[16],
                                                         float (&act_out)[3])
{
  constexpr int S = 7;
  const int H = __builtin_amdgcn_readfirstlane(dd.hidden), L = __builtin_amdgcn_readfirstlane(dd.num_layers);
  const int act = __builtin_amdgcn_readfirstlane(dd.activation);
  const int Hq = H >> 2;
  const serl_gbytes base = (serl_gbytes)wt;
  const uint64_t gs = (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane(wt_members) * 16u;      // bytes from group g to group g + 1 (wave-uniform, 64-bit products)
  const unsigned moff = member * 16u;                                                              // (serl_rollout_regrouped takes at most 2^22 members)
  auto at = [&](const int g) -> serl_gbytes { return base + (uint64_t)(unsigned)g * gs; };
  auto ld4 = [&](const serl_gbytes gp, const unsigned mo) -> serl_v4f { return *(serl_gptr4)(serl_group_base(gp) + mo); };
  __attribute__((aligned(16))) float hbuf[2][SERL_MAX_HIDDEN];
  float *h0 = hbuf[0], *h1 = hbuf[1];
  // ---- Linear(7, H) act: rows i .. i + 3 = 28 floats = groups 7 (i / 4) .. 7 (i / 4) + 6, the bias group 7 H / 4 + i / 4
  {
    const int b0 = S * Hq;
#pragma nounroll
    for (int i = 0; i < H; i += 4) {
      float p[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[r][0] = 0.0f; p[r][1] = 0.0f; p[r][2] = 0.0f; p[r][3] = 0.0f; }
      const serl_gbytes gw = at(S * (i >> 2));
      const unsigned mo = serl_lane_offset(moff);
      float wf[4 * S];      // (all loads of the four rows first)
#pragma unroll
      for (int g = 0; g < S; ++g) {
        const serl_v4f v = ld4(gw + (uint64_t)g * gs, mo);
        wf[4 * g] = v.x; wf[4 * g + 1] = v.y; wf[4 * g + 2] = v.z; wf[4 * g + 3] = v.w;
      }
      const serl_v4f bv = ld4(at(b0 + (i >> 2)), mo);
#pragma unroll
      for (int j = 0; j < S; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r][j & 3] = __builtin_fmaf(wf[r * S + j], obs[j], p[r][j & 3]);
      }
      serl_v4f t;
      t.x = serl_act(bv.x + ((p[0][0] + p[0][1]) + (p[0][2] + p[0][3])), act);
      t.y = serl_act(bv.y + ((p[1][0] + p[1][1]) + (p[1][2] + p[1][3])), act);
      t.z = serl_act(bv.z + ((p[2][0] + p[2][1]) + (p[2][2] + p[2][3])), act);
      t.w = serl_act(bv.w + ((p[3][0] + p[3][1]) + (p[3][2] + p[3][3])), act);
      *(serl_v4f *)(h0 + i) = t;
    }
  }
  const int lgroups = Hq * H + 3 * Hq, hid = S * Hq + Hq;      // groups per hidden layer, first group of the first hidden layer
  const serl_v4f zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma nounroll
  for (int l = 0; l < L; ++l) {
    const int Wl = hid + l * lgroups, bl = Wl + Hq * H;       // groups: weights (row r = groups r H / 4 ..), then bias / gamma / beta (H / 4 groups each)
#pragma nounroll
    for (int i = 0; i < H; i += 4) {
      float t[4];
      serl_lane_rows_t<4>(at(Wl + i * Hq), gs, moff, H, h0, t);
      const serl_v4f bv = ld4(at(bl + (i >> 2)), serl_lane_offset(moff));
      serl_v4f o;
      o.x = bv.x + t[0]; o.y = bv.y + t[1]; o.z = bv.z + t[2]; o.w = bv.w + t[3];
      *(serl_v4f *)(h1 + i) = o;
    }
    // LayerNorm: the two sums block by block of 16 rows (the last block zero padded: H % 4 == 0, so whole groups of four)
    float sum = 0.0f;
#pragma nounroll
    for (int b = 0; b < H; b += 16) {
      serl_v4f v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = b + 4 * q < H ? *(const serl_v4f *)(h1 + b + 4 * q) : zero4;
      const float t = serl_tree16_v4(v[0], v[1], v[2], v[3]);
      sum = b == 0 ? t : sum + t;
    }
    const float mean = sum / (float)H;
    float var = 0.0f;
#pragma nounroll
    for (int b = 0; b < H; b += 16) {
      serl_v4f v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = zero4;
        if (b + 4 * q < H) {
          const serl_v4f hv = *(const serl_v4f *)(h1 + b + 4 * q);
          const float d0 = hv.x - mean, d1 = hv.y - mean, d2 = hv.z - mean, d3 = hv.w - mean;
          v[q].x = d0 * d0; v[q].y = d1 * d1; v[q].z = d2 * d2; v[q].w = d3 * d3;
        }
      }
      const float t = serl_tree16_v4(v[0], v[1], v[2], v[3]);
      var = b == 0 ? t : var + t;
    }
    const float den = sqrtf(var / (float)(H - 1)) + 1e-6f;
#pragma nounroll
    for (int i = 0; i < H; i += 4) {
      const serl_v4f hv = *(const serl_v4f *)(h1 + i);
      const serl_gbytes gg = at(bl + Hq + (i >> 2));
      const unsigned mo = serl_lane_offset(moff);
      const serl_v4f gm = ld4(gg, mo), bt = ld4(gg + (uint64_t)(unsigned)Hq * gs, mo);
      serl_v4f t;
      t.x = serl_act(gm.x * (hv.x - mean) / den + bt.x, act);
      t.y = serl_act(gm.y * (hv.y - mean) / den + bt.y, act);
      t.z = serl_act(gm.z * (hv.z - mean) / den + bt.z, act);
      t.w = serl_act(gm.w * (hv.w - mean) / den + bt.w, act);
      *(serl_v4f *)(h0 + i) = t;
    }
  }
  // ---- Linear(H, 3) tanh: rows of H / 4 groups, the bias in elements 0 .. 2 of the last group of the copy
  const int outl = hid + L * lgroups;
  const serl_v4f ob = ld4(at(outl + 3 * Hq), serl_lane_offset(moff));
  const float ob3[3] = {ob.x, ob.y, ob.z};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float t[1];
    serl_lane_rows_t<1>(at(outl + i * Hq), gs, moff, H, h0, t);
    act_out[i] = det_tanhf(ob3[i] + t[0]);
  }
}

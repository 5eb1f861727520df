// serl_td3_core.inc -- the training core of the fused TD3 learner (serl_td3.hip), shared with the kernels built from its phases outside
// the learner: the distillation crossover (serl_distill_general.inc, inside serl_td3.hip) and the batch-parallel sensitivity
// (serl_ga_sens.hip).  Included inside the including unit's unnamed namespace, after serl_ctx.h and serl_td3_mfma.h.  The text is the
// learner's own, moved here unchanged: thread map, tiles and phase barriers are described at the top of serl_td3.hip.
constexpr int NT = 512;                 // threads per workgroup
constexpr int NW = NT / 64;             // wavefronts
constexpr int BP = 128;                 // samples per row of a global activation array = the largest minibatch but for the chunked flavours
constexpr int BIG_B = 512;              // the largest minibatch of the chunked flavours (serl_td3_train_big): four chunks of BP samples
constexpr int NG = NT / BP;             // output groups
constexpr int LP = 132;                 // floats per row of an LDS tile (128 samples + 4: consecutive rows start 4 banks apart)
constexpr int TILE_ROWS = 128;          // the widest layer
constexpr int HC = 64;                  // hidden units of the critic (td3.py:24)
constexpr int MAX_IN = 20;              // S + A at most

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__device__ __forceinline__ float t_act(float v, int act)
{
  if (act == SERL_ACT_TANH) return tanhf(v);
  if (act == SERL_ACT_ELU) return v > 0.0f ? v : expm1f(v);
  return v > 0.0f ? v : 0.01f * v;
}

// derivative of the activation, from its VALUE a
__device__ __forceinline__ float t_dact(float a, int act)
{
  if (act == SERL_ACT_TANH) return 1.0f - a * a;
  if (act == SERL_ACT_ELU) return a > 0.0f ? 1.0f : a + 1.0f;
  return a > 0.0f ? 1.0f : 0.01f;
}

// one Linear of a packed row: offsets of W[N][K], b[N] and, with ln, gamma[N], beta[N]; fin: 0 = activation, 1 = tanh, 2 = identity
struct Layer { int oW, ob, og, obe, N, K, ln, fin; };
struct Net { int critic, S, H, L, A; };          // critic: one twin of the Critic (K0 = S + A); else the actor

__device__ __forceinline__ int net_layers(const Net &n) { return n.critic ? 3 : n.L + 2; }
__device__ __forceinline__ int net_width(const Net &n) { return n.critic ? HC : n.H; }
__device__ __forceinline__ int net_in(const Net &n) { return n.critic ? n.S + n.A : n.S; }

__device__ __forceinline__ Layer net_layer(const Net &n, int l)
{
  Layer y;
  y.og = y.obe = 0; y.ln = 0; y.fin = 0;
  if (n.critic) {
    const int K0 = n.S + n.A, l1 = HC * K0 + 3 * HC, l2 = l1 + HC * HC + 3 * HC;
    if (l == 0) { y.oW = 0; y.N = HC; y.K = K0; y.ln = 1; }
    else if (l == 1) { y.oW = l1; y.N = HC; y.K = HC; y.ln = 1; }
    else { y.oW = l2; y.N = 1; y.K = HC; y.fin = 2; }
  } else {
    const int H = n.H, l1 = H * n.S + H, ls = H * H + 3 * H;
    if (l == 0) { y.oW = 0; y.N = H; y.K = n.S; }
    else if (l <= n.L) { y.oW = l1 + (l - 1) * ls; y.N = H; y.K = H; y.ln = 1; }
    else { y.oW = l1 + n.L * ls; y.N = n.A; y.K = H; y.fin = 1; }
  }
  y.ob = y.oW + y.N * y.K;
  if (y.ln) { y.og = y.ob + y.N; y.obe = y.og + y.N; }
  return y;
}

// floats of a tape: per layer the normalised values n [W][BP] and the outputs h [W][BP], then the standard deviations [layers][BP]
__host__ __device__ inline int64_t tape_floats(int layers, int width) { return ((int64_t)2 * layers * width + layers) * BP; }

// parameters of a packed actor row and of ONE twin of a packed critic row (the shapes the entries accept: far below 2^31)
__host__ __device__ inline int actor_params(int S, int A, int H, int L) { return H * S + H + L * (H * H + 3 * H) + A * H + A; }
__host__ __device__ inline int twin_params(int S, int A) { return HC * (S + A) + 3 * HC + HC * HC + 3 * HC + HC + 1; }

// A learner's workspace: gradients | per chunk of BP samples: inputs s, s2, (s, a), (s2, a2) | the actor's tape | the critic's tape.
// The host sizes it and the kernels carve it with these two.
__host__ __device__ inline int grad_floats(int S, int A, int H, int L)
{
  const int Pa = actor_params(S, A, H, L), Pc = 2 * twin_params(S, A);
  return ((Pa > Pc ? Pa : Pc) + 3) & ~3;
}
__host__ __device__ inline int64_t chunk_floats(int H, int L) { return 4 * MAX_IN * BP + tape_floats(L + 2, H) + tape_floats(3, HC); }

struct Td3Work { float *g, *in_s, *in_s2, *in_sa, *in_sa2, *tape_a, *tape_c; };

__device__ __forceinline__ Td3Work td3_carve(float *wk, int S, int A, int H, int L, int chunk)
{
  Td3Work k;
  k.g = wk;
  k.in_s = wk + grad_floats(S, A, H, L) + chunk * chunk_floats(H, L); k.in_s2 = k.in_s + MAX_IN * BP; k.in_sa = k.in_s2 + MAX_IN * BP;
  k.in_sa2 = k.in_sa + MAX_IN * BP; k.tape_a = k.in_sa2 + MAX_IN * BP; k.tape_c = k.tape_a + tape_floats(L + 2, H);
  return k;
}

struct Ctx {
  float *T0, *T1;               // LDS tiles [TILE_ROWS][LP]
  float *red, *red4;            // LDS [NW], [NG][BP]
  int t, b, g, wave, lane;
  int B, B4, act;
  bool live;                    // this wavefront holds samples of the minibatch
};

__device__ __forceinline__ float block_sum(const Ctx &c, float v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if (c.lane == 0) c.red[c.wave] = v;
  __syncthreads();
  float s = 0.0f;
#pragma unroll
  for (int w = 0; w < NW; ++w) s += c.red[w];
  return s;
}

// the sum over the four output groups of a sample
__device__ __forceinline__ float sample_sum(const Ctx &c, float v)
{
  __syncthreads();
  c.red4[c.g * BP + c.b] = v;
  __syncthreads();
  return (c.red4[c.b] + c.red4[BP + c.b]) + (c.red4[2 * BP + c.b] + c.red4[3 * BP + c.b]);
}

// rows [K][BP] of a global array -> an LDS tile
__device__ __forceinline__ void stage(const Ctx &c, const float *src, int K, float *T)
{
  for (int e = c.t; e < K * BP; e += NT) T[(e >> 7) * LP + (e & 127)] = src[e];
}

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // four consecutive weights of a row that is only 4 B aligned

// Y[i][b] = bias[i] + sum_j W[i][j] X[j][b]
__device__ __forceinline__ void dense_fwd(const Ctx &c, const float *W, const float *bias, int N, int K, const float *X, float *Y)
{
  if (!c.live) return;
  for (int i0 = 4 * c.g; i0 < N; i0 += 4 * NG) {
    const int i1 = min(i0 + 1, N - 1), i2 = min(i0 + 2, N - 1), i3 = min(i0 + 3, N - 1);
    const float *w0 = W + (size_t)i0 * K, *w1 = W + (size_t)i1 * K, *w2 = W + (size_t)i2 * K, *w3 = W + (size_t)i3 * K;
    float a0 = bias[i0], a1 = bias[i1], a2 = bias[i2], a3 = bias[i3];
    int j = 0;
    for (; j + 3 < K; j += 4) {
      const f4u u0 = *reinterpret_cast<const f4u *>(w0 + j), u1 = *reinterpret_cast<const f4u *>(w1 + j);
      const f4u u2 = *reinterpret_cast<const f4u *>(w2 + j), u3 = *reinterpret_cast<const f4u *>(w3 + j);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float x = X[(j + q) * LP + c.b];
        a0 = fmaf(u0[q], x, a0); a1 = fmaf(u1[q], x, a1); a2 = fmaf(u2[q], x, a2); a3 = fmaf(u3[q], x, a3);
      }
    }
    for (; j < K; ++j) {
      const float x = X[j * LP + c.b];
      a0 = fmaf(w0[j], x, a0); a1 = fmaf(w1[j], x, a1); a2 = fmaf(w2[j], x, a2); a3 = fmaf(w3[j], x, a3);
    }
    Y[i0 * LP + c.b] = a0;
    if (i0 + 1 < N) Y[(i0 + 1) * LP + c.b] = a1;
    if (i0 + 2 < N) Y[(i0 + 2) * LP + c.b] = a2;
    if (i0 + 3 < N) Y[(i0 + 3) * LP + c.b] = a3;
  }
}

// Xo[j][b] = sum_i W[i][j] D[i][b]
__device__ __forceinline__ void dense_bwd_x(const Ctx &c, const float *W, int N, int K, const float *D, float *Xo)
{
  if (!c.live) return;
  for (int j0 = 4 * c.g; j0 < K; j0 += 4 * NG) {
    const int j1 = min(j0 + 1, K - 1), j2 = min(j0 + 2, K - 1), j3 = min(j0 + 3, K - 1);
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (j0 + 3 < K) {
#pragma unroll 4
      for (int i = 0; i < N; ++i) {
        const float dv = D[i * LP + c.b];
        const f4u u = *reinterpret_cast<const f4u *>(W + (size_t)i * K + j0);
        a0 = fmaf(u[0], dv, a0); a1 = fmaf(u[1], dv, a1); a2 = fmaf(u[2], dv, a2); a3 = fmaf(u[3], dv, a3);
      }
    } else {
      for (int i = 0; i < N; ++i) {
        const float dv = D[i * LP + c.b];
        const float *w = W + (size_t)i * K;
        a0 = fmaf(w[j0], dv, a0); a1 = fmaf(w[j1], dv, a1); a2 = fmaf(w[j2], dv, a2); a3 = fmaf(w[j3], dv, a3);
      }
    }
    Xo[j0 * LP + c.b] = a0;
    if (j0 + 1 < K) Xo[(j0 + 1) * LP + c.b] = a1;
    if (j0 + 2 < K) Xo[(j0 + 2) * LP + c.b] = a2;
    if (j0 + 3 < K) Xo[(j0 + 3) * LP + c.b] = a3;
  }
}

// gW[i][j] (+)= sum_b D[i][b] X[j][b] over the samples below B4; a thread's block: rows a + ti r, columns q + tj s (r, s < 4)
__device__ __forceinline__ void dense_bwd_w(const Ctx &c, const float *D, const float *X, int N, int K, float *gW, bool accum)
{
  const int ti = (N + 3) >> 2, tj = (K + 3) >> 2;
  for (int tile = c.t; tile < ti * tj; tile += NT) {
    const int a = tile / tj, q = tile - a * tj;
    const float *dr[4], *xr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { dr[r] = D + min(a + ti * r, N - 1) * LP; xr[r] = X + min(q + tj * r, K - 1) * LP; }
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[r][s] = 0.0f;
    for (int b = 0; b < c.B4; b += 4) {
      float4 dv[4], xv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) { dv[r] = *reinterpret_cast<const float4 *>(dr[r] + b); xv[r] = *reinterpret_cast<const float4 *>(xr[r] + b); }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[r][s] = fmaf(dv[r].x, xv[s].x, fmaf(dv[r].y, xv[s].y, fmaf(dv[r].z, xv[s].z, fmaf(dv[r].w, xv[s].w, acc[r][s]))));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int i = a + ti * r, j = q + tj * s;
        if (i < N && j < K) gW[(size_t)i * K + j] = accum ? gW[(size_t)i * K + j] + acc[r][s] : acc[r][s];
      }
  }
}

// The dense phases of a kernel flavour: MFMA = false runs the scalar chains above, MFMA = true the same chains, element for element in
// the same order, on the f32 matrix cores (serl_td3_mfma.h).  Everything else in this file is shared by both flavours.
typedef td3_mfma::Dense<LP, NW> DenseMx;

template <bool MFMA>
__device__ __forceinline__ void dense_fwd_k(const Ctx &c, const float *W, const float *bias, int N, int K, const float *X, float *Y)
{
  if constexpr (MFMA) DenseMx::fwd(c.wave, c.lane, c.B, W, bias, N, K, X, Y);
  else dense_fwd(c, W, bias, N, K, X, Y);
}

template <bool MFMA>
__device__ __forceinline__ void dense_bwd_x_k(const Ctx &c, const float *W, int N, int K, const float *D, float *Xo)
{
  if constexpr (MFMA) DenseMx::bwd_x(c.wave, c.lane, c.B, W, N, K, D, Xo);
  else dense_bwd_x(c, W, N, K, D, Xo);
}

template <bool MFMA>
__device__ __forceinline__ void dense_bwd_w_k(const Ctx &c, const float *D, const float *X, int N, int K, float *gW, bool accum)
{
  if constexpr (MFMA) DenseMx::bwd_w(c.wave, c.lane, c.B4, D, X, N, K, gW, accum);
  else dense_bwd_w(c, D, X, N, K, gW, accum);
}

// g1[i] (+)= sum_b D[i][b], and with tn: g2[i] (+)= sum_b D[i][b] tn[i][b]; one wavefront per row
__device__ __forceinline__ void row_grads(const Ctx &c, const float *D, const float *tn, int N, float *g1, float *g2, bool accum)
{
  for (int i = c.wave; i < N; i += NW) {
    float s = 0.0f, p = 0.0f;
    for (int b = c.lane; b < c.B4; b += 64) {
      const float dv = D[i * LP + b];
      s += dv;
      if (tn) p = fmaf(dv, tn[i * BP + b], p);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); p += __shfl_xor(p, o); }
    if (c.lane == 0) {
      g1[i] = accum ? g1[i] + s : s;
      if (tn) g2[i] = accum ? g2[i] + p : p;
    }
  }
}

// the project's LayerNorm (unbiased std, eps on the std) and the activation, in place on Y; n, h and the std go to the tape
__device__ __forceinline__ void ln_act(const Ctx &c, float *Y, const float *gam, const float *bet, int N, float *tn, float *th, float *tsd)
{
  float s = 0.0f;
  for (int i = c.g; i < N; i += NG) s += Y[i * LP + c.b];
  const float mean = sample_sum(c, s) / (float)N;
  float v = 0.0f;
  for (int i = c.g; i < N; i += NG) { const float dv = Y[i * LP + c.b] - mean; v = fmaf(dv, dv, v); }
  const float sd = sqrtf(sample_sum(c, v) / (float)(N - 1));
  const float Dn = sd + 1e-6f;
  for (int i = c.g; i < N; i += NG) {
    const float n = (Y[i * LP + c.b] - mean) / Dn;
    const float h = t_act(gam[i] * n + bet[i], c.act);
    Y[i * LP + c.b] = h;
    if (tn) { tn[i * BP + c.b] = n; th[i * BP + c.b] = h; }
  }
  if (tn && c.g == 0) tsd[c.b] = sd;
}

// D = dL/dh of a LayerNorm layer -> dL/dy in place; dgamma / dbeta to gg / gbe when given
__device__ __forceinline__ void ln_act_bwd(const Ctx &c, float *D, const float *gam, int N, const float *tn, const float *th, const float *tsd,
                                           float *gg, float *gbe, bool accum)
{
  float s1 = 0.0f, s2 = 0.0f;
  for (int i = c.g; i < N; i += NG) {
    const float dz = D[i * LP + c.b] * t_dact(th[i * BP + c.b], c.act);
    D[i * LP + c.b] = dz;
    const float dn = dz * gam[i];
    s1 += dn;
    s2 = fmaf(dn, tn[i * BP + c.b], s2);
  }
  s1 = sample_sum(c, s1);
  s2 = sample_sum(c, s2);
  if (gg) row_grads(c, D, tn, N, gbe, gg, accum);
  __syncthreads();
  const float sd = tsd[c.b];
  const float Dn = sd + 1e-6f, m = s1 / (float)N;
  const float k2 = sd > 0.0f ? s2 / ((float)(N - 1) * sd) : 0.0f;
  for (int i = c.g; i < N; i += NG) D[i * LP + c.b] = (D[i * LP + c.b] * gam[i] - m) / Dn - tn[i * BP + c.b] * k2;
}

// forward pass of `net` (parameters w) on the global input x [K0][BP]; -> the LDS tile that holds the output rows.  With a tape the
// outputs of every layer (and n, std of the LayerNorm ones) are kept for mlp_bwd.
template <bool MFMA>
__device__ __forceinline__ float *mlp_fwd(const Ctx &c, const Net &net, const float *w, const float *x, float *tape)
{
  const int nl = net_layers(net), Wd = net_width(net);
  float *Tin = c.T0, *Tout = c.T1;
  __syncthreads();
  stage(c, x, net_in(net), Tin);
  __syncthreads();
  for (int l = 0; l < nl; ++l) {
    const Layer y = net_layer(net, l);
    dense_fwd_k<MFMA>(c, w + y.oW, w + y.ob, y.N, y.K, Tin, Tout);
    __syncthreads();
    float *tn = tape ? tape + (size_t)(2 * l) * Wd * BP : nullptr, *th = tape ? tn + (size_t)Wd * BP : nullptr;
    float *tsd = tape ? tape + (size_t)2 * nl * Wd * BP + (size_t)l * BP : nullptr;
    if (y.ln) ln_act(c, Tout, w + y.og, w + y.obe, y.N, tn, th, tsd);
    else if (y.fin != 2) {
      for (int i = c.g; i < y.N; i += NG) {
        const float v = Tout[i * LP + c.b];
        const float h = y.fin == 1 ? tanhf(v) : t_act(v, c.act);
        Tout[i * LP + c.b] = h;
        if (th) th[i * BP + c.b] = h;
      }
    }
    __syncthreads();
    float *s = Tin; Tin = Tout; Tout = s;
  }
  return Tin;
}

// backward pass from D = dL/d(the last Linear's output) (an LDS tile, rows of the last layer): parameter gradients to g (laid out
// like the row; added to when accum), unless g is NULL; with DX_INPUT the gradient of the input is returned (an LDS tile, K0 rows).
enum Dx { DX_NONE, DX_INPUT };
template <bool MFMA>
__device__ __forceinline__ float *mlp_bwd(const Ctx &c, const Net &net, const float *w, const float *x, const float *tape, float *D, float *g, bool accum,
                          Dx dx)
{
  const int nl = net_layers(net), Wd = net_width(net);
  float *X = D == c.T0 ? c.T1 : c.T0;
  for (int l = nl - 1; l >= 0; --l) {
    const Layer y = net_layer(net, l);
    __syncthreads();
    if (g) {
      stage(c, l == 0 ? x : tape + (size_t)(2 * (l - 1) + 1) * Wd * BP, y.K, X);
      __syncthreads();
      dense_bwd_w_k<MFMA>(c, D, X, y.N, y.K, g + y.oW, accum);
      row_grads(c, D, nullptr, y.N, g + y.ob, nullptr, accum);
      __syncthreads();
    }
    if (l == 0 && dx == DX_NONE) break;
    dense_bwd_x_k<MFMA>(c, w + y.oW, y.N, y.K, D, X);
    __syncthreads();
    float *s = D; D = X; X = s;
    if (l == 0) break;
    const Layer p = net_layer(net, l - 1);
    const float *tn = tape + (size_t)(2 * (l - 1)) * Wd * BP, *th = tn + (size_t)Wd * BP;
    if (p.ln) ln_act_bwd(c, D, w + p.og, p.N, tn, th, tape + (size_t)2 * nl * Wd * BP + (size_t)(l - 1) * BP, g ? g + p.og : nullptr,
                         g ? g + p.obe : nullptr, accum);
    else
      for (int i = c.g; i < p.N; i += NG) D[i * LP + c.b] *= t_dact(th[i * BP + c.b], c.act);
  }
  __syncthreads();
  return D;
}

// the shapes this core runs and the LDS it takes are stated in serl_shapes.h (serl_learner_range, serl_shape_learner_takes)
static_assert(NT == SERL_LEARNER_THREADS && BP == SERL_LEARNER_BP && BIG_B == SERL_LEARNER_BIG_B && LP == SERL_LEARNER_LP && TILE_ROWS == SERL_LEARNER_TILE_ROWS,
              "serl_shapes.h states this core's contract");

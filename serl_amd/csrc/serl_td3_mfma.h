// serl_td3_mfma.h -- the three dense phases of the TD3 learner (serl_td3.hip) on the f32-in / f32-accumulate matrix cores.
//
// v_mfma_f32_16x16x4_f32 computes D = A B + C of a 16 x 4 and a 4 x 16 f32 block per wavefront; every element of D is the f32 fmaf
// chain C -> k = 0 -> 1 -> 2 -> 3, one rounding per product, nothing wider inside, subnormals kept.  That is the chain the scalar
// phases of serl_td3.hip run per output element, so the phases below feed the k slots in the scalar code's order and their results
// are bit for bit the scalar ones (tests/test_gpu_td3_mfma.py):
//   fwd     C = bias[i], k = j ascending                          Y[i][b] = bias[i] + sum_j W[i][j] X[j][b]
//   bwd_x   C = 0,       k = i ascending                          Xo[j][b] = sum_i W[i][j] D[i][b]
//   bwd_w   C = 0,       slots 0 .. 3 of a step = samples b + 3 .. b, steps b = 0, 4, .. < B4; gW (+)= afterwards, a separate f32 add
// Operands, lane l = 16 s + m:  A[row m][k s], B[k s][column m];  results: D[row 4 s + r][column m] in register r.
//
// A k slot past the end of the reduction (K or N no multiple of 4) multiplies +0 x +0 -- BOTH operands are replaced by zero in
// registers, whatever the LDS row or the weight behind the clamped address holds: fma(+0, +0, acc) changes nothing but the sign of a
// -0.  Rows and columns of a block past the end of the output are computed from clamped (valid, written) addresses and not stored.
// No address is formed outside W[0 .. N K) or the rows [0 .. N) / [0 .. K) of a tile.
//
// Work: one 16-row block of outputs x 32 samples (fwd, bwd_x: two accumulators that share the weight operand; sample 2 m + q of the
// group is column m of accumulator q, so a lane's pair is one 8 B LDS access) or x 32 columns (bwd_w: two accumulators that share the
// D operand) per wavefront and turn.  Groups of 32 samples from B on are skipped; what they hold is never reduced over (B4 <= the end
// of the last group) and reaches no output.  No barriers in here: the callers' __syncthreads separate the phases.
#pragma once
#include <hip/hip_runtime.h>

namespace td3_mfma {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// LP: floats per row of an LDS tile; NW: wavefronts of the workgroup.  `wave` must be wavefront-uniform (the loops around the
// matrix instructions are), lane = 0 .. 63.
template <int LP, int NW>
struct Dense {
  static __device__ __forceinline__ void fwd(int wave, int lane, int B, const float *W, const float *bias, int N, int K, const float *X, float *Y)
  {
    const int m = lane & 15, s = lane >> 4;
    const int nib = (N + 15) >> 4, ngr = (B + 31) >> 5;
    for (int task = wave; task < nib * ngr; task += NW) {
      const int ib = task / ngr, i0 = ib << 4, b0 = (task - ib * ngr) << 5;
      const bool iok = i0 + m < N;
      const float *wr = W + (size_t)min(i0 + m, N - 1) * K;
      const float *xc = X + b0 + 2 * m;
      f32x4 c0, c1;
#pragma unroll
      for (int r = 0; r < 4; ++r) c0[r] = c1[r] = bias[min(i0 + 4 * s + r, N - 1)];
      // four steps (16 k) per turn; the operands of the next turn are fetched before this turn's products are issued
      float wv[4], wn[4];
      float2 xv[4], xn[4];
      auto fetch = [&](int j0, float *w, float2 *x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int jc = min(j0 + 4 * q + s, K - 1);
          w[q] = wr[jc];
          x[q] = *reinterpret_cast<const float2 *>(xc + jc * LP);
        }
      };
      fetch(0, wv, xv);
      for (int j0 = 0; j0 < K; j0 += 16) {
        const bool more = j0 + 16 < K;
        if (more) fetch(j0 + 16, wn, xn);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int j = j0 + 4 * q + s;
          if (j0 + 4 * q < K) {                                       // (wavefront-uniform)
            const float a = (j < K && iok) ? wv[q] : 0.0f, x0 = j < K ? xv[q].x : 0.0f, x1 = j < K ? xv[q].y : 0.0f;
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x0, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x1, c1, 0, 0, 0);
          }
        }
        if (more) {
#pragma unroll
          for (int q = 0; q < 4; ++q) { wv[q] = wn[q]; xv[q] = xn[q]; }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * s + r;
        if (i < N) *reinterpret_cast<float2 *>(Y + i * LP + b0 + 2 * m) = make_float2(c0[r], c1[r]);
      }
    }
  }

  static __device__ __forceinline__ void bwd_x(int wave, int lane, int B, const float *W, int N, int K, const float *D, float *Xo)
  {
    const int m = lane & 15, s = lane >> 4;
    const int njb = (K + 15) >> 4, ngr = (B + 31) >> 5;
    for (int task = wave; task < njb * ngr; task += NW) {
      const int jb = task / ngr, j0 = jb << 4, b0 = (task - jb * ngr) << 5;
      const bool jok = j0 + m < K;
      const float *wc = W + min(j0 + m, K - 1);
      const float *dc = D + b0 + 2 * m;
      f32x4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = {0.0f, 0.0f, 0.0f, 0.0f};
      float wv[4], wn[4];
      float2 dv[4], dn[4];
      auto fetch = [&](int i0, float *w, float2 *x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ic = min(i0 + 4 * q + s, N - 1);
          w[q] = wc[(size_t)ic * K];
          x[q] = *reinterpret_cast<const float2 *>(dc + ic * LP);
        }
      };
      fetch(0, wv, dv);
      for (int i0 = 0; i0 < N; i0 += 16) {
        const bool more = i0 + 16 < N;
        if (more) fetch(i0 + 16, wn, dn);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + 4 * q + s;
          if (i0 + 4 * q < N) {                                       // (wavefront-uniform)
            const float a = (i < N && jok) ? wv[q] : 0.0f, d0 = i < N ? dv[q].x : 0.0f, d1 = i < N ? dv[q].y : 0.0f;
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, d0, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, d1, c1, 0, 0, 0);
          }
        }
        if (more) {
#pragma unroll
          for (int q = 0; q < 4; ++q) { wv[q] = wn[q]; dv[q] = dn[q]; }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + 4 * s + r;
        if (j < K) *reinterpret_cast<float2 *>(Xo + j * LP + b0 + 2 * m) = make_float2(c0[r], c1[r]);
      }
    }
  }

  // B4: the samples reduced over, a multiple of 4
  static __device__ __forceinline__ void bwd_w(int wave, int lane, int B4, const float *D, const float *X, int N, int K, float *gW, bool accum)
  {
    const int m = lane & 15, s = lane >> 4;
    const int nib = (N + 15) >> 4, njp = (K + 31) >> 5;
    for (int task = wave; task < nib * njp; task += NW) {
      const int ib = task / njp, i0 = ib << 4, j0 = (task - ib * njp) << 5;
      const bool two = j0 + 16 < K;                                   // (wavefront-uniform) the second block of columns exists
      const float *dr = D + min(i0 + m, N - 1) * LP + 3 - s;          // slot s of the step at b: sample b + 3 - s
      const float *xr0 = X + min(j0 + m, K - 1) * LP + 3 - s, *xr1 = X + min(j0 + 16 + m, K - 1) * LP + 3 - s;
      f32x4 c0 = {0.0f, 0.0f, 0.0f, 0.0f}, c1 = {0.0f, 0.0f, 0.0f, 0.0f};
      // four steps (16 samples) per turn, their operands read first; a step from B4 on is not issued (what its reads return -- they
      // stay inside the rows, b + 4 q + 3 <= 127 -- is dropped)
      for (int b = 0; b < B4; b += 16) {
        float dv[4], x0[4], x1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { dv[q] = dr[b + 4 * q]; x0[q] = xr0[b + 4 * q]; x1[q] = xr1[b + 4 * q]; }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (b + 4 * q < B4) {                                       // (wavefront-uniform)
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[q], x0[q], c0, 0, 0, 0);
            if (two) c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[q], x1[q], c1, 0, 0, 0);
          }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + 4 * s + r, ja = j0 + m, jb = j0 + 16 + m;
        if (i < N && ja < K) { float *o = gW + (size_t)i * K + ja; *o = accum ? *o + c0[r] : c0[r]; }
        if (two && i < N && jb < K) { float *o = gW + (size_t)i * K + jb; *o = accum ? *o + c1[r] : c1[r]; }
      }
    }
  }
};

}  // namespace td3_mfma

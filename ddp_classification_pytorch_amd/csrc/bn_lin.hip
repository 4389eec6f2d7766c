// Backward of a training-mode BN behind a 1x1 stride-1 conv, as a linear map of the conv's own operands.
//
// An identity bottleneck ends in  x3 = a2 * W3^T  ->  bn3  ->  (+ residual, ReLU).  The next block's
// conv1 dgrad epilogue leaves the masked gradient g [n rows][C] of bn3's output and the sums
// S1 = sum g, S2 = sum g * xhat.  BN backward is affine per channel,
//     dx3 = a o g + b o (x3 - mean) - e,     a = gamma * invstd,  b = -a * invstd * S2 / n,  e = a * S1 / n,
// and with mean = colmean(a2) * W3^T the (x3 - mean) term folds into m x m matrices (m = width of a2):
//     d_a2 = g * (diag(a) W3) + a2 * Q + bias,     Q = W3^T diag(b) W3,   bias = -colmean(a2) * Q - e * W3
//     dW3  = diag(a) (g^T a2) + diag(b) W3 (a2^T a2 - n colmean^T colmean) - e (x) colsum(a2)
// so dx3 [n][C] is never written or read: the data gradient is one GEMM over the K-concatenated sources
// [g | a2] (conv_igemm.hip, second A source) and the weight gradient the usual g^T a2 plus a fix-up.
//
// This file holds the small fp32 kernels around those GEMMs: the concatenated weight and its bias
// (bn_lin_prep) and the weight-gradient fix-up (bn_lin_dw).  The bias is computed from the bf16-ROUNDED
// Q the GEMM multiplies a2 with, so the rounding error of Q only meets the centred a2 - colmean(a2)
// (BN inputs have means large against their spread: an uncentred constant would leave a2 * dQ whole).
#include "common.cuh"
#include "launchers.h"

namespace dcp {

// coef [3][C]: a, b, e
__global__ void __launch_bounds__(256) bn_lin_coef_kernel(const float* __restrict__ scale,
                                                          const float* __restrict__ invstd,
                                                          const float* __restrict__ sums, float inv_count, int C,
                                                          float* __restrict__ coef) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float a = scale[c];
  coef[c] = a;
  coef[C + c] = -a * invstd[c] * (sums[C + c] * inv_count);
  coef[2 * C + c] = a * (sums[c] * inv_count);
}

// wcat[j][c] = bf16(a[c] * wt[j][c]), c < C: the first C columns of the [m][C + m] concatenated weight
__global__ void __launch_bounds__(256) bn_lin_scale_kernel(const bf16* __restrict__ wt, const float* __restrict__ coef,
                                                           int m, int C, bf16* __restrict__ wcat) {
  const int c8 = C / 8;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m * c8) return;
  const int j = i / c8, c0 = (i - j * c8) * 8;
  const bf16x8 w = *(const bf16x8*)(wt + (size_t)j * C + c0);
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = f2bf(coef[c0 + e] * bf2f(w[e]));
  *(bf16x8*)(wcat + (size_t)j * (C + m) + c0) = o;
}

// Q[j][k] = sum_c b[c] W3[c][j] W3[c][k]   (w3: [C][m] bf16), as fp32 partial slices qpart[z][j][k] over
// the channel ranges [z cper, (z + 1) cper) (cper % 64 == 0): m / 64 x m / 32 tiles alone are 32
// workgroups at m = 256.  Workgroup tile 32 j x 64 k; thread (k = tid & 63, 8 j's of group tid >> 6).
// Per 64-channel chunk the b-scaled [64 c][32 j] operand sits in LDS (read as wave-wide broadcasts), the
// k operand streams coalesced from the weight (L2 resident).  fp32 throughout: m <= 512 is at most 1 GFLOP.
__global__ void __launch_bounds__(256) bn_lin_q_kernel(const bf16* __restrict__ w3, const float* __restrict__ coef,
                                                       int m, int C, int cper, float* __restrict__ qpart) {
  __shared__ __attribute__((aligned(16))) float L[64][32];
  const int tid = threadIdx.x, kl = tid & 63, jg = tid >> 6;
  const int j0 = blockIdx.y * 32, k = blockIdx.x * 64 + kl;
  const float* b = coef + C;
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.f;
  const int cbeg = blockIdx.z * cper, cend = min(C, cbeg + cper);
  for (int c0 = cbeg; c0 < cend; c0 += 64) {
    __syncthreads();
    // 64 x 32 tile: 8 elements per thread (row tid / 4, columns (tid % 4) * 8 ..)
    {
      const int r = tid >> 2, q = (tid & 3) * 8;
      const bf16x8 w = *(const bf16x8*)(w3 + (size_t)(c0 + r) * m + j0 + q);
      const float bc = b[c0 + r];
#pragma unroll
      for (int e = 0; e < 8; ++e) L[r][q + e] = bc * bf2f(w[e]);
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < 64; ++r) {
      const float wk = bf2f(w3[(size_t)(c0 + r) * m + k]);
      const f32x4 l0 = *(const f32x4*)&L[r][jg * 8], l1 = *(const f32x4*)&L[r][jg * 8 + 4];
      acc[0] = fmaf(l0[0], wk, acc[0]);
      acc[1] = fmaf(l0[1], wk, acc[1]);
      acc[2] = fmaf(l0[2], wk, acc[2]);
      acc[3] = fmaf(l0[3], wk, acc[3]);
      acc[4] = fmaf(l1[0], wk, acc[4]);
      acc[5] = fmaf(l1[1], wk, acc[5]);
      acc[6] = fmaf(l1[2], wk, acc[6]);
      acc[7] = fmaf(l1[3], wk, acc[7]);
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) qpart[((size_t)blockIdx.z * m + j0 + jg * 8 + u) * m + k] = acc[u];
}

// wcat[j][C + k] = bf16(sum_z qpart[z][j][k]): the slices in order, one rounding
__global__ void __launch_bounds__(256) bn_lin_q_round_kernel(const float* __restrict__ qpart, int slices, int m, int C,
                                                             bf16* __restrict__ wcat) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m * m) return;
  float t = 0.f;
  for (int z = 0; z < slices; ++z) t += qpart[(size_t)z * m * m + i];
  const int j = i / m, k = i - j * m;
  wcat[(size_t)j * (C + m) + C + k] = f2bf(t);
}

// Column sums of a2 [M][m] as per-workgroup partials part[blockIdx.x][m] (summed by launch_partial_sum).
// The generic colsum (bn.hip) is sized for a linear layer's bias gradient (<= 128 workgroups, one load in
// flight per thread: 1.1 TB/s on a 1.6 GB activation); here every CU streams, four 16-byte loads in
// flight per thread.  Thread = one 8-channel chunk of row slot tid / (m / 8), as the row-tiled BN kernels.
__global__ void __launch_bounds__(256) bn_lin_colsum_kernel(const bf16* __restrict__ x, int M, int m,
                                                            float* __restrict__ part) {
  const int cpr = m >> 3, rpi = 256 / cpr;
  const int slot = threadIdx.x / cpr, ch = threadIdx.x - slot * cpr;
  float s[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = 0.f;
  if (slot < rpi) {
    const size_t step = (size_t)gridDim.x * rpi;
    size_t r = (size_t)blockIdx.x * rpi + slot;
    for (; r + 3 * step < (size_t)M; r += 4 * step) {
      bf16x8 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const bf16x8*)(x + (r + u * step) * m + ch * 8);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += bf2f(v[u][k]);
    }
    for (; r < (size_t)M; r += step) {
      const bf16x8 v = *(const bf16x8*)(x + r * m + ch * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += bf2f(v[k]);
    }
  }
  __shared__ float sh[2048];
#pragma unroll
  for (int k = 0; k < 8; ++k) sh[threadIdx.x * 8 + k] = s[k];
  __syncthreads();
  if (slot == 0)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float t = 0.f;
      for (int sl = 0; sl < rpi; ++sl) t += sh[(sl * cpr + ch) * 8 + k];  // fixed order
      part[(size_t)blockIdx.x * m + ch * 8 + k] = t;
    }
}

// sums[1][c] = S2[c] = sum g xhat = invstd[c] * sum_k W3[c][k] * (G[c][k] - S1[c] * colmean[k]),  S1 = sums[0]:
// the BN input is x3 = a2 W3^T, so sum_rows g (x3 - mean) = W3 (g^T a2 - S1 (x) colmean(a2)) row by row -- from
// the weight-gradient GEMM's G = g^T a2 [C][m] instead of a pass over x3 (the dgrad epilogue that hands g
// over then loads no BN-input rows, conv_igemm.hip EPI 5).  The difference is taken per k, before the
// sum: each term is a centred covariance, so a BN input whose mean is large against its spread cancels
// nothing here.  One wave per channel, lanes strided over k, fixed-order shuffle reduction (deterministic).
__global__ void __launch_bounds__(256) bn_lin_s2_kernel(const float* __restrict__ G, const bf16* __restrict__ w3,
                                                        const float* __restrict__ colsum,
                                                        const float* __restrict__ invstd, float inv_count, int m,
                                                        int C, float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const float s1 = sums[c];
  const float* g = G + (size_t)c * m;
  const bf16* w = w3 + (size_t)c * m;
  float s = 0.f;
  for (int k = lane; k < m; k += 64) s = fmaf(bf2f(w[k]), fmaf(-s1, colsum[k] * inv_count, g[k]), s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) sums[C + c] = s * invstd[c];
}

// bias[j] = -( sum_k colmean[k] * Qr[j][k] + sum_c e[c] * wt[j][c] ),  Qr = the ROUNDED Q of wcat's row j
// (exactly what the GEMM multiplies a2 with).  One wave per j, fixed-order shuffle reduction.
__global__ void __launch_bounds__(256) bn_lin_bias_kernel(const bf16* __restrict__ wt, const bf16* __restrict__ wcat,
                                                          const float* __restrict__ coef,
                                                          const float* __restrict__ colsum, float inv_count, int m,
                                                          int C, float* __restrict__ bias) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= m) return;
  const float* e = coef + 2 * C;
  float s = 0.f;
  for (int k = lane; k < m; k += 64) s = fmaf(colsum[k] * inv_count, bf2f(wcat[(size_t)j * (C + m) + C + k]), s);
  float t = 0.f;
  for (int c = lane; c < C; c += 64) t = fmaf(e[c], bf2f(wt[(size_t)j * C + c]), t);
  s += t;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) bias[j] = -s;
}

// dw[c][j] = a[c] G[c][j] + b[c] sum_k W3[c][k] (A2[k][j] - colsum[k] colsum[j] / n) - e[c] colsum[j]
// G = g^T a2 [C][m], A2 = a2^T a2 [m][m] (fp32, from the weight-gradient GEMMs).  Workgroup tile
// 32 c x 64 j; thread (j = tid & 63, 8 c's of group tid >> 6); per 64-deep k chunk the [32 c][64 k]
// weight rows sit in LDS (k-major, read as broadcasts) beside the chunk's column sums.
__global__ void __launch_bounds__(256) bn_lin_dw_kernel(const float* __restrict__ G, const float* __restrict__ A2,
                                                        const bf16* __restrict__ w3, const float* __restrict__ coef,
                                                        const float* __restrict__ colsum, float inv_count, int m,
                                                        int C, float* __restrict__ dw) {
  __shared__ __attribute__((aligned(16))) float L[64][32];  // [k][c]
  __shared__ float cs[64];
  const int tid = threadIdx.x, jl = tid & 63, cg = tid >> 6;
  const int c0 = blockIdx.y * 32, j = blockIdx.x * 64 + jl;
  const float csj = colsum[j] * inv_count;
  float acc[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) acc[u] = 0.f;
  for (int k0 = 0; k0 < m; k0 += 64) {
    __syncthreads();
    {
      // rows c0 + tid / 8, columns k0 + (tid % 8) * 8 .. of the weight, transposed into L[k][c]
      const int r = tid >> 3, q = (tid & 7) * 8;
      const bf16x8 w = *(const bf16x8*)(w3 + (size_t)(c0 + r) * m + k0 + q);
#pragma unroll
      for (int e = 0; e < 8; ++e) L[q + e][r] = bf2f(w[e]);
      if (tid < 64) cs[tid] = colsum[k0 + tid];
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < 64; ++kk) {
      const float cov = fmaf(-cs[kk], csj, A2[(size_t)(k0 + kk) * m + j]);
      const f32x4 l0 = *(const f32x4*)&L[kk][cg * 8], l1 = *(const f32x4*)&L[kk][cg * 8 + 4];
      acc[0] = fmaf(l0[0], cov, acc[0]);
      acc[1] = fmaf(l0[1], cov, acc[1]);
      acc[2] = fmaf(l0[2], cov, acc[2]);
      acc[3] = fmaf(l0[3], cov, acc[3]);
      acc[4] = fmaf(l1[0], cov, acc[4]);
      acc[5] = fmaf(l1[1], cov, acc[5]);
      acc[6] = fmaf(l1[2], cov, acc[6]);
      acc[7] = fmaf(l1[3], cov, acc[7]);
    }
  }
  const float csum = colsum[j];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int c = c0 + cg * 8 + u;
    const size_t o = (size_t)c * m + j;
    dw[o] = coef[c] * G[o] + coef[C + c] * acc[u] - coef[2 * C + c] * csum;
  }
}

// (m <= 2048: a workgroup's 256 threads cover one row of 8-channel chunks in the column sums)
bool bn_lin_supported(int m, int C) { return m >= 64 && m % 64 == 0 && m <= 2048 && C >= 64 && C % 64 == 0; }

// workgroups (= partial rows) of the column sums: two per CU (8 MB of loads in flight; the partial rows are
// then summed by one launch_partial_sum workgroup per 64 columns), at least 4 x 4 rows each
int bn_lin_colsum_partials(int M, int m) {
  const int rpi = 256 / (m / 8);
  const long g = ((long)M + 16L * rpi - 1) / (16L * rpi);
  return (int)(g > 512 ? 512 : (g < 1 ? 1 : g));
}

// channel slices of the Q product: enough workgroups for the chip, whole 64-channel chunks
int bn_lin_q_slices(int m, int C) {
  const int tiles = (m / 64) * (m / 32);
  int s = (256 + tiles - 1) / tiles;
  if (s > C / 64) s = C / 64;
  return s < 1 ? 1 : s;
}

// part: [bn_lin_colsum_partials(M, m)][m] fp32 scratch; out: [m]
void launch_bn_lin_colsum(const bf16* a2, int M, int m, float* part, float* out, hipStream_t s) {
  const int P = bn_lin_colsum_partials(M, m);
  hipLaunchKernelGGL(bn_lin_colsum_kernel, dim3(P), dim3(256), 0, s, a2, M, m, part);
  launch_partial_sum(part, P, m, out, s);
}

// sums: [2][C] fp32, row 0 = S1 read, row 1 = S2 written; G: [C][m] fp32 = g^T a2; colsum: [m]
void launch_bn_lin_s2(const float* G, const bf16* w3, const float* colsum, const float* invstd, float inv_count,
                      int m, int C, float* sums, hipStream_t s) {
  hipLaunchKernelGGL(bn_lin_s2_kernel, dim3((C + 3) / 4), dim3(256), 0, s, G, w3, colsum, invstd, inv_count, m, C,
                     sums);
}

// coef: [3][C] fp32 scratch (kept for launch_bn_lin_dw); qpart: [bn_lin_q_slices(m, C)][m][m] fp32 scratch;
// wcat: [m][C + m] bf16; bias: [m] fp32
void launch_bn_lin_prep(const bf16* w3, const bf16* wt, const float* scale, const float* invstd, const float* sums,
                        const float* colsum, float inv_count, int m, int C, float* coef, float* qpart, bf16* wcat,
                        float* bias, hipStream_t s) {
  hipLaunchKernelGGL(bn_lin_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, s, scale, invstd, sums, inv_count, C,
                     coef);
  hipLaunchKernelGGL(bn_lin_scale_kernel, dim3((m * (C / 8) + 255) / 256), dim3(256), 0, s, wt, coef, m, C, wcat);
  const int slices = bn_lin_q_slices(m, C);
  const int cper = ((C / 64 + slices - 1) / slices) * 64;
  hipLaunchKernelGGL(bn_lin_q_kernel, dim3(m / 64, m / 32, slices), dim3(256), 0, s, w3, coef, m, C, cper, qpart);
  hipLaunchKernelGGL(bn_lin_q_round_kernel, dim3((m * m + 255) / 256), dim3(256), 0, s, qpart, slices, m, C, wcat);
  hipLaunchKernelGGL(bn_lin_bias_kernel, dim3((m + 3) / 4), dim3(256), 0, s, wt, wcat, coef, colsum, inv_count, m, C,
                     bias);
}

void launch_bn_lin_dw(const float* G, const float* A2, const bf16* w3, const float* coef, const float* colsum,
                      float inv_count, int m, int C, float* dw, hipStream_t s) {
  hipLaunchKernelGGL(bn_lin_dw_kernel, dim3(m / 64, C / 32), dim3(256), 0, s, G, A2, w3, coef, colsum, inv_count, m, C,
                     dw);
}

}  // namespace dcp

// Noise-robust classification losses in one row kernel: generalised cross-entropy (GCE, Zhang &
// Sabuncu 2018), symmetric cross-entropy (SCE, Wang et al. 2019) and early-learning regularisation
// (ELR, Liu et al. 2020).  With p = softmax(x), a the label, y its one-hot:
//
//   gce  loss = (1 - p_a^q) / q                          c = p_a^q
//   sce  loss = alpha (lse - x_a) + beta A (1 - p_a)     c = alpha + beta A p_a      A = -ln(1e-4)
//   elr  loss = (lse - x_a) + lam ln(1 - s)              c = 1
//
// gce / sce:  d_j = g c (p_j - y_j): cross-entropy's gradient times a row scalar.
// elr: T [N][C] fp32 holds a moving-average target per training sample, row b carries i = idx[b];
//   pc_j = clamp(p_j, 1e-4, 1 - 1e-4),  m_j = [1e-4 < p_j < 1 - 1e-4]
//   T_i <- mom T_i + (1 - mom) pc / sum(pc)              (the forward; a row touches only its own T_i)
//   s = sum_j pc_j T_ij,  s_m = sum_j m_j p_j T_ij       (on the updated T_i)
//   d_j = g [ (p_j - y_j) - lam / (1 - s) p_j (m_j T_ij - s_m) ]
// A row whose label is outside [0, C) (or, in elr, whose index is outside [0, N)) has loss 0 and a
// zero gradient row, and leaves T alone.  Pad columns C <= j < ldo of the gradient are 0.
//
// Forward, C <= 2048: one 64-lane wave owns a row and keeps it in registers, 32 values per lane,
// loaded 16 bytes at a time where the row's address allows (scalar otherwise and at the tail); a
// 256-thread workgroup carries four rows.  Max, sum-exp, the label's rank and the elr dots come from
// that one read, reduced with wave shuffles: no LDS, no barrier.  C > 2048: one workgroup per row as
// xent_fwd_kernel, re-reading the row, the same element functions and outputs.  Both write loss[b],
// rank[b] = #{j : x_j > x_a} and the fp64 record rec[b] = (lse, c, s, s_m).
// Backward: one streaming pass, no reduction, no LDS: p_j = exp(x_j - lse) from the saved lse.
//
// Bytes per row (e = 2 for bf16 logits, 4 for fp32; eo likewise for the gradient):
//   forward   C e read + 40 written               elr: + 4 C read + 4 C written (T_i)
//             (C > 2048: the row is read twice, under elr four times; the re-reads hit cache)
//   backward  C e + 32 read + ldo eo written      elr: + 4 C read (T_i)
// xent_fwd + xent_bwd read the row five times and write it once.  No atomics, no scratch; every
// hyper-parameter is a kernel argument and idx a device tensor, so a step is HIP-graph capturable.
#include "common.cuh"
#include "launchers.h"

namespace dcp {

namespace {

constexpr double kElrLo = 1e-4, kElrHi = 1.0 - 1e-4;
constexpr double kSceA = 9.210340371976182;  // -ln(1e-4)
constexpr int kRowRegs = 32;                 // values per lane of the register-resident forward
constexpr int kRowMaxC = kRowRegs * kWave;   // 2048

enum RobustMode { kGce = 0, kSce = 1, kElr = 2 };

struct RobustArgs {
  int mode;
  float a0, a1;  // gce: q, -   sce: alpha, beta   elr: lam, mom
};

template <typename T>
struct Chunk {
  static constexpr int kVec = 16 / (int)sizeof(T);  // elements of one 16-byte load
};

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// N contiguous elements at a 16-byte aligned address -> fp32
template <int N>
__device__ __forceinline__ void load_vec(const bf16* p, float* out) {
  static_assert(N == 8, "bf16 chunks are 8 wide");
  const bf16x8 u = *(const bf16x8*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = bf2f(u[e]);
}
template <int N>
__device__ __forceinline__ void load_vec(const float* p, float* out) {
#pragma unroll
  for (int k = 0; k < N / 4; ++k) {
    const f32x4 u = *(const f32x4*)(p + 4 * k);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[4 * k + e] = u[e];
  }
}
template <int N>
__device__ __forceinline__ void store_vec(float* p, const float* v) {
#pragma unroll
  for (int k = 0; k < N / 4; ++k) {
    f32x4 u;
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = v[4 * k + e];
    *(f32x4*)(p + 4 * k) = u;
  }
}
template <int N>
__device__ __forceinline__ void store_vec(bf16* p, const float* v) {
  if constexpr (N == 8) {
    bf16x8 u;
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] = f2bf(v[e]);
    *(bf16x8*)p = u;
  } else {
    static_assert(N == 4, "bf16 stores are 4 or 8 wide");
    bf16x4 u;
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = f2bf(v[e]);
    *(bf16x4*)p = u;  // 8 bytes: a multiple-of-4 column of a 16-byte aligned row
  }
}

// ---- the element functions shared by both forward shapes and the backward.  All arithmetic past the
// loads is fp64 and every output is rounded once: an fp32 lse alone is uncertain by half an ulp of a
// value near 5 (2.4e-7), and p = exp(x - lse) hands that to every class as a relative error, several ulps
// of the gradient.  The kernels stay bound by memory and launch, not by the fp64 exp (see the README).
__device__ __forceinline__ double prob(float x, double lse) { return exp((double)x - lse); }
__device__ __forceinline__ double elr_clamp(double p) { return fmin(fmax(p, kElrLo), kElrHi); }
__device__ __forceinline__ bool elr_inside(double p) { return p > kElrLo && p < kElrHi; }
__device__ __forceinline__ double elr_target(double t, double pc, double inv_sum, double mom) {
  return mom * t + (1.0 - mom) * (pc * inv_sum);
}
// one class of the elr dots on the updated target: s += pc t, s_m += m p t
__device__ __forceinline__ void elr_dots(double p, double pc, double t, double& s, double& sm) {
  s += pc * t;
  sm += elr_inside(p) ? p * t : 0.0;
}
// per-row loss and coefficient from ce = lse - x_a (and s under elr)
__device__ __forceinline__ void row_loss(const RobustArgs& a, double ce, double s, double& loss, double& c) {
  const double a0 = a.a0, a1 = a.a1;
  if (a.mode == kGce) {
    c = exp(-a0 * ce);  // p_a^q
    loss = -expm1(-a0 * ce) / a0;
  } else if (a.mode == kSce) {
    c = a0 + a1 * kSceA * exp(-ce);
    loss = a0 * ce - a1 * kSceA * expm1(-ce);
  } else {
    c = 1.0;
    loss = ce + a0 * log1p(-s);
  }
}
// one class of the gradient; gc = g c, k = lam / (1 - s) (0 outside elr)
__device__ __forceinline__ float grad_elem(float x, double lse, bool hot, double gc, double k, double t, double sm) {
  const double p = prob(x, lse);
  double d = p - (hot ? 1.0 : 0.0);
  d -= k * p * ((elr_inside(p) ? t : 0.0) - sm);
  return (float)(gc * d);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// workgroup-wide fp64 sum for 256 threads; `red` holds 4 doubles
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

// ---------------------------------------------------------------------------
// forward, C <= 2048: a wave per row, the row in registers
// ---------------------------------------------------------------------------
template <typename T, bool ELR>
__global__ void __launch_bounds__(256) robust_fwd_wave_kernel(const T* __restrict__ logits, int ld, int C, int B,
                                                              const int64_t* __restrict__ labels, RobustArgs a,
                                                              float* __restrict__ table, const int64_t* __restrict__ idx,
                                                              int64_t N, float* __restrict__ loss,
                                                              int* __restrict__ rank, double* __restrict__ rec) {
  constexpr int V = Chunk<T>::kVec, NCH = kRowRegs / V;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform, and there is no barrier below
  const T* row = logits + (size_t)b * ld;
  const int lab = (int)labels[b];
  bool valid = lab >= 0 && lab < C;
  const float xl = valid ? (float)row[lab] : 0.f;
  const bool xa = aligned16(row);
  float v[kRowRegs];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j0 = (c * kWave + lane) * V;
    if (xa && j0 + V <= C) {
      load_vec<V>(row + j0, v + c * V);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v[c * V + e] = j0 + e < C ? (float)row[j0 + e] : -INFINITY;
    }
  }
  float mx = -INFINITY;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < kRowRegs; ++r) {
    mx = fmaxf(mx, v[r]);
    cnt += v[r] > xl;
  }
  mx = wave_max(mx);
  cnt = wave_sum_int(cnt);
  double se = 0.0;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int e = 0; e < V; ++e)
      if ((c * kWave + lane) * V + e < C) se += exp((double)v[c * V + e] - (double)mx);
  se = wave_sum_d(se);
  const double lse = (double)mx + log(se);
  double s = 0.0, sm = 0.0;
  if constexpr (ELR) {
    const int64_t i = idx[b];
    valid = valid && i >= 0 && i < N;
    if (valid) {
      double spc = 0.0;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < V; ++e)
          if ((c * kWave + lane) * V + e < C) spc += elr_clamp(prob(v[c * V + e], lse));
      const double inv = 1.0 / wave_sum_d(spc);
      float* trow = table + (size_t)i * C;
      const bool ta = aligned16(trow);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j0 = (c * kWave + lane) * V;
        if (j0 >= C) continue;
        const bool vec = ta && j0 + V <= C;
        float t[V];
        if (vec) {
          load_vec<V>(trow + j0, t);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) t[e] = j0 + e < C ? trow[j0 + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (j0 + e < C) {
            const double p = prob(v[c * V + e], lse);
            const double pc = elr_clamp(p);
            t[e] = (float)elr_target(t[e], pc, inv, a.a1);
            elr_dots(p, pc, t[e], s, sm);  // on the target as stored: what the backward reads
          }
        }
        if (vec) {
          store_vec<V>(trow + j0, t);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (j0 + e < C) trow[j0 + e] = t[e];
        }
      }
      s = wave_sum_d(s);
      sm = wave_sum_d(sm);
    }
  }
  if (lane == 0) {
    double l, c;
    row_loss(a, lse - (double)xl, s, l, c);
    loss[b] = valid ? (float)l : 0.f;
    rank[b] = cnt;
    rec[4 * b + 0] = lse;
    rec[4 * b + 1] = c;
    rec[4 * b + 2] = s;
    rec[4 * b + 3] = sm;
  }
}

// ---------------------------------------------------------------------------
// forward, C > 2048: a workgroup per row, the row re-read (the shape of xent_fwd_kernel)
// ---------------------------------------------------------------------------
template <typename T, bool ELR>
__global__ void __launch_bounds__(256) robust_fwd_wg_kernel(const T* __restrict__ logits, int ld, int C, int B,
                                                            const int64_t* __restrict__ labels, RobustArgs a,
                                                            float* __restrict__ table, const int64_t* __restrict__ idx,
                                                            int64_t N, float* __restrict__ loss,
                                                            int* __restrict__ rank, double* __restrict__ rec) {
  __shared__ float red[16];
  __shared__ double redd[4];
  const int b = blockIdx.x;
  const T* row = logits + (size_t)b * ld;
  const int lab = (int)labels[b];
  bool valid = lab >= 0 && lab < C;
  const float xl = valid ? (float)row[lab] : 0.f;
  float mx = -INFINITY;
  int cnt = 0;
  for (int j = threadIdx.x; j < C; j += blockDim.x) {
    const float x = (float)row[j];
    mx = fmaxf(mx, x);
    cnt += x > xl;
  }
  mx = block_max(mx, red);
  double se = 0.0;
  for (int j = threadIdx.x; j < C; j += blockDim.x) se += exp((double)(float)row[j] - (double)mx);
  se = block_sum_d(se, redd);
  const float cntf = block_sum((float)cnt, red);  // exact: C < 2^24
  const double lse = (double)mx + log(se);
  double s = 0.0, sm = 0.0;
  if constexpr (ELR) {
    const int64_t i = idx[b];
    valid = valid && i >= 0 && i < N;  // workgroup-uniform
    if (valid) {
      double spc = 0.0;
      for (int j = threadIdx.x; j < C; j += blockDim.x) spc += elr_clamp(prob((float)row[j], lse));
      const double inv = 1.0 / block_sum_d(spc, redd);
      float* trow = table + (size_t)i * C;
      for (int j = threadIdx.x; j < C; j += blockDim.x) {
        const double p = prob((float)row[j], lse);
        const double pc = elr_clamp(p);
        const float t = (float)elr_target(trow[j], pc, inv, a.a1);
        trow[j] = t;
        elr_dots(p, pc, t, s, sm);
      }
      s = block_sum_d(s, redd);
      sm = block_sum_d(sm, redd);
    }
  }
  if (threadIdx.x == 0) {
    double l, c;
    row_loss(a, lse - (double)xl, s, l, c);
    loss[b] = valid ? (float)l : 0.f;
    rank[b] = (int)cntf;
    rec[4 * b + 0] = lse;
    rec[4 * b + 1] = c;
    rec[4 * b + 2] = s;
    rec[4 * b + 3] = sm;
  }
}

// ---------------------------------------------------------------------------
// backward: TPR threads stream one row (64: four rows per workgroup, C <= 2048; 256: one row)
// ---------------------------------------------------------------------------
template <typename T, typename TO, bool ELR, int TPR>
__global__ void __launch_bounds__(256) robust_bwd_kernel(const T* __restrict__ logits, int ld, int C, int B,
                                                         const int64_t* __restrict__ labels,
                                                         const double* __restrict__ rec, float lam,
                                                         const float* __restrict__ table,
                                                         const int64_t* __restrict__ idx, int64_t N,
                                                         const float* __restrict__ grad_out, float scale,
                                                         TO* __restrict__ dlogits, int ldo) {
  constexpr int V = Chunk<T>::kVec;
  const int b = blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
  if (b >= B) return;
  const int t0 = threadIdx.x % TPR;
  const T* row = logits + (size_t)b * ld;
  TO* drow = dlogits + (size_t)b * ldo;
  const int lab = (int)labels[b];
  bool valid = lab >= 0 && lab < C;
  const double lse = rec[4 * b + 0];
  double k = 0.0, sm = 0.0;
  const float* trow = nullptr;
  if constexpr (ELR) {
    const int64_t i = idx[b];
    valid = valid && i >= 0 && i < N;
    if (valid) {
      trow = table + (size_t)i * C;
      k = (double)lam / (1.0 - rec[4 * b + 2]);
      sm = rec[4 * b + 3];
    }
  }
  const double gc = valid ? (double)grad_out[0] * (double)scale * rec[4 * b + 1] : 0.0;
  const bool xa = aligned16(row), oa = aligned16(drow), ta = ELR && aligned16(trow);
  for (int j0 = t0 * V; j0 < ldo; j0 += TPR * V) {
    float x[V], t[V], d[V];
    if (xa && j0 + V <= C) {
      load_vec<V>(row + j0, x);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) x[e] = j0 + e < C ? (float)row[j0 + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) t[e] = 0.f;
    if constexpr (ELR) {
      if (valid) {
        if (ta && j0 + V <= C) {
          load_vec<V>(trow + j0, t);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) t[e] = j0 + e < C ? trow[j0 + e] : 0.f;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e)
      d[e] = (valid && j0 + e < C) ? grad_elem(x[e], lse, j0 + e == lab, gc, k, t[e], sm) : 0.f;
    if (oa && j0 + V <= ldo) {
      store_vec<V>(drow + j0, d);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (j0 + e < ldo) drow[j0 + e] = (TO)d[e];
    }
  }
}

// ---------------------------------------------------------------------------
template <typename T>
static void robust_fwd_t(const T* logits, int B, int ld, int C, const int64_t* labels, RobustArgs a, float* table,
                         const int64_t* idx, int64_t N, float* loss, int* rank, double* rec, hipStream_t s) {
  const bool elr = a.mode == kElr;
  if (C <= kRowMaxC) {
    const dim3 grid((B + 3) / 4), block(256);
    if (elr)
      hipLaunchKernelGGL((robust_fwd_wave_kernel<T, true>), grid, block, 0, s, logits, ld, C, B, labels, a, table, idx,
                         N, loss, rank, rec);
    else
      hipLaunchKernelGGL((robust_fwd_wave_kernel<T, false>), grid, block, 0, s, logits, ld, C, B, labels, a, table,
                         idx, N, loss, rank, rec);
  } else {
    if (elr)
      hipLaunchKernelGGL((robust_fwd_wg_kernel<T, true>), dim3(B), dim3(256), 0, s, logits, ld, C, B, labels, a, table,
                         idx, N, loss, rank, rec);
    else
      hipLaunchKernelGGL((robust_fwd_wg_kernel<T, false>), dim3(B), dim3(256), 0, s, logits, ld, C, B, labels, a,
                         table, idx, N, loss, rank, rec);
  }
}

void launch_xent_robust_fwd(const void* logits, bool is_bf16, int B, int ld, int C, const int64_t* labels, int mode,
                            float a0, float a1, float* table, const int64_t* idx, int64_t N, float* loss, int* rank,
                            double* rec, hipStream_t s) {
  if (B <= 0) return;
  const RobustArgs a{mode, a0, a1};
  if (is_bf16)
    robust_fwd_t((const bf16*)logits, B, ld, C, labels, a, table, idx, N, loss, rank, rec, s);
  else
    robust_fwd_t((const float*)logits, B, ld, C, labels, a, table, idx, N, loss, rank, rec, s);
}

template <typename T, typename TO>
static void robust_bwd_t(const T* logits, int B, int ld, int C, const int64_t* labels, const double* rec, bool elr,
                         float lam, const float* table, const int64_t* idx, int64_t N, const float* grad_out,
                         float scale, TO* d, int ldo, hipStream_t s) {
  if (C <= kRowMaxC) {
    const dim3 grid((B + 3) / 4), block(256);
    if (elr)
      hipLaunchKernelGGL((robust_bwd_kernel<T, TO, true, 64>), grid, block, 0, s, logits, ld, C, B, labels, rec, lam,
                         table, idx, N, grad_out, scale, d, ldo);
    else
      hipLaunchKernelGGL((robust_bwd_kernel<T, TO, false, 64>), grid, block, 0, s, logits, ld, C, B, labels, rec, lam,
                         table, idx, N, grad_out, scale, d, ldo);
  } else {
    if (elr)
      hipLaunchKernelGGL((robust_bwd_kernel<T, TO, true, 256>), dim3(B), dim3(256), 0, s, logits, ld, C, B, labels,
                         rec, lam, table, idx, N, grad_out, scale, d, ldo);
    else
      hipLaunchKernelGGL((robust_bwd_kernel<T, TO, false, 256>), dim3(B), dim3(256), 0, s, logits, ld, C, B, labels,
                         rec, lam, table, idx, N, grad_out, scale, d, ldo);
  }
}

void launch_xent_robust_bwd(const void* logits, bool in_bf16, int B, int ld, int C, const int64_t* labels,
                            const double* rec, int mode, float lam, const float* table, const int64_t* idx, int64_t N,
                            const float* grad_out, float scale, void* dlogits, int ldo, bool out_bf16,
                            hipStream_t s) {
  if (B <= 0) return;
  const bool elr = mode == kElr;
  if (in_bf16 && out_bf16)
    robust_bwd_t((const bf16*)logits, B, ld, C, labels, rec, elr, lam, table, idx, N, grad_out, scale,
                 (bf16*)dlogits, ldo, s);
  else if (in_bf16)
    robust_bwd_t((const bf16*)logits, B, ld, C, labels, rec, elr, lam, table, idx, N, grad_out, scale,
                 (float*)dlogits, ldo, s);
  else if (out_bf16)
    robust_bwd_t((const float*)logits, B, ld, C, labels, rec, elr, lam, table, idx, N, grad_out, scale,
                 (bf16*)dlogits, ldo, s);
  else
    robust_bwd_t((const float*)logits, B, ld, C, labels, rec, elr, lam, table, idx, N, grad_out, scale,
                 (float*)dlogits, ldo, s);
}

}  // namespace dcp

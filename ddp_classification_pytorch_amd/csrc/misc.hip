// Layout / conversion / small fused kernels:
//   * weight_prep: fp32 master weight [Co][T][Ci] -> bf16 GEMM copy [Co_pad][T][Ci]
//     and the transposed copy [Ci][T][Co_pad] used by the data-gradient pass
//     (LDS-tiled transpose, one launch per layer per step);
//   * to_nhwc: image batch (uint8 or fp32; NCHW or NHWC) -> normalised bf16
//     NHWC with zero-padded channels (replaces the
//     ToTensor+Normalize CPU transforms of BASELINE/main.py:58-76);
//   * relu_bwd, feature-mask (nested dropout, NESTED/train.py:247-252, K18);
//   * nested_eval: best-K search of TestNested (NESTED/train.py:103-166, K19)
//     as a prefix-cumulative classifier, with per-K top-1/top-3 counters and
//     nothing materialised (the reference builds a [feat_dim, B, C] tensor).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "common.cuh"
#include "launchers.h"

namespace dcp {

// Small host table (kernel argument lists) -> device, carried in the KERNEL ARGUMENTS instead of a
// host->device copy: a launch captured into a HIP graph replays with its arguments baked in, so
// tables built while a step is being captured (optimizer / weight-prep pointer lists) need no
// pinned staging buffer that outlives the capture.
constexpr int kFillWords = 448;  // 3584 bytes of kernel arguments per launch
struct FillArgs {
  int64_t v[kFillWords];
};

__global__ void __launch_bounds__(kFillWords) table_fill_kernel(const FillArgs a, int64_t* __restrict__ out, int n) {
  const int i = threadIdx.x;
  if (i < n) out[i] = a.v[i];
}

void launch_table_fill(const int64_t* host, int64_t n, int64_t* out, hipStream_t s) {
  for (int64_t o = 0; o < n; o += kFillWords) {
    FillArgs a;
    const int k = (int)std::min<int64_t>(kFillWords, n - o);
    for (int i = 0; i < k; ++i) a.v[i] = host[o + i];
    hipLaunchKernelGGL(table_fill_kernel, dim3(1), dim3(kFillWords), 0, s, a, out + o, k);
  }
}

__global__ void __launch_bounds__(256) weight_prep_kernel(const float* __restrict__ w, int Co, int T, int Ci,
                                                          int Co_pad, bf16* __restrict__ wb, bf16* __restrict__ wt) {
  // block: 64 (co) x 64 (ci) tile of tap t
  __shared__ float tile[64][65];
  const int ci0 = blockIdx.x * 64, co0 = blockIdx.y * 64, t = blockIdx.z;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 4 rows per pass
  for (int r = ty; r < 64; r += 4) {
    const int co = co0 + r, ci = ci0 + tx;
    float v = 0.f;
    if (co < Co && ci < Ci) v = w[((size_t)co * T + t) * Ci + ci];
    tile[r][tx] = v;
    if (co < Co_pad && ci < Ci) wb[((size_t)co * T + t) * Ci + ci] = f2bf(v);
  }
  if (!wt) return;
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < Ci && co < Co_pad) wt[((size_t)ci * T + t) * Co_pad + co] = f2bf(tile[tx][r]);
  }
}

// Multi-tensor weight_prep: every conv / linear weight of the model in ONE launch
// (one block per (weight, tap, 64x64 tile) from a host-built block list), run once
// per optimizer step instead of one launch per layer.  Source rows may be narrower
// than the destination (stem: Ci_src = 3 zero-padded to Ci = 8).
struct WPEntry {
  const float* w;
  bf16* wb;
  bf16* wt;
  int Co, T, Ci_src, Ci, Cp, tci, tco, pad_;
};

__global__ void __launch_bounds__(256) mt_weight_prep_kernel(const WPEntry* __restrict__ entries,
                                                             const int2* __restrict__ blocks) {
  __shared__ float tile[64][65];
  const int2 b = blocks[blockIdx.x];
  const WPEntry e = entries[b.x];
  const int per_t = e.tci * e.tco;
  const int t = b.y / per_t, rr = b.y - t * per_t;
  const int co0 = (rr / e.tci) * 64, ci0 = (rr % e.tci) * 64;
  // 4-wide path (uniform per block): 16-byte fp32 loads, 8-byte bf16 stores in both layouts (the
  // 2-byte-per-lane stores of the scalar path ran the whole-model refresh at ~3.9 TB/s); every
  // 4-group is then wholly inside or outside each bound.  The stem (Ci_src 3) takes the scalar path.
  const bool vec = ((e.Ci_src | e.Ci | e.Cp) & 3) == 0 &&
                   (((uintptr_t)e.w & 15u) | ((uintptr_t)e.wb & 7u) | ((uintptr_t)e.wt & 7u)) == 0;
  if (vec) {
    const int c4 = (threadIdx.x & 15) * 4, rw = threadIdx.x >> 4;  // 16 rows per pass
#pragma unroll
    for (int r = rw; r < 64; r += 16) {
      const int co = co0 + r, ci = ci0 + c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (co < e.Co && ci < e.Ci_src) v = *(const float4*)(e.w + ((size_t)co * e.T + t) * e.Ci_src + ci);
      tile[r][c4] = v.x;
      tile[r][c4 + 1] = v.y;
      tile[r][c4 + 2] = v.z;
      tile[r][c4 + 3] = v.w;
      if (co < e.Cp && ci < e.Ci)
        *(bf16x4*)(e.wb + ((size_t)co * e.T + t) * e.Ci + ci) = bf16x4{f2bf(v.x), f2bf(v.y), f2bf(v.z), f2bf(v.w)};
    }
    if (!e.wt) return;
    __syncthreads();
#pragma unroll
    for (int r = rw; r < 64; r += 16) {
      const int ci = ci0 + r, co = co0 + c4;
      if (ci < e.Ci && co < e.Cp)
        *(bf16x4*)(e.wt + ((size_t)ci * e.T + t) * e.Cp + co) =
            bf16x4{f2bf(tile[c4][r]), f2bf(tile[c4 + 1][r]), f2bf(tile[c4 + 2][r]), f2bf(tile[c4 + 3][r])};
    }
    return;
  }
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int co = co0 + r, ci = ci0 + tx;
    float v = 0.f;
    if (co < e.Co && ci < e.Ci_src) v = e.w[((size_t)co * e.T + t) * e.Ci_src + ci];
    tile[r][tx] = v;
    if (co < e.Cp && ci < e.Ci) e.wb[((size_t)co * e.T + t) * e.Ci + ci] = f2bf(v);
  }
  if (!e.wt) return;
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int ci = ci0 + r, co = co0 + tx;
    if (ci < e.Ci && co < e.Cp) e.wt[((size_t)ci * e.T + t) * e.Cp + co] = f2bf(tile[tx][r]);
  }
}

void launch_mt_weight_prep(const void* entries, const void* blocks, int nblocks, hipStream_t s) {
  if (nblocks <= 0) return;
  hipLaunchKernelGGL(mt_weight_prep_kernel, dim3(nblocks), dim3(256), 0, s, (const WPEntry*)entries,
                     (const int2*)blocks);
}

// src: [N][C][H][W] (nchw) or [N][H][W][C]; dtype u8 (is_u8) or fp32
// dst: [N][H][W][Cp] bf16 = (src*in_scale - mean[c]) / std[c], zero for c >= C
__global__ void __launch_bounds__(256) to_nhwc_kernel(const void* __restrict__ src, int is_u8, int nchw, int N,
                                                      int C, int H, int W, int Cp, float in_scale,
                                                      const float* __restrict__ mean, const float* __restrict__ stdv,
                                                      bf16* __restrict__ dst) {
  const size_t total = (size_t)N * H * W * Cp;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cp);
    const size_t pix = i / Cp;
    float v = 0.f;
    if (c < C) {
      const size_t hw = pix % ((size_t)H * W);
      const size_t n = pix / ((size_t)H * W);
      const size_t si = nchw ? (n * C + c) * (size_t)H * W + hw : pix * C + c;
      const float raw = is_u8 ? (float)((const uint8_t*)src)[si] : ((const float*)src)[si];
      v = (raw * in_scale - (mean ? mean[c] : 0.f)) / (stdv ? stdv[c] : 1.f);
    }
    dst[i] = f2bf(v);
  }
}

// backward of an activation from its OUTPUT y: 1 ReLU (y>0), 2 sigmoid (y(1-y))
__global__ void __launch_bounds__(256) act_bwd_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ y,
                                                      bf16* __restrict__ dx, size_t n8, int act) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const bf16x8 g = *(const bf16x8*)(dy + i * 8);
    const bf16x8 v = *(const bf16x8*)(y + i * 8);
    bf16x8 o;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float yv = bf2f(v[q]);
      const float d = act == 2 ? yv * (1.f - yv) : (yv > 0.f ? 1.f : 0.f);
      o[q] = f2bf(bf2f(g[q]) * d);
    }
    *(bf16x8*)(dx + i * 8) = o;
  }
}

// y[b][d] = x[b][d] * (d < keep) for keep = k+1 (nested dropout prefix mask)
__global__ void __launch_bounds__(256) prefix_mask_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int B,
                                                          int D, const int* __restrict__ keep) {
  const int kp = keep[0];
  const size_t total = (size_t)B * D;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int d = (int)(i % D);
    y[i] = d < kp ? x[i] : f2bf(0.f);
  }
}

// TestNested (NESTED/train.py:103-166, K19): for every prefix length k + 1 (k = 0..D-1) the
// scores s_k[b][c] = sum_{d<=k} f[b][d] W[d][c] of every validation sample, and whether the label
// ranks first / in the top 3: count[k][0] += (no class scores above the label), count[k][1] +=
// (fewer than three do).  Scores are sequential fp32 fma chains over d (s = fma(f_d, w_d, s)), in
// every kernel below, so all of them count exactly the same ranks; ties go to the label.
//
// nested_eval_scalar_kernel: one workgroup per sample, a block reduction per feature dimension
// (the round-4 kernel; kept as the reference the fast path is tested against).
constexpr int kNestedMaxPerThread = 16;  // C <= 4096
__global__ void __launch_bounds__(256) nested_eval_scalar_kernel(const float* __restrict__ feat,
                                                                 const float* __restrict__ W,
                                                                 const int64_t* __restrict__ labels, int D, int C,
                                                                 int* __restrict__ counts) {
  __shared__ float red[16];
  __shared__ float slab;
  const int b = blockIdx.x;
  const int lab = (int)labels[b];
  float s[kNestedMaxPerThread];
#pragma unroll
  for (int q = 0; q < kNestedMaxPerThread; ++q) s[q] = 0.f;
  const float* f = feat + (size_t)b * D;
  for (int d = 0; d < D; ++d) {
    const float fd = f[d];
    const float* wr = W + (size_t)d * C;
#pragma unroll
    for (int q = 0; q < kNestedMaxPerThread; ++q) {
      const int j = threadIdx.x + q * 256;
      if (j < C) s[q] = fmaf(fd, wr[j], s[q]);
    }
#pragma unroll
    for (int q = 0; q < kNestedMaxPerThread; ++q)
      if (threadIdx.x + q * 256 == lab) slab = s[q];
    __syncthreads();
    const float sl = slab;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < kNestedMaxPerThread; ++q) {
      const int j = threadIdx.x + q * 256;
      if (j < C && j != lab) cnt += s[q] > sl;  // ties resolved in favour of the label
    }
    const float rank = block_sum((float)cnt, red);
    if (threadIdx.x == 0) {
      if (rank < 0.5f) atomicAdd(&counts[2 * d], 1);
      if (rank < 2.5f) atomicAdd(&counts[2 * d + 1], 1);
    }
  }
}

// Fast path, three launches.
// (1) the label's own score chain L[b][d] (one wave per sample: 64 dims loaded at once, the chain
//     itself serial over d -- the same fma order as every class's score);
__global__ void __launch_bounds__(64) nested_label_prefix_kernel(const float* __restrict__ feat,
                                                                 const float* __restrict__ W,
                                                                 const int64_t* __restrict__ labels, int D, int C,
                                                                 float* __restrict__ L) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int lab = (int)labels[b];
  const float* f = feat + (size_t)b * D;
  float acc = 0.f;
  for (int d0 = 0; d0 < D; d0 += 64) {
    const int d = d0 + lane;
    const float fv = d < D ? f[d] : 0.f;
    const float wv = d < D ? W[(size_t)d * C + lab] : 0.f;
    float out = 0.f;
    const int n = min(64, D - d0);
    for (int i = 0; i < n; ++i) {
      const float fi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(fv), i));
      const float wi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), i));
      acc = fmaf(fi, wi, acc);
      out = lane == i ? acc : out;
    }
    if (d < D) L[(size_t)b * D + d] = out;
  }
}

// (2) ranks: a lane owns one class for NB samples, a wave 64 classes, a workgroup 4 waves (256
//     classes) x NB samples.  Per dimension d and sample: one fma per lane, then the wave's count
//     of classes scoring above the label is a ballot + popcount (the label's lane and classes past
//     C masked out), kept in lane d % 64 of a count register; per 64 dimensions the
//     four waves' counts are summed through LDS and stored: gt[class block][b][d].  The 64 weight
//     values of a chunk are loaded before its dimension loop (all in flight together).
template <int NB>
__global__ void __launch_bounds__(256) nested_rank_kernel(const float* __restrict__ feat, const float* __restrict__ W,
                                                          const int64_t* __restrict__ labels,
                                                          const float* __restrict__ L, int B, int D, int C,
                                                          int* __restrict__ gt) {
  __shared__ float fs[NB][64];
  __shared__ float ls[NB][64];
  __shared__ int red[4][NB][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x * 256 + wave * 64 + lane;
  const int b0 = blockIdx.y * NB;
  const bool cok = c < C;
  uint64_t valid[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int b = b0 + j;
    const int lab = b < B ? (int)labels[b] : -1;
    valid[j] = __ballot(cok && c != lab && b < B);
  }
  float s[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) s[j] = 0.f;
  const int cc = cok ? c : 0;
  for (int d0 = 0; d0 < D; d0 += 64) {
    const int n = min(64, D - d0);
    __syncthreads();  // the previous chunk's fs / ls / red reads are done
    for (int i = tid; i < NB * 64; i += 256) {
      const int j = i >> 6, dd = i & 63, b = b0 + j, d = d0 + dd;
      const bool ok = b < B && d < D;
      fs[j][dd] = ok ? feat[(size_t)b * D + d] : 0.f;
      ls[j][dd] = ok ? L[(size_t)b * D + d] : 0.f;
    }
    __syncthreads();
    int cnt[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) cnt[j] = 0;
    // 8 dimensions per step; the next step's 8 weights are loaded behind this step's work
    float w[8], wn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = (e < n && cok) ? W[(size_t)(d0 + e) * C + cc] : 0.f;
#pragma unroll 1
    for (int e0 = 0; e0 < n; e0 += 8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int dd = e0 + 8 + e;
        wn[e] = (dd < n && cok) ? W[(size_t)(d0 + dd) * C + cc] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int dd = e0 + e;
        if (dd < n) {
          const bool mine = lane == dd;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            s[j] = fmaf(fs[j][dd], w[e], s[j]);
            const int k = __popcll(__ballot(s[j] > ls[j][dd]) & valid[j]);
            cnt[j] = mine ? k : cnt[j];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = wn[e];
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) red[wave][j][lane] = cnt[j];
    __syncthreads();
    for (int i = tid; i < NB * 64; i += 256) {
      const int j = i >> 6, dd = i & 63, b = b0 + j, d = d0 + dd;
      if (b < B && d < D)
        gt[((size_t)blockIdx.x * B + b) * D + d] = red[0][j][dd] + red[1][j][dd] + red[2][j][dd] + red[3][j][dd];
    }
  }
}

// (3) per dimension: a sample's rank is the sum of its class blocks' counts; count the samples
//     whose label ranks first / in the top three (one thread per d and 4 samples, one atomic pair)
__global__ void __launch_bounds__(256) nested_count_kernel(const int* __restrict__ gt, int X, int B, int D,
                                                           int* __restrict__ counts) {
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  const int b0 = blockIdx.y * 4;
  int top1 = 0, top3 = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int b = b0 + q;
    if (b < B) {
      int r = 0;
      for (int x = 0; x < X; ++x) r += gt[((size_t)x * B + b) * D + d];
      top1 += r == 0;
      top3 += r < 3;
    }
  }
  if (top1) atomicAdd(&counts[2 * d], top1);
  if (top3) atomicAdd(&counts[2 * d + 1], top3);
}

// y[c][r] = x[r][c], bf16, 64x64 LDS tiles
__global__ void __launch_bounds__(256) transpose2d_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int R,
                                                          int C) {
  __shared__ bf16 tile[64][66];
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4)
    if (r0 + r < R && c0 + tx < C) tile[r][tx] = x[(size_t)(r0 + r) * C + c0 + tx];
  __syncthreads();
  for (int c = ty; c < 64; c += 4)
    if (c0 + c < C && r0 + tx < R) y[(size_t)(c0 + c) * R + r0 + tx] = tile[tx][c];
}

// ---------------------------------------------------------------------------
void launch_transpose2d(const bf16* x, bf16* y, int R, int C, hipStream_t s) {
  hipLaunchKernelGGL(transpose2d_kernel, dim3((C + 63) / 64, (R + 63) / 64), dim3(256), 0, s, x, y, R, C);
}

void launch_weight_prep(const float* w, int Co, int T, int Ci, int Co_pad, bf16* wb, bf16* wt, hipStream_t s) {
  dim3 grid((Ci + 63) / 64, (Co_pad + 63) / 64, T);
  hipLaunchKernelGGL(weight_prep_kernel, grid, dim3(256), 0, s, w, Co, T, Ci, Co_pad, wb, wt);
}

// One thread per OUTPUT pixel, 16-byte stores: dst [N][H/S][W/S][S*S*Cq] with channel
// (py*S + px)*Cq + c = normalised src[n][c][i*S+py][j*S+px] (c < C, else 0).  S = 2 is the
// space-to-depth input of the 4x4 stride-1 form of the 7x7/2 stem (models/resnet.py), S = 4 /
// Cq = 3 TResNet's SpaceToDepth(4) stem input (models/tresnet.py; timm's channel order).
template <int S, int CQ>
__global__ void __launch_bounds__(256) to_nhwc_pix_kernel(const void* __restrict__ src, int is_u8, int nchw, int N,
                                                          int C, int H, int W, float in_scale,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ stdv, bf16* __restrict__ dst) {
  constexpr int OC = S * S * CQ;
  const int Ho = H / S, Wo = W / S;
  const size_t total = (size_t)N * Ho * Wo;
  float mu[CQ], is[CQ];
#pragma unroll
  for (int c = 0; c < CQ; ++c) {
    mu[c] = (c < C && mean) ? mean[c] : 0.f;
    is[c] = (c < C && stdv) ? 1.f / stdv[c] : 1.f;
  }
  // 32-bit index math (the host checks total < 2^31): 64-bit division is emulated on the GPU
  for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < (uint32_t)total; pix += gridDim.x * blockDim.x) {
    const int j = (int)(pix % (uint32_t)Wo);
    const uint32_t q = pix / (uint32_t)Wo;
    const int i = (int)(q % (uint32_t)Ho);
    const size_t n = q / (uint32_t)Ho;
    bf16 o[OC];
    if (S == 2 && is_u8 && nchw && (W & 1) == 0) {
      // uint8 NCHW (the benchmark / ToTensor layout): the two horizontal taps of a channel row
      // are adjacent bytes -- one 2-byte load each instead of two byte loads
#pragma unroll
      for (int c = 0; c < CQ; ++c)
#pragma unroll
        for (int py = 0; py < S; ++py) {
          float v0 = 0.f, v1 = 0.f;
          if (c < C) {
            const size_t si = ((n * C + c) * H + (size_t)i * S + py) * W + (size_t)j * S;
            const uint16_t two = *(const uint16_t*)((const uint8_t*)src + si);
            v0 = ((float)(two & 0xff) * in_scale - mu[c]) * is[c];
            v1 = ((float)(two >> 8) * in_scale - mu[c]) * is[c];
          }
          o[(py * S + 0) * CQ + c] = f2bf(v0);
          o[(py * S + 1) * CQ + c] = f2bf(v1);
        }
    } else
#pragma unroll
    for (int py = 0; py < S; ++py)
#pragma unroll
      for (int px = 0; px < S; ++px) {
        const size_t y = (size_t)i * S + py, x = (size_t)j * S + px;
#pragma unroll
        for (int c = 0; c < CQ; ++c) {
          float v = 0.f;
          if (c < C) {
            const size_t si = nchw ? ((n * C + c) * H + y) * W + x : ((n * H + y) * W + x) * C + c;
            const float raw = is_u8 ? (float)((const uint8_t*)src)[si] : ((const float*)src)[si];
            v = (raw * in_scale - mu[c]) * is[c];
          }
          o[(py * S + px) * CQ + c] = f2bf(v);
        }
      }
#pragma unroll
    for (int k = 0; k < OC / 8; ++k) {
      bf16x8 w;
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = o[k * 8 + e];
      *(bf16x8*)(dst + (size_t)pix * OC + k * 8) = w;
    }
  }
}

// The mixed form of to_nhwc_pix_kernel (Mixup / CutMix, data/mix.py): image n is mixed with image
// partner[n] of the same batch while it is normalised.  With na / nb the values the kernel above
// WRITES for the row's own and for the partner's source pixel (same expression, rounded to bf16 as
// there: the bits of the unmixed output):
//   inside box[n] = {y0, x0, y1, x1} (source pixels, half open):  v = nb
//   elsewhere:                                                    v = fmaf(blend, na, (1 - blend) * nb)
// and dst = f2bf(v): the blend of the two unmixed bf16 images, formed in fp32 and rounded once, so it
// is within one bf16 rounding of blend * A + (1 - blend) * B for the unmixed outputs A, B (blending
// the unrounded fp32 values instead would sit up to three roundings from that).  The decision is per SOURCE pixel: a 2x2 / 4x4 output block may straddle a
// box edge.  The plan of a row is read once per output pixel (uniform over a wave except where the
// wave spans two images).  A row with blend == 1 reads one image per pixel -- its partner inside the
// box, itself elsewhere, so the identity plan never touches a partner and costs the bytes of the
// unmixed kernel -- and takes na outside the box as it is (fmaf(1, na, 0 * nb) for every finite nb).
// partner is clamped into [0, N) and the box into the image, so no plan can address outside the batch.
template <int S, int CQ>
__global__ void __launch_bounds__(256) to_nhwc_pix_mix_kernel(const void* __restrict__ src, int is_u8, int nchw,
                                                              int N, int C, int H, int W, float in_scale,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ stdv,
                                                              const int* __restrict__ partner,
                                                              const float* __restrict__ blend,
                                                              const int* __restrict__ box, bf16* __restrict__ dst) {
  constexpr int OC = S * S * CQ;
  const int Ho = H / S, Wo = W / S;
  const size_t total = (size_t)N * Ho * Wo;
  float mu[CQ], is[CQ];
#pragma unroll
  for (int c = 0; c < CQ; ++c) {
    mu[c] = (c < C && mean) ? mean[c] : 0.f;
    is[c] = (c < C && stdv) ? 1.f / stdv[c] : 1.f;
  }
  for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < (uint32_t)total; pix += gridDim.x * blockDim.x) {
    const int j = (int)(pix % (uint32_t)Wo);
    const uint32_t q = pix / (uint32_t)Wo;
    const int i = (int)(q % (uint32_t)Ho);
    const uint32_t ni = q / (uint32_t)Ho;
    const size_t n = ni;
    const size_t m = (size_t)min(max(partner[ni], 0), N - 1);
    const float bl = blend[ni];
    const float cb = 1.f - bl;
    const int by0 = min(max(box[4 * ni + 0], 0), H), bx0 = min(max(box[4 * ni + 1], 0), W);
    const int by1 = min(max(box[4 * ni + 2], 0), H), bx1 = min(max(box[4 * ni + 3], 0), W);
    const bool boxed = by1 > by0 && bx1 > bx0;
    const bool blended = bl != 1.f;
    bf16 o[OC];
    // Every pixel loads its first operand unconditionally, as the unmixed kernel does, from the image
    // it comes from (the partner inside the box, the row's own elsewhere); only a blending row
    // (uniform per image) loads the partner's pixel as a second operand.
    if (S == 2 && is_u8 && nchw && (W & 1) == 0) {
      // the packed two-byte load of the unmixed kernel; a pair that straddles a box edge loads twice
#pragma unroll
      for (int py = 0; py < S; ++py) {
        const int y = i * S + py, x = j * S;
        const bool iny = boxed && y >= by0 && y < by1;
        const bool in0 = iny && x >= bx0 && x < bx1, in1 = iny && x + 1 >= bx0 && x + 1 < bx1;
        const size_t f0 = in0 ? m : n, f1 = in1 ? m : n;
#pragma unroll
        for (int c = 0; c < CQ; ++c) {
          float v0 = 0.f, v1 = 0.f;
          if (c < C) {
            const size_t off = ((size_t)c * H + (size_t)y) * W + (size_t)x;
            const size_t img = (size_t)C * H * W;
            const uint16_t t0 = *(const uint16_t*)((const uint8_t*)src + f0 * img + off);
            const uint16_t t1 = f1 == f0 ? t0 : *(const uint16_t*)((const uint8_t*)src + f1 * img + off);
            v0 = ((float)(t0 & 0xff) * in_scale - mu[c]) * is[c];
            v1 = ((float)(t1 >> 8) * in_scale - mu[c]) * is[c];
            if (blended) {
              const uint16_t tb = *(const uint16_t*)((const uint8_t*)src + m * img + off);
              const float nb0 = ((float)(tb & 0xff) * in_scale - mu[c]) * is[c];
              const float nb1 = ((float)(tb >> 8) * in_scale - mu[c]) * is[c];
              v0 = in0 ? nb0 : fmaf(bl, bf2f(f2bf(v0)), cb * bf2f(f2bf(nb0)));
              v1 = in1 ? nb1 : fmaf(bl, bf2f(f2bf(v1)), cb * bf2f(f2bf(nb1)));
            }
          }
          o[(py * S + 0) * CQ + c] = f2bf(v0);
          o[(py * S + 1) * CQ + c] = f2bf(v1);
        }
      }
    } else
#pragma unroll
    for (int py = 0; py < S; ++py)
#pragma unroll
      for (int px = 0; px < S; ++px) {
        const size_t y = (size_t)i * S + py, x = (size_t)j * S + px;
        const bool in = boxed && (int)y >= by0 && (int)y < by1 && (int)x >= bx0 && (int)x < bx1;
        const size_t f = in ? m : n;
#pragma unroll
        for (int c = 0; c < CQ; ++c) {
          float v = 0.f;
          if (c < C) {
            const size_t si = nchw ? ((f * C + c) * H + y) * W + x : ((f * H + y) * W + x) * C + c;
            const float raw = is_u8 ? (float)((const uint8_t*)src)[si] : ((const float*)src)[si];
            v = (raw * in_scale - mu[c]) * is[c];
            if (blended) {
              const size_t sb = nchw ? ((m * C + c) * H + y) * W + x : ((m * H + y) * W + x) * C + c;
              const float rawb = is_u8 ? (float)((const uint8_t*)src)[sb] : ((const float*)src)[sb];
              const float nb = (rawb * in_scale - mu[c]) * is[c];
              v = in ? nb : fmaf(bl, bf2f(f2bf(v)), cb * bf2f(f2bf(nb)));
            }
          }
          o[(py * S + px) * CQ + c] = f2bf(v);
        }
      }
#pragma unroll
    for (int k = 0; k < OC / 8; ++k) {
      bf16x8 w;
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = o[k * 8 + e];
      *(bf16x8*)(dst + (size_t)pix * OC + k * 8) = w;
    }
  }
}

// block 2: [N][H/2][W/2][16] (2x2, 4 channel slots: the ResNet s2d stem); block 4:
// [N][H/4][W/4][48] (4x4, 3 channels: TResNet's SpaceToDepth(4) stem, written straight from the
// images instead of an NHWC pass plus a space_to_depth pass)
void launch_to_nhwc_s2d(const void* src, int is_u8, int nchw, int N, int C, int H, int W, float in_scale,
                        const float* mean, const float* stdv, bf16* dst, hipStream_t s, int block) {
  size_t total = (size_t)N * (H / block) * (W / block);
  if (total >= (1ull << 31)) {
    fprintf(stderr, "to_nhwc_s2d: %zu output pixels exceed the 32-bit index range\n", total);
    abort();
  }
  size_t g = (total + 255) / 256;
  if (g > (1u << 20)) g = 1u << 20;
  if (block == 4)
    hipLaunchKernelGGL((to_nhwc_pix_kernel<4, 3>), dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W,
                       in_scale, mean, stdv, dst);
  else
    hipLaunchKernelGGL((to_nhwc_pix_kernel<2, 4>), dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W,
                       in_scale, mean, stdv, dst);
}

void launch_to_nhwc(const void* src, int is_u8, int nchw, int N, int C, int H, int W, int Cp, float in_scale,
                    const float* mean, const float* stdv, bf16* dst, hipStream_t s) {
  if (Cp == 8 && C <= 8) {
    size_t total = (size_t)N * H * W;
    if (total >= (1ull << 31)) {
      fprintf(stderr, "to_nhwc: %zu pixels exceed the 32-bit index range\n", total);
      abort();
    }
    size_t g = (total + 255) / 256;
    if (g > (1u << 20)) g = 1u << 20;
    hipLaunchKernelGGL((to_nhwc_pix_kernel<1, 8>), dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W,
                       in_scale, mean, stdv, dst);
    return;
  }
  size_t total = (size_t)N * H * W * Cp;
  size_t g = (total + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(to_nhwc_kernel, dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W, Cp, in_scale, mean,
                     stdv, dst);
}

// The mixed input kernels: block 0 the plain 8-slot NHWC layout, 2 / 4 the space-to-depth stems.
// Returns 0, or 1 when the output pixels exceed the 32-bit index range (nothing is launched).
int launch_to_nhwc_mix(const void* src, int is_u8, int nchw, int N, int C, int H, int W, float in_scale,
                       const float* mean, const float* stdv, const int* partner, const float* blend, const int* box,
                       bf16* dst, hipStream_t s, int block) {
  const int b = block ? block : 1;
  size_t total = (size_t)N * (H / b) * (W / b);
  if (total >= (1ull << 31)) return 1;
  if (total == 0) return 0;
  size_t g = (total + 255) / 256;
  if (g > (1u << 20)) g = 1u << 20;
  if (block == 4)
    hipLaunchKernelGGL((to_nhwc_pix_mix_kernel<4, 3>), dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W,
                       in_scale, mean, stdv, partner, blend, box, dst);
  else if (block == 2)
    hipLaunchKernelGGL((to_nhwc_pix_mix_kernel<2, 4>), dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W,
                       in_scale, mean, stdv, partner, blend, box, dst);
  else
    hipLaunchKernelGGL((to_nhwc_pix_mix_kernel<1, 8>), dim3((int)g), dim3(256), 0, s, src, is_u8, nchw, N, C, H, W,
                       in_scale, mean, stdv, partner, blend, box, dst);
  return 0;
}

void launch_act_bwd(const bf16* dy, const bf16* y, bf16* dx, size_t numel, int act, hipStream_t s) {
  const size_t n8 = numel / 8;
  size_t g = (n8 + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(act_bwd_kernel, dim3((int)g), dim3(256), 0, s, dy, y, dx, n8, act);
}

void launch_prefix_mask(const bf16* x, bf16* y, int B, int D, const int* keep, hipStream_t s) {
  size_t total = (size_t)B * D;
  size_t g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(prefix_mask_kernel, dim3((int)g), dim3(256), 0, s, x, y, B, D, keep);
}

void launch_nested_eval_scalar(const float* feat, const float* W, const int64_t* labels, int B, int D, int C,
                               int* counts, hipStream_t s) {
  hipLaunchKernelGGL(nested_eval_scalar_kernel, dim3(B), dim3(256), 0, s, feat, W, labels, D, C, counts);
}

size_t nested_eval_workspace(int B, int D, int C) {
  return (size_t)B * D * sizeof(float) + (size_t)((C + 255) / 256) * B * D * sizeof(int);
}

void launch_nested_eval(const float* feat, const float* W, const int64_t* labels, int B, int D, int C, int* counts,
                        void* ws, hipStream_t s) {
  // 2 samples per workgroup: ~2,300 waves at the reference's val batch of 128 (the per-dimension
  // fma -> ballot -> popcount chain is latency-bound below a few waves per SIMD; the weight
  // matrix is re-read per sample pair from L2 / the Infinity Cache)
  constexpr int NB = 2;
  float* L = (float*)ws;
  int* gt = (int*)((char*)ws + (size_t)B * D * sizeof(float));
  const int X = (C + 255) / 256;
  hipLaunchKernelGGL(nested_label_prefix_kernel, dim3(B), dim3(64), 0, s, feat, W, labels, D, C, L);
  hipLaunchKernelGGL(nested_rank_kernel<NB>, dim3(X, (B + NB - 1) / NB), dim3(256), 0, s, feat, W, labels, L, B, D, C,
                     gt);
  hipLaunchKernelGGL(nested_count_kernel, dim3((D + 255) / 256, (B + 3) / 4), dim3(256), 0, s, gt, X, B, D, counts);
}


// ---------------------------------------------------------------------------
// Dropout (NESTED --dropout, NESTED/train.py:252; VGG classifier) with a
// counter-based Philox-4x32-10 mask: element i of call `offset` keeps iff the uniform drawn from
// counter (i / 4, 0, offset) under key `seed` is >= p.  The backward regenerates the same mask
// from (seed, offset) -- nothing is stored.  The call offset lives in a device counter the
// launcher bumps after the kernel (so a HIP-graph replay draws a fresh mask every replay); the
// kernel copies the value it used to `used` for the backward.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

template <typename T>
__device__ __forceinline__ float ld_f(const T* p, size_t i) {
  if constexpr (sizeof(T) == 2) return bf2f(((const bf16*)p)[i]);
  else return ((const float*)p)[i];
}
template <typename T>
__device__ __forceinline__ void st_f(T* p, size_t i, float v) {
  if constexpr (sizeof(T) == 2) ((bf16*)p)[i] = f2bf(v);
  else ((float*)p)[i] = v;
}

template <typename T>
__global__ void __launch_bounds__(256) dropout_kernel(const T* __restrict__ x, T* __restrict__ y, size_t n, float p,
                                                      uint64_t seed, const int64_t* __restrict__ offset_ptr,
                                                      int64_t* __restrict__ used) {
  const uint64_t off = (uint64_t)*offset_ptr;
  if (used && blockIdx.x == 0 && threadIdx.x == 0) *used = (int64_t)off;
  const float scale = 1.f / (1.f - p);
  const size_t n4 = (n + 3) / 4;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (size_t)gridDim.x * 256) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)(q >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t i = q * 4 + e;
      if (i < n) {
        const float u = (float)(c[e] >> 8) * (1.f / 16777216.f);
        st_f(y, i, u >= p ? ld_f(x, i) * scale : 0.f);
      }
    }
  }
}

void launch_dropout(const void* x, void* y, size_t n, int is_bf16, float p, uint64_t seed, const int64_t* offset_ptr,
                    int64_t* used, hipStream_t s) {
  size_t g = ((n + 3) / 4 + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  if (is_bf16)
    hipLaunchKernelGGL(dropout_kernel<bf16>, dim3((int)g), dim3(256), 0, s, (const bf16*)x, (bf16*)y, n, p, seed,
                       offset_ptr, used);
  else
    hipLaunchKernelGGL(dropout_kernel<float>, dim3((int)g), dim3(256), 0, s, (const float*)x, (float*)y, n, p, seed,
                       offset_ptr, used);
}

// ---------------------------------------------------------------------------
// InplaceABN effective weight (mapillary inplace_abn, X3/K21): g_eff = |g| + eps and its
// reciprocal in one launch; backward dg = dg_eff * sign(g) (one launch) -- instead of the abs / add
// / reciprocal / sgn / mul ATen chain per layer
// ---------------------------------------------------------------------------
__global__ void iabn_gamma_kernel(const float* __restrict__ g, float eps, float* __restrict__ geff,
                                  float* __restrict__ rg, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float e = fabsf(g[c]) + eps;
  geff[c] = e;
  rg[c] = 1.f / e;
}

__global__ void sign_mul_kernel(const float* __restrict__ d, const float* __restrict__ g, float* __restrict__ out,
                                int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float v = g[c];
  out[c] = v > 0.f ? d[c] : (v < 0.f ? -d[c] : 0.f);
}

void launch_iabn_gamma(const float* g, float eps, float* geff, float* rg, int C, hipStream_t s) {
  hipLaunchKernelGGL(iabn_gamma_kernel, dim3((C + 255) / 256), dim3(256), 0, s, g, eps, geff, rg, C);
}

void launch_sign_mul(const float* d, const float* g, float* out, int C, hipStream_t s) {
  hipLaunchKernelGGL(sign_mul_kernel, dim3((C + 255) / 256), dim3(256), 0, s, d, g, out, C);
}


// ---------------------------------------------------------------------------
// The stem weight between its 7x7 / stride-2 master form [Co][7][7][C <= 4] and the 4x4 / stride-1
// form over the 2x2 space-to-depth input [Co][4][4][16] (ops/functional.py stem_s2d_weight):
//   w16[co][ta][tb][(py * 2 + px) * 4 + c] = w7[co][2 ta + py - 1][2 tb + px - 1][c]
// (0 outside the 7x7 window or past C).  Forward: refresh the persistent s2d buffer every step in
// one launch; backward: the 4x4 weight gradient back onto the 7x7 master (each 7x7 element has
// exactly one 4x4 image, so a gather).
__global__ void __launch_bounds__(256) s2d_weight_kernel(const float* __restrict__ w7, int Co, int C,
                                                         float* __restrict__ w16) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Co * 256) return;
  const int co = i >> 8, k = i & 255;
  const int ta = k >> 6, tb = (k >> 4) & 3, q = k & 15, py = q >> 3, px = (q >> 2) & 1, c = q & 3;
  const int kh = 2 * ta + py - 1, kw = 2 * tb + px - 1;
  const bool ok = kh >= 0 && kh < 7 && kw >= 0 && kw < 7 && c < C;
  w16[i] = ok ? w7[((co * 7 + kh) * 7 + kw) * C + c] : 0.f;
}

__global__ void __launch_bounds__(256) s2d_weight_bwd_kernel(const float* __restrict__ g16, int Co, int C,
                                                             float* __restrict__ g7) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Co * 49 * C) return;
  const int c = i % C, t = i / C, kw = t % 7, kh = (t / 7) % 7, co = t / 49;
  const int u = kh + 1, v = kw + 1;  // 8 x 8 padded index
  const int ta = u >> 1, py = u & 1, tb = v >> 1, px = v & 1;
  g7[i] = g16[co * 256 + ta * 64 + tb * 16 + (py * 2 + px) * 4 + c];
}

void launch_s2d_weight(const float* w7, int Co, int C, float* w16, hipStream_t s) {
  hipLaunchKernelGGL(s2d_weight_kernel, dim3((Co * 256 + 255) / 256), dim3(256), 0, s, w7, Co, C, w16);
}
void launch_s2d_weight_bwd(const float* g16, int Co, int C, float* g7, hipStream_t s) {
  hipLaunchKernelGGL(s2d_weight_bwd_kernel, dim3((Co * 49 * C + 255) / 256), dim3(256), 0, s, g16, Co, C, g7);
}

}  // namespace dcp

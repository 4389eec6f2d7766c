// Partial FC (An et al., CVPR 2022): the fused ArcFace head over a class subset drawn on the device.
//
// A step scores its rows against Cs of the C classes: the batch's own labels ("positives") and the
// Cs - |pos| other classes with the smallest pairs (h(c), c), h(c) = word 0 of
// Philox-4x32-10(counter = (c, 0, step), key = seed).  Cs is a host integer, so every shape is static;
// `step` is a device call counter, so a replayed HIP graph draws a new subset every replay.  Nothing
// here reads the host, no float atomics (integer atomics only: their results do not depend on order).
//
//   sampler   pfc_clear_kernel        zeroes the workspace (positives bitmap, 4 x 256 histograms, the
//                                     positives counter) and the -1 tail of idx
//             pfc_mark_kernel         one thread per row: sets its label's bit (atomicOr); the thread
//                                     that flipped the bit counts the class -> |pos|
//             pfc_hist_kernel<P>      pass P = 0..3 of an exact 4 x 8-bit radix select of the
//                                     need = Cs - |pos| smallest keys among the non-positive classes:
//                                     grid-stride over C, the key recomputed from Philox (never
//                                     stored), a 256-bin histogram of digit P of the keys that match
//                                     the prefix so far, per workgroup in LDS, merged by atomicAdd.
//                                     The prefix is not stored either: every workgroup re-derives it
//                                     from the earlier passes' global histograms (pfc_resolve: one
//                                     256-wide block scan per earlier pass), so a pass reads only what
//                                     earlier launches wrote
//             pfc_count_kernel        per 1024-class chunk: (sure, eq) = number of classes taken for
//                                     certain (positive, or key < threshold T) and of non-positive
//                                     classes with key == T (ties: the first need_eq by class id win)
//             pfc_scan_kernel         one workgroup: exclusive scan of both counts over the chunks
//             pfc_write_kernel        per chunk: block scan of the packed per-thread counts, then the
//                                     ordered write: idx[position] = c, slot[c] = position or -1
//             pfc_relabel_kernel      lab'[b] = slot[labels[b]] (-1 for an invalid label)
//   operand   arc_gather_l2norm_t_kernel   l2norm_t_tile (score_tile.cuh), as arc_l2norm_t_kernel, with
//                                     row r read from W[idx[r]]: a compact row has the bits the full
//                                     pass gives for that class; rows with idx = -1 are zero.  Reads
//                                     Cs rows of W, nothing else of [C, D]
//   head      launch_arcface_fused_fwd / _dx / _dw (arcface.hip, unchanged) on the compact operands
//             with lab' and C := Cs
//   scatter   arc_scatter_rows_kernel one wave per output row of the dense dW [C, D]: copies compact
//                                     row slot[c] or writes zeros; every element written exactly once
//
// Resources (hipcc -O3, gfx950; scratch 0 bytes everywhere):
//   pfc_hist_kernel<0..3>  VGPR 13 / 15 / 18 / 20, LDS 1024 B (+ 32 B for P > 0)
//   pfc_count_kernel       VGPR 24, LDS 32 B        pfc_write_kernel  VGPR 32, LDS 32 B
//   pfc_scan_kernel        VGPR 33, LDS 32 B        pfc_clear / _mark / _relabel  VGPR <= 6, LDS 0
//   arc_gather_l2norm_t_kernel<128 / 256 / 512>  VGPR 34 / 38 / 42, LDS 17 / 33 / 65 KB
//   arc_scatter_rows_kernel<1 / 4>  VGPR 12 / 16, LDS 0
#include "launchers.h"
#include "score_tile.cuh"

namespace dcp {

namespace {

constexpr int kPfcChunk = 1024;   // classes per compaction chunk: 256 threads x 4 consecutive classes
constexpr int kPfcMaxGrid = 2048; // grid-stride beyond this many workgroups

// workspace layout (int32 words): [0] |pos|, [16 .. 16 + 1024) the 4 histograms, then the positives
// bitmap ((C + 31) / 32 words), then the chunk counts / offsets (2 per chunk)
constexpr int kWsHist = 16, kWsBits = kWsHist + 4 * 256;

__host__ __device__ inline int pfc_words(int C) { return (C + 31) / 32; }
__host__ __device__ inline int pfc_chunks(int C) { return (C + kPfcChunk - 1) / kPfcChunk; }

__device__ __forceinline__ uint32_t pfc_key(uint32_t c, uint64_t step, uint64_t seed) {
  uint32_t v[4] = {c, 0u, (uint32_t)step, (uint32_t)(step >> 32)};
  philox4x32_10(v, (uint32_t)seed, (uint32_t)(seed >> 32));
  return v[0];
}

// inclusive scan over the 256 threads of a workgroup; red: 4 words of LDS.  -> (inclusive, total)
__device__ __forceinline__ uint32_t block_scan256(uint32_t v, uint32_t* red, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();  // (red may still be read from an earlier call)
  if (lane == 63) red[w] = v;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t t = red[i];
    base += i < w ? t : 0u;
    total += t;
  }
  return v + base;
}

// The state of the radix select after passes 0 .. P - 1, derived from their global histograms:
// prefix = the top 8 P bits of the threshold key, need = how many keys with that prefix are still to
// be taken (in key order).  Every thread of the workgroup gets the same values.  sh: 8 words of LDS.
template <int P>
__device__ __forceinline__ void pfc_resolve(const int* __restrict__ ws, int Cs, uint32_t* sh, uint32_t& prefix,
                                            uint32_t& need) {
  prefix = 0;
  need = (uint32_t)(Cs - ws[0]);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const uint32_t h = (uint32_t)ws[kWsHist + p * 256 + threadIdx.x];
    uint32_t total;
    const uint32_t incl = block_scan256(h, sh, total), excl = incl - h;
    // the digit whose bin holds the need-th smallest key (need = 0: nothing is taken, digit 0)
    if (need == 0 ? threadIdx.x == 0 : (excl < need && need <= incl)) {
      sh[4] = threadIdx.x;
      sh[5] = need == 0 ? 0u : excl;
    }
    __syncthreads();
    prefix = (prefix << 8) | sh[4];
    need -= sh[5];
  }
}

__device__ __forceinline__ bool pfc_is_pos(const int* __restrict__ ws, uint32_t c) {
  return (((const uint32_t*)ws)[kWsBits + (c >> 5)] >> (c & 31u)) & 1u;
}

}  // namespace

__global__ void __launch_bounds__(256) pfc_clear_kernel(int* __restrict__ ws, int nclear, int* __restrict__ idx,
                                                        int Cs, int Csp) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nclear; i += gridDim.x * 256) ws[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x < 64 && Cs + (int)threadIdx.x < Csp) idx[Cs + threadIdx.x] = -1;
}

__global__ void __launch_bounds__(256) pfc_mark_kernel(const int64_t* __restrict__ labels, int B, int C,
                                                       int* __restrict__ ws) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t y = labels[b];
  if (y < 0 || y >= C) return;
  const uint32_t bit = 1u << ((uint32_t)y & 31u);
  const uint32_t old = atomicOr((uint32_t*)ws + kWsBits + ((uint32_t)y >> 5), bit);
  if (!(old & bit)) atomicAdd(ws, 1);
}

template <int P>
__global__ void __launch_bounds__(256) pfc_hist_kernel(int* __restrict__ ws, int C, int Cs, uint64_t seed,
                                                       const int64_t* __restrict__ step_ptr) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh[8];
  const uint64_t step = (uint64_t)*step_ptr;
  uint32_t prefix, need;
  pfc_resolve<P>(ws, Cs, sh, prefix, need);
  hist[threadIdx.x] = 0;
  __syncthreads();
  if (need != 0) {  // (uniform; need = 0 takes no negative: the histograms stay zero)
    for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < (uint32_t)C; c += gridDim.x * 256u) {
      if (pfc_is_pos(ws, c)) continue;
      const uint32_t h = pfc_key(c, step, seed);
      bool match = true;
      if constexpr (P > 0) match = (h >> (32 - 8 * P)) == prefix;
      if (match) atomicAdd(&hist[(h >> (24 - 8 * P)) & 255u], 1u);
    }
  }
  __syncthreads();
  const uint32_t n = hist[threadIdx.x];
  if (n) atomicAdd(ws + kWsHist + P * 256 + threadIdx.x, (int)n);
}

// the 4 classes of a thread: flags -> packed count (sure in the low half, eq in the high half)
__device__ __forceinline__ uint32_t pfc_flags(const int* __restrict__ ws, uint32_t c0, int C, uint32_t T,
                                              uint64_t step, uint64_t seed, bool sure[4], bool eq[4]) {
  uint32_t packed = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t c = c0 + e;
    sure[e] = eq[e] = false;
    if (c < (uint32_t)C) {
      if (pfc_is_pos(ws, c)) {
        sure[e] = true;
      } else {
        const uint32_t h = pfc_key(c, step, seed);
        sure[e] = h < T;
        eq[e] = h == T;
      }
    }
    packed += (sure[e] ? 1u : 0u) + (eq[e] ? 0x10000u : 0u);
  }
  return packed;
}

__global__ void __launch_bounds__(256) pfc_count_kernel(int* __restrict__ ws, int C, int Cs, uint64_t seed,
                                                        const int64_t* __restrict__ step_ptr) {
  __shared__ uint32_t sh[8];
  const uint64_t step = (uint64_t)*step_ptr;
  uint32_t T, need_eq;
  pfc_resolve<4>(ws, Cs, sh, T, need_eq);
  int* cnt = ws + kWsBits + pfc_words(C);
  const int nchunks = pfc_chunks(C);
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    bool sure[4], eq[4];
    const uint32_t packed = pfc_flags(ws, (uint32_t)ch * kPfcChunk + 4u * threadIdx.x, C, T, step, seed, sure, eq);
    uint32_t total;
    block_scan256(packed, sh, total);
    if (threadIdx.x == 0) {
      cnt[2 * ch] = (int)(total & 0xFFFFu);
      cnt[2 * ch + 1] = (int)(total >> 16);
    }
  }
}

// one workgroup: cnt [nchunks][2] -> exclusive prefix sums of both columns, in place
__global__ void __launch_bounds__(256) pfc_scan_kernel(int* __restrict__ ws, int C) {
  __shared__ uint32_t sh[8];
  int* cnt = ws + kWsBits + pfc_words(C);
  const int nchunks = pfc_chunks(C);
  uint32_t carry0 = 0, carry1 = 0;
  for (int base = 0; base < nchunks; base += 256) {
    const int ch = base + (int)threadIdx.x;
    const uint32_t a = ch < nchunks ? (uint32_t)cnt[2 * ch] : 0u, b = ch < nchunks ? (uint32_t)cnt[2 * ch + 1] : 0u;
    uint32_t ta, tb;
    const uint32_t ia = block_scan256(a, sh, ta);
    const uint32_t ib = block_scan256(b, sh, tb);
    if (ch < nchunks) {
      cnt[2 * ch] = (int)(carry0 + ia - a);
      cnt[2 * ch + 1] = (int)(carry1 + ib - b);
    }
    carry0 += ta;
    carry1 += tb;
  }
}

__global__ void __launch_bounds__(256) pfc_write_kernel(const int* __restrict__ ws, int C, int Cs, uint64_t seed,
                                                        const int64_t* __restrict__ step_ptr, int* __restrict__ idx,
                                                        int* __restrict__ slot) {
  __shared__ uint32_t sh[8];
  const uint64_t step = (uint64_t)*step_ptr;
  uint32_t T, need_eq;
  pfc_resolve<4>(ws, Cs, sh, T, need_eq);
  const int* off = ws + kWsBits + pfc_words(C);
  const int nchunks = pfc_chunks(C);
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    bool sure[4], eq[4];
    const uint32_t c0 = (uint32_t)ch * kPfcChunk + 4u * threadIdx.x;
    const uint32_t packed = pfc_flags(ws, c0, C, T, step, seed, sure, eq);
    uint32_t total;
    const uint32_t excl = block_scan256(packed, sh, total) - packed;
    // classes before this thread's first: taken for certain / tied at the threshold
    uint32_t ns = (uint32_t)off[2 * ch] + (excl & 0xFFFFu), ne = (uint32_t)off[2 * ch + 1] + (excl >> 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t c = c0 + e;
      if (c >= (uint32_t)C) break;
      const bool take = sure[e] || (eq[e] && ne < need_eq);
      const uint32_t pos = ns + min(ne, need_eq);
      int sl = -1;
      if (take && pos < (uint32_t)Cs) {  // (pos < Cs always holds: the subset has exactly Cs classes)
        idx[pos] = (int)c;
        sl = (int)pos;
      }
      slot[c] = sl;
      ns += sure[e] ? 1u : 0u;
      ne += eq[e] ? 1u : 0u;
    }
  }
}

__global__ void __launch_bounds__(256) pfc_relabel_kernel(const int64_t* __restrict__ labels, int B, int C,
                                                          const int* __restrict__ slot, int64_t* __restrict__ lab) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t y = labels[b];
  lab[b] = (y >= 0 && y < C) ? (int64_t)slot[y] : (int64_t)-1;
}

size_t pfc_workspace_words(int C) { return (size_t)kWsBits + pfc_words(C) + 2 * (size_t)pfc_chunks(C); }

bool launch_pfc_sample(const int64_t* labels, int B, int C, int Cs, uint64_t seed, const int64_t* step_ptr, int* ws,
                       int* idx, int* slot, int64_t* lab, hipStream_t st) {
  const int Csp = (Cs + 63) / 64 * 64;
  if (B < 1 || C < 1 || Cs < 1 || Cs > C || Cs < std::min(B, C)) return false;
  const int nclear = kWsBits + pfc_words(C);
  const int gb = (B + 255) / 256;
  const int gc = std::min(kPfcMaxGrid, (C + 255) / 256), gch = std::min(kPfcMaxGrid, pfc_chunks(C));
  hipLaunchKernelGGL(pfc_clear_kernel, dim3(std::min(kPfcMaxGrid, (nclear + 255) / 256)), dim3(256), 0, st, ws, nclear,
                     idx, Cs, Csp);
  hipLaunchKernelGGL(pfc_mark_kernel, dim3(gb), dim3(256), 0, st, labels, B, C, ws);
  hipLaunchKernelGGL(pfc_hist_kernel<0>, dim3(gc), dim3(256), 0, st, ws, C, Cs, seed, step_ptr);
  hipLaunchKernelGGL(pfc_hist_kernel<1>, dim3(gc), dim3(256), 0, st, ws, C, Cs, seed, step_ptr);
  hipLaunchKernelGGL(pfc_hist_kernel<2>, dim3(gc), dim3(256), 0, st, ws, C, Cs, seed, step_ptr);
  hipLaunchKernelGGL(pfc_hist_kernel<3>, dim3(gc), dim3(256), 0, st, ws, C, Cs, seed, step_ptr);
  hipLaunchKernelGGL(pfc_count_kernel, dim3(gch), dim3(256), 0, st, ws, C, Cs, seed, step_ptr);
  hipLaunchKernelGGL(pfc_scan_kernel, dim3(1), dim3(256), 0, st, ws, C);
  hipLaunchKernelGGL(pfc_write_kernel, dim3(gch), dim3(256), 0, st, ws, C, Cs, seed, step_ptr, idx, slot);
  hipLaunchKernelGGL(pfc_relabel_kernel, dim3(gb), dim3(256), 0, st, labels, B, C, slot, lab);
  return true;
}

// ---------------------------------------------------------------------------
// rows W[idx[r]] of w [C][D] fp32 -> the operands l2norm_t_tile makes of them: y [Rp][DP], yT [DP][Rp],
// inverse norms [Rp]; idx [Rp], -1 (or anything outside [0, C)) gives a zero row.
template <int DP>
__global__ void __launch_bounds__(256) arc_gather_l2norm_t_kernel(const float* __restrict__ w, const int* __restrict__ idx,
                                                                  int C, int D, int Rp, bf16* __restrict__ y,
                                                                  bf16* __restrict__ yT, float* __restrict__ inv_norm,
                                                                  float eps) {
  l2norm_t_tile<DP>(
      [=](int r) {
        const int src = idx[r];
        return OperandRow<float>{src >= 0 && src < C, w, (size_t)src};
      },
      D, Rp, y, yT, inv_norm, eps);
}

bool launch_arcface_gather_l2norm_t(const float* w, const int* idx, int C, int D, int Rp, int Dp, bf16* y, bf16* yT,
                                    float* inv, float eps, hipStream_t st) {
  if (Rp < 64 || Rp % 64 || D < 1 || D > Dp || !score_dp_ok(Dp)) return false;
#define ARC_GT(DP_) \
  hipLaunchKernelGGL((arc_gather_l2norm_t_kernel<DP_>), dim3(Rp / 64), dim3(256), 0, st, w, idx, C, D, Rp, y, yT, inv, eps);
  if (Dp == 128) { ARC_GT(128) } else if (Dp == 256) { ARC_GT(256) } else { ARC_GT(512) }
#undef ARC_GT
  return true;
}

// ---------------------------------------------------------------------------
// dense dW [C][D] from the compact gradient src [Cs][D]: row c = src[slot[c]] or zeros.  One wave per
// output row (4 rows per workgroup, grid-stride); VEC = 4 when D % 4 == 0 (16-byte accesses).
template <int VEC>
__global__ void __launch_bounds__(256) arc_scatter_rows_kernel(const float* __restrict__ src, const int* __restrict__ slot,
                                                               int C, int Cs, int D, float* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < C; c += gridDim.x * 4) {
    const int sl = slot[c];
    const bool on = sl >= 0 && sl < Cs;
    const float* s = src + (size_t)(on ? sl : 0) * D;
    float* d = dst + (size_t)c * D;
    if constexpr (VEC == 4) {
      for (int j = lane * 4; j < D; j += 256) *(f32x4*)(d + j) = on ? *(const f32x4*)(s + j) : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      for (int j = lane; j < D; j += 64) d[j] = on ? s[j] : 0.f;
    }
  }
}

bool launch_arcface_scatter_rows(const float* src, const int* slot, int C, int Cs, int D, float* dst, hipStream_t st) {
  if (C < 1 || Cs < 1 || D < 1) return false;
  const int grid = (int)std::min<int64_t>(((int64_t)C + 3) / 4, 65536);
  if (D % 4 == 0)
    hipLaunchKernelGGL(arc_scatter_rows_kernel<4>, dim3(grid), dim3(256), 0, st, src, slot, C, Cs, D, dst);
  else
    hipLaunchKernelGGL(arc_scatter_rows_kernel<1>, dim3(grid), dim3(256), 0, st, src, slot, C, Cs, D, dst);
  return true;
}

}  // namespace dcp

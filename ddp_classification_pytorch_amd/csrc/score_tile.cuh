// The streamed MFMA score tile shared by the fused ArcFace heads (arcface.hip, arcface_sub.hip,
// arcface_pfc.hip) and the fused top-k retrieval (knn.hip, knn_wide.hip).
//
// One tile: a 64-row block of queries / features is held as v_mfma_f32_16x16x32_bf16 B fragments in
// VGPRs for the whole kernel (lane = row l15, k slice q), and the other operand is streamed through LDS
// in tiles of TILE rows: row-major [TILE][Dp] bf16, XOR-swizzled, staged by LDS-DMA into a double-
// buffered ring (stage tile t + 1, tile_landed(), read tile t).  After the first MFMA a lane holds
// score(row, c0 + 16 j + 4 q + i) in acc[j][i].  The backward kernels also stage the transposed tile
// [Dp][TILE] and feed a register tile computed from acc straight into a second MFMA.
//
// The permuted k-fragment.  The accumulator layout of two 16-wide MFMA results (acc[2 kk], acc[2 kk + 1]:
// lane (l15, q) holds 4 consecutive rows 4 q .. + 3 of one column in each) is read as ONE 32-deep
// k-fragment of the second MFMA without any data movement: k slots 8 q .. 8 q + 3 <- rows
// 32 kk + 4 q .. + 3, slots 8 q + 4 .. 8 q + 7 <- rows 32 kk + 16 + 4 q .. + 3.  That is a fixed
// permutation of k, so the A operand is read from the transposed tile in the same permuted order
// (tr_frag / tr32_frag) and the product is the plain one.
//
// What the kernels of those files must agree on bit for bit is defined here once: the layouts, the operand
// normalisation (norm_row, l2norm_t_tile) and the margin.
// The host helpers at the end are plain inline functions (both compile passes parse the launchers).
#pragma once
#include <algorithm>

#include "common.cuh"

namespace dcp {

// ---- LDS layouts ------------------------------------------------------------------------------
// byte offset of 16-byte chunk c of row r in a row-major [rows][Dp] bf16 tile, XOR-swizzled
// (16 consecutive rows at one chunk -> 16 distinct bank groups for the fragment reads)
__device__ __forceinline__ uint32_t rm_off(uint32_t r, uint32_t c, uint32_t Dp) {
  return r * Dp * 2u + ((c ^ (r & 15u)) << 4);
}
// byte offset of 8-byte half h of chunk c of row d in a [Dp][64] bf16 tile (128-byte rows)
__device__ __forceinline__ uint32_t tr_off(uint32_t d, uint32_t c, uint32_t h) {
  return d * 128u + ((c ^ (d & 7u)) << 4) + (h << 3);
}
// the same for a [Dp][32] tile (64-byte rows): the 4 rows d, d + 4, d + 8, d + 12 that share a 256-byte
// bank window take 4 distinct chunks, so 16 consecutive rows at one chunk cover all 64 banks
__device__ __forceinline__ uint32_t tr32_off(uint32_t d, uint32_t c, uint32_t h) {
  return d * 64u + ((c ^ ((d >> 2) & 3u)) << 4) + (h << 3);
}

// ---- staging ----------------------------------------------------------------------------------
// LDS-DMA versions of the stagings (one 16-byte global_load_lds per lane and instruction, the lane's
// data landing at base + 16 lane: the swizzle is applied on the source side).  Untracked: the caller
// calls tile_landed() before reading the tile.  4 waves share the tile.
template <int DP, int TILE = 64>
__device__ __forceinline__ void dma_rm(char* T, const bf16* g, int r0, int w, int lane) {
  constexpr int CPR = DP / 8, RPB = 64 / CPR, NI = TILE / RPB / 4;  // rows per 1 KB block; blocks per wave
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int blk = w * NI + i;
    const int r = blk * RPB + lane / CPR, pos = lane % CPR;
    const int c = pos ^ (r & 15);
    dma16(g + (size_t)(r0 + r) * DP + c * 8, T + blk * 1024);
  }
}
template <int DP>
__device__ __forceinline__ void dma_tr(char* T, const bf16* g, int c0, int ld, int w, int lane) {
  constexpr int NI = DP / 8 / 4;  // 8 rows (128 B each) per 1 KB block
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int blk = w * NI + i;
    const int d = blk * 8 + lane / 8, pos = lane % 8;
    const int c = pos ^ (d & 7);
    dma16(g + (size_t)d * ld + c0 + c * 8, T + blk * 1024);
  }
}
template <int DP>
__device__ __forceinline__ void dma_tr32(char* T, const bf16* g, int c0, int ld, int w, int lane) {
  constexpr int NI = DP / 16 / 4;  // 16 rows (64 B each) per 1 KB block
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int blk = w * NI + i;
    const int d = blk * 16 + lane / 4, pos = lane % 4;
    const int c = pos ^ ((d >> 2) & 3);
    dma16(g + (size_t)d * ld + c0 + c * 8, T + blk * 1024);
  }
}

// the 8 bf16 of the permuted 32-deep k-fragment kk (above) of row d of a transposed [Dp][64] tile
__device__ __forceinline__ bf16x8 tr_frag(const char* T, uint32_t d, int kk, uint32_t q) {
  const uint32_t lo = 32u * kk + 4u * q, hi = lo + 16u;  // column indices (bf16)
  const bf16x4 a = *LDS_PTR(const bf16x4, T + tr_off(d, lo >> 3, (lo >> 2) & 1u));
  const bf16x4 b = *LDS_PTR(const bf16x4, T + tr_off(d, hi >> 3, (hi >> 2) & 1u));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
// the same from a [Dp][32] tile, whose 32 columns are the one k-fragment
__device__ __forceinline__ bf16x8 tr32_frag(const char* T, uint32_t d, uint32_t q) {
  const bf16x4 a = *LDS_PTR(const bf16x4, T + tr32_off(d, q >> 1, q & 1u));       // columns 4 q .. + 3
  const bf16x4 b = *LDS_PTR(const bf16x4, T + tr32_off(d, 2u + (q >> 1), q & 1u));  // 16 + 4 q .. + 3
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// The head of a ring iteration: this wave's DMA and LDS traffic is complete, then the workgroup barrier
// (every wave's part of the tile landed; every wave is done reading the buffer staged next).
__device__ __forceinline__ void tile_landed() {
  asm volatile("s_waitcnt vmcnt(0)\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// XCD-aware (row block, split) of a workgroup of a (row blocks, S splits) grid: workgroups are
// dispatched round-robin over the 8 XCDs, so for S % 8 == 0 the ones sharing an XCD (and its L2) take
// the SAME splits for all row blocks -- each XCD streams 1 / 8 of the tiles instead of all of them
__device__ __forceinline__ void xcd_row_split(int& rb, int& split) {
  rb = blockIdx.x;
  split = blockIdx.y;
  const int RB = gridDim.x, S = gridDim.y, L = blockIdx.x + blockIdx.y * RB;
  if ((S & 7) == 0) {
    const int xcd = L & 7, idx = L >> 3;
    split = xcd * (S >> 3) + idx / RB;
    rb = idx % RB;
  }
}

// ---- the ArcFace arithmetic -------------------------------------------------------------------
// margin (ARCFACE/arc_main.py:157-176), guarded at cos = +-1
__device__ __forceinline__ void arc_margin(float c, float cos_m, float sin_m, float th, float mm, int easy, float& phi,
                                           float& dphi) {
  c = fminf(fmaxf(c, -1.f), 1.f);
  const float sn = sqrtf(fminf(fmaxf(1.f - c * c, 0.f), 1.f));
  const float p = c * cos_m - sn * sin_m;
  const float dp = cos_m + (sn > 1e-6f ? sin_m * c / sn : 0.f);
  if (easy) {
    phi = c > 0.f ? p : c;
    dphi = c > 0.f ? dp : 1.f;
  } else {
    phi = c > th ? p : c - mm;
    dphi = c > th ? dp : 1.f;
  }
}

// ---- operands ---------------------------------------------------------------------------------
// One wave, one row: lane holds elements lane EPL .. + EPL - 1 of row r of x [..][D] (zero past D, or
// when !on) -> b = the row times iv = 1 / max(|row|, eps), rounded to bf16 once; returns iv (0 when !on).  THE
// normalisation of every score-tile operand: equal rows give equal bits in every kernel that calls it.
template <int EPL, typename T>
__device__ __forceinline__ float norm_row(const T* x, size_t r, bool on, int D, int lane, float eps, bf16 (&b)[EPL]) {
  float v[EPL];
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int j = lane * EPL + e;
    v[e] = (on && j < D) ? (float)x[r * D + j] : 0.f;
    ss += v[e] * v[e];
  }
  ss = wave_sum(ss);
  const float iv = on ? 1.f / fmaxf(sqrtf(ss), eps) : 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) b[e] = f2bf(v[e] * iv);
  return iv;
}

// A workgroup of 256: operand rows r0 = 64 blockIdx.x .. + 63 -> normalised bf16 rows y [Rp][DP], their
// transpose yT [DP][Rp] (the tile goes through LDS), inverse norms [Rp]; zero padding in both
// dimensions.  One pass for all three: a separate transpose launch per operand cost as much as the
// normalisation.  Each wave normalises 16 rows.  rows(r) says where operand row r comes from.
template <typename T>
struct OperandRow {
  bool on;     // false: a zero row
  const T* x;  // row r of x [..][D]
  size_t r;
};
template <int DP, typename Rows>
__device__ __forceinline__ void l2norm_t_tile(const Rows& rows, int D, int Rp, bf16* __restrict__ y,
                                              bf16* __restrict__ yT, float* __restrict__ inv_norm, float eps) {
  constexpr int EPL = DP / 64;  // elements per lane of a row
  __shared__ __attribute__((aligned(16))) bf16 tile[64][DP + 8];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = blockIdx.x * 64;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int rl = w * 16 + k, r = r0 + rl;
    const auto row = rows(r);
    bf16 b[EPL];
    const float iv = norm_row<EPL>(row.x, row.r, row.on, D, lane, eps, b);
    if (lane == 0) inv_norm[r] = iv;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      tile[rl][lane * EPL + e] = b[e];
      y[(size_t)r * DP + lane * EPL + e] = b[e];
    }
  }
  __syncthreads();
  // yT rows d: the 64 columns r0 .. r0 + 63 (128 contiguous bytes); a thread writes 8 columns
  for (int e = threadIdx.x; e < DP * 8; e += 256) {
    const int d = e >> 3, c = (e & 7) * 8;
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = tile[c + k][d];
    *(bf16x8*)(yT + (size_t)d * Rp + r0 + c) = o;
  }
}

// ---- host -------------------------------------------------------------------------------------
// the compile-time widths of the tile kernels (KS = Dp / 32 = 4 / 8 / 16)
inline bool score_dp_ok(int Dp) { return Dp == 128 || Dp == 256 || Dp == 512; }
// a kernel's dynamic LDS above the 64 KB default
inline void score_set_lds(const void* f, size_t bytes) {
  (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// splits of the streamed dimension: about `target` workgroups over `blocks` row blocks, at most one
// tile per split and `cap` splits; from 8 up a multiple of 8 (the XCD-aware mapping)
inline int score_splits(int blocks, int ntiles, int target, int cap) {
  blocks = std::max(1, blocks);
  int s = (target + blocks - 1) / blocks;
  s = std::max(1, std::min(s, std::min(std::max(1, ntiles), cap)));
  return s >= 8 ? s / 8 * 8 : s;
}

}  // namespace dcp

// Fused in-batch supervised contrastive loss (SupCon, Khosla et al. NeurIPS 2020, L_out^sup; with one
// label per image and two views SimCLR's NT-Xent), nothing [B, B] in memory.
//
// z_i = the bf16 operand row arc_l2norm_t_kernel makes of x_i (norm_row: the bits the ArcFace and kNN
// kernels read), s_ia = <z_i, z_a> / tau on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  A row is
// valid when its label is in [0, 2^31); A(i) = the valid rows but i, P(i) = those of A(i) with i's label,
// an anchor is a valid row with a positive.
//
//   loss_i = lse_i - (sum_{p in P(i)} s_ip) / |P(i)|,   lse_i = log sum_{a in A(i)} exp(s_ia)
//   loss   = (1 / n) sum_{anchors} loss_i,              n = max(1, #anchors)  (counted on the device)
//
//   forward   supcon_labels_kernel    labels int64 [B] -> y32 [Bp]: the label, -1 for an invalid or padding row
//             supcon_rows_kernel      (row block x column split) workgroups (xcd_row_split): the 64-row
//                                     anchor block in B fragments for the whole kernel, 64-row tiles of
//                                     the SAME zn through the dma_rm ring, each tile's 64 y32 beside it;
//                                     per lane an online (max, sum-exp) over A(i), the fp32 sum of s_ip
//                                     and the count |P(i)|; the kernel masks the diagonal, the padding
//                                     and the invalid columns (y32 < 0) -> partials [S][Bp][4]
//             supcon_finalize_kernel  merges the splits (one wave per row, a fixed butterfly) -> the row
//                                     record rec [Bp][4] = (lse, 1 / |P| or 0 for a non-anchor, y32 bits,
//                                     loss_i)
//             supcon_mean_kernel      one workgroup, fixed order: stat = (mean loss, 1 / n), the anchor count
//   backward  supcon_dz_kernel        same grid; recomputes each score tile and forms in the accumulators
//                                       G_ia = (g / (n tau)) (dS_ia + dS_ai)
//                                       dS_ia = anchor_i [a in A(i)] (exp(s_ia - lse_i) - [a in P(i)] / |P(i)|)
//                                     rounds G to bf16 into the permuted k-fragment and multiplies it
//                                     into dz += G z against the transposed tile (dma_tr / dma_tr32)
//             arc_norm_bwd_kernel     (arcface.hip) sums the split partials, dx = inv (dz - <dz, z> z)
//
// The one design decision: the Gram matrix is symmetric, every cosine appears as s_ia in row i's loss and
// as s_ai in row a's, so dz_i needs dS_ia AND dS_ai.  The transpose term is NOT a second GEMM: dS_ai is
// a function of the same score s_ia (bitwise: the MFMA sums the same products in the same order for
// (i, a) and (a, i)) and of row a's saved statistics (lse_a, 1 / |P(a)|, y_a).  So each staged tile
// carries its 64 (32) row records through the DMA ring, as the ArcFace dW kernel's row info does, the
// lane adds the column term from them to the row term from its own record, and one pass over the
// tiles yields the whole gradient.  G is exactly 0 on the diagonal, on padding and on invalid columns
// or rows (selects, not products).  1 / tau is folded into G before the bf16 rounding, so
// arc_norm_bwd_kernel runs unchanged.  No float atomics, no host read: capturable, deterministic.
//
// Widths as arcface.hip: Dp = 128 / 256 / 512 (KS = 4 / 8 / 16); at Dp = 512 the backward stages
// 32-row tiles (one 32-deep k-fragment) and runs one wave per SIMD.  gfx950 resources per variant
// (VGPR + AGPR, scratch, LDS), KS = 4 / 8 / 16:
//   supcon_rows_kernel   95 / 123 / 191 + 16,   scratch 0 / 0 / 0,  LDS 34 / 66 / 130 KB
//   supcon_dz_kernel     160 / 200 / 152 + 136, scratch 0 / 0 / 0,  LDS 66 / 130 / 130 KB
#include "launchers.h"
#include "score_tile.cuh"

namespace dcp {

namespace {

constexpr int kSupTile = 64;    // rows per staged column tile (32 in the Dp = 512 backward kernel)
constexpr int kSupInfo = 1024;  // bytes of per-row data staged beside a tile (labels, or 64 records x 16 B)

constexpr int sup_bwd_tile(int KS) { return KS == 16 ? 32 : kSupTile; }

struct SupParams {
  const bf16* zn;      // [Bp][Dp] normalised rows (rows >= B zero)
  const bf16* znT;     // [Dp][Bp] (backward)
  const int* y32;      // [Bp] label, -1 for an invalid or padding row (forward)
  const float* rec;    // [Bp][4] (lse, 1 / |P| or 0, y32 bits, loss_i) (backward)
  const float* gout;   // [1] upstream gradient of the mean loss (backward)
  const float* stat;   // [2] (mean loss, 1 / max(1, #anchors)) (backward)
  float* part;         // split partials
  float inv_tau;
  int B, Bp, S, tps;
};

}  // namespace

__global__ void __launch_bounds__(256) supcon_labels_kernel(const int64_t* __restrict__ labels, int B, int Bp,
                                                            int* __restrict__ y32) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= Bp) return;
  const int64_t y = r < B ? labels[r] : -1;
  y32[r] = (y >= 0 && y <= 0x7fffffffLL) ? (int)y : -1;
}

// forward partials (max, scaled sum, sum of positive scores, |P| as int bits) per (split, row).
// Grid (Bp / 64, S); 4 waves x 16 rows.
template <int KS>
__global__ void __launch_bounds__(256, KS == 16 ? 1 : 2) supcon_rows_kernel(const SupParams p) {
  constexpr int DP = KS * 32, TILE = kSupTile;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two buffers of ([64 rows][DP] swizzled, the rows' y32 four times over in a 1 KB slot)
  constexpr int TB = TILE * DP * 2, BUF = TB + kSupInfo;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t q = lane >> 4, l15 = lane & 15;
  int rb, split;  // (row block, column split)
  xcd_row_split(rb, split);
  const int row = rb * 64 + w * 16 + (int)l15;
  bf16x8 xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const bf16x8*)(p.zn + (size_t)row * DP + ks * 32 + q * 8);
  const int y = p.y32[row];
  float run_m = -INFINITY, run_s = 0.f, psum = 0.f;
  int pcnt = 0;

  const int ntiles = p.Bp / TILE;
  const int t0 = split * p.tps, t1 = min(ntiles, t0 + p.tps);
  auto stage = [&](int tile, int b) {
    char* Zb = smem + b * BUF;
    dma_rm<DP, TILE>(Zb, p.zn, tile * TILE, w, lane);
    // the tile's 64 labels: one DMA of one wave, 16 lanes' worth landing four times in the slot
    if (w == 0) dma16(p.y32 + tile * TILE + (lane & 15) * 4, Zb + TB);
  };
  if (t0 < t1) stage(t0, 0);
  for (int tile = t0; tile < t1; ++tile) {
    const int c0 = tile * TILE, b = (tile - t0) & 1;
    const char* Zt = smem + b * BUF;
    const float* lab = (const float*)(Zt + TB);  // [64] int bits
    tile_landed();
    if (tile + 1 < t1) stage(tile + 1, b ^ 1);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 a = *LDS_PTR(const bf16x8, Zt + rm_off(16 * j + l15, ks * 4 + q, DP));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc[j], 0, 0, 0);
      }
    // lane: cos of columns c0 + 16 j + 4 q + i (i = 0..3) for its row
    float v[16];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 yc = *LDS_PTR(const f32x4, lab + 16 * j + 4 * (int)q);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int col = c0 + 16 * j + 4 * (int)q + i, ya = __float_as_int(yc[i]);
        const bool on = ya >= 0 && col != row;  // in A(row): valid (padding rows carry -1), not the diagonal
        const bool pos = on && ya == y;
        const float s = p.inv_tau * acc[j][i];
        v[4 * j + i] = on ? s : -INFINITY;
        tmax = fmaxf(tmax, v[4 * j + i]);
        psum += pos ? s : 0.f;
        pcnt += pos ? 1 : 0;
      }
    }
    const float m_new = fmaxf(run_m, tmax);
    if (m_new > -INFINITY) {
      float sum = run_m > -INFINITY ? run_s * __expf(run_m - m_new) : 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) sum += __expf(v[k] - m_new);
      run_s = sum;
      run_m = m_new;
    }
  }
  // the 4 lanes of a row (l15, + 16, + 32, + 48): merge (max, sum), the positive sums and counts
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    const float om = __shfl_xor(run_m, o, 64), os = __shfl_xor(run_s, o, 64);
    const float m_new = fmaxf(run_m, om);
    float sum = 0.f;
    if (m_new > -INFINITY) {
      sum = (run_m > -INFINITY ? run_s * __expf(run_m - m_new) : 0.f) +
            (om > -INFINITY ? os * __expf(om - m_new) : 0.f);
    }
    run_m = m_new;
    run_s = sum;
    psum += __shfl_xor(psum, o, 64);
    pcnt += __shfl_xor(pcnt, o, 64);
  }
  if (q == 0) {
    float* o = p.part + ((size_t)split * p.Bp + row) * 4;
    *(f32x4*)o = f32x4{run_m, run_s, psum, __int_as_float(pcnt)};
  }
}

// merge the forward splits per row -> rec [Bp][4] = (lse, 1 / |P| (0 for a non-anchor), y32 bits, loss_i).
// One wave per row, one lane per split (S <= 64), the sums in the butterfly's fixed order.
__global__ void __launch_bounds__(256) supcon_finalize_kernel(const float* __restrict__ part, int S, int Bp,
                                                              const int* __restrict__ y32,
                                                              float* __restrict__ rec) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= Bp) return;
  f32x4 v = f32x4{-INFINITY, 0.f, 0.f, 0.f};
  if (lane < S) v = *(const f32x4*)(part + ((size_t)lane * Bp + r) * 4);
  const float M = wave_max(v[0]);
  const float sum = wave_sum(v[0] > -INFINITY ? v[1] * __expf(v[0] - M) : 0.f);
  const float ps = wave_sum(v[2]);
  int cnt = __float_as_int(v[3]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) {
    const int y = y32[r];
    const bool anchor = y >= 0 && cnt > 0;
    const float lse = M > -INFINITY ? M + __logf(sum) : 0.f;  // (an empty A(r): no anchor, a defined value)
    *(f32x4*)(rec + (size_t)r * 4) =
        f32x4{lse, anchor ? 1.f / (float)cnt : 0.f, __int_as_float(y), anchor ? lse - ps / (float)cnt : 0.f};
  }
}

// stat = (sum of loss_i / n, 1 / n), nanch = #anchors, n = max(1, #anchors).  One workgroup: thread t sums
// rows t, t + 256, .. in order, then the block reduction -- a fixed order for a given B.
__global__ void __launch_bounds__(256) supcon_mean_kernel(const float* __restrict__ rec, int B,
                                                          float* __restrict__ stat, int* __restrict__ nanch) {
  __shared__ float red[16];
  float s = 0.f;
  int n = 0;
  for (int r = threadIdx.x; r < B; r += 256) {
    const f32x4 v = *(const f32x4*)(rec + (size_t)r * 4);
    s += v[3];
    n += v[1] > 0.f ? 1 : 0;
  }
  s = block_sum(s, red);
  const float nf = block_sum((float)n, red);  // (integers below 2^24: exact)
  if (threadIdx.x == 0) {
    const float inv = 1.f / fmaxf(nf, 1.f);
    stat[0] = s * inv;
    stat[1] = inv;
    nanch[0] = (int)nf;
  }
}

// dz partials [S][Bp][Dp].  Grid (Bp / 64, S); 4 waves x 16 rows.  KS = 16 (Dp = 512): 32-row tiles, one
// wave per SIMD (128 accumulator + 64 fragment registers), see arc_rows_kernel.
template <int KS>
__global__ void __launch_bounds__(256, KS == 16 ? 1 : 2) supcon_dz_kernel(const SupParams p) {
  constexpr int DP = KS * 32, DF = DP / 16;
  constexpr int TILE = sup_bwd_tile(KS), NJ = TILE / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two buffers of ([TILE rows][DP] swizzled, [DP][TILE rows], the rows' records [TILE][4] in a 1 KB slot)
  constexpr int TB = TILE * DP * 2 * 2, BUF = TB + kSupInfo;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t q = lane >> 4, l15 = lane & 15;
  int rb, split;
  xcd_row_split(rb, split);
  const int row = rb * 64 + w * 16 + (int)l15;
  bf16x8 xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const bf16x8*)(p.zn + (size_t)row * DP + ks * 32 + q * 8);
  const f32x4 rr = *(const f32x4*)(p.rec + (size_t)row * 4);
  const float lse = rr[0], invp = rr[1];
  const int y = __float_as_int(rr[2]);
  const bool valid = y >= 0, anchor = invp > 0.f;
  const float gs = p.gout[0] * p.stat[1] * p.inv_tau;  // g / (n tau): 1 / tau folded into G
  f32x4 dacc[DF];
#pragma unroll
  for (int f = 0; f < DF; ++f) dacc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ntiles = p.Bp / TILE;  // (p.tps counts tiles of this width)
  const int t0 = split * p.tps, t1 = min(ntiles, t0 + p.tps);
  auto stage = [&](int tile, int b) {
    char* Zb = smem + b * BUF;
    dma_rm<DP, TILE>(Zb, p.zn, tile * TILE, w, lane);
    if constexpr (TILE == 32)
      dma_tr32<DP>(Zb + TILE * DP * 2, p.znT, tile * TILE, p.Bp, w, lane);
    else
      dma_tr<DP>(Zb + TILE * DP * 2, p.znT, tile * TILE, p.Bp, w, lane);
    // the tile's row records: one DMA of one wave (a 32-row tile lands twice in the 1 KB slot)
    if (w == 0) dma16(p.rec + (size_t)(tile * TILE + (lane & (TILE - 1))) * 4, Zb + TB);
  };
  if (t0 < t1) stage(t0, 0);
  for (int tile = t0; tile < t1; ++tile) {
    const int c0 = tile * TILE, b = (tile - t0) & 1;
    const char* Zt = smem + b * BUF;
    const char* ZT = Zt + TILE * DP * 2;
    const float* info = (const float*)(Zt + TB);  // [TILE][4]
    tile_landed();
    if (tile + 1 < t1) stage(tile + 1, b ^ 1);
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bf16x8 a = *LDS_PTR(const bf16x8, Zt + rm_off(16 * j + l15, ks * 4 + q, DP));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc[j], 0, 0, 0);
      }
    // lane: cos(row, a = c0 + 16 j + 4 q + i) -> G, the row term from its own record, the column term
    // (dS_ai) from row a's staged record
    bf16x8 dfr[NJ / 2];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cl = 16 * j + 4 * (int)q + i;
        const f32x4 in = *LDS_PTR(const f32x4, info + cl * 4);  // (lse_a, 1 / |P(a)|, y_a, -)
        const int ya = __float_as_int(in[2]);
        const float s = p.inv_tau * acc[j][i];
        const bool same = ya == y;
        const bool pair = valid && ya >= 0 && c0 + cl != row;  // a in A(row) and row in A(a)
        const float rt = anchor ? __expf(s - lse) - (same ? invp : 0.f) : 0.f;
        const float ct = in[1] > 0.f ? __expf(s - in[0]) - (same ? in[1] : 0.f) : 0.f;
        const float d = pair ? gs * (rt + ct) : 0.f;  // (a select: a non-anchor's exp may overflow)
        dfr[j >> 1][(j & 1) * 4 + i] = f2bf(d);
      }
#pragma unroll
    for (int kk = 0; kk < NJ / 2; ++kk)
#pragma unroll
      for (int f = 0; f < DF; ++f) {
        bf16x8 a;
        if constexpr (TILE == 32)
          a = tr32_frag(ZT, 16u * f + l15, q);
        else
          a = tr_frag(ZT, 16u * f + l15, kk, q);
        dacc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dfr[kk], dacc[f], 0, 0, 0);
      }
  }
  // lane holds dz[row][16 f + 4 q + i]
  float* o = p.part + ((size_t)split * p.Bp + row) * DP + 4 * q;
#pragma unroll
  for (int f = 0; f < DF; ++f) *(f32x4*)(o + 16 * f) = dacc[f];
}

// ---------------------------------------------------------------------------
namespace {
constexpr size_t kSupLdsMax = 160 * 1024;
constexpr int kSupMaxRows = 1 << 24;  // the anchor count is summed in fp32
}  // namespace

int supcon_fwd_splits(int Bp) { return score_splits(Bp / 64, Bp / kSupTile, 1024, 64); }
int supcon_dz_splits(int Bp) { return score_splits(Bp / 64, Bp / kSupTile, 256, 16); }

bool launch_supcon_fwd(const bf16* zn, const int64_t* labels, int B, int Bp, int Dp, float tau, int S, int* y32,
                       float* part, float* rec, float* stat, int* nanch, hipStream_t st) {
  if (Bp % 64 || B < 1 || B > Bp || Bp > kSupMaxRows || !score_dp_ok(Dp) || !(tau > 0.f) || S < 1 || S > 64)
    return false;
  hipLaunchKernelGGL(supcon_labels_kernel, dim3((Bp + 255) / 256), dim3(256), 0, st, labels, B, Bp, y32);
  SupParams p{};
  p.zn = zn; p.y32 = y32; p.part = part;
  p.inv_tau = 1.f / tau; p.B = B; p.Bp = Bp; p.S = S;
  p.tps = (Bp / kSupTile + S - 1) / S;
  const size_t lds = 2 * ((size_t)kSupTile * Dp * 2 + kSupInfo);
  if (lds > kSupLdsMax) return false;
  const dim3 grid(Bp / 64, S);
#define SUP_FWD(KS_)                                                                                   \
  score_set_lds((const void*)supcon_rows_kernel<KS_>, lds);                                            \
  hipLaunchKernelGGL((supcon_rows_kernel<KS_>), grid, dim3(256), lds, st, p);
  if (Dp == 128) { SUP_FWD(4) } else if (Dp == 256) { SUP_FWD(8) } else { SUP_FWD(16) }
#undef SUP_FWD
  hipLaunchKernelGGL(supcon_finalize_kernel, dim3(Bp / 4), dim3(256), 0, st, part, S, Bp, y32, rec);
  hipLaunchKernelGGL(supcon_mean_kernel, dim3(1), dim3(256), 0, st, rec, B, stat, nanch);
  return true;
}

bool launch_supcon_dz(const bf16* zn, const bf16* znT, const float* rec, const float* stat, const float* gout,
                      const float* inv, int B, int Bp, int Dp, int D, float tau, int S, float* part, void* dx,
                      bool dx_bf16, hipStream_t st) {
  if (Bp % 64 || B < 1 || B > Bp || !score_dp_ok(Dp) || D < 1 || D > Dp || !(tau > 0.f) || S < 1 || S > 64)
    return false;
  SupParams p{};
  p.zn = zn; p.znT = znT; p.rec = rec; p.stat = stat; p.gout = gout; p.part = part;
  p.inv_tau = 1.f / tau; p.B = B; p.Bp = Bp; p.S = S;
  const int tile = sup_bwd_tile(Dp / 32);  // the kernel's column tile: the splits count tiles of that width
  p.tps = (Bp / tile + S - 1) / S;
  const size_t lds = 2 * ((size_t)tile * Dp * 2 * 2 + kSupInfo);
  if (lds > kSupLdsMax) return false;
  const dim3 grid(Bp / 64, S);
#define SUP_DZ(KS_)                                                                                    \
  score_set_lds((const void*)supcon_dz_kernel<KS_>, lds);                                              \
  hipLaunchKernelGGL((supcon_dz_kernel<KS_>), grid, dim3(256), lds, st, p);
  if (Dp == 128) { SUP_DZ(4) } else if (Dp == 256) { SUP_DZ(8) } else { SUP_DZ(16) }
#undef SUP_DZ
  launch_arc_norm_bwd(part, S, (size_t)Bp * Dp, zn, Dp, D, inv, B, dx, dx_bf16, st);
  return true;
}

}  // namespace dcp

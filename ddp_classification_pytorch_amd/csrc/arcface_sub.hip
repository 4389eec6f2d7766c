// Fused Sub-center ArcFace head (Deng et al., ECCV 2020): K centres per class, a sample scored against
// the nearest centre of each class, nothing [B, C K] in memory.  The K = 1 head is arcface.hip; both
// are built on the streamed tile of score_tile.cuh (cosine tiles live in v_mfma_f32_16x16x32_bf16
// accumulators only, weight / row tiles come through LDS by LDS-DMA, XOR-swizzled, double buffered; no
// atomics, fixed sum orders), which also holds the margin and the operand normalisation.
//
// Operand layout, sub-centre-planar.  KP = 2 planes for K = 2, 4 planes for K = 3 and 4 (K = 3 carries
// one all-zero plane).  A staged tile is 64 operand rows = G = 4 / KP class groups x KP planes x 16
// classes, CT = 16 G classes (32 for K = 2, 16 for K = 3, 4):
//     operand row of (class c, centre k) = (c / CT) * 64 + (((c % CT) / 16) * KP + k) * 16 + c % 16
// so accumulator acc[g KP + k] of the first MFMA is plane k of the same 16 classes: a lane holds
// cos(row, class, k) for every k at a fixed (q, i), and the max / first argmax over K is K - 1 compares
// in registers.  wn [Wp][Dp], its transpose wnT [Dp][Wp] and the inverse norms [Wp] all use this row
// order (Wp = 64 * ceil(C / CT)); rows of classes >= C and of planes >= K are zero.
//
//   operand   arcs_l2norm_t_kernel    W [C][K][D] fp32 -> wn, wnT, inverse norms in the order above
//   forward   arcs_label_kernel       per row: the K cosines of the label class (fp32 dots), their
//                                     first maximum -> sub_idx, target logit t = s phi(max), dphi
//             arcs_rows_kernel<0>     streams tiles, max over the K planes in registers, t substituted
//                                     at the label class, online (max, sum, rank count) per (split, row):
//                                     4 G logits per lane and tile, so 1 / K of the K = 1 head's exps
//             arc_fwd_finalize        (arcface.hip) merges the splits: loss, rank, lse
//   backward  arcs_rows_kernel<1>     recomputes the tile, dcbar = g s (softmax - onehot) (dphi at the
//                                     label), written into the winning plane's slot of the 32-deep
//                                     k-fragment of the second MFMA and zeros into the others (the
//                                     stored sub_idx at the label class, the first maximum elsewhere)
//             arcs_dw_kernel          one workgroup per 64 operand rows (= all planes of CT classes)
//                                     over all batch rows, wave w owning rows 16 w .. + 15 = one
//                                     (group, plane).  The planes of a class sit in different waves, so
//                                     the waves exchange their cosine tiles through 16 KB of LDS (lane-
//                                     linear: no bank conflicts) and each wave decides for itself
//                                     whether its plane is the first maximum, by exact fp32 compares.
//             arcs_norm_bwd_kernel    split sums + L2-normalisation backward (dX; dW when row-split)
//
// K = 3: the pairing of two 16-row groups into one 32-deep k-fragment needs an even group count.
// Staging two class groups (96 rows) would take 2 x 96 KB of LDS at Dp = 256, past the 160 KB of a CU,
// so the tile is padded with a zero plane instead.  The first MFMA skips that plane (24 of 32 slots
// issued); the second runs all 32 with a quarter structurally zero, the tile stream carries 1 / 3 more
// bytes, and the fourth wave of the dW kernel only stages.  Per class that is 56 MFMAs where an
// unpadded tile would need 48.
// Why dW does not keep all planes in one wave: K planes x (KS fragment + DF accumulator registers) is
// 4 x (32 + 64) = 384 VGPRs at K = 4, Dp = 256 before the cosine tile; the exchange costs 64 B written
// and (K - 1) 64 B read per lane and tile beside 1 KB of fragment reads, and one more barrier per tile.
//
// Widths: Dp = 128 / 256 (KS = 4 / 8).  LDS: 64 KB (forward), 128 KB (dX), 146 KB (dW) at Dp = 256.
#include "launchers.h"
#include "score_tile.cuh"

namespace dcp {

namespace {

constexpr int kTile = 64;      // operand rows per staged tile
constexpr int kInfo = 1024;    // bytes of per-row info beside a dW row tile (64 rows x 16 B)
constexpr int kExch = 16384;   // bytes of the dW kernel's cosine exchange (4 waves x 16 values x 64 lanes)

constexpr int sub_kp(int K) { return K == 2 ? 2 : 4; }
// operand row of (class c, centre k)
__host__ __device__ __forceinline__ int sub_row(int c, int k, int KP) {
  const int CT = 64 / KP;
  return (c / CT) * 64 + (((c % CT) >> 4) * KP + k) * 16 + (c & 15);
}

struct SubParams {
  const bf16* xn;    // [Bp][Dp] normalised features (rows >= B zero)
  const bf16* xnT;   // [Dp][Bp]
  const bf16* wn;    // [Wp][Dp] normalised centres, planar row order
  const bf16* wnT;   // [Dp][Wp]
  const int64_t* labels;  // [B]
  const float* lab;  // [Bp][2]: target logit s * phi, d phi / d cos (0, 0 for an invalid row)
  const int* sub;    // [Bp] winning centre of the label class
  const float* lse;  // [Bp] (backward)
  const float* info; // [Bp][4] (bits of label * 4 + sub_idx or -1; t; dphi; lse): dW's per-row operands
  const float* gout; // [1] upstream gradient of the mean loss (backward)
  float* part;       // split partials
  float scale;       // 1 / B (mean reduction)
  int B, Bp, C, Wp, S, tps;
  float s;
};

}  // namespace

// W [C][K][D] fp32 -> the operands l2norm_t_tile makes of its rows in the planar order: y [Wp][Dp],
// yT [Dp][Wp], inverse norms [Wp] (zero for padding rows).  One workgroup per tile; operand row
// 64 t + 16 (g KP + k) + i is centre k of class CT t + 16 g + i (the inverse of sub_row).
template <int DP>
__global__ void __launch_bounds__(256) arcs_l2norm_t_kernel(const float* __restrict__ W, int C, int K, int D, int Wp,
                                                            bf16* __restrict__ y, bf16* __restrict__ yT,
                                                            float* __restrict__ inv_norm, float eps) {
  const int KP = sub_kp(K), CT = 64 / KP;
  l2norm_t_tile<DP>(
      [=](int r) {
        const int p = (r & 63) >> 4, k = p % KP, c = (r >> 6) * CT + (p / KP) * 16 + (r & 15);
        return OperandRow<float>{c < C && k < K, W, (size_t)c * K + k};
      },
      D, Wp, y, yT, inv_norm, eps);
}

// per row: the K cosines of the label class, their first maximum, target logit, margin derivative
__global__ void __launch_bounds__(256) arcs_label_kernel(const bf16* __restrict__ xn, const bf16* __restrict__ wn,
                                                         const int64_t* __restrict__ labels, int B, int Bp, int C,
                                                         int K, int Dp, float s, float cos_m, float sin_m, float th,
                                                         float mm, int easy, float* __restrict__ lab,
                                                         int* __restrict__ sub) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= Bp) return;
  const int64_t y64 = r < B ? labels[r] : -1;
  const bool valid = y64 >= 0 && y64 < C;
  const int y = valid ? (int)y64 : 0;
  const int KP = sub_kp(K);
  float best = -INFINITY;
  int bk = 0;
  if (valid)
    for (int k = 0; k < K; ++k) {
      const bf16* wr = wn + (size_t)sub_row(y, k, KP) * Dp;
      float acc = 0.f;
      for (int j = lane; j < Dp; j += 64) acc += bf2f(xn[(size_t)r * Dp + j]) * bf2f(wr[j]);
      acc = wave_sum(acc);
      if (acc > best) {  // strict: the smallest k of equal maxima stays
        best = acc;
        bk = k;
      }
    }
  if (lane == 0) {
    float phi = 0.f, dphi = 0.f;
    if (valid) arc_margin(best, cos_m, sin_m, th, mm, easy, phi, dphi);
    lab[2 * r] = valid ? s * phi : 0.f;
    lab[2 * r + 1] = valid ? dphi : 0.f;
    sub[r] = bk;
  }
}

// MODE 0: forward partials (max, scaled sum, rank count) per (split, row);
// MODE 1: dxn partials [S][Bp][DP].  Grid (Bp / 64, S); 4 waves x 16 rows.
template <int KS, int K, int MODE>
__global__ void __launch_bounds__(256, 2) arcs_rows_kernel(const SubParams p) {
  constexpr int DP = KS * 32, DF = DP / 16;
  constexpr int KP = sub_kp(K), G = 4 / KP, CT = 16 * G;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BUF = kTile * DP * 2 * (MODE == 1 ? 2 : 1);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t q = lane >> 4, l15 = lane & 15;
  int rb, split;  // (row block, class split)
  xcd_row_split(rb, split);
  const int row = rb * 64 + w * 16 + (int)l15;
  bf16x8 xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const bf16x8*)(p.xn + (size_t)row * DP + ks * 32 + q * 8);
  const int64_t y64 = row < p.B ? p.labels[row] : -1;
  const bool valid = y64 >= 0 && y64 < p.C;
  const int y = valid ? (int)y64 : -1;
  const float t = p.lab[2 * row], dphi = p.lab[2 * row + 1];
  float lse = 0.f, gs = 0.f;
  int sub = 0;
  if constexpr (MODE == 1) {
    lse = p.lse[row];
    sub = p.sub[row];
    gs = valid ? p.gout[0] * p.scale * p.s : 0.f;
  }
  float run_m = -INFINITY, run_s = 0.f, cnt = 0.f;
  f32x4 dacc[MODE == 1 ? DF : 1];
  if constexpr (MODE == 1)
#pragma unroll
    for (int f = 0; f < DF; ++f) dacc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ntiles = p.Wp / kTile;
  const int t0 = split * p.tps, t1 = min(ntiles, t0 + p.tps);
  auto stage = [&](int tile, int b) {
    char* Wb = smem + b * BUF;
    dma_rm<DP>(Wb, p.wn, tile * kTile, w, lane);
    if constexpr (MODE == 1) dma_tr<DP>(Wb + kTile * DP * 2, p.wnT, tile * kTile, p.Wp, w, lane);
  };
  if (t0 < t1) stage(t0, 0);
  for (int tile = t0; tile < t1; ++tile) {
    const int c0 = tile * CT, b = (tile - t0) & 1;
    const char* Wt = smem + b * BUF;
    const char* WT = Wt + kTile * DP * 2;
    tile_landed();  // this tile landed for every wave; the other buffer's reads are done
    if (tile + 1 < t1) stage(tile + 1, b ^ 1);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j % KP >= K) continue;  // the zero plane of K = 3
        const bf16x8 a = *LDS_PTR(const bf16x8, Wt + rm_off(16 * j + l15, ks * 4 + q, DP));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc[j], 0, 0, 0);
      }
    // lane: cos(row, class c0 + 16 g + 4 q + i, centre k) = acc[g KP + k][i]
    if constexpr (MODE == 0) {
      float v[4 * G];
      float tmax = -INFINITY;
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cls = c0 + 16 * g + 4 * (int)q + i;
          float cb = acc[g * KP][i];
#pragma unroll
          for (int k = 1; k < K; ++k) cb = fmaxf(cb, acc[g * KP + k][i]);
          const bool on = cls < p.C;
          const float x = cls == y ? t : p.s * cb;
          v[4 * g + i] = on ? x : -INFINITY;
          tmax = fmaxf(tmax, v[4 * g + i]);
          cnt += (on && cls != y && x > t) ? 1.f : 0.f;
        }
      const float m_new = fmaxf(run_m, tmax);
      if (m_new > -INFINITY) {
        float sum = run_m > -INFINITY ? run_s * __expf(run_m - m_new) : 0.f;
#pragma unroll
        for (int u = 0; u < 4 * G; ++u) sum += __expf(v[u] - m_new);
        run_s = sum;
        run_m = m_new;
      }
    } else {
      bf16x8 dfr[2];
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cls = c0 + 16 * g + 4 * (int)q + i;
          const bool lab_col = cls == y;
          float cb = acc[g * KP][i];
          int kw = 0;
#pragma unroll
          for (int k = 1; k < K; ++k) {
            const float o = acc[g * KP + k][i];
            if (o > cb) {  // strict: the first maximum
              cb = o;
              kw = k;
            }
          }
          if (lab_col) kw = sub;  // the forward's decision, the one t and dphi came from
          const float x = lab_col ? t : p.s * cb;
          const float pr = __expf(x - lse);
          const float d0 = gs * (pr - (lab_col ? 1.f : 0.f)) * (lab_col ? dphi : 1.f);
          const bf16 d = f2bf((valid && cls < p.C) ? d0 : 0.f);
#pragma unroll
          for (int k = 0; k < KP; ++k) {
            const int j = g * KP + k;
            dfr[j >> 1][(j & 1) * 4 + i] = k == kw ? d : f2bf(0.f);
          }
        }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int f = 0; f < DF; ++f) {
          const bf16x8 a = tr_frag(WT, 16u * f + l15, kk, q);
          dacc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dfr[kk], dacc[f], 0, 0, 0);
        }
    }
  }
  if constexpr (MODE == 0) {
    // the 4 lanes of a row (l15, + 16, + 32, + 48): merge (max, sum) and counts
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float om = __shfl_xor(run_m, o, 64), os = __shfl_xor(run_s, o, 64), oc = __shfl_xor(cnt, o, 64);
      const float m_new = fmaxf(run_m, om);
      float sum = 0.f;
      if (m_new > -INFINITY) {
        sum = (run_m > -INFINITY ? run_s * __expf(run_m - m_new) : 0.f) +
              (om > -INFINITY ? os * __expf(om - m_new) : 0.f);
      }
      run_m = m_new;
      run_s = sum;
      cnt += oc;
    }
    if (q == 0) {
      float* o = p.part + ((size_t)split * p.Bp + row) * 4;
      *(f32x4*)o = f32x4{run_m, run_s, cnt, 0.f};
    }
  } else {
    float* o = p.part + ((size_t)split * p.Bp + row) * DP + 4 * q;
#pragma unroll
    for (int f = 0; f < DF; ++f) *(f32x4*)(o + 16 * f) = dacc[f];
  }
}

// out row r (grid.x): g = sum_s part[s][src][:D], out[r] = inv[src] * (g - y[src] <g, y[src]>), the
// backward of y = x / |x|.  K == 0: src = r (dX); K > 0: r = c K + k of dW [C][K][D], src its operand row.
template <typename TO>
__global__ void __launch_bounds__(256) arcs_norm_bwd_kernel(const float* __restrict__ part, int S, size_t sstride,
                                                            const bf16* __restrict__ y, int Dp, int D, int K,
                                                            const float* __restrict__ inv, TO* __restrict__ out) {
  __shared__ float red[16];
  const int r = blockIdx.x;
  const int src = K ? sub_row(r / K, r % K, sub_kp(K)) : r;
  const int j = threadIdx.x;  // Dp <= 256
  float g = 0.f, yv = 0.f;
  if (j < D) {
    for (int s0 = 0; s0 < S; s0 += 16) {  // the split loads issued together, summed in split order
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = s0 + u < S ? part[(s0 + u) * sstride + (size_t)src * Dp + j] : 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) g += v[u];
    }
    yv = bf2f(y[(size_t)src * Dp + j]);
  }
  const float dot = block_sum(g * yv, red);
  if (j < D) out[(size_t)r * D + j] = (TO)(inv[src] * (g - yv * dot));
}

// the dW kernel's per-row operands: info[r] = (int bits of label * 4 + sub_idx, or -1 for an invalid or
// padding row; t; dphi; lse)
__global__ void __launch_bounds__(256) arcs_rowinfo_kernel(const int64_t* __restrict__ labels,
                                                           const float* __restrict__ lab, const int* __restrict__ sub,
                                                           const float* __restrict__ lse, int B, int Bp, int C,
                                                           float* __restrict__ info) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= Bp) return;
  const int64_t y = r < B ? labels[r] : -1;
  const int code = (y >= 0 && y < C) ? (int)y * 4 + sub[r] : -1;
  *(f32x4*)(info + (size_t)r * 4) = f32x4{__int_as_float(code), lab[2 * r], lab[2 * r + 1], lse[r]};
}

// dW: grid (Wp / 64, S row splits); wave w owns operand rows 16 w .. + 15 of the block = plane w % KP of
// class group w / KP.  S == 1: dw[c][k][:D] = inv_w (dwn - wn <dwn, wn>) written from the epilogue;
// S > 1: dwn partials [S][Wp][DP] for arcs_norm_bwd_kernel.
template <int KS, int K>
__global__ void __launch_bounds__(256, 2) arcs_dw_kernel(const SubParams p, const float* __restrict__ inv_w, int D,
                                                         float* __restrict__ dw) {
  constexpr int DP = KS * 32, DF = DP / 16;
  constexpr int KP = sub_kp(K), CT = 64 / KP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TB = kTile * DP * 2 * 2, BUF = TB + kInfo;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t q = lane >> 4, l15 = lane & 15;
  const int k = w % KP, gbase = (w / KP) * KP;  // this wave's plane; wave of plane 0 of its class group
  const bool live = k < K;                      // (the zero plane of K = 3 only stages)
  const int cls = blockIdx.x * CT + (w / KP) * 16 + (int)l15;
  const int wrow = blockIdx.x * 64 + w * 16 + (int)l15;
  float* exch = (float*)(smem + 2 * BUF);  // [4 waves][16 values][64 lanes]
  bf16x8 wf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) wf[ks] = *(const bf16x8*)(p.wn + (size_t)wrow * DP + ks * 32 + q * 8);
  const float g0 = p.gout[0] * p.scale * p.s;
  f32x4 dacc[DF];
#pragma unroll
  for (int f = 0; f < DF; ++f) dacc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto stage = [&](int r0, int b) {
    char* Xb = smem + b * BUF;
    dma_rm<DP>(Xb, p.xn, r0, w, lane);
    dma_tr<DP>(Xb + kTile * DP * 2, p.xnT, r0, p.Bp, w, lane);
    if (w == 0) dma16(p.info + (size_t)(r0 + lane) * 4, Xb + TB);
  };
  const int nrt = p.Bp / kTile, rps = (nrt + p.S - 1) / p.S;
  const int rt0 = blockIdx.y * rps, rt1 = min(nrt, rt0 + rps);
  const int rbeg = rt0 * kTile, rend = rt1 * kTile;
  if (rbeg < rend) stage(rbeg, 0);
  for (int r0 = rbeg; r0 < rend; r0 += kTile) {
    const int b = ((r0 - rbeg) / kTile) & 1;
    const char* Xt = smem + b * BUF;
    const char* XT = Xt + kTile * DP * 2;
    const float* info = (const float*)(Xt + TB);  // [64][4]
    tile_landed();  // this row tile landed; the other buffer and the exchange of the last tile are free
    if (r0 + kTile < rend) stage(r0 + kTile, b ^ 1);
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bf16x8 a = *LDS_PTR(const bf16x8, Xt + rm_off(16 * j + l15, ks * 4 + q, DP));
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wf[ks], acc[j], 0, 0, 0);
        }
      // lane: cos(row r0 + 16 j + 4 q + i, cls, k); the other planes' lanes hold the same (row, class)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) *LDS_PTR(float, exch + (w * 16 + j * 4 + i) * 64 + lane) = acc[j][i];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every plane's cosines are in the exchange
    asm volatile("" ::: "memory");
    if (live) {
      bf16x8 dfr[2];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float mine = acc[j][i];
          bool win = true;  // first maximum: above every earlier plane, not below any later one
#pragma unroll
          for (int k2 = 0; k2 < K; ++k2) {
            if (k2 == k) continue;
            const float o = *LDS_PTR(const float, exch + ((gbase + k2) * 16 + j * 4 + i) * 64 + lane);
            win = win && (k2 < k ? o < mine : o <= mine);
          }
          const f32x4 in = *LDS_PTR(const f32x4, info + (16 * j + 4 * (int)q + i) * 4);
          const int code = __float_as_int(in[0]);
          const bool lab_col = code >= 0 && (code >> 2) == cls;
          if (lab_col) win = (code & 3) == k;  // the forward's decision
          const float x = lab_col ? in[1] : p.s * mine;
          const float pr = __expf(x - in[3]);
          const float d0 = g0 * (pr - (lab_col ? 1.f : 0.f)) * (lab_col ? in[2] : 1.f);
          const float d = (win && code >= 0 && cls < p.C) ? d0 : 0.f;
          dfr[j >> 1][(j & 1) * 4 + i] = f2bf(d);
        }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int f = 0; f < DF; ++f) {
          const bf16x8 a = tr_frag(XT, 16u * f + l15, kk, q);
          dacc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, dfr[kk], dacc[f], 0, 0, 0);
        }
    }
  }
  if (p.S > 1) {  // (the zero plane writes zeros: the merge kernel never reads them)
    float* o = p.part + ((size_t)blockIdx.y * p.Wp + wrow) * DP + 4 * q;
#pragma unroll
    for (int f = 0; f < DF; ++f) *(f32x4*)(o + 16 * f) = dacc[f];
    return;
  }
  if (!live) return;
  // lane holds dwn[wrow][16 f + 4 q + i]; <dwn, wn> over the 4 lanes of a row (q = 0..3)
  float dot = 0.f;
#pragma unroll
  for (int f = 0; f < DF; ++f) {
    const bf16x4 wv = *(const bf16x4*)(p.wn + (size_t)wrow * DP + 16 * f + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) dot += dacc[f][i] * bf2f(wv[i]);
  }
  dot += __shfl_xor(dot, 16, 64);
  dot += __shfl_xor(dot, 32, 64);
  if (cls >= p.C) return;
  const float iv = inv_w[wrow];
  float* o = dw + ((size_t)cls * K + k) * D;
#pragma unroll
  for (int f = 0; f < DF; ++f) {
    const bf16x4 wv = *(const bf16x4*)(p.wn + (size_t)wrow * DP + 16 * f + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = 16 * f + 4 * (int)q + i;
      if (j < D) o[j] = iv * (dacc[f][i] - bf2f(wv[i]) * dot);
    }
  }
}

// ---------------------------------------------------------------------------
namespace {
bool sub_ok(int K, int Dp) { return K >= 2 && K <= 4 && (Dp == 128 || Dp == 256); }
// F(KS, K) for the runtime (Dp, K)
#define ARCS_DISPATCH(F)                                                                              \
  if (Dp == 128) {                                                                                    \
    if (K == 2) { F(4, 2) } else if (K == 3) { F(4, 3) } else { F(4, 4) }                             \
  } else {                                                                                            \
    if (K == 2) { F(8, 2) } else if (K == 3) { F(8, 3) } else { F(8, 4) }                             \
  }
}  // namespace

int arcface_sub_rows(int C, int K) {
  const int CT = 64 / sub_kp(K);
  return (C + CT - 1) / CT * 64;
}

bool launch_arcface_sub_l2norm_t(const float* W, int C, int K, int D, int Dp, bf16* y, bf16* yT, float* inv,
                                 float eps, hipStream_t st) {
  if (!sub_ok(K, Dp) || D > Dp || C < 1) return false;
  const int Wp = arcface_sub_rows(C, K);
  if (Dp == 128)
    hipLaunchKernelGGL(arcs_l2norm_t_kernel<128>, dim3(Wp / 64), dim3(256), 0, st, W, C, K, D, Wp, y, yT, inv, eps);
  else
    hipLaunchKernelGGL(arcs_l2norm_t_kernel<256>, dim3(Wp / 64), dim3(256), 0, st, W, C, K, D, Wp, y, yT, inv, eps);
  return true;
}

bool launch_arcface_sub_fwd(const bf16* xn, const bf16* wn, const int64_t* labels, int B, int Bp, int C, int K,
                            int Dp, float s, float m, int easy, float* lab, int* sub, float* part, float* loss,
                            int* rank, float* lse, hipStream_t st) {
  if (Bp % 64 || !sub_ok(K, Dp)) return false;
  const float cm = cosf(m), sm = sinf(m), th = cosf(3.14159265358979f - m), mm = sinf(3.14159265358979f - m) * m;
  hipLaunchKernelGGL(arcs_label_kernel, dim3(Bp / 4), dim3(256), 0, st, xn, wn, labels, B, Bp, C, K, Dp, s, cm, sm,
                     th, mm, easy, lab, sub);
  SubParams p{};
  p.xn = xn; p.wn = wn; p.labels = labels; p.lab = lab; p.part = part;
  p.B = B; p.Bp = Bp; p.C = C; p.Wp = arcface_sub_rows(C, K); p.s = s;
  p.S = arcface_fused_fwd_splits(Bp, p.Wp);
  p.tps = (p.Wp / kTile + p.S - 1) / p.S;
  const size_t lds = (size_t)kTile * Dp * 2 * 2;
  const dim3 grid(Bp / 64, p.S);
#define ARCS_FWD(KS_, K_)                                                                             \
  score_set_lds((const void*)arcs_rows_kernel<KS_, K_, 0>, lds);                                      \
  hipLaunchKernelGGL((arcs_rows_kernel<KS_, K_, 0>), grid, dim3(256), lds, st, p);
  ARCS_DISPATCH(ARCS_FWD)
#undef ARCS_FWD
  launch_arc_fwd_finalize(part, p.S, B, Bp, C, labels, lab, loss, rank, lse, true, st);
  return true;
}

bool launch_arcface_sub_dx(const bf16* xn, const bf16* wn, const bf16* wnT, const int64_t* labels, int B, int Bp,
                           int C, int K, int Dp, int D, float s, const float* lab, const int* sub, const float* lse,
                           const float* gout, float scale, const float* inv_x, float* part, void* dx, bool dx_bf16,
                           hipStream_t st) {
  if (Bp % 64 || !sub_ok(K, Dp) || D > Dp) return false;
  SubParams p{};
  p.xn = xn; p.wn = wn; p.wnT = wnT; p.labels = labels; p.lab = lab; p.sub = sub; p.lse = lse; p.gout = gout;
  p.part = part; p.scale = scale; p.B = B; p.Bp = Bp; p.C = C; p.Wp = arcface_sub_rows(C, K); p.s = s;
  p.S = arcface_fused_dx_splits(Bp, p.Wp);
  p.tps = (p.Wp / kTile + p.S - 1) / p.S;
  const size_t lds = (size_t)kTile * Dp * 2 * 2 * 2;
  const dim3 grid(Bp / 64, p.S);
#define ARCS_DX(KS_, K_)                                                                              \
  score_set_lds((const void*)arcs_rows_kernel<KS_, K_, 1>, lds);                                      \
  hipLaunchKernelGGL((arcs_rows_kernel<KS_, K_, 1>), grid, dim3(256), lds, st, p);
  ARCS_DISPATCH(ARCS_DX)
#undef ARCS_DX
  const size_t ss = (size_t)Bp * Dp;
  if (dx_bf16)
    hipLaunchKernelGGL(arcs_norm_bwd_kernel<bf16>, dim3(B), dim3(256), 0, st, part, p.S, ss, xn, Dp, D, 0, inv_x,
                       (bf16*)dx);
  else
    hipLaunchKernelGGL(arcs_norm_bwd_kernel<float>, dim3(B), dim3(256), 0, st, part, p.S, ss, xn, Dp, D, 0, inv_x,
                       (float*)dx);
  return true;
}

bool launch_arcface_sub_dw(const bf16* xn, const bf16* xnT, const bf16* wn, const int64_t* labels, int B, int Bp,
                           int C, int K, int Dp, int D, float s, const float* lab, const int* sub, const float* lse,
                           const float* gout, float scale, const float* inv_w, float* part, float* info, float* dw,
                           hipStream_t st) {
  if (Bp % 64 || !sub_ok(K, Dp) || D > Dp) return false;
  SubParams p{};
  p.xn = xn; p.xnT = xnT; p.wn = wn; p.gout = gout; p.info = info; p.part = part;
  p.scale = scale; p.B = B; p.Bp = Bp; p.C = C; p.Wp = arcface_sub_rows(C, K); p.s = s;
  p.S = arcface_fused_dw_splits(Bp, p.Wp);
  if ((p.S > 1 && part == nullptr) || info == nullptr) return false;
  const size_t lds = 2 * ((size_t)kTile * Dp * 2 * 2 + kInfo) + kExch;
  hipLaunchKernelGGL(arcs_rowinfo_kernel, dim3((Bp + 255) / 256), dim3(256), 0, st, labels, lab, sub, lse, B, Bp, C,
                     info);
#define ARCS_DW(KS_, K_)                                                                              \
  score_set_lds((const void*)arcs_dw_kernel<KS_, K_>, lds);                                           \
  hipLaunchKernelGGL((arcs_dw_kernel<KS_, K_>), dim3(p.Wp / 64, p.S), dim3(256), lds, st, p, inv_w, D, dw);
  ARCS_DISPATCH(ARCS_DW)
#undef ARCS_DW
  if (p.S > 1)
    hipLaunchKernelGGL(arcs_norm_bwd_kernel<float>, dim3(C * K), dim3(256), 0, st, part, p.S, (size_t)p.Wp * Dp, wn,
                       Dp, D, K, inv_w, dw);
  return true;
}

}  // namespace dcp

// Fused cosine / dot-product top-k retrieval: for every query row the k (1..8) gallery rows of largest
// score, nothing [Nq, Ng] in memory.  The score tiles live in v_mfma_f32_16x16x32_bf16 accumulators
// only (the streamed tile of score_tile.cuh) and are consumed there by a register top-k selection.
//
// Order, everywhere: score descending, then gallery index ascending (the first of equal scores wins).
// Never a candidate: a gallery index >= Ng (zero padding), the query's exclude[r], a NaN score.
// Fewer than k candidates: the tail is (-inf, -1).  No atomics and a strict total order, so the result
// does not depend on the number of gallery splits.
//
//   operands  knn_prep_kernel       x [R][D] fp32 / bf16 -> bf16 rows [Rp][Dp], zero padded; L2-normalised
//                                   by norm_row (score_tile.cuh: the ArcFace operands' bits) or converted
//   select    knn_rows_kernel       grid (query blocks of 64, S gallery splits), XCD-aware for S % 8 == 0.
//                                   4 waves x 16 query rows, fragments in VGPRs for the whole kernel;
//                                   64-row gallery tiles through a double-buffered LDS-DMA ring.  After
//                                   a tile a lane holds 16 scores of ONE query row whose gallery indices
//                                   c0 + 16 j + 4 q + i ascend in (tile, j, i) order.  It keeps a sorted
//                                   list of KMAX (score, index) pairs in registers; a score enters only
//                                   if it is strictly above the list's tail, so inside a lane the earlier
//                                   index keeps a tie without any index compare.
//                                   Two wave-uniform early-outs (s_cbranch on a ballot): the tile is
//                                   skipped when no lane's tile maximum beats its tail, and inside an
//                                   entered tile each of the 16 candidates is skipped when no lane takes
//                                   it -- the insertion (4 KMAX selects) runs for ~ 64 KMAX / (16 t)
//                                   of the candidates after t tiles.  The padding / exclude mask costs
//                                   nothing on tiles that hold neither (a ballot decides).
//                                   At the end the four lanes of a row (lane ^ 16, lane ^ 32) exchange
//                                   their lists by shuffles and merge them under the full (score desc,
//                                   index asc) order; q == 0 writes the split's partial [S][Nqp][KMAX].
//   merge     knn_merge_kernel      one wave per query row, one lane per split: k rounds of a wave
//                                   arg-best over the lanes' list heads (the winner advances), writes
//                                   val / idx [Nq][k] and first_hit [Nq] = position of the first neighbour
//                                   with the query's label (k if none): the `rank` of metric_accum.
//
// Compile-time widths: Dp = 128 / 256 / 512 (KS = 4 / 8 / 16) x KMAX = 1 / 4 / 8 (the smallest >= k;
// k = 1 is Recall@1 with a one-compare insertion, 4 covers Recall@3).  hipcc 6.x, gfx950:
//
//     KS  KMAX   VGPRs (+ AGPRs)   waves / SIMD by registers   by LDS   LDS
//      4     1      79                 6                        5       32 KB
//      4     4     104                 4                        5       32 KB
//      4     8     148                 3                        5       32 KB
//      8     1      98                 4                        2       64 KB
//      8     4     134                 3                        2       64 KB
//      8     8     170                 2                        2       64 KB
//     16     1     151 + 16            3                        1      128 KB
//     16     4     184 + 30            2                        1      128 KB
//     16     8     227 + 38            1                        1      128 KB
//
// The occupancy is the smaller of the two columns (one workgroup is one wave per SIMD): registers bind
// at Dp = 128 for KMAX 4 and 8, LDS everywhere else.
// Scratch is 0 in every instantiation.
#include "launchers.h"
#include "score_tile.cuh"

namespace dcp {

namespace {

constexpr int kKnnTile = 64;  // gallery rows per staged tile

struct KnnParams {
  const bf16* qn;      // [Nqp][Dp] query operands (rows >= Nq zero)
  const bf16* gn;      // [Ngp][Dp] gallery operands (rows >= Ng zero)
  const int* exclude;  // [Nq] gallery index a query must not return (-1: none), or null
  float* pval;         // [S][Nqp][KMAX]
  int* pidx;           // [S][Nqp][KMAX]
  int Nq, Nqp, Ng, Ngp, tps;
};

// the full order: score descending, index ascending ((-inf, -1) entries after everything)
__device__ __forceinline__ bool knn_before(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && (uint32_t)ia < (uint32_t)ib);
}

// (s, id) into the sorted list, strictly: it passes only entries of smaller score.  For a stream of
// ascending indices that IS the full order.  A score not above the tail changes nothing.
template <int KMAX>
__device__ __forceinline__ void knn_push(float (&v)[KMAX], int (&ix)[KMAX], float s, int id) {
#pragma unroll
  for (int p = KMAX - 1; p >= 1; --p) {
    const bool up = s > v[p - 1], here = s > v[p];
    ix[p] = up ? ix[p - 1] : here ? id : ix[p];
    v[p] = up ? v[p - 1] : here ? s : v[p];
  }
  const bool here = s > v[0];
  ix[0] = here ? id : ix[0];
  v[0] = here ? s : v[0];
}

// the same under the full order (the lists of two lanes interleave in index)
template <int KMAX>
__device__ __forceinline__ void knn_merge_in(float (&v)[KMAX], int (&ix)[KMAX], float s, int id) {
#pragma unroll
  for (int p = KMAX - 1; p >= 1; --p) {
    const bool up = knn_before(s, id, v[p - 1], ix[p - 1]), here = knn_before(s, id, v[p], ix[p]);
    const int ni = up ? ix[p - 1] : here ? id : ix[p];
    v[p] = up ? v[p - 1] : here ? s : v[p];
    ix[p] = ni;
  }
  const bool here = knn_before(s, id, v[0], ix[0]);
  ix[0] = here ? id : ix[0];
  v[0] = here ? s : v[0];
}

template <int N> struct BfVec;
template <> struct BfVec<2> { typedef bf16x2 type; };
template <> struct BfVec<4> { typedef bf16x4 type; };
template <> struct BfVec<8> { typedef bf16x8 type; };

}  // namespace

// rows of x [R][D] (fp32 or bf16) -> bf16 rows y [Rp][DP], zero padded in both dimensions; NORM: norm_row,
// so a row has the bits arc_l2norm_t_kernel gives it.  One wave per row.
template <typename T, int DP, bool NORM>
__global__ void __launch_bounds__(256) knn_prep_kernel(const T* __restrict__ x, int R, int D, int Rp,
                                                       bf16* __restrict__ y, float eps) {
  constexpr int EPL = DP / 64;  // elements per lane of a row
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= Rp) return;
  bf16 b[EPL];
  if constexpr (NORM) {
    norm_row<EPL>(x, r, r < R, D, lane, eps, b);
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int j = lane * EPL + e;
      b[e] = f2bf((r < R && j < D) ? (float)x[(size_t)r * D + j] : 0.f);
    }
  }
  typename BfVec<EPL>::type o;
#pragma unroll
  for (int e = 0; e < EPL; ++e) o[e] = b[e];
  *(typename BfVec<EPL>::type*)(y + (size_t)r * DP + lane * EPL) = o;
}

// Grid (Nqp / 64, S); 4 waves x 16 query rows.  LDS: two [64][DP] swizzled gallery tiles.
template <int KS, int KMAX>
__global__ void __launch_bounds__(256, KS == 16 ? 1 : 2) knn_rows_kernel(const KnnParams p) {
  constexpr int DP = KS * 32, NJ = kKnnTile / 16;
  constexpr int BUF = kKnnTile * DP * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t q = lane >> 4, l15 = lane & 15;
  int rb, split;  // (query block, gallery split)
  xcd_row_split(rb, split);
  const int row = rb * 64 + w * 16 + (int)l15;
  bf16x8 xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const bf16x8*)(p.qn + (size_t)row * DP + ks * 32 + q * 8);
  const int excl = (p.exclude != nullptr && row < p.Nq) ? p.exclude[row] : -1;
  float lv[KMAX];
  int li[KMAX];
#pragma unroll
  for (int e = 0; e < KMAX; ++e) {
    lv[e] = -INFINITY;
    li[e] = -1;
  }

  const int ntiles = p.Ngp / kKnnTile;
  const int t0 = split * p.tps, t1 = min(ntiles, t0 + p.tps);
  if (t0 < t1) dma_rm<DP, kKnnTile>(smem, p.gn, t0 * kKnnTile, w, lane);
  for (int tile = t0; tile < t1; ++tile) {
    const int c0 = tile * kKnnTile, b = (tile - t0) & 1;
    const char* Gt = smem + b * BUF;
    tile_landed();  // this tile landed for every wave; the other buffer's reads are done
    if (tile + 1 < t1) dma_rm<DP, kKnnTile>(smem + (b ^ 1) * BUF, p.gn, (tile + 1) * kKnnTile, w, lane);
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bf16x8 a = *LDS_PTR(const bf16x8, Gt + rm_off(16 * j + l15, ks * 4 + q, DP));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc[j], 0, 0, 0);
      }
    // lane: score of gallery rows c0 + 16 j + 4 q + i (i = 0..3) for its query row
    const int base = c0 + 4 * (int)q;
    const bool edge = c0 + kKnnTile > p.Ng;                         // the tile holds padding rows
    const bool mine = (uint32_t)(excl - c0) < (uint32_t)kKnnTile;  // the tile holds this row's exclusion
    if (edge || __ballot(mine) != 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int g = base + 16 * j + i;
          acc[j][i] = (g >= p.Ng || g == excl) ? -INFINITY : acc[j][i];
        }
    }
    float tmax = -INFINITY;  // (fmaxf drops a NaN; a NaN score fails every compare below)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) tmax = fmaxf(tmax, acc[j][i]);
    if (__ballot(tmax > lv[KMAX - 1]) != 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = acc[j][i];
          if (__ballot(s > lv[KMAX - 1]) != 0) knn_push<KMAX>(lv, li, s, base + 16 * j + i);
        }
    }
  }
  // the 4 lanes of a row (l15, + 16, + 32, + 48): every lane ends with the row's list
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    float ov[KMAX];
    int oi[KMAX];
#pragma unroll
    for (int e = 0; e < KMAX; ++e) {
      ov[e] = __shfl_xor(lv[e], o, 64);
      oi[e] = __shfl_xor(li[e], o, 64);
    }
#pragma unroll
    for (int e = 0; e < KMAX; ++e) knn_merge_in<KMAX>(lv, li, ov[e], oi[e]);
  }
  if (q == 0) {
    const size_t o = ((size_t)split * p.Nqp + row) * KMAX;
#pragma unroll
    for (int e = 0; e < KMAX; ++e) {
      p.pval[o + e] = lv[e];
      p.pidx[o + e] = li[e];
    }
  }
}

// One wave per query row, lane s = split s (S <= 64).  Every split's list is sorted, so the row's k best
// are k rounds of "best head over the lanes"; the indices of different splits are distinct, so exactly
// one lane owns a round's winner and advances.
__global__ void __launch_bounds__(256) knn_merge_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                        int S, int kmax, int Nq, int Nqp, int k,
                                                        const int64_t* __restrict__ ql,
                                                        const int64_t* __restrict__ gl, float* __restrict__ val,
                                                        int* __restrict__ idx, int* __restrict__ first_hit) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= Nq) return;
  const size_t base = ((size_t)lane * Nqp + r) * kmax;
  int pos = 0;
  float hv = -INFINITY;
  int hi = -1;
  if (lane < S) {
    hv = pval[base];
    hi = pidx[base];
  }
  const int64_t yq = ql != nullptr ? ql[r] : 0;
  int fh = k;
  for (int j = 0; j < k; ++j) {
    float bv = hv;
    int bi = hi;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (knn_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      val[(size_t)r * k + j] = bv;
      idx[(size_t)r * k + j] = bi;
    }
    if (bi < 0) continue;  // every head is (-inf, -1): the tail
    if (ql != nullptr && fh == k && gl[bi] == yq) fh = j;
    if (hi == bi) {
      ++pos;
      hv = pos < kmax ? pval[base + pos] : -INFINITY;
      hi = pos < kmax ? pidx[base + pos] : -1;
    }
  }
  if (first_hit != nullptr && lane == 0) first_hit[r] = fh;
}

// ---------------------------------------------------------------------------
bool launch_knn_prep(const void* x, bool is_bf16, int R, int D, int Rp, int Dp, bool normalize, bf16* y, float eps,
                     hipStream_t st) {
  if (Rp % 64 || Rp < R || D > Dp || !score_dp_ok(Dp)) return false;
#define KNN_PREP(T_, DP_)                                                                                        \
  if (normalize)                                                                                                 \
    hipLaunchKernelGGL((knn_prep_kernel<T_, DP_, true>), dim3(Rp / 4), dim3(256), 0, st, (const T_*)x, R, D, Rp, \
                       y, eps);                                                                                  \
  else                                                                                                           \
    hipLaunchKernelGGL((knn_prep_kernel<T_, DP_, false>), dim3(Rp / 4), dim3(256), 0, st, (const T_*)x, R, D,    \
                       Rp, y, eps);
  if (is_bf16) {
    if (Dp == 128) { KNN_PREP(bf16, 128) } else if (Dp == 256) { KNN_PREP(bf16, 256) } else { KNN_PREP(bf16, 512) }
  } else {
    if (Dp == 128) { KNN_PREP(float, 128) } else if (Dp == 256) { KNN_PREP(float, 256) } else { KNN_PREP(float, 512) }
  }
#undef KNN_PREP
  return true;
}

int knn_kmax(int k) { return k < 1 || k > 8 ? 0 : k == 1 ? 1 : k <= 4 ? 4 : 8; }

int knn_splits(int Nqp, int Ngp) {
  // ~ 1024 workgroups (4 per CU), at most 64 splits (the merge kernel's lanes); multiples of 8 take
  // the XCD-aware mapping
  return score_splits(Nqp / 64, Ngp / kKnnTile, 1024, 64);
}

bool launch_knn_topk(const bf16* qn, const bf16* gn, int Nq, int Nqp, int Ng, int Ngp, int Dp, int k, int S,
                     const int* exclude, const int64_t* q_labels, const int64_t* g_labels, float* pval, int* pidx,
                     float* val, int* idx, int* first_hit, hipStream_t st) {
  const int kmax = knn_kmax(k);
  if (Nqp % 64 || Ngp % kKnnTile || Nq < 1 || Nq > Nqp || Ng < 1 || Ng > Ngp || !score_dp_ok(Dp) || kmax == 0 ||
      S < 1 || S > 64)
    return false;
  if ((q_labels == nullptr) != (g_labels == nullptr) || (q_labels != nullptr && first_hit == nullptr)) return false;
  KnnParams p{};
  p.qn = qn; p.gn = gn; p.exclude = exclude; p.pval = pval; p.pidx = pidx;
  p.Nq = Nq; p.Nqp = Nqp; p.Ng = Ng; p.Ngp = Ngp;
  p.tps = (Ngp / kKnnTile + S - 1) / S;
  const size_t lds = (size_t)kKnnTile * Dp * 2 * 2;
  const dim3 grid(Nqp / 64, S);
#define KNN_ROWS(KS_, KM_)                                                                                      \
  {                                                                                                             \
    score_set_lds((const void*)knn_rows_kernel<KS_, KM_>, lds);                                                 \
    hipLaunchKernelGGL((knn_rows_kernel<KS_, KM_>), grid, dim3(256), lds, st, p);                               \
  }
#define KNN_ROWS_K(KS_) \
  if (kmax == 1) KNN_ROWS(KS_, 1) else if (kmax == 4) KNN_ROWS(KS_, 4) else KNN_ROWS(KS_, 8)
  if (Dp == 128) { KNN_ROWS_K(4) } else if (Dp == 256) { KNN_ROWS_K(8) } else { KNN_ROWS_K(16) }
#undef KNN_ROWS_K
#undef KNN_ROWS
  hipLaunchKernelGGL(knn_merge_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, pval, pidx, S, kmax, Nq, Nqp, k, q_labels,
                     g_labels, val, idx, first_hit);
  return true;
}

// the merge alone, for the wide selection of knn_wide.hip (kmax = its KCAP)
void launch_knn_merge(const float* pval, const int* pidx, int S, int kmax, int Nq, int Nqp, int k, float* val,
                      int* idx, hipStream_t st) {
  hipLaunchKernelGGL(knn_merge_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, pval, pidx, S, kmax, Nq, Nqp, k,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, val, idx, (int*)nullptr);
}

}  // namespace dcp

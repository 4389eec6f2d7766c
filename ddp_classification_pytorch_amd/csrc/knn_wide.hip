// Fused cosine / dot-product top-k for 1 <= k <= 256 and the weighted kNN label vote on top of it.
// The streamed tile is score_tile.cuh's.  Same contract as knn.hip (operands from knn_prep_kernel,
// order = score descending then gallery index ascending, never a candidate: padding rows, exclude[r],
// NaN scores; tail (-inf, -1); the bits do not depend on the number of gallery splits), another
// selection: a register list costs KMAX selects per insertion and stops at 8, so here every query row
// of the workgroup owns a CANDIDATE POOL in LDS.
//
//   select  knn_pool_rows_kernel  grid (query blocks of 32, S gallery splits), XCD-aware for S % 8 == 0.
//                                 4 waves = 2 query groups of 16 rows x 2 halves of the T-row gallery tile;
//                                 query fragments in VGPRs, gallery tiles through the double-buffered
//                                 LDS-DMA ring, scores in v_mfma_f32_16x16x32_bf16 accumulators.
//           the pool              per query row P = KCAP + NEW 64-bit keys (score bits made order
//                                 preserving << 32 | ~index: one unsigned compare IS the full order; -0.0
//                                 packs as +0.0, the (-inf, -1) filler packs below everything that can
//                                 enter), a fill counter and a threshold thr.  Slots [0, KCAP) are the
//                                 row's best so far, sorted (fillers at the end); thr is the score of slot
//                                 KCAP - 1.  A lane whose score is STRICTLY above thr takes slots
//                                 [KCAP, count) with one LDS atomic add per lane and stores its keys there.
//                                 Strict is exact: inside a split gallery indices ascend with the tiles, so
//                                 a later score equal to thr ranks behind the KCAP entries already held.
//                                 -inf (masked) and NaN fail the compare.  The append order is arbitrary,
//                                 the top KCAP of a set under a strict total order is not.
//           the prune             a row whose count exceeds P - T before a tile is pruned by ONE wave
//                                 (wave w owns rows w, w + 4, ..): the n = count - KCAP new keys are
//                                 sorted by a bitonic network (every comparator sends the larger key to
//                                 the lower slot, so comparators that touch a slot >= count are skipped:
//                                 those slots act as minus infinity), then one flip step (slot KCAP - 1 - c
//                                 against KCAP + c, c < n) leaves the best KCAP of the union as a bitonic
//                                 sequence in [0, KCAP) and log2(KCAP) half-cleaner steps sort it.
//                                 Wave-synchronous (lgkmcnt(0) between steps), no workgroup barrier
//                                 inside; rows prune at their own pace.  Two barriers per tile: A (the
//                                 tile landed, the appends of the last tile are complete), then the
//                                 owners prune, then B (unconditional, so never divergent) before thr is
//                                 read and anything is appended.  The next tile's DMA is in flight.
//           the end               every row is pruned once more and [0, KCAP) decoded into the split's
//                                 sorted partial [S][Nqp][KCAP].
//   merge   knn_merge_kernel (knn.hip), kmax = KCAP, cuts to k.
//   vote    knn_vote_kernel       one wave per query row over val / idx [Nq][k]: weights
//                                 exp((val_j - val_0) / T) or 1 and labels in LDS, a lane per neighbour
//                                 sums the weights of the neighbours sharing its label in ascending j,
//                                 a wave arg-best under (vote descending, class ascending) picks pred.
//                                 No atomics, nothing [Nq, C]: the class count never enters.
//
// Instantiations (KS = Dp / 32).  KCAP = 64 serves k <= 64, KCAP = 256 the rest; T = gallery rows per
// tile; a row is pruned when more than NEW - T new keys wait.  hipcc 6.x, gfx950, 256 threads, one
// workgroup per CU wherever LDS is above 80 KB:
//
//     KS  KCAP   T  NEW   ring     pool     LDS total   VGPRs (+ AGPRs)   scratch
//      4    64  32   64   16 KB    32 KB     48.3 KB     60 + 4            0
//      8    64  32   64   32 KB    32 KB     64.3 KB     86 + 4            0
//     16    64  32   64   64 KB    32 KB     96.3 KB    126 + 4            0
//      4   256  64  112   32 KB    92 KB    124.3 KB     70 + 8            0
//      8   256  64  112   64 KB    92 KB    156.3 KB    100 + 8            0
//     16   256  32  112   64 KB    92 KB    156.3 KB    130 + 4            0
//
// Scratch is 0 in every instantiation.
#include "launchers.h"
#include "score_tile.cuh"

namespace dcp {

namespace {

constexpr int kPoolRows = 32;  // query rows per workgroup

struct KnnPoolParams {
  const bf16* qn;      // [Nqp][Dp] query operands (rows >= Nq zero)
  const bf16* gn;      // [Ngp][Dp] gallery operands (rows >= Ng zero)
  const int* exclude;  // [Nq] gallery index a query must not return (-1: none), or null
  float* pval;         // [S][Nqp][KCAP]
  int* pidx;           // [S][Nqp][KCAP]
  int Nq, Nqp, Ng, Ngp, tps;
};

// (score, index) as one key: a larger key is earlier in the order (score descending, index ascending)
constexpr uint64_t kPoolFiller = 0x007FFFFF00000000ull;  // (-inf, -1): below every key that can enter
__device__ __forceinline__ uint64_t pool_key(float s, int id) {
  uint32_t u = __float_as_uint(s + 0.0f);  // -0.0 -> +0.0: equal scores, equal bits
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (uint32_t)~id;
}
__device__ __forceinline__ float key_score(uint64_t k) {
  const uint32_t h = (uint32_t)(k >> 32);
  return __uint_as_float((h & 0x80000000u) ? (h ^ 0x80000000u) : ~h);
}
__device__ __forceinline__ int key_index(uint64_t k) { return (int)~(uint32_t)k; }

// one wave, between two steps of a network: the step's LDS traffic is complete and stays in order
__device__ __forceinline__ void pool_step_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// comparator: the larger key to slot i < l; a slot >= n counts as minus infinity (nothing to do)
__device__ __forceinline__ void pool_ce(uint64_t* s, int i, int l, int n) {
  if (l < n) {
    const uint64_t a = s[i], b = s[l];
    if (b > a) {
      s[i] = b;
      s[l] = a;
    }
  }
}

// One wave: row pool pr with [0, KCAP) sorted and cnt - KCAP > 0 unsorted keys behind -> the best KCAP of
// all of them sorted in [0, KCAP).  cnt is wave-uniform.
template <int KCAP>
__device__ __forceinline__ void pool_prune(uint64_t* pr, int cnt, int lane) {
  const int n = cnt - KCAP;
  int NB = 2;
  while (NB < n) NB <<= 1;  // <= 128 <= KCAP for KCAP = 256, <= 64 for KCAP = 64
  uint64_t* nb = pr + KCAP;
  // the new keys, descending: merges of blocks of k (a flip step, then strides k / 4 .. 1)
  for (int k = 2; k <= NB; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int c = lane; c < (NB >> 1); c += 64) {
        const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
        pool_ce(nb, i, j == (k >> 1) ? (i ^ (k - 1)) : (i | j), n);
      }
      pool_step_sync();
    }
  // the flip step of the merge of [0, KCAP) with the new block: only the pairs whose upper slot exists
  for (int c = lane; c < n; c += 64) pool_ce(pr, KCAP - 1 - c, KCAP + c, cnt);
  pool_step_sync();
  // [0, KCAP) holds the best KCAP as a bitonic sequence; whatever is behind it is dropped
  for (int j = KCAP >> 1; j > 0; j >>= 1) {
    for (int c = lane; c < (KCAP >> 1); c += 64) {
      const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
      pool_ce(pr, i, i | j, KCAP);
    }
    pool_step_sync();
  }
}

}  // namespace

// Grid (Nqp / 32, S).  LDS: two [T][DP] swizzled gallery tiles, 32 pools of P keys, 32 counters, 32 thr.
template <int KS, int KCAP, int T, int NEW>
__global__ void __launch_bounds__(256, 1) knn_pool_rows_kernel(const KnnPoolParams p) {
  constexpr int DP = KS * 32, NJ = T / 32, BUF = T * DP * 2, P = KCAP + NEW;
  static_assert(NEW > T && NEW <= KCAP && NEW <= 128, "room for one tile past the prune level; NB <= KCAP");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* pool = (uint64_t*)(smem + 2 * BUF);
  int* cntL = (int*)(pool + kPoolRows * P);
  float* thrL = (float*)(cntL + kPoolRows);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qg = w & 1, half = w >> 1;  // query rows 16 qg .., gallery rows half T / 2 .. of a tile
  const uint32_t q = lane >> 4, l15 = lane & 15;
  int rb, split;  // (query block, gallery split)
  xcd_row_split(rb, split);
  const int lrow = qg * 16 + (int)l15, row = rb * kPoolRows + lrow;
  bf16x8 xf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) xf[ks] = *(const bf16x8*)(p.qn + (size_t)row * DP + ks * 32 + q * 8);
  const int excl = (p.exclude != nullptr && row < p.Nq) ? p.exclude[row] : -1;
  uint64_t* prow = pool + lrow * P;

  for (int e = tid; e < kPoolRows * P; e += 256) pool[e] = kPoolFiller;
  if (tid < kPoolRows) {
    cntL[tid] = KCAP;
    thrL[tid] = -INFINITY;
  }

  const int ntiles = p.Ngp / T;
  const int t0 = split * p.tps, t1 = min(ntiles, t0 + p.tps);
  if (t0 < t1) dma_rm<DP, T>(smem, p.gn, t0 * T, w, lane);
  for (int tile = t0; tile < t1; ++tile) {
    const int c0 = tile * T, b = (tile - t0) & 1;
    const char* Gt = smem + b * BUF;
    tile_landed();  // A: this tile landed; the last tile's reads and appends are complete
    if (tile + 1 < t1) dma_rm<DP, T>(smem + (b ^ 1) * BUF, p.gn, (tile + 1) * T, w, lane);
    // Nobody appends between A and B, so the counters are stable; a wave looks at its own 8 rows only
    // and B is unconditional: no barrier depends on what a wave read.
    // INVARIANT: after B every count is <= P - T, a tile appends at most T keys to a row, so a slot
    // index is always < P.
    if (__ballot(cntL[w + 4 * (lane & 7)] > P - T) != 0) {
      for (int r = w; r < kPoolRows; r += 4) {
        const int cr = __builtin_amdgcn_readfirstlane(cntL[r]);
        if (cr > P - T) {
          pool_prune<KCAP>(pool + r * P, cr, lane);
          if (lane == 0) {
            thrL[r] = key_score(pool[r * P + KCAP - 1]);
            cntL[r] = KCAP;
          }
        }
      }
    }
    __syncthreads();  // B
    const float thr = thrL[lrow];
    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const bf16x8 a = *LDS_PTR(const bf16x8, Gt + rm_off(half * (T / 2) + 16 * j + l15, ks * 4 + q, DP));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[ks], acc[j], 0, 0, 0);
      }
    // lane: score of gallery rows base + 16 j + i (i = 0..3) for its query row
    const int base = c0 + half * (T / 2) + 4 * (int)q;
    const bool edge = c0 + T > p.Ng;                         // the tile holds padding rows
    const bool mine = (uint32_t)(excl - c0) < (uint32_t)T;  // the tile holds this row's exclusion
    if (edge || __ballot(mine) != 0) {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int g = base + 16 * j + i;
          acc[j][i] = (g >= p.Ng || g == excl) ? -INFINITY : acc[j][i];
        }
    }
    float tmax = -INFINITY;  // (fmaxf drops a NaN; a NaN score fails the compare below)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) tmax = fmaxf(tmax, acc[j][i]);
    if (__ballot(tmax > thr) != 0) {  // the tile maximum beats nothing: no append at all
      int n = 0;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) n += acc[j][i] > thr ? 1 : 0;
      if (n > 0) {
        int slot = atomicAdd(&cntL[lrow], n);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (acc[j][i] > thr) prow[slot++] = pool_key(acc[j][i], base + 16 * j + i);
      }
    }
  }
  __syncthreads();  // every append (and, for an empty split, the initial fill) is complete
  for (int r = w; r < kPoolRows; r += 4) {
    const int cr = __builtin_amdgcn_readfirstlane(cntL[r]);
    if (cr > KCAP) pool_prune<KCAP>(pool + r * P, cr, lane);
    const size_t o = ((size_t)split * p.Nqp + rb * kPoolRows + r) * KCAP;
    for (int e = lane; e < KCAP; e += 64) {
      const uint64_t key = pool[r * P + e];
      p.pval[o + e] = key_score(key);
      p.pidx[o + e] = key_index(key);
    }
  }
}

// One wave per query row, k <= 256.  vote(c) = sum of w_j over the valid neighbours of label c, W = sum
// of w_j, both in ascending j; pred = largest vote, smallest class among equals (-1: no valid neighbour);
// conf = vote(pred) / W, agree = vote(q_label) / W (0 with no valid neighbour).
__global__ void __launch_bounds__(256) knn_vote_kernel(const float* __restrict__ val, const int* __restrict__ idx,
                                                       int Nq, int k, int Ng, const int64_t* __restrict__ gl,
                                                       const int64_t* __restrict__ ql, float temperature,
                                                       int weighted, int64_t* __restrict__ pred,
                                                       float* __restrict__ conf, float* __restrict__ agree) {
  __shared__ float sw[4][256];
  __shared__ long long sl[4][256];
  __shared__ int sv[4][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + wv;
  if (r >= Nq) return;  // (a whole wave; no workgroup barrier below)
  const float v0 = val[(size_t)r * k];
  long long myl[4];
  bool myv[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int j = s * 64 + lane;
    myv[s] = false;
    myl[s] = 0;
    if (j < k) {
      const int id = idx[(size_t)r * k + j];
      myv[s] = (uint32_t)id < (uint32_t)Ng;
      if (myv[s]) myl[s] = gl[id];
      sw[wv][j] = weighted ? expf((val[(size_t)r * k + j] - v0) / temperature) : 1.f;
      sl[wv][j] = myl[s];
      sv[wv][j] = myv[s] ? 1 : 0;
    }
  }
  pool_step_sync();
  const long long yq = ql != nullptr ? ql[r] : 0;
  float W = 0.f, vq = 0.f, vote[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < k; ++i) {
    if (sv[wv][i] == 0) continue;  // (wave-uniform)
    const float wi = sw[wv][i];
    const long long li = sl[wv][i];
    W += wi;
    vq += li == yq ? wi : 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) vote[s] += li == myl[s] ? wi : 0.f;
  }
  // arg-best under (vote descending, class ascending); -1 marks "no neighbour" (votes are >= 0)
  float bv = -1.f;
  long long bc = -1;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (myv[s] && (vote[s] > bv || (vote[s] == bv && myl[s] < bc))) {
      bv = vote[s];
      bc = myl[s];
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const long long oc = __shfl_xor(bc, o, 64);
    if (ov > bv || (ov == bv && ov >= 0.f && oc < bc)) {
      bv = ov;
      bc = oc;
    }
  }
  if (lane == 0) {
    const bool any = bv >= 0.f;
    pred[r] = any ? bc : -1;
    conf[r] = any ? bv / W : 0.f;
    if (agree != nullptr) agree[r] = any ? vq / W : 0.f;
  }
}

// ---------------------------------------------------------------------------
int knn_wide_kcap(int k) { return k < 1 || k > 256 ? 0 : k <= 64 ? 64 : 256; }

namespace {
int knn_wide_tile(int Dp, int kcap) { return kcap == 256 && Dp <= 256 ? 64 : 32; }
}  // namespace

int knn_wide_splits(int Nqp, int Ngp) {
  // ~ 1024 workgroups of 32 query rows, at most 64 splits (the merge kernel's lanes), multiples of 8 for
  // the XCD-aware mapping: S blocks < 1024 + blocks, so the partials hold fewer than (32768 + Nqp) KCAP
  // (score, index) pairs
  return score_splits(Nqp / kPoolRows, Ngp / 64, 1024, 64);
}

bool launch_knn_topk_wide(const bf16* qn, const bf16* gn, int Nq, int Nqp, int Ng, int Ngp, int Dp, int k, int S,
                          const int* exclude, float* pval, int* pidx, float* val, int* idx, hipStream_t st) {
  const int kcap = knn_wide_kcap(k);
  if (Nqp % 64 || Ngp % 64 || Nq < 1 || Nq > Nqp || Ng < 1 || Ng > Ngp || !score_dp_ok(Dp) ||
      kcap == 0 || S < 1 || S > 64)
    return false;
  const int T = knn_wide_tile(Dp, kcap), NEW = kcap == 256 ? 112 : 64;
  KnnPoolParams p{};
  p.qn = qn; p.gn = gn; p.exclude = exclude; p.pval = pval; p.pidx = pidx;
  p.Nq = Nq; p.Nqp = Nqp; p.Ng = Ng; p.Ngp = Ngp;
  p.tps = (Ngp / T + S - 1) / S;
  const size_t lds = (size_t)T * Dp * 2 * 2 + (size_t)kPoolRows * (kcap + NEW) * 8 + kPoolRows * 8;
  const dim3 grid(Nqp / kPoolRows, S);
  bool ok = true;
#define KNN_POOL(KS_, KC_, T_, NEW_)                                                                          \
  {                                                                                                           \
    ok = hipFuncSetAttribute((const void*)knn_pool_rows_kernel<KS_, KC_, T_, NEW_>,                           \
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;             \
    if (ok) hipLaunchKernelGGL((knn_pool_rows_kernel<KS_, KC_, T_, NEW_>), grid, dim3(256), lds, st, p);      \
  }
  if (kcap == 64) {
    if (Dp == 128) KNN_POOL(4, 64, 32, 64) else if (Dp == 256) KNN_POOL(8, 64, 32, 64) else KNN_POOL(16, 64, 32, 64)
  } else {
    if (Dp == 128) KNN_POOL(4, 256, 64, 112) else if (Dp == 256) KNN_POOL(8, 256, 64, 112) else KNN_POOL(16, 256, 32, 112)
  }
#undef KNN_POOL
  if (!ok) return false;
  launch_knn_merge(pval, pidx, S, kcap, Nq, Nqp, k, val, idx, st);
  return true;
}

bool launch_knn_vote(const float* val, const int* idx, int Nq, int k, int Ng, const int64_t* g_labels,
                     const int64_t* q_labels, float temperature, bool weighted, int64_t* pred, float* conf,
                     float* agree, hipStream_t st) {
  if (Nq < 1 || k < 1 || k > 256 || Ng < 1 || !(temperature > 0.f) || (q_labels == nullptr) != (agree == nullptr))
    return false;
  hipLaunchKernelGGL(knn_vote_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, val, idx, Nq, k, Ng, g_labels, q_labels,
                     temperature, weighted ? 1 : 0, pred, conf, agree);
  return true;
}

}  // namespace dcp

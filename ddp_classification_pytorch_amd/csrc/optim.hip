// Fused multi-tensor optimizer steps and the CDR critical-parameter gradient
// mask.
//
// * SGD (momentum, dampening, weight decay, nesterov) and Adam/AdamW replace
//   torch.optim.SGD/Adam used at BASELINE/main.py:153, ARCFACE/arc_main.py:249-253,
//   CDR/main.py:339, NESTED/train.py:386-392, PLC/utils.py:237 (SURVEY.md
//   §2.5 K14/K15). One launch updates every parameter: a device table lists
//   (param, grad, state, bf16 shadow) per tensor and a chunk table maps
//   workgroups to 4096-element slices.  The step optionally refreshes the
//   bf16 compute copy of each weight, so the forward pass reads weights that
//   the optimizer already converted.
// * LARS over the same tables: per-chunk sums of squares, a per-tensor trust ratio, the SGD update on
//   the scaled gradient; the learning rate optionally from a device scalar (HIP-graph replay under
//   a per-iteration schedule).
// * LAMB over the same tables and scratch: Adam's moments with the per-chunk sums of w^2 and u^2, the
//   per-tensor trust ratio |w| / |u|, the update on the recomputed u.  Adam reads its learning rate
//   from a device scalar too when one is given.
// * Global gradient-norm clipping and the non-finite skip in front of Adam, LARS (FusedSGD through it)
//   and LAMB: per-chunk sums of g^2, one workgroup that merges them into a device control block
//   (coefficient, skip flag, norm), which every update kernel reads.
// * The exponential moving average of the weights over the same tables (mt_ema: e += omd (w - e), omd
//   from a device scalar, honouring the skip flag) and the in-place exchange of weights and averages
//   that evaluation on the average uses (mt_swap).
// * CDR (CDR/main.py:186-204): threshold = k-th largest |g*w| over all 2-D/4-D
//   parameters, found by a 4-pass 8-bit radix select over the float bit
//   patterns (non-negative floats order like their uint32 bits) without
//   materialising the 25.6M-element concatenation or sorting it; then
//   g *= (|g*w| >= thr) * clip in place.
#include "common.cuh"
#include "launchers.h"

namespace dcp {


constexpr int kChunk = 4096;


// One element of the SGD update, shared by the 16-byte and the 4-byte loop.  The fused multiply-adds
// are explicit, so that both loops round alike whatever the compiler contracts in either: a gradient
// view at an odd offset steps exactly as an aligned one does.
__device__ __forceinline__ void sgd_elem(float gin, float& p, float& b, const SgdHyper& h) {
  float g = gin * h.grad_scale;
  if (h.wd != 0.f) g = fmaf(h.wd, p, g);
  if (h.momentum != 0.f) {
    b = h.first ? g : fmaf(1.f - h.dampening, g, h.momentum * b);
    g = h.nesterov ? fmaf(h.momentum, b, g) : b;
  }
  p = fmaf(-h.lr, g, p);
}

__global__ void __launch_bounds__(256) mt_sgd_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                     SgdHyper h) {
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  // 16-byte path (uniform per chunk): the 4-byte loop kept one 4-byte load per lane and tensor in
  // flight per iteration (96 us for ResNet-50's 25.6M parameters, ~5.3 TB/s); the per-element math
  // is the same function (sgd_elem), so both paths give identical results.  Bucket views at odd
  // offsets take the scalar loop.
  const uintptr_t mis = ((uintptr_t)(e.p + base) | (uintptr_t)(e.g + base) |
                         (h.momentum != 0.f ? (uintptr_t)(e.s1 + base) : 0)) & 15u;
  const uintptr_t smis = e.shadow ? ((uintptr_t)(e.shadow + base) & 7u) : 0;
  if (mis == 0 && smis == 0 && ((end - base) & 3) == 0) {
    const int64_t n4 = (end - base) >> 2;
    float4* p4 = (float4*)(e.p + base);
    const float4* g4 = (const float4*)(e.g + base);
    float4* s4 = (float4*)(e.s1 + base);
#pragma unroll 4
    for (int64_t j = threadIdx.x; j < n4; j += blockDim.x) {
      float gv[4], pv[4], bv[4];
      *(float4*)gv = g4[j];
      *(float4*)pv = p4[j];
      const bool mom = h.momentum != 0.f;
      if (mom && !h.first) *(float4*)bv = s4[j];
#pragma unroll
      for (int u = 0; u < 4; ++u) sgd_elem(gv[u], pv[u], bv[u], h);
      if (mom) s4[j] = *(float4*)bv;
      p4[j] = *(float4*)pv;
      if (e.shadow) {
        bf16x4 sv;
#pragma unroll
        for (int u = 0; u < 4; ++u) sv[u] = f2bf(pv[u]);
        *(bf16x4*)(e.shadow + base + 4 * j) = sv;
      }
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    float p = e.p[i];
    float b = (h.momentum != 0.f && !h.first) ? e.s1[i] : 0.f;
    sgd_elem(e.g[i], p, b, h);
    if (h.momentum != 0.f) e.s1[i] = b;
    e.p[i] = p;
    if (e.shadow) e.shadow[i] = f2bf(p);
  }
}


// ---------------------------------------------------------------------------
// Global gradient-norm clipping and the non-finite skip.
//   norm = fl32(sqrt(sum over parameters of (grad_scale g)^2)), the sum merged in fp64
//   coef = max_norm / (norm + 1e-6), replaced by 1 when it exceeds 1 (clip_grad_norm_'s formula)
// The clipped step IS the plain step with grad_scale' = fl32(grad_scale coef): every update kernel
// forms that product once (clip_scale) and uses it wherever it used grad_scale.  With the skip flag
// set a kernel returns before it writes anything.  A null control block leaves every kernel as it was.
// ---------------------------------------------------------------------------

// wave-uniform: whether this step is skipped, and the effective grad_scale of the launch
__device__ __forceinline__ bool clip_skip(const ClipCtl* c) { return c && c->skip != 0; }
__device__ __forceinline__ float clip_scale(float grad_scale, const ClipCtl* c) {
  return c ? __fmul_rn(grad_scale, c->coef) : grad_scale;
}

// One workgroup per chunk: partials[slots[entry] + chunk] = (sum g^2 of the chunk, this step's
// epoch).  mt_norm2_kernel's ownership and order: thread t owns the chunk elements 4 (t + 256 k) + u
// and accumulates them in that order with one fused multiply-add each, then block_sum; the 16-byte
// path loads the same four elements as one float4.  Gradients only: 4 B / element.  The epoch stamp
// marks the slot as written in this step: gnorm_finish counts no slot of an earlier step, so a
// parameter without a gradient drops out of the norm without a host-side clear.
__global__ void __launch_bounds__(256) mt_gnorm2_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                        const int* __restrict__ slots, const ClipCtl* __restrict__ ctl,
                                                        GnormPartial* __restrict__ partials) {
  __shared__ float red[16];
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int len = (int)(min(e.n, base + kChunk) - base);
  const float* g = e.g + base;
  float sg = 0.f;
  if ((((uintptr_t)g) & 15u) == 0 && (len & 3) == 0) {
    const int n4 = len >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x + 256 * k;
      if (j < n4) {
        float gv[4];
        *(float4*)gv = ((const float4*)g)[j];
#pragma unroll
        for (int u = 0; u < 4; ++u) sg = fmaf(gv[u], gv[u], sg);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i0 = 4 * (threadIdx.x + 256 * k);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i0 + u < len) {
          const float gv = g[i0 + u];
          sg = fmaf(gv, gv, sg);
        }
      }
    }
  }
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) {
    GnormPartial o;
    o.sum = sg;
    o.epoch = ctl->epoch;
    partials[slots[ck.x] + ck.y] = o;
  }
}

// One workgroup: every slot of the optimizer merged in fp64 in a fixed order (thread t takes slots
// t, t + 256, ... serially, then the shared-memory tree of merge_partials), each weighted with its
// group's grad_scale^2; slots not stamped with this step's epoch count as zero.  The norm is rounded
// to fp32 once; the coefficient is formed in fp32.  A NaN norm gives a NaN coefficient (the compare
// is false, nothing is replaced).  Thread 0 then opens the next epoch.
__global__ void __launch_bounds__(256) gnorm_finish_kernel(const GnormPartial* __restrict__ partials, int nslots,
                                                           const float* __restrict__ slot_gs, float max_norm,
                                                           int skip_nonfinite, ClipCtl* __restrict__ ctl) {
  __shared__ double sh[256];
  const unsigned epoch = ctl->epoch;
  double a = 0.0;
  for (int c = threadIdx.x; c < nslots; c += 256) {
    const GnormPartial v = partials[c];
    const double gs = (double)slot_gs[c];
    if (v.epoch == epoch) a += gs * gs * (double)v.sum;
  }
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(sh[0]);
    float coef = 1.f;
    if (max_norm > 0.f) {
      coef = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
      if (coef > 1.f) coef = 1.f;
    }  // max_norm 0: the norm is computed for the skip flag only
    const int skip = (skip_nonfinite && !(fabsf(norm) <= 3.402823466e+38f)) ? 1 : 0;
    ctl->coef = coef;
    ctl->skip = skip;
    ctl->norm = norm;
    ctl->skipped += skip;
    ctl->epoch = epoch + 1u;
  }
}

// ---------------------------------------------------------------------------
// LARS (layer-wise adaptive rate scaling; You, Gitman, Ginsburg 2017), "scaled gradient into SGD":
//   g~ = grad_scale g;  trust = eta |w| / (|g~| + wd |w| + eps)  (1 when not adaptive or a norm is 0);
//   d = trust (g~ + wd w);  then the SGD momentum / nesterov update on d with no further decay.
// Three launches per (group, first / not-first) subset: per-chunk sums of squares, the per-tensor
// trust ratio, the update.  Every reduction has a fixed order (no float atomics): a step is
// bit-reproducible, and the same values give the same trust ratio at any pointer alignment.
// ---------------------------------------------------------------------------

// One workgroup per chunk: partials[blockIdx.x] = (sum w^2, sum g^2) of the chunk.  Thread t owns
// the chunk elements 4 (t + 256 k) + u, k, u = 0..3, and accumulates them in that order with one
// fused multiply-add each; then the wave butterfly and the serial sum over the four waves
// (block_sum).  The 16-byte path loads the same four elements as one float4, so both paths add the
// same values in the same order.
__global__ void __launch_bounds__(256) mt_norm2_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                       float2* __restrict__ partials) {
  __shared__ float red[2][16];
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int len = (int)(min(e.n, base + kChunk) - base);
  const float* p = e.p + base;
  const float* g = e.g + base;
  float sw = 0.f, sg = 0.f;
  const uintptr_t mis = ((uintptr_t)p | (uintptr_t)g) & 15u;
  if (mis == 0 && (len & 3) == 0) {
    const int n4 = len >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x + 256 * k;
      if (j < n4) {
        float pv[4], gv[4];
        *(float4*)pv = ((const float4*)p)[j];
        *(float4*)gv = ((const float4*)g)[j];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          sw = fmaf(pv[u], pv[u], sw);
          sg = fmaf(gv[u], gv[u], sg);
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i0 = 4 * (threadIdx.x + 256 * k);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i0 + u < len) {
          const float pv = p[i0 + u], gv = g[i0 + u];
          sw = fmaf(pv, pv, sw);
          sg = fmaf(gv, gv, sg);
        }
      }
    }
  }
  sw = block_sum(sw, red[0]);
  sg = block_sum(sg, red[1]);
  if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(sw, sg);
}

// One workgroup per tensor: its chunk partials summed in fp64 in a fixed order (thread t takes
// partials t, t + 256, ... serially, then a shared-memory tree), so the merge adds no rounding of
// its own; |w| and |grad_scale| |g| are rounded to fp32 once and the ratio is formed in fp32.
// The fixed-order fp64 merge of one tensor's chunk partials (256 threads); the sums end in sh[.][0].
__device__ __forceinline__ void merge_partials(const int2 sp, const float2* __restrict__ partials, double (*sh)[256]) {
  double aw = 0.0, ag = 0.0;
  for (int c = threadIdx.x; c < sp.y; c += 256) {
    const float2 v = partials[sp.x + c];
    aw += (double)v.x;
    ag += (double)v.y;
  }
  sh[0][threadIdx.x] = aw;
  sh[1][threadIdx.x] = ag;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + o];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + o];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) lars_trust_kernel(const int2* __restrict__ spans, const float2* __restrict__ partials,
                                                         float grad_scale, float wd, float eta, float eps,
                                                         float* __restrict__ trust, LarsHyper lh) {
  __shared__ double sh[2][256];
  if (clip_skip(lh.clip)) return;  // a skipped step keeps the last step's ratios
  grad_scale = clip_scale(grad_scale, lh.clip);
  merge_partials(spans[blockIdx.x], partials, sh);  // spans: (first chunk, number of chunks)
  if (threadIdx.x == 0) {
    const float wn = (float)sqrt(sh[0][0]);
    const float gn = (float)(fabs((double)grad_scale) * sqrt(sh[1][0]));
    float t = 1.f;
    if (wn > 0.f && gn > 0.f) {
      t = eta * wn / (fmaf(wd, wn, gn) + eps);
      if (lh.trust_clip) {  // LARC's clip mode: the local rate lr * t never exceeds lr
        const float lr = lh.lr_dev ? *lh.lr_dev : lh.sgd.lr;
        t = lr > 0.f ? __fdiv_rn(t, lr) : 1.f;
        if (t > 1.f) t = 1.f;
      }
    }
    trust[blockIdx.x] = t;
  }
}

// mt_sgd_kernel's two loops with d = trust * (grad_scale g + wd p) in front of sgd_elem (which then
// runs with wd = 0, grad_scale = 1: d * 1 is exact, so a trust ratio of 1 steps exactly as mt_sgd
// does).  The learning rate comes from the device scalar when one is given: a replayed HIP graph
// then follows a per-iteration schedule without recapture.
__device__ __forceinline__ float lars_dir(float g, float p, float trust, float gs, float wd) {
  float d = g * gs;
  if (wd != 0.f) d = fmaf(wd, p, d);
  return trust * d;
}

__global__ void __launch_bounds__(256) mt_lars_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                      LarsHyper lh) {
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  if (clip_skip(lh.clip)) return;
  SgdHyper h = lh.sgd;
  const float gs = clip_scale(h.grad_scale, lh.clip), wd = h.wd;
  h.grad_scale = 1.f;
  h.wd = 0.f;
  if (lh.lr_dev) h.lr = *lh.lr_dev;
  const float trust = lh.trust ? lh.trust[ck.x] : 1.f;
  const uintptr_t mis = ((uintptr_t)(e.p + base) | (uintptr_t)(e.g + base) |
                         (h.momentum != 0.f ? (uintptr_t)(e.s1 + base) : 0)) & 15u;
  const uintptr_t smis = e.shadow ? ((uintptr_t)(e.shadow + base) & 7u) : 0;
  if (mis == 0 && smis == 0 && ((end - base) & 3) == 0) {
    const int64_t n4 = (end - base) >> 2;
    float4* p4 = (float4*)(e.p + base);
    const float4* g4 = (const float4*)(e.g + base);
    float4* s4 = (float4*)(e.s1 + base);
#pragma unroll 4
    for (int64_t j = threadIdx.x; j < n4; j += blockDim.x) {
      float gv[4], pv[4], bv[4];
      *(float4*)gv = g4[j];
      *(float4*)pv = p4[j];
      const bool mom = h.momentum != 0.f;
      if (mom && !h.first) *(float4*)bv = s4[j];
#pragma unroll
      for (int u = 0; u < 4; ++u) sgd_elem(lars_dir(gv[u], pv[u], trust, gs, wd), pv[u], bv[u], h);
      if (mom) s4[j] = *(float4*)bv;
      p4[j] = *(float4*)pv;
      if (e.shadow) {
        bf16x4 sv;
#pragma unroll
        for (int u = 0; u < 4; ++u) sv[u] = f2bf(pv[u]);
        *(bf16x4*)(e.shadow + base + 4 * j) = sv;
      }
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    float p = e.p[i];
    float b = (h.momentum != 0.f && !h.first) ? e.s1[i] : 0.f;
    sgd_elem(lars_dir(e.g[i], p, trust, gs, wd), p, b, h);
    if (h.momentum != 0.f) e.s1[i] = b;
    e.p[i] = p;
    if (e.shadow) e.shadow[i] = f2bf(p);
  }
}


__global__ void __launch_bounds__(256) mt_adam_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                      AdamHyper h) {
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  float bc1 = h.bc1, bc2 = h.bc2;
  if (h.step_dev) {  // 1 - beta^t without the cancellation of 1 - powf
    const float t = (float)*h.step_dev;
    bc1 = -expm1f(t * h.lb1);
    bc2 = -expm1f(t * h.lb2);
  }
  const float rbc2 = 1.f / sqrtf(bc2);
  const float lr = h.lr_dev ? *h.lr_dev : h.lr;  // the device scalar: a replayed graph follows a schedule
  if (clip_skip(h.clip)) return;
  const float gs = clip_scale(h.grad_scale, h.clip);
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    float g = e.g[i] * gs;
    float p = e.p[i];
    if (h.wd != 0.f) {
      if (h.decoupled)
        p *= 1.f - lr * h.wd;
      else
        g += h.wd * p;
    }
    const float m = h.beta1 * e.s1[i] + h.omb1 * g;
    const float v = h.beta2 * e.s2[i] + h.omb2 * g * g;
    e.s1[i] = m;
    e.s2[i] = v;
    const float denom = sqrtf(v) * rbc2 + h.eps;
    p -= (lr / bc1) * m / denom;
    e.p[i] = p;
    if (e.shadow) e.shadow[i] = f2bf(p);
  }
}

// ---------------------------------------------------------------------------
// LAMB (You et al. 2020): Adam's moments, a layer-wise trust ratio in front of the update.
//   g~ = grad_scale g;  m = b1 m + (1 - b1) g~;  v = b2 v + (1 - b2) g~^2
//   r = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps);  u = r + wd w
//   trust = |w| / |u|  (1 when not adaptive or a norm is 0);  w -= lr trust u
// Adaptive: mt_lamb_moments (m, v, per-chunk (sum w^2, sum u^2)), lamb_trust, mt_lamb_update, which
// recomputes u from w and the new m, v (40 B / element; u is never stored).  Not adaptive: the moments
// kernel applies the update itself.  Both kernels form u with lamb_u, so the norm is taken over exactly
// the u that is applied; no float atomics, every reduction in a fixed order.
// ---------------------------------------------------------------------------

// Bias corrections of this launch: (bc1, 1 / sqrt(bc2)); from the device step count when there is one.
__device__ __forceinline__ void lamb_bias(const LambHyper& h, float& bc1, float& rbc2) {
  float bc2 = h.bc2;
  bc1 = h.bc1;
  if (h.bias_correction && h.step_dev) {
    const float t = (float)*h.step_dev;
    bc1 = -expm1f(t * h.lb1);
    bc2 = -expm1f(t * h.lb2);
  }
  rbc2 = 1.f / sqrtf(bc2);
}

// One element's moments and its u.  Every operation is named (no bare a * b + c for the compiler to
// contract one way in the 16-byte loop and another in the 4-byte loop): both loops, and both
// kernels, round alike.
__device__ __forceinline__ void lamb_moments(float gin, float gs, float& m, float& v, const LambHyper& h) {
  const float g = __fmul_rn(gin, gs);
  m = fmaf(h.beta1, m, __fmul_rn(h.omb1, g));
  v = fmaf(h.beta2, v, __fmul_rn(h.omb2, __fmul_rn(g, g)));
}

__device__ __forceinline__ float lamb_u(float m, float v, float p, float bc1, float rbc2, const LambHyper& h) {
  const float denom = fmaf(__fsqrt_rn(v), rbc2, h.eps);
  const float r = __fdiv_rn(__fdiv_rn(m, bc1), denom);
  return h.wd != 0.f ? fmaf(h.wd, p, r) : r;
}

// One workgroup per chunk, thread-to-element ownership and accumulation order of mt_norm2_kernel:
// thread t owns the chunk elements 4 (t + 256 k) + u.  APPLY (non-adaptive group): w = fma(-lr, u, w)
// here, no partials.  Otherwise partials[blockIdx.x] = (sum w^2, sum u^2), w untouched.
template <bool APPLY>
__global__ void __launch_bounds__(256) mt_lamb_moments_kernel(const MTEntry* __restrict__ tab,
                                                              const int2* __restrict__ chunks,
                                                              float2* __restrict__ partials, LambHyper h) {
  __shared__ float red[2][16];
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int len = (int)(min(e.n, base + kChunk) - base);
  float* p = e.p + base;
  const float* g = e.g + base;
  float* m = e.s1 + base;
  float* v = e.s2 + base;
  bf16* shadow = (APPLY && e.shadow) ? e.shadow + base : nullptr;
  if (clip_skip(h.clip)) return;  // whole workgroups: no barrier is left waiting
  const float gs = clip_scale(h.grad_scale, h.clip);
  float bc1, rbc2;
  lamb_bias(h, bc1, rbc2);
  const float nlr = APPLY ? -(h.lr_dev ? *h.lr_dev : h.lr) : 0.f;
  float sw = 0.f, su = 0.f;
  const uintptr_t mis = ((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u;
  const uintptr_t smis = shadow ? ((uintptr_t)shadow & 7u) : 0;
  if (mis == 0 && smis == 0 && (len & 3) == 0) {
    const int n4 = len >> 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x + 256 * k;
      if (j < n4) {
        float pv[4], gv[4], mv[4], vv[4];
        *(float4*)pv = ((const float4*)p)[j];
        *(float4*)gv = ((const float4*)g)[j];
        *(float4*)mv = ((const float4*)m)[j];
        *(float4*)vv = ((const float4*)v)[j];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          lamb_moments(gv[u], gs, mv[u], vv[u], h);
          const float uu = lamb_u(mv[u], vv[u], pv[u], bc1, rbc2, h);
          if (APPLY) {
            pv[u] = fmaf(nlr, uu, pv[u]);
          } else {
            sw = fmaf(pv[u], pv[u], sw);
            su = fmaf(uu, uu, su);
          }
        }
        ((float4*)m)[j] = *(float4*)mv;
        ((float4*)v)[j] = *(float4*)vv;
        if (APPLY) {
          ((float4*)p)[j] = *(float4*)pv;
          if (shadow) {
            bf16x4 sv;
#pragma unroll
            for (int u = 0; u < 4; ++u) sv[u] = f2bf(pv[u]);
            *(bf16x4*)(shadow + 4 * j) = sv;
          }
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i0 = 4 * (threadIdx.x + 256 * k);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u;
        if (i < len) {
          float pv = p[i], mv = m[i], vv = v[i];
          lamb_moments(g[i], gs, mv, vv, h);
          const float uu = lamb_u(mv, vv, pv, bc1, rbc2, h);
          m[i] = mv;
          v[i] = vv;
          if (APPLY) {
            pv = fmaf(nlr, uu, pv);
            p[i] = pv;
            if (shadow) shadow[i] = f2bf(pv);
          } else {
            sw = fmaf(pv, pv, sw);
            su = fmaf(uu, uu, su);
          }
        }
      }
    }
  }
  if (!APPLY) {
    sw = block_sum(sw, red[0]);
    su = block_sum(su, red[1]);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(sw, su);
  }
}

// One workgroup per tensor: lars_trust_kernel's merge; |w| and |u| rounded to fp32 once each, the
// ratio formed in fp32.
__global__ void __launch_bounds__(256) lamb_trust_kernel(const int2* __restrict__ spans, const float2* __restrict__ partials,
                                                         float* __restrict__ trust, const ClipCtl* __restrict__ clip,
                                                         float phi_min, float phi_max) {
  __shared__ double sh[2][256];
  if (clip_skip(clip)) return;  // a skipped step left no partials: the last step's ratios stay
  merge_partials(spans[blockIdx.x], partials, sh);
  if (threadIdx.x == 0) {
    const float wn = (float)sqrt(sh[0][0]);
    const float un = (float)sqrt(sh[1][0]);
    // the paper's phi: |w| clamped to [phi_min, phi_max] (0 and +inf leave every positive |w| as it is)
    trust[blockIdx.x] = (wn > 0.f && un > 0.f) ? __fdiv_rn(fminf(fmaxf(wn, phi_min), phi_max), un) : 1.f;
  }
}

// w = fma(-(lr trust), u, w), u recomputed from w and the moments mt_lamb_moments left; the learning
// rate from the device scalar when one is given.
__global__ void __launch_bounds__(256) mt_lamb_update_kernel(const MTEntry* __restrict__ tab,
                                                             const int2* __restrict__ chunks, LambHyper h) {
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  if (clip_skip(h.clip)) return;
  float bc1, rbc2;
  lamb_bias(h, bc1, rbc2);
  const float nlt =-__fmul_rn(h.lr_dev ? *h.lr_dev : h.lr, h.trust[ck.x]);
  const uintptr_t mis = ((uintptr_t)(e.p + base) | (uintptr_t)(e.s1 + base) | (uintptr_t)(e.s2 + base)) & 15u;
  const uintptr_t smis = e.shadow ? ((uintptr_t)(e.shadow + base) & 7u) : 0;
  if (mis == 0 && smis == 0 && ((end - base) & 3) == 0) {
    const int64_t n4 = (end - base) >> 2;
    float4* p4 = (float4*)(e.p + base);
    const float4* m4 = (const float4*)(e.s1 + base);
    const float4* v4 = (const float4*)(e.s2 + base);
#pragma unroll 4
    for (int64_t j = threadIdx.x; j < n4; j += blockDim.x) {
      float pv[4], mv[4], vv[4];
      *(float4*)pv = p4[j];
      *(float4*)mv = m4[j];
      *(float4*)vv = v4[j];
#pragma unroll
      for (int u = 0; u < 4; ++u) pv[u] = fmaf(nlt, lamb_u(mv[u], vv[u], pv[u], bc1, rbc2, h), pv[u]);
      p4[j] = *(float4*)pv;
      if (e.shadow) {
        bf16x4 sv;
#pragma unroll
        for (int u = 0; u < 4; ++u) sv[u] = f2bf(pv[u]);
        *(bf16x4*)(e.shadow + base + 4 * j) = sv;
      }
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    float p = e.p[i];
    p = fmaf(nlt, lamb_u(e.s1[i], e.s2[i], p, bc1, rbc2, h), p);
    e.p[i] = p;
    if (e.shadow) e.shadow[i] = f2bf(p);
  }
}

// ---------------------------------------------------------------------------
// CDR radix select.  state: [0] prefix bits, [1] prefix mask, [2] k remaining
// (1-based rank among elements matching the prefix), [3] threshold bits.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cdr_hist_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                       const uint32_t* __restrict__ state, int shift,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[256];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t prefix = state[0], pmask = state[1];
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const float v = fabsf(e.g[i] * e.p[i]);
    const uint32_t u = __float_as_uint(v);
    if ((u & pmask) == prefix) atomicAdd(&lh[(u >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

// single workgroup: walk bins from the top, find the bin holding the k-th largest
__global__ void cdr_select_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ hist, int shift) {
  if (threadIdx.x == 0) {
    uint32_t k = state[2];
    int b = 255;
    for (; b > 0; --b) {
      const uint32_t c = hist[b];
      if (c >= k) break;
      k -= c;
    }
    state[0] |= (uint32_t)b << shift;
    state[1] |= 255u << shift;
    state[2] = k;
    if (shift == 0) state[3] = state[0];
  }
  __syncthreads();
  hist[threadIdx.x] = 0;  // ready for the next pass (blockDim = 256)
}

__global__ void __launch_bounds__(256) cdr_mask_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                       const uint32_t* __restrict__ state, float clip) {
  const float thr = __uint_as_float(state[3]);
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const float g = e.g[i];
    const float v = fabsf(g * e.p[i]);
    e.g[i] = (v >= thr) ? g * clip : 0.f;
  }
}

// ---------------------------------------------------------------------------
// Multi-tensor scaled copy: dst_t[i] = src_t[i] * scale for every table entry (MTEntry.p = dst,
// MTEntry.g = src, raw pointers; SRC_BF16 / DST_BF16 pick the element types).  The gradient
// bucket engine (parallel/reducer.py) packs a bucket's parameter gradients into its flat
// all-reduce buffer with one launch (pre-divided by the world size; optionally rounded to bf16
// for a half-size all-reduce) and, for a bf16 bucket, unpacks the reduced values into the fp32
// gradient views in one launch.
template <bool SRC_BF16, bool DST_BF16>
__global__ void __launch_bounds__(256) mt_copy_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                      float scale) {
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  const void* src = (const void*)e.g;
  void* dst = (void*)e.p;
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const float v = (SRC_BF16 ? bf2f(((const bf16*)src)[i]) : ((const float*)src)[i]) * scale;
    if (DST_BF16)
      ((bf16*)dst)[i] = f2bf(v);
    else
      ((float*)dst)[i] = v;
  }
}

// ---------------------------------------------------------------------------
// Exponential moving average of the weights (optim/ema.py), over the same tables: MTEntry.p = the
// live tensor w (read only), MTEntry.s1 = its average e.  Per element, in fp32,
//   t  = w - e               (one rounding)
//   e' = fma(omd, t, e)      (one rounding)
// with omd ("one minus decay") read from a device scalar, so a replayed HIP graph follows a decay
// warm-up.  e == w is a fixed point bit for bit.  The 16-byte and the 4-byte loop call the same
// element function (the rule of sgd_elem): alignment never changes a bit.  With a clipping control
// block whose skip flag is set the kernel writes nothing: a step the optimizer skipped leaves the
// average (and the BN statistics a non-finite forward pass poisoned in the live model) alone.
// 12 B / element; the loads of a chunk's (up to) four 16-byte rounds are issued before its stores.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float ema_elem(float w, float e, float omd) { return fmaf(omd, __fsub_rn(w, e), e); }

__global__ void __launch_bounds__(256) mt_ema_kernel(const MTEntry* __restrict__ tab, const int2* __restrict__ chunks,
                                                     const float* __restrict__ omd_dev,
                                                     const ClipCtl* __restrict__ ctl) {
  if (clip_skip(ctl)) return;
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  const float omd = *omd_dev;
  const uintptr_t mis = ((uintptr_t)(e.p + base) | (uintptr_t)(e.s1 + base)) & 15u;
  if (mis == 0 && ((end - base) & 3) == 0) {  // uniform per chunk
    const int n4 = (int)((end - base) >> 2);  // <= kChunk / 4 = 4 rounds of 256 lanes
    const float4* __restrict__ w4 = (const float4*)(e.p + base);
    float4* __restrict__ a4 = (float4*)(e.s1 + base);
    float wv[4][4], av[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = threadIdx.x + r * 256;
      if (j < n4) {
        *(float4*)wv[r] = w4[j];
        *(float4*)av[r] = a4[j];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = threadIdx.x + r * 256;
      if (j < n4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) av[r][u] = ema_elem(wv[r][u], av[r][u], omd);
        a4[j] = *(float4*)av[r];
      }
    }
    return;
  }
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) e.s1[i] = ema_elem(e.p[i], e.s1[i], omd);
}

// In-place exchange of w (MTEntry.p) and e (MTEntry.s1): two loads and two stores per element, pure
// copies of the bit patterns (integer lanes: no NaN payload, signed zero or denormal is touched).
// Evaluation on the averaged weights swaps, evaluates, swaps back: no address changes, so a captured
// graph, the optimizer's tables and the bucket views stay valid.  16 B / element.
__global__ void __launch_bounds__(256) mt_swap_kernel(const MTEntry* __restrict__ tab,
                                                      const int2* __restrict__ chunks) {
  const int2 ck = chunks[blockIdx.x];
  const MTEntry e = tab[ck.x];
  const int64_t base = (int64_t)ck.y * kChunk;
  const int64_t end = min(e.n, base + kChunk);
  const uintptr_t mis = ((uintptr_t)(e.p + base) | (uintptr_t)(e.s1 + base)) & 15u;
  if (mis == 0 && ((end - base) & 3) == 0) {  // uniform per chunk
    const int n4 = (int)((end - base) >> 2);
    uint4* __restrict__ w4 = (uint4*)(e.p + base);
    uint4* __restrict__ a4 = (uint4*)(e.s1 + base);
    // Values are named and unconditionally written, never conditionally filled arrays (those left
    // the registers for LDS and scratch).  A whole chunk, the common case, is straight-line code: its
    // eight 16-byte loads are issued before the first store.  A tensor's last chunk takes the loop.
    if (n4 == kChunk / 4) {
      const int j = threadIdx.x;
      const uint4 x0 = w4[j], x1 = w4[j + 256], x2 = w4[j + 512], x3 = w4[j + 768];
      const uint4 y0 = a4[j], y1 = a4[j + 256], y2 = a4[j + 512], y3 = a4[j + 768];
      w4[j] = y0;
      w4[j + 256] = y1;
      w4[j + 512] = y2;
      w4[j + 768] = y3;
      a4[j] = x0;
      a4[j + 256] = x1;
      a4[j + 512] = x2;
      a4[j + 768] = x3;
      return;
    }
#pragma unroll 4
    for (int j = threadIdx.x; j < n4; j += 256) {
      const uint4 x = w4[j];
      const uint4 y = a4[j];
      w4[j] = y;
      a4[j] = x;
    }
    return;
  }
  uint32_t* w = (uint32_t*)e.p;
  uint32_t* a = (uint32_t*)e.s1;
  for (int64_t i = base + threadIdx.x; i < end; i += blockDim.x) {
    const uint32_t x = w[i], y = a[i];
    w[i] = y;
    a[i] = x;
  }
}

void launch_mt_ema(const MTEntry* tab, const int2* chunks, int nchunks, const float* omd_dev, const ClipCtl* ctl,
                   hipStream_t s) {
  if (nchunks) hipLaunchKernelGGL(mt_ema_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, omd_dev, ctl);
}
void launch_mt_swap(const MTEntry* tab, const int2* chunks, int nchunks, hipStream_t s) {
  if (nchunks) hipLaunchKernelGGL(mt_swap_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks);
}

void launch_mt_copy(const MTEntry* tab, const int2* chunks, int nchunks, float scale, int mode, hipStream_t s) {
  if (!nchunks) return;
  switch (mode & 3) {
    case 0: hipLaunchKernelGGL((mt_copy_kernel<false, false>), dim3(nchunks), dim3(256), 0, s, tab, chunks, scale); break;
    case 1: hipLaunchKernelGGL((mt_copy_kernel<true, false>), dim3(nchunks), dim3(256), 0, s, tab, chunks, scale); break;
    case 2: hipLaunchKernelGGL((mt_copy_kernel<false, true>), dim3(nchunks), dim3(256), 0, s, tab, chunks, scale); break;
    default: hipLaunchKernelGGL((mt_copy_kernel<true, true>), dim3(nchunks), dim3(256), 0, s, tab, chunks, scale); break;
  }
}

void launch_mt_sgd(const MTEntry* tab, const int2* chunks, int nchunks, SgdHyper h, hipStream_t s) {
  if (nchunks) hipLaunchKernelGGL(mt_sgd_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, h);
}
void launch_mt_lars(const MTEntry* tab, const int2* chunks, int nchunks, const int2* spans, int ntensors,
                    float2* partials, float* trust, float eta, float eps, LarsHyper h, hipStream_t s) {
  if (!nchunks) return;
  if (trust) {  // adaptive: the update reads the trust ratios this step's norms give
    hipLaunchKernelGGL(mt_norm2_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, partials);
    hipLaunchKernelGGL(lars_trust_kernel, dim3(ntensors), dim3(256), 0, s, spans, partials, h.sgd.grad_scale,
                       h.sgd.wd, eta, eps, trust, h);
  }
  h.trust = trust;
  hipLaunchKernelGGL(mt_lars_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, h);
}
void launch_mt_adam(const MTEntry* tab, const int2* chunks, int nchunks, AdamHyper h, hipStream_t s) {
  if (nchunks) hipLaunchKernelGGL(mt_adam_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, h);
}
void launch_mt_lamb(const MTEntry* tab, const int2* chunks, int nchunks, const int2* spans, int ntensors,
                    float2* partials, float* trust, LambHyper h, hipStream_t s) {
  if (!nchunks) return;
  h.trust = trust;
  if (!trust) {  // not adaptive: one launch, every ratio 1
    hipLaunchKernelGGL((mt_lamb_moments_kernel<true>), dim3(nchunks), dim3(256), 0, s, tab, chunks, partials, h);
    return;
  }
  hipLaunchKernelGGL((mt_lamb_moments_kernel<false>), dim3(nchunks), dim3(256), 0, s, tab, chunks, partials, h);
  hipLaunchKernelGGL(lamb_trust_kernel, dim3(ntensors), dim3(256), 0, s, spans, partials, trust, h.clip, h.phi_min,
                     h.phi_max);
  hipLaunchKernelGGL(mt_lamb_update_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, h);
}
void launch_mt_gnorm2(const MTEntry* tab, const int2* chunks, int nchunks, const int* slots, const ClipCtl* ctl,
                      GnormPartial* partials, hipStream_t s) {
  if (nchunks) hipLaunchKernelGGL(mt_gnorm2_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, slots, ctl, partials);
}
void launch_gnorm_finish(const GnormPartial* partials, int nslots, const float* slot_gs, float max_norm,
                         int skip_nonfinite, ClipCtl* ctl, hipStream_t s) {
  hipLaunchKernelGGL(gnorm_finish_kernel, dim3(1), dim3(256), 0, s, partials, nslots, slot_gs, max_norm, skip_nonfinite,
                     ctl);
}
void launch_cdr_threshold(const MTEntry* tab, const int2* chunks, int nchunks, uint32_t* state, uint32_t* hist,
                          hipStream_t s) {
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(cdr_hist_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, state, shift, hist);
    hipLaunchKernelGGL(cdr_select_kernel, dim3(1), dim3(256), 0, s, state, hist, shift);
  }
}
void launch_cdr_mask(const MTEntry* tab, const int2* chunks, int nchunks, const uint32_t* state, float clip,
                     hipStream_t s) {
  if (nchunks) hipLaunchKernelGGL(cdr_mask_kernel, dim3(nchunks), dim3(256), 0, s, tab, chunks, state, clip);
}

}  // namespace dcp

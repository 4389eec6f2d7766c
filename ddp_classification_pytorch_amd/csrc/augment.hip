// On-device augmentation for the native shard loader (csrc/host/loader.cpp, data/shards.py).
//
// crop_resize: for every image b of a gathered batch of raw uint8 HWC records (variable size,
// record b at meta[b][0] bytes into `src`), resample the crop box (y0, x0, h, w) to Ho x Wo with
// bilinear interpolation (half-pixel centres, edge clamp: F.interpolate(mode="bilinear",
// align_corners=False) on the crop) and optionally mirror it horizontally.  This is the tensor
// half of torchvision's RandomResizedCrop + RandomHorizontalFlip / Resize + CenterCrop
// (BASELINE/main.py:58-76, CDR/main.py:112-130, NESTED/train.py:40-65); the host thread pool only
// samples the boxes and gathers bytes.  The uint8 output feeds the to_nhwc / to_nhwc_s2d
// normalisation kernels (misc.hip).
//
// One thread per output pixel; the 4 source taps x 3 channels are byte loads from L2-resident
// records (a 256x256 record is 192 KB), the output is written as 3 bytes per lane (contiguous per
// wave).  The pass moves ~150 KB per 224x224 image: a few microseconds per 1k-image batch.
#include <cstdint>
#include <cstdio>

#include "common.cuh"
#include "launchers.h"

namespace dcp {

__global__ void __launch_bounds__(256) crop_resize_kernel(const uint8_t* __restrict__ src,
                                                          const int64_t* __restrict__ meta, int B, int Ho, int Wo,
                                                          uint8_t* __restrict__ out) {
  const uint32_t per = (uint32_t)Ho * Wo;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= per * (uint32_t)B) return;
  const uint32_t b = p / per, r = p - b * per;
  const int oy = r / Wo, ox0 = r - oy * Wo;
  const int64_t* m = meta + (size_t)b * 8;
  const uint8_t* img = src + m[0];
  const int W = (int)m[2];
  const int cy = (int)m[3], cx = (int)m[4], ch = (int)m[5], cw = (int)m[6];
  const int ox = m[7] ? Wo - 1 - ox0 : ox0;
  // F.interpolate(bilinear, align_corners=False): src = (dst + 0.5) * in/out - 0.5, clamped at 0
  float sy = fmaxf(((float)oy + 0.5f) * ((float)ch / (float)Ho) - 0.5f, 0.f);
  float sx = fmaxf(((float)ox + 0.5f) * ((float)cw / (float)Wo) - 0.5f, 0.f);
  int y0 = min((int)sy, ch - 1), x0 = min((int)sx, cw - 1);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const int y1 = min(y0 + 1, ch - 1), x1 = min(x0 + 1, cw - 1);
  const uint8_t* r0 = img + ((size_t)(cy + y0) * W + cx) * 3;
  const uint8_t* r1 = img + ((size_t)(cy + y1) * W + cx) * 3;
  uint8_t* o = out + (size_t)p * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = (float)r0[x0 * 3 + c], bb = (float)r0[x1 * 3 + c];
    const float cc = (float)r1[x0 * 3 + c], d = (float)r1[x1 * 3 + c];
    const float top = a + (bb - a) * lx, bot = cc + (d - cc) * lx;
    const float v = top + (bot - top) * ly;
    o[c] = (uint8_t)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
  }
}

void launch_crop_resize(const uint8_t* src, const int64_t* meta, int B, int Ho, int Wo, uint8_t* out,
                        hipStream_t s) {
  const size_t total = (size_t)B * Ho * Wo;
  if (total == 0) return;
  if (total >= (1ull << 32)) {
    fprintf(stderr, "crop_resize: %zu output pixels exceed the 32-bit index range\n", total);
    abort();
  }
  hipLaunchKernelGGL(crop_resize_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, meta, B, Ho, Wo,
                     out);
}

// warp_crop: inverse-affine resample of the crop box with a zero border -- the tensor half of the
// presets that rotate or pad (CDR/main.py:112-130 RandomResizedCrop -> RandomRotation(15) -> flip ->
// CenterCrop; NESTED/train.py:40-45 RandomCrop(32, padding=4) -> flip; PLC/FolderDataset.py
// Resize((256, 256)) -> flip -> CenterCrop).  The host composes each chain into one 2x3 matrix per
// image (csrc/host/loader.cpp:affine_matrix; the flip is part of the matrix, meta[7] is not read):
//   sx = m00*ox + m01*oy + m02,  sy = m10*ox + m11*oy + m12     (box-relative, pixel k centred at k)
// A sample inside the box, -0.5 <= sx < w-0.5 and -0.5 <= sy < h-0.5, is bilinear at the position
// clamped to [0, w-1] x [0, h-1] with taps clamped to the box and rounded half up like
// crop_resize_kernel; everything else, a NaN coordinate included (it compares false), is PIL's
// fill 0.  Taps never leave the box and the binding checks the box against its record, so no
// matrix can address outside a record.  Same launch shape as crop_resize_kernel.
__global__ void __launch_bounds__(256) warp_crop_kernel(const uint8_t* __restrict__ src,
                                                        const int64_t* __restrict__ meta,
                                                        const float* __restrict__ xf, int B, int Ho, int Wo,
                                                        uint8_t* __restrict__ out) {
  const uint32_t per = (uint32_t)Ho * Wo;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= per * (uint32_t)B) return;
  const uint32_t b = p / per, r = p - b * per;
  const int oy = r / Wo, ox = r - oy * Wo;
  const int64_t* m = meta + (size_t)b * 8;
  const float* t = xf + (size_t)b * 8;
  const int ch = (int)m[5], cw = (int)m[6];
  float sx = t[0] * (float)ox + t[1] * (float)oy + t[2];
  float sy = t[3] * (float)ox + t[4] * (float)oy + t[5];
  uint8_t* o = out + (size_t)p * 3;
  const bool inside = sx >= -0.5f && sx < (float)cw - 0.5f && sy >= -0.5f && sy < (float)ch - 0.5f;
  if (!inside) {
    o[0] = 0, o[1] = 0, o[2] = 0;
    return;
  }
  const uint8_t* img = src + m[0];
  const int W = (int)m[2];
  const int cy = (int)m[3], cx = (int)m[4];
  sx = fminf(fmaxf(sx, 0.f), (float)(cw - 1));
  sy = fminf(fmaxf(sy, 0.f), (float)(ch - 1));
  const int y0 = min((int)sy, ch - 1), x0 = min((int)sx, cw - 1);
  const float ly = sy - (float)y0, lx = sx - (float)x0;
  const int y1 = min(y0 + 1, ch - 1), x1 = min(x0 + 1, cw - 1);
  const uint8_t* r0 = img + ((size_t)(cy + y0) * W + cx) * 3;
  const uint8_t* r1 = img + ((size_t)(cy + y1) * W + cx) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float a = (float)r0[x0 * 3 + c], bb = (float)r0[x1 * 3 + c];
    const float cc = (float)r1[x0 * 3 + c], d = (float)r1[x1 * 3 + c];
    const float top = a + (bb - a) * lx, bot = cc + (d - cc) * lx;
    const float v = top + (bot - top) * ly;
    o[c] = (uint8_t)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
  }
}

void launch_warp_crop(const uint8_t* src, const int64_t* meta, const float* xf, int B, int Ho, int Wo, uint8_t* out,
                      hipStream_t s) {
  const size_t total = (size_t)B * Ho * Wo;
  if (total == 0) return;
  if (total >= (1ull << 32)) {
    fprintf(stderr, "warp_crop: %zu output pixels exceed the 32-bit index range\n", total);
    abort();
  }
  hipLaunchKernelGGL(warp_crop_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, meta, xf, B, Ho,
                     Wo, out);
}

// ---------------------------------------------------------------------------------------------
// PIL-exact resampling (the loader's `pil` mode).  Pillow's Image.resize is fixed point: per axis
// it builds, in double, a normalised filter bank whose width grows with the downscale (the
// antialiasing crop_resize_kernel lacks), rounds it to 22-bit integers, and runs a horizontal and
// then a vertical integer pass with a uint8 image between them.  Image.rotate(NEAREST) is a 16.16
// integer map.  Both are reproduced bit for bit, so the tests are torch.equal against Pillow.
//
// The banks are computed here, on the device, in fp64 with contraction switched off: every
// operation is then the one IEEE operation the host would do (divide and multiply are correctly
// rounded; a fused multiply-add would move a coefficient by one).  The alternative, banks from
// the host thread pool, costs up to (Sw + Sh) * 33 * 4 bytes per image in every pinned slot -- 277 MB
// per slot at batch 4096 if sized for the 8x case -- and host time per batch; the device recomputes
// a tile's few hundred coefficients in well under a microsecond.
//
// geo rows, int32 [B][12]: {Sh, Sw, dy, dx, a0, a1, a2, a3, a4, a5, rotate, angle float32 bits}.
constexpr int RS_KMAX = 33;    // taps of a bicubic 8x downscale: ceil(2 * 8) * 2 + 1
constexpr int RS_TH = 16;      // output rows per workgroup
constexpr int RS_TW = 128;     // output columns per workgroup
constexpr int RS_ROWCAP = 35;  // staged source rows (>= RS_KMAX, so one output row always fits)
constexpr int RS_MAX_CANVAS = 4096;
constexpr int RS_MAX_SCALE = 8;

__device__ __forceinline__ double pil_filter(double t, int bicubic) {
#pragma clang fp contract(off)
  if (t < 0.0) t = -t;
  if (!bicubic) return t < 1.0 ? 1.0 - t : 0.0;
  const double a = -0.5;
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
  return 0.0;
}

// The integer filter bank of output index `xx` of one axis (in_size -> out_size): first tap and
// tap count, coefficients to K[0 .. count).  count <= RS_KMAX whenever in_size <= 8 * out_size (the
// launcher refuses anything else); the clamp only keeps a caller's mistake inside K.
__device__ __forceinline__ void pil_bank(int in_size, int out_size, int xx, int bicubic, int* __restrict__ K,
                                         int* __restrict__ first, int* __restrict__ count) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = (bicubic ? 2.0 : 1.0) * fs;
  const double ss = 1.0 / fs;
  const double center = ((double)xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  const int n = min(max(xmax - xmin, 0), RS_KMAX);
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += pil_filter(((double)(x + xmin) - center + 0.5) * ss, bicubic);
  for (int x = 0; x < n; ++x) {
    double k = pil_filter(((double)(x + xmin) - center + 0.5) * ss, bicubic);
    if (ww != 0.0) k = k / ww;
    const double v = k * 4194304.0;
    K[x] = k < 0.0 ? (int)(v - 0.5) : (int)(v + 0.5);
  }
  *first = xmin;
  *count = n;
}

__device__ __forceinline__ uint8_t pil_clip8(int acc) { return (uint8_t)min(max(acc >> 22, 0), 255); }

// One workgroup per (image, RS_TH x RS_TW tile of the output window).  Lanes 0..Wt-1 build the
// horizontal banks of the tile's canvas columns, lanes 128..143 the vertical banks of its canvas
// rows; then, for as many output rows at a time as their source rows fit RS_ROWCAP, the source rows
// are resampled horizontally into LDS as uint8 (Pillow's intermediate image) and the vertical pass
// runs from there.  Only the canvas rows and columns the window shows are computed; a window
// pixel off the canvas is 0 (Image.crop).  `whole` writes the canvas itself: offset 0, no mirror.
__global__ void __launch_bounds__(256) resample_crop_kernel(const uint8_t* __restrict__ src,
                                                            const int64_t* __restrict__ meta,
                                                            const int32_t* __restrict__ geo, int Ho, int Wo,
                                                            int tiles_x, int tiles_y, int bicubic, int whole,
                                                            uint8_t* __restrict__ out) {
  __shared__ int hK[RS_TW * RS_KMAX];
  __shared__ int vK[RS_TH * RS_KMAX];
  __shared__ int hmin[RS_TW], hcnt[RS_TW], vmin[RS_TH], vcnt[RS_TH];
  __shared__ uint8_t rows[RS_ROWCAP * RS_TW * 3];
  const int t = threadIdx.x;
  const int per = tiles_x * tiles_y;
  const int b = blockIdx.x / per, tile = blockIdx.x - b * per;
  const int oy0 = (tile / tiles_x) * RS_TH, ox0 = (tile % tiles_x) * RS_TW;
  const int Ht = min(RS_TH, Ho - oy0), Wt = min(RS_TW, Wo - ox0);
  const int64_t* m = meta + (size_t)b * 8;
  const int32_t* g = geo + (size_t)b * 12;
  const uint8_t* img = src + m[0];
  const int W = (int)m[2], y0 = (int)m[3], x0 = (int)m[4], h = (int)m[5], w = (int)m[6];
  const int Sh = g[0], Sw = g[1], dy = whole ? 0 : g[2], dx = whole ? 0 : g[3];
  const bool flip = !whole && m[7] != 0;

  if (t < Wt) {
    const int ox = ox0 + t;
    const int X = flip ? Sw - 1 - dx - ox : dx + ox;  // mirrored first, then the window
    hmin[t] = 0, hcnt[t] = 0;
    if (X >= 0 && X < Sw) pil_bank(w, Sw, X, bicubic, hK + t * RS_KMAX, &hmin[t], &hcnt[t]);
  } else if (t >= RS_TW && t < RS_TW + RS_TH) {
    const int r = t - RS_TW, Y = dy + oy0 + r;
    vmin[r] = 0, vcnt[r] = 0;
    if (r < Ht && Y >= 0 && Y < Sh) pil_bank(h, Sh, Y, bicubic, vK + r * RS_KMAX, &vmin[r], &vcnt[r]);
  }
  __syncthreads();

  for (int r0 = 0; r0 < Ht;) {
    // the longest run of output rows from r0 whose source rows [lo, hi) fit the staging buffer
    int lo = 0x7fffffff, hi = 0, n = 0;
    for (int q = r0; q < Ht; ++q, ++n) {
      if (vcnt[q] == 0) continue;
      const int nlo = min(lo, vmin[q]), nhi = max(hi, vmin[q] + vcnt[q]);
      if (nhi - nlo > RS_ROWCAP) break;
      lo = nlo, hi = nhi;
    }
    const int nr = max(hi - lo, 0);
    for (int i = t; i < nr * Wt; i += 256) {  // horizontal pass: source row lo + rr, tile column c
      const int rr = i / Wt, c = i - rr * Wt;
      const int cnt = hcnt[c];
      if (cnt == 0) continue;
      const uint8_t* p = img + ((size_t)(y0 + lo + rr) * W + x0 + hmin[c]) * 3;
      const int* kk = hK + c * RS_KMAX;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int k = 0; k < cnt; ++k) {
        const int kv = kk[k];
        a0 += (int)p[k * 3] * kv, a1 += (int)p[k * 3 + 1] * kv, a2 += (int)p[k * 3 + 2] * kv;
      }
      uint8_t* d = rows + (size_t)i * 3;
      d[0] = pil_clip8(a0), d[1] = pil_clip8(a1), d[2] = pil_clip8(a2);
    }
    __syncthreads();
    for (int i = t; i < n * Wt; i += 256) {  // vertical pass: output row r0 + q, tile column c
      const int q = i / Wt, c = i - q * Wt, r = r0 + q;
      uint8_t* o = out + (((size_t)b * Ho + oy0 + r) * Wo + ox0 + c) * 3;
      const int cnt = hcnt[c] ? vcnt[r] : 0;
      if (cnt == 0) {
        o[0] = 0, o[1] = 0, o[2] = 0;
        continue;
      }
      const uint8_t* p = rows + ((size_t)(vmin[r] - lo) * Wt + c) * 3;
      const int* kk = vK + r * RS_KMAX;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int k = 0; k < cnt; ++k) {
        const int kv = kk[k];
        const uint8_t* pk = p + (size_t)k * Wt * 3;
        a0 += (int)pk[0] * kv, a1 += (int)pk[1] * kv, a2 += (int)pk[2] * kv;
      }
      o[0] = pil_clip8(a0), o[1] = pil_clip8(a1), o[2] = pil_clip8(a2);
    }
    __syncthreads();
    r0 += n;
  }
}

// Image.rotate(theta, NEAREST) -> mirror -> window of uniform Sh x Sw canvases [B][Sh][Sw][3]: one
// thread per output pixel.  Window pixel (ox, oy) is pixel (X, Y) of the mirrored rotated canvas,
// which reads canvas ((a2 + a1*Y + a0*X) >> 16, (a5 + a4*Y + a3*X) >> 16), 0 when that (or (X, Y)
// itself) is off the canvas.  Canvases are at most 4096 px, so the 16.16 sums stay below 2^31.
__global__ void __launch_bounds__(256) rotate_nearest_crop_kernel(const uint8_t* __restrict__ canvas,
                                                                  const int64_t* __restrict__ meta,
                                                                  const int32_t* __restrict__ geo, int B, int Sh,
                                                                  int Sw, int Ho, int Wo, uint8_t* __restrict__ out) {
  const uint32_t per = (uint32_t)Ho * Wo;
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= per * (uint32_t)B) return;
  const uint32_t b = p / per, r = p - b * per;
  const int oy = r / Wo, ox = r - oy * Wo;
  const int32_t* g = geo + (size_t)b * 12;
  const int Y = g[2] + oy;
  const int X = meta[(size_t)b * 8 + 7] ? Sw - 1 - g[3] - ox : g[3] + ox;
  uint8_t* o = out + (size_t)p * 3;
  o[0] = 0, o[1] = 0, o[2] = 0;
  if (X < 0 || X >= Sw || Y < 0 || Y >= Sh) return;
  const int xin = (g[6] + g[5] * Y + g[4] * X) >> 16;
  const int yin = (g[9] + g[8] * Y + g[7] * X) >> 16;
  if (xin < 0 || xin >= Sw || yin < 0 || yin >= Sh) return;
  const uint8_t* c = canvas + (((size_t)b * Sh + yin) * Sw + xin) * 3;
  o[0] = c[0], o[1] = c[1], o[2] = c[2];
}

// Host-side refusal of what the kernels do not cover, from the HOST copies of meta and geo (the
// boxes themselves are checked against their records by the binding).  0 = fine, else a code and
// the offending image in *bad: 1 canvas outside 1..4096, 2 a downscale above 8x (the filter would
// need more than RS_KMAX taps; it is never truncated), 3 `whole` with a canvas that is not the
// output, 4 window entirely off the canvas, 5 output size.
static int resample_check(const int64_t* hmeta, const int32_t* hgeo, int B, int Ho, int Wo, int whole, int* bad) {
  if (Ho <= 0 || Wo <= 0 || Ho > 8192 || Wo > 8192 || (size_t)B * Ho * Wo >= (1ull << 31) / 3) return 5;
  for (int b = 0; b < B; ++b) {
    const int64_t h = hmeta[(size_t)b * 8 + 5], w = hmeta[(size_t)b * 8 + 6];
    const int32_t* g = hgeo + (size_t)b * 12;
    const int64_t Sh = g[0], Sw = g[1], dy = g[2], dx = g[3];
    int rc = 0;
    if (Sh <= 0 || Sw <= 0 || Sh > RS_MAX_CANVAS || Sw > RS_MAX_CANVAS) rc = 1;
    else if (h > RS_MAX_SCALE * Sh || w > RS_MAX_SCALE * Sw) rc = 2;
    else if (whole ? (Sh != Ho || Sw != Wo) : false) rc = 3;
    else if (!whole && (dy >= Sh || dx >= Sw || dy + Ho <= 0 || dx + Wo <= 0)) rc = 4;
    if (rc) {
      if (bad) *bad = b;
      return rc;
    }
  }
  return 0;
}

int launch_resample_crop(const uint8_t* src, const int64_t* meta, const int32_t* geo, const int64_t* hmeta,
                         const int32_t* hgeo, int B, int Ho, int Wo, int bicubic, int whole, uint8_t* out, int* bad,
                         hipStream_t s) {
  const int rc = resample_check(hmeta, hgeo, B, Ho, Wo, whole, bad);
  if (rc || B == 0) return rc;
  const int tx = (Wo + RS_TW - 1) / RS_TW, ty = (Ho + RS_TH - 1) / RS_TH;
  hipLaunchKernelGGL(resample_crop_kernel, dim3((unsigned)((size_t)B * tx * ty)), dim3(256), 0, s, src, meta, geo, Ho,
                     Wo, tx, ty, bicubic, whole, out);
  return 0;
}

int launch_rotate_nearest_crop(const uint8_t* canvas, const int64_t* meta, const int32_t* geo, const int32_t* hgeo,
                               int B, int Sh, int Sw, int Ho, int Wo, uint8_t* out, int* bad, hipStream_t s) {
  if (Ho <= 0 || Wo <= 0 || Ho > 8192 || Wo > 8192 || (size_t)B * Ho * Wo >= (1ull << 31) / 3) return 5;
  if (Sh <= 0 || Sw <= 0 || Sh > RS_MAX_CANVAS || Sw > RS_MAX_CANVAS) return 1;
  for (int b = 0; b < B; ++b) {
    const int32_t* g = hgeo + (size_t)b * 12;
    int rc = 0;
    if (g[0] != Sh || g[1] != Sw) rc = 3;
    else if (g[2] >= Sh || g[3] >= Sw || (int64_t)g[2] + Ho <= 0 || (int64_t)g[3] + Wo <= 0) rc = 4;
    if (rc) {
      if (bad) *bad = b;
      return rc;
    }
  }
  if (B == 0) return 0;
  const size_t total = (size_t)B * Ho * Wo;
  hipLaunchKernelGGL(rotate_nearest_crop_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, canvas, meta,
                     geo, B, Sh, Sw, Ho, Wo, out);
  return 0;
}

}  // namespace dcp

// RandAugment on the device (data/randaug.py is the definition: 14 ops written as Pillow calls).
//
// rand_augment: uint8 [N][H][W][3] + plan int32 [N][K][8] = {op, parameter, a0..a5} -> uint8 [N][H][W][3],
// byte for byte what Pillow computes (the arithmetic is in randaug_math.cuh).
//
// One workgroup of 1024 threads per image, and the whole image in LDS (150,528 B at 224 x 224 of the
// CU's 160 KB), so a chain of K ops costs one global read and one global write as long as its ops
// can run in place:
//   * byte -> byte ops (Brightness, Contrast, Posterize, Solarize, AutoContrast, Equalize) build a
//     3 x 256 lookup table in LDS and map the image through it a dword at a time.  Their statistics
//     are integers: per-channel histograms by LDS atomics, the L mean of Contrast by an integer sum,
//     so the order of the atomics cannot show.  One wave per channel turns a histogram into its
//     table (4 bins per lane, shuffles for min / max / sum / prefix sum);
//   * Color is a per-pixel op, in place, 4 pixels (3 dwords) per thread;
//   * Sharpness (3 x 3 SMOOTH, borders copied, then the blend) and the five geometric ops (16.16
//     inverse map, nearest, zero fill) read neighbours or other pixels and cannot run in place.
//     Where two copies fit (2 x H W 3 <= RA_CAP) they write the second LDS buffer and the two swap;
//     else they write the output image in global memory and the workgroup stages it back in only
//     if another op follows.
// No float atomics, no scratch; dynamic LDS is sized per launch, so small images leave room for a
// second workgroup on the CU.
#include <hip/hip_runtime.h>

#include "launchers.h"
#include "randaug_math.cuh"

namespace dcp {
namespace {

constexpr int RA_THREADS = 1024;
// image bytes one LDS buffer holds: a multiple of 48, so that the last group of 4 pixels (12 B) and
// the last uint4 stay inside the buffer whatever H W 3 is
constexpr int RA_CAP = 155136;
constexpr int RA_AUX = 768 * 4 + 768 + 64;  // histograms, lookup table, the L sum

__device__ __forceinline__ int wave_min(int v) {
  for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ int byte_of(const uint32_t w[3], int j) { return (w[j >> 2] >> ((j & 3) * 8)) & 255; }

// flags: bit 0 = both images 16-byte aligned with H W 3 % 16 == 0 (uint4 staging), bit 1 = the output
// 4-byte aligned with H W 3 % 4 == 0 (dword stores of the out-of-place ops), bit 2 = two LDS copies
__global__ void __launch_bounds__(RA_THREADS) rand_augment_kernel(const uint8_t* __restrict__ in,
                                                                  const int* __restrict__ plan, int K, int H, int W,
                                                                  int buf, int flags, uint8_t* out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, P = H * W, n = P * 3;
  const bool vec16 = flags & 1, vec4 = flags & 2, two = flags & 4;
  uint8_t* cur = lds;
  uint8_t* alt = lds + buf;  // used only when `two`
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds + (two ? 2 : 1) * buf);
  uint8_t* lut = reinterpret_cast<uint8_t*>(hist + 768);
  uint32_t* lsum = reinterpret_cast<uint32_t*>(lut + 768);
  const size_t base = (size_t)blockIdx.x * n;
  const uint8_t* gin = in + base;
  uint8_t* gout = out + base;
  const int* rows = plan + (size_t)blockIdx.x * K * 8;
  const int nwords = (n + 3) >> 2, ngroups = (P + 3) >> 2;

  int last = -1;
  for (int k = 0; k < K; ++k)
    if (rows[k * 8] > ra::IDENTITY && rows[k * 8] < ra::NUM_OPS) last = k;
  if (last < 0) {  // nothing to do: global to global
    if (vec16) {
      for (int i = tid; i < (n >> 4); i += RA_THREADS)
        reinterpret_cast<uint4*>(gout)[i] = reinterpret_cast<const uint4*>(gin)[i];
    } else {
      for (int i = tid; i < n; i += RA_THREADS) gout[i] = gin[i];
    }
    return;
  }

  const uint8_t* gsrc = gin;  // where the current image is when it is not in LDS
  bool in_lds = false;
  for (int k = 0; k <= last; ++k) {
    const int op = rows[k * 8], p = rows[k * 8 + 1];
    if (op <= ra::IDENTITY || op >= ra::NUM_OPS) continue;
    if (!in_lds) {
      if (vec16) {
        for (int i = tid; i < (n >> 4); i += RA_THREADS)
          reinterpret_cast<uint4*>(cur)[i] = reinterpret_cast<const uint4*>(gsrc)[i];
      } else {
        for (int i = tid; i < n; i += RA_THREADS) cur[i] = gsrc[i];
      }
      in_lds = true;
      __syncthreads();
    }
    uint32_t* cur32 = reinterpret_cast<uint32_t*>(cur);

    if (op <= ra::ROTATE || op == ra::SHARPNESS) {
      // ---- out of place: 4 output pixels per thread and step
      int a[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) a[i] = rows[k * 8 + 2 + i];
      const float factor = __int_as_float(p);
      for (int g = tid; g < ngroups; g += RA_THREADS) {
        int y = (4 * g) / W, x = 4 * g - y * W;
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int v[3] = {0, 0, 0};
          if (op != ra::SHARPNESS) {
            const int s = ra::affine_src(a, x, y, H, W);
            if (s >= 0) {
#pragma unroll
              for (int c = 0; c < 3; ++c) v[c] = cur[s * 3 + c];
            }
          } else if (y < H) {
            const uint8_t* mid = cur + (y * W + x) * 3;
            const bool border = y == 0 || x == 0 || y == H - 1 || x == W - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int self = mid[c];
              int d = self;
              if (!border) {
                const uint8_t* up = mid - W * 3;
                const uint8_t* dn = mid + W * 3;
                const int u3[3] = {up[c - 3], up[c], up[c + 3]};
                const int m3[3] = {mid[c - 3], self, mid[c + 3]};
                const int d3[3] = {dn[c - 3], dn[c], dn[c + 3]};
                d = ra::smooth(u3, m3, d3);
              }
              v[c] = ra::blend(d, self, factor);
            }
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) w[(3 * i + c) >> 2] |= (uint32_t)v[c] << (((3 * i + c) & 3) * 8);
          if (++x == W) x = 0, ++y;
        }
        if (two) {
#pragma unroll
          for (int i = 0; i < 3; ++i) reinterpret_cast<uint32_t*>(alt)[3 * g + i] = w[i];
        } else if (vec4) {  // H W % 4 == 0: every group is whole
#pragma unroll
          for (int i = 0; i < 3; ++i) reinterpret_cast<uint32_t*>(gout)[3 * g + i] = w[i];
        } else {
#pragma unroll
          for (int j = 0; j < 12; ++j)
            if (12 * g + j < n) gout[12 * g + j] = (uint8_t)byte_of(w, j);
        }
      }
      __syncthreads();  // also orders this workgroup's global stores before its staging loads of them
      if (two) {
        uint8_t* t = cur;
        cur = alt;
        alt = t;
      } else {
        in_lds = false;
        gsrc = gout;
      }
      continue;
    }

    if (op == ra::COLOR) {
      // ---- per pixel, in place (the padding of the buffer takes the pixels past the last)
      const float factor = __int_as_float(p);
      for (int g = tid; g < ngroups; g += RA_THREADS) {
        const uint32_t w[3] = {cur32[3 * g], cur32[3 * g + 1], cur32[3 * g + 2]};
        uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = byte_of(w, 3 * i), gr = byte_of(w, 3 * i + 1), b = byte_of(w, 3 * i + 2);
          const int l = ra::lum(r, gr, b);
          const int v[3] = {ra::blend(l, r, factor), ra::blend(l, gr, factor), ra::blend(l, b, factor)};
#pragma unroll
          for (int c = 0; c < 3; ++c) o[(3 * i + c) >> 2] |= (uint32_t)v[c] << (((3 * i + c) & 3) * 8);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) cur32[3 * g + i] = o[i];
      }
      __syncthreads();
      continue;
    }

    // ---- byte -> byte through a lookup table
    int mean = 0;
    if (op == ra::AUTOCONTRAST || op == ra::EQUALIZE) {
      if (tid < 768) hist[tid] = 0u;
      __syncthreads();
      for (int j = tid; j < nwords; j += RA_THREADS) {
        const uint32_t w = cur32[j];
        int c = j % 3;  // byte 4 j is of channel (4 j) % 3 = j % 3
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (4 * j + i < n) atomicAdd(&hist[c * 256 + ((w >> (8 * i)) & 255)], 1u);
          c = c == 2 ? 0 : c + 1;
        }
      }
      __syncthreads();
      if (tid < 192) {  // wave c builds the table of channel c, 4 bins per lane
        const int c = tid >> 6, lane = tid & 63;
        int h[4], occ = 0, lo = 256, hi = -1, s = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          h[i] = (int)hist[c * 256 + 4 * lane + i];
          s += h[i];
          if (h[i]) {
            ++occ;
            lo = min(lo, 4 * lane + i);
            hi = 4 * lane + i;
          }
        }
        lo = wave_min(lo);
        hi = wave_max(hi);
        int step = 0, below = 0;
        if (op == ra::EQUALIZE) {
          occ = wave_sum(occ);
          step = ra::equalize_step(occ, P, hi >= 0 ? (int)hist[c * 256 + hi] : 0);
          int inc = s;
          for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
          }
          below = inc - s;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int v = 4 * lane + i;
          lut[c * 256 + v] =
              (uint8_t)(op == ra::EQUALIZE ? ra::equalize_lut(step, below, v) : ra::autocontrast_lut(lo, hi, v));
          below += h[i];
        }
      }
    } else {
      if (op == ra::CONTRAST) {  // ImageEnhance.Contrast: int(mean of convert("L") + 0.5), in integers
        if (tid == 0) *lsum = 0u;
        __syncthreads();
        uint32_t acc = 0u;
        for (int g = tid; g < ngroups; g += RA_THREADS) {
          const uint32_t w[3] = {cur32[3 * g], cur32[3 * g + 1], cur32[3 * g + 2]};
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (4 * g + i < P) acc += (uint32_t)ra::lum(byte_of(w, 3 * i), byte_of(w, 3 * i + 1), byte_of(w, 3 * i + 2));
        }
        acc = (uint32_t)wave_sum((int)acc);
        if ((tid & 63) == 0) atomicAdd(lsum, acc);
        __syncthreads();
        mean = (int)((2u * *lsum + (uint32_t)P) / (2u * (uint32_t)P));
      }
      if (tid < 768) lut[tid] = (uint8_t)ra::lut_param(op, p, mean, tid & 255);
    }
    __syncthreads();
    for (int j = tid; j < nwords; j += RA_THREADS) {
      const uint32_t w = cur32[j];
      const int c0 = j % 3, c1 = c0 == 2 ? 0 : c0 + 1, c2 = c1 == 2 ? 0 : c1 + 1;
      cur32[j] = (uint32_t)lut[c0 * 256 + (w & 255)] | (uint32_t)lut[c1 * 256 + ((w >> 8) & 255)] << 8 |
                 (uint32_t)lut[c2 * 256 + ((w >> 16) & 255)] << 16 | (uint32_t)lut[c0 * 256 + (w >> 24)] << 24;
    }
    __syncthreads();
  }

  if (in_lds) {
    if (vec16) {
      for (int i = tid; i < (n >> 4); i += RA_THREADS)
        reinterpret_cast<uint4*>(gout)[i] = reinterpret_cast<const uint4*>(cur)[i];
    } else {
      for (int i = tid; i < n; i += RA_THREADS) gout[i] = cur[i];
    }
  }
}

}  // namespace

int rand_augment_max_bytes() { return RA_CAP; }

int launch_rand_augment(const uint8_t* in, const int* plan, int N, int K, int H, int W, uint8_t* out, hipStream_t s) {
  const long long n = (long long)H * W * 3;
  if (H <= 0 || W <= 0 || n > RA_CAP) return 1;
  if (K < 1 || K > 4) return 2;
  if (N <= 0) return 0;
  const int buf = (int)((n + 47) / 48 * 48);
  const bool two = 2 * buf <= RA_CAP;
  const uintptr_t both = reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out);
  const int flags = ((n % 16 == 0 && both % 16 == 0) ? 1 : 0) |
                    ((n % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0) ? 2 : 0) | (two ? 4 : 0);
  const int lds = (two ? 2 : 1) * buf + RA_AUX;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)rand_augment_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              RA_CAP + RA_AUX);
    attr = true;
  }
  hipLaunchKernelGGL(rand_augment_kernel, dim3((unsigned)N), dim3(RA_THREADS), lds, s, in, plan, K, H, W, buf, flags,
                     out);
  return 0;
}

}  // namespace dcp

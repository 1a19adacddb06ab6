// The two per-image device passes of prediction on images without an HR partner (srhip/predict.py), one launch each:
//   * srhip_ingest_pad: integer pages -> float32 in [0, 1] (uint2single / uint162single, dlib/utils/utils_image.py:322-331)
//     and, for SwinIR, the flipped-strip padding of _forward_with_padding (dlib/utils/utils_trainer.py:829-862) -- the cast,
//     the division and the two cat + flip of the reference in one pass,
//   * srhip_emit_uint: float32 -> integer pages (tensor2uint / single2uint16, utils_image.py:334-335,362-366) of the top-left
//     Ho x Wo rectangle -- the slice, clamp, multiply, round and cast in one pass -- with a non-finite flag.
// Both are row copies with arithmetic.  A thread owns four consecutive pixels of one row, cut so that the FLOAT side (four
// bytes a pixel, most of the traffic) is one aligned 16-byte access: a row whose first float is `a` elements past a 16-byte
// boundary is walked in groups [4g - a, 4g - a + 4); the first and last group of a row may be partial and go element by
// element.  The integer side of a full group is one 4-byte (8-bit pages) or 8-byte (16-bit pages) access where that piece is
// aligned, else four scalar ones.  Any width works, odd ones included.
#include "common.h"
#include "levels.h"

namespace {

typedef unsigned char u8;
typedef unsigned short u16;
typedef u8 u8x4 __attribute__((ext_vector_type(4)));
typedef u16 u16x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Vec4;
template <> struct Vec4<u8> { typedef u8x4 type; };
template <> struct Vec4<u16> { typedef u16x4 type; };

// dst[b][i][j] = unit(src[b][ri(i)][rj(j)]), ri(i) = i < H ? i : 2H - 1 - i (row H + k is row H - 1 - k), rj alike: the
// columns are reflected in the row-padded image, so the corner is flipped both ways.  G groups per row (see above).
template <typename T>
__global__ __launch_bounds__(256) void k_ingest_pad(const T* __restrict__ src, float* __restrict__ dst, long rows, int H, int W,
                                                    int Hp, int Wp, int G, unsigned in_max) {
  typedef typename Vec4<T>::type TV;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = t / G;                                       // b * Hp + i
  if (row >= rows) return;
  const int g = (int)(t - row * G);
  const int b = (int)(row / Hp), i = (int)(row - (long)b * Hp);
  const int si = i < H ? i : 2 * H - 1 - i;                     // 0 <= si < H: the host checked Hp - H <= H
  const T* s = src + ((long)b * H + si) * W;
  float* d = dst + row * Wp;
  const int a = (int)((((uintptr_t)d) >> 2) & 3);
  const int j0 = 4 * g - a;
  if (j0 >= Wp) return;
  const double dmax = (double)in_max;
  if (j0 >= 0 && j0 + 3 < Wp) {
    unsigned v0, v1, v2, v3;
    if (j0 + 3 < W && (((uintptr_t)(s + j0)) & (4 * sizeof(T) - 1)) == 0) {
      const TV v = *(const TV*)(s + j0);
      v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
    } else {                                                    // 0 <= 2W - 1 - j < W: the host checked Wp - W <= W
      v0 = s[j0 < W ? j0 : 2 * W - 1 - j0];
      v1 = s[j0 + 1 < W ? j0 + 1 : 2 * W - 2 - j0];
      v2 = s[j0 + 2 < W ? j0 + 2 : 2 * W - 3 - j0];
      v3 = s[j0 + 3 < W ? j0 + 3 : 2 * W - 4 - j0];
    }
    *(f32x4*)(d + j0) = f32x4{unit_of(v0, in_max, dmax), unit_of(v1, in_max, dmax), unit_of(v2, in_max, dmax),
                              unit_of(v3, in_max, dmax)};
  } else {
    for (int j = max(j0, 0); j < min(j0 + 4, Wp); ++j) d[j] = unit_of(s[j < W ? j : 2 * W - 1 - j], in_max, dmax);
  }
}

// level_of (levels.h) with the non-finite flag
__device__ __forceinline__ unsigned uint_of(float x, float out_max, int& bad) {
  bad |= !(fabsf(x) <= 3.402823466e+38f);                       // NaN or +-inf
  return level_of(x, out_max);
}

// dst[b][i][j] = uint_of(x[b][i][j]) for i < Ho, j < Wo; the groups follow the alignment of x's rows (16-byte loads)
template <typename T>
__global__ __launch_bounds__(256) void k_emit_uint(const float* __restrict__ x, T* __restrict__ dst, long rows, int Hs, int Ws,
                                                   int Ho, int Wo, int G, float out_max, int* __restrict__ nonfinite) {
  typedef typename Vec4<T>::type TV;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = t / G;                                       // b * Ho + i
  if (row >= rows) return;
  const int g = (int)(t - row * G);
  const int b = (int)(row / Ho), i = (int)(row - (long)b * Ho);
  const float* s = x + ((long)b * Hs + i) * Ws;
  T* d = dst + row * Wo;
  const int a = (int)((((uintptr_t)s) >> 2) & 3);
  const int j0 = 4 * g - a;
  if (j0 >= Wo) return;
  int bad = 0;
  if (j0 >= 0 && j0 + 3 < Wo) {
    const f32x4 v = ldg_f4(s + j0);
    const unsigned u0 = uint_of(v.x, out_max, bad), u1 = uint_of(v.y, out_max, bad), u2 = uint_of(v.z, out_max, bad),
                   u3 = uint_of(v.w, out_max, bad);
    if ((((uintptr_t)(d + j0)) & (4 * sizeof(T) - 1)) == 0) {
      *(TV*)(d + j0) = TV{(T)u0, (T)u1, (T)u2, (T)u3};
    } else {
      d[j0] = (T)u0, d[j0 + 1] = (T)u1, d[j0 + 2] = (T)u2, d[j0 + 3] = (T)u3;
    }
  } else {
    for (int j = max(j0, 0); j < min(j0 + 4, Wo); ++j) d[j] = (T)uint_of(ldg_f(s + j), out_max, bad);
  }
  if (bad && nonfinite) atomicOr(nonfinite, 1);                 // rare; an integer atomic, every writer stores the same bit
}

}  // namespace

extern "C" {

/* dst[b][Hp][Wp] = float32(min(src, in_max) / in_max), rows then columns extended by flipped strips (include/srhip.h) */
int srhip_ingest_pad(const void* src, int bits, int in_max, int B, int H, int W, float* dst, int Hp, int Wp, void* stream) {
  SR_REQUIRE(src && dst, "ingest_pad: NULL argument");
  SR_REQUIRE(bits == 8 || bits == 16, "ingest_pad: 8- or 16-bit pages (got %d)", bits);
  SR_REQUIRE(in_max >= 1 && in_max <= (bits == 8 ? 255 : 65535), "ingest_pad: 1 <= in_max <= %d for %d-bit pages (got %d)",
             bits == 8 ? 255 : 65535, bits, in_max);
  SR_REQUIRE(B > 0 && H > 0 && W > 0, "ingest_pad: B, H, W > 0 (got %d, %d, %d)", B, H, W);
  SR_REQUIRE(Hp >= H && Wp >= W, "ingest_pad: the target %d x %d is smaller than the page %d x %d", Hp, Wp, H, W);
  // the reference's slice im[H - pad :] would start at a negative index: there is no rule for that case
  SR_REQUIRE(Hp - H <= H && Wp - W <= W, "ingest_pad: a %d x %d page cannot be padded to %d x %d (the pad exceeds the page)", H,
             W, Hp, Wp);
  SR_REQUIRE((((uintptr_t)src) & (bits / 8 - 1)) == 0 && (((uintptr_t)dst) & 3) == 0, "ingest_pad: misaligned pointer");
  const long es = bits / 8, rows = (long)B * Hp;
  SR_REQUIRE(sr_disjoint(src, (long)B * H * W * es, dst, rows * Wp * 4), "ingest_pad: dst overlaps src");
  const int G = (Wp + 3 + 3) / 4;                               // groups of a row whose first float is 3 past a 16-byte boundary
  const long blocks = (rows * G + 255) / 256;
  SR_REQUIRE(blocks <= 0x7fffffffL, "ingest_pad: too many pixels");
  if (bits == 8)
    hipLaunchKernelGGL(k_ingest_pad<u8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const u8*)src, dst, rows, H,
                       W, Hp, Wp, G, (unsigned)in_max);
  else
    hipLaunchKernelGGL(k_ingest_pad<u16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const u16*)src, dst, rows,
                       H, W, Hp, Wp, G, (unsigned)in_max);
  SR_LAUNCH_CHECK("ingest_pad");
  return 0;
}

/* dst[b][Ho][Wo] = round_half_even(clamp(x[b][: Ho][: Wo], 0, 1) * (2^bits - 1)) (include/srhip.h) */
int srhip_emit_uint(const float* x, int B, int Hs, int Ws, void* dst, int bits, int Ho, int Wo, int* nonfinite, void* stream) {
  SR_REQUIRE(x && dst, "emit_uint: NULL argument");
  SR_REQUIRE(bits == 8 || bits == 16, "emit_uint: 8- or 16-bit pages (got %d)", bits);
  SR_REQUIRE(B > 0 && Hs > 0 && Ws > 0, "emit_uint: B, Hs, Ws > 0 (got %d, %d, %d)", B, Hs, Ws);
  SR_REQUIRE(Ho > 0 && Wo > 0 && Ho <= Hs && Wo <= Ws, "emit_uint: the crop %d x %d is not inside the image %d x %d", Ho, Wo, Hs,
             Ws);
  SR_REQUIRE((((uintptr_t)x) & 3) == 0 && (((uintptr_t)dst) & (bits / 8 - 1)) == 0 && (((uintptr_t)nonfinite) & 3) == 0,
             "emit_uint: misaligned pointer");
  const long es = bits / 8, rows = (long)B * Ho;
  SR_REQUIRE(sr_disjoint(x, (long)B * Hs * Ws * 4, dst, rows * Wo * es), "emit_uint: dst overlaps x");
  SR_REQUIRE(sr_disjoint(nonfinite, 4, dst, rows * Wo * es) && sr_disjoint(nonfinite, 4, x, (long)B * Hs * Ws * 4),
             "emit_uint: the flag overlaps an image");
  const int G = (Wo + 3 + 3) / 4;
  const long blocks = (rows * G + 255) / 256;
  SR_REQUIRE(blocks <= 0x7fffffffL, "emit_uint: too many pixels");
  if (bits == 8)
    hipLaunchKernelGGL(k_emit_uint<u8>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (u8*)dst, rows, Hs, Ws, Ho,
                       Wo, G, 255.0f, nonfinite);
  else
    hipLaunchKernelGGL(k_emit_uint<u16>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (u16*)dst, rows, Hs, Ws,
                       Ho, Wo, G, 65535.0f, nonfinite);
  SR_LAUNCH_CHECK("emit_uint");
  return 0;
}

}  // extern "C"

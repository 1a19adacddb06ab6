// The camera model behind --lr_synth psf: the low-resolution image of an HR-only pair as a microscope would record it, not as
// an antialiased bicubic down-scaling.  Two entry points (include/srhip.h states the arithmetic, dlib/datasets/lowres.py
// restates it in numpy: psf_bin_np, photon_noise_np):
//
//   srhip_psf_bin       clean = bin_s(G_sigma * HR), once per tile: scipy's Gaussian filter ('reflect' border, any radius) and
//                       the mean over s x s pixels folded into ONE strided correlation per axis with the 2 r + s weights
//                       box_s (*) gaussian.  Two launches, along the rows and then down the columns, float64 sums in ascending
//                       tap order, one rounding to float32 per pass.  A thread makes four neighbouring outputs of one row.
//   srhip_photon_noise  LR = (Poisson(photons * clean) + read_std * N(0, 1)) / photons in place on a gathered batch, fresh per
//                       batch: every draw is Philox4x32-10 of (pixel, sample, attempt) under a seed read from device memory, so
//                       the result does not depend on the launch geometry and a captured launch replays with the seed of that
//                       moment.  The Poisson sampler is exact: inversion below 30, Hoermann's transformed rejection (PTRS) from
//                       30 on.  One thread per pixel.
//
// Both are memory- and latency-sized work (a 1024 x 1024 tile once per set; 8 x 64 x 64 pixels per batch).
#include "common.h"
#include "levels.h"
#include "philox.h"
#include <math.h>

// every product and sum below is rounded on its own, as numpy rounds them: a fused multiply-add would move last bits
#pragma clang fp contract(off)

namespace {

constexpr int PSF_MAX_RADIUS = 64;      // ops.LR_BLUR_MAX_RADIUS, the bound of srhip_lr_augment's blur
constexpr int PSF_RUN = 4;              // outputs per thread: one 16-byte store
constexpr int NOISE_CHUNK = 1024;       // samples per launch of the noise kernel: their flags travel as a kernel argument

enum { KIND_F32 = 0, KIND_U8 = 1, KIND_U16 = 2 };

// scipy's 'reflect' border (d c b a | a b c d | d c b a) for any distance from the line
__device__ __forceinline__ int reflect(int i, int n) {
  if (i >= 0 && i < n) return i;
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

template <int KIND>
__device__ __forceinline__ double source_value(const void* src, long at, unsigned in_max, double dmax) {
  if (KIND == KIND_U8) return (double)(float)((double)((const unsigned char*)src)[at] / 255.0);
  if (KIND == KIND_U16) return (double)unit_of(((const unsigned short*)src)[at], in_max, dmax);
  return (double)ldg_f((const float*)src + at);
}

// along a row: tmp[b][y][ox] = sum_k wt[k] src[b][y][reflect(ox s - r + k, W)], k ascending.  VEC: whole runs per row of tmp
// on a 16-byte aligned buffer.
template <int KIND, bool VEC>
__global__ void __launch_bounds__(256) k_psf_bin_x(const void* __restrict__ src, float* __restrict__ tmp, long rows, int W, int Wo,
                                                   int s, const double* __restrict__ wt, int taps, int radius, unsigned in_max) {
  const int runs = (Wo + PSF_RUN - 1) / PSF_RUN;
  const long item = blockIdx.x * 256L + threadIdx.x;
  if (item >= rows * runs) return;
  const int ox0 = (int)(item % runs) * PSF_RUN;
  const long row = item / runs;                 // b * H + y
  const long base = row * W;
  const double dmax = (double)in_max;
  int first[PSF_RUN];
#pragma unroll
  for (int e = 0; e < PSF_RUN; ++e) first[e] = min(ox0 + e, Wo - 1) * s - radius;   // a ragged run recomputes the row's last output
  double acc[PSF_RUN] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < taps; ++k) {
    const double w = wt[k];
#pragma unroll
    for (int e = 0; e < PSF_RUN; ++e) acc[e] += w * source_value<KIND>(src, base + reflect(first[e] + k, W), in_max, dmax);
  }
  float* d = tmp + row * Wo + ox0;
  if (VEC) {
    *(f32x4*)d = f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
  } else {
#pragma unroll
    for (int e = 0; e < PSF_RUN; ++e)
      if (ox0 + e < Wo) d[e] = (float)acc[e];
  }
}

// down the columns: dst[b][oy][ox] = sum_k wt[k] tmp[b][reflect(oy s - r + k, H)][ox], k ascending.  VEC: a tap is one 16-byte
// load of four neighbouring columns and the result one 16-byte store.
template <bool VEC>
__global__ void __launch_bounds__(256) k_psf_bin_y(const float* __restrict__ tmp, float* __restrict__ dst, int B, int H, int Ho,
                                                   int Wo, int s, const double* __restrict__ wt, int taps, int radius) {
  const int runs = (Wo + PSF_RUN - 1) / PSF_RUN;
  const long item = blockIdx.x * 256L + threadIdx.x;
  if (item >= (long)B * Ho * runs) return;
  const int ox0 = (int)(item % runs) * PSF_RUN;
  const long row = item / runs;                 // b * Ho + oy
  const int oy = (int)(row % Ho);
  const float* img = tmp + (row / Ho) * (long)H * Wo;
  const int first = oy * s - radius;
  double acc[PSF_RUN] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < taps; ++k) {
    const double w = wt[k];
    const float* p = img + (long)reflect(first + k, H) * Wo + ox0;
    float v[PSF_RUN];
    if (VEC) {
      const f32x4 q = ldg_f4(p);
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
      for (int e = 0; e < PSF_RUN; ++e) v[e] = ox0 + e < Wo ? ldg_f(p + e) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < PSF_RUN; ++e) acc[e] += w * (double)v[e];
  }
  float* d = dst + row * Wo + ox0;
  if (VEC) {
    *(f32x4*)d = f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
  } else {
#pragma unroll
    for (int e = 0; e < PSF_RUN; ++e)
      if (ox0 + e < Wo) d[e] = (float)acc[e];
  }
}

// a 32-bit word as a double strictly inside (0, 1), and one standard normal from two words: augment.hip's rules
__device__ __forceinline__ double u01(unsigned w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }
__device__ __forceinline__ double normal01(unsigned w1, unsigned w2) {
  return sqrt(-2.0 * log(u01(w1))) * cos(6.283185307179586 * u01(w2));
}

// Poisson(lam), 0 < lam < 30: inversion by sequential search from one uniform
__device__ __forceinline__ double poisson_inversion(double lam, double u) {
  double p = exp(-lam), cum = p;
  int k = 0;
  while (u > cum && k < 255) {
    ++k;
    p = p * lam / (double)k;
    cum += p;
  }
  return (double)k;
}

// Poisson(lam), lam >= 30: W. Hoermann, "The transformed rejection method for generating Poisson random variables" (1993),
// algorithm PTRS, attempt t from words (2 t % 4, 2 t % 4 + 1) of counter (i, b, t / 2); after 16 rejections round(lam)
__device__ double poisson_ptrs(double lam, unsigned i, unsigned b, uint4 c, unsigned k0, unsigned k1) {
  const double slam = sqrt(lam), loglam = log(lam);
  const double bb = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * bb;
  const double invalpha = 1.1239 + 1.1328 / (bb - 3.4);
  const double vr = 0.9277 - 3.6224 / (bb - 2.0);
  for (int t = 0; t < 16; ++t) {
    if (t > 0 && (t & 1) == 0) c = philox4x32_10(i, b, (unsigned)(t >> 1), k0, k1);
    const double U = u01((t & 1) ? c.z : c.x) - 0.5;
    const double V = u01((t & 1) ? c.w : c.y);
    const double us = 0.5 - fabs(U);
    const double k = floor((2.0 * a / us + bb) * U + lam + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    if (log(V) + log(invalpha) - log(a / (us * us) + bb) <= -lam + k * loglam - lgamma(k + 1.0)) return k;
  }
  return rint(lam);
}

struct OnMask {
  unsigned m[NOISE_CHUNK / 32];
};

// one thread per pixel of the samples b0 .. b0 + nb - 1; sample b0 + j is touched iff bit j of the mask is set
__global__ void __launch_bounds__(256) k_photon_noise(float* x, int b0, int nb, int hw, const long long* seed, OnMask on,
                                                      double photons, double read_std) {
  const long e = blockIdx.x * 256L + threadIdx.x;
  if (e >= (long)nb * hw) return;
  const int j = (int)(e / hw);
  if (!((on.m[j >> 5] >> (j & 31)) & 1u)) return;
  const unsigned i = (unsigned)(e - (long)j * hw), b = (unsigned)(b0 + j);
  const unsigned long long sd = (unsigned long long)*seed;
  const unsigned k0 = (unsigned)sd, k1 = (unsigned)(sd >> 32);
  float* px = x + (long)b0 * hw + e;
  const double lam = photons * (double)*px;
  double n = 0.0;
  if (lam > 0.0) {        // a pixel at or below 0 (or not a number) records no photon
    const uint4 c = philox4x32_10(i, b, 0u, k0, k1);
    n = lam < 30.0 ? poisson_inversion(lam, u01(c.x)) : poisson_ptrs(lam, i, b, c, k0, k1);
  }
  if (read_std != 0.0) {
    const uint4 g = philox4x32_10(i, b, 0x80000000u, k0, k1);
    n = n + read_std * normal01(g.x, g.y);
  }
  *px = (float)(n / photons);
}

}  // namespace

extern "C" {

/* clean = bin_s(G_sigma * HR) of B one-channel images (include/srhip.h) */
int srhip_psf_bin(const void* src, int kind, int in_max, const double* weights, int n_taps, float* tmp, float* dst, int B, int H,
                  int W, int s, void* stream) {
  SR_REQUIRE(src && weights && tmp && dst, "psf_bin: NULL argument");
  SR_REQUIRE(kind == KIND_F32 || kind == KIND_U8 || kind == KIND_U16, "psf_bin: kind %d (0 float32, 1 uint8, 2 uint16)", kind);
  SR_REQUIRE(kind != KIND_U16 || (in_max >= 1 && in_max <= 65535), "psf_bin: 1 <= in_max <= 65535 (got %d)", in_max);
  SR_REQUIRE(s >= 2 && s <= 16, "psf_bin: the bin side s is 2 .. 16 (got %d)", s);
  SR_REQUIRE(B > 0 && H > 0 && W > 0 && H % s == 0 && W % s == 0, "psf_bin: H and W are multiples of s (got %d x %d x %d, s = %d)",
             B, H, W, s);
  SR_REQUIRE(n_taps >= s && (n_taps - s) % 2 == 0, "psf_bin: 2 * radius + s weights (got %d, s = %d)", n_taps, s);
  const int radius = (n_taps - s) / 2;
  SR_REQUIRE(radius <= PSF_MAX_RADIUS, "psf_bin: the blur radius is 0 .. %d (got %d)", PSF_MAX_RADIUS, radius);
  const int es = kind == KIND_F32 ? 4 : (kind == KIND_U8 ? 1 : 2);
  SR_REQUIRE(((uintptr_t)src & (es - 1)) == 0 && ((uintptr_t)tmp & 3) == 0 && ((uintptr_t)dst & 3) == 0 && ((uintptr_t)weights & 7) == 0,
             "psf_bin: misaligned pointer");
  const int Ho = H / s, Wo = W / s;
  const long src_bytes = (long)B * H * W * es, tmp_bytes = (long)B * H * Wo * 4, dst_bytes = (long)B * Ho * Wo * 4, wt_bytes = n_taps * 8L;
  SR_REQUIRE(sr_disjoint(tmp, tmp_bytes, src, src_bytes) && sr_disjoint(dst, dst_bytes, src, src_bytes) &&
             sr_disjoint(dst, dst_bytes, tmp, tmp_bytes) && sr_disjoint(weights, wt_bytes, tmp, tmp_bytes) &&
             sr_disjoint(weights, wt_bytes, dst, dst_bytes), "psf_bin: src, weights, tmp and dst overlap");
  const int runs = sr_cdiv(Wo, PSF_RUN);
  const long n1 = ((long)B * H * runs + 255) / 256, n2 = ((long)B * Ho * runs + 255) / 256;
  SR_REQUIRE((long)B * H * W < (1L << 31) && n1 < (1L << 31), "psf_bin: too many pixels for one launch");
  const hipStream_t st = (hipStream_t)stream;
  const dim3 g1((unsigned)n1), g2((unsigned)n2), blk(256);
  // 16-byte accesses where every row of tmp / dst starts on one: whole runs per row and aligned bases
  const bool v1 = Wo % PSF_RUN == 0 && ((uintptr_t)tmp & 15) == 0;
  const bool v2 = v1 && ((uintptr_t)dst & 15) == 0;
  const long rows = (long)B * H;
  const unsigned im = (unsigned)(kind == KIND_U16 ? in_max : 1);
#define PSF_X(KIND, VEC) \
  hipLaunchKernelGGL((k_psf_bin_x<KIND, VEC>), g1, blk, 0, st, src, tmp, rows, W, Wo, s, weights, n_taps, radius, im)
  if (kind == KIND_F32) { if (v1) PSF_X(KIND_F32, true); else PSF_X(KIND_F32, false); }
  else if (kind == KIND_U8) { if (v1) PSF_X(KIND_U8, true); else PSF_X(KIND_U8, false); }
  else { if (v1) PSF_X(KIND_U16, true); else PSF_X(KIND_U16, false); }
#undef PSF_X
  SR_LAUNCH_CHECK("psf_bin along the rows");
  if (v2) hipLaunchKernelGGL(k_psf_bin_y<true>, g2, blk, 0, st, (const float*)tmp, dst, B, H, Ho, Wo, s, weights, n_taps, radius);
  else hipLaunchKernelGGL(k_psf_bin_y<false>, g2, blk, 0, st, (const float*)tmp, dst, B, H, Ho, Wo, s, weights, n_taps, radius);
  SR_LAUNCH_CHECK("psf_bin down the columns");
  return 0;
}

/* x = (Poisson(photons * x) + read_std * N(0, 1)) / photons in place on x [B][1][h][w] (include/srhip.h) */
int srhip_photon_noise(float* x, int B, int h, int w, const long long* seed, const unsigned char* on, double photons,
                       double read_std, void* stream) {
  SR_REQUIRE(x && seed, "photon_noise: NULL argument");
  SR_REQUIRE(B > 0 && h > 0 && w > 0 && (long)B * h * w < (1L << 31), "photon_noise: B, h, w > 0 and B * h * w < 2^31 (got %d, %d, %d)",
             B, h, w);
  SR_REQUIRE(photons > 0.0 && photons <= 1e6, "photon_noise: photons lies in (0, 1e6] (got %g)", photons);
  SR_REQUIRE(read_std >= 0.0 && isfinite(read_std), "photon_noise: read_std is a finite number >= 0 (got %g)", read_std);
  SR_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)seed & 7) == 0, "photon_noise: misaligned pointer");
  const int hw = h * w;
  for (int b0 = 0; b0 < B; b0 += NOISE_CHUNK) {
    const int nb = B - b0 < NOISE_CHUNK ? B - b0 : NOISE_CHUNK;
    OnMask m;
    memset(&m, 0, sizeof(m));
    bool any = false;
    for (int j = 0; j < nb; ++j)
      if (!on || on[b0 + j]) {
        m.m[j >> 5] |= 1u << (j & 31);
        any = true;
      }
    if (!any) continue;
    hipLaunchKernelGGL(k_photon_noise, dim3((unsigned)sr_cdiv((long)nb * hw, 256)), dim3(256), 0, (hipStream_t)stream, x, b0, nb, hw,
                       seed, m, photons, read_std);
    SR_LAUNCH_CHECK("photon_noise");
  }
  return 0;
}

}  // extern "C"

// cv2.resize(..., interpolation=cv2.INTER_CUBIC) on 1-channel images: the 'l_to_h_img' tensors of the reference's
// dataset (dlib/datasets/dataset_dpsr.py:659-683 _resize_low_to_scale: uint8 tiles at construction / evaluation,
// :813-821,:836,:905-906 float32 patches after the LR-only augmentations), consumed by the SRCNN-style nets
// (model_plain.py:184-195).
//
// cv2 is not in this image and its source is not under /root/reference: this restates OpenCV's published algorithm
// (imgproc/resize.cpp: interpolateCubic with A = -0.75; pixel centre mapping fx = (dx + 0.5) * scale - 0.5; border
// replicate; uint8 images in fixed point -- coefficients rounded to 1/2048 (INTER_RESIZE_COEF_BITS = 11), horizontal
// pass in int, vertical pass (sum + 2^21) >> 22 saturated; float32 images in plain float arithmetic).  PARITY UNPINNED
// against cv2 itself (OpenCV's vectorised vertical pass rounds a float sum instead of the integer one: on rare
// near-ties it may differ by one grey level); pinned bit-exact (uint8) / 1e-6 (float32) against oracle/cv2_cubic.py,
// the same restatement in numpy.
#include "common.h"
#include "../../include/srhip.h"

namespace {

// identical float arithmetic on host and device: no FMA contraction in the coefficient formulas
#pragma clang fp contract(off)
__host__ __device__ inline void cubic_coeffs(float x, float (&c)[4]) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

template <bool U8>
__global__ void __launch_bounds__(256) k_resize_cubic(const void* __restrict__ srcv, void* __restrict__ dstv, int B, int H,
                                                      int W, int Ho, int Wo, double scale_y, double scale_x) {
#pragma clang fp contract(off)
  const long n = (long)B * Ho * Wo;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int dx = (int)(i % Wo), dy = (int)((i / Wo) % Ho);
    const long b = i / ((long)Wo * Ho);
    float fx = (float)((dx + 0.5) * scale_x - 0.5), fy = (float)((dy + 0.5) * scale_y - 0.5);
    const int sx = (int)floorf(fx), sy = (int)floorf(fy);
    fx -= sx; fy -= sy;
    float cx[4], cy[4];
    cubic_coeffs(fx, cx);
    cubic_coeffs(fy, cy);
    int xs[4], ys[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      xs[k] = min(max(sx - 1 + k, 0), W - 1);
      ys[k] = min(max(sy - 1 + k, 0), H - 1);
    }
    if (U8) {
      const unsigned char* src = (const unsigned char*)srcv + b * H * W;
      int ax[4], ay[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {       // saturate_cast<short>(c * 2048): round to nearest even, as cvRound
        ax[k] = (int)rintf(cx[k] * 2048.f);
        ay[k] = (int)rintf(cy[k] * 2048.f);
      }
      int acc = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned char* row = src + (long)ys[r] * W;
        const int h = row[xs[0]] * ax[0] + row[xs[1]] * ax[1] + row[xs[2]] * ax[2] + row[xs[3]] * ax[3];
        acc += h * ay[r];
      }
      const int v = (acc + (1 << 21)) >> 22;
      ((unsigned char*)dstv)[i] = (unsigned char)min(max(v, 0), 255);
    } else {
      const float* src = (const float*)srcv + b * H * W;
      float hr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* row = src + (long)ys[r] * W;
        hr[r] = row[xs[0]] * cx[0] + row[xs[1]] * cx[1] + row[xs[2]] * cx[2] + row[xs[3]] * cx[3];
      }
      ((float*)dstv)[i] = hr[0] * cy[0] + hr[1] * cy[1] + hr[2] * cy[2] + hr[3] * cy[3];
    }
  }
}

// uint8 -> float32 / 255 (util.uint2single, utils_image.py:322-323) and clip to [0, 1], in place variants used around the resize
__global__ void __launch_bounds__(256) k_u8_to_unit(const unsigned char* __restrict__ src, float* __restrict__ dst, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (float)((double)src[i] / 255.0);
}
__global__ void __launch_bounds__(256) k_clip01(float* __restrict__ x, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) x[i] = fminf(fmaxf(x[i], 0.f), 1.f);
}

// ---- the multi-scale loss's target pyramid: F.interpolate(mode="bicubic", align_corners=True) [+ clamp to [0, 1]] ----------
// torch's bicubic (aten/src/ATen/native/UpSample.h: area_pixel_compute_scale / guard_index_and_lambda /
// get_cubic_upsample_coefficients, A = -0.75; cpu/UpSampleKernel.cpp: separable, horizontal inside vertical), evaluated the
// way torch evaluates it on float64 input and rounded ONCE to f32.  torch's float32 kernel forms the source coordinate as the
// f32 product of an f32 scale (H - 1) / (Ho - 1) and the output index: at 512 pixels that moves the fractional part by ~3e-5
// and the resized target by up to 6e-5 (3e-6 at 32 pixels) -- 2.5e-5 of the L2 gradient 2 lam (y - t) / N of a level whose
// output sits 0.1 from the target, where the loss kernels themselves are held to 1e-6.  Here the coordinate is the exact
// rational o (H - 1) / (Ho - 1) (integer quotient and remainder), the four coefficients and the 16-tap sum are f64 (the
// f64 FMA rate of this GPU equals the f32 one; the kernel waits for its 16 loads per pixel either way).
constexpr int PYR_MAXL = 8;     // levels per launch
constexpr int PYR_RUN = 4;      // consecutive output pixels of one row per thread: one 16-byte store
constexpr int PYR_MAXDIM = 32768;   // image edge: o * (n_in - 1) stays inside 32 bits

struct PyrArgs {
  float* dst[PYR_MAXL];
  int Ho[PYR_MAXL], Wo[PYR_MAXL];
  int runs[PYR_MAXL];           // runs per output row: ceil(Wo / PYR_RUN)
  int vec[PYR_MAXL];            // rows are whole runs and dst is 16-byte aligned: float4 stores
  int blk0[PYR_MAXL + 1];       // first block of each level (prefix sums): block -> level
  int n;
};

__device__ __forceinline__ void bicubic_coeffs_torch(double t, double (&c)[4]) {
  const double A = -0.75;
  const double x0 = t + 1.0, x2 = 1.0 - t, x3 = x2 + 1.0;
  c[0] = ((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A;
  c[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
  c[2] = ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0;
  c[3] = ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A;
}

// source index and fractional part of output index o < n_out: o * (n_in - 1) / (n_out - 1), 0 for a single output pixel
__device__ __forceinline__ int bicubic_src(int n_in, int n_out, int o, double& t) {
  if (n_out == 1) { t = 0.0; return 0; }
  const unsigned num = (unsigned)o * (unsigned)(n_in - 1), d = (unsigned)(n_out - 1);   // sizes <= PYR_MAXDIM: no overflow
  const unsigned q = num / d;
  t = (double)(num - q * d) / (double)d;
  return (int)q;
}

__global__ void __launch_bounds__(256) k_bicubic_ac_pyramid(const float* __restrict__ src, int B, int H, int W, PyrArgs a,
                                                            int clamp01) {
  int l = 0;
  while (l + 1 < a.n && (int)blockIdx.x >= a.blk0[l + 1]) ++l;
  const int Ho = a.Ho[l], Wo = a.Wo[l], runs = a.runs[l];
  const long item = (long)((int)blockIdx.x - a.blk0[l]) * 256 + threadIdx.x;
  if (item >= (long)B * Ho * runs) return;
  const int ox0 = (int)(item % runs) * PYR_RUN;
  const long row = item / runs;                 // b * Ho + oy
  const int oy = (int)(row % Ho);
  const float* img = src + (row / Ho) * (long)H * W;
  double ty, cy[4];
  const int iy = bicubic_src(H, Ho, oy, ty);
  bicubic_coeffs_torch(ty, cy);
  const float* r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = img + (long)min(max(iy - 1 + k, 0), H - 1) * W;
  float out[PYR_RUN];
#pragma unroll
  for (int j = 0; j < PYR_RUN; ++j) {
    const int ox = min(ox0 + j, Wo - 1);        // a ragged row's last run recomputes its last pixel; stored once below
    double tx, cx[4];
    const int ix = bicubic_src(W, Wo, ox, tx);
    bicubic_coeffs_torch(tx, cx);
    int xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[k] = min(max(ix - 1 + k, 0), W - 1);
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double h = (double)ldg_f(r[k] + xs[0]) * cx[0];
      h = fma((double)ldg_f(r[k] + xs[1]), cx[1], h);
      h = fma((double)ldg_f(r[k] + xs[2]), cx[2], h);
      h = fma((double)ldg_f(r[k] + xs[3]), cx[3], h);
      v = k == 0 ? h * cy[0] : fma(h, cy[k], v);
    }
    if (clamp01) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);     // torch.clamp: a NaN stays a NaN
    out[j] = (float)v;
  }
  float* d = a.dst[l] + row * Wo + ox0;
  if (a.vec[l]) {
    *(f32x4*)d = f32x4{out[0], out[1], out[2], out[3]};
  } else {
#pragma unroll
    for (int j = 0; j < PYR_RUN; ++j)
      if (ox0 + j < Wo) d[j] = out[j];
  }
}

inline int rs_grid(long n) {
  long g = (n + 255) / 256;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" {

int srhip_resize_cubic(const void* src, void* dst, int is_u8, int B, int H, int W, int Ho, int Wo, void* stream) {
  SR_REQUIRE(src && dst && B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "resize_cubic: empty image / NULL argument");
  const double sy = (double)H / Ho, sx = (double)W / Wo;      // scale = 1 / inv_scale, inv_scale = dsize / ssize (resize.cpp)
  const double scale_y = 1.0 / ((double)Ho / H), scale_x = 1.0 / ((double)Wo / W);
  (void)sy; (void)sx;
  const long n = (long)B * Ho * Wo;
  if (is_u8) hipLaunchKernelGGL(k_resize_cubic<true>, dim3(rs_grid(n)), dim3(256), 0, (hipStream_t)stream, src, dst, B, H, W, Ho, Wo, scale_y, scale_x);
  else hipLaunchKernelGGL(k_resize_cubic<false>, dim3(rs_grid(n)), dim3(256), 0, (hipStream_t)stream, src, dst, B, H, W, Ho, Wo, scale_y, scale_x);
  SR_LAUNCH_CHECK("resize_cubic");
  return 0;
}

int srhip_u8_to_unit(const unsigned char* src, float* dst, long n, void* stream) {
  SR_REQUIRE(src && dst && n > 0, "u8_to_unit: empty");
  hipLaunchKernelGGL(k_u8_to_unit, dim3(rs_grid(n)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
  SR_LAUNCH_CHECK("u8_to_unit");
  return 0;
}

int srhip_clip01(float* x, long n, void* stream) {
  SR_REQUIRE(x && n > 0, "clip01: empty");
  hipLaunchKernelGGL(k_clip01, dim3(rs_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n);
  SR_LAUNCH_CHECK("clip01");
  return 0;
}

int srhip_resize_bicubic_ac_pyramid(const float* src, int B, int H, int W, const srhip_pyr_level* levels, int n, int clamp01,
                                    void* stream) {
  SR_REQUIRE(src && levels && B > 0 && H > 0 && W > 0, "resize_bicubic_ac_pyramid: empty image / NULL argument");
  SR_REQUIRE(H <= PYR_MAXDIM && W <= PYR_MAXDIM, "resize_bicubic_ac_pyramid: source larger than %d pixels a side", PYR_MAXDIM);
  SR_REQUIRE(n >= 1 && n <= PYR_MAXL, "resize_bicubic_ac_pyramid: %d levels (1 .. %d per call)", n, PYR_MAXL);
  const long src_bytes = (long)B * H * W * 4;
  PyrArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n;
  long blk = 0;
  for (int l = 0; l < n; ++l) {
    const srhip_pyr_level& lv = levels[l];
    SR_REQUIRE(lv.dst && lv.Ho > 0 && lv.Wo > 0, "resize_bicubic_ac_pyramid: level %d is empty / NULL", l);
    SR_REQUIRE(lv.Ho <= PYR_MAXDIM && lv.Wo <= PYR_MAXDIM, "resize_bicubic_ac_pyramid: level %d larger than %d pixels a side", l,
               PYR_MAXDIM);
    const long bytes = (long)B * lv.Ho * lv.Wo * 4;
    SR_REQUIRE(sr_disjoint(lv.dst, bytes, src, src_bytes), "resize_bicubic_ac_pyramid: level %d overlaps the source", l);
    for (int m = 0; m < l; ++m)
      SR_REQUIRE(sr_disjoint(lv.dst, bytes, levels[m].dst, (long)B * levels[m].Ho * levels[m].Wo * 4),
                 "resize_bicubic_ac_pyramid: levels %d and %d overlap", m, l);
    a.dst[l] = lv.dst;
    a.Ho[l] = lv.Ho;
    a.Wo[l] = lv.Wo;
    a.runs[l] = sr_cdiv(lv.Wo, PYR_RUN);
    a.vec[l] = lv.Wo % PYR_RUN == 0 && ((uintptr_t)lv.dst & 15) == 0;
    a.blk0[l] = (int)blk;
    blk += ((long)B * lv.Ho * a.runs[l] + 255) / 256;
    SR_REQUIRE(blk < (1L << 31), "resize_bicubic_ac_pyramid: too many output pixels for one launch");
  }
  for (int l = n; l <= PYR_MAXL; ++l) a.blk0[l] = (int)blk;
  hipLaunchKernelGGL(k_bicubic_ac_pyramid, dim3((unsigned)blk), dim3(256), 0, (hipStream_t)stream, src, B, H, W, a, clamp01);
  SR_LAUNCH_CHECK("resize_bicubic_ac_pyramid");
  return 0;
}

}  // extern "C"

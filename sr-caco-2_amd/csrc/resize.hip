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
#include "levels.h"
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

// ---- util.imresize_np(img, scale, antialiasing=True), scale < 1: MATLAB-style antialiased bicubic down-scaling -------------
// dlib/utils/utils_image.py:1358-1422 (cubic, calculate_weights_indices), :1505-1578 (imresize_np); the low-resolution image
// of an HR-only pair (dataset_dpsr.py:798-824).  Along each axis output pixel o (1-based x = o + 1) sits at the input
// coordinate u = x / scale + (1 - 1 / scale) / 2; its taps are the P = ceil(4 / scale) + 2 pixels from floor(u - 2 / scale)
// on, weighted by scale * cubic((u - i) * scale) (the Keys kernel, a = -0.5, stretched by 1 / scale) and normalised to sum
// 1; a tap outside the image is mirrored about the border with the edge pixel repeated.  Rows first (contraction over H)
// into an f32 intermediate [B][Ho][W], then columns: the reference stores out_1 in float32, so does this.  Coordinates,
// weights and sums are f64, rounded once per pass; every weight is recomputed from the output index, so there is no table
// and nothing to reduce across threads: bit-identical from run to run.
//
// Two launches, one per axis.  The rows pass has one thread per 4 consecutive columns of one output row: its taps are rows
// of the source, so a wave reads and writes whole contiguous row segments (16 bytes a lane when the rows allow).  The columns
// pass has one thread per 4 consecutive output pixels, which walk the same intermediate row 4 / scale floats apart: those
// loads are strided, the row segment a wave covers stays in L1 / L2 for all of its taps, and the store is 16 bytes a lane.
constexpr int AA_RUN = 4;          // pixels per thread: one 16-byte access
constexpr int AA_MAXDIM = 32768;   // image edge
constexpr int AA_MAXTAPS = 258;    // ceil(4 / scale) + 2 at scale = 1 / 64

__host__ __device__ inline double aa_cubic(double x) {
#pragma clang fp contract(off)
  const double a = fabs(x), a2 = a * a, a3 = a2 * a;
  if (a <= 1.0) return 1.5 * a3 - 2.5 * a2 + 1.0;
  if (a <= 2.0) return -0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0;
  return 0.0;
}
// input coordinate (1-based) of output pixel o and its left-most tap (1-based)
__host__ __device__ inline int aa_left(int o, double scale, double& u) {
#pragma clang fp contract(off)
  u = (double)(o + 1) / scale + 0.5 * (1.0 - 1.0 / scale);
  return (int)floor(u - (4.0 / scale) / 2.0);
}
// un-normalised weight of tap k
__host__ __device__ inline double aa_weight(double u, int left, int k, double scale) {
#pragma clang fp contract(off)
  return scale * aa_cubic((u - (double)(left + k)) * scale);
}
// 0-based source index of tap k, mirrored about the borders with the edge repeated; outside [0, n) only when the tap lies
// more than n pixels beyond a border
__host__ __device__ inline int aa_index(int left, int k, int n) {
  const int j = left + k - 1;
  return j < 0 ? -j - 1 : (j >= n ? 2 * n - 1 - j : j);
}
__host__ __device__ inline double aa_weight_sum(double u, int left, int P, double scale) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int k = 0; k < P; ++k) s += aa_weight(u, left, k, scale);
  return s;
}
// every tap of non-zero weight mirrors into the image (the kernels skip the others)
inline bool aa_axis_fits(int n_in, int n_out, int P, double scale) {
  for (int o = 0; o < n_out; ++o) {
    double u;
    const int left = aa_left(o, scale, u);
    const double ws = aa_weight_sum(u, left, P, scale);
    for (int k = 0; k < P; ++k) {
      if (aa_weight(u, left, k, scale) / ws == 0.0) continue;
      const int j = aa_index(left, k, n_in);
      if (j < 0 || j >= n_in) return false;
    }
  }
  return true;
}

template <bool U8, bool VEC>
__global__ void __launch_bounds__(256) k_imresize_aa_rows(const void* __restrict__ srcv, float* __restrict__ tmp, int B, int H,
                                                          int W, int Ho, double scale, int P) {
#pragma clang fp contract(off)
  const int runs = (W + AA_RUN - 1) / AA_RUN;
  const long item = blockIdx.x * 256L + threadIdx.x;
  if (item >= (long)B * Ho * runs) return;
  const int x0 = (int)(item % runs) * AA_RUN;
  const long row = item / runs;                 // b * Ho + oy
  const int oy = (int)(row % Ho);
  const long img = (row / Ho) * (long)H * W;
  double u;
  const int left = aa_left(oy, scale, u);
  const double ws = aa_weight_sum(u, left, P, scale);
  double acc[AA_RUN] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < P; ++k) {
    const double w = aa_weight(u, left, k, scale) / ws;
    if (w == 0.0) continue;                     // its mirrored row may lie outside a small image: never dereferenced
    const int j = min(max(aa_index(left, k, H), 0), H - 1);     // in range already: the entry point refuses shapes where not
    const long off = img + (long)j * W + x0;
    float v[AA_RUN];
    if (U8) {
      const unsigned char* p = (const unsigned char*)srcv + off;
      if (VEC) {
        const unsigned q = *(const unsigned*)p;
#pragma unroll
        for (int e = 0; e < AA_RUN; ++e) v[e] = (float)((double)((q >> (8 * e)) & 255u) / 255.0);
      } else {
#pragma unroll
        for (int e = 0; e < AA_RUN; ++e) v[e] = x0 + e < W ? (float)((double)p[e] / 255.0) : 0.f;
      }
    } else {
      const float* p = (const float*)srcv + off;
      if (VEC) {
        const f32x4 q = ldg_f4(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
#pragma unroll
        for (int e = 0; e < AA_RUN; ++e) v[e] = x0 + e < W ? ldg_f(p + e) : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < AA_RUN; ++e) acc[e] += w * (double)v[e];
  }
  float* d = tmp + row * W + x0;
  if (VEC) {
    *(f32x4*)d = f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
  } else {
#pragma unroll
    for (int e = 0; e < AA_RUN; ++e)
      if (x0 + e < W) d[e] = (float)acc[e];
  }
}

// The rows pass on a 16-BIT source, read at full depth by unit_of (levels.h): the same weights, tap order and f64 sums, so a
// source of 257 v gives the bits of the uint8 kernel on v.  One thread per 8 consecutive columns: with VEC (whole runs per row,
// 16-byte aligned src and tmp) a tap is ONE 16-byte load of 8 pixels and the result two 16-byte stores.
constexpr int AA_RUN16 = 8;
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

template <bool VEC>
__global__ void __launch_bounds__(256) k_imresize_aa_rows_u16(const unsigned short* __restrict__ src, float* __restrict__ tmp,
                                                              int B, int H, int W, int Ho, double scale, int P, unsigned in_max) {
#pragma clang fp contract(off)
  const int runs = (W + AA_RUN16 - 1) / AA_RUN16;
  const long item = blockIdx.x * 256L + threadIdx.x;
  if (item >= (long)B * Ho * runs) return;
  const int x0 = (int)(item % runs) * AA_RUN16;
  const long row = item / runs;                 // b * Ho + oy
  const int oy = (int)(row % Ho);
  const long img = (row / Ho) * (long)H * W;
  const double dmax = (double)in_max;
  double u;
  const int left = aa_left(oy, scale, u);
  const double ws = aa_weight_sum(u, left, P, scale);
  double acc[AA_RUN16] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < P; ++k) {
    const double w = aa_weight(u, left, k, scale) / ws;
    if (w == 0.0) continue;                     // as k_imresize_aa_rows: never dereferenced
    const int j = min(max(aa_index(left, k, H), 0), H - 1);
    const unsigned short* p = src + img + (long)j * W + x0;
    float v[AA_RUN16];
    if (VEC) {
      const u16x8 q = *(const u16x8*)p;
#pragma unroll
      for (int e = 0; e < AA_RUN16; ++e) v[e] = unit_of(q[e], in_max, dmax);
    } else {
#pragma unroll
      for (int e = 0; e < AA_RUN16; ++e) v[e] = x0 + e < W ? unit_of(p[e], in_max, dmax) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < AA_RUN16; ++e) acc[e] += w * (double)v[e];
  }
  float* d = tmp + row * W + x0;
  if (VEC) {
    *(f32x4*)d = f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
    *(f32x4*)(d + 4) = f32x4{(float)acc[4], (float)acc[5], (float)acc[6], (float)acc[7]};
  } else {
#pragma unroll
    for (int e = 0; e < AA_RUN16; ++e)
      if (x0 + e < W) d[e] = (float)acc[e];
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_imresize_aa_cols(const float* __restrict__ tmp, float* __restrict__ dst, long rows, int W,
                                                          int Wo, double scale, int P) {
#pragma clang fp contract(off)
  const int runs = (Wo + AA_RUN - 1) / AA_RUN;
  const long item = blockIdx.x * 256L + threadIdx.x;
  if (item >= rows * runs) return;
  const int ox0 = (int)(item % runs) * AA_RUN;
  const long row = item / runs;                 // b * Ho + oy
  const float* src = tmp + row * W;
  float out[AA_RUN];
#pragma unroll
  for (int e = 0; e < AA_RUN; ++e) {
    const int ox = min(ox0 + e, Wo - 1);        // a ragged row's last run recomputes its last pixel; stored once below
    double u;
    const int left = aa_left(ox, scale, u);
    const double ws = aa_weight_sum(u, left, P, scale);
    double acc = 0.0;
    for (int k = 0; k < P; ++k) {
      const double w = aa_weight(u, left, k, scale) / ws;
      if (w == 0.0) continue;
      const int j = min(max(aa_index(left, k, W), 0), W - 1);
      acc += w * (double)ldg_f(src + j);
    }
    out[e] = (float)acc;
  }
  float* d = dst + row * Wo + ox0;
  if (VEC) {
    *(f32x4*)d = f32x4{out[0], out[1], out[2], out[3]};
  } else {
#pragma unroll
    for (int e = 0; e < AA_RUN; ++e)
      if (ox0 + e < Wo) d[e] = out[e];
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

// both entry points: es = bytes per source pixel (4 float32, 1 uint8, 2 uint16 read by in_max)
static int imresize_aa_run(const void* src, int es, int in_max, float* tmp, float* dst, int B, int H, int W, int Ho, int Wo,
                           double scale, void* stream) {
  const bool is_u8 = es == 1;
  SR_REQUIRE(src && tmp && dst && B > 0 && H > 0 && W > 0, "imresize_aa: empty image / NULL argument");
  SR_REQUIRE(scale > 0.0 && scale < 1.0 && scale >= 1.0 / 64, "imresize_aa: scale %g (antialiased down-scaling: 1/64 <= scale < 1)",
             scale);
  SR_REQUIRE(H <= AA_MAXDIM && W <= AA_MAXDIM, "imresize_aa: source larger than %d pixels a side", AA_MAXDIM);
  SR_REQUIRE(Ho == (int)ceil(H * scale) && Wo == (int)ceil(W * scale), "imresize_aa: output %dx%d is not ceil(%dx%d * %g)", Ho, Wo,
             H, W, scale);
  const int P = (int)ceil(4.0 / scale) + 2;
  SR_REQUIRE(P <= AA_MAXTAPS, "imresize_aa: %d taps (at most %d)", P, AA_MAXTAPS);
  SR_REQUIRE(aa_axis_fits(H, Ho, P, scale) && aa_axis_fits(W, Wo, P, scale),
             "imresize_aa: a %dx%d image is too small for scale %g: a tap would mirror past the opposite border", H, W, scale);
  const long src_bytes = (long)B * H * W * es, tmp_bytes = (long)B * Ho * W * 4, dst_bytes = (long)B * Ho * Wo * 4;
  SR_REQUIRE(sr_disjoint(tmp, tmp_bytes, src, src_bytes) && sr_disjoint(dst, dst_bytes, src, src_bytes) &&
             sr_disjoint(dst, dst_bytes, tmp, tmp_bytes), "imresize_aa: src, tmp and dst overlap");
  const long n1 = ((long)B * Ho * sr_cdiv(W, es == 2 ? AA_RUN16 : AA_RUN) + 255) / 256;
  const long n2 = ((long)B * Ho * sr_cdiv(Wo, AA_RUN) + 255) / 256;
  SR_REQUIRE(n1 < (1L << 31) && n2 < (1L << 31), "imresize_aa: too many pixels for one launch");
  hipStream_t st = (hipStream_t)stream;
  // 16-byte accesses where every row starts on one: whole runs per row and aligned bases (4 bytes for a uint8 source)
  const bool v1 = W % AA_RUN == 0 && ((uintptr_t)src & (is_u8 ? 3 : 15)) == 0 && ((uintptr_t)tmp & 15) == 0;
  const bool v2 = Wo % AA_RUN == 0 && ((uintptr_t)dst & 15) == 0;
  const dim3 g1((unsigned)n1), g2((unsigned)n2), blk(256);
  if (es == 2) {      // 8 pixels a thread: whole runs per row and 16-byte aligned bases
    const bool v16 = W % AA_RUN16 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)tmp & 15) == 0;
    const unsigned short* s16 = (const unsigned short*)src;
    if (v16) hipLaunchKernelGGL(k_imresize_aa_rows_u16<true>, g1, blk, 0, st, s16, tmp, B, H, W, Ho, scale, P, (unsigned)in_max);
    else hipLaunchKernelGGL(k_imresize_aa_rows_u16<false>, g1, blk, 0, st, s16, tmp, B, H, W, Ho, scale, P, (unsigned)in_max);
  } else if (is_u8) {
    if (v1) hipLaunchKernelGGL((k_imresize_aa_rows<true, true>), g1, blk, 0, st, src, tmp, B, H, W, Ho, scale, P);
    else hipLaunchKernelGGL((k_imresize_aa_rows<true, false>), g1, blk, 0, st, src, tmp, B, H, W, Ho, scale, P);
  } else {
    if (v1) hipLaunchKernelGGL((k_imresize_aa_rows<false, true>), g1, blk, 0, st, src, tmp, B, H, W, Ho, scale, P);
    else hipLaunchKernelGGL((k_imresize_aa_rows<false, false>), g1, blk, 0, st, src, tmp, B, H, W, Ho, scale, P);
  }
  if (v2) hipLaunchKernelGGL(k_imresize_aa_cols<true>, g2, blk, 0, st, (const float*)tmp, dst, (long)B * Ho, W, Wo, scale, P);
  else hipLaunchKernelGGL(k_imresize_aa_cols<false>, g2, blk, 0, st, (const float*)tmp, dst, (long)B * Ho, W, Wo, scale, P);
  SR_LAUNCH_CHECK("imresize_aa");
  return 0;
}

int srhip_imresize_aa(const void* src, int is_u8, float* tmp, float* dst, int B, int H, int W, int Ho, int Wo, double scale,
                      void* stream) {
  return imresize_aa_run(src, is_u8 ? 1 : 4, 0, tmp, dst, B, H, W, Ho, Wo, scale, stream);
}

int srhip_imresize_aa_u16(const unsigned short* src, int in_max, float* tmp, float* dst, int B, int H, int W, int Ho, int Wo,
                          double scale, void* stream) {
  SR_REQUIRE(in_max >= 1 && in_max <= 65535, "imresize_aa_u16: 1 <= in_max <= 65535 (got %d)", in_max);
  SR_REQUIRE((((uintptr_t)src) & 1) == 0, "imresize_aa_u16: misaligned pointer");
  return imresize_aa_run(src, 2, in_max, tmp, dst, B, H, W, Ho, Wo, scale, stream);
}

}  // extern "C"

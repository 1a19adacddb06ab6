// The LR-only augmentations of a training batch (np_blur, np_prod_binary_noise, np_add_gaussian_noise and their random block,
// dlib/datasets/dataset_dpsr.py:899-905,1060-1180) in place on the gathered low-resolution patches [B][1][h][w]: every draw is
// a pure function of (seed, sample, stage) or of (seed, site, element index) through Philox4x32-10, so nothing is read back
// or uploaded per batch and the result does not depend on the launch geometry.  The seed is read from device memory: launches
// captured in a hipGraph replay with whatever the seed tensor holds then.  include/srhip.h states the draws and the
// arithmetic, tests/lr_augment_ref.py restates them in numpy.
//
// Three launches: the Gaussian blur along the rows axis and along the columns axis (only when the blur is on; float64
// accumulation, float32 stores, through the caller's workspace), then one pass that selects blurred or original pixels, applies
// the Bernoulli mask and adds the noise.  Each thread of that pass recomputes the (sample, stage) block it needs: two Philox
// calls per stage, against a round trip through memory.  Memory- and latency-bound on a few hundred KB.
#include "common.h"
#include "philox.h"
#include <math.h>

// every product and sum below is rounded on its own, as numpy and scipy round them: a fused multiply-add would move last bits
#pragma clang fp contract(off)

namespace {

typedef srhip_lr_augment_params Params;

// a 32-bit word as a double strictly inside (0, 1)
__device__ __forceinline__ double u01(unsigned w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }
// one standard normal from two words (Box-Muller, the cosine branch)
__device__ __forceinline__ double normal01(unsigned w1, unsigned w2) {
  return sqrt(-2.0 * log(u01(w1))) * cos(6.283185307179586 * u01(w2));
}

__device__ __forceinline__ bool stage_applied(int b, int s, double prob, double area, unsigned k0, unsigned k1, uint4& a) {
  a = philox4x32_10((unsigned)b, 0xFFFFFFFFu, (unsigned)s, k0, k1);
  return area != 0.0 && u01(a.x) < prob;
}

// the random block of stage s in sample b (get_random_coordinates_block, :1060-1070, with the block clamped to the patch)
struct Block {
  bool applied, inside;
  int ch, cw, bh, bw;
  __device__ __forceinline__ bool has(int y, int x) const { return y >= ch && y < ch + bh && x >= cw && x < cw + bw; }
};
__device__ __forceinline__ int block_side(int n, double ratio) {
  const long v = (long)((double)n * ratio);           // np.int64(h * ratio): towards zero
  return (int)(v < 0 ? 0 : (v > n ? n : v));
}
__device__ __forceinline__ int block_origin(int n, int bn, unsigned w) {
  const int v = (int)floor(u01(w) * (double)(n - bn + 1));
  return v < n - bn ? v : n - bn;
}
__device__ Block stage_block(int b, int s, int h, int w, double prob, double area, unsigned k0, unsigned k1) {
  Block r{false, false, 0, 0, 0, 0};
  uint4 a;
  r.applied = stage_applied(b, s, prob, area, k0, k1, a);
  if (!r.applied) return r;
  const uint4 c = philox4x32_10((unsigned)b, 0xFFFFFFFEu, (unsigned)s, k0, k1);
  const double ratio = normal01(a.y, a.z) * 0.01 + area;
  r.bh = block_side(h, ratio);
  r.bw = block_side(w, ratio);
  r.ch = block_origin(h, r.bh, a.w);
  r.cw = block_origin(w, r.bw, c.x);
  r.inside = u01(c.y) >= 0.98;
  return r;
}

// scipy's 'reflect' border (d c b a | a b c d | d c b a) for any distance from the line
__device__ __forceinline__ int reflect(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// One axis of scipy.ndimage.gaussian_filter(img_hwc, sigma) (correlate1d's symmetric form: the centre tap first, then the
// pairs from the farthest to the nearest), float64 accumulation, one rounding to float32.  AXIS 0 filters along the rows
// index (scipy's first pass), AXIS 1 along the columns index and then applies the pass over the channel axis of length 1:
// the same sum over one value, reflected onto itself.  Samples whose blur is not applied are left alone: nobody reads them.
template <int AXIS>
__global__ __launch_bounds__(256) void k_blur_pass(const float* __restrict__ in, float* __restrict__ out, int B, int h, int w,
                                                   const double* __restrict__ wt, int radius, const long long* seed,
                                                   double prob, double area) {
  const unsigned long long sd = (unsigned long long)*seed;
  const unsigned k0 = (unsigned)sd, k1 = (unsigned)(sd >> 32);
  const long hw = (long)h * w, n = (long)B * hw;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;         // one thread per pixel: n < 2^31, so the grid holds it
  if (e < n) {
    const int b = (int)(e / hw);
    uint4 a;
    if (!stage_applied(b, 0, prob, area, k0, k1, a)) return;
    const int rem = (int)(e - (long)b * hw), y = rem / w, x = rem - y * w;
    const float* img = in + (long)b * hw;
    const int len = AXIS == 0 ? h : w, pos = AXIS == 0 ? y : x, step = AXIS == 0 ? w : 1, base = AXIS == 0 ? x : y * w;
    double acc = (double)img[base + pos * step] * wt[radius];
    for (int jj = -radius; jj < 0; ++jj) {
      const double lo = (double)img[base + reflect(pos + jj, len) * step];
      const double hi = (double)img[base + reflect(pos - jj, len) * step];
      acc += (lo + hi) * wt[radius + jj];
    }
    float v = (float)acc;
    if (AXIS == 1) {
      const double d = (double)v;
      acc = d * wt[radius];
      for (int jj = -radius; jj < 0; ++jj) acc += (d + d) * wt[radius + jj];
      v = (float)acc;
    }
    out[e] = v;
  }
}

// One thread per Philox group of four consecutive elements of the whole batch (a group may straddle two samples when h * w is
// no multiple of 4).  VEC: x is 16-byte aligned, so a whole group is one 16-byte load and one 16-byte store.
template <bool VEC>
__global__ __launch_bounds__(256) void k_lr_compose(float* x, const float* __restrict__ blurred, int B, int h, int w,
                                                    const long long* seed, Params p, unsigned thr) {
  const unsigned long long sd = (unsigned long long)*seed;
  const unsigned k0 = (unsigned)sd, k1 = (unsigned)(sd >> 32);
  const long hw = (long)h * w, n = (long)B * hw;
  const long ngroups = (n + 3) >> 2;
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < ngroups) {
    const long i = q << 2;
    const int cnt = (int)(n - i < 4 ? n - i : 4);
    const bool whole = VEC && cnt == 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (whole) {
      const f32x4 t = *(const f32x4*)(x + i);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      for (int j = 0; j < cnt; ++j) v[j] = x[i + j];
    }
    const unsigned g0 = (unsigned)q, g1 = (unsigned)((unsigned long long)q >> 32);
    uint4 m{0u, 0u, 0u, 0u}, n1{0u, 0u, 0u, 0u}, n2{0u, 0u, 0u, 0u};
    if (p.dot_on) m = philox4x32_10(g0, g1, 1u, k0, k1);
    if (p.gaus_on) {
      n1 = philox4x32_10(g0, g1, 2u, k0, k1);
      n2 = philox4x32_10(g0, g1, 3u, k0, k1);
    }
    const unsigned mw[4] = {m.x, m.y, m.z, m.w}, w1[4] = {n1.x, n1.y, n1.z, n1.w}, w2[4] = {n2.x, n2.y, n2.z, n2.w};
    int cur = -1;
    Block blk[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) break;
      const long e = i + j;
      const int b = (int)(e / hw);
      if (b != cur) {
        cur = b;
        blk[0] = p.blur_on ? stage_block(b, 0, h, w, p.blur_prob, p.blur_area, k0, k1) : Block{false, false, 0, 0, 0, 0};
        blk[1] = p.dot_on ? stage_block(b, 1, h, w, p.dot_prob, p.dot_area, k0, k1) : Block{false, false, 0, 0, 0, 0};
        blk[2] = p.gaus_on ? stage_block(b, 2, h, w, p.gaus_prob, p.gaus_area, k0, k1) : Block{false, false, 0, 0, 0, 0};
      }
      const int rem = (int)(e - (long)b * hw), y = rem / w, xx = rem - y * w;
      float t = v[j];
      if (blk[0].applied && blk[0].has(y, xx) == blk[0].inside) t = blurred[e];
      if (blk[1].applied && blk[1].has(y, xx)) t = t * (mw[j] >= thr ? 1.0f : 0.0f);
      if (blk[2].applied && blk[2].has(y, xx)) t = (float)((double)t + p.gaus_std * normal01(w1[j], w2[j]));
      v[j] = t;
    }
    if (whole) {
      *(f32x4*)(x + i) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
      for (int j = 0; j < cnt; ++j) x[i + j] = v[j];
    }
  }
}

bool unit(double v) { return v >= 0.0 && v <= 1.0; }

}  // namespace

extern "C" {

/* blur, dot noise, Gaussian noise on x [B][1][h][w] in place (include/srhip.h) */
int srhip_lr_augment(float* x, int B, int h, int w, const long long* seed, const srhip_lr_augment_params* params,
                     const double* blur_weights, float* workspace, void* stream) {
  SR_REQUIRE(x && seed && params, "lr_augment: bad operand");
  SR_REQUIRE(B > 0 && h > 0 && w > 0 && (long)B * h * w < (1L << 31), "lr_augment: B, h, w > 0 and B * h * w < 2^31 (got %d, %d, %d)",
             B, h, w);
  const Params p = *params;
  SR_REQUIRE(!p.blur_on || (unit(p.blur_prob) && unit(p.blur_area)), "lr_augment: blur: prob and area lie in [0, 1] (got %g, %g)",
             p.blur_prob, p.blur_area);
  SR_REQUIRE(!p.dot_on || (unit(p.dot_prob) && unit(p.dot_area)), "lr_augment: dot noise: prob and area lie in [0, 1] (got %g, %g)",
             p.dot_prob, p.dot_area);
  SR_REQUIRE(!p.gaus_on || (unit(p.gaus_prob) && unit(p.gaus_area)),
             "lr_augment: Gaussian noise: prob and area lie in [0, 1] (got %g, %g)", p.gaus_prob, p.gaus_area);
  SR_REQUIRE(!p.dot_on || (p.dot_p >= 0.0 && p.dot_p < 1.0), "lr_augment: dot noise: 0 <= p < 1 (got %g)", p.dot_p);
  SR_REQUIRE(!p.gaus_on || (p.gaus_std >= 0.0 && isfinite(p.gaus_std)), "lr_augment: Gaussian noise: std >= 0 (got %g)", p.gaus_std);
  const long n = (long)B * h * w;
  const hipStream_t st = (hipStream_t)stream;
  float* blurred = nullptr;
  if (p.blur_on) {
    SR_REQUIRE(p.blur_radius >= 0 && p.blur_radius <= 64, "lr_augment: the blur radius is 0 .. 64 (got %d)", p.blur_radius);
    SR_REQUIRE(blur_weights && workspace, "lr_augment: the blur needs its weights and a workspace of 2 * B * h * w floats");
    SR_REQUIRE(sr_disjoint(x, n * 4, workspace, 2 * n * 4), "lr_augment: the workspace overlaps x");
    blurred = workspace + n;
    const int grid = sr_cdiv(n, 256);
    hipLaunchKernelGGL(k_blur_pass<0>, dim3(grid), dim3(256), 0, st, (const float*)x, workspace, B, h, w, blur_weights,
                       p.blur_radius, seed, p.blur_prob, p.blur_area);
    SR_LAUNCH_CHECK("lr_augment blur rows");
    hipLaunchKernelGGL(k_blur_pass<1>, dim3(grid), dim3(256), 0, st, (const float*)workspace, blurred, B, h, w, blur_weights,
                       p.blur_radius, seed, p.blur_prob, p.blur_area);
    SR_LAUNCH_CHECK("lr_augment blur columns");
  }
  if (!p.blur_on && !p.dot_on && !p.gaus_on) return 0;
  const double t = rint(p.dot_p * 4294967296.0);          // round(p 2^32), the rule of srhip_dropout without its rescale
  const unsigned thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
  const int grid = sr_cdiv((n + 3) >> 2, 256);
  if (((uintptr_t)x & 15) == 0)
    hipLaunchKernelGGL(k_lr_compose<true>, dim3(grid), dim3(256), 0, st, x, (const float*)blurred, B, h, w, seed, p, thr);
  else
    hipLaunchKernelGGL(k_lr_compose<false>, dim3(grid), dim3(256), 0, st, x, (const float*)blurred, B, h, w, seed, p, thr);
  SR_LAUNCH_CHECK("lr_augment compose");
  return 0;
}

}  // extern "C"

// Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) as an evaluation metric at L levels, float64 (--msssim).  Not a reference
// call: the definition is the one of include/srhip.h.
//
// One launch per scale (k_msssim_scale) and one for the product (k_msssim_fin).  A block of a scale stages its 32 x 16 output tile
// plus the 10-pixel halo of both images once, takes the five window moments of srhip_metrics_ssim_lv (ssim.hip: the same taps, the
// same two separable passes in LDS, in double, over the integer values, scaled after the passes) and stores its (sum cs, sum ss);
// out of the same staged pixels it writes its share of the next scale's image pair.  A scale's images are therefore read from HBM
// once, and a call is M + 1 launches.
//
// The pyramid is kept as integer sums: scale j holds, per pixel, the sum of the 4^(j-1) levels below it (a zero where the grid of
// F.avg_pool2d(x, 2, padding=(h % 2, w % 2)) reaches in front of an odd extent), below L * 4^4 < 2^24, so exact in uint32 and in
// the float32 of the staging; x = sum / (L * 4^(j-1)) is formed after the passes.  Nothing is accumulated with atomics.
#include "common.h"
#include "kernels.h"
#include "levels.h"
#include "ssim_taps.h"

namespace {

constexpr int TX = 32, TY = 16, WS = 11;                // output tile, window (those of k_ssim_metric_lv)
constexpr int IX = TX + WS - 1, IY = TY + WS - 1;       // staged inputs
constexpr int MAXM = 5;
static_assert(2 * IY * IX * sizeof(float) + 5 * IY * TX * sizeof(double) + 8 * sizeof(double) <= 48 * 1024,
              "k_msssim_scale: static LDS");

__host__ __device__ inline int pooled(int n) { return (n + 1) / 2; }

// The pooled pixel p of an axis of extent n covers the inputs 2p - (n % 2) and 2p - (n % 2) + 1.  It belongs to the tile that
// holds the first of them (input -1, the zero in front, goes with input 0); the last tile of the axis has staged the axis to its
// end and owns all that is left.  Returns the first pooled pixel of the tile at origin o0.
__device__ __forceinline__ int pool_first(int o0, int pad) { return o0 == 0 ? 0 : (o0 + pad + 1) / 2; }

// part[b][tile][2] doubles (sum cs, sum ss).  FIRST: E / Hh are the float images [B][H][W] (quantised here, cropped by border);
// else cur = the uint32 pair [B][2][h][w] of this scale.  next (or NULL): the pair [B][2][ceil(h/2)][ceil(w/2)] of the next one.
template <bool FIRST>
__global__ void __launch_bounds__(256) k_msssim_scale(const float* __restrict__ E, const float* __restrict__ Hh,
                                                      const unsigned* __restrict__ cur, unsigned* __restrict__ next,
                                                      double* __restrict__ part, int H, int W, int border, int h, int w,
                                                      int L, int in_is_lv, double inv_div, Taps tp) {
  __shared__ float sx[IY * IX], sy[IY * IX];
  __shared__ double sh[5 * IY * TX];
  __shared__ double red[4][2];
  const int b = blockIdx.z, oy0 = blockIdx.y * TY, ox0 = blockIdx.x * TX;
  const int oh = h - (WS - 1), ow = w - (WS - 1);          // valid output
  const int tid = threadIdx.x;
  const float fL = (float)L;
  const long img = (long)b * H * W, plane = (long)h * w;
  for (int i = tid; i < IY * IX; i += 256) {
    const int r = i / IX, c = i - r * IX;
    const int y = oy0 + r, x = ox0 + c;
    float a = 0.f, t = 0.f;
    if (y < h && x < w) {
      if (FIRST) {
        const long o = img + (long)(y + border) * W + x + border;
        a = metric_level(E[o], in_is_lv, fL);
        t = metric_level(Hh[o], in_is_lv, fL);
      } else {
        const long o = (long)b * 2 * plane + (long)y * w + x;
        a = (float)cur[o];
        t = (float)cur[o + plane];
      }
    }
    sx[i] = a; sy[i] = t;
  }
  __syncthreads();
  if (next) {                                              // block-uniform
    const int pady = h & 1, padx = w & 1, ph = pooled(h), pw = pooled(w);
    const int py0 = pool_first(oy0, pady), px0 = pool_first(ox0, padx);
    const int py1 = blockIdx.y + 1 == gridDim.y ? ph : pool_first(oy0 + TY, pady);
    const int px1 = blockIdx.x + 1 == gridDim.x ? pw : pool_first(ox0 + TX, padx);
    const int ny = py1 - py0, nx = px1 - px0;
    const long pplane = (long)ph * pw;
    for (int i = tid; i < ny * nx; i += 256) {
      const int py = py0 + i / nx, px = px0 + i % nx;
      const int r = 2 * py - pady - oy0, c = 2 * px - padx - ox0;      // -1: the zero in front; r + 1 < IY, c + 1 < IX
      float a = 0.f, t = 0.f;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          if (r + dy >= 0 && c + dx >= 0) { a += sx[(r + dy) * IX + c + dx]; t += sy[(r + dy) * IX + c + dx]; }
      const long o = (long)b * 2 * pplane + (long)py * pw + px;
      next[o] = (unsigned)a;
      next[o + pplane] = (unsigned)t;
    }
  }
  for (int i = tid; i < IY * TX; i += 256) {
    const int r = i / TX, c = i - r * TX;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (int k = 0; k < WS; ++k) {
      const double x = (double)sx[r * IX + c + k], y = (double)sy[r * IX + c + k], g = (double)tp.g[k];
      a0 += g * x; a1 += g * y; a2 += g * (x * x); a3 += g * (y * y); a4 += g * (x * y);
    }
    sh[(0 * IY + r) * TX + c] = a0; sh[(1 * IY + r) * TX + c] = a1; sh[(2 * IY + r) * TX + c] = a2;
    sh[(3 * IY + r) * TX + c] = a3; sh[(4 * IY + r) * TX + c] = a4;
  }
  __syncthreads();
  const int tx = tid & 31, ty = tid >> 5;
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const double i1 = inv_div, i2 = inv_div * inv_div;
  double scs = 0, sss = 0;
#pragma unroll
  for (int k2 = 0; k2 < TY / 8; ++k2) {
    const int r = ty + 8 * k2;
    if (oy0 + r < oh && ox0 + tx < ow) {
      double m[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        double a = 0;
        for (int k = 0; k < WS; ++k) a += (double)tp.g[k] * sh[(q * IY + r + k) * TX + tx];
        m[q] = a * (q < 2 ? i1 : i2);
      }
      const double sxx = m[2] - m[0] * m[0], syy = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
      const double cs = (2.0 * sxy + C2) / (sxx + syy + C2);
      const double ss = ((2.0 * m[0] * m[1] + C1) / (m[0] * m[0] + m[1] * m[1] + C1)) * cs;
      scs += cs; sss += ss;
    }
  }
  scs = wave_sum_d(scs); sss = wave_sum_d(sss);
  if ((tid & 63) == 0) { red[tid >> 6][0] = scs; red[tid >> 6][1] = sss; }
  __syncthreads();
  if (tid < 2) {                                           // the four waves in a fixed order
    const long tile = (long)blockIdx.y * gridDim.x + blockIdx.x, ntile = (long)gridDim.x * gridDim.y;
    part[((long)b * ntile + tile) * 2 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  }
}

struct Fin {
  long part_off[MAXM];      // doubles, from the workspace's start
  int ntile[MAXM];
  double npix[MAXM], weight[MAXM];
};

// one wave per image: per scale, lane l adds tiles l, l + 64, .. in order, then the lanes are added in wave_sum_d's fixed tree;
// out[b] = {prod_j max(v_j, 0)^w_j, v_1 .. v_M}
__global__ void __launch_bounds__(64) k_msssim_fin(const double* __restrict__ ws, double* __restrict__ out, int M, Fin f) {
  const int b = blockIdx.x;
  double prod = 1.0;
  for (int j = 0; j < M; ++j) {
    const double* p = ws + f.part_off[j] + (long)b * f.ntile[j] * 2 + (j + 1 == M ? 1 : 0);   // cs below the last scale, ss there
    double s = 0;
    for (int t = threadIdx.x; t < f.ntile[j]; t += 64) s += p[2L * t];
    s = wave_sum_d(s);
    const double v = s / f.npix[j];
    if (threadIdx.x == 0) out[(long)b * (M + 1) + 1 + j] = v;
    prod *= v > 0.0 ? pow(v, f.weight[j]) : 0.0;          // 0^w = 0; a NaN gives 0 too, and shows in v_j
  }
  if (threadIdx.x == 0) out[(long)b * (M + 1)] = prod;
}

// the plan of a call, shared by _ws and the entry point: extents, tiles and workspace offsets (in doubles) of every scale
struct Plan {
  int h[MAXM], w[MAXM], gx[MAXM], gy[MAXM];
  long part_off[MAXM], pyr_off[MAXM];     // pyr_off[0] unused: scale 1 is the input
  long total;
};
bool make_plan(int B, int H, int W, int border, int M, Plan& p) {
  if (B <= 0 || border < 0 || M < 1 || M > MAXM) return false;
  const long need = 10L * (1 << (M - 1)) + 1;
  long h = (long)H - 2L * border, w = (long)W - 2L * border;
  if (h < need || w < need) return false;
  long off = 0;
  for (int j = 0; j < M; ++j) {
    p.h[j] = (int)h; p.w[j] = (int)w;
    p.gx[j] = sr_cdiv(w - (WS - 1), TX); p.gy[j] = sr_cdiv(h - (WS - 1), TY);
    p.part_off[j] = off; off += 2L * B * p.gx[j] * p.gy[j];
    h = pooled((int)h); w = pooled((int)w);
  }
  for (int j = 1; j < M; ++j) {                            // uint32 pairs, counted in doubles
    p.pyr_off[j] = off; off += ((long)B * 2 * p.h[j] * p.w[j] + 1) / 2;
  }
  p.pyr_off[0] = 0;
  p.total = off;
  return true;
}

}  // namespace

extern "C" {

long srhip_metrics_msssim_lv_ws(int B, int H, int W, int border, int M) {
  Plan p;
  return make_plan(B, H, W, border, M, p) ? p.total : 0;
}

int srhip_metrics_msssim_lv(const float* E, const float* Hh, int B, int H, int W, int border, int L, int inputs_are_levels,
                            int M, const double* weights_host, double* workspace, long workspace_doubles, double* out,
                            void* stream) {
  SR_REQUIRE(M >= 1 && M <= MAXM, "metrics_msssim_lv: the number of scales is 1 .. %d (got %d)", MAXM, M);
  SR_REQUIRE(L >= 255 && L <= 65535, "metrics_msssim_lv: the white level is 255 .. 65535 (got %d)", L);
  SR_REQUIRE(B > 0 && border >= 0 && H > 0 && W > 0, "metrics_msssim_lv: empty input");
  Plan p;
  SR_REQUIRE(make_plan(B, H, W, border, M, p),
             "metrics_msssim_lv: %d scales need both sides of the cropped image to be at least %d (got %d x %d after a border of %d)",
             M, 10 * (1 << (M - 1)) + 1, H - 2 * border, W - 2 * border, border);
  SR_REQUIRE(E && Hh && workspace && out, "metrics_msssim_lv: null pointer");
  SR_REQUIRE(workspace_doubles >= p.total && ((uintptr_t)workspace & 7) == 0,
             "metrics_msssim_lv: the workspace holds %ld doubles, the call needs %ld (srhip_metrics_msssim_lv_ws), 8-byte aligned",
             workspace_doubles, p.total);
  SR_REQUIRE(p.gy[0] <= 65535 && B <= 65535, "metrics_msssim_lv: more than 65535 tile rows or images");
  static const double published[MAXM] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  Fin f;
  double wsum = 0;
  for (int j = 0; j < M; ++j) wsum += published[j];
  for (int j = 0; j < M; ++j) {
    f.weight[j] = weights_host ? weights_host[j] : (M == MAXM ? published[j] : published[j] / wsum);
    SR_REQUIRE(f.weight[j] > 0.0 && f.weight[j] <= 1.0, "metrics_msssim_lv: weight %d is outside (0, 1]", j);
    f.part_off[j] = p.part_off[j];
    f.ntile[j] = p.gx[j] * p.gy[j];
    f.npix[j] = (double)(p.h[j] - (WS - 1)) * (p.w[j] - (WS - 1));
  }
  hipStream_t st = (hipStream_t)stream;
  const Taps tp = gaussian_taps(WS, true);        // the window of srhip_metrics_ssim_lv
  double div = (double)L;
  for (int j = 0; j < M; ++j, div *= 4.0) {
    const dim3 grid(p.gx[j], p.gy[j], B);
    unsigned* next = j + 1 < M ? (unsigned*)(workspace + p.pyr_off[j + 1]) : nullptr;
    if (j == 0)
      hipLaunchKernelGGL(k_msssim_scale<true>, grid, dim3(256), 0, st, E, Hh, (const unsigned*)nullptr, next,
                         workspace + p.part_off[j], H, W, border, p.h[j], p.w[j], L, inputs_are_levels, 1.0 / div, tp);
    else
      hipLaunchKernelGGL(k_msssim_scale<false>, grid, dim3(256), 0, st, (const float*)nullptr, (const float*)nullptr,
                         (const unsigned*)(workspace + p.pyr_off[j]), next, workspace + p.part_off[j], H, W, border, p.h[j],
                         p.w[j], L, 1, 1.0 / div, tp);
  }
  hipLaunchKernelGGL(k_msssim_fin, dim3(B), dim3(64), 0, st, workspace, out, M, f);
  SR_LAUNCH_CHECK("metrics_msssim_lv");
  return 0;
}

}  // extern "C"

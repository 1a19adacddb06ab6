// Fourier ring correlation of prediction against target at L levels, float64 (--frc).  Not a reference call: the definition is the
// one of include/srhip.h (srhip_metrics_frc_lv).
//
// Three launches.  E and H are real, so a pair costs ONE complex transform: z = win x_E + i win x_H, and with A = Z(k),
// B = conj Z(-k) the two spectra are F1 = (A + B) / 2, F2 = (A - B) / (2i).
//   k_frc_rows   a block quantises, windows and packs 4 image rows into LDS, transforms them and writes them TRANSPOSED into the
//                workspace, T[b][p][y]: 4 rows x 16 B are the 64-byte runs of the store, and a column of the spectrum is one
//                contiguous run of S elements for the next pass.
//   k_frc_cols   block kx (0 .. S/2) loads column kx and, where it is another one, column S - kx, transforms both and takes the
//                ring sums of column kx: one thread per ring walks that ring's ky in ascending order.  Column -kx holds the
//                conjugates (F(-k) = conj F(k) for a real image), the same three real terms on the same rings, so its share is
//                the factor 2.  part[b][q][kx][r], r >= kx.
//   k_frc_fin    one block per image: thread r adds part[.][.][0 .. r][r] in ascending kx, forms the curve, and the block finds
//                the first ring under the threshold by a min over lanes and waves.
// Nothing is accumulated with atomics, in LDS or in memory: two calls give the same bits.
//
// The transform, its LDS layout and budget, the side rule, the window and the ring bounds are those of fft_lds.h, shared with
// decorr.hip.
#include "common.h"
#include "levels.h"
#include "fft_lds.h"

namespace {

// grid (S / ROWS, B).  T[b][p][y] = the row transform of row y at position p (frequency bitrev(p)).
__global__ void __launch_bounds__(1024) k_frc_rows(const float* __restrict__ E, const float* __restrict__ Hh,
                                                   double2* __restrict__ T, int H, int W, int lg, int L, int in_is_lv) {
  extern __shared__ double2 frc_sm[];
  const int S = 1 << lg, rs = S + RPAD;
  double2* const tw = frc_sm;                 // [S / 2]
  double2* const x = frc_sm + (S >> 1);       // [ROWS][rs]
  const int b = blockIdx.y, y0 = blockIdx.x * ROWS;
  const int oy = (H - S) / 2, ox = (W - S) / 2;
  const float fL = (float)L;
  const double dL = (double)L;
  make_twiddles(tw, lg);
  __syncthreads();
  for (int i = threadIdx.x; i < ROWS * S; i += blockDim.x) {
    const int r = i >> lg, c = i & (S - 1);
    const long o = ((long)b * H + oy + y0 + r) * W + ox + c;
    const double win = hann(tw, y0 + r, lg) * hann(tw, c, lg);
    x[r * rs + c] = make_double2(win * ((double)metric_level(E[o], in_is_lv, fL) / dL),
                                 win * ((double)metric_level(Hh[o], in_is_lv, fL) / dL));
  }
  __syncthreads();
  fft_rows(x, tw, ROWS, rs, lg);
  for (int i = threadIdx.x; i < ROWS * S; i += blockDim.x) {
    const int r = i & (ROWS - 1), p = i >> 2;
    T[((long)b * S + p) * S + y0 + r] = x[r * rs + p];
  }
}

// grid (S / 2 + 1, B).  part[b][q][kx][r], q = 0: sum Re(F1 conj F2), 1: sum |F1|^2, 2: sum |F2|^2 over ring r of columns +-kx
__global__ void __launch_bounds__(1024) k_frc_cols(const double2* __restrict__ T, double* __restrict__ part, int lg) {
  extern __shared__ double2 frc_sm[];
  const int S = 1 << lg, rs = S + RPAD, nr = (S >> 1) + 1;
  double2* const tw = frc_sm;
  double2* const x = frc_sm + (S >> 1);       // [2][rs]: column kx, column S - kx
  const int b = blockIdx.y, kx = blockIdx.x;
  const int kxm = (S - kx) & (S - 1);
  const bool pair = kxm != kx;                // kx = 0 and kx = S / 2 are their own mirrors
  make_twiddles(tw, lg);
  const double2* const c0 = T + ((long)b * S + bitrev(kx, lg)) * S;
  const double2* const c1 = T + ((long)b * S + bitrev(kxm, lg)) * S;
  for (int i = threadIdx.x; i < S; i += blockDim.x) {
    x[i] = c0[i];
    if (pair) x[rs + i] = c1[i];
  }
  __syncthreads();
  fft_rows(x, tw, pair ? 2 : 1, rs, lg);
  const double2* const xm = pair ? x + rs : x;
  const double mult = pair ? 2.0 : 1.0;
  for (int r = kx + threadIdx.x; r < nr; r += blockDim.x) {
    // ring r of this column: (2r - 1)^2 <= 4 (kx^2 + ky^2) < (2r + 1)^2, that is a <= |ky| < e, ky in [-S/2, S/2)
    const int a = r == 0 ? 0 : half_root_up((2 * r - 1) * (2 * r - 1) - 4 * kx * kx);
    const int e = half_root_up((2 * r + 1) * (2 * r + 1) - 4 * kx * kx);
    double sc = 0, s1 = 0, s2 = 0;
    auto term = [&](int ky) {
      const double2 A = x[bitrev(ky & (S - 1), lg)], B = xm[bitrev(-ky & (S - 1), lg)];    // Z(k), Z(-k)
      const double f1x = 0.5 * (A.x + B.x), f1y = 0.5 * (A.y - B.y);
      const double f2x = 0.5 * (A.y + B.y), f2y = -0.5 * (A.x - B.x);
      sc += f1x * f2x + f1y * f2y;
      s1 += f1x * f1x + f1y * f1y;
      s2 += f2x * f2x + f2y * f2y;
    };
    const int top = e - 1 < (S >> 1) ? e - 1 : (S >> 1);
    for (int ky = -top; ky <= -(a > 1 ? a : 1); ++ky) term(ky);
    for (int ky = a; ky <= (top < (S >> 1) ? top : (S >> 1) - 1); ++ky) term(ky);
    const long o = (((long)b * 3) * nr + kx) * nr + r;
    part[o] = mult * sc;
    part[o + (long)nr * nr] = mult * s1;
    part[o + 2L * nr * nr] = mult * s2;
  }
}

// grid B.  curve[b][r] = C_r / sqrt(P1_r P2_r) (0 where the product is not positive); cut[b] as the header states it
__global__ void __launch_bounds__(256) k_frc_fin(const double* __restrict__ part, double* __restrict__ curve,
                                                 double* __restrict__ cut, int lg, double thr) {
  __shared__ double sc[(MAXS >> 1) + 1];
  __shared__ int first_w[4];
  const int S = 1 << lg, nr = (S >> 1) + 1, b = blockIdx.x;
  const long plane = (long)nr * nr;
  const double* const p = part + (long)b * 3 * plane;
  for (int r = threadIdx.x; r < nr; r += 256) {
    double c = 0, p1 = 0, p2 = 0;
    for (int kx = 0; kx <= r; ++kx) {
      const long o = (long)kx * nr + r;
      c += p[o]; p1 += p[o + plane]; p2 += p[o + 2 * plane];
    }
    const double den = p1 * p2;
    const double f = den > 0.0 ? c / sqrt(den) : 0.0;
    curve[(long)b * nr + r] = f;
    sc[r] = f;
  }
  __syncthreads();
  int first = nr;                             // the first ring from 1 on under the threshold
  for (int r = threadIdx.x; r < nr; r += 256)
    if (r >= 1 && sc[r] < thr) { first = r; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(first, o, 64); first = v < first ? v : first; }
  if ((threadIdx.x & 63) == 0) first_w[threadIdx.x >> 6] = first;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) first = first_w[w] < first ? first_w[w] : first;
    double xr = (double)(S >> 1);
    if (first < nr) {
      const double q = sc[first - 1];
      xr = q < thr ? 0.0 : (double)(first - 1) + (q - thr) / (q - sc[first]);
    }
    cut[b] = xr / (double)(S >> 1);
  }
}

long ws_doubles(int B, int S) {
  const long nr = (S >> 1) + 1;
  return 2L * B * S * S + 3L * B * nr * nr;
}

}  // namespace

extern "C" {

long srhip_metrics_frc_lv_ws(int B, int H, int W) {
  const int lg = side_log2(H, W);
  return B > 0 && lg ? ws_doubles(B, 1 << lg) : 0;
}

int srhip_metrics_frc_lv(const float* E, const float* Hh, int B, int H, int W, int L, int inputs_are_levels, double threshold,
                         double* workspace, long workspace_doubles, double* curve, double* cut, void* stream) {
  SR_REQUIRE(L >= 255 && L <= 65535, "metrics_frc_lv: the white level is 255 .. 65535 (got %d)", L);
  SR_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "metrics_frc_lv: empty input or more than 65535 images");
  SR_REQUIRE(threshold > 0.0 && threshold < 1.0, "metrics_frc_lv: the threshold lies in (0, 1) (got %g)", threshold);
  const int lg = side_log2(H, W);
  SR_REQUIRE(lg, "metrics_frc_lv: both sides must be at least %d (got %d x %d)", MINS, H, W);
  const int S = 1 << lg;
  SR_REQUIRE(E && Hh && workspace && curve && cut, "metrics_frc_lv: null pointer");
  const long need = ws_doubles(B, S);
  SR_REQUIRE(workspace_doubles >= need && ((uintptr_t)workspace & 15) == 0,
             "metrics_frc_lv: the workspace holds %ld doubles, the call needs %ld (srhip_metrics_frc_lv_ws), 16-byte aligned",
             workspace_doubles, need);
  const size_t lr = rows_lds(S), lc = cols_lds(S);
  // above the 64 KiB default the attribute is set at every call: it belongs to the current device, so a value remembered per
  // process would be wrong on a second device (and a race between host threads); it is one host call, no synchronisation
  constexpr size_t LDS_DEFAULT = 64 * 1024;
  if (lr > LDS_DEFAULT &&
      hipFuncSetAttribute((const void*)k_frc_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lr) != hipSuccess)
    return sr_fail(-5, "metrics_frc_lv: cannot reserve %zu bytes of LDS", lr);
  if (lc > LDS_DEFAULT &&
      hipFuncSetAttribute((const void*)k_frc_cols, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lc) != hipSuccess)
    return sr_fail(-5, "metrics_frc_lv: cannot reserve %zu bytes of LDS", lc);
  hipStream_t st = (hipStream_t)stream;
  double2* const T = (double2*)workspace;
  double* const part = workspace + 2L * B * S * S;
  const int nt_r = ROWS * S / 2 < 1024 ? ROWS * S / 2 : 1024;      // a butterfly per thread and stage, 64 .. 1024
  const int nt_c = S < 64 ? 64 : (S < 1024 ? S : 1024);
  hipLaunchKernelGGL(k_frc_rows, dim3(S / ROWS, B), dim3(nt_r), lr, st, E, Hh, T, H, W, lg, L, inputs_are_levels);
  hipLaunchKernelGGL(k_frc_cols, dim3(S / 2 + 1, B), dim3(nt_c), lc, st, (const double2*)T, part, lg);
  hipLaunchKernelGGL(k_frc_fin, dim3(B), dim3(256), 0, st, (const double*)part, curve, cut, lg, threshold);
  SR_LAUNCH_CHECK("metrics_frc_lv");
  return 0;
}

}  // extern "C"

// The float64 radix-2 transform in LDS that the spectral metrics share (frc.hip: --frc; decorr.hip: predict.py --resolution),
// with the side rule, the periodic Hann window and the integer ring rule of include/srhip.h (srhip_metrics_frc_lv).
//
// The transform is radix-2, in place, natural order in and bit-reversed order out, in the form whose twiddle depends on the
// GROUP of a butterfly and not on the position in it: a sub-transform of length n that computes Y[k] = sum x[j] e^(-2 pi i j
// (k + t) / n) splits into the two of length n / 2 over x[j] + w x[j + n/2] (offset t / 2, the even k) and x[j] - w x[j + n/2]
// (offset (t + 1) / 2, the odd k) with w = e^(-pi i t).  Group g of any stage has t = 0.g_0 g_1 g_2 .. in binary, so ONE table
// tw[g] = e^(-pi i t(g)) of S / 2 entries serves every stage, a wave reads it at consecutive or equal addresses (the table in
// natural order would be read at power-of-two strides, all on one bank), and t is exact: sincospi of the reduced index, as in
// dfca.hip.  Neither pass of a 2-D transform undoes the bit reversal: the row pass stores position p as row p of T, the column
// pass loads row bitrev(kx), and the ring walk reads position bitrev(ky).
//
// LDS: 16-byte elements.  ds_read_b128 serves 16 lanes at a time over a 256-byte bank row; the butterflies read runs of
// consecutive elements, which is conflict-free, but the transposed store of the row pass reads the same p of the 4 rows in one lane
// group, S * 16 bytes apart: rows are therefore RPAD = 4 elements further apart, which puts the 4 x 4 elements of a lane group on
// 16 different slots.  At S = 2048 the row pass holds 4 x 2052 + 1024 elements, 144.3 KiB of the CU's 160, the column pass 80.1 KiB
// (two blocks a CU would need 160.2); both are dynamic LDS above the 64 KiB default.
#pragma once
#include "common.h"

namespace {

constexpr int ROWS = 4, RPAD = 4;
constexpr int MINS = 32, MAXS = 2048;

// log2 of the side S: the largest power of two not above min(H, W), at most MAXS; 0: below MINS
int side_log2(int H, int W) {
  const int m = H < W ? H : W;
  if (m < MINS) return 0;
  int lg = 5;
  while (lg < 11 && (2 << lg) <= m) ++lg;
  return lg;
}

__device__ __forceinline__ int bitrev(int v, int bits) { return bits ? (int)(__brev((unsigned)v) >> (32 - bits)) : 0; }

// tw[g] = e^(-pi i t), t = bitrev(g) / (S / 2) in [0, 1)
__device__ __forceinline__ void make_twiddles(double2* tw, int lg) {
  const int half = 1 << (lg - 1);
  for (int g = threadIdx.x; g < half; g += blockDim.x) {
    double s, c;
    sincospi((double)bitrev(g, lg - 1) / (double)half, &s, &c);
    tw[g] = make_double2(c, -s);
  }
}

// periodic Hann, 0.5 - 0.5 cos(2 pi i / S): the cosine is the twiddle of t = 2 i / S, negated in the upper half
__device__ __forceinline__ double hann(const double2* tw, int i, int lg) {
  const int half = 1 << (lg - 1);
  const double c = tw[bitrev(i & (half - 1), lg - 1)].x;
  return 0.5 - 0.5 * ((i & half) ? -c : c);
}

// nrow transforms of length S = 2^lg, rows rs elements apart, in place; position p of a row ends as frequency bitrev(p)
__device__ __forceinline__ void fft_rows(double2* x, const double2* tw, int nrow, int rs, int lg) {
  const int half = 1 << (lg - 1);
  for (int s = 0; s < lg; ++s) {
    const int lh = lg - 1 - s, h = 1 << lh;
    for (int j = threadIdx.x; j < nrow * half; j += blockDim.x) {
      const int row = j >> (lg - 1), jj = j & (half - 1);
      const int g = jj >> lh, pos = jj & (h - 1);
      double2* p = x + row * rs + (g << (lh + 1)) + pos;
      const double2 w = tw[g], a = p[0], b = p[h];
      const double vx = w.x * b.x - w.y * b.y, vy = w.x * b.y + w.y * b.x;
      p[0] = make_double2(a.x + vx, a.y + vy);
      p[h] = make_double2(a.x - vx, a.y - vy);
    }
    __syncthreads();
  }
}

// the smallest n >= 0 with 4 n^2 >= v
__device__ __forceinline__ int half_root_up(int v) {
  if (v <= 0) return 0;
  int n = (int)ceil(0.5 * sqrt((double)v));
  while (n > 0 && 4 * (n - 1) * (n - 1) >= v) --n;
  while (4 * n * n < v) ++n;
  return n;
}

size_t rows_lds(int S) { return ((size_t)(S >> 1) + (size_t)ROWS * (S + RPAD)) * sizeof(double2); }
size_t cols_lds(int S) { return ((size_t)(S >> 1) + 2 * (size_t)(S + RPAD)) * sizeof(double2); }
static_assert(((MAXS >> 1) + ROWS * (MAXS + RPAD)) * 16 <= 160 * 1024, "row pass: LDS at the largest side");
static_assert(((MAXS >> 1) + 2 * (MAXS + RPAD)) * 16 <= 160 * 1024, "column pass: LDS at the largest side");

}  // namespace
